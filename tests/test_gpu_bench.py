"""bench.py's GPU runner against the CPU oracle (test infrastructure: the
oracle is the checker).  Every slot-addressing mode the bench can time --
range, grouped, declared and scattered ids (scattered with a ragged last
group) -- must crypt exactly the sessions a plain range crypt of
the same batches would, so the bench never times a path that differs from
the parity-tested one."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "oracle"))
sys.path.insert(0, str(ROOT / "tests"))


@pytest.mark.gpu
@pytest.mark.parametrize("ids,S", [("range", 300), ("scattered", 300), ("scattered", 512),
                                   ("grouped", 512), ("declared", 512)])
def test_bench_runner_matches_oracle(built, ids, S):
    import torch
    import bench
    from oracle_runner import OracleRunner
    L, R, steps = 64, 2, 3
    run = bench.GpuRunner(torch, 0, S, L, R, 0, ids)
    ref = OracleRunner(S, L, R, 0)
    try:
        for i in range(steps):
            run.step(i)
            ref.step(i)
        run.check()
        got = run.payload.cpu().numpy()
        want = ref.w.payload
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (f"{ids}: {bad.size} bytes differ, first at {bad[:8].tolist()} "
                               f"(sessions {sorted(set((bad[:64] // L).tolist()))[:8]})")
    finally:
        run.close()


@pytest.mark.gpu
def test_dump_outputs_is_the_last_timed_steps_batch(built, tmp_path, monkeypatch):
    """--dump-outputs: after W warmup and K timed steps over R rotating batches
    the file holds batch (W + K - 1) % R exactly as the oracle leaves it
    (300 sessions: a ragged last group), as float32 [S][L]; K really is the
    number of timed steps and the line carries ms_per_step."""
    import bench
    from oracle_runner import OracleRunner
    S, L, W, K = 300, 64, 1, 3
    monkeypatch.setitem(bench.CONFIG_SHAPES, "tiny300", (S, L))
    monkeypatch.setitem(bench.CONFIG_TEXT, "tiny300", "300 sessions x 64 B (test shape)")
    args = bench.parse(["--steps", str(K), "--warmup", str(W), "--footprint-mib", "1",
                        "--dump-outputs", str(tmp_path / "out")])
    args.workload = "tiny300"
    res, run = bench.run_bench(args, 1, 0, 0)
    try:
        R = run.R
        assert R > W + K                       # every step its own batch: the last one is batch W + K - 1
        ref = OracleRunner(S, L, R, 0)
        for i in range(W + K):
            ref.step(i)
        got = np.load(tmp_path / "out" / "payload.npy")
        assert got.dtype == np.float32 and got.shape == (S, L)
        assert np.array_equal(got, ref.last_output(W + K - 1).astype(np.float32))
        assert np.array_equal(run.payload.cpu().numpy(), ref.w.payload)      # K timed steps, no more
        assert res["steps"] == K and res["ms_per_step"] > 0
        assert res["cpu_baseline"] is None and "configs4_strong" not in res
    finally:
        run.close()
