#!/usr/bin/env python3
"""Timing of the bulk state calls (zrc4_export_states / zrc4_import_states /
zrc4_copy_states) against yardsticks that are not the code under test.

  python tools/states_bench.py [--out profiles/states/states_bench.jsonl]
                               [--slots 65536,524288] [--reps 20] [--threshold]

Per shape (call x slots x addressing: range, ids permuted inside each group,
ids permuted over the whole arena) the variants -- the call and a device-to-
device copy of the same byte count (n * 258 read, n * 258 written) -- are
warmed up and then timed alternately in one process with HIP events; the
median, minimum and maximum of --reps runs go out as one JSON line each.

Old paths (unchanged by the bulk calls, so these are the parent's figures):
get_states of 65 536 slots, and a get_state + set_state loop over 256 slots
(the former zrc4_ks_copy path) against copy_states of 256 slots; wall clock,
the calls block.

--threshold: export by ids of buckets with k busy entries of one group, on
builds that force the image path (ZRC4_STATES_GATHER_MAX=0) and the gather
path (=256): where the two cross is the product's ZRC4_STATES_GATHER_MAX.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def dev(torch, a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def timed(torch, fns: dict, reps: int) -> dict:
    """Alternate the variants rep by rep; HIP-event time of each run in us."""
    for f in fns.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) * 1e3)
    return {k: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
            for k, v in out.items()}


def ids_for(kind: str, n: int, rng):
    if kind == "range":
        return None
    if kind == "ids_in_group":
        return np.concatenate([g * 256 + rng.permutation(256) for g in range(n // 256)]).astype(np.uint32)
    return rng.permutation(n).astype(np.uint32)


def bench_shapes(torch, Context, slots, reps, emit):
    rng = np.random.default_rng(1)
    for n in slots:
        with Context(0, n) as a, Context(0, n) as b:
            sb = torch.empty((n, 256), dtype=torch.uint8, device="cuda")
            xy = torch.empty((n,), dtype=torch.int16, device="cuda")
            a.export_states(sb, xy, first_slot=0, n=n)          # valid records (identity boxes) for the imports
            y_src = torch.empty(n * 258, dtype=torch.uint8, device="cuda")
            y_dst = torch.empty_like(y_src)
            for kind in ("range", "ids_in_group", "ids_arena"):
                ids = ids_for(kind, n, rng)
                d_ids = None if ids is None else dev(torch, ids)
                calls = {
                    "export": lambda: a.export_states(sb, xy, ids=d_ids, first_slot=0, n=n),
                    "import": lambda: a.import_states(sb, xy, ids=d_ids, first_slot=0, n=n),
                    "copy": lambda: b.copy_states(a, dst_ids=d_ids, src_ids=d_ids, n=n),
                }
                for call, fn in calls.items():
                    r = timed(torch, {"call": fn, "d2d_copy": lambda: y_dst.copy_(y_src)}, reps)
                    a.sync()
                    b.sync()
                    emit({"what": call, "slots": n, "addressing": kind, "record_bytes": n * 258, **
                          {f"{k}_{m}": v for k, d in r.items() for m, v in d.items()},
                          "ratio_to_d2d": round(r["call"]["median_us"] / r["d2d_copy"]["median_us"], 2)})


def bench_old_paths(torch, Context, reps, emit):
    n = 65536
    with Context(0, n) as c:
        t = []
        for _ in range(max(3, reps // 4)):
            t0 = time.perf_counter()
            c.get_states(0, n)
            t.append((time.perf_counter() - t0) * 1e6)
        sb = torch.empty((n, 256), dtype=torch.uint8, device="cuda")
        xy = torch.empty((n,), dtype=torch.int16, device="cuda")
        t2 = []
        for _ in range(max(3, reps // 4)):
            t0 = time.perf_counter()
            c.export_states(sb, xy, first_slot=0, n=n)
            c.sync()
            h = (sb.cpu(), xy.cpu())                            # to host memory too, as get_states delivers
            t2.append((time.perf_counter() - t0) * 1e6)
        del h
        emit({"what": "get_states_vs_export", "slots": n, "get_states_median_us": round(statistics.median(t), 1),
              "export_sync_and_d2h_median_us": round(statistics.median(t2), 1)})
        old, new = [], []
        for _ in range(max(3, reps // 4)):
            t0 = time.perf_counter()
            for i in range(256):
                s, x, y = c.get_state(i)
                c.set_state(256 + i, s, x, y)
            old.append((time.perf_counter() - t0) * 1e6)
            t0 = time.perf_counter()
            c.copy_states(c, dst_first=256, src_first=0, n=256)
            c.sync()
            new.append((time.perf_counter() - t0) * 1e6)
        emit({"what": "copy_256_slots", "get_state_set_state_loop_median_us": round(statistics.median(old), 1),
              "copy_states_and_sync_median_us": round(statistics.median(new), 1)})


def bench_threshold(torch, Context, reps, emit):
    from zsummerx_amd import build
    libs = {"image": build.build_variant("stimg", {"ZRC4_STATES_GATHER_MAX": 0}),
            "gather": build.build_variant("stgat", {"ZRC4_STATES_GATHER_MAX": 256})}
    rng = np.random.default_rng(2)
    for buckets in (1, 256):
        n = buckets * 256
        ctxs = {k: Context(0, n, lib=p) for k, p in libs.items()}
        sb = torch.empty((n, 256), dtype=torch.uint8, device="cuda")
        xy = torch.empty((n,), dtype=torch.int16, device="cuda")
        for k in (1, 2, 3, 4, 6, 8, 16, 32, 64, 256):
            ids = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
            for g in range(buckets):
                ids[g * 256 + rng.permutation(256)[:k]] = g * 256 + rng.permutation(256)[:k]
            d_ids = dev(torch, ids)
            r = timed(torch, {name: (lambda c=c: c.export_states(sb, xy, ids=d_ids, n=n)) for name, c in ctxs.items()},
                      reps)
            emit({"what": "export_threshold", "buckets": buckets, "busy_per_bucket": k,
                  **{f"{name}_{m}": v for name, d in r.items() for m, v in d.items()}})
        for c in ctxs.values():
            c.close()


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "states" / "states_bench.jsonl"))
    ap.add_argument("--slots", default="65536,524288")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--threshold", action="store_true", help="also run the gather-threshold sweep (variant builds)")
    ap.add_argument("--only", default="", help="comma list of: shapes, old, threshold")
    args = ap.parse_args()
    import torch
    from zsummerx_amd import Context
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    only = set(filter(None, args.only.split(",")))
    with out.open("w") as fh:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            fh.write(line + "\n")
            fh.flush()
        if not only or "shapes" in only:
            bench_shapes(torch, Context, [int(s) for s in args.slots.split(",")], args.reps, emit)
        if not only or "old" in only:
            bench_old_paths(torch, Context, args.reps, emit)
        if args.threshold or "threshold" in only:
            bench_threshold(torch, Context, args.reps, emit)


if __name__ == "__main__":
    main()
