#!/usr/bin/env python3
"""Per-call cost of R broadcasts to the same sessions, two ways, in one process:

  (a) what a caller does without the rounds call: R successive
      zrc4_crypt_to_grouped calls (groups declared), one per message;
  (b) zrc4_crypt_to_grouped_rounds (groups declared): one call.

  python tools/crypt_to_rounds_bench.py [--out profiles/crypt_to_rounds/crypt_to_rounds_bench.jsonl]
                                        [--reps 10] [--repeats 3] [--shapes 4096x128x8,...]

Shapes (entries x bytes per message x rounds, every entry its own slot, whole
groups): 4 096 x 128 B x 8 and 4 096 x 1 KiB x 2 (16 buckets: (a) runs the
window kernel, (b) the half-group kernel), 65 536 x 128 B x 8 and 65 536 x
1 KiB x 2 (256 buckets: the whole-group kernel both ways), 131 072 x 128 B x 4
(512 buckets: (b) is the host loop over (a)'s launches).  Round r's message is
one span of device memory shared by every entry (a broadcast); entry i's
destination span of round r is its own, in device memory and in pinned host
memory.  All spans are 16-byte aligned.

Per repeat the two variants are warmed up and timed alternately, rep by rep,
with HIP events around the variant's calls.  Each repeat reports a median per
variant; the spread (max - min) of (a)'s repeat medians is the yardstick for a
difference between the two.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

SHAPES = "4096x128x8,4096x1024x2,65536x128x8,65536x1024x2,131072x128x4"


def dev(torch, a):
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view else a).cuda()


def one_repeat(torch, fns: dict, reps: int) -> dict:
    for f in fns.values():
        for _ in range(2):
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
    return {k: statistics.median(v) for k, v in out.items()}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "crypt_to_rounds" / "crypt_to_rounds_bench.jsonl"))
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--where", default="device,pinned_host")
    args = ap.parse_args()
    import torch
    from zsummerx_amd import Context
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    s = torch.cuda.current_stream()
    with out.open("w") as fh:
        for shape in args.shapes.split(","):
            n, size, R = (int(v) for v in shape.split("x"))
            assert n % 256 == 0 and size % 16 == 0
            ids = np.arange(n, dtype=np.uint32)
            groups = np.arange(n // 256, dtype=np.uint32)
            length = np.full(R * n, size, dtype=np.uint32)
            doff = np.arange(R * n, dtype=np.uint64) * size               # round-major: round r, entry i
            soff = np.repeat(np.arange(R, dtype=np.uint64) * size, n)      # round r reads message r
            d_ids, d_len, d_doff, d_soff = dev(torch, ids), dev(torch, length), dev(torch, doff), dev(torch, soff)
            src = torch.randint(0, 256, (R * size,), dtype=torch.uint8, device="cuda")
            total = R * n * size
            nb = n // 256
            path = ("host loop over copy+persistent" if nb > cus else
                    "half-group" if 2 * nb <= cus else "whole-group")
            path_a = "copy+persistent" if nb > cus else "window" if nb <= 32 else path
            for where in args.where.split(","):
                dst = (torch.empty(total, dtype=torch.uint8, device="cuda") if where == "device"
                       else torch.empty(total, dtype=torch.uint8).pin_memory())
                with Context(0, n) as ca, Context(0, n) as cb:
                    def successive():
                        for r in range(R):
                            w = slice(r * n, (r + 1) * n)
                            ca.crypt_to_grouped(src, d_soff[w], dst, d_doff[w], d_len[w], d_ids, groups, n=n, stream=s)

                    def rounds():
                        cb.crypt_to_grouped_rounds(src, d_soff, dst, d_doff, d_len, d_ids, n, R, bucket_group=groups,
                                                   stream=s)

                    fns = {"successive": successive, "rounds": rounds}
                    reps = [one_repeat(torch, fns, args.reps) for _ in range(args.repeats)]
                    ca.sync(s)
                    cb.sync(s)
                med = {k: [round(r[k], 2) for r in reps] for k in fns}
                a, b = statistics.median(med["successive"]), statistics.median(med["rounds"])
                rec = {"entries": n, "bytes_per_message": size, "rounds": R, "buckets": nb, "dst": where,
                       "successive_path": path_a, "rounds_path": path, "reps": args.reps,
                       "successive_repeat_medians_us": med["successive"], "rounds_repeat_medians_us": med["rounds"],
                       "successive_us": round(a, 2), "rounds_us": round(b, 2),
                       "successive_spread_us": round(max(med["successive"]) - min(med["successive"]), 2),
                       "rounds_spread_us": round(max(med["rounds"]) - min(med["rounds"]), 2),
                       "rounds_over_successive": round(b / a, 3)}
                line = json.dumps(rec)
                print(line, flush=True)
                fh.write(line + "\n")
                fh.flush()
                del dst
                torch.cuda.synchronize()


if __name__ == "__main__":
    main()
