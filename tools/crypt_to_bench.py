#!/usr/bin/env python3
"""Per-call cost of an out-of-place grouped crypt, two ways, in one process:

  (a) what a caller does without the call: a dense torch copy_ of the sources
      into the destinations (for a broadcast: of the one message expanded to
      every destination), then the in-place zrc4_crypt_grouped_declared over
      the destinations; both inside the timed window;
  (b) zrc4_crypt_to_grouped (groups declared): one call.

  python tools/crypt_to_bench.py [--out profiles/crypt_to/crypt_to_bench.jsonl]
                                 [--reps 10] [--rounds 3] [--shapes 4x16384,...]
                                 [--src-shift BYTES] [--parent-rev REV]

Shapes (entries x bytes, every entry its own slot, whole groups): 4 x 16 KiB,
4 096 x 16 KiB, 16 384 x 16 KiB, 65 536 x 4 KiB (the native out-of-place
kernels, at most 256 buckets), and 131 072 x 1 KiB (512 buckets: the span copy
and the persistent kernel, two launches).  Each shape runs with distinct
sources (entry i reads its own span) and as a broadcast (every entry reads the
same span), the sources in device memory, the destinations in device memory
and in pinned host memory.  All spans are 16-byte aligned unless --src-shift
moves every source span by that many bytes: with a shift that is no multiple
of 16 every entry of (b) is non-congruent (unaligned 16-byte loads on the
lane-per-stream kernels, the byte path on the window kernel).

--parent-rev REV adds (c): the same call through the library built from git
revision REV (zsummerx_amd.build.build_variant("parent", {}, rev=REV); built
beforehand where there is no history), alternated with the others, so that a
kernel change is measured against its parent in one process.

Per round the variants are warmed up and timed alternately, rep by rep,
with HIP events around the variant's calls.  Each round reports a median per
variant; the spread (max - min) of a variant's round medians is the yardstick
for a difference between the two.
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

SHAPES = "4x16384,4096x16384,16384x16384,65536x4096,131072x1024"


def dev(torch, a):
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view else a).cuda()


def one_round(torch, fns: dict, reps: int) -> dict:
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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "crypt_to" / "crypt_to_bench.jsonl"))
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--src-shift", type=int, default=0, help="bytes added to every source offset")
    ap.add_argument("--parent-rev", default="", help="also time crypt_to through the library of this git revision")
    args = ap.parse_args()
    import torch
    from zsummerx_amd import Context, build
    parent = build.build_variant("parent", {}, rev=args.parent_rev) if args.parent_rev else None
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    s = torch.cuda.current_stream()
    with out.open("w") as fh:
        for shape in args.shapes.split(","):
            n, size = (int(v) for v in shape.split("x"))
            m = (n + 255) // 256 * 256                   # entries the launch sees: whole buckets
            cap = max(256, m)
            ids = np.full(m, 0xFFFFFFFF, dtype=np.uint32)
            ids[:n] = np.arange(n, dtype=np.uint32)
            busy = ids != 0xFFFFFFFF
            length = np.where(busy, size, 0).astype(np.uint32)
            off = (np.arange(m, dtype=np.uint64) * size) * busy
            groups = np.arange(m // 256, dtype=np.uint32)
            d_ids, d_len, d_off = dev(torch, ids), dev(torch, length), dev(torch, off)
            shift = np.uint64(args.src_shift)
            d_zero = dev(torch, np.zeros(m, dtype=np.uint64) + shift * busy)
            d_shifted = dev(torch, off + shift * busy)
            total = n * size
            for sources in ("distinct", "broadcast"):
                src = torch.randint(0, 256, ((total if sources == "distinct" else size) + args.src_shift,),
                                    dtype=torch.uint8, device="cuda")
                d_soff = d_shifted if sources == "distinct" else d_zero
                for where in ("device", "pinned_host"):
                    dst = (torch.empty(total, dtype=torch.uint8, device="cuda") if where == "device"
                           else torch.empty(total, dtype=torch.uint8).pin_memory())
                    body = src[args.src_shift:]
                    dense = body if sources == "distinct" else body.expand(n, size)
                    dview = dst if sources == "distinct" else dst.view(n, size)
                    with Context(0, cap) as ca, Context(0, cap) as cb, Context(0, cap, lib=parent) as cp:
                        def copy_then_in_place():
                            dview.copy_(dense, non_blocking=True)
                            ca.crypt_grouped_declared(dst, d_off, d_len, d_ids, groups, n=m, stream=s)

                        def crypt_to():
                            cb.crypt_to_grouped(src, d_soff, dst, d_off, d_len, d_ids, groups, n=m, stream=s)

                        def crypt_to_parent():
                            cp.crypt_to_grouped(src, d_soff, dst, d_off, d_len, d_ids, groups, n=m, stream=s)

                        fns = {"copy_then_in_place": copy_then_in_place, "crypt_to": crypt_to}
                        if parent:
                            fns["crypt_to_parent"] = crypt_to_parent
                        rounds = [one_round(torch, fns, args.reps) for _ in range(args.rounds)]
                        ca.sync(s)
                        cb.sync(s)
                        cp.sync(s)
                    med = {k: [round(r[k], 2) for r in rounds] for k in fns}
                    a, b = statistics.median(med["copy_then_in_place"]), statistics.median(med["crypt_to"])
                    rec = {"entries": n, "bytes_per_entry": size, "buckets": m // 256, "sources": sources,
                           "src_shift": args.src_shift,
                           "dst": where, "path": "native" if m // 256 <= 256 else "copy+persistent",
                           "reps": args.reps,
                           "copy_then_in_place_round_medians_us": med["copy_then_in_place"],
                           "crypt_to_round_medians_us": med["crypt_to"],
                           "copy_then_in_place_us": round(a, 2), "crypt_to_us": round(b, 2),
                           "copy_then_in_place_spread_us": round(max(med["copy_then_in_place"]) -
                                                                 min(med["copy_then_in_place"]), 2),
                           "crypt_to_spread_us": round(max(med["crypt_to"]) - min(med["crypt_to"]), 2),
                           "crypt_to_over_copy_then_in_place": round(b / a, 3)}
                    if parent:
                        pm = med["crypt_to_parent"]
                        rec.update({"parent_rev": args.parent_rev, "crypt_to_parent_round_medians_us": pm,
                                    "crypt_to_parent_us": round(statistics.median(pm), 2),
                                    "crypt_to_parent_spread_us": round(max(pm) - min(pm), 2),
                                    "crypt_to_over_parent": round(b / statistics.median(pm), 3)})
                    line = json.dumps(rec)
                    print(line, flush=True)
                    fh.write(line + "\n")
                    fh.flush()
                    del dst, dview
                del src, dense, body
                torch.cuda.synchronize()


if __name__ == "__main__":
    main()
