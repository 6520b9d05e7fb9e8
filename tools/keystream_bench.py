#!/usr/bin/env python3
"""Per-launch cost of a refill-shaped grouped launch, two ways, in one process:

  (a) zrc4_crypt_grouped_declared over ZEROED spans on the library given with
      --lib (the parent revision: `python -c "from zsummerx_amd.build import
      build_variant; build_variant('parent', {}, rev='<rev>')"` builds
      zsummerx_amd/libzrc4_parent.so); how the reservoirs refilled before;
  (b) zrc4_keystream_grouped on the product library (--new): write-only.

  python tools/keystream_bench.py --lib zsummerx_amd/libzrc4_parent.so
                                  [--out profiles/keystream/keystream_bench.jsonl]
                                  [--reps 10] [--rounds 3] [--shapes 4x16384,...]

Shapes (entries x bytes, every entry its own slot, whole groups, the groups
declared), each with `out` in device memory and in coherent pinned host
memory (where the session engine's rings live): 4 x 16 KiB, 4 096 x 16 KiB,
16 384 x 16 KiB, 65 536 x 4 KiB (the native write-only kernels, at most 256
buckets), and 131 072 x 1 KiB (512 buckets: the persistent kernel behind the
span fill, two launches).

Per round the two variants are warmed up and timed alternately, rep by rep,
with HIP events around the launch alone; (a)'s spans are zeroed before each
of its launches, outside the timed window (the parent's callers zeroed on the
host).  Each round reports a median per variant; the spread of a variant's
round medians is the yardstick for a difference between the two.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

SHAPES = "4x16384,4096x16384,16384x16384,65536x4096,131072x1024"
HOST_COHERENT = 0x40000000        # hipHostMallocCoherent


def hip_runtime():
    """The HIP runtime this process already uses (torch's)."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    return C.CDLL("libamdhip64.so")


def dev(torch, a):
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view else a).cuda()


def one_round(torch, fns: dict, prep: dict, reps: int) -> dict:
    for k, f in fns.items():
        for _ in range(2):
            prep[k]()
            f()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            prep[k]()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) * 1e3)
    return {k: statistics.median(v) for k, v in out.items()}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", required=True, help="baseline library (the parent revision's build)")
    ap.add_argument("--new", default=None, help="library with zrc4_keystream_grouped (default: the product)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "keystream" / "keystream_bench.jsonl"))
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch
    from zsummerx_amd import Context
    hip = hip_runtime()
    hip.hipHostMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
    hip.hipHostFree.argtypes = [C.c_void_p]
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    s = torch.cuda.current_stream()
    with out.open("w") as fh:
        for shape in args.shapes.split(","):
            n, size = (int(v) for v in shape.split("x"))
            cap = max(256, (n + 255) // 256 * 256)
            m = (n + 255) // 256 * 256                   # entries the launch sees: whole buckets
            ids = np.full(m, 0xFFFFFFFF, dtype=np.uint32)
            ids[:n] = np.arange(n, dtype=np.uint32)
            length = np.where(ids != 0xFFFFFFFF, size, 0).astype(np.uint32)
            off = (np.arange(m, dtype=np.uint64) * size) * (ids != 0xFFFFFFFF)
            groups = np.arange(m // 256, dtype=np.uint32)
            d_ids, d_len, d_off = dev(torch, ids), dev(torch, length), dev(torch, off)
            total = n * size
            for where in ("device", "pinned_host"):
                host = C.c_void_p()
                if where == "device":
                    buf = torch.empty(total, dtype=torch.uint8, device="cuda")
                    ptr = buf.data_ptr()
                    zero = buf.zero_
                else:
                    if hip.hipHostMalloc(C.byref(host), total, HOST_COHERENT) != 0:
                        raise MemoryError("hipHostMalloc")
                    ptr = host.value
                    zero = lambda: C.memset(ptr, 0, total)
                with Context(0, cap, lib=args.lib) as base, Context(0, cap, lib=args.new) as new:
                    fns = {
                        "crypt_zeroed_parent": lambda: base.crypt_grouped_declared(ptr, d_off, d_len, d_ids, groups,
                                                                                   n=m, stream=s),
                        "keystream": lambda: new.keystream_grouped(ptr, d_off, d_len, d_ids, groups, n=m, stream=s),
                    }
                    prep = {"crypt_zeroed_parent": zero, "keystream": lambda: None}
                    rounds = [one_round(torch, fns, prep, args.reps) for _ in range(args.rounds)]
                    base.sync(s)
                    new.sync(s)
                med = {k: [round(r[k], 2) for r in rounds] for k in fns}
                a, b = statistics.median(med["crypt_zeroed_parent"]), statistics.median(med["keystream"])
                rec = {"entries": n, "bytes_per_entry": size, "buckets": m // 256, "out": where,
                       "path": "native" if m // 256 <= 256 else "fill+persistent", "reps": args.reps,
                       "crypt_zeroed_parent_round_medians_us": med["crypt_zeroed_parent"],
                       "keystream_round_medians_us": med["keystream"],
                       "crypt_zeroed_parent_us": round(a, 2), "keystream_us": round(b, 2),
                       "keystream_over_parent": round(b / a, 3)}
                line = json.dumps(rec)
                print(line, flush=True)
                fh.write(line + "\n")
                fh.flush()
                if host.value:
                    torch.cuda.synchronize()
                    hip.hipHostFree(host)


if __name__ == "__main__":
    main()
