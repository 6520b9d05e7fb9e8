#!/usr/bin/env python3
"""Compare the gfx950 instruction streams of two builds of libzrc4.so, kernel
by kernel (CPU only: llvm-objdump on the code objects).

    tools/isa_compare.py OLD.so NEW.so

A kernel of OLD is matched to the kernel of NEW with the same demangled name
once template arguments are reduced to their values (`false` = 0, `true` = 1,
casts dropped), so that widening a bool template parameter to an int does not
hide a kernel.  Streams are compared as instruction text without addresses;
branch targets are the disassembler's relative labels.  Prints one line per
kernel of OLD (same / DIFFERENT / missing), then the kernels only NEW has, and
exits 1 if any kernel of OLD is missing or different."""
import re
import subprocess
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
import vmem_hazard_check as vh  # noqa: E402


def _demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return dict(zip(names, out.splitlines()))


def _key(demangled: str) -> str:
    k = re.sub(r"\((?:int|bool|zrc4::\w+)\)", "", demangled)          # value casts
    k = re.sub(r"\bfalse\b", "0", k)
    k = re.sub(r"\btrue\b", "1", k)
    k = re.sub(r"\(.*$", "", k)                                       # the parameter list
    return k.replace(" ", "")


def _streams(lib: Path):
    funcs = vh.parse(vh.disassemble(lib))
    dm = _demangle(list(funcs))
    def text(i):
        if i.target is not None:                    # a label's name carries the asm statement's number
            return f"{i.mnem} {i.target - i.addr:+d}"
        return re.sub(r"\s+", " ", i.text.strip())
    return {_key(dm[n]): [text(i) for i in insns] for n, insns in funcs.items()}


def main(old: str, new: str) -> int:
    a, b = _streams(Path(old)), _streams(Path(new))
    bad = 0
    for k in sorted(a):
        if k not in b:
            print(f"missing    {k}")
            bad += 1
        elif a[k] != b[k]:
            first = next((i for i, (x, y) in enumerate(zip(a[k], b[k])) if x != y), min(len(a[k]), len(b[k])))
            print(f"DIFFERENT  {k}  ({len(a[k])} vs {len(b[k])} instructions, first difference at #{first})")
            bad += 1
        else:
            print(f"same       {k}  ({len(a[k])} instructions)")
    for k in sorted(set(b) - set(a)):
        print(f"new        {k}  ({len(b[k])} instructions)")
    print(f"{len(a)} kernels in {Path(old).name}: {len(a) - bad} identical, {bad} not; "
          f"{len(set(b) - set(a))} only in {Path(new).name}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
