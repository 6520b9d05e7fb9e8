"""The crypt kernel choice (zsummerx_amd/csrc/zrc4_plan.hpp), on the CPU.

tools/bin/plan_check (tests/cpp/plan_check.cpp) compiles the header alone with
g++.  Here:
  a. its hand-written table of shapes and the plans the dispatch must give;
  b. over a sweep of shapes, every plan names a kernel form that exists, and
     the names reached are exactly the crypt-family kernels of the built
     libzrc4.so: none unreachable, none missing;
  c. for in-place range and grouped shapes the plan's family is what
     kernel_class() of tests/dispatch_model.py says.
$ZSX_TOOLS_BIN (scripts/sanitize.sh) points the test at the ASan + UBSan build
of the binary.
"""
import os
import subprocess
import sys
from pathlib import Path

import pytest

from dispatch_model import kernel_class

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))

import isa_compare  # noqa: E402
import vmem_hazard_check as vh  # noqa: E402

LIB = ROOT / "zsummerx_amd" / "libzrc4.so"
CRYPT_KERNELS = 49          # win 12, decl 10, half 10, whole 11, stream 6
LLVM_OK = all((vh.LLVM / t).exists() for t in ("llvm-objdump", "llvm-objcopy", "clang-offload-bundler"))


def _plan_check(*args):
    exe = Path(os.environ.get("ZSX_TOOLS_BIN", ROOT / "tools" / "bin")) / "plan_check"
    return subprocess.run([str(exe), *args], capture_output=True, text=True)


def test_plan_table(built):
    got = _plan_check()
    assert got.returncode == 0, got.stdout + got.stderr
    rows, _, rest = got.stdout.strip().splitlines()[-1].partition(" rows, ")
    assert int(rows) >= 100 and rest == "0 mismatches", got.stdout


@pytest.mark.skipif(not LLVM_OK, reason="ROCm LLVM tools not found")
def test_sweep_reaches_exactly_the_built_kernels(built):
    got = _plan_check("sweep")
    assert got.returncode == 0, got.stdout + got.stderr       # every plan names a form that exists
    reached = set(got.stdout.split())
    names = list(vh.kernel_resources(LIB))
    keys = {isa_compare._key(d).split("zrc4::", 1)[-1] for d in isa_compare._demangle(names).values()}
    built_crypt = {k for k in keys if k.startswith("crypt_")}
    assert len(built_crypt) == CRYPT_KERNELS, sorted(built_crypt)
    assert reached == built_crypt, (sorted(built_crypt - reached), sorted(reached - built_crypt))


def test_family_follows_kernel_class(built):
    got = _plan_check("classes")
    assert got.returncode == 0, got.stderr
    lines = got.stdout.splitlines()
    assert len(lines) == 2 * 2 * 700 * 3 * 2
    for line in lines:
        mode, aligned, groups, cus, _frame, family = line.split()
        want = kernel_class({"1": "range", "2": "grouped"}[mode], 0 if aligned == "1" else 37, int(groups), int(cus))
        assert family == want, line
