"""The reservoir hooks (zsummerx_amd/engine/rc4_hooks_device.cpp) refill their
rings through the write-only zrc4_keystream_grouped (include/zrc4.h): the
rings are never zeroed, never read by the device, and only the levels say
which ring bytes hold keystream.  tests/cpp/hooks_check.cpp drives the hooks
like the session engine and checks every byte against the oracle RC4
(rc4_encryption.h:46-93); here it runs with fresh ring slabs poisoned with
0xA5 ($ZSX_RING_POISON=1, so a ring byte read outside the levels cannot pass
for the zero the old refills relied on), the reservoir alone
($ZSX_RC4_DIRECT_BYTES=0), and every refill counted as a keystream launch.

CPU: over the emulation of the C-ABI (tests/cpp/emu_zrc4_hip.cpp with
tests/cpp/emu_zrc4_keystream.cpp), plus the emulated calls themselves against
the oracle (tests/cpp/emu_keystream_check.cpp).  GPU: the gfx950 path."""
import json
import os
import subprocess

import pytest

from conftest import ROOT

BIN = ROOT / "tools" / "bin"
ENV = dict(os.environ, ZSX_RING_POISON="1", ZSX_RC4_DIRECT_BYTES="0")


@pytest.fixture(scope="module")
def tools(built):
    from zsummerx_amd import build
    build.build_test_tools()
    return BIN


def run(exe, *args):
    p = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, timeout=300, env=ENV)
    assert p.returncode == 0, (p.stdout, p.stderr)
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["ok"], out
    h = out["hooks"]
    assert h["refill_launches"] > 0 and h["keystream_launches"] == h["refill_launches"], h
    return out


def test_emulated_keystream_calls_vs_oracle(tools):
    """zrc4_keystream_range / zrc4_keystream_grouped of the emulation: oracle
    keystream in the spans, skipped spans and guard bytes untouched, a mixed
    bucket refused, every stream continued by a following crypt."""
    p = subprocess.run([str(tools / "emu_keystream_check")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.count(": ok") == 10 and "MISMATCH" not in p.stdout, p.stdout


@pytest.mark.parametrize("ring", [256, 4096])
def test_reservoir_poisoned_rings_emulated(tools, ring):
    run(tools / "hooks_check_emu", "device", 40, 120, 5, ring)


@pytest.mark.gpu
def test_reservoir_poisoned_rings_small_ring(tools):
    run(tools / "hooks_check", "device", 64, 60, 7, 4096)


@pytest.mark.gpu
def test_reservoir_poisoned_rings_at_scale(tools):
    run(tools / "hooks_check", "device", 2048, 20, 3)
