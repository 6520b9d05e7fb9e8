"""Engine broadcast (include/zsummerx_amd/frame.h: broadcastSessionData,
broadcastAccepter; include/zsummerx_amd/rc4_hooks.h: Rc4Hooks::cryptBatch): one
plaintext for N sessions, encrypted out of place from one shared copy.

Wire parity (tests/broadcast_support.py): 6 keyed clients and 2 on a plain
accepter beside them, Python oracle peers, each decrypting its whole stream
with one continuous RC4.  CPU: the oracle as hooks (the base-class cryptBatch)
and the device hooks over the CPU emulation of the C-ABI.  GPU: the product
hooks in reservoir, direct and direct + device-framing mode.

tools/bin/hooks_bcast_check drives cryptBatch without sockets (random in-place
spans and to-spans with shared sources, slots in both lists, reseeds, rings
below the message size) and checks its whole pool against the oracle."""
import json
import os
import subprocess
from pathlib import Path

import pytest

from broadcast_support import ORACLE_HOOKS, run_broadcast_parity
from conftest import ROOT

STRESS = Path(os.environ.get("ZSX_STRESS", str(ROOT / "zsummerx_amd" / "bin" / "frame_stress")))


def tools_bin(built):
    from zsummerx_amd import build
    if os.environ.get("ZSX_TOOLS_BIN"):                # sanitizer builds of the *_emu binaries
        return Path(os.environ["ZSX_TOOLS_BIN"])
    build.build_test_tools()
    return ROOT / "tools" / "bin"


@pytest.fixture(scope="module")
def stress(built):
    from zsummerx_amd import build
    build.build_frame()
    assert STRESS.exists()
    return STRESS


@pytest.fixture(scope="module")
def stress_emu(built):
    return tools_bin(built) / "frame_stress_emu"


@pytest.fixture(scope="module")
def check_emu(built):
    return tools_bin(built) / "hooks_bcast_check_emu"


@pytest.fixture(scope="module")
def check(built):
    from zsummerx_amd import build
    build.build_test_tools()
    return ROOT / "tools" / "bin" / "hooks_bcast_check"


def check_paths(st, device_hooks):
    """The shared-source path ran, and ran behind staged bytes (the sender of
    the quiet-phase broadcast: its echo, then the broadcast at a nonzero
    offset of the same block)."""
    assert st["bcast_shared"] >= 6, st                 # the quiet phase alone: every keyed session
    assert st["bcast_joined"] >= 1, st
    assert st["mismatches"] == 0
    if device_hooks:
        assert st["hooks"]["to_spans"] == st["bcast_shared"], st
        assert st["hooks"]["to_bytes"] > 0


def run_check(binary, *args, timeout=120):
    p = subprocess.run([str(binary), *map(str, args)], capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    st = json.loads(p.stdout.strip().splitlines()[-1])
    assert st["ok"] and st["to_spans"] > 0 and st["slot_in_both"] > 0 and st["apart"] > 0 and st["non_congruent"] > 0
    return st


# ------------------------------------------------------------------ CPU
def test_broadcast_parity_cpu_hooks(stress):
    """The interface's own cryptBatch: hooks that have only crypt()."""
    st = run_broadcast_parity(stress, ORACLE_HOOKS)
    assert st["rc4"] == "host:oracle"
    check_paths(st, False)


def test_broadcast_parity_emulated_device_hooks(stress_emu):
    st = run_broadcast_parity(stress_emu, "device")
    assert st["rc4"] == "zrc4-gfx950"
    check_paths(st, True)


def test_broadcast_parity_emulated_small_ring(stress_emu):
    """A 256-byte ring: most regions are partly ring-covered, partly device tail."""
    st = run_broadcast_parity(stress_emu, "device", extra=("--ring", "256"), seed0=4100)
    check_paths(st, True)
    assert st["hooks"]["tail_bytes"] > 0


def test_broadcast_parity_emulated_direct(stress_emu):
    st = run_broadcast_parity(stress_emu, "device-direct", seed0=4200)
    assert st["rc4"] == "zrc4-gfx950-direct"
    check_paths(st, True)


def test_broadcast_parity_emulated_device_framing(stress_emu):
    st = run_broadcast_parity(stress_emu, "device-direct", extra=("--device-framing",), seed0=4300)
    check_paths(st, True)
    assert st["device_framed"] > 0


@pytest.mark.parametrize("ring", [256, 1000, 4096])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_hooks_bcast_check_emulated_reservoir(check_emu, seed, ring):
    st = run_check(check_emu, "device", 40, 30, seed, ring)
    assert st["hooks"]["to_spans"] == st["to_spans"] and st["hooks"]["to_bytes"] == st["to_bytes"]
    assert st["hooks"]["ring_bytes"] > 0 and st["hooks"]["tail_bytes"] > 0


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_hooks_bcast_check_emulated_direct(check_emu, seed):
    st = run_check(check_emu, "direct", 300, 12, seed)          # 600 slots: three buckets per launch
    assert st["hooks"]["to_spans"] == st["to_spans"]


def test_hooks_bcast_check_base_class(check_emu):
    run_check(check_emu, "base", 40, 30, 1)


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("hooks,extra", [("device", ()), ("device-direct", ()),
                                         ("device-direct", ("--device-framing",))],
                         ids=["reservoir", "direct", "direct-framing"])
def test_broadcast_parity_device(stress, hooks, extra):
    st = run_broadcast_parity(stress, hooks, extra=extra)
    assert st["rc4"] == ("zrc4-gfx950" if hooks == "device" else "zrc4-gfx950-direct")
    check_paths(st, True)
    if extra:
        assert st["device_framed"] > 0


# Sessions whose write slots fill 16, 100 and 200 buckets of 256 (a session
# holds two slots): the out-of-place launch of the direct mode is then the
# window kernel, the declared half-group kernel and the declared whole-group
# kernel (csrc/zrc4_plan.hpp).
@pytest.mark.gpu
@pytest.mark.parametrize("sessions,rounds", [(2048, 9), (12800, 5), (25600, 4)])
@pytest.mark.parametrize("mode", ["direct", "device"])
def test_hooks_bcast_check_device(check, mode, sessions, rounds):
    st = run_check(check, mode, sessions, rounds, 1, 4096)
    assert st["hooks"]["to_spans"] == st["to_spans"] and st["hooks"]["to_bytes"] == st["to_bytes"]
