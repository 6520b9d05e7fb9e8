"""CPU tests of the multi-round out-of-place crypt calls' boundary
(include/zrc4.h: zrc4_crypt_to_range_rounds, zrc4_crypt_to_grouped_rounds):
declared in the header with their contract, exported by the built library,
bound by ctypes and wrapped by Context; the argument errors are answered
without a launch.  The checks on `rounds` come before the library looks for a
device, so they run anywhere; the ones behind it need a context and are marked
gpu, as tests/test_crypt_to_api.py leaves every call that needs one to the GPU
suite.  Also here, because it needs no device: the GPU sweep's generator
(tests/test_gpu_crypt_to_rounds.py) never produces overlapping destinations."""
import ctypes as C
import re

import numpy as np
import pytest

from conftest import ROOT

NEW = ("zrc4_crypt_to_range_rounds", "zrc4_crypt_to_grouped_rounds")
OK, INVALID_ARG = 0, -1
MAX_ROUNDS = 64


def _header():
    return (ROOT / "include" / "zrc4.h").read_text()


def test_header_declares_both_functions():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    decl = {m.group(1): re.sub(r"\s+", " ", m.group(2))
            for m in re.finditer(r"\bint\s+(zrc4_crypt_to_\w+_rounds)\s*\(([^)]*)\)", text)}
    assert set(decl) == set(NEW)
    for name in NEW:
        a = decl[name]
        assert "const uint8_t *src, const uint64_t *src_off" in a, a
        assert "uint8_t *dst, const uint64_t *dst_off" in a and "const uint8_t *dst" not in a, a
        assert a.endswith("const uint32_t *len, uint32_t n, uint32_t rounds, void *stream"), a
    assert decl[NEW[0]].startswith("zrc4_ctx *ctx, uint32_t first_slot,")
    assert decl[NEW[1]].startswith("zrc4_ctx *ctx, const uint32_t *ids, const uint32_t *bucket_group,")
    assert re.search(r"#define\s+ZRC4_MAX_ROUNDS\s+64u\b", text)


def test_header_states_the_contract():
    text = re.sub(r"[\s*]+", " ", _header())
    for phrase in ("ROUND-MAJOR", "of round r is at index","`rounds` successive", "loaded once and stored once",
                   "skips that round for that slot only", "ONCE PER LAUNCH", "judged busy by its ids",
                   "untouched in every round", "over the union of ALL rounds", "pairwise disjoint",
                   "rounds > ZRC4_MAX_ROUNDS", "0xFFF00000", "has no rounds form", "from a host loop",
                   "PER ROUND", "all-or-nothing per round, not per call"):
        assert phrase in text, phrase


def test_library_exports_both(built):
    from zsummerx_amd import _capi
    lib = C.CDLL(str(_capi.LIB_PATH))
    for name in NEW:
        assert hasattr(lib, name), name
    sigs = {n: (r, a) for n, r, a in _capi.SIGNATURES}
    assert len(sigs[NEW[0]][1]) == 10 and len(sigs[NEW[1]][1]) == 11
    assert sigs[NEW[0]][0] is C.c_int and sigs[NEW[1]][0] is C.c_int
    # n and rounds are the two 32-bit integers ahead of the stream
    for name in NEW:
        assert sigs[name][1][-3:-1] == [C.c_uint32, C.c_uint32], name


def test_wrapper_exposes_both_methods():
    import inspect
    from zsummerx_amd import Context
    assert list(inspect.signature(Context.crypt_to_range_rounds).parameters) == [
        "self", "first_slot", "src", "src_off", "dst", "dst_off", "length", "n", "rounds", "stream"]
    assert list(inspect.signature(Context.crypt_to_grouped_rounds).parameters) == [
        "self", "src", "src_off", "dst", "dst_off", "length", "ids", "n", "rounds", "bucket_group", "stream"]


class _NoLib:
    """Stands where the loaded library does: any call through it is a failure."""
    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def test_wrapper_rejects_a_short_bucket_group():
    from zsummerx_amd import Context
    c = Context.__new__(Context)                 # no device: the check comes before the call
    c._lib, c._h = _NoLib(), None
    with pytest.raises(ValueError, match="bucket_group"):
        c.crypt_to_grouped_rounds(0, 0, 0, 0, 0, 0, 600, 3, bucket_group=[0, 1])      # 600 entries: 3 buckets


def _calls(lib, ctx, a, n, rounds):
    return (lib.zrc4_crypt_to_range_rounds(ctx, 0, a, a, a, a, a, n, rounds, None),
            lib.zrc4_crypt_to_grouped_rounds(ctx, a, None, a, a, a, a, a, n, rounds, None))


def test_null_context_is_invalid_arg(built):
    from zsummerx_amd import _capi
    lib = _capi.load()
    buf = (C.c_uint8 * 16)()
    a = C.cast(buf, C.c_void_p)
    assert _calls(lib, None, a, 1, 2) == (INVALID_ARG, INVALID_ARG)


class _Handle:
    """A stand-in context pointer for the checks that come before the context
    is read: zeroed memory, never a live context."""
    def __init__(self):
        self.mem = (C.c_uint8 * 4096)()
        self.p = C.cast(self.mem, C.c_void_p)


@pytest.mark.parametrize("n,rounds", [(1, 0), (0, 0), (1, MAX_ROUNDS + 1), (1, 0xFFFFFFFF),
                                      (0xFFF00000 // 64 + 1, 64), (0xFFF00001, 2), (0x80000000, 2)],
                         ids=["rounds0", "rounds0-n0", "rounds65", "rounds-max", "n*64-over", "n*2-over", "n*2-wraps"])
def test_rounds_and_product_limits_need_no_device(built, n, rounds):
    """rounds == 0, rounds > ZRC4_MAX_ROUNDS and n * rounds > 0xFFF00000 (in 64
    bits: 0x80000000 * 2 wraps to 0 in 32) are refused before the context, a
    device or any table is touched."""
    from zsummerx_amd import _capi
    lib = _capi.load()
    h = _Handle()
    assert _calls(lib, h.p, h.p, n, rounds) == (INVALID_ARG, INVALID_ARG)
    assert not any(h.mem)                         # (nothing was written through it either)


@pytest.fixture()
def ctx(built):
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from zsummerx_amd import Context
    with Context(0, 512) as c:
        yield c


@pytest.mark.gpu
def test_null_tables_are_invalid_arg(ctx):
    """Every NULL table with n > 0, at rounds 2 and (forwarded) at rounds 1."""
    import torch
    lib, h = ctx._lib, ctx._h
    t = torch.zeros(64, dtype=torch.int64, device="cuda")
    a = C.c_void_p(t.data_ptr())
    for rounds in (1, 2):
        for k in range(5):                                   # src, src_off, dst, dst_off, len
            args = [a] * 5
            args[k] = None
            assert lib.zrc4_crypt_to_range_rounds(h, 0, *args, 4, rounds, None) == INVALID_ARG, (rounds, k)
            assert lib.zrc4_crypt_to_grouped_rounds(h, a, None, *args, 4, rounds, None) == INVALID_ARG, (rounds, k)
        assert lib.zrc4_crypt_to_grouped_rounds(h, None, None, a, a, a, a, a, 4, rounds, None) == INVALID_ARG
    ctx.sync()


@pytest.mark.gpu
def test_n_zero_is_ok(ctx):
    """n == 0 with valid rounds: ZRC4_OK, NULL tables and all, nothing launched."""
    lib, h = ctx._lib, ctx._h
    for rounds in (1, 2, MAX_ROUNDS):
        assert lib.zrc4_crypt_to_range_rounds(h, 0, None, None, None, None, None, 0, rounds, None) == OK
        assert lib.zrc4_crypt_to_grouped_rounds(h, None, None, None, None, None, None, None, 0, rounds, None) == OK
    ctx.sync()


@pytest.mark.gpu
def test_bad_declared_group_is_invalid_arg(ctx):
    """bucket_group naming a group >= capacity / 256: refused, nothing launched
    (zrc4_crypt_to_grouped's rule)."""
    import torch
    lib, h = ctx._lib, ctx._h
    t = torch.zeros(64, dtype=torch.int64, device="cuda")
    a = C.c_void_p(t.data_ptr())
    bg = (C.c_uint32 * 1)(2)                                 # capacity 512: groups 0 and 1
    assert lib.zrc4_crypt_to_grouped_rounds(h, a, C.cast(bg, C.c_void_p), a, a, a, a, a, 4, 2, None) == INVALID_ARG
    ctx.sync()


def test_sweep_generator_never_overlaps_destinations():
    """The seeded sweep of tests/test_gpu_crypt_to_rounds.py (sweep_call of
    tests/gpu_support.py), generator only:
    over its own ten calls and 200 more, all destination spans of all rounds
    are pairwise disjoint, sources stay inside their buffer, buckets are valid
    (one group each, no group twice, no slot twice), and the ten calls cover
    one round, several rounds, one bucket-ish and many buckets."""
    import gpu_support as g
    from zsummerx_amd._capi import IDLE_SLOT
    rng = np.random.default_rng(9999)                        # the sweep's seed
    seen_rounds, seen_nb = set(), set()
    for call in range(g.SWEEP_CALLS + 200):
        ids, groups, rounds, L, doff, size, soff, ssize = g.sweep_call(rng)
        n = ids.size
        assert 1 <= rounds <= 6 and 1 <= n // 256 <= 40 and n % 256 == 0
        assert L.size == doff.size == soff.size == rounds * n
        assert g.disjoint(doff, L), call
        assert int((doff + L).max()) <= size and int((soff + L).max()) <= ssize
        busy = ids[ids != IDLE_SLOT]
        assert busy.size and np.unique(busy).size == busy.size and (busy < g.SWEEP_GROUPS * 256).all()
        assert np.unique(groups).size == groups.size
        for b, gr in enumerate(groups):
            mine = ids[256 * b: 256 * b + 256]
            assert ((mine[mine != IDLE_SLOT] >> 8) == gr).all()
        if call < g.SWEEP_CALLS:
            rng.integers(0, 256, ssize, dtype=np.uint8)      # the draw the GPU test makes between calls
            seen_rounds.add(rounds)
            seen_nb.add(n // 256)
    assert len(seen_rounds) >= 3 and min(seen_nb) <= 8 and max(seen_nb) >= 24, (seen_rounds, seen_nb)


def test_disjoint_helper_sees_an_overlap():
    import gpu_support as g
    off = np.array([0, 10, 30], dtype=np.uint64)
    assert g.disjoint(off, np.array([10, 20, 5], dtype=np.uint32))
    assert not g.disjoint(off, np.array([11, 20, 5], dtype=np.uint32))
    assert g.disjoint(off, np.array([10, 0, 5], dtype=np.uint32))          # zero-length spans take no byte
    assert not g.disjoint(np.array([5, 0], dtype=np.uint64), np.array([5, 6], dtype=np.uint32))
