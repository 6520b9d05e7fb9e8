"""CPU tests of the out-of-place crypt calls' boundary (include/zrc4.h:
zrc4_crypt_to_range, zrc4_crypt_to_grouped): declared in the header, exported
by the built library, bound by ctypes and wrapped by Context; argument errors
that need no device are answered as the existing calls answer them.  No compute
calls here (the GPU parity is tests/test_gpu_crypt_to.py)."""
import ctypes as C
import re

import numpy as np
import pytest

from conftest import ROOT

NEW = ("zrc4_crypt_to_range", "zrc4_crypt_to_grouped")
INVALID_ARG = -1


def _header():
    return (ROOT / "include" / "zrc4.h").read_text()


def test_header_declares_both_functions():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    decl = {m.group(1): re.sub(r"\s+", " ", m.group(2)) for m in re.finditer(r"\bint (zrc4_crypt_to_\w+)\s*\(([^)]*)\)", text)}
    assert set(decl) == set(NEW)
    for name in NEW:
        a = decl[name]
        # a const source and a writable destination, each with its own offsets
        assert "const uint8_t *src, const uint64_t *src_off" in a, a
        assert "uint8_t *dst, const uint64_t *dst_off" in a and "const uint8_t *dst" not in a, a
        assert a.endswith("const uint32_t *len, uint32_t n, void *stream"), a
    assert decl[NEW[0]].startswith("zrc4_ctx *ctx, uint32_t first_slot,")
    assert decl[NEW[1]].startswith("zrc4_ctx *ctx, const uint32_t *ids, const uint32_t *bucket_group,")


def test_header_states_the_contract():
    text = re.sub(r"[\s*]+", " ", _header())
    for phrase in ("`src` is never written", "outside the spans are never written", "SAME ADDRESS",
                   "may overlap each other freely", "must not overlap another entry's destination span",
                   "never partly crypted", "TWO launches", "written twice and read once"):
        assert phrase in text, phrase


def test_library_exports_both(built):
    from zsummerx_amd import _capi
    lib = C.CDLL(str(_capi.LIB_PATH))
    for name in NEW:
        assert hasattr(lib, name), name
    sigs = {n: (r, a) for n, r, a in _capi.SIGNATURES}
    assert len(sigs[NEW[0]][1]) == 9 and len(sigs[NEW[1]][1]) == 10
    assert sigs[NEW[0]][0] is C.c_int and sigs[NEW[1]][0] is C.c_int


def test_wrapper_exposes_both_methods():
    import inspect
    from zsummerx_amd import Context
    assert list(inspect.signature(Context.crypt_to_range).parameters) == [
        "self", "first_slot", "src", "src_off", "dst", "dst_off", "length", "n", "stream"]
    assert list(inspect.signature(Context.crypt_to_grouped).parameters) == [
        "self", "src", "src_off", "dst", "dst_off", "length", "ids", "bucket_group", "n", "stream"]


class _NoLib:
    """Stands where the loaded library does: any call through it is a failure."""
    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def test_wrapper_rejects_a_short_bucket_group():
    from zsummerx_amd import Context
    c = Context.__new__(Context)                 # no device: the check comes before the call
    c._lib, c._h = _NoLib(), None
    z = np.zeros(600, dtype=np.uint32)
    with pytest.raises(ValueError, match="bucket_group"):
        c.crypt_to_grouped(0, 0, 0, 0, z, 0, bucket_group=[0, 1], n=600)       # 600 entries: 3 buckets
    with pytest.raises(ValueError, match="bucket_group"):
        c.keystream_grouped(0, 0, z, 0, bucket_group=[0, 1], n=600)            # (the call it follows)


def test_null_context_is_invalid_arg(built):
    """As zrc4_crypt_range / zrc4_keystream_grouped answer it: before any
    device call."""
    from zsummerx_amd import _capi
    lib = _capi.load()
    buf = (C.c_uint8 * 16)()
    a = C.cast(buf, C.c_void_p)
    assert lib.zrc4_crypt_range(None, 0, a, a, a, 1, None) == INVALID_ARG
    assert lib.zrc4_keystream_grouped(None, a, None, a, a, a, 1, None) == INVALID_ARG
    assert lib.zrc4_crypt_to_range(None, 0, a, a, a, a, a, 1, None) == INVALID_ARG
    assert lib.zrc4_crypt_to_grouped(None, a, None, a, a, a, a, a, 1, None) == INVALID_ARG
