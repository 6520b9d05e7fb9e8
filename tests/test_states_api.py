"""CPU tests of the bulk state calls' surface: the header declares them, the
ctypes binding and Context carry them, and each refuses a NULL context before
it looks for a device."""
import ctypes as C
import re

import pytest

from conftest import ROOT

CALLS = ["zrc4_export_states", "zrc4_import_states", "zrc4_copy_states", "zrc4_set_states"]


def test_header_declares_the_state_calls():
    text = (ROOT / "include" / "zrc4.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = set(re.findall(r"\b(zrc4_[a-z_]+)\s*\(", text))
    assert set(CALLS) <= syms


def test_binding_and_context_carry_the_state_calls(built):
    from zsummerx_amd import Context, _capi
    bound = {n for n, _, _ in _capi.SIGNATURES}
    assert set(CALLS) <= bound
    lib = _capi.load()
    for name in CALLS:
        assert getattr(lib, name).restype is C.c_int
    for m in ("export_states", "import_states", "copy_states", "set_states"):
        assert callable(getattr(Context, m))


@pytest.mark.parametrize("call", CALLS)
def test_null_context_is_invalid_arg(built, call):
    from zsummerx_amd import _capi
    lib = _capi.load()
    buf = (C.c_uint8 * 512)()
    p = C.cast(buf, C.c_void_p)
    if call == "zrc4_copy_states":
        rc = lib.zrc4_copy_states(None, None, 0, None, None, 0, 1, None)
    elif call == "zrc4_set_states":
        rc = lib.zrc4_set_states(None, 0, 1, p, p, p)
    else:
        rc = getattr(lib, call)(None, None, 0, 1, p, p, None)
    assert rc == -1
