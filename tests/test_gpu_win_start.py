"""The window kernel's way from kernel entry to its first window
(zsummerx_amd/csrc/zrc4_win.hpp): the entry's length, offsets and x/y are
loaded on every lane, the chunk-0 payload prefetch is issued on every lane
without a branch (a unit past the message reads the message's last whole unit
of that lane again, or the lane's sink bytes), and the compiler's waits around
them are counted.  What can go wrong there is a load or store outside a span,
a stale unit XORed into the payload, or a state built from the wrong entry.

Every case stays on the window kernel (at most 32 groups, asserted through
tests/dispatch_model.py), compares payload and states bit for bit against the
oracle (pyoracle.Batch: RC4Encryption::encryption,
depends/rc4/rc4_encryption.h:74-93), and keeps 64 guard bytes before and after
every span, which must read back untouched.

  lengths   0, 1, 15, 16, 17, 255, 1 023, 1 024, 2 047, 2 048, 2 049, 4 097
            mixed within one call: no unit, a ragged tail, one whole unit, the
            2 KiB ring chunk and the chunks after it
  starts    16-byte aligned spans shifted by 0 (the 16-byte prefetch path), 1
            and 8 bytes (the byte path), and 0 / 1 / 8 cycling within one call
  range     n = 1, 3, 255, 256, 257, 300: partly idle and wholly idle dword
            columns of the last group (the return with loads in flight)
  grouped   slots permuted inside a group, ZRC4_IDLE_SLOT padding, one idle
            bucket, one bucket whose only busy entry has length 0; declared
            and undeclared
  forms     in place, write-only keystream, out of place (source alignment
            equal to and different from the destination's), framing launch
"""
import numpy as np
import pytest

import pyoracle
from dispatch_model import family
from frame_support import BOUND, frame_report, payload_report
from gpu_support import FILL, assert_equal, buckets, check_continues, check_states, cu_count, host, oracle, seeded
from gpu_support import torch_cuda  # noqa: F401
from zsummerx_amd._capi import IDLE_SLOT

pytestmark = pytest.mark.gpu

LENS = np.array([0, 1, 15, 16, 17, 255, 1023, 1024, 2047, 2048, 2049, 4097], dtype=np.uint32)
GUARD = 64
SHIFTS = [0, 1, 8, "mixed"]
NS = [1, 3, 255, 256, 257, 300]


def _lens(n):
    """Entry i's length: the list from its end in steps of 5 (coprime to its
    size), so that n = 1 is the longest message and n = 3 already holds a
    ragged one and a whole chunk."""
    return LENS[(LENS.size - 1 + 5 * np.arange(n)) % LENS.size]


def _shifts(kind, n):
    if kind == "mixed":
        return np.array([0, 1, 8], dtype=np.uint64)[np.arange(n) % 3]
    return np.full(n, kind, dtype=np.uint64)


def _spans(L, shifts):
    """Span i starts at a 16-byte boundary plus shifts[i], GUARD bytes or more
    behind the end of span i - 1 plus its own GUARD: offsets, buffer size."""
    off = np.empty(L.size, dtype=np.uint64)
    pos = 0
    for i in range(L.size):
        start = ((pos + GUARD + 15) & ~15) + int(shifts[i])
        off[i] = start
        pos = start + int(L[i]) + GUARD
    return off, pos + 16


def _index(off, L):
    L = L.astype(np.int64)
    start = np.cumsum(L) - L
    return np.repeat(off.astype(np.int64) - start, L) + np.arange(int(L.sum()), dtype=np.int64)


def _oracle_crypt(ob, cap, buf, slots, off, L):
    so = np.zeros(cap, dtype=np.uint64)
    sl = np.zeros(cap, dtype=np.uint32)
    so[slots] = off
    sl[slots] = L
    ob.crypt(buf, so, sl)


def _run(torch, c, ob, T, cap, rng, form, how, L, kind, first=0, ids=None, groups=None):
    """One call of `form` ("inplace", "ks", "to") through `how` ("range",
    "grouped", "declared") and its checks: every byte of the destination
    (spans and guards), the source where there is one, every state."""
    s = torch.cuda.current_stream()
    n = L.size
    if how == "range":
        busy = np.ones(n, dtype=bool)
        slots = first + np.arange(n)
    else:
        busy = ids != IDLE_SLOT
        slots = ids[busy].astype(np.int64)
    assert family(how, first, n, cu_count(torch), {"inplace": 0, "ks": 1, "to": 2}[form]) == "win"
    sh = _shifts(kind, n)
    doff, size = _spans(L, sh)
    Td, Tl = T(doff.view(np.int64)), T(L.view(np.int32))
    Ti = None if ids is None else T(ids.view(np.int32))
    decl = groups if how == "declared" else None
    what = f"{form} {how} n={n} shift={kind}"
    if form == "inplace":
        data = rng.integers(0, 256, size, dtype=np.uint8)
        want = data.copy()
        _oracle_crypt(ob, cap, want, slots, doff[busy], L[busy])
        buf = T(data)
        if how == "range":
            c.crypt_range(first, buf, Td, Tl, stream=s)
        elif how == "grouped":
            c.crypt_grouped(buf, Td, Tl, Ti, stream=s)
        else:
            c.crypt_grouped_declared(buf, Td, Tl, Ti, groups, stream=s)
        c.sync(s)
        rep = payload_report(host(buf), want, doff, L)
        assert not rep, (what, rep)
    elif form == "ks":
        want = np.full(size, FILL, dtype=np.uint8)
        want[_index(doff[busy], L[busy])] = 0
        _oracle_crypt(ob, cap, want, slots, doff[busy], L[busy])
        out = T(np.full(size, FILL, dtype=np.uint8))
        if how == "range":
            c.keystream_range(first, out, Td, Tl, stream=s)
        else:
            c.keystream_grouped(out, Td, Tl, Ti, decl, stream=s)
        c.sync(s)
        rep = payload_report(host(out), want, doff, L)
        assert not rep, (what, rep)
    else:
        # every other entry's source 8 bytes off its destination's alignment
        ssh = (sh + np.uint64(8) * (np.arange(n, dtype=np.uint64) % np.uint64(2))) % np.uint64(16)
        soff, ssize = _spans(L, ssh)
        assert ((soff - doff) % np.uint64(16) != 0).any() or n == 1
        src = rng.integers(0, 256, ssize, dtype=np.uint8)
        want = np.full(size, FILL, dtype=np.uint8)
        want[_index(doff[busy], L[busy])] = src[_index(soff[busy], L[busy])]
        _oracle_crypt(ob, cap, want, slots, doff[busy], L[busy])
        ts, td = T(src.copy()), T(np.full(size, FILL, dtype=np.uint8))
        Ts = T(soff.view(np.int64))
        if how == "range":
            c.crypt_to_range(first, ts, Ts, td, Td, Tl, stream=s)
        else:
            c.crypt_to_grouped(ts, Ts, td, Td, Tl, Ti, decl, stream=s)
        c.sync(s)
        rep = payload_report(host(td), want, doff, L)
        assert not rep, (what, rep)
        assert_equal(host(ts), src, what + ": source changed")
    check_states(c, ob, cap)


# -- range, aligned first slot --------------------------------------------------------

@pytest.mark.parametrize("kind", SHIFTS, ids=lambda k: f"shift{k}")
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("form", ["inplace", "ks", "to"])
def test_range(built, torch_cuda, form, n, kind):
    torch = torch_cuda
    cap = 768                                            # group 2 is never touched
    c, ob, T = seeded(torch, 9100 + n, cap)
    rng = np.random.default_rng(9200 + n)
    with c:
        _run(torch, c, ob, T, cap, rng, form, "range", _lens(n), kind, first=256)


# -- grouped and declared -------------------------------------------------------------

GROUPS = np.array([2, IDLE_SLOT, 0, 3, 1], dtype=np.uint32)      # bucket 1 idle; group 4 never touched
G_CAP = 5 * 256


def _grouped_case(rng):
    """Bucket 0 a random subset of group 2, bucket 1 idle, bucket 2 all of
    group 0 permuted, bucket 3 one busy entry of group 3 with length 0, bucket
    4 a random subset of group 1; idle entries have spans too (never touched)."""
    ids = np.concatenate([buckets(rng, GROUPS[0:1]), buckets(rng, GROUPS[1:2]),
                          buckets(rng, GROUPS[2:3], fill=(256, 256)), buckets(rng, GROUPS[3:4], fill=(1, 1)),
                          buckets(rng, GROUPS[4:5])])
    L = _lens(ids.size).copy()
    lone = 768 + int(np.flatnonzero(ids[768:1024] != IDLE_SLOT)[0])
    L[lone] = 0
    idle = ids == IDLE_SLOT
    L[idle] = np.maximum(L[idle], 1)                      # an idle entry's span would show a store
    assert (ids[256:512] == IDLE_SLOT).all() and (ids[512:768] != IDLE_SLOT).all()
    assert (ids[512:768] != 256 * 0 + np.arange(256)).any()
    return ids, L


@pytest.mark.parametrize("kind", SHIFTS, ids=lambda k: f"shift{k}")
@pytest.mark.parametrize("how", ["grouped", "declared"])
@pytest.mark.parametrize("form", ["inplace", "ks", "to"])
def test_grouped(built, torch_cuda, form, how, kind):
    torch = torch_cuda
    c, ob, T = seeded(torch, 9300, G_CAP)
    rng = np.random.default_rng(9400 + SHIFTS.index(kind))
    with c:
        ids, L = _grouped_case(rng)
        _run(torch, c, ob, T, G_CAP, rng, form, how, L, kind, ids=ids, groups=GROUPS)


# -- framing launch -------------------------------------------------------------------

def test_range_frame_300(built, torch_cuda):
    """zrc4_crypt_range_frame over 300 sessions: the FRAME instantiation.  The
    plaintext of every session starts with a packet header naming about half
    its length, so the walk finds whole packets, short tails and bad headers."""
    torch = torch_cuda
    n, cap, maxp = 300, 512, 4
    c, ob, T = seeded(torch, 9500, cap)
    enc, *_ = oracle(9500, cap)                            # the same streams, to make the ciphertext
    rng = np.random.default_rng(9501)
    s = torch.cuda.current_stream()
    with c:
        L = _lens(n)
        off, size = _spans(L, _shifts("mixed", n))
        plain = rng.integers(0, 256, size, dtype=np.uint8)
        for i in np.flatnonzero(L >= 6):
            plain[int(off[i]):int(off[i]) + 4] = np.frombuffer(int(max(6, L[i] // 2)).to_bytes(4, "little"), np.uint8)
        data = plain.copy()
        _oracle_crypt(enc, cap, data, np.arange(n), off, L)
        _oracle_crypt(ob, cap, data.copy(), np.arange(n), off, L)       # advances the checker's streams
        want = pyoracle.frame_scan(plain, off, L, BOUND, maxp)
        sent = lambda k: T(np.full(k, 0xFFFFFFFF, np.uint32).view(np.int32))
        npk, used, status, pk = sent(n), sent(n), sent(n), sent(n * maxp)
        Toff, Tlen = T(off.view(np.int64)), T(L.view(np.int32))
        frame = {"off": Toff, "len": Tlen, "bound": BOUND, "max_packets": maxp, "npk": npk, "used": used,
                 "status": status, "pkt_len": pk}
        buf = T(data)
        c.crypt_range_frame(0, buf, Toff, Tlen, frame, stream=s)
        c.sync(s)
        rep = payload_report(host(buf), plain, off, L)
        assert not rep, rep
        u32 = lambda t: host(t).view(np.uint32)
        for name, w, g in (("npk", want[0], u32(npk)), ("used", want[1], u32(used)), ("status", want[2], u32(status))):
            rep = frame_report(w, g, name)
            assert not rep, rep
        assert (want[0] > 0).any() and (want[2] != want[2][0]).any()      # the walk saw more than one outcome
        filled = np.arange(maxp)[None, :] < np.minimum(want[0], maxp)[:, None]
        assert_equal(u32(pk).reshape(n, maxp)[filled], want[3][:, :maxp][filled], "pkt_len")
        check_states(c, ob, cap)


# -- continuity and empty calls -------------------------------------------------------

@pytest.mark.parametrize("how", ["range", "grouped", "declared"])
def test_two_calls_continue(built, torch_cuda, how):
    """Two calls in a row on the same sessions (the second starts from the
    x/y and image the first stored), then a crypt_range over every slot."""
    torch = torch_cuda
    cap = 512 if how == "range" else G_CAP
    c, ob, T = seeded(torch, 9600, cap)
    rng = np.random.default_rng(9601)
    with c:
        if how == "range":
            ids, L = None, _lens(300)
        else:
            ids, L = _grouped_case(rng)
        for kind in ("mixed", 0):
            _run(torch, c, ob, T, cap, rng, "inplace", how, np.roll(L, 3 * (kind == 0)) if ids is None else L, kind,
                 ids=ids, groups=GROUPS)
        check_continues(torch, c, ob, T, cap, rng)


@pytest.mark.parametrize("how", ["range", "grouped", "declared"])
@pytest.mark.parametrize("form", ["inplace", "ks", "to"])
def test_all_lengths_zero(built, torch_cuda, form, how):
    """Every length 0: no byte moves, every S-box, x and y is bit-identical."""
    torch = torch_cuda
    cap = 512 if how == "range" else G_CAP
    c, ob, T = seeded(torch, 9700, cap)
    rng = np.random.default_rng(9701)
    with c:
        before = c.get_states(0, cap)
        ids = None if how == "range" else _grouped_case(rng)[0]
        n = 300 if ids is None else ids.size
        _run(torch, c, ob, T, cap, rng, form, how, np.zeros(n, dtype=np.uint32), "mixed", ids=ids, groups=GROUPS)
        after = c.get_states(0, cap)
        for a, b in zip(before, after):
            assert np.array_equal(a, b)
