"""The window loop's exits (zrc4::win_windows, zsummerx_amd/csrc/zrc4_win.hpp).
The loop runs two windows per trip and leaves either from the middle (a
forward branch after the first half) or from the bottom, per wave and per
2 KiB chunk; both halves alternate two address registers and share one drain.
What that can newly get wrong is the exit: which half the wave leaves from,
streams of one wave that finish in different halves (a finished stream goes on
with rem = 0: it cuts 0, commits nothing, its tag still advances), and the
state the next chunk's or the next call's preamble picks up (x, y, tag, ring
position).

Every case stays on the window kernel (asserted through
tests/dispatch_model.py), compares payload and every state bit for bit with
the oracle (pyoracle.Batch: RC4Encryption::encryption,
depends/rc4/rc4_encryption.h:74-93) and keeps 64 guard bytes around every
span, through the call helper of tests/test_gpu_win_start.py.

  short call   entry i has (7 i) % 49 bytes (0, 7, .., 42: 0-7 windows); the
               four streams of a wave (entries e, e + 32, e + 64, e + 96 of a
               128-entry half) get four different lengths
  long call    the same entries with LONG[i % 6] = 2 047, 2 048, 2 049, 4 097,
               6 145, 1 024 bytes: re-entry into the loop per 2 KiB chunk and
               the headline's own length
  edge call    entry i has (11 i) % 49 bytes: every length 0-48, so every
               16-byte edge, again four different lengths per wave; after
               the long call, from the states it left
  starts       16-byte aligned spans, and shifted by 1
  calls        range (first slot 256, n = 300, capacity 768), grouped and
               declared (slots permuted inside each group, one idle bucket),
               write-only keystream, out of place, the framing launch, and the
               ZRC4_WIN_TAG_LIMIT=4 library on the long call (the marker
               restart then falls in either half)

The precondition is computed on the CPU before any launch of the range case:
tools/window_sim.py's prga_window at W = 16 over the states get_states
returns, chunk by chunk (2 048 bytes, state carried over), gives the window
count of every stream in every chunk, and the case must hold what it is
there for (window_counts).
"""
import sys
from pathlib import Path

import numpy as np
import pytest

import pyoracle
from dispatch_model import family
from frame_support import BOUND, frame_report, payload_report
from gpu_support import assert_equal, buckets, check_continues, check_states, cu_count, dev, host, oracle, seeded
from gpu_support import torch_cuda  # noqa: F401
from test_gpu_win_start import _oracle_crypt, _run, _shifts, _spans
from zsummerx_amd import Context
from zsummerx_amd._capi import IDLE_SLOT

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
import window_sim  # noqa: E402

pytestmark = pytest.mark.gpu

N, CAP, FIRST, SEED = 300, 768, 256, 9800
CHUNK, W = 2048, 16
LONG = np.array([2047, 2048, 2049, 4097, 6145, 1024], dtype=np.uint32)
SHORT_L = ((7 * np.arange(N)) % 49).astype(np.uint32)
LONG_L = LONG[np.arange(N) % 6]
EDGE_L = ((11 * np.arange(N)) % 49).astype(np.uint32)
KINDS = [0, 1]


def _windows(S, x, y, L):
    """Window counts of one stream per 2 KiB chunk of an L-byte message, and
    the state after it."""
    counts = []
    for c0 in range(0, L, CHUNK):
        _, S, x, y, w = window_sim.prga_window(S, x, y, min(CHUNK, L - c0), W)
        counts.append(w)
    return counts, S, x, y


def _waves(n):
    """Entries of the four streams of every wave of a range launch: dword
    column q of a group holds group-lanes 128 h + L + 32 b, b = 0..3."""
    for g0 in range(0, n, 256):
        for h in range(2):
            for lane in range(32):
                yield [e for e in (g0 + 128 * h + lane + 32 * b for b in range(4)) if e < n]


@pytest.fixture(scope="module")
def window_counts(built, torch_cuda):
    """Per entry of the range case, the window counts per chunk of the short
    and of the long call (the long call starts where the short one ended),
    from the states of a context seeded as every case here is."""
    c, ob, T = seeded(torch_cuda, SEED, CAP)
    with c:
        sb, gx, gy = c.get_states(FIRST, N)
    short, long_ = [], []
    for i in range(N):
        S, x, y = [int(v) for v in sb[i]], int(gx[i]), int(gy[i])
        cs, S, x, y = _windows(S, x, y, int(SHORT_L[i]))
        cl, S, x, y = _windows(S, x, y, int(LONG_L[i]))
        short.append(cs)
        long_.append(cl)
    return short, long_


def _check_precondition(counts):
    short, long_ = counts
    first = [c[0] if c else 0 for c in short]             # length 0: no window
    assert 1 in first and 2 in first, sorted(set(first))
    mixed = [w for w in _waves(N) if len({first[e] % 2 for e in w if SHORT_L[e]}) == 2]
    assert mixed, "no wave with window counts of both parities in chunk 0"
    later = {c % 2 for cl in long_ for c in cl[1:]}
    assert later == {0, 1}, later
    # and the four streams of a full wave have four different lengths
    assert all(len({int(L[e]) for e in w}) == 4 for w in _waves(256) for L in (SHORT_L, EDGE_L))
    assert set(EDGE_L.tolist()) == set(range(49))


def _two_calls(torch, c, ob, T, cap, rng, form, how, kind, ids=None, groups=None, Ls=None):
    for L in Ls if Ls is not None else (SHORT_L, LONG_L, EDGE_L):
        _run(torch, c, ob, T, cap, rng, form, how, L, kind, first=FIRST, ids=ids, groups=groups)


# -- range ----------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS, ids=lambda k: f"shift{k}")
def test_range_exits(built, torch_cuda, window_counts, kind):
    _check_precondition(window_counts)
    torch = torch_cuda
    c, ob, T = seeded(torch, SEED, CAP)
    rng = np.random.default_rng(SEED + 1 + kind)
    with c:
        _two_calls(torch, c, ob, T, CAP, rng, "inplace", "range", kind)
        check_continues(torch, c, ob, T, CAP, rng)


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: f"shift{k}")
@pytest.mark.parametrize("form", ["ks", "to"])
def test_range_forms(built, torch_cuda, form, kind):
    torch = torch_cuda
    c, ob, T = seeded(torch, SEED, CAP)
    rng = np.random.default_rng(SEED + 10 + kind)
    with c:
        _two_calls(torch, c, ob, T, CAP, rng, form, "range", kind)


# -- grouped and declared -------------------------------------------------------------

GROUPS = np.array([2, IDLE_SLOT, 0, 1], dtype=np.uint32)         # bucket 1 idle; group 3 never touched
G_CAP = 4 * 256


def _grouped_case(rng):
    """Bucket 0 a random subset of group 2, bucket 1 idle, bucket 2 all of
    group 0 permuted, bucket 3 a random subset of group 1; entry i has the
    range case's lengths of entry i % 300 (idle entries have spans too, never
    touched)."""
    ids = np.concatenate([buckets(rng, GROUPS[0:1]), buckets(rng, GROUPS[1:2]),
                          buckets(rng, GROUPS[2:3], fill=(256, 256)), buckets(rng, GROUPS[3:4])])
    assert (ids[256:512] == IDLE_SLOT).all() and (ids[512:768] != IDLE_SLOT).all()
    assert (ids[512:768] != np.arange(256)).any()
    e = np.arange(ids.size) % N
    idle = ids == IDLE_SLOT
    Ls = [L[e].copy() for L in (SHORT_L, LONG_L, EDGE_L)]
    for L in Ls:
        L[idle] = np.maximum(L[idle], 1)                  # an idle entry's span would show a store
    return ids, Ls


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: f"shift{k}")
@pytest.mark.parametrize("how", ["grouped", "declared"])
@pytest.mark.parametrize("form", ["inplace", "ks", "to"])
def test_grouped_exits(built, torch_cuda, form, how, kind):
    torch = torch_cuda
    c, ob, T = seeded(torch, SEED + 20, G_CAP)
    rng = np.random.default_rng(SEED + 21 + kind)
    with c:
        ids, Ls = _grouped_case(rng)
        _two_calls(torch, c, ob, T, G_CAP, rng, form, how, kind, ids=ids, groups=GROUPS, Ls=Ls)


# -- framing launch -------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS, ids=lambda k: f"shift{k}")
def test_range_frame_exits(built, torch_cuda, kind):
    """zrc4_crypt_range_frame over the 300 sessions, the short call and then
    the long one: the FRAME instantiation of the same loop.  The plaintext of
    every session of six bytes or more starts with a packet header naming
    about half its length."""
    torch = torch_cuda
    maxp = 4
    c, ob, T = seeded(torch, SEED + 30, CAP)
    enc, *_ = oracle(SEED + 30, CAP)                       # the same streams, to make the ciphertext
    rng = np.random.default_rng(SEED + 31 + kind)
    s = torch.cuda.current_stream()
    assert family("range", 0, N, cu_count(torch)) == "win"
    with c:
        for L in (SHORT_L, LONG_L, EDGE_L):
            off, size = _spans(L, _shifts(kind, N))
            plain = rng.integers(0, 256, size, dtype=np.uint8)
            for i in np.flatnonzero(L >= 6):
                plain[int(off[i]):int(off[i]) + 4] = np.frombuffer(int(max(6, L[i] // 2)).to_bytes(4, "little"),
                                                                   np.uint8)
            data = plain.copy()
            _oracle_crypt(enc, CAP, data, np.arange(N), off, L)
            _oracle_crypt(ob, CAP, data.copy(), np.arange(N), off, L)       # advances the checker's streams
            want = pyoracle.frame_scan(plain, off, L, BOUND, maxp)
            sent = lambda k: T(np.full(k, 0xFFFFFFFF, np.uint32).view(np.int32))
            npk, used, status, pk = sent(N), sent(N), sent(N), sent(N * maxp)
            Toff, Tlen = T(off.view(np.int64)), T(L.view(np.int32))
            frame = {"off": Toff, "len": Tlen, "bound": BOUND, "max_packets": maxp, "npk": npk, "used": used,
                     "status": status, "pkt_len": pk}
            buf = T(data)
            c.crypt_range_frame(0, buf, Toff, Tlen, frame, stream=s)
            c.sync(s)
            rep = payload_report(host(buf), plain, off, L)
            assert not rep, rep
            u32 = lambda t: host(t).view(np.uint32)
            for name, w, g in (("npk", want[0], u32(npk)), ("used", want[1], u32(used)),
                               ("status", want[2], u32(status))):
                rep = frame_report(w, g, name)
                assert not rep, rep
            filled = np.arange(maxp)[None, :] < np.minimum(want[0], maxp)[:, None]
            assert_equal(u32(pk).reshape(N, maxp)[filled], want[3][:, :maxp][filled], "pkt_len")
            check_states(c, ob, CAP)


# -- marker restart -------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS, ids=lambda k: f"shift{k}")
def test_tag_restart_exits(built, torch_cuda, kind):
    """The library that restarts the marker tags at every chunk
    (ZRC4_WIN_TAG_LIMIT=4) on the short and the long call: tags count windows
    of either half, streams past their end included, so the restart (markers
    cleared, tags back to 1) follows exits from both halves."""
    from zsummerx_amd import build
    torch = torch_cuda
    var = build.build_variant("wintag4", build.TEST_VARIANTS["wintag4"])
    ob, keys, koff, klen = oracle(SEED + 40, CAP)
    T = dev(torch)
    rng = np.random.default_rng(SEED + 41 + kind)
    with Context(0, CAP, lib=var) as c:
        c.ksa_range(0, T(klen.view(np.int32)), T(koff.view(np.int64)), T(keys), stream=torch.cuda.current_stream())
        _two_calls(torch, c, ob, T, CAP, rng, "inplace", "range", kind)
        _run(torch, c, ob, T, CAP, rng, "inplace", "range", LONG_L, kind, first=FIRST)
