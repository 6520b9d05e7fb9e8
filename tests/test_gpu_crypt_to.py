"""GPU parity of the out-of-place crypt calls (include/zrc4.h:
zrc4_crypt_to_range, zrc4_crypt_to_grouped): entry i reads its SOURCE span and
stores source ^ keystream to its DESTINATION span; sources may be shared by
any number of entries.  The oracle is pyoracle.Batch.crypt over a host copy of
the gathered sources (RC4Encryption::encryption, depends/rc4/rc4_encryption.h:
74-93, in place on each session's own copy of the message -- what
TcpSession::send does, src/frame/session.cpp:533-538, 584-606).

Every destination buffer is pre-filled with 0xA5 and spans are separated by
guard bytes.  Every case checks the destination spans bit-exactly, that every
other destination byte is still 0xA5, that the source buffer is byte-identical
to what it was, that every state of the context equals the oracle's, and that
a following crypt_range of 24 bytes per slot continues every stream.

Kernel paths on 256 CUs: 1 / 32 groups the window kernel, 33 / 128 the
half-group kernel, 129 / 256 the whole-group kernel, 257 the span copy and the
persistent kernel; first_slot = 3 the gather path; grouped 2 / 33 / 200 / 300
buckets the same four, declared and undeclared.  "Congruent" layouts keep
(source - destination) a multiple of 16 (16-byte loads from the source);
"non-congruent" ones take the byte path for most entries."""
import numpy as np
import pytest

from gpu_support import (FILL, LONG, SHORT, assert_equal, buckets, check_continues, check_states, host, layout, oracle,
                         seeded, sources, span_index)
from gpu_support import torch_cuda  # noqa: F401
from zsummerx_amd import ZRC4Error
from zsummerx_amd._capi import IDLE_SLOT

pytestmark = pytest.mark.gpu


def _want(ob, cap, size, slots, src, soff, doff, L, base=None):
    """The expected destination: `base` (default 0xA5 everywhere) with the
    source bytes of entry i gathered into span i and crypted there by the
    oracle as slot slots[i]; the oracle advanced."""
    want = np.full(size, FILL, dtype=np.uint8) if base is None else base.copy()
    want[span_index(doff, L)] = src[span_index(soff, L)]
    so = np.zeros(cap, dtype=np.uint64)
    sl = np.zeros(cap, dtype=np.uint32)
    so[slots] = doff
    sl[slots] = L
    ob.crypt(want, so, sl)
    return want


def _run_range(torch, c, ob, T, cap, first, src, soff, doff, L, size, what, Tsrc=None, Tdst=None):
    """One crypt_to_range over fresh buffers, the five checks but the last."""
    s = torch.cuda.current_stream()
    n = L.size
    want = _want(ob, cap, size, first + np.arange(n), src, soff, doff, L)
    ts = (Tsrc or T)(src.copy())
    td = (Tdst or T)(np.full(size, FILL, dtype=np.uint8))
    c.crypt_to_range(first, ts, T(soff.view(np.int64)), td, T(doff.view(np.int64)), T(L.view(np.int32)), stream=s)
    c.sync(s)
    assert_equal(host(td), want, what)
    assert_equal(host(ts), src, what + ": source changed")


# -- range ---------------------------------------------------------------------

@pytest.mark.parametrize("congruent", [True, False], ids=["congruent", "noncongruent"])
@pytest.mark.parametrize("groups", [1, 32, 33, 128, 129, 256, 257])
def test_crypt_to_range_whole_groups(built, torch_cuda, groups, congruent):
    torch = torch_cuda
    rng = np.random.default_rng(7100 + groups)
    lens = LONG if groups <= 32 else SHORT
    n = 256 * groups
    cap = n + 256                                        # one group the call does not touch
    c, ob, T = seeded(torch, 8100 + groups, cap)
    with c:
        pos = np.arange(n) % lens.size
        L = lens[pos]
        doff, size = layout(L, groups % 16)
        # every length of the list meets every start misalignment of the destination
        pairs = set(zip(pos.tolist(), (doff % 16).tolist()))
        assert len(pairs) == 16 * lens.size or n < 16 * lens.size, len(pairs)
        if congruent:
            soff, ssize = doff + np.uint64(48), size + 48
        else:
            soff, ssize = layout(L, (groups + 5) % 16, cycle=5)
            d = ((soff.astype(np.int64) - doff.astype(np.int64)) % 16)
            for k in range(lens.size):                   # nonzero (src - dst) mod 16 for every length of the list
                assert (d[pos == k] != 0).any(), k
        src = rng.integers(0, 256, ssize, dtype=np.uint8)
        _run_range(torch, c, ob, T, cap, 0, src, soff, doff, L, size, "crypt_to_range")
        check_continues(torch, c, ob, T, cap, rng)


def test_crypt_to_range_unaligned_first_slot(built, torch_cuda):
    """first_slot = 3, n = 700: three workgroups on the gather path (a slot's
    S-box column by column), slots 0-2 and 703.. untouched."""
    torch = torch_cuda
    rng = np.random.default_rng(7400)
    first, n, cap = 3, 700, 1024
    c, ob, T = seeded(torch, 8400, cap)
    with c:
        L = SHORT[np.arange(n) % SHORT.size]
        doff, size = layout(L, 7)
        soff, ssize = layout(L, 2, cycle=5)
        soff[::2] = doff[::2] + np.uint64(32)            # every other entry congruent
        ssize = max(ssize, size + 32)
        src = rng.integers(0, 256, ssize, dtype=np.uint8)
        _run_range(torch, c, ob, T, cap, first, src, soff, doff, L, size, "crypt_to_range first_slot=3")
        check_continues(torch, c, ob, T, cap, rng)


# -- broadcast -------------------------------------------------------------------

@pytest.mark.parametrize("groups,length", [(1, 64), (1, 1029), (33, 250), (129, 250), (257, 100), (1, -1), (33, -2),
                                           (257, -2)],
                         ids=["1g-64B", "1g-1KiB+5", "33g-250B", "129g-250B", "257g-100B", "1g-prefix-long",
                              "33g-prefix-short", "257g-prefix-short"])
def test_crypt_to_broadcast(built, torch_cuda, groups, length):
    """One message for every session: every entry has the same src_off (and
    length; `prefix`: lengths cycling through the list, every entry a prefix
    of the one message)."""
    torch = torch_cuda
    rng = np.random.default_rng(7500 + groups + max(length, 0))
    n = 256 * groups
    cap = n + 256
    c, ob, T = seeded(torch, 8500 + groups, cap)
    with c:
        if length > 0:
            L = np.full(n, length, dtype=np.uint32)
        else:
            lens = LONG if length == -1 else SHORT
            L = lens[np.arange(n) % lens.size]
        doff, size = layout(L, 3)
        soff = np.full(n, 21, dtype=np.uint64)
        src = rng.integers(0, 256, 21 + int(L.max()) + 9, dtype=np.uint8)
        _run_range(torch, c, ob, T, cap, 0, src, soff, doff, L, size, "broadcast")
        check_continues(torch, c, ob, T, cap, rng)


# -- in place through the new call --------------------------------------------------

@pytest.mark.parametrize("groups", [1, 33, 257])
def test_crypt_to_in_place(built, torch_cuda, groups):
    """src is dst and src_off == dst_off: exactly crypt_range's bytes and states."""
    torch = torch_cuda
    rng = np.random.default_rng(7600 + groups)
    lens = LONG if groups <= 32 else SHORT
    n = 256 * groups
    cap = n + 256
    c, ob, T = seeded(torch, 8600 + groups, cap)
    s = torch.cuda.current_stream()
    with c:
        L = lens[np.arange(n) % lens.size]
        off, size = layout(L, groups % 16)
        data = rng.integers(0, 256, size, dtype=np.uint8)
        want = data.copy()
        ob.crypt(want, np.concatenate((off, np.zeros(256, np.uint64))), np.concatenate((L, np.zeros(256, np.uint32))))
        buf, toff = T(data), T(off.view(np.int64))
        c.crypt_to_range(0, buf, toff, buf, toff, T(L.view(np.int32)), stream=s)
        c.sync(s)
        assert_equal(buf.cpu().numpy(), want, "in place through crypt_to_range")
        check_continues(torch, c, ob, T, cap, rng)


# -- grouped -------------------------------------------------------------------

def _grouped_case(rng, nb, G, idle_bucket=True):
    groups = rng.permutation(G)[:nb].astype(np.uint32)
    if idle_bucket:
        groups[nb // 2] = IDLE_SLOT
    ids = buckets(rng, groups)
    # every entry has a span (idle entries too: theirs must stay 0xA5);
    # SHORT holds a zero, so some busy entries have len == 0
    L = SHORT[rng.integers(0, SHORT.size, ids.size)]
    busy = np.flatnonzero(ids != IDLE_SLOT)
    idle = np.flatnonzero(ids == IDLE_SLOT)
    L[busy[busy.size // 2]] = 0                          # whatever the draw: a busy entry with no bytes,
    assert busy.size and idle.size
    L[idle[idle.size // 2]] = 17                         # and an idle one with a span to keep
    return groups, ids, L


def _run_grouped(torch, c, ob, T, cap, ids, groups, src, soff, doff, L, size, ran, what):
    s = torch.cuda.current_stream()
    want = _want(ob, cap, size, ids[ran], src, soff[ran], doff[ran], L[ran])
    ts, td = T(src.copy()), T(np.full(size, FILL, dtype=np.uint8))
    c.crypt_to_grouped(ts, T(soff.view(np.int64)), td, T(doff.view(np.int64)), T(L.view(np.int32)),
                       T(ids.view(np.int32)), groups, stream=s)
    return want, ts, td


@pytest.mark.parametrize("declared", [False, True], ids=["undeclared", "declared"])
@pytest.mark.parametrize("nb", [2, 33, 200, 300])
def test_crypt_to_grouped(built, torch_cuda, nb, declared):
    torch = torch_cuda
    rng = np.random.default_rng(7700 + nb + declared)
    G = nb + 8
    cap = 256 * G
    c, ob, T = seeded(torch, 8700 + nb, cap)
    s = torch.cuda.current_stream()
    with c:
        groups, ids, L = _grouped_case(rng, nb, G)
        doff, size = layout(L, nb % 16)
        soff, ssize = sources(rng, L, doff)
        busy = ids != IDLE_SLOT
        assert (L[busy] == 0).any() and (L[~busy] != 0).any()
        d = (soff.astype(np.int64) - doff.astype(np.int64)) % 16
        assert (d[busy] == 0).any() and (d[busy] != 0).any()
        src = rng.integers(0, 256, ssize, dtype=np.uint8)
        want, ts, td = _run_grouped(torch, c, ob, T, cap, ids, groups if declared else None, src, soff, doff, L, size,
                                    busy, "grouped")
        c.sync(s)
        assert_equal(td.cpu().numpy(), want, "crypt_to_grouped")
        assert_equal(ts.cpu().numpy(), src, "crypt_to_grouped: source changed")
        check_continues(torch, c, ob, T, cap, rng)


def test_crypt_to_grouped_id_out_of_range(built, torch_cuda):
    """One id >= capacity: ZRC4_ERR_SLOT_RANGE, its span still 0xA5, the rest
    of its bucket (and every other bucket) exact."""
    torch = torch_cuda
    nb = 33
    rng = np.random.default_rng(7900)
    G = nb + 8
    cap = 256 * G
    c, ob, T = seeded(torch, 8900, cap)
    s = torch.cuda.current_stream()
    with c:
        groups, ids, L = _grouped_case(rng, nb, G, idle_bucket=False)
        e = int(np.flatnonzero(ids[:256] == IDLE_SLOT)[0]) if (ids[:256] == IDLE_SLOT).any() else 0
        ids[e] = cap + 77
        L[e] = 193
        doff, size = layout(L, nb % 16)
        soff, ssize = sources(rng, L, doff)
        ran = (ids != IDLE_SLOT) & (ids < cap)
        src = rng.integers(0, 256, ssize, dtype=np.uint8)
        want, ts, td = _run_grouped(torch, c, ob, T, cap, ids, groups, src, soff, doff, L, size, ran, "range fault")
        with pytest.raises(ZRC4Error) as ei:
            c.sync(s)
        assert ei.value.code == -5                         # ZRC4_ERR_SLOT_RANGE
        got = td.cpu().numpy()
        assert (got[int(doff[e]): int(doff[e]) + 193] == FILL).all()
        assert_equal(got, want, "id out of range")
        assert_equal(ts.cpu().numpy(), src, "id out of range: source changed")
        check_continues(torch, c, ob, T, cap, rng)


# -- refusal -------------------------------------------------------------------

@pytest.mark.parametrize("declared", [False, True], ids=["undeclared", "declared"])
@pytest.mark.parametrize("nb", [2, 300])
def test_crypt_to_grouped_two_buckets_one_group(built, torch_cuda, nb, declared):
    """Buckets 0 and 1 name the same group (disjoint slots of it): each of the
    group's claim parts goes to one of them, the other bucket's entries of
    that part are refused (ZRC4_ERR_GROUP).  Which bucket wins a part is the
    hardware's choice, so the test reads it off the result: an entry's span
    is either exactly its crypt (the slot ran, and its state advanced) or --
    refused -- untouched at 2 buckets, untouched or a plain copy of the
    source at 300; never anything else."""
    torch = torch_cuda
    rng = np.random.default_rng(7800 + nb + declared)
    G = nb + 8
    cap = 256 * G
    seed = 8800 + nb
    c, ob, T = seeded(torch, seed, cap)
    s = torch.cuda.current_stream()
    with c:
        groups, ids, L = _grouped_case(rng, nb, G, idle_bucket=False)
        g = int(groups[0])
        groups[1] = g
        perm = rng.permutation(256)
        ids[:512] = IDLE_SLOT
        ids[rng.permutation(256)[:100]] = g * 256 + perm[:100]
        ids[256 + rng.permutation(256)[:100]] = g * 256 + perm[100:200]
        L[:512] = np.maximum(L[:512], 16)                # long enough to tell crypted from copied or untouched
        doff, size = layout(L, nb % 16)
        soff, ssize = sources(rng, L, doff)
        src = rng.integers(0, 256, ssize, dtype=np.uint8)
        busy = ids != IDLE_SLOT
        # what every span would hold had every entry run (a second oracle)
        all_ran = _want(oracle(seed, cap)[0], cap, size, ids[busy], src, soff[busy], doff[busy], L[busy])
        ts, td = T(src.copy()), T(np.full(size, FILL, dtype=np.uint8))
        c.crypt_to_grouped(ts, T(soff.view(np.int64)), td, T(doff.view(np.int64)), T(L.view(np.int32)),
                           T(ids.view(np.int32)), groups if declared else None, stream=s)
        with pytest.raises(ZRC4Error) as ei:
            c.sync(s)
        assert ei.value.code == -7                         # ZRC4_ERR_GROUP
        got = td.cpu().numpy()
        ran = busy.copy()
        for e in np.flatnonzero(busy[:512]):
            a, z = int(doff[e]), int(doff[e]) + int(L[e])
            sp = got[a:z]
            if (sp == all_ran[a:z]).all():
                continue
            ran[e] = False
            copied = (sp == src[int(soff[e]): int(soff[e]) + int(L[e])]).all()
            assert (sp == FILL).all() or (nb > 256 and copied), (e, sp[:16])
            sp[:] = FILL
        assert not ran[:512][busy[:512]].all()           # somebody was refused
        want = _want(ob, cap, size, ids[ran], src, soff[ran], doff[ran], L[ran])
        assert_equal(got, want, "two buckets, one group")
        assert_equal(ts.cpu().numpy(), src, "refusal: source changed")
        check_continues(torch, c, ob, T, cap, rng)        # (states: the oracle ran exactly the slots that ran)


# -- pinned host memory ----------------------------------------------------------------

@pytest.mark.parametrize("where", ["src_pinned", "dst_pinned"])
@pytest.mark.parametrize("groups", [1, 33])
def test_crypt_to_pinned_host(built, torch_cuda, groups, where):
    torch = torch_cuda
    rng = np.random.default_rng(7950 + groups)
    lens = LONG if groups <= 32 else SHORT
    n = 256 * groups
    cap = n + 256
    c, ob, T = seeded(torch, 8950 + groups, cap)
    P = lambda a: torch.from_numpy(np.ascontiguousarray(a)).pin_memory()
    with c:
        L = lens[np.arange(n) % lens.size]
        doff, size = layout(L, 9)
        soff, ssize = layout(L, 4, cycle=5)
        soff[::2] = doff[::2] + np.uint64(16)
        ssize = max(ssize, size + 16)
        src = rng.integers(0, 256, ssize, dtype=np.uint8)
        _run_range(torch, c, ob, T, cap, 0, src, soff, doff, L, size, where,
                   Tsrc=P if where == "src_pinned" else None, Tdst=P if where == "dst_pinned" else None)
        check_continues(torch, c, ob, T, cap, rng)


# -- random sweep ----------------------------------------------------------------------

def test_crypt_to_random_sweep(built, torch_cuda):
    """20 seeded calls on one context, the oracle carried across them: group
    counts around every kernel threshold, lengths 0..300 (0..4100 up to 32
    groups), any misalignment, sources overlapping freely (half the entries
    read from one shared start, the rest anywhere in the source buffer)."""
    torch = torch_cuda
    rng = np.random.default_rng(7999)
    counts = [1, 2, 3, 31, 32, 33, 34, 127, 128, 129, 130, 255, 256, 257, 258]
    cap = 259 * 256
    c, ob, T = seeded(torch, 8999, cap)
    with c:
        for call in range(20):
            groups = int(counts[call] if call < len(counts) else rng.choice(counts))
            n = 256 * (groups - 1) + int(rng.integers(1, 257))
            L = rng.integers(0, 4101 if groups <= 32 else 301, n).astype(np.uint32)
            gap = rng.integers(1, 18, n).astype(np.uint64)
            end = np.cumsum(L.astype(np.uint64) + gap)
            doff = np.concatenate(([0], end[:-1])).astype(np.uint64) + np.uint64(rng.integers(0, 16))
            size = int(end[-1]) + 32
            ssize = int(L.max()) + 4096
            src = rng.integers(0, 256, ssize, dtype=np.uint8)
            soff = (rng.random(n) * (ssize - L.astype(np.int64))).astype(np.uint64)
            soff[rng.random(n) < 0.5] = int(rng.integers(0, 4096))
            some = rng.random(n) < 0.25                  # a quarter congruent with their destination
            adj = soff[some] + (doff[some] - soff[some]) % np.uint64(16)
            ok = adj + L[some].astype(np.uint64) <= ssize
            soff[np.flatnonzero(some)[ok]] = adj[ok]
            _run_range(torch, c, ob, T, cap, 0, src, soff, doff, L, size, f"sweep call {call} ({groups} groups)")
            check_states(c, ob, cap)
        check_continues(torch, c, ob, T, cap, rng)
