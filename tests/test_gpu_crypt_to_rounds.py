"""GPU parity of the multi-round out-of-place crypt calls (include/zrc4.h:
zrc4_crypt_to_range_rounds, zrc4_crypt_to_grouped_rounds): one launch that
behaves like `rounds` successive zrc4_crypt_to_* calls on the same slots, the
tables round-major (entry i of round r at r * n + i).  The oracle is
pyoracle.Batch.crypt, one stream per slot, fed the rounds' sources in order
(RC4Encryption::encryption, depends/rc4/rc4_encryption.h:74-93, called once per
message of a session: what TcpSession::send does for each of them in turn,
src/frame/session.cpp:533-538, 584-606).

Every destination buffer is pre-filled with 0xA5 and every span of every round
is separated from the next by guard bytes.  Every case checks all destination
spans of all rounds bit-exactly, that every other destination byte is still
0xA5, that the source is byte-identical to what it was, every state of the
context against the oracle's, and that a following crypt_range of 24 bytes per
slot continues every stream.

Kernel paths with C CUs (256 on MI355X): 1 and 33 groups the half-group kernel
(1: where a one-round call takes the window kernel), C/2 + 1 the whole-group
kernel, 257 the host loop over the two-launch one-round calls; first_slot = 3
the gather path; grouped 2 and 200 buckets the half-group and whole-group
kernels, declared and undeclared."""
import numpy as np
import pytest

from dispatch_model import rounds_groups
from gpu_support import (FILL, SWEEP_CALLS, SWEEP_GROUPS, assert_equal, buckets, check_continues, check_states, cu_count,
                         disjoint, host, layout, oracle, seeded, span_index, sweep_call)
from gpu_support import torch_cuda  # noqa: F401
from zsummerx_amd import ZRC4Error
from zsummerx_amd._capi import IDLE_SLOT

gpu = pytest.mark.gpu

# nothing, head or tail bytes only, one 16-byte piece and around it, one block
# and around it, four blocks with pieces and a tail
LENS = np.array([0, 1, 15, 16, 17, 63, 64, 65, 300], dtype=np.uint32)
HEAD_ONLY = np.array([1, 15], dtype=np.uint32)         # (300 bytes run the block loop at any alignment)


def _want(ob, cap, base, slots, ran, src, soff, doff, L, rounds):
    """`base` with, round after round, the source bytes of every entry that
    runs gathered into its span and crypted there by the oracle as its slot;
    the oracle advanced.  Tables round-major, `slots` and `ran` per entry."""
    want = base.copy()
    n = slots.size
    for r in range(rounds):
        so, do, l = soff[r * n:(r + 1) * n][ran], doff[r * n:(r + 1) * n][ran], L[r * n:(r + 1) * n][ran]
        want[span_index(do, l)] = src[span_index(so, l)]
        po = np.zeros(cap, dtype=np.uint64)
        pl = np.zeros(cap, dtype=np.uint32)
        po[slots[ran]] = do
        pl[slots[ran]] = l
        ob.crypt(want, po, pl)
    return want


def _round_lengths(rng, n, rounds):
    """Lengths [rounds, n] from LENS.  From three rounds on every lane has a
    zero round, a head-only round and a round of 300 bytes (the block loop at
    any alignment) at random positions; with fewer rounds every length of the
    list turns up in every round."""
    L = LENS[rng.integers(0, LENS.size, (rounds, n))]
    if rounds >= 3:
        order = np.argsort(rng.random((rounds, n)), axis=0)[:3]         # three distinct rounds per lane
        cols = np.arange(n)
        L[order[0], cols] = 0
        L[order[1], cols] = HEAD_ONLY[rng.integers(0, 2, n)]
        L[order[2], cols] = 300
        assert ((L == 0).any(axis=0) & np.isin(L, HEAD_ONLY).any(axis=0) & (L == 300).any(axis=0)).all()
    elif n >= 256:
        for r in range(rounds):
            assert set(L[r].tolist()) == set(LENS.tolist())
    return L


def _range_tables(rng, n, rounds, congruent, shift):
    """Round-major tables of a range call: every span of every round has its
    own place in the destination; sources 48 bytes on in a buffer of their own
    (congruent), or 49..63 bytes on ((src - dst) mod 16 nonzero everywhere)."""
    L = _round_lengths(rng, n, rounds).reshape(-1)
    doff, size = layout(L, shift)
    if congruent:
        soff = doff + np.uint64(48)
    else:
        soff = doff + np.uint64(48) + rng.integers(1, 16, L.size).astype(np.uint64)
        assert ((soff - doff) % np.uint64(16) != 0).all()
    return L, doff, size, soff, size + 64


def _run_range(torch, c, ob, T, cap, first, n, rounds, src, soff, doff, L, size, what, Tsrc=None, Tdst=None):
    """One crypt_to_range_rounds over fresh buffers: destination, guards and source."""
    s = torch.cuda.current_stream()
    assert disjoint(doff, L)
    slots = first + np.arange(n)
    want = _want(ob, cap, np.full(size, FILL, dtype=np.uint8), slots, np.ones(n, dtype=bool), src, soff, doff, L, rounds)
    ts = (Tsrc or T)(src.copy())
    td = (Tdst or T)(np.full(size, FILL, dtype=np.uint8))
    c.crypt_to_range_rounds(first, ts, T(soff.view(np.int64)), td, T(doff.view(np.int64)), T(L.view(np.int32)), n,
                            rounds, stream=s)
    c.sync(s)
    assert_equal(host(td), want, what)
    assert_equal(host(ts), src, what + ": source changed")


# -- range ---------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("congruent", [True, False], ids=["congruent", "noncongruent"])
@pytest.mark.parametrize("which,rounds", [("1", 1), ("1", 2), ("1", 5), ("1", 64), ("33", 2), ("33", 5), ("half+1", 2),
                                          ("half+1", 5), ("257", 2), ("257", 5)])
def test_rounds_range_whole_groups(built, torch_cuda, which, rounds, congruent):
    torch = torch_cuda
    groups = rounds_groups(which, cu_count(torch))
    rng = np.random.default_rng(9100 + 100 * groups + rounds)
    n = 256 * groups
    cap = n + 256                                        # one group the call does not touch
    c, ob, T = seeded(torch, 9200 + groups, cap)
    with c:
        L, doff, size, soff, ssize = _range_tables(rng, n, rounds, congruent, groups % 16)
        src = rng.integers(0, 256, ssize, dtype=np.uint8)
        _run_range(torch, c, ob, T, cap, 0, n, rounds, src, soff, doff, L, size, f"{groups} groups x {rounds} rounds")
        check_continues(torch, c, ob, T, cap, rng)


@gpu
@pytest.mark.parametrize("rounds", [2, 5])
def test_rounds_range_unaligned_first_slot(built, torch_cuda, rounds):
    """first_slot = 3, n = 700: three workgroups on the gather path; slots 0-2
    and 703.. untouched.  Every other entry-round congruent."""
    torch = torch_cuda
    rng = np.random.default_rng(9300 + rounds)
    first, n, cap = 3, 700, 1024
    c, ob, T = seeded(torch, 9301, cap)
    with c:
        L, doff, size, soff, ssize = _range_tables(rng, n, rounds, False, 7)
        soff[::2] = doff[::2] + np.uint64(32)
        src = rng.integers(0, 256, ssize, dtype=np.uint8)
        _run_range(torch, c, ob, T, cap, first, n, rounds, src, soff, doff, L, size, "first_slot=3")
        check_continues(torch, c, ob, T, cap, rng)


# -- equivalence ---------------------------------------------------------------

@gpu
@pytest.mark.parametrize("which", ["1", "half+1"])
def test_rounds_equal_successive_calls(built, torch_cuda, which):
    """One rounds call on context A against R successive zrc4_crypt_to_range
    calls on context B with the same seeds: the same destination bytes and the
    same states (at 1 group B runs the window kernel, A the half-group one)."""
    torch = torch_cuda
    groups, rounds = rounds_groups(which, cu_count(torch)), 4
    rng = np.random.default_rng(9400 + groups)
    n = 256 * groups
    cap = n + 256
    s = torch.cuda.current_stream()
    a, _, T = seeded(torch, 9401, cap)
    b, _, _ = seeded(torch, 9401, cap)
    with a, b:
        L, doff, size, soff, ssize = _range_tables(rng, n, rounds, False, 5)
        soff[::3] = doff[::3] + np.uint64(16)
        src = rng.integers(0, 256, ssize, dtype=np.uint8)
        ts, tso, tdo, tl = T(src), T(soff.view(np.int64)), T(doff.view(np.int64)), T(L.view(np.int32))
        da = T(np.full(size, FILL, dtype=np.uint8))
        db = T(np.full(size, FILL, dtype=np.uint8))
        a.crypt_to_range_rounds(0, ts, tso, da, tdo, tl, n, rounds, stream=s)
        for r in range(rounds):
            w = slice(r * n, (r + 1) * n)
            b.crypt_to_range(0, ts, tso[w], db, tdo[w], tl[w], n, stream=s)
        a.sync(s)
        b.sync(s)
        assert_equal(da.cpu().numpy(), db.cpu().numpy(), "rounds call against successive calls")
        for x, y in zip(a.get_states(0, cap), b.get_states(0, cap)):
            assert (np.asarray(x) == np.asarray(y)).all()


# -- grouped: queued bytes in place, then three broadcasts -----------------------------

MSG = (100, 64, 37)        # the three broadcast messages' lengths


def _tick_case(rng, ids):
    """INTEGRATION.md 2e in one buffer (src == dst): entry i owns a run of
    queue + 100 + 64 + 37 bytes, guard bytes between the runs.  Round 0 crypts
    its queued bytes (a LENS length) in place; rounds 1-3 take the three shared
    messages, which lie behind all the runs, into the adjacent spans.  A third
    of the entries are outside the audience of each broadcast (length 0)."""
    n, rounds = ids.size, 4
    q = LENS[rng.integers(0, LENS.size, n)]
    run = q.astype(np.uint64) + np.uint64(sum(MSG))
    start, end = layout(run, 9)
    L = np.zeros((rounds, n), dtype=np.uint32)
    doff = np.zeros((rounds, n), dtype=np.uint64)
    soff = np.zeros((rounds, n), dtype=np.uint64)
    L[0], doff[0], soff[0] = q, start, start
    at = start + q.astype(np.uint64)
    mpos = end + 7
    for k, m in enumerate(MSG, start=1):
        L[k] = np.where(rng.random(n) < 2 / 3, m, 0)
        doff[k] = at                                      # adjacent to the span before it, audience or not
        soff[k] = mpos
        at = at + np.uint64(m)
        mpos += m + 3
    return L.reshape(-1), doff.reshape(-1), soff.reshape(-1), mpos + 16, end, rounds


@gpu
@pytest.mark.parametrize("declared", [False, True], ids=["undeclared", "declared"])
@pytest.mark.parametrize("nb", [2, 200])
def test_rounds_grouped_queue_then_broadcasts(built, torch_cuda, nb, declared):
    torch = torch_cuda
    rng = np.random.default_rng(9500 + nb + declared)
    G = nb + 8
    cap = 256 * G
    c, ob, T = seeded(torch, 9501 + nb, cap)
    s = torch.cuda.current_stream()
    with c:
        groups = rng.permutation(G)[:nb].astype(np.uint32)
        if nb > 2:
            groups[nb // 2] = IDLE_SLOT
        ids = buckets(rng, groups)
        ids[np.flatnonzero(ids != IDLE_SLOT)[::7]] = IDLE_SLOT             # idle slots inside busy buckets too
        busy = ids != IDLE_SLOT
        assert busy.any() and not busy.all()
        n = ids.size
        L, doff, soff, size, msgs_at, rounds = _tick_case(rng, ids)
        assert disjoint(doff, L) and int((doff + L).max()) <= msgs_at      # no destination reaches a message
        data = rng.integers(0, 256, size, dtype=np.uint8)                  # queued bytes, messages, and filler
        want = _want(ob, cap, data, ids, busy, data, soff, doff, L, rounds)
        buf = T(data)
        c.crypt_to_grouped_rounds(buf, T(soff.view(np.int64)), buf, T(doff.view(np.int64)), T(L.view(np.int32)),
                                  T(ids.view(np.int32)), n, rounds, bucket_group=groups if declared else None,
                                  stream=s)
        c.sync(s)
        got = buf.cpu().numpy()
        assert_equal(got, want, "queue in place, then three broadcasts")
        # (want outside the spans that ran is `data`: guards, idle entries' runs and the messages unchanged)
        assert_equal(got[msgs_at:], data[msgs_at:], "the broadcast sources changed")
        check_continues(torch, c, ob, T, cap, rng)


# -- faults and refusals -----------------------------------------------------------

def _grouped_tables(rng, n, rounds, shift):
    """Round-major tables of a grouped call in buffers of their own: a third of
    the entry-rounds read one shared message (a prefix each), a third are
    congruent with their destination, the rest lie anywhere."""
    L = _round_lengths(rng, n, rounds).reshape(-1)
    doff, size = layout(L, shift)
    soff, ssize = layout(L, 11, cycle=5)
    kind = rng.integers(0, 3, L.size)
    cong = kind == 1
    soff[cong] += (doff[cong] - soff[cong]) % np.uint64(16)        # (may run into the next source: allowed)
    shared = ssize + 5
    soff[kind == 0] = shared
    return L, doff, size, soff, shared + 300 + 16


@gpu
def test_rounds_grouped_id_out_of_range(built, torch_cuda):
    """One id >= capacity: skipped in every round, ZRC4_ERR_SLOT_RANGE from
    zrc4_sync, the rest of its bucket and every other bucket exact."""
    torch = torch_cuda
    nb, rounds = 33, 3
    rng = np.random.default_rng(9600)
    G = nb + 8
    cap = 256 * G
    c, ob, T = seeded(torch, 9601, cap)
    s = torch.cuda.current_stream()
    with c:
        groups = rng.permutation(G)[:nb].astype(np.uint32)
        ids = buckets(rng, groups)
        n = ids.size
        e = int(np.flatnonzero(ids[:256] == IDLE_SLOT)[0]) if (ids[:256] == IDLE_SLOT).any() else 0
        ids[e] = cap + 77
        L, doff, size, soff, ssize = _grouped_tables(rng, n, rounds, 4)
        L[e::n] = 193                                    # a span to keep in every round
        doff, size = layout(L, 4)
        assert disjoint(doff, L)
        ran = (ids != IDLE_SLOT) & (ids < cap)
        src = rng.integers(0, 256, ssize, dtype=np.uint8)
        slots = np.where(ran, ids, 0)
        want = _want(ob, cap, np.full(size, FILL, dtype=np.uint8), slots, ran, src, soff, doff, L, rounds)
        ts, td = T(src.copy()), T(np.full(size, FILL, dtype=np.uint8))
        c.crypt_to_grouped_rounds(ts, T(soff.view(np.int64)), td, T(doff.view(np.int64)), T(L.view(np.int32)),
                                  T(ids.view(np.int32)), n, rounds, bucket_group=groups, stream=s)
        with pytest.raises(ZRC4Error) as ei:
            c.sync(s)
        assert ei.value.code == -5                         # ZRC4_ERR_SLOT_RANGE
        got = td.cpu().numpy()
        for r in range(rounds):
            a = int(doff[r * n + e])
            assert (got[a: a + 193] == FILL).all(), r
        assert_equal(got, want, "id out of range")
        assert_equal(ts.cpu().numpy(), src, "id out of range: source changed")
        check_continues(torch, c, ob, T, cap, rng)


@gpu
@pytest.mark.parametrize("declared", [False, True], ids=["undeclared", "declared"])
def test_rounds_grouped_two_buckets_one_group(built, torch_cuda, declared):
    """Buckets 0 and 1 name the same group (disjoint slots of it), 2 buckets:
    ZRC4_ERR_GROUP; each of the group's halves goes to one bucket, ONCE for the
    whole call.  Which bucket wins is the hardware's choice, so the test reads
    it off the result: an entry's spans are exactly its crypt in EVERY round
    (its state advanced by all of them), or 0xA5 in every round."""
    torch = torch_cuda
    nb, rounds = 2, 3
    rng = np.random.default_rng(9700 + declared)
    G = nb + 8
    cap = 256 * G
    seed = 9701
    c, ob, T = seeded(torch, seed, cap)
    s = torch.cuda.current_stream()
    with c:
        g = 5
        groups = np.array([g, g], dtype=np.uint32)
        perm = rng.permutation(256)
        ids = np.full(512, IDLE_SLOT, dtype=np.uint32)
        ids[rng.permutation(256)[:100]] = g * 256 + perm[:100]
        ids[256 + rng.permutation(256)[:100]] = g * 256 + perm[100:200]
        n = ids.size
        L, doff, size, soff, ssize = _grouped_tables(rng, n, rounds, 2)
        L = np.maximum(L, 16)                            # long enough to tell crypted from untouched, in every round
        doff, size = layout(L, 2)
        soff, ssize = doff + np.uint64(32), size + 32
        soff[1::2] += np.uint64(5)
        assert disjoint(doff, L)
        src = rng.integers(0, 256, ssize, dtype=np.uint8)
        busy = ids != IDLE_SLOT
        slots = np.where(busy, ids, 0)
        blank = np.full(size, FILL, dtype=np.uint8)
        all_ran = _want(oracle(seed, cap)[0], cap, blank, slots, busy, src, soff, doff, L, rounds)
        ts, td = T(src.copy()), T(blank)
        c.crypt_to_grouped_rounds(ts, T(soff.view(np.int64)), td, T(doff.view(np.int64)), T(L.view(np.int32)),
                                  T(ids.view(np.int32)), n, rounds, bucket_group=groups if declared else None,
                                  stream=s)
        with pytest.raises(ZRC4Error) as ei:
            c.sync(s)
        assert ei.value.code == -7                         # ZRC4_ERR_GROUP
        got = td.cpu().numpy()
        ran = busy.copy()
        for e in np.flatnonzero(busy):
            spans = [(int(doff[r * n + e]), int(doff[r * n + e]) + int(L[r * n + e])) for r in range(rounds)]
            if all((got[a:z] == all_ran[a:z]).all() for a, z in spans):
                continue
            ran[e] = False
            assert all((got[a:z] == FILL).all() for a, z in spans), (e, [got[a:a + 8] for a, _ in spans])
        assert not ran[busy].all()                       # somebody was refused
        want = _want(ob, cap, blank, slots, ran, src, soff, doff, L, rounds)
        assert_equal(got, want, "two buckets, one group")
        assert_equal(ts.cpu().numpy(), src, "refusal: source changed")
        check_continues(torch, c, ob, T, cap, rng)        # (states: the oracle ran exactly the slots that ran)


# -- pinned host memory ----------------------------------------------------------------

@gpu
@pytest.mark.parametrize("where", ["src_pinned", "dst_pinned"])
def test_rounds_pinned_host(built, torch_cuda, where):
    torch = torch_cuda
    rng = np.random.default_rng(9800)
    n, rounds = 256, 3
    cap = n + 256
    c, ob, T = seeded(torch, 9801, cap)
    P = lambda a: torch.from_numpy(np.ascontiguousarray(a)).pin_memory()
    with c:
        L, doff, size, soff, ssize = _range_tables(rng, n, rounds, False, 9)
        soff[::2] = doff[::2] + np.uint64(16)
        src = rng.integers(0, 256, ssize, dtype=np.uint8)
        _run_range(torch, c, ob, T, cap, 0, n, rounds, src, soff, doff, L, size, where,
                   Tsrc=P if where == "src_pinned" else None, Tdst=P if where == "dst_pinned" else None)
        check_continues(torch, c, ob, T, cap, rng)


# -- seeded sweep ----------------------------------------------------------------------

@gpu
def test_rounds_random_sweep(built, torch_cuda):
    """10 seeded calls on one context, the oracle carried across them; valid
    buckets only, so every busy entry runs."""
    torch = torch_cuda
    rng = np.random.default_rng(9999)
    cap = SWEEP_GROUPS * 256
    c, ob, T = seeded(torch, 9998, cap)
    s = torch.cuda.current_stream()
    with c:
        for call in range(SWEEP_CALLS):
            ids, groups, rounds, L, doff, size, soff, ssize = sweep_call(rng)
            n = ids.size
            assert disjoint(doff, L)
            busy = ids != IDLE_SLOT
            src = rng.integers(0, 256, ssize, dtype=np.uint8)
            blank = np.full(size, FILL, dtype=np.uint8)
            want = _want(ob, cap, blank, np.where(busy, ids, 0), busy, src, soff, doff, L, rounds)
            ts, td = T(src.copy()), T(blank)
            c.crypt_to_grouped_rounds(ts, T(soff.view(np.int64)), td, T(doff.view(np.int64)), T(L.view(np.int32)),
                                      T(ids.view(np.int32)), n, rounds, bucket_group=groups if call % 2 else None,
                                      stream=s)
            c.sync(s)
            what = f"sweep call {call} ({n // 256} buckets x {rounds} rounds)"
            assert_equal(td.cpu().numpy(), want, what)
            assert_equal(ts.cpu().numpy(), src, what + ": source changed")
            check_states(c, ob, cap)
        check_continues(torch, c, ob, T, cap, rng)
