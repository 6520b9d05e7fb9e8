"""GPU coverage of out-of-place entries whose source and destination are NOT
congruent mod 16 (include/zrc4.h: zrc4_crypt_to_*; csrc/zrc4_kernels.hpp:
crypt_message, span_copy_kernel): the lane-per-stream kernels walk them like
congruent ones -- head bytes up to the destination's 16-byte boundary, 64-byte
blocks, 16-byte pieces, tail bytes -- with aligned 16-byte stores fed by 16-byte
loads at unaligned source addresses.

Layout inside every group or bucket: entry e has destination alignment e mod 16
and (source - destination) mod 16 = (e / 16) mod 15 + 1, so one launch holds
all 240 pairs of alignments; lengths cycle through LENS (no block, one block,
two blocks for the loop's next-block path, every piece and tail count; 17 is
coprime to 256, so over 17 groups every entry position meets every length).
Every source byte outside the spans and every destination byte outside them is
a guard: sources must come back unchanged, destinations still 0xA5.

Launches on 256 CUs: range 33 groups (half-group kernel), 129 (whole-group),
257 (span_copy_kernel, then the persistent kernel in place); grouped 33 and 200
buckets, declared and not; the rounds forms at 33 with 3 rounds.  Sources:
distinct, one shared message, prefixes of one message; source or destination
in pinned host memory; one launch per family mixes non-congruent, congruent
and identical-address (in place) entries.

Each case checks the destination spans, the guards, the source, every state,
and a following crypt_range against the oracle.  The byte-by-byte path these
entries took before computes the same bytes: the tests cover the walk, they do
not tell the two apart."""
import numpy as np
import pytest

from gpu_support import FILL, assert_equal, check_continues, host, seeded, span_index
from gpu_support import torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

LENS = np.array([1, 15, 16, 17, 63, 64, 65, 79, 80, 127, 128, 129, 143, 191, 192, 193, 300], dtype=np.uint32)


def aligned_layout(L, align, start=0):
    """Spans in entry order with at least one guard byte between them, span i
    starting at an address congruent to align[i] mod 16."""
    off = np.empty(L.size, dtype=np.uint64)
    cur = start
    for i in range(L.size):
        cur += 1
        cur += (int(align[i]) - cur) % 16
        off[i] = cur
        cur += int(L[i])
    return off, cur + 32


def pairs_layout(n):
    """Lengths, destination offsets and the wanted (src - dst) mod 16 of n
    entries, entry e of each 256 laid out as the module text says."""
    e = np.arange(n) % 256
    L = LENS[np.arange(n) % LENS.size]
    doff, size = aligned_layout(L, e % 16)
    delta = (e // 16) % 15 + 1
    assert len(set(zip((doff % 16).tolist(), delta.tolist()))) == 240 or n < 256
    return L, doff, size, delta


def make_sources(kind, L, doff, delta):
    """Source offsets and buffer size: distinct spans at the wanted deltas, one
    shared message (`broadcast`, every entry its whole length: lengths are made
    equal by the caller) or prefixes of one message."""
    if kind == "distinct":
        soff, ssize = aligned_layout(L, (doff + delta.astype(np.uint64)) % np.uint64(16), start=5)
        assert (((soff - doff) % np.uint64(16)) == delta).all()
        return soff, ssize
    soff = np.full(L.size, 37, dtype=np.uint64)             # 37: non-congruent with 15 of the 16 destination alignments
    return soff, 37 + int(L.max()) + 11


def want_of(ob, cap, base, slots, src, soff, doff, L):
    want = base.copy()
    live = L > 0
    want[span_index(doff[live], L[live])] = src[span_index(soff[live], L[live])]
    so = np.zeros(cap, dtype=np.uint64)
    sl = np.zeros(cap, dtype=np.uint32)
    so[slots] = doff
    sl[slots] = L
    ob.crypt(want, so, sl)
    return want


def i64(T, a):
    return T(a.view(np.int64))


def i32(T, a):
    return T(a.view(np.int32))


def pinned(torch):
    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).pin_memory()


# -- range -----------------------------------------------------------------------

@pytest.mark.parametrize("groups,kind,where", [
    (33, "distinct", "device"), (129, "distinct", "device"), (257, "distinct", "device"),
    (33, "broadcast", "device"), (129, "prefix", "device"), (257, "prefix", "device"),
    (33, "distinct", "src_pinned"), (129, "distinct", "dst_pinned"), (129, "broadcast", "dst_pinned"),
], ids=lambda v: str(v))
def test_crypt_to_range_all_alignment_pairs(built, torch_cuda, groups, kind, where):
    torch = torch_cuda
    rng = np.random.default_rng(9100 + groups)
    n = 256 * groups
    cap = n + 256
    c, ob, T = seeded(torch, 9200 + groups, cap)
    s = torch.cuda.current_stream()
    with c:
        L, doff, size, delta = pairs_layout(n)
        if kind == "broadcast":
            L = np.full(n, 300, dtype=np.uint32)
            doff, size = aligned_layout(L, np.arange(n) % 16)
        soff, ssize = make_sources(kind, L, doff, delta)
        src = rng.integers(0, 256, ssize, dtype=np.uint8)
        want = want_of(ob, cap, np.full(size, FILL, dtype=np.uint8), np.arange(n), src, soff, doff, L)
        ts = (pinned(torch) if where == "src_pinned" else T)(src.copy())
        td = (pinned(torch) if where == "dst_pinned" else T)(np.full(size, FILL, dtype=np.uint8))
        c.crypt_to_range(0, ts, i64(T, soff), td, i64(T, doff), i32(T, L), stream=s)
        c.sync(s)
        assert_equal(host(td), want, f"crypt_to_range {groups} groups, {kind}, {where}")
        assert_equal(host(ts), src, "source changed")
        check_continues(torch, c, ob, T, cap, rng)


# -- grouped ---------------------------------------------------------------------

def full_buckets(rng, nb, G):
    """nb buckets of distinct groups, every entry busy, slots shuffled."""
    groups = rng.permutation(G)[:nb].astype(np.uint32)
    ids = np.concatenate([g * 256 + rng.permutation(256) for g in groups.astype(np.int64)]).astype(np.uint32)
    return groups, ids


@pytest.mark.parametrize("declared", [False, True], ids=["undeclared", "declared"])
@pytest.mark.parametrize("nb", [33, 200])
def test_crypt_to_grouped_all_alignment_pairs(built, torch_cuda, nb, declared):
    torch = torch_cuda
    rng = np.random.default_rng(9300 + nb + declared)
    G = nb + 4
    cap = 256 * G
    c, ob, T = seeded(torch, 9400 + nb, cap)
    s = torch.cuda.current_stream()
    with c:
        groups, ids = full_buckets(rng, nb, G)
        L, doff, size, delta = pairs_layout(ids.size)
        soff, ssize = make_sources("distinct", L, doff, delta)
        src = rng.integers(0, 256, ssize, dtype=np.uint8)
        want = want_of(ob, cap, np.full(size, FILL, dtype=np.uint8), ids, src, soff, doff, L)
        ts, td = T(src.copy()), T(np.full(size, FILL, dtype=np.uint8))
        c.crypt_to_grouped(ts, i64(T, soff), td, i64(T, doff), i32(T, L), i32(T, ids),
                           groups if declared else None, stream=s)
        c.sync(s)
        assert_equal(host(td), want, f"crypt_to_grouped {nb} buckets")
        assert_equal(host(ts), src, "source changed")
        check_continues(torch, c, ob, T, cap, rng)


# -- rounds ----------------------------------------------------------------------

ROUNDS = 3


def rounds_tables(n, kind):
    """Round-major tables: round r shifts the entry pattern by 5 * r positions
    (other alignment pairs and lengths per slot in every round), destinations
    of all rounds disjoint, sources distinct or one message's prefixes."""
    Ls, ds, ss = [], [], []
    dcur, scur = 0, 5
    for r in range(ROUNDS):
        e = (np.arange(n) + 5 * r) % 256
        L = LENS[(np.arange(n) + 5 * r) % LENS.size]
        doff, dcur = aligned_layout(L, e % 16, start=dcur)
        delta = ((e // 16) % 15 + 1).astype(np.uint64)
        if kind == "distinct":
            soff, scur = aligned_layout(L, (doff + delta) % np.uint64(16), start=scur)
        else:
            soff = np.full(n, 37, dtype=np.uint64)
            scur = 37 + 300 + 11
        Ls.append(L), ds.append(doff), ss.append(soff)
    return np.concatenate(Ls), np.concatenate(ds), dcur, np.concatenate(ss), scur


@pytest.mark.parametrize("kind", ["distinct", "prefix"])
@pytest.mark.parametrize("form", ["range", "grouped", "declared"])
def test_crypt_to_rounds_all_alignment_pairs(built, torch_cuda, form, kind):
    torch = torch_cuda
    rng = np.random.default_rng(9500)
    nb = 33
    G = nb + 3
    cap = 256 * G
    c, ob, T = seeded(torch, 9600, cap)
    s = torch.cuda.current_stream()
    with c:
        if form == "range":
            groups, ids = None, np.arange(256 * nb, dtype=np.uint32)
        else:
            groups, ids = full_buckets(rng, nb, G)
        n = ids.size
        L, doff, size, soff, ssize = rounds_tables(n, kind)
        src = rng.integers(0, 256, ssize, dtype=np.uint8)
        want = np.full(size, FILL, dtype=np.uint8)
        for r in range(ROUNDS):
            q = slice(r * n, (r + 1) * n)
            want = want_of(ob, cap, want, ids, src, soff[q], doff[q], L[q])
        ts, td = T(src.copy()), T(np.full(size, FILL, dtype=np.uint8))
        if form == "range":
            c.crypt_to_range_rounds(0, ts, i64(T, soff), td, i64(T, doff), i32(T, L), n, ROUNDS, stream=s)
        else:
            c.crypt_to_grouped_rounds(ts, i64(T, soff), td, i64(T, doff), i32(T, L), i32(T, ids), n, ROUNDS,
                                      groups if form == "declared" else None, stream=s)
        c.sync(s)
        assert_equal(host(td), want, f"rounds, {form}, {kind}")
        assert_equal(host(ts), src, "source changed")
        check_continues(torch, c, ob, T, cap, rng)


# -- non-congruent, congruent and in-place entries in one launch -----------------------

@pytest.mark.parametrize("family", ["range-33", "range-129", "range-257", "declared-33", "rounds-33"])
def test_crypt_to_mixed_entries(built, torch_cuda, family):
    """One buffer is source and destination: entry i with i % 5 == 0 is in place
    (identical addresses), i % 3 == 0 congruent, the others at the wanted
    nonzero delta; sources lie behind the destination region."""
    torch = torch_cuda
    form, groups = family.split("-")
    groups = int(groups)
    rng = np.random.default_rng(9700 + groups)
    n = 256 * groups
    cap = n + 256
    c, ob, T = seeded(torch, 9800 + groups, cap)
    s = torch.cuda.current_stream()
    with c:
        L, doff, dsize, delta = pairs_layout(n)
        i = np.arange(n)
        delta = np.where(i % 3 == 0, 0, delta)
        soff, size = aligned_layout(L, (doff + delta.astype(np.uint64)) % np.uint64(16), start=dsize)
        inplace = i % 5 == 0
        soff[inplace] = doff[inplace]
        data = rng.integers(0, 256, size, dtype=np.uint8)
        data[:dsize] = FILL
        data[span_index(doff[inplace], L[inplace])] = rng.integers(0, 256, int(L[inplace].sum()), dtype=np.uint8)
        ids = np.arange(n, dtype=np.uint32)
        want = want_of(ob, cap, data, ids, data, soff, doff, L)
        buf = T(data.copy())
        if form == "range":
            c.crypt_to_range(0, buf, i64(T, soff), buf, i64(T, doff), i32(T, L), stream=s)
        elif form == "declared":
            c.crypt_to_grouped(buf, i64(T, soff), buf, i64(T, doff), i32(T, L), i32(T, ids),
                               np.arange(groups, dtype=np.uint32), stream=s)
        else:                                            # one round of work and an empty round behind it
            z = np.zeros(n, dtype=np.uint32)
            c.crypt_to_range_rounds(0, buf, i64(T, np.concatenate((soff, soff))), buf,
                                    i64(T, np.concatenate((doff, doff))), i32(T, np.concatenate((L, z))), n, 2,
                                    stream=s)
        c.sync(s)
        # (the sources behind the destination region are part of `want`: unchanged)
        assert_equal(host(buf), want, f"mixed entries, {family}")
        check_continues(torch, c, ob, T, cap, rng)
