"""GPU parity of the write-only keystream calls (include/zrc4.h:
zrc4_keystream_range, zrc4_keystream_grouped): entry i STORES the next len[i]
keystream bytes of its slot and never reads the destination.  RC4's keystream
is what RC4Encryption::encryption (depends/rc4/rc4_encryption.h:74-93) XORs
into the data, so the oracle is pyoracle.Batch: KSA, then `crypt` over zeros.

Every output buffer is pre-filled with 0xA5 and spans are separated by 1-3
guard bytes.  Every case checks that the spans equal the oracle keystream,
that every other byte is still 0xA5, that every state of the context equals
the oracle's, and that a following crypt_range over random plaintext continues
each stream bit-exactly.

Kernel paths on 256 CUs: 1 / 32 groups the window kernel, 33 / 128 the
half-group kernel, 129 / 256 the whole-group kernel, 257 the persistent kernel
behind the span fill; first_slot = 3 the gather path; grouped 2 / 33 / 200 /
300 buckets the same four, declared (groups in the kernel arguments up to 256
buckets) and undeclared."""
import numpy as np
import pytest

from gpu_support import FILL, LONG, SHORT, assert_equal, buckets, check_continues, layout, seeded, span_index
from gpu_support import torch_cuda  # noqa: F401
from zsummerx_amd import ZRC4Error
from zsummerx_amd._capi import IDLE_SLOT

pytestmark = pytest.mark.gpu


def _want(ob, cap, size, slots, off, L, base=None):
    """The expected buffer: `base` (default 0xA5 everywhere) with the oracle
    keystream of slot slots[i] in span i, the oracle advanced."""
    want = np.full(size, FILL, dtype=np.uint8) if base is None else base.copy()
    want[span_index(off, L)] = 0
    so = np.zeros(cap, dtype=np.uint64)
    sl = np.zeros(cap, dtype=np.uint32)
    so[slots] = off
    sl[slots] = L
    ob.crypt(want, so, sl)
    return want


# -- range ---------------------------------------------------------------------

@pytest.mark.parametrize("groups", [1, 32, 33, 128, 129, 256, 257])
def test_keystream_range_whole_groups(built, torch_cuda, groups):
    torch = torch_cuda
    rng = np.random.default_rng(4100 + groups)
    lens = LONG if groups <= 32 else SHORT
    n = 256 * groups
    cap = n + 256                                        # one group the call does not touch
    c, ob, T = seeded(torch, 5100 + groups, cap)
    s = torch.cuda.current_stream()
    with c:
        L = lens[np.arange(n) % lens.size]
        off, size = layout(L, groups % 16)
        # every length of the list meets every start misalignment
        pairs = set(zip((np.arange(n) % lens.size).tolist(), (off % 16).tolist()))
        assert len(pairs) == 16 * lens.size or n < 16 * lens.size, len(pairs)
        want = _want(ob, cap, size, np.arange(n), off, L)
        out = T(np.full(size, FILL, dtype=np.uint8))
        c.keystream_range(0, out, T(off.view(np.int64)), T(L.view(np.int32)), stream=s)
        c.sync(s)
        assert_equal(out.cpu().numpy(), want, "keystream_range")
        check_continues(torch, c, ob, T, cap, rng)


def test_keystream_range_unaligned_first_slot(built, torch_cuda):
    """first_slot = 3, n = 700: three workgroups on the gather path (a slot's
    S-box column by column), slots 0-2 and 703.. untouched."""
    torch = torch_cuda
    rng = np.random.default_rng(4400)
    first, n, cap = 3, 700, 1024
    c, ob, T = seeded(torch, 5400, cap)
    s = torch.cuda.current_stream()
    with c:
        L = SHORT[np.arange(n) % SHORT.size]
        off, size = layout(L, 7)
        want = _want(ob, cap, size, first + np.arange(n), off, L)
        out = T(np.full(size, FILL, dtype=np.uint8))
        c.keystream_range(first, out, T(off.view(np.int64)), T(L.view(np.int32)), stream=s)
        c.sync(s)
        assert_equal(out.cpu().numpy(), want, "keystream_range first_slot=3")
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
    off, size = layout(L, nb % 16)
    return groups, ids, L, off, size


@pytest.mark.parametrize("declared", [False, True], ids=["undeclared", "declared"])
@pytest.mark.parametrize("nb", [2, 33, 200, 300])
def test_keystream_grouped(built, torch_cuda, nb, declared):
    torch = torch_cuda
    rng = np.random.default_rng(4600 + nb + declared)
    G = nb + 8
    cap = 256 * G
    c, ob, T = seeded(torch, 5600 + nb, cap)
    s = torch.cuda.current_stream()
    with c:
        groups, ids, L, off, size = _grouped_case(rng, nb, G)
        busy = ids != IDLE_SLOT
        assert (L[busy] == 0).any() and (L[~busy] != 0).any()
        want = _want(ob, cap, size, ids[busy], off[busy], L[busy])
        out = T(np.full(size, FILL, dtype=np.uint8))
        c.keystream_grouped(out, T(off.view(np.int64)), T(L.view(np.int32)), T(ids.view(np.int32)),
                            groups if declared else None, stream=s)
        c.sync(s)
        assert_equal(out.cpu().numpy(), want, "keystream_grouped")
        check_continues(torch, c, ob, T, cap, rng)


def _refused_spans_then_mask(got, off, L, entries):
    """A refused bucket's spans are unspecified: each untouched or zero.
    Checked, then put back to 0xA5 for the whole-buffer comparison."""
    for e in entries:
        sp = got[int(off[e]): int(off[e]) + int(L[e])]
        assert (sp == FILL).all() or (sp == 0).all(), (e, sp[:16])
        sp[:] = FILL


@pytest.mark.parametrize("declared", [False, True], ids=["undeclared", "declared"])
@pytest.mark.parametrize("nb", [2, 200])
def test_keystream_grouped_mixed_bucket_is_refused(built, torch_cuda, nb, declared):
    """Bucket 1 names two groups (its own and H, which no bucket holds):
    ZRC4_ERR_GROUP, its slots keep their states, every other bucket is exact."""
    torch = torch_cuda
    rng = np.random.default_rng(4800 + nb + declared)
    G = nb + 8
    cap = 256 * G
    c, ob, T = seeded(torch, 5800 + nb, cap)
    s = torch.cuda.current_stream()
    with c:
        groups, ids, L, off, size = _grouped_case(rng, nb, G, idle_bucket=False)
        H = int(np.setdiff1d(np.arange(G), groups)[0])
        e = 256 + int(np.flatnonzero(ids[256:512] != IDLE_SLOT)[0])
        ids[e] = H * 256 + 5
        L[256:512] = np.maximum(L[256:512], 1)           # every entry of the refused bucket has bytes to show
        off, size = layout(L, nb % 16)
        ran = ids != IDLE_SLOT
        ran[256:512] = False
        want = _want(ob, cap, size, ids[ran], off[ran], L[ran])
        out = T(np.full(size, FILL, dtype=np.uint8))
        c.keystream_grouped(out, T(off.view(np.int64)), T(L.view(np.int32)), T(ids.view(np.int32)),
                            groups if declared else None, stream=s)
        with pytest.raises(ZRC4Error) as ei:
            c.sync(s)
        assert ei.value.code == -7                         # ZRC4_ERR_GROUP
        got = out.cpu().numpy()
        _refused_spans_then_mask(got, off, L, 256 + np.flatnonzero(ids[256:512] != IDLE_SLOT))
        assert_equal(got, want, "mixed bucket")
        check_continues(torch, c, ob, T, cap, rng)        # (states: the oracle skipped bucket 1's slots)


@pytest.mark.parametrize("nb", [2, 200])
def test_keystream_grouped_id_out_of_range(built, torch_cuda, nb):
    """One id >= capacity: ZRC4_ERR_SLOT_RANGE, its span still 0xA5, the rest
    of its bucket (and every other bucket) exact."""
    torch = torch_cuda
    rng = np.random.default_rng(4900 + nb)
    G = nb + 8
    cap = 256 * G
    c, ob, T = seeded(torch, 5900 + nb, cap)
    s = torch.cuda.current_stream()
    with c:
        groups, ids, L, off, size = _grouped_case(rng, nb, G, idle_bucket=False)
        e = int(np.flatnonzero(ids[:256] == IDLE_SLOT)[0]) if (ids[:256] == IDLE_SLOT).any() else 0
        ids[e] = cap + 77
        L[e] = 193
        off, size = layout(L, nb % 16)
        ran = (ids != IDLE_SLOT) & (ids < cap)
        want = _want(ob, cap, size, ids[ran], off[ran], L[ran])
        out = T(np.full(size, FILL, dtype=np.uint8))
        c.keystream_grouped(out, T(off.view(np.int64)), T(L.view(np.int32)), T(ids.view(np.int32)), groups, stream=s)
        with pytest.raises(ZRC4Error) as ei:
            c.sync(s)
        assert ei.value.code == -5                         # ZRC4_ERR_SLOT_RANGE
        got = out.cpu().numpy()
        assert (got[int(off[e]): int(off[e]) + 193] == FILL).all()
        assert_equal(got, want, "id out of range")
        check_continues(torch, c, ob, T, cap, rng)


# -- the destination is never read -----------------------------------------------

@pytest.mark.parametrize("kind,count", [("range", 1), ("range", 33), ("range", 200), ("range", 257),
                                        ("grouped", 20), ("grouped", 200)])
def test_destination_is_never_read(built, torch_cuda, kind, count):
    """The same call on two fresh, identically seeded contexts, `out`
    pre-filled once with zeros and once with random bytes: identical spans
    (the oracle's), and every other byte keeps its pre-fill."""
    torch = torch_cuda
    rng = np.random.default_rng(5000 + count)
    G = count + 8
    cap = 256 * G
    if kind == "range":
        ids = np.arange(256 * count, dtype=np.uint32)
        L = SHORT[np.arange(ids.size) % SHORT.size]
        off, size = layout(L, 5)
        groups = None
    else:
        groups, ids, L, off, size = _grouped_case(rng, count, G)
    busy = ids != IDLE_SLOT
    fills = [np.zeros(size, dtype=np.uint8), rng.integers(0, 256, size, dtype=np.uint8)]
    spans = []
    s = torch.cuda.current_stream()
    for fill in fills:
        c, ob, T = seeded(torch, 6000 + count, cap)
        with c:
            want = _want(ob, cap, size, ids[busy], off[busy], L[busy], base=fill)
            out = T(fill)
            if kind == "range":
                c.keystream_range(0, out, T(off.view(np.int64)), T(L.view(np.int32)), stream=s)
            else:
                c.keystream_grouped(out, T(off.view(np.int64)), T(L.view(np.int32)), T(ids.view(np.int32)), groups,
                                    stream=s)
            c.sync(s)
            got = out.cpu().numpy()
            assert_equal(got, want, "pre-filled destination")
            spans.append(got[span_index(off[busy], L[busy])])
    assert (spans[0] == spans[1]).all()
