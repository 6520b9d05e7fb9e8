"""GPU tests of the bulk state calls (zrc4_export_states, zrc4_import_states,
zrc4_copy_states, zrc4_set_states): every case is exact byte equality against
the oracle's states, with Context.get_states (host transposition, written
independently of the kernels) as a second check where it applies.

Contexts have 1 536 slots (6 groups); slot i is seeded with its own 1-40 byte
key and advanced by (7 i) % 301 bytes, the oracle batch alike.  Output buffers
are pre-filled with 0xA5 and carry one guard record behind them.

The issue's "swap of two 150-slot sets inside one group" cannot be built: a
group has 256 slots, two disjoint sets of 150 need 300.  The in-group swap
here exchanges the two largest disjoint sets a group holds (128 and 128, all
256 slots of group 3); the swap across groups uses two 150-slot sets."""
import ctypes as C

import numpy as np
import pytest

import pyoracle
from gpu_support import torch_cuda  # noqa: F401
from zsummerx_amd import Context, ZRC4Error
from zsummerx_amd._capi import IDLE_SLOT

pytestmark = pytest.mark.gpu

N = 1536
FILL = 0xA5


class World:
    """Keys, advances and the oracle's states of N streams (never modified)."""

    def __init__(self, seed, mul, mod):
        rng = np.random.default_rng(seed)
        self.klen = rng.integers(1, 41, N).astype(np.uint32)
        self.koff = np.concatenate([[0], np.cumsum(self.klen[:-1])]).astype(np.uint64)
        self.keys = rng.integers(0, 256, int(self.klen.sum()), dtype=np.uint8)
        self.adv = ((mul * np.arange(N)) % mod).astype(np.uint32)
        self.aoff = np.concatenate([[0], np.cumsum(self.adv[:-1])]).astype(np.uint64)
        ob = pyoracle.Batch(N)
        ob.make_sbox(self.keys, self.koff, self.klen)
        ob.crypt(np.zeros(int(self.adv.sum()) + 1, dtype=np.uint8), self.aoff, self.adv)
        self.sb, self.x, self.y = (a.copy() for a in ob.states())
        self.xy = self.x.astype(np.uint16) | (self.y.astype(np.uint16) << 8)
        for a in (self.sb, self.x, self.y, self.xy):
            a.setflags(write=False)


@pytest.fixture(scope="module")
def wa():
    return World(11, 7, 301)


@pytest.fixture(scope="module")
def wb():
    return World(12, 11, 257)


def T(torch, a):
    a = np.array(a, copy=True, order="C")
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    elif a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).cuda()


def seeded(torch, w):
    c = Context(0, N)
    s = torch.cuda.current_stream()
    c.ksa_range(0, T(torch, w.klen), T(torch, w.koff), T(torch, w.keys), stream=s)
    c.crypt_range(0, torch.zeros(int(w.adv.sum()) + 1, dtype=torch.uint8, device="cuda"), T(torch, w.aoff),
                  T(torch, w.adv), stream=s)
    c.sync(s)
    return c


@pytest.fixture(scope="module")
def ctx_a(built, torch_cuda, wa):
    """World A on the device; the export tests only read it."""
    c = seeded(torch_cuda, wa)
    yield c
    c.close()


def out_bufs(torch, n):
    """Record buffers for n entries plus one guard record, filled with 0xA5."""
    sb = torch.full((n + 1, 256), FILL, dtype=torch.uint8, device="cuda")
    xy = torch.full((n + 1,), FILL * 257 - 65536, dtype=torch.int16, device="cuda")
    return sb, xy


def host(sb, xy):
    return sb.cpu().numpy(), xy.cpu().numpy().view(np.uint16)


def check_records(sb, xy, w, slots):
    """Entry i holds slot slots[i] of world w; entries with slots[i] < 0 and
    the guard record behind the last entry keep the fill."""
    sbh, xyh = host(sb, xy)
    slots = np.asarray(slots, dtype=np.int64)
    want_sb = np.full(sbh.shape, FILL, dtype=np.uint8)
    want_xy = np.full(xyh.shape, FILL * 257, dtype=np.uint16)
    live = np.flatnonzero(slots >= 0)
    want_sb[live] = w.sb[slots[live]]
    want_xy[live] = w.xy[slots[live]]
    assert np.array_equal(sbh, want_sb)
    assert np.array_equal(xyh, want_xy)


def check_context(c, sb, x, y):
    got_sb, got_x, got_y = c.get_states(0, N)
    assert np.array_equal(got_sb, sb)
    assert np.array_equal(got_x, x)
    assert np.array_equal(got_y, y)


def oracle_from(sb, x, y):
    n = len(x)
    ob = pyoracle.Batch(n)
    for i in range(n):
        pyoracle.lib().oracle_state_from_bytes(C.byref(ob.st[i]), C.c_void_p(np.ascontiguousarray(sb[i]).ctypes.data),
                                               int(x[i]), int(y[i]))
    return ob


def crypt_all_and_check(torch, c, sb, x, y, length=64, stream=None):
    """crypt_range `length` bytes on every slot of c: ciphertext and final
    states equal the oracle continuing from (sb, x, y)."""
    s = stream if stream is not None else torch.cuda.current_stream()
    rng = np.random.default_rng(5)
    pay = rng.integers(0, 256, N * length, dtype=np.uint8)
    off = (np.arange(N) * length).astype(np.uint64)
    ln = np.full(N, length, dtype=np.uint32)
    d = T(torch, pay)
    c.crypt_range(0, d, T(torch, off), T(torch, ln), stream=s)
    c.sync(s)
    ob = oracle_from(sb, x, y)
    want = pay.copy()
    ob.crypt(want, off, ln)
    assert np.array_equal(d.cpu().numpy(), want)
    check_context(c, *ob.states())


# ------------------------------------------------------------- 1. export, range
@pytest.mark.parametrize("first,n", [(0, 1536), (0, 1), (255, 2), (3, 509), (256, 256), (1535, 1), (0, 0)])
def test_export_range(ctx_a, torch_cuda, wa, first, n):
    sb, xy = out_bufs(torch_cuda, n)
    ctx_a.export_states(sb, xy, first_slot=first, n=n)
    ctx_a.sync()
    check_records(sb, xy, wa, list(range(first, first + n)) + [-1])
    got_sb, got_x, got_y = ctx_a.get_states(first, n) if n else (wa.sb[:0], wa.x[:0], wa.y[:0])
    sbh, xyh = host(sb, xy)
    assert np.array_equal(sbh[:n], got_sb)
    assert np.array_equal(xyh[:n], got_x.astype(np.uint16) | (got_y.astype(np.uint16) << 8))


# --------------------------------------------------------------- 2. export, ids
def _ids_cases():
    rng = np.random.default_rng(21)
    cases = {}
    cases["all_permuted"] = rng.permutation(N)
    cases["group_buckets_reversed"] = np.concatenate([g * 256 + rng.permutation(256) for g in range(5, -1, -1)])
    c = np.full(256, IDLE_SLOT, dtype=np.int64)
    c[rng.permutation(256)[:200]] = 2 * 256 + rng.permutation(256)[:200]
    cases["200_of_group2_56_idle"] = c
    cases["257_group1_plus_one_of_group4"] = np.concatenate([256 + rng.permutation(256), [4 * 256 + 77]])
    c = np.full(256, IDLE_SLOT, dtype=np.int64)
    c[100] = 777
    cases["single_busy"] = c
    return cases


IDS_CASES = _ids_cases()


@pytest.mark.parametrize("name", list(IDS_CASES))
def test_export_ids(ctx_a, torch_cuda, wa, name):
    ids = IDS_CASES[name]
    sb, xy = out_bufs(torch_cuda, len(ids))
    ctx_a.export_states(sb, xy, ids=T(torch_cuda, ids.astype(np.uint32)))
    ctx_a.sync()
    check_records(sb, xy, wa, [int(i) if i != IDLE_SLOT else -1 for i in ids] + [-1])


def test_export_ids_out_of_range(ctx_a, torch_cuda, wa):
    ids = np.random.default_rng(22).permutation(N).astype(np.int64)
    ids[700] = ctx_a.capacity + 5
    sb, xy = out_bufs(torch_cuda, N)
    ctx_a.export_states(sb, xy, ids=T(torch_cuda, ids.astype(np.uint32)))
    with pytest.raises(ZRC4Error) as ei:
        ctx_a.sync()
    assert ei.value.code == -5
    ctx_a.sync()                                  # the latch is cleared
    slots = [int(i) for i in ids] + [-1]
    slots[700] = -1
    check_records(sb, xy, wa, slots)


# -------------------------------------------------------------------- 3. import
def test_import_range(built, torch_cuda, wa, wb):
    torch = torch_cuda
    with seeded(torch, wa) as c:
        c.import_states(T(torch, wb.sb[:509]), T(torch, wb.xy[:509]), first_slot=3, n=509)
        c.sync()
        sb, x, y = wa.sb.copy(), wa.x.copy(), wa.y.copy()
        sb[3:512], x[3:512], y[3:512] = wb.sb[:509], wb.x[:509], wb.y[:509]
        check_context(c, sb, x, y)                # slots 0-2 and 512-1535 unchanged
        crypt_all_and_check(torch, c, sb, x, y)


def test_import_ids(built, torch_cuda, wa, wb):
    torch = torch_cuda
    rng = np.random.default_rng(23)
    ids = rng.permutation(N)[:300].astype(np.int64)
    idle = rng.permutation(300)[:11]
    ids[idle] = IDLE_SLOT
    with seeded(torch, wa) as c:
        c.import_states(T(torch, wb.sb[:300]), T(torch, wb.xy[:300]), ids=T(torch, ids.astype(np.uint32)))
        c.sync()
        sb, x, y = wa.sb.copy(), wa.x.copy(), wa.y.copy()
        live = np.flatnonzero(ids != IDLE_SLOT)
        sb[ids[live]], x[ids[live]], y[ids[live]] = wb.sb[live], wb.x[live], wb.y[live]
        check_context(c, sb, x, y)                # every unnamed slot unchanged
        crypt_all_and_check(torch, c, sb, x, y)


# ---------------------------------------------------------------- 4. round trip
def test_round_trip(ctx_a, torch_cuda, wa):
    torch = torch_cuda
    sb1, xy1 = out_bufs(torch, N)
    ctx_a.export_states(sb1, xy1, first_slot=0, n=N)
    ctx_a.sync()
    with Context(0, N) as b:
        b.import_states(sb1, xy1, first_slot=0, n=N)
        sb2, xy2 = out_bufs(torch, N)
        b.export_states(sb2, xy2, first_slot=0, n=N)
        b.sync()
        assert torch.equal(sb1, sb2) and torch.equal(xy1, xy2)
        check_context(b, wa.sb, wa.x, wa.y)


# ---------------------------------------------------------------------- 5. copy
def test_copy_overlapping_range_reads_before_it_writes(built, torch_cuda, wa):
    with seeded(torch_cuda, wa) as c:
        c.copy_states(c, dst_first=1, src_first=0, n=700)
        c.sync()
        sb, x, y = wa.sb.copy(), wa.x.copy(), wa.y.copy()
        sb[1:701], x[1:701], y[1:701] = wa.sb[:700], wa.x[:700], wa.y[:700]
        check_context(c, sb, x, y)


@pytest.mark.parametrize("where", ["one_group", "across_groups"])
def test_copy_swap_through_ids(built, torch_cuda, wa, where):
    rng = np.random.default_rng(24)
    if where == "one_group":
        p = 3 * 256 + rng.permutation(256)
        a, b = p[:128], p[128:]
    else:
        p = rng.permutation(N)
        a, b = p[:150], p[150:300]
    dst = np.concatenate([a, b]).astype(np.uint32)
    src = np.concatenate([b, a]).astype(np.uint32)
    with seeded(torch_cuda, wa) as c:
        c.copy_states(c, dst_ids=T(torch_cuda, dst), src_ids=T(torch_cuda, src))
        c.sync()
        sb, x, y = wa.sb.copy(), wa.x.copy(), wa.y.copy()
        sb[dst], x[dst], y[dst] = wa.sb[src], wa.x[src], wa.y[src]
        check_context(c, sb, x, y)


def test_copy_across_contexts(built, torch_cuda, wa, wb):
    torch = torch_cuda
    rng = np.random.default_rng(25)
    src = rng.permutation(N)[:600].astype(np.uint32)
    dst = rng.permutation(N)[:600].astype(np.uint32)
    with seeded(torch, wa) as ca, seeded(torch, wb) as cb:
        cb.copy_states(ca, dst_ids=T(torch, dst), src_ids=T(torch, src))
        cb.sync()
        ca.sync()
        check_context(ca, wa.sb, wa.x, wa.y)                          # the source is only read
        sb, x, y = wb.sb.copy(), wb.x.copy(), wb.y.copy()
        sb[dst], x[dst], y[dst] = wa.sb[src], wa.x[src], wa.y[src]
        check_context(cb, sb, x, y)                                   # untouched slots of the destination
        off = T(torch, (np.arange(600) * 100).astype(np.uint64))
        ln = T(torch, np.full(600, 100, dtype=np.uint32))
        pa = torch.zeros(600 * 100, dtype=torch.uint8, device="cuda")
        pb = torch.zeros(600 * 100, dtype=torch.uint8, device="cuda")
        ca.crypt(pa, off, ln, ids=T(torch, src))
        cb.crypt(pb, off, ln, ids=T(torch, dst))
        ca.sync()
        cb.sync()
        want = np.zeros(600 * 100, dtype=np.uint8)
        oracle_from(wa.sb[src], wa.x[src], wa.y[src]).crypt(want, (np.arange(600) * 100).astype(np.uint64),
                                                            np.full(600, 100, dtype=np.uint32))
        assert torch.equal(pa, pb)
        assert np.array_equal(pa.cpu().numpy(), want)


def test_copy_of_nothing_is_ok(ctx_a):
    ctx_a.copy_states(ctx_a, dst_first=0, src_first=0, n=0)
    ctx_a.sync()


# ---------------------------------------------------------------- 6. set_states
def test_set_states_reads_back(built, torch_cuda, wa, wb):
    with seeded(torch_cuda, wa) as c:
        c.set_states(3, wb.sb[:509], wb.x[:509], wb.y[:509])
        got = c.get_states(3, 509)
        assert np.array_equal(got[0], wb.sb[:509])
        assert np.array_equal(got[1], wb.x[:509]) and np.array_equal(got[2], wb.y[:509])
        sb, x, y = wa.sb.copy(), wa.x.copy(), wa.y.copy()
        sb[3:512], x[3:512], y[3:512] = wb.sb[:509], wb.x[:509], wb.y[:509]
        check_context(c, sb, x, y)


# -------------------------------------------------------------- 7. stream order
def test_copy_then_crypt_on_one_stream(ctx_a, torch_cuda, wa):
    torch = torch_cuda
    s = torch.cuda.Stream()
    with torch.cuda.stream(s), Context(0, N) as b:
        b.copy_states(ctx_a, dst_first=0, src_first=0, n=N, stream=s)       # no sync before the crypt
        crypt_all_and_check(torch, b, wa.sb, wa.x, wa.y, stream=s)


# ------------------------------------------------- paths the cases above leave out
def test_export_ids_slot_named_twice(ctx_a, torch_cuda, wa):
    """A one-group bucket that names a slot twice leaves the image path (a
    column has one record there): both entries get the slot's record."""
    ids = 256 + np.random.default_rng(26).permutation(256).astype(np.int64)
    ids[9] = ids[5]
    sb, xy = out_bufs(torch_cuda, 256)
    ctx_a.export_states(sb, xy, ids=T(torch_cuda, ids.astype(np.uint32)))
    ctx_a.sync()
    check_records(sb, xy, wa, [int(i) for i in ids] + [-1])


@pytest.mark.parametrize("dst_by", ["ids", "range"])
def test_copy_skips_an_entry_with_an_idle_side(built, torch_cuda, wa, wb, dst_by):
    """An idle source leaves its destination alone (by ids: the scatter
    kernel's gate; by range: the image kernel's), an idle destination drops
    its source's record."""
    torch = torch_cuda
    rng = np.random.default_rng(27)
    n = 400
    src = rng.permutation(N)[:n].astype(np.int64)
    src[rng.permutation(n)[:30]] = IDLE_SLOT
    dst = 500 + np.arange(n, dtype=np.int64)
    if dst_by == "ids":
        dst = rng.permutation(N)[:n].astype(np.int64)
        dst[rng.permutation(n)[:30]] = IDLE_SLOT
    with seeded(torch, wa) as ca, seeded(torch, wb) as cb:
        if dst_by == "ids":
            cb.copy_states(ca, dst_ids=T(torch, dst.astype(np.uint32)), src_ids=T(torch, src.astype(np.uint32)))
        else:
            cb.copy_states(ca, dst_first=500, src_ids=T(torch, src.astype(np.uint32)))
        cb.sync()
        ca.sync()
        sb, x, y = wb.sb.copy(), wb.x.copy(), wb.y.copy()
        live = np.flatnonzero((src != IDLE_SLOT) & (dst != IDLE_SLOT))
        sb[dst[live]], x[dst[live]], y[dst[live]] = wa.sb[src[live]], wa.x[src[live]], wa.y[src[live]]
        check_context(cb, sb, x, y)


def test_copies_on_two_streams_share_the_scratch_in_order(ctx_a, torch_cuda, wa):
    """Two copies into one context from two streams, disjoint groups, no host
    wait in between: the second waits on the device for the first to be done
    with the context's record scratch."""
    torch = torch_cuda
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with Context(0, N) as b:
        b.copy_states(ctx_a, dst_first=0, src_first=768, n=768, stream=s1)
        b.copy_states(ctx_a, dst_first=768, src_first=0, n=768, stream=s2)
        b.sync(s1)
        b.sync(s2)
        order = np.concatenate([np.arange(768, N), np.arange(768)])
        check_context(b, wa.sb[order], wa.x[order], wa.y[order])


def test_unaligned_records_are_refused(ctx_a, torch_cuda):
    sb, xy = out_bufs(torch_cuda, 4)
    for call in (ctx_a.export_states, ctx_a.import_states):
        with pytest.raises(ZRC4Error) as ei:
            call(sb.data_ptr() + 8, xy, first_slot=0, n=2)
        assert ei.value.code == -1
    ctx_a.sync()
