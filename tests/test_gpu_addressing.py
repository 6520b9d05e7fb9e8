"""64-bit address arithmetic of every batched entry point: spans across a
multiple of 2^32, offsets of 2^32 and more, and offsets that wrap.

Every batched call of include/zrc4.h takes one base pointer and 64-bit
per-entry offsets, and `base + off` is computed modulo 2^64: the session engine
(engine/rc4_hooks_device.cpp) and the reservoir refills (zrc4_ks.inc) pass an
entry's address minus the base, whichever of the two is higher.  The kernels
keep addresses as lo/hi register pairs and step them in inline assembly; a
step that adds to the low half only is bit-exact on every buffer that holds no
multiple of 2^32.  The tests here choose the addresses (tests/addr_layout.py):
one 12.1 GiB device allocation that is never touched as a whole, three 8 MiB
windows around its three multiples of 2^32 (A1 < A < A3) that are filled with
random bytes and read back IN FULL after every call, the spans of a call laid
out so that one message (the straddler) has A inside it at a chosen split, and
the base pointer below, near, at or above A.  The windows at A1 and A3 are
guards: a lost carry or a truncated offset lands 2^32 below, a spurious carry
2^32 above, inside the allocation.

The reference is the oracle (oracle/rc4_oracle.c through pyoracle, pinned to
the reference header) run over a host copy of the windows; everything is
compared bit for bit: the three windows (spans, gaps, guards), the states of
the slots (zrc4_get_states), and zrc4_sync's return.  One context lives through
the module, so every stream carries on from call to call and from test to
test.  Each crypt test is one (I/O form, kernel family and shape, base mode)
and asserts the family it means to reach; inside it the straddler's position
and split cycle, one launch per split.

The layouts are checked on the CPU (test_layouts_*, test_family_*).  What the
tests make of a library with a lost carry is recorded in
profiles/addressing/sensitivity_lost_carry.log.
"""
import os
import subprocess
from collections import namedtuple
from contextlib import contextmanager
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import pyoracle
from addr_layout import (ARENA_BYTES, G4, M, MODES, SPLITS, WIN, base_of, check_offsets, check_spans, lines, offsets,
                         span_bytes, span_layout, window_index)
from dispatch_model import family
from frame_support import BOUND, frame_report
from gpu_support import cu_count, dev

ROOT = Path(__file__).resolve().parents[1]
IDLE = 0xFFFFFFFF                       # ZRC4_IDLE_SLOT
SPARE_GROUPS = 8                        # groups of the arena no bucket of the largest call names
BUDGET = WIN - (192 << 10)              # bytes of one call's spans and gaps (they may all lie on one side of A)
FAKE_START = 0x7F1234500000             # the CPU checks' arena start
MAXP = 4                                # frame tests: max_packets

# ------------------------------------------------------------------ the shapes
# id, entry point, first_slot, entries(CUs), the family plan_crypt picks, second pass
Shape = namedtuple("Shape", "id call first n family second", defaults=(False,))


def _g(groups, last=77):
    """groups(CUs) groups or buckets, the last one ragged."""
    return lambda cus: (groups(cus) - 1) * 256 + last


SHAPES = [
    Shape("win-range-1g", "range", 0, lambda cus: 200, "win"),
    Shape("win-grouped-2b", "grouped", 0, lambda cus: 456, "win"),
    Shape("win-declared-2b", "declared", 0, lambda cus: 456, "win"),
    Shape("half-range-33g", "range", 0, _g(lambda cus: 33), "half"),
    Shape("half-grouped-33b", "grouped", 0, _g(lambda cus: 33), "half"),
    Shape("decl-half-33b", "declared", 0, _g(lambda cus: 33), "decl"),
    Shape("decl-whole-halfCUs+1b", "declared", 0, _g(lambda cus: cus // 2 + 1), "decl"),      # 129 on 256 CUs
    Shape("whole-range-fs3-n300", "range", 3, lambda cus: 300, "whole"),
    Shape("whole-ids-n300", "ids", 0, lambda cus: 300, "whole"),
    Shape("whole-range-halfCUs+1g", "range", 0, _g(lambda cus: cus // 2 + 1), "whole"),       # 129 on 256 CUs
    Shape("stream-range-CUs+1g", "range", 0, _g(lambda cus: cus + 1), "stream"),
    Shape("stream-range-fs3-CUs+1g", "range", 3, _g(lambda cus: cus + 1), "stream"),          # non-prefetching form
    Shape("stream-ids-CUs+1g", "ids", 0, _g(lambda cus: cus + 1), "stream"),
    Shape("stream2-grouped-2CUs+3b", "grouped", 0, _g(lambda cus: 2 * cus + 3), "stream", True),
    Shape("stream2-declared-2CUs+3b", "declared", 0, _g(lambda cus: 2 * cus + 3), "stream", True),
]
BY_ID = {s.id: s for s in SHAPES}
NO_IDS = [s for s in SHAPES if s.call != "ids"]             # the forms without a scattered-ids call
FRAME_SHAPES = [BY_ID[i] for i in ("win-range-1g", "win-grouped-2b", "win-declared-2b", "half-range-33g",
                                   "half-grouped-33b", "decl-half-33b", "stream-range-CUs+1g")] + [
    Shape("stream-grouped-CUs+1b", "grouped", 0, _g(lambda cus: cus + 1), "stream"),
    Shape("stream-declared-CUs+1b", "declared", 0, _g(lambda cus: cus + 1), "stream"),
]
ROUNDS_SHAPES = [                       # no window form: 2 groups run the lane-per-stream half-group kernel
    Shape("rounds-range-2g", "range", 0, lambda cus: 456, "half"),
    Shape("rounds-grouped-2b", "grouped", 0, lambda cus: 456, "half"),
    Shape("rounds-range-halfCUs+1g", "range", 0, _g(lambda cus: cus // 2 + 1), "whole"),
    Shape("rounds-grouped-halfCUs+1b", "grouped", 0, _g(lambda cus: cus // 2 + 1), "whole"),
    Shape("rounds-range-CUs+1g", "range", 0, _g(lambda cus: cus + 1), "stream"),              # host-split path
    Shape("rounds-grouped-CUs+1b", "grouped", 0, _g(lambda cus: cus + 1), "stream"),
]
ROUNDS = 3
# form -> (CryptIo of zrc4_plan.hpp, framed, its shapes, its base modes)
FORMS = {
    "inplace": (0, False, SHAPES, MODES),
    "keystream": (1, False, NO_IDS, MODES),
    "to-a": (2, False, NO_IDS, MODES),                      # destinations across A, sources elsewhere
    "to-b": (2, False, NO_IDS, ("near", "above")),          # one shared source across A (broadcast)
    "to-c": (2, False, NO_IDS, ("near", "above")),          # as to-a, every entry on the byte path
    "frame": (0, True, FRAME_SHAPES, ("near", "above")),
    "rounds": (3, False, ROUNDS_SHAPES, ("near", "above")),
}
FORM_NAMES = list(FORMS)
ALL_SHAPES = SHAPES + FRAME_SHAPES[-2:] + ROUNDS_SHAPES
SHAPE_NO = {s.id: i for i, s in enumerate(ALL_SHAPES)}


LONG_SPLITS = (448, 777)                # with a 1500-byte straddler (below)


def launch_plan(shape):
    """(split, straddler length or 0 for a random 200..1500) of every launch:
    one launch per split of SPLITS; then two splits deep inside a 1500-byte
    straddler, one on a 64-byte block boundary and one not, so that the
    pointers a kernel only steps from the fifth block on (the line loop's
    per-lane loads, two lines ahead) carry too.  On the window shapes the
    straddler of the `len - 1` launch is 5000 bytes, and one more launch splits
    5000 bytes at 2048 + 16: a ring chunk boundary and A inside one message."""
    win = shape.family == "win"
    plan = [(s, 0) for s in SPLITS[:-1]] + [(-1, 5000 if win else 0)] + [(s, 1500) for s in LONG_SPLITS]
    return plan + [(2048 + 16, 5000)] * win


def n_launches(shape):
    return len(launch_plan(shape))


def k_positions(shape, n, cus):
    """Where the straddler sits: the first entry, the last, lanes 63 and 64 of
    a middle workgroup, the last busy lane of the last workgroup (the two
    entries after it idle); on the second-pass shapes also an entry of a bucket
    some workgroup runs as its second, and one of the bucket before those."""
    mid = ((-(-n // 256) - 1) // 2) * 256
    ks = [("first", 0), ("last", n - 1), ("lane63", mid + 63), ("lane64", mid + 64), ("last-busy", n - 3)]
    if shape.second:
        ks += [("second-pass", 256 * 2 * cus + 5), ("before-second-pass", 256 * (2 * cus - 1) + 200)]
    return ks


def entries(shape, cus, rng, li, cap):
    """Which slot each entry uses, and which entry is the straddler."""
    n = shape.n(cus)
    G = -(-n // 256)
    ks = k_positions(shape, n, cus)
    kind, k = ks[li % len(ks)]
    e = SimpleNamespace(n=n, first=shape.first, call=shape.call, k=k, kind=kind, ids=None, decl=None)
    busy = np.ones(n, bool)
    if shape.call in ("grouped", "declared"):
        busy = rng.random(n) >= 0.1                             # ~10 % of every bucket is padding
        busy[[kk for _, kk in ks]] = True
        groups = rng.permutation(min(cap // 256, G + SPARE_GROUPS))[:G]
        slots = (groups[:, None] * 256 + rng.permuted(np.tile(np.arange(256), (G, 1)), axis=1)).reshape(-1)[:n]
        e.slot_hi = min(cap, (G + SPARE_GROUPS) * 256)
    elif shape.call == "ids":
        e.slot_hi = min(cap, max(4096, 2 * n))
        slots = rng.permutation(e.slot_hi)[:n]
    else:
        slots = shape.first + np.arange(n)
        e.slot_hi = -(-(shape.first + n) // 256) * 256
    if kind == "last-busy":
        busy[k + 1:] = False
    e.busy = busy
    if shape.call in ("grouped", "declared"):
        slots = np.where(busy, slots, -1)
        e.ids = np.where(busy, slots, IDLE).astype(np.uint32)
        if shape.call == "declared":
            e.decl = groups.astype(np.uint32)
    elif shape.call == "ids":
        e.ids = slots.astype(np.uint32)
    e.slots = slots.astype(np.int64)
    return e


def lengths(rng, e, klen, budget, cost=lambda L, gaps: int(L.sum() + gaps.sum())):
    """Most entries 0..96 bytes, 8 % of them empty; 64 entries of 200..1500
    bytes, the straddler one of them (or klen bytes); gaps of 0..19 bytes.
    Where that is more than `budget` (the large shapes: the window is 4 MiB
    either side of A), random short entries are emptied until it fits."""
    n = e.n
    L = rng.integers(0, 97, n)
    L[rng.random(n) < 0.08] = 0
    long = rng.permutation(np.flatnonzero(e.busy))[:64]
    L[long] = rng.integers(200, 1501, long.size)
    L[e.k] = klen or int(rng.integers(200, 1501))
    L[~e.busy] = 0
    gaps = rng.integers(0, 20, n)
    keep = np.zeros(n, bool)
    keep[long] = True
    keep[e.k] = True
    while cost(L, gaps) > budget:
        drop = ~keep & (rng.random(n) < 0.2)
        L[drop] = 0
        gaps[L == 0] = 0
    return L.astype(np.int64), gaps


def _slots16(L, extra):
    """A 16-aligned slot of ceil16(len) + extra bytes per non-empty entry:
    (slot starts, total)."""
    size = np.where(L > 0, (L + 15) // 16 * 16 + extra, 0)
    return np.cumsum(size) - size, int(size.sum())


def _residues(rng, ref_addr, congruent):
    """addr mod 16 for each entry: the reference address's residue where
    `congruent`, another one elsewhere."""
    return (ref_addr % 16 + np.where(congruent, 0, rng.integers(1, 16, ref_addr.size))) % 16


def build(shape, cus, form, li, a, cap):
    """Launch li of one (form, shape) test: every table of the call as absolute
    addresses (the base mode turns them into offsets).  Deterministic, so the
    CPU checks see exactly what the GPU tests launch."""
    rng = np.random.default_rng([20261020, SHAPE_NO[shape.id], FORM_NAMES.index(form), li])
    e = entries(shape, cus, rng, li, cap)
    s, klen = launch_plan(shape)[li]
    cl = e
    cl.form = form
    if form == "to-b":
        # one source from a - s on for every entry (entry k reads len[k] > s bytes of it, the longer ones more);
        # destinations in 16-aligned slots above a + 64 KiB
        L, _ = lengths(rng, e, klen, BUDGET - (128 << 10), lambda L, g: _slots16(L, 32)[1])
        cl.s = int(L[e.k]) - 1 if s < 0 else s
        cl.src = np.full(e.n, a - cl.s, np.int64)
        at, _ = _slots16(L, 32)
        cl.addr = a + (64 << 10) + at + _residues(rng, cl.src, rng.random(e.n) < 0.5)
        cl.L = L
        cl.src_spans = (np.array([a - cl.s]), np.array([int(L.max())]))
        return cl
    if form == "rounds":
        return _build_rounds(cl, rng, s, klen, a)
    L, gaps = lengths(rng, e, klen, BUDGET)
    cl.s = int(L[e.k]) - 1 if s < 0 else s
    cl.L = L
    cl.addr = span_layout(L, gaps, e.k, cl.s, a)
    if form in ("to-a", "to-c"):
        # sources in a tensor of their own, entry i's at src_pos[i] of it
        cong = rng.random(e.n) < 0.5 if form == "to-a" else np.zeros(e.n, bool)
        at, cl.src_size = _slots16(L, 16)
        cl.src_pos = at + _residues(rng, cl.addr, cong)
        cl.src_size += 32
    if form == "frame":
        # the spans are the receive BLOCKS; an earlier iteration decrypted the first 0..40 bytes of each
        head = np.minimum(rng.integers(0, 41, e.n), L)
        head[e.k] = min(int(head[e.k]), int(L[e.k]) - 1)
        cl.head = head
        cl.seed = int(rng.integers(1 << 30))
    return cl


def _build_rounds(cl, rng, s, klen, a):
    """Three rounds, all in A's window, src == dst pointer.  Round 0 is in
    place on a layout across A (the straddler's source and destination are the
    same address).  Rounds 1 and 2 are out of place into 16-aligned slots above
    round 0's layout; their sources lie in the guard windows, which the call
    only reads: round 1's around A3, the straddler's own across A3 at the same
    split, round 2's around A1 likewise.  (A destination may overlap no source
    of the call but its own identical one, include/zrc4.h, so no later round
    can read across A itself.)"""
    n = cl.n
    part = BUDGET // 3
    L0, gaps = lengths(rng, cl, klen, part)
    cl.s = int(L0[cl.k]) - 1 if s < 0 else s
    d0 = span_layout(L0, gaps, cl.k, cl.s, a)
    top = (int((d0 + L0).max()) + 15) // 16 * 16 + 64
    Ls, dst, src = [L0], [d0], [d0]
    for r, line in ((1, a + G4), (2, a - G4)):
        L, _ = lengths(rng, cl, 0, part, lambda L, g: _slots16(L, 32)[1])
        sa = line - (32 << 10) + rng.integers(0, (64 << 10) - 1600, n)
        sa[cl.k] = line - min(cl.s, int(L[cl.k]) - 1)
        at, total = _slots16(L, 32)
        dst.append(top + at + _residues(rng, sa, rng.random(n) < 0.5))
        top += total + 64
        Ls.append(L)
        src.append(sa)
    cl.L, cl.addr, cl.src = np.concatenate(Ls), np.concatenate(dst), np.concatenate(src)
    return cl


# ------------------------------------------------------------------ CPU checks
def _plan_lines(shapes):
    exe = Path(os.environ.get("ZSX_TOOLS_BIN", ROOT / "tools" / "bin")) / "plan_check"
    got = subprocess.run([str(exe), "plan", *[str(v) for sh in shapes for v in sh]], capture_output=True, text=True)
    assert got.returncode == 0, got.stdout + got.stderr
    return got.stdout.splitlines()


def test_family_matches_plan_crypt(built):
    """family() of tests/dispatch_model.py against plan_crypt (tools/bin/plan_check
    plan) for every (form, shape) of this module at 104, 256 and 304 CUs; at 256 CUs, an
    MI355X's, every shape reaches the family its id names, the persistent
    write-only and out-of-place shapes take the two-launch path
    (span_fill_kernel / span_copy_kernel) and the persistent rounds shapes the
    host-split path."""
    rows, args = [], []
    for form, (io, frame, shapes, _) in FORMS.items():
        for sh in shapes:
            for cus in (104, 256, 304):
                n = sh.n(cus)
                rows.append((form, sh, cus, n, io))
                args.append(({"ids": 0, "range": 1}.get(sh.call, 2), int(sh.first % 256 == 0), n, cus, int(frame),
                             int(sh.call == "declared"), io, ROUNDS if io == 3 else 1))
    for (form, sh, cus, n, io), line in zip(rows, _plan_lines(args)):
        fam, name, pre, split = line.split()
        assert family(sh.call, sh.first, n, cus, io) == fam, (form, sh.id, cus, line)
        if cus == 256:
            assert fam == sh.family, (form, sh.id, line)
            if fam == "stream":
                assert int(pre) == {0: 0, 1: 1, 2: 2, 3: 2}[io] and int(split) == (io == 3), (form, sh.id, line)
            if sh.second:
                assert -(-n // 256) > 2 * cus                       # more buckets than workgroups: a second pass


CASES = [(form, sh) for form, (_, _, shapes, _) in FORMS.items() for sh in shapes]


@pytest.mark.parametrize("form,shape", CASES, ids=lambda v: v if isinstance(v, str) else v.id)
def test_layouts_of_every_launch(form, shape):
    """CPU: every launch of every GPU test below, as built for 256 CUs over a
    made-up arena start.  Exactly one span holds both A - 1 and A; the spans
    are pairwise disjoint and inside A's window; sources written by nobody lie
    in a window too; in every base mode the offsets give the addresses back
    modulo 2^64, in `low` mode each has a nonzero high word, in `above` mode
    each is >= 2^63.  Every straddler position of k_positions is used."""
    a1, a, a3 = lines(FAKE_START)
    assert FAKE_START + M <= a1 and a3 + M <= FAKE_START + ARENA_BYTES and a % G4 == 0
    cap = (2 * 256 + 3 + SPARE_GROUPS) * 256
    kinds = set()
    for li in range(n_launches(shape)):
        cl = build(shape, 256, form, li, a, cap)
        kinds.add(cl.kind)
        live = cl.L > 0
        if form == "to-b":
            check_spans(cl.addr, cl.L, a, straddler=False)
            check_spans(np.concatenate([cl.addr, cl.src_spans[0]]), np.concatenate([cl.L, cl.src_spans[1]]), a)
            assert (cl.addr[live] >= a + (64 << 10)).all() and 0 < cl.s < cl.L[cl.k]
            same = (cl.addr - cl.src)[live] % 16 == 0
            assert 0.3 < same.mean() < 0.7
        else:
            check_spans(cl.addr, cl.L, a)
            assert cl.addr[cl.k] == a - cl.s and 0 < cl.s < cl.L[cl.k]
        if cl.k > 0 and form not in ("to-b", "rounds"):
            gap = cl.addr[cl.k] - (cl.addr[cl.k - 1] + cl.L[cl.k - 1])
            assert 0 <= gap <= 19 and (cl.addr[:cl.k] + cl.L[:cl.k] <= a).all() and (cl.addr[cl.k + 1:] > a).all()
        if form in ("to-a", "to-c"):
            same = (cl.addr - cl.src_pos)[live] % 16 == 0
            assert (0.3 < same.mean() < 0.7) if form == "to-a" else not same.any()
            check_spans(cl.src_pos, cl.L, 0, straddler=False, window=False)
            assert (cl.src_pos + cl.L).max() <= cl.src_size
        if form == "rounds":
            n = cl.n
            assert cl.L.size == ROUNDS * n and np.array_equal(cl.src[:n], cl.addr[:n])
            for r, line in ((1, a3), (2, a1)):
                sa, L = cl.src[r * n:(r + 1) * n], cl.L[r * n:(r + 1) * n]
                assert (sa >= line - WIN).all() and (sa + L <= line + WIN).all()
                assert sa[cl.k] < line < sa[cl.k] + L[cl.k]              # the straddler's source crosses a line
        if form == "frame":
            assert (cl.head <= cl.L).all() and cl.head[cl.k] < cl.L[cl.k]
        per_round = cl.L.reshape(-1, cl.n)
        assert (per_round[:, ~cl.busy] == 0).all() and ((per_round >= 200).sum(axis=1) >= min(64, cl.busy.sum())).all()
        assert np.unique(cl.slots[cl.slots >= 0]).size == (cl.slots >= 0).sum() and cl.slots.max() < cl.slot_hi
        assert np.array_equal(cl.slots >= 0, cl.busy) if cl.call in ("grouped", "declared") else (cl.slots >= 0).all()
        for mode in MODES:
            check_offsets(cl.addr, mode, FAKE_START)
            if hasattr(cl, "src"):
                check_offsets(cl.src, mode, FAKE_START, in_window=form == "to-b")
    assert kinds == {kd for kd, _ in k_positions(shape, shape.n(256), 256)}
    deep = [build(shape, 256, form, li, a, cap) for li, (_, klen) in enumerate(launch_plan(shape)) if klen]
    want = [(1500, 448), (1500, 777)]
    if shape.family == "win":
        want = [(5000, 4999)] + want + [(5000, 2064)]
    assert [(int(c.L[c.k]), c.s) for c in deep] == want


def test_layout_helper_edges():
    """span_layout with the straddler first, last and alone; window_index maps
    each window onto its third of the host mirror."""
    a1, a, a3 = lines(FAKE_START)
    L, g = np.array([5, 0, 40, 7]), np.array([3, 19, 0, 2])
    for k, s in ((0, 1), (0, 4), (2, 39), (3, 6), (2, 16)):
        st = span_layout(L, g, k, s, a)
        assert st[k] == a - s and np.array_equal(st[1:], st[:-1] + L[:-1] + g[1:])
        check_spans(st, L, a)
    assert span_layout([9], [0], 0, 8, a).tolist() == [a - 8]
    assert window_index([a1 - WIN, a - WIN, a, a3 + WIN - 1], a).tolist() == [0, 2 * WIN, 3 * WIN, 6 * WIN - 1]
    for mode in MODES:
        off = check_offsets(np.array([a - 1, a]), mode, FAKE_START)
        assert (int(off[1]) - int(off[0])) % (1 << 64) == 1
    assert base_of("low", FAKE_START) == FAKE_START and base_of("above", FAKE_START) == a + WIN


# ------------------------------------------------------------------------- GPU
class Rig:
    """The arena, the host mirror of its three windows, one context and the
    oracle's streams of its slots."""

    def __init__(self, torch):
        from zsummerx_amd import Context
        self.torch = torch
        self.cus = cu_count(torch)
        self.T = dev(torch)
        self.arena = torch.empty(ARENA_BYTES, dtype=torch.uint8, device="cuda")     # never touched as a whole
        self.start = self.arena.data_ptr()
        self.a1, self.a, self.a3 = lines(self.start)
        assert self.start + M <= self.a1 and self.a3 + M <= self.start + ARENA_BYTES
        self.cap = (2 * self.cus + 3 + SPARE_GROUPS) * 256
        self.c = Context(0, self.cap)
        self.H0 = np.random.default_rng(4).integers(0, 256, 6 * WIN, dtype=np.uint8)
        self.H = None
        self.dirty = True

    def close(self):
        self.c.close()
        del self.arena
        self.torch.cuda.empty_cache()

    def reseed(self):
        rng = np.random.default_rng(5)
        keys = rng.integers(0, 256, 16 * self.cap, dtype=np.uint8)
        koff = np.arange(self.cap, dtype=np.uint64) * 16
        klen = np.full(self.cap, 16, np.uint32)
        self.ob = pyoracle.Batch(self.cap)
        self.ob.make_sbox(keys, koff, klen)
        self.c.ksa_range(0, self.T(klen.view(np.int32)), self.T(koff.view(np.int64)), self.T(keys))
        self.c.sync()

    @contextmanager
    def session(self):
        """The windows refilled; the streams carry on from the last test (they
        are seeded again only after a test that failed)."""
        if self.dirty:
            self.reseed()
        self.dirty = True
        self.H = self.H0.copy()
        for w in range(3):
            self.upload(w)
        yield self.H
        self.dirty = False

    def _win(self, w):
        lo = (self.a1, self.a, self.a3)[w] - WIN - self.start
        return self.arena[lo:lo + 2 * WIN]

    def upload(self, w, data=None):
        src = self.H[w * 2 * WIN:(w + 1) * 2 * WIN] if data is None else data
        self._win(w).copy_(self.torch.from_numpy(src))

    def read(self):
        return self.torch.cat([self._win(w) for w in range(3)]).cpu().numpy()

    def view(self, mode):
        base = base_of(mode, self.start)
        return self.arena[base - self.start:], base

    def idx(self, addr):
        return window_index(addr, self.a)

    def oracle(self, buf, slots, index, L):
        """Every busy entry's stream over buf[index, index + L), in place."""
        m = (slots >= 0) & (L > 0)
        off = np.zeros(self.cap, np.uint64)
        ln = np.zeros(self.cap, np.uint32)
        off[slots[m]] = index[m]
        ln[slots[m]] = L[m]
        self.ob.crypt(buf, off, ln, threads=8)

    def windows_report(self, got=None):
        got = self.read() if got is None else got
        bad = np.flatnonzero(got != self.H)
        if bad.size == 0:
            return ""
        out = []
        for w, name in enumerate(("guard window A1", "window A", "guard window A3")):
            b = bad[bad // (2 * WIN) == w]
            if b.size:
                rel = b % (2 * WIN) - WIN
                out.append(f"{name}: {b.size} bytes differ, first at {name.split()[-1]}{int(rel[0]):+d} "
                           f"last at {int(rel[-1]):+d} (got {got[b[:6]].tolist()} want {self.H[b[:6]].tolist()})")
        return "; ".join(out)

    def states_report(self, hi):
        gsb, gx, gy = self.c.get_states(0, hi)
        o = np.frombuffer(self.ob.st, dtype=np.int32).reshape(-1, 258)[:hi]
        bad = np.flatnonzero((gsb != o[:, 2:].astype(np.uint8)).any(axis=1) | (gx != o[:, 0].astype(np.uint8))
                             | (gy != o[:, 1].astype(np.uint8)))
        return f"states of {bad.size} slots differ, first {bad[:8].tolist()}" if bad.size else ""

    def verify(self, what, hi):
        """zrc4_sync is ZRC4_OK (Context.sync raises otherwise), the three
        windows are the host mirror, the first `hi` slots are the oracle's."""
        self.c.sync()
        msgs = [m for m in (self.windows_report(), self.states_report(hi)) if m]
        assert not msgs, f"{what}: " + "; ".join(msgs)


@pytest.fixture(scope="module")
def rig(built):
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    r = Rig(torch)                      # the allocation failing is an error: an MI355X has the memory
    yield r
    r.close()


def _packets(rng, buf, at, L):
    """proto4z packets over buf[at[i], at[i] + L[i]) for every i: the packet
    form of tests/test_frame_scan.py::packet_streams (a u32 length first) with
    the block lengths given, packets of 6..40 bytes back to back, the last one
    usually cut short by the block's end; 3 % of the blocks carry a length
    field below 6 in their second packet (status 2).  The other bytes stay."""
    pool = rng.integers(6, 41, 1 << 16)
    cum = np.concatenate([[0], np.cumsum(pool)])
    live = np.flatnonzero(L > 0)
    s = rng.integers(0, pool.size - 900, live.size)
    cnt = np.searchsorted(cum, cum[s] + L[live], side="left") - s
    ent = np.repeat(np.arange(live.size), cnt)
    j = np.arange(ent.size) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    val = pool[s[ent] + j].copy()
    pst = cum[s[ent] + j] - cum[s[ent]]
    corrupt = rng.random(live.size) < 0.03
    corrupt[np.flatnonzero(cnt >= 3)[:2]] = True
    val[(j == 1) & corrupt[ent]] = 3
    for b in range(4):
        ok = pst + b < L[live][ent]
        buf[at[live][ent][ok] + pst[ok] + b] = (val[ok] >> (8 * b)) & 255


def _dispatch(rig, cl, view, base, src=None, src_off=None):
    """The call of cl's form and entry point over offsets from `base`."""
    c, T = rig.c, rig.T
    off = T(offsets(cl.addr, base).view(np.int64))
    ln = T(cl.L.astype(np.uint32).view(np.int32))
    ids = None if cl.ids is None else T(cl.ids.view(np.int32))
    ranged = cl.ids is None
    if cl.form == "inplace":
        if ranged:
            c.crypt_range(cl.first, view, off, ln)
        elif cl.call == "ids":
            c.crypt(view, off, ln, ids=ids)
        elif cl.call == "grouped":
            c.crypt_grouped(view, off, ln, ids)
        else:
            c.crypt_grouped_declared(view, off, ln, ids, cl.decl)
    elif cl.form == "keystream":
        if ranged:
            c.keystream_range(cl.first, view, off, ln)
        else:
            c.keystream_grouped(view, off, ln, ids, bucket_group=cl.decl)
    elif cl.form == "rounds":
        if ranged:
            c.crypt_to_range_rounds(cl.first, src, src_off, view, off, ln, cl.n, ROUNDS)
        else:
            c.crypt_to_grouped_rounds(src, src_off, view, off, ln, ids, cl.n, ROUNDS, bucket_group=cl.decl)
    else:
        if ranged:
            c.crypt_to_range(cl.first, src, src_off, view, off, ln)
        else:
            c.crypt_to_grouped(src, src_off, view, off, ln, ids, bucket_group=cl.decl)


def _run_launch(rig, cl, mode, what):
    H, T = rig.H, rig.T
    view, base = rig.view(mode)
    at = rig.idx(cl.addr)
    form = cl.form
    if form == "inplace":
        rig.oracle(H, cl.slots, at, cl.L)
        _dispatch(rig, cl, view, base)
    elif form == "keystream":
        H[rig.idx(span_bytes(cl.addr, cl.L))] = 0               # the oracle's keystream: its crypt of zeros
        rig.oracle(H, cl.slots, at, cl.L)
        _dispatch(rig, cl, view, base)                          # (the device's spans still hold random bytes)
    elif form in ("to-a", "to-c"):
        sh = np.random.default_rng(cl.src_size).integers(0, 256, cl.src_size, dtype=np.uint8)
        H[rig.idx(span_bytes(cl.addr, cl.L))] = sh[span_bytes(cl.src_pos, cl.L)]
        rig.oracle(H, cl.slots, at, cl.L)
        src = T(sh)
        assert src.data_ptr() % 16 == 0
        _dispatch(rig, cl, view, base, src, T(cl.src_pos.astype(np.uint64).view(np.int64)))
        rig.c.sync()
        assert np.array_equal(src.cpu().numpy(), sh), f"{what}: the sources were written"
    elif form == "to-b":
        H[rig.idx(span_bytes(cl.addr, cl.L))] = H[rig.idx(span_bytes(cl.src, cl.L))]
        rig.oracle(H, cl.slots, at, cl.L)
        _dispatch(rig, cl, view, base, view, T(offsets(cl.src, base).view(np.int64)))
    elif form == "rounds":
        n = cl.n
        for r in range(ROUNDS):                                 # the oracle's three successive calls
            q = slice(r * n, (r + 1) * n)
            if r:
                H[rig.idx(span_bytes(cl.addr[q], cl.L[q]))] = H[rig.idx(span_bytes(cl.src[q], cl.L[q]))]
            rig.oracle(H, cl.slots, at[q], cl.L[q])
        _dispatch(rig, cl, view, base, view, T(offsets(cl.src, base).view(np.int64)))
    rig.verify(what, cl.slot_hi)


def _run_frame_launch(rig, cl, mode, what):
    """Decrypt + frame: the blocks are the laid-out spans, proto4z packets
    before encryption; each entry's tail (all but its first 0..40 bytes) is
    ciphertext on the device.  After the call the windows are the plaintext
    and npk / used / status / pkt_len are the oracle's scan of it."""
    H, T, c = rig.H, rig.T, rig.c
    view, base = rig.view(mode)
    at = rig.idx(cl.addr)
    _packets(np.random.default_rng(cl.seed), H, at, cl.L)
    want = pyoracle.frame_scan(H, at, cl.L, BOUND, MAXP)
    enc = H[2 * WIN:4 * WIN].copy()
    rig.oracle(enc, cl.slots, at + cl.head - 2 * WIN, cl.L - cl.head)
    rig.upload(1, enc)
    z = lambda k: rig.torch.zeros(k, dtype=rig.torch.int32, device="cuda")
    npk, used, status, pk = z(cl.n), z(cl.n), z(cl.n), z(cl.n * MAXP)
    frame = {"off": T(offsets(cl.addr, base).view(np.int64)), "len": T(cl.L.astype(np.uint32).view(np.int32)),
             "bound": BOUND, "max_packets": MAXP, "npk": npk, "used": used, "status": status, "pkt_len": pk}
    off = T(offsets(cl.addr + cl.head, base).view(np.int64))
    ln = T((cl.L - cl.head).astype(np.uint32).view(np.int32))
    if cl.ids is None:
        c.crypt_range_frame(cl.first, view, off, ln, frame)
    elif cl.call == "grouped":
        c.crypt_grouped_frame(view, off, ln, T(cl.ids.view(np.int32)), frame)
    else:
        c.crypt_grouped_declared(view, off, ln, T(cl.ids.view(np.int32)), cl.decl, frame=frame)
    rig.verify(what, cl.slot_hi)
    got = [t.cpu().numpy().view(np.uint32) for t in (npk, used, status)] + \
          [pk.cpu().numpy().view(np.uint32).reshape(cl.n, MAXP)]
    msgs = [m for m in (frame_report(w, g, nm) for w, g, nm in zip(want, got, ("npk", "used", "status", "pkt_len")))
            if m]
    assert not msgs, f"{what}: " + "; ".join(msgs)
    # the cases the framing is there for were there
    assert (want[2] == 2).any() and (want[0] > MAXP).any()


def _run_form(rig, form, shape, mode):
    io = FORMS[form][0]
    n = shape.n(rig.cus)
    fam = family(shape.call, shape.first, n, rig.cus, io)
    assert fam == shape.family, f"{shape.id}: {n} entries on {rig.cus} CUs run the {fam} family, not {shape.family}"
    with rig.session():
        for li in range(n_launches(shape)):
            cl = build(shape, rig.cus, form, li, rig.a, rig.cap)
            what = f"{form} {shape.id} ({shape.family}) base={mode} launch {li}: k={cl.k} ({cl.kind}) s={cl.s}"
            (_run_frame_launch if form == "frame" else _run_launch)(rig, cl, mode, what)


def _params(form):
    _, _, shapes, modes = FORMS[form]
    return [pytest.param(sh, mode, id=f"{sh.id}-{mode}") for sh in shapes for mode in modes]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,mode", _params("inplace"))
def test_inplace(rig, shape, mode):
    """zrc4_crypt_range / zrc4_crypt / zrc4_crypt_grouped /
    zrc4_crypt_grouped_declared on every family, every base mode."""
    _run_form(rig, "inplace", shape, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,mode", _params("keystream"))
def test_keystream(rig, shape, mode):
    """zrc4_keystream_range / zrc4_keystream_grouped (declared and not): the
    spans hold random bytes beforehand, so a read of the destination shows; the
    persistent shapes run span_fill_kernel in front."""
    _run_form(rig, "keystream", shape, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,mode", _params("to-a"))
def test_crypt_to_destinations_across_the_line(rig, shape, mode):
    """zrc4_crypt_to_range / zrc4_crypt_to_grouped, the destination layout
    across A, the sources in a tensor of their own, half the entries congruent
    mod 16 with their source; the persistent shapes run span_copy_kernel in
    front."""
    _run_form(rig, "to-a", shape, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,mode", _params("to-b"))
def test_crypt_to_shared_source_across_the_line(rig, shape, mode):
    """Broadcast: every entry reads a prefix of ONE source span that has A
    inside it; the destinations lie above A + 64 KiB, half of them congruent."""
    _run_form(rig, "to-b", shape, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,mode", _params("to-c"))
def test_crypt_to_byte_path(rig, shape, mode):
    """As the first out-of-place test with every source start incongruent to
    its destination mod 16."""
    _run_form(rig, "to-c", shape, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,mode", _params("frame"))
def test_fused_frame(rig, shape, mode):
    """zrc4_crypt_range_frame / zrc4_crypt_grouped_frame / declared with a
    frame; frame->off goes through the same base mode, and for the small
    splits the straddler's block starts below A and its tail at or above."""
    _run_form(rig, "frame", shape, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,mode", _params("rounds"))
def test_rounds(rig, shape, mode):
    """zrc4_crypt_to_range_rounds / zrc4_crypt_to_grouped_rounds, rounds = 3
    (_build_rounds), against the oracle's three successive calls."""
    _run_form(rig, "rounds", shape, mode)


# ------------------------------------------------ the other base + offset kernels
KSA_EDGES = np.array([0, 1, 2, 4, 8, 16, 31, 32, 33, 48, 49, 50, 63, 64, 65, 128, 255, 256, 257, 300])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["low", "near", "above"])
@pytest.mark.parametrize("how", ["range-fs0", "range-fs3", "ids"])
def test_ksa_keys_across_the_line(rig, how, mode):
    """zrc4_ksa_range / zrc4_ksa, 600 keys: key i is the key_len[i] bytes from
    A - (i % 40) - 1 on (keys are only read, so they overlap; all but the
    empty and the shortest cross A), the lengths from test_ksa_soak's edge
    list, so the register, LDS-window and per-step fetch paths each cross."""
    from zsummerx_amd import Context
    n, cap = 600, 1024
    rng = np.random.default_rng(31)
    klen = np.concatenate([KSA_EDGES, rng.choice(KSA_EDGES, n - KSA_EDGES.size)]).astype(np.uint32)
    addr = rig.a - (np.arange(n) % 40) - 1
    assert ((addr < rig.a) & (addr + klen > rig.a)).sum() > n // 2
    slots = {"range-fs0": np.arange(n), "range-fs3": 3 + np.arange(n), "ids": rng.permutation(cap)[:n]}[how]
    with rig.session() as H, Context(0, cap) as c:
        view, base = rig.view(mode)
        ob = pyoracle.Batch(n)
        ob.make_sbox(H, rig.idx(addr).astype(np.uint64), klen)
        osb, ox, oy = ob.states()
        koff, kl = rig.T(offsets(addr, base).view(np.int64)), rig.T(klen.view(np.int32))
        if how == "ids":
            c.ksa(kl, koff, view, ids=rig.T(slots.astype(np.uint32).view(np.int32)))
        else:
            c.ksa_range(int(slots[0]), kl, koff, view)
        c.sync()
        gsb, gx, gy = c.get_states(0, cap)
        bad = np.flatnonzero((gsb[slots] != osb).any(axis=1) | (gx[slots] != ox) | (gy[slots] != oy))
        assert bad.size == 0, (how, mode, bad[:8].tolist(), klen[bad[:8]].tolist(), int(bad.size))
        msg = rig.windows_report()
        assert not msg, f"ksa {how} base={mode}: {msg}"


def _ring_entries(rig, rng, rings, line_ring):
    """(rid, pos, len) over `rings` (ring ids from the arena's start): three
    plain reads and one wrapped read per ring; with line_ring, also one wrapped
    read of that ring and one of the ring below it, so placed that A and A - 1
    are among the bytes used."""
    cap = RING_CAP
    rid, pos, ln = [], [], []
    for r in rings:
        for p in (5000, 300000, 600000):
            rid.append(r), pos.append(p + int(rng.integers(0, 64))), ln.append(int(rng.integers(100, 3001)))
        back = int(rng.integers(1, 2001))
        rid.append(r), pos.append(cap - back), ln.append(back + int(rng.integers(1, 2001)))
    if line_ring is not None:
        pa = (rig.a - rig.start) % cap                          # A's position in its ring
        if pa < cap // 2:
            rid.append(line_ring), pos.append(cap - 300), ln.append(300 + pa + 500)
        else:
            rid.append(line_ring), pos.append(pa - 200), ln.append(cap - (pa - 200) + 300)
        rid.append(line_ring - 1), pos.append(cap - 400), ln.append(900)
    order = rng.permutation(len(rid))
    return tuple(np.array(v, np.int64)[order] for v in (rid, pos, ln))


RING_CAP = 1 << 20


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["line-in-ring", "payload-across-line-near", "payload-across-line-above"])
def test_xor_ring_across_the_line(rig, case):
    """zrc4_xor_ring, ring_cap = 1 MiB, the ring pointer at the arena's start,
    so every ring id used has rid * ring_cap >= 2^32.  line-in-ring: the ring
    that holds A and the one below it are read wrapped (pos + len > ring_cap)
    with A and A - 1 among the used bytes, the payload in a tensor of its own.
    payload-across-line: the payload spans lie across A (base near A, and
    above it: wrapped offsets), the rings further off.  The payload against
    numpy; the used ring bytes are zero and nothing else changed."""
    cap = RING_CAP
    rng = np.random.default_rng(41)
    ra = (rig.a - rig.start) // cap                                # the ring that holds A
    assert (ra - 3) * cap >= G4
    in_ring = case == "line-in-ring"
    with rig.session() as H:
        rid, pos, ln = _ring_entries(rig, rng, [ra - 3, ra - 2, ra + 2] + [ra + 1] * in_ring, ra if in_ring else None)
        n = rid.size
        used = np.concatenate([rig.start + rid[i] * cap + (pos[i] + np.arange(ln[i])) % cap for i in range(n)])
        assert np.unique(used).size == used.size and (np.abs(used - rig.a) < WIN).all()
        keystream = H[rig.idx(used)].copy()
        gaps = rng.integers(0, 20, n)
        if in_ring:
            assert (used == rig.a).any() and (used == rig.a - 1).any()
            at = np.cumsum(gaps + np.concatenate([[0], ln[:-1]]))
            want = rng.integers(0, 256, int(at[-1] + ln[-1]) + 16, dtype=np.uint8)
            payload = rig.T(want)
            want[span_bytes(at, ln)] ^= keystream
            off = rig.T(at.astype(np.uint64).view(np.int64))
        else:
            addr = span_layout(ln, gaps, n // 2, 33, rig.a)
            check_spans(addr, ln, rig.a)
            assert not np.isin(span_bytes(addr, ln), used).any()
            H[rig.idx(span_bytes(addr, ln))] ^= keystream
            payload, base = rig.view(case.rsplit("-", 1)[1])
            off = rig.T(offsets(addr, base).view(np.int64))
        H[rig.idx(used)] = 0
        rig.c.xor_ring(rig.arena, cap, rig.T(rid.astype(np.uint32).view(np.int32)),
                       rig.T(pos.astype(np.uint32).view(np.int32)), payload, off,
                       rig.T(ln.astype(np.uint32).view(np.int32)))
        rig.c.sync()
        if in_ring:
            assert np.array_equal(payload.cpu().numpy(), want), "xor_ring: the payload differs"
        msg = rig.windows_report()
        assert not msg, f"xor_ring {case}: {msg}"


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["low", "above"])
def test_frame_scan_across_the_line(rig, mode):
    """zrc4_frame_scan over 600 buffers laid out across A as the in-place
    calls' spans, one launch per straddler position and a few splits, against
    the oracle scan; the buffers are only read."""
    shape = Shape("scan-600", "range", 0, lambda cus: 600, "-")
    rng = np.random.default_rng(51)
    with rig.session() as H:
        view, base = rig.view(mode)
        for li, s in enumerate((1, 3, 4, 17, 65, -1)):
            e = entries(shape, rig.cus, rng, li, rig.cap)
            L, gaps = lengths(rng, e, 0, BUDGET)
            s = int(L[e.k]) - 1 if s < 0 else s
            addr = span_layout(L, gaps, e.k, s, rig.a)
            check_spans(addr, L, rig.a)
            at = rig.idx(addr)
            _packets(rng, H, at, L)
            rig.upload(1)
            want = pyoracle.frame_scan(H, at, L, BOUND, MAXP)
            z = lambda k: rig.torch.zeros(k, dtype=rig.torch.int32, device="cuda")
            npk, used, status, pk = z(e.n), z(e.n), z(e.n), z(e.n * MAXP)
            rig.c.frame_scan(view, rig.T(offsets(addr, base).view(np.int64)),
                             rig.T(L.astype(np.uint32).view(np.int32)), BOUND, npk, used, status, pk, MAXP)
            rig.c.sync()
            got = [t.cpu().numpy().view(np.uint32) for t in (npk, used, status)] + \
                  [pk.cpu().numpy().view(np.uint32).reshape(e.n, MAXP)]
            msgs = [m for m in (frame_report(w, g, nm)
                                for w, g, nm in zip(want, got, ("npk", "used", "status", "pkt_len"))) if m]
            msgs.append(rig.windows_report())
            msgs = [m for m in msgs if m]
            assert not msgs, f"frame_scan base={mode} k={e.k} s={s}: " + "; ".join(msgs)
            assert (want[0] > MAXP).any() and (want[2] == 2).any()


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["range-fs3", "ids"])
def test_state_records_across_the_line(rig, how):
    """zrc4_export_states / zrc4_import_states, 600 slots.  The record buffer
    starts 256 * 300 + 128 bytes below a multiple of 2^32 (16-aligned), so
    record 300 has the line inside it; the xy array starts 600 bytes below
    another, so the line falls between its words 299 and 300.  range-fs3:
    records across A, xy across A3; ids: records across A3, xy across A.
    Export, compare with zrc4_get_states, import into a second context,
    compare; nothing but the records changed in the windows."""
    from zsummerx_amd import Context
    n, cap = 600, 1024
    rng = np.random.default_rng(61)
    ids = None if how == "range-fs3" else rng.permutation(cap)[:n]
    slots = 3 + np.arange(n) if ids is None else ids
    first = 3 if ids is None else 0
    rec_line, xy_line = (rig.a, rig.a3) if ids is None else (rig.a3, rig.a)
    sb_at, xy_at = rec_line - 256 * 300 - 128, xy_line - 2 * 300
    assert sb_at % 16 == 0 and xy_at % 2 == 0
    keys = rng.integers(0, 256, 16 * cap, dtype=np.uint8)
    koff, klen = np.arange(cap, dtype=np.uint64) * 16, np.full(cap, 16, np.uint32)
    d_ids = None if ids is None else rig.T(ids.astype(np.uint32).view(np.int32))
    with rig.session() as H, Context(0, cap) as c1, Context(0, cap) as c2:
        c1.ksa_range(0, rig.T(klen.view(np.int32)), rig.T(koff.view(np.int64)), rig.T(keys))
        c1.sync()
        sb, x, y = c1.get_states(0, cap)
        c1.export_states(int(sb_at), int(xy_at), ids=d_ids, first_slot=first, n=n)
        c1.sync()
        H[rig.idx(sb_at + np.arange(256 * n))] = sb[slots].reshape(-1)
        xy = (x[slots].astype(np.uint16) | (y[slots].astype(np.uint16) << 8))
        H[rig.idx(xy_at + np.arange(2 * n))] = xy.view(np.uint8)
        msg = rig.windows_report()
        assert not msg, f"export_states {how}: {msg}"
        before = c2.get_states(0, cap)
        c2.import_states(int(sb_at), int(xy_at), ids=d_ids, first_slot=first, n=n)
        c2.sync()
        gsb, gx, gy = c2.get_states(0, cap)
        bad = np.flatnonzero((gsb[slots] != sb[slots]).any(axis=1) | (gx[slots] != x[slots]) | (gy[slots] != y[slots]))
        assert bad.size == 0, f"import_states {how}: records {bad[:8].tolist()} of {bad.size} differ"
        rest = np.setdiff1d(np.arange(cap), slots)
        assert all(np.array_equal(g[rest], b[rest]) for g, b in zip((gsb, gx, gy), before)), \
            f"import_states {how}: a slot outside the call changed"
        msg = rig.windows_report()
        assert not msg, f"import_states {how}: {msg}"
