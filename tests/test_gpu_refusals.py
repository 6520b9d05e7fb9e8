"""Every break of the bucket contract on every kernel family and I/O form.

The grouped calls (include/zrc4.h:114-145) take a promise: every busy entry of
a 256-entry bucket names one 256-slot group, no slot appears twice, no two
buckets name one group, a declared group is the true one.  The header says what
a broken promise costs; this module walks every break through

  form     in place (zrc4_crypt_grouped / _declared), write-only
           (zrc4_keystream_grouped), out of place (zrc4_crypt_to_grouped),
           rounds (zrc4_crypt_to_grouped_rounds, 3 rounds);
  declared bucket_group given or not;
  regime   by bucket count, from the device's CU count: 4 (window kernel; the
           rounds form has none and runs the half-group kernel), 33 (half-group
           / declared-half), CUs/2 + 1 (whole-group / declared), CUs + 1 (the
           persistent kernel behind span_fill_kernel / span_copy_kernel, above
           256 buckets decl_check_kernel too; the rounds form's host-split
           path).

One call carries every break, each in a bucket of its own, on spare groups no
other bucket of the call names (a broken bucket may block a valid bucket of a
group it names, zrc4.h:132-140, and decl_check_kernel blocks the groups a
disagreeing bucket's ids name, zrc4.h:163-167):

  M  two groups: slots of H1 and one slot of H2;
  T  a slot of H3 in two entries, both with bytes;
  Z  a slot of H4 in a second entry whose length is 0 (in every round);
  P  two buckets naming H5, 64 disjoint slots each, both in both halves of the
     group and in the same 32 dword columns;
  D  (declared) declared H6, its one busy entry names H7;
  I  (declared) declared ZRC4_IDLE_SLOT, one busy entry of H8;
  J  (declared rounds form on the host-split path) declared ZRC4_IDLE_SLOT,
     names a slot, every length 0: idle there, no break;
  R  a valid bucket with the ids capacity + 77 and 0xFFFFFFFE, 193-byte spans;
  W  (window kernel) two groups, the one of its lowest busy entry being the
     group of the valid bucket w next to it, in the dword columns w uses;
  B  bystanders: 1-8 busy entries, lengths from SHORT (0 included), one of them
     with a busy entry of length 0; every bucket has idle entries with spans;
  -  a bucket with no busy entry.

Four buckets cannot hold them all, so the 4-bucket regime makes three calls on
one context (M T B -, Z P P R, and W w with D I or two bystanders).

The oracle is pyoracle.Batch (KSA, then `crypt` over the gathered sources, over
zeros for the write-only form), every destination byte of every call is
compared, every state of the context after every call, and the streams are
continued by a crypt_range at the end.  A second call with the same ids, every
break but R repaired, follows each call: whatever a refused call left behind
(claims, slot tables) would show there.

test_generator_* check the generator on the CPU.  What the tests make of three
libraries with a refusal taken out is in profiles/refusals/sensitivity.log."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import pyoracle
from dispatch_model import family
from gpu_support import (FILL, SHORT, assert_equal, check_continues, check_states, cu_count, disjoint, layout, seeded,
                         sources)
from gpu_support import torch_cuda  # noqa: F401
from zsummerx_amd import ZRC4Error
from zsummerx_amd._capi import IDLE_SLOT

gpu = pytest.mark.gpu

FORMS = {"inplace": 0, "keystream": 1, "to": 2, "rounds": 3}       # CryptIo of zrc4_plan.hpp
REGIMES = ("small", "half", "whole", "persistent")
ROUNDS = 3
SPARE = 16                              # groups of the arena beyond one per bucket
BREAKS = "MTZPDIW"                      # kinds whose busy entries have at least 16 bytes
NONE, RUN, REFUSED, PAIR = 0, 1, 2, 3   # what the test expects of an entry

# dword column q of the window kernel holds the group lanes (q >> 5) * 128 + (q & 31) + 32 b, b = 0..3
# (zrc4_win.hpp, kb); lanes 0..127 are the first half of the half-group and persistent kernels' claims
PAIR_COLS = list(range(16)) + list(range(32, 48))


def _pair_lanes(bs):
    return np.array([(q >> 5) * 128 + (q & 31) + 32 * b for q in PAIR_COLS for b in bs], dtype=np.uint32)


def n_buckets(regime, cus):
    return {"small": 4, "half": 33, "whole": cus // 2 + 1, "persistent": cus + 1}[regime]


def expected_family(form, regime, declared, cus):
    """The family each regime is there for (the issue's table), stated without family()."""
    nb = n_buckets(regime, cus)
    if regime == "small":
        fam = "half" if form == "rounds" else "win"
    elif regime == "persistent":
        fam = "stream"
    else:
        fam = "half" if 2 * nb <= cus else "whole"
    return "decl" if declared and fam in ("half", "whole") and nb <= 256 else fam


def one_launch(form, regime):
    """A rounds call is one launch, judged once (zrc4.h:281-289), except on the
    host-split path: one kIoTo launch per round, each judged as a one-round
    call by that round's lengths (zrc4.h:316-320)."""
    return not (form == "rounds" and regime == "persistent")


def plans(form, regime, declared, nb):
    """The kind of every bucket of every call."""
    rounds = form == "rounds"
    if regime == "small":
        third = ([] if rounds else ["W", "w"]) + (["D", "I"] if declared else [])
        return [list("MTB-"), list("ZPPR")] + ([(third + ["B", "B"])[:4]] if third else [])
    brk = list("MTZPPR") + (list("DI") if declared else [])
    if rounds and declared and regime == "persistent":
        brk.insert(4, "J")
    kinds = ["B"] * nb
    at = np.linspace(0, nb - 1, len(brk)).round().astype(int)      # the first, the last, the others between
    assert len(set(at.tolist())) == len(brk)
    for kind, a in zip(brk, at):
        kinds[a] = kind
    assert kinds[1] == "B"
    kinds[1] = "-"
    return [kinds]


def build_call(rng, form, regime, declared, kinds, cap):
    """One call's tables.  ids / groups break the contract, ids_fixed /
    groups_fixed are the same with every break but R repaired."""
    nb, n = len(kinds), 256 * len(kinds)
    R = ROUNDS if form == "rounds" else 1
    free = rng.permutation(cap // 256).tolist()
    ids = np.full(n, IDLE_SLOT, dtype=np.uint32)
    fixed = ids.copy()
    groups = np.full(nb, IDLE_SLOT, dtype=np.uint32)
    gfixed = groups.copy()
    L = np.zeros((R, n), dtype=np.uint32)
    role = np.zeros(n, dtype=np.int8)

    def place(b, slots, fixed_slots, kind, what, lowest_first=False):
        k = len(slots)
        pos = 256 * b + rng.permutation(256)[:k]
        if lowest_first:
            pos = np.sort(pos)
        ids[pos], fixed[pos] = slots, fixed_slots
        lens = SHORT[rng.integers(0, SHORT.size, (R, k))]
        L[:, pos] = np.maximum(lens, 16) if kind in BREAKS else lens
        role[pos] = what
        return pos

    zero_len_done = False
    w_lanes = None
    pair_group = None
    for b, kind in sorted(enumerate(kinds), key=lambda bk: bk[1] == "W"):     # W after its bystander w
        if kind in "Bw":
            g = free.pop()
            groups[b] = gfixed[b] = g
            if kind == "w":                          # lanes l with l ^ 32 and l ^ 64 unused
                pick = np.sort(rng.permutation(64)[:4])
                lanes = w_lanes = ((pick >> 5) << 7) | (pick & 31)
            else:
                lanes = rng.permutation(256)[:int(rng.integers(2, 9) if not zero_len_done else rng.integers(1, 9))]
            s = g * 256 + lanes
            pos = place(b, s, s, kind, RUN)
            if kind == "B" and not zero_len_done:
                L[:, pos[0]] = 0                     # a busy entry with no bytes in any round
                L[:, pos[1]] = np.maximum(L[:, pos[1]], 1)
                zero_len_done = True
        elif kind == "M":
            h1, h2 = free.pop(), free.pop()
            p = rng.permutation(256)[:6]
            groups[b] = gfixed[b] = h1
            place(b, np.append(h1 * 256 + p[:5], h2 * 256 + p[5]), h1 * 256 + p, kind, REFUSED)
        elif kind == "T":
            h = free.pop()
            p = rng.permutation(256)[:5]
            groups[b] = gfixed[b] = h
            place(b, h * 256 + np.append(p[:4], p[0]), h * 256 + p, kind, REFUSED)
        elif kind == "Z":
            h = free.pop()
            p = rng.permutation(256)[:4]
            groups[b] = gfixed[b] = h
            judged_once = form == "rounds" and one_launch(form, regime)
            pos = place(b, h * 256 + np.append(p, p[1]), np.append(h * 256 + p, IDLE_SLOT), kind,
                        REFUSED if judged_once else RUN)
            L[:, pos[-1]] = 0
            role[pos[-1]] = NONE
        elif kind == "P":
            first = pair_group is None
            if first:
                pair_group = free.pop()
            lanes = _pair_lanes((0, 1) if first else (2, 3))
            groups[b] = pair_group
            gfixed[b] = pair_group if first else free.pop()
            place(b, pair_group * 256 + lanes, gfixed[b] * 256 + lanes, kind, PAIR)
        elif kind in "DIJ":
            h = free.pop()
            groups[b] = free.pop() if kind == "D" else IDLE_SLOT
            gfixed[b] = IDLE_SLOT if kind == "J" else h
            s = np.array([h * 256 + int(rng.integers(256))])
            pos = place(b, s, s, kind, NONE if kind == "J" else REFUSED)
            if kind == "J":
                L[:, pos] = 0
        elif kind == "R":
            g = free.pop()
            groups[b] = gfixed[b] = g
            s = g * 256 + rng.permutation(256)[:4]
            place(b, s, s, kind, RUN)
            bad = np.array([cap + 77, 0xFFFFFFFE], dtype=np.uint32)
            pos = place(b, bad, bad, kind, NONE)
            L[:, pos] = 193
        elif kind == "W":
            h, gw = free.pop(), int(groups[kinds.index("w")])
            a, z = int(w_lanes[0]), int(w_lanes[-1])
            groups[b] = gfixed[b] = h
            place(b, np.array([gw * 256 + (a ^ 32), h * 256 + a, h * 256 + z, h * 256 + (a ^ 64), gw * 256 + (z ^ 32)]),
                  h * 256 + np.array([a ^ 32, a, z, a ^ 64, z ^ 32]), kind, REFUSED, lowest_first=True)
        else:
            assert kind == "-"
    for b in range(nb):                              # idle entries with spans that must stay as they are
        idle = 256 * b + np.flatnonzero(ids[256 * b: 256 * b + 256] == IDLE_SLOT)
        L[:, idle[[1, -2]]] = 17
    L = L.reshape(-1)
    doff, size = layout(L, nb % 16)
    soff, ssize = sources(rng, L, doff)
    return SimpleNamespace(kinds=kinds, nb=nb, n=n, R=R, ids=ids, ids_fixed=fixed, groups=groups, groups_fixed=gfixed,
                           L=L, doff=doff, size=size, soff=soff, ssize=ssize, role=role)


def build_case(form, regime, declared, cus):
    nb = n_buckets(regime, cus)
    cap = (nb + SPARE) * 256
    rng = np.random.default_rng(1000 * FORMS[form] + 100 * REGIMES.index(regime) + 10 * declared + 31)
    calls = [build_call(rng, form, regime, declared, kinds, cap) for kinds in plans(form, regime, declared, nb)]
    return SimpleNamespace(form=form, regime=regime, declared=declared, cus=cus, cap=cap, calls=calls,
                           family=expected_family(form, regime, declared, cus))


# ------------------------------------------------------------------ CPU checks of the generator

def diagnose(k, b, ids, groups, declared, cap, judged_once):
    """What bucket b breaks, read from the tables alone.  judged_once: busy by
    id, whatever the lengths (a one-launch rounds call, zrc4.h:284-287)."""
    w = slice(256 * b, 256 * b + 256)
    idb = ids[w]
    Lb = k.L.reshape(k.R, k.n)[:, w]
    found = set()
    if ((idb >= cap) & (idb != IDLE_SLOT)).any():
        found.add("range")
    named = idb < cap
    busy = named & ((Lb != 0).any(axis=0) | judged_once)
    slots, count = np.unique(idb[busy], return_counts=True)
    if (count > 1).any():
        found.add("twice")
    if np.unique(idb[busy] >> 8).size > 1:
        found.add("two groups")
    if declared and busy.any():
        if groups[b] == IDLE_SLOT:
            found.add("declared idle")
        elif (idb[busy] >> 8 != groups[b]).any() and np.unique(idb[busy] >> 8).size == 1:
            found.add("mismatch")
    return found


MEANT = {"M": {"two groups"}, "T": {"twice"}, "D": {"mismatch"}, "I": {"declared idle"}, "W": {"two groups"},
         "R": {"range"}, "Z": set(), "P": set(), "B": set(), "w": set(), "-": set(), "J": set()}


@pytest.mark.parametrize("cus", [256, 64])
@pytest.mark.parametrize("declared", [False, True], ids=["undeclared", "declared"])
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("form", list(FORMS))
def test_generator_breaks_the_contract_as_meant(form, regime, declared, cus):
    """Every call of the matrix, as built for 256 and for 64 CUs: each bucket
    breaks what its kind says and nothing else, a group is named by two buckets
    only where that is the break (P P, W w), destinations are pairwise
    disjoint over all rounds and lie in a buffer of their own, break entries
    have 16 bytes and more, and the regime reaches its family."""
    case = build_case(form, regime, declared, cus)
    io = FORMS[form]
    if cus == 256:
        want = {"small": "half" if form == "rounds" else "win", "half": "half", "whole": "whole",
                "persistent": "stream"}[regime]
        if declared and want in ("half", "whole"):
            want = "decl"
        assert case.family == want
    seen = set()
    for k in case.calls:
        assert family("declared" if declared else "grouped", 0, k.n, cus, io) == case.family
        assert k.n * k.R <= 0xFFF00000 and k.nb == n_buckets(regime, cus)
        seen |= set(k.kinds)
        judged_once = form == "rounds" and one_launch(form, regime)
        for ids, groups, fixed in ((k.ids, k.groups, False), (k.ids_fixed, k.groups_fixed, True)):
            named_by = {}
            for b, kind in enumerate(k.kinds):
                found = diagnose(k, b, ids, groups, declared, case.cap, judged_once)
                meant = set(MEANT[kind]) if not fixed or kind == "R" else set()
                if kind == "Z" and judged_once and not fixed:
                    meant = {"twice"}
                assert found == meant, (kind, b, found, fixed)
                idb = ids[256 * b: 256 * b + 256]
                gs = set((idb[idb < case.cap] >> 8).tolist())
                if declared and groups[b] != IDLE_SLOT:
                    assert groups[b] < case.cap // 256
                    gs.add(int(groups[b]))
                for g in gs:
                    named_by.setdefault(g, []).append(kind)
            shared = sorted("".join(sorted(v)) for v in named_by.values() if len(v) > 1)
            assert shared == ([] if fixed else ["PP"] * ("P" in k.kinds) + ["Ww"] * ("W" in k.kinds)), shared
        assert disjoint(k.doff, k.L) and int((k.doff + k.L).max()) <= k.size
        assert int((k.soff + k.L).max()) <= k.ssize                # (sources: a buffer of their own, read only)
        Lr = k.L.reshape(k.R, k.n)
        brk = (k.role == REFUSED) | (k.role == PAIR)
        assert brk.any() and (Lr[:, brk] >= 16).all()
        tail = np.flatnonzero((k.ids >= case.cap) & (k.ids != IDLE_SLOT))
        assert (Lr[:, tail] == 193).all()
        if "Z" in k.kinds:
            b = k.kinds.index("Z")
            idb = k.ids[256 * b: 256 * b + 256]
            slots, count = np.unique(idb[idb != IDLE_SLOT], return_counts=True)
            e = 256 * b + np.flatnonzero(idb == slots[count == 2][0])
            assert sorted((Lr[:, e] != 0).all(axis=0).tolist()) == [False, True] and (Lr[:, e].min(axis=0) == 0).any()
        if "P" in k.kinds:
            a, b = [256 * i for i, kind in enumerate(k.kinds) if kind == "P"]
            la, lb = k.ids[a: a + 256], k.ids[b: b + 256]
            la, lb = la[la != IDLE_SLOT] & 255, lb[lb != IDLE_SLOT] & 255
            col = lambda l: set((((l >> 7) << 5) | (l & 31)).tolist())
            assert la.size == lb.size == 64 and not set(la.tolist()) & set(lb.tolist())
            assert col(la) == col(lb) and len(col(la)) == 32 and set((la >> 7).tolist()) == set((lb >> 7).tolist()) == {0, 1}
        if "W" in k.kinds:
            w = k.ids[256 * k.kinds.index("w"):][:256]
            W = k.ids[256 * k.kinds.index("W"):][:256]
            W = W[W != IDLE_SLOT]
            assert W[0] >> 8 == k.groups[k.kinds.index("w")] and not set(W.tolist()) & set(w.tolist())
            col = lambda l: set(((((l & 255) >> 7) << 5) | (l & 31)).tolist())
            assert col(W) <= col(w[w != IDLE_SLOT])         # every column W would claim is one w runs
        busy = (k.ids < case.cap) & (k.role != NONE)
        d = (k.soff.astype(np.int64) - k.doff.astype(np.int64)) % 16
        assert (d[:k.n][busy] == 0).any() and (d[:k.n][busy] != 0).any()
        assert ((k.ids == IDLE_SLOT) & (Lr != 0).all(axis=0)).reshape(k.nb, 256).any(axis=1).all()
        assert ((k.role == RUN) & (Lr == 0).all(axis=0)).any() or "B" not in k.kinds
    need = set("MTZPR") | (set("DI") if declared else set()) | (set("Ww") if regime == "small" and io != 3 else set())
    assert need <= seen and "-" in seen and "B" in seen, seen


# ------------------------------------------------------------------ the GPU side

def _launch(c, form, declared, k, ids, groups, T, dst, src, s):
    bg = groups if declared else None
    off, L, tid = T(k.doff.view(np.int64)), T(k.L.view(np.int32)), T(ids.view(np.int32))
    if form == "inplace":
        if declared:
            c.crypt_grouped_declared(dst, off, L, tid, bg, stream=s)
        else:
            c.crypt_grouped(dst, off, L, tid, stream=s)
    elif form == "keystream":
        c.keystream_grouped(dst, off, L, tid, bg, stream=s)
    elif form == "to":
        c.crypt_to_grouped(src, T(k.soff.view(np.int64)), dst, off, L, tid, bg, stream=s)
    else:
        c.crypt_to_grouped_rounds(src, T(k.soff.view(np.int64)), dst, off, L, tid, k.n, k.R, bucket_group=bg, stream=s)


def _run(torch, c, ob, T, case, k, ids, groups, role, rng, expect, what):
    """One call and everything it may have touched.  role: per entry, RUN (must
    be exact), REFUSED (the table check refuses its bucket), PAIR (read off the
    result), NONE (nothing may happen)."""
    form, persistent = case.form, case.regime == "persistent"
    s = torch.cuda.current_stream()
    n, R, cap = k.n, k.R, case.cap
    base = rng.integers(0, 256, k.size, dtype=np.uint8) if form == "inplace" else np.full(k.size, FILL, dtype=np.uint8)
    src = rng.integers(0, 256, k.ssize, dtype=np.uint8)
    td, ts = T(base), T(src)
    _launch(c, form, case.declared, k, ids, groups, T, td, ts, s)
    if expect:
        # zrc4.h:121-123 ZRC4_ERR_GROUP from zrc4_sync; :141-142 an id >= capacity is ZRC4_ERR_SLOT_RANGE;
        # the group code is reported ahead of the range latch, and the report clears both (:455)
        with pytest.raises(ZRC4Error) as ei:
            c.sync(s)
        assert ei.value.code == expect, what
    c.sync(s)
    got = td.cpu().numpy()

    def start(e, a, z, so):
        """What the oracle crypts for a span that runs."""
        if form == "inplace":
            return base[a:z].copy()
        if form == "keystream":
            return np.zeros(z - a, dtype=np.uint8)
        return src[so: so + z - a].copy()

    want = base.copy()
    ranP = np.zeros((R, n), dtype=bool)
    enc = pyoracle.lib().oracle_encryption
    for r in range(R):
        Lr, do, so = k.L[r * n:(r + 1) * n], k.doff[r * n:(r + 1) * n], k.soff[r * n:(r + 1) * n]
        m = np.flatnonzero((role == RUN) & (Lr > 0) & (ids < cap))
        for e in m:
            a = int(do[e])
            want[a: a + int(Lr[e])] = start(e, a, a + int(Lr[e]), int(so[e]))
        po, pl = np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint32)
        po[ids[m]], pl[ids[m]] = do[m], Lr[m]
        ob.crypt(want, po, pl)
        for e in np.flatnonzero(((role == REFUSED) | (role == PAIR)) & (Lr > 0)):
            a, z = int(do[e]), int(do[e]) + int(Lr[e])
            sp = got[a:z]
            if role[e] == PAIR:
                # zrc4.h:125-131 two buckets naming one group: the first claimant of a part runs, and a slot is
                # all or nothing: crypted with its state advanced, or refused
                st = ob.st[int(ids[e])]
                saved = type(st).from_buffer_copy(st)
                tmp = start(e, a, z, int(so[e]))
                enc(C.byref(st), C.c_void_p(tmp.ctypes.data), z - a)
                if (sp == tmp).all():
                    ranP[r, e] = True
                    want[a:z] = tmp
                    continue
                C.memmove(C.byref(st), C.byref(saved), C.sizeof(saved))
            # A refused bucket's spans.  In place: untouched at every size (zrc4.h:121-123).  Out of place and
            # rounds: untouched with at most one bucket per CU (:243-245, :287-289), else untouched or a plain
            # copy of the source (:240-242).  Write-only: untouched with at most one bucket per CU (:195-198), else
            # untouched or zero (:193-194).  Never a mix within a span.
            allowed = [base[a:z]]
            if persistent and form == "keystream":
                allowed.append(np.zeros(z - a, dtype=np.uint8))
            if persistent and form in ("to", "rounds"):
                allowed.append(src[int(so[e]): int(so[e]) + z - a])
            assert any((sp == v).all() for v in allowed), (what, k.kinds[e // 256], e, r, sp[:16], base[a:a + 16])
            want[a:z] = sp
    pair = np.flatnonzero(role == PAIR)
    if pair.size:
        assert (k.L.reshape(R, n)[:, pair] > 0).all()
        if one_launch(form, case.regime):            # zrc4.h:281-284 decided once per launch, not per round
            assert (ranP[:, pair] == ranP[0, pair]).all(), (what, "a slot ran in some rounds only")
        # each part of the group goes to one bucket, and both buckets name slots of every part
        assert (~ranP[:, pair]).any(axis=1).all(), (what, "nobody was refused")
        assert ((ranP[:, pair]).sum() + (~ranP[:, pair]).sum()) == R * pair.size
    # R's two spans and every idle entry's: untouched (zrc4.h:141-142, :191-192, :237-239); bystanders exact;
    # guards, and everything else outside the spans that ran: as they were (:190, :229)
    assert_equal(got, want, what)
    assert_equal(ts.cpu().numpy(), src, what + ": source changed")                # zrc4.h:228
    check_states(c, ob, cap)                        # refused buckets' slots keep their states (:121-123, :194, :242)
    return ranP


def _seed(case):
    return 77000 + 1000 * FORMS[case.form] + 100 * REGIMES.index(case.regime) + case.declared


@gpu
@pytest.mark.parametrize("declared", [False, True], ids=["undeclared", "declared"])
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("form", list(FORMS))
def test_refusals(built, torch_cuda, form, regime, declared):
    """One cell of the matrix (module docstring): every call of the case with
    its breaks (ZRC4_ERR_GROUP), then repaired (ZRC4_ERR_SLOT_RANGE where R is
    in the call, else nothing), then every stream continued."""
    torch = torch_cuda
    cus = cu_count(torch)
    case = build_case(form, regime, declared, cus)
    rng = np.random.default_rng(_seed(case))
    c, ob, T = seeded(torch, _seed(case) + 1, case.cap)
    with c:
        for i, k in enumerate(case.calls):
            assert family("declared" if declared else "grouped", 0, k.n, cus, FORMS[form]) == case.family
            what = f"{form} {regime} call {i} ({''.join(x for x in k.kinds if x != 'B')})"
            _run(torch, c, ob, T, case, k, k.ids, k.groups, k.role, rng, -7, what)
            # the same ids repaired: every bucket valid, R kept.  Everything runs, so nothing of the refused
            # call lingers (claims carry a per-call tag, zrc4.h:142-143)
            fixed_role = np.where(k.ids_fixed < case.cap, RUN, NONE).astype(np.int8)
            fixed_role[(k.role == NONE) & (k.ids_fixed < case.cap) & (k.ids == k.ids_fixed)] = NONE       # J
            _run(torch, c, ob, T, case, k, k.ids_fixed, k.groups_fixed, fixed_role, rng, -5 if "R" in k.kinds else 0,
                 what + ", repaired")
        check_continues(torch, c, ob, T, case.cap, rng)


@gpu
@pytest.mark.parametrize("regime", ["half", "whole"])
def test_rounds_declared_idle_bucket_of_zero_lengths_is_refused(built, torch_cuda, regime):
    """A one-launch rounds call judges a bucket busy by its ids (zrc4.h:284-287):
    a bucket declared idle that names a slot is refused even if all its lengths
    are zero.  The call's only break is such a bucket: ZRC4_ERR_GROUP, no byte
    of it written (it has none), its slot's state unchanged, every other bucket
    exact.  (On the host-split path the same bucket is idle: J in test_refusals.)"""
    torch = torch_cuda
    cus = cu_count(torch)
    nb = n_buckets(regime, cus)
    case = SimpleNamespace(form="rounds", regime=regime, declared=True, cus=cus, cap=(nb + SPARE) * 256)
    rng = np.random.default_rng(88000 + nb)
    kinds = ["B"] * nb
    kinds[1], kinds[nb // 2] = "-", "J"
    k = build_call(rng, "rounds", regime, True, kinds, case.cap)
    assert family("declared", 0, k.n, cus, 3) == "decl"
    b = nb // 2
    e = 256 * b + np.flatnonzero(k.ids[256 * b:][:256] != IDLE_SLOT)
    assert e.size == 1 and k.groups[b] == IDLE_SLOT and (k.L.reshape(k.R, k.n)[:, e] == 0).all()
    c, ob, T = seeded(torch, 88001 + nb, case.cap)
    with c:
        _run(torch, c, ob, T, case, k, k.ids, k.groups, k.role, rng, -7, f"declared idle, all lengths zero, {regime}")
        k.groups_fixed[b] = k.ids[e[0]] >> 8         # declared as what it names: a valid bucket with nothing to do
        _run(torch, c, ob, T, case, k, k.ids, k.groups_fixed, k.role, rng, 0, "the same, declared truly")
        check_continues(torch, c, ob, T, case.cap, rng)
