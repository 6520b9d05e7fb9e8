"""Fused decrypt + frame (zrc4_crypt_range_frame, zrc4_crypt_grouped_frame) on
every kernel launch_crypt (zsummerx_amd/csrc/zrc4.hip) can pick for them, with
the slot states checked afterwards.

The recv path of a session (src/frame/session.cpp:313-371) decrypts the fresh
tail of its receive block and then frames the WHOLE block; the fused entry
points do both in one launch, and every kernel has an epilogue and a state
write-back of its own.  Each case here is a deterministic batch built by
make_case() -- blocks with the framing's edge cases placed on purpose -- run
twice on one context (the second call continues every keystream from the
written-back state) and compared bit for bit with the oracle
(oracle/rc4_oracle.c through pyoracle): every payload byte, every framing
output of every entry (padding entries included), every state of the arena.

The generator itself is checked on the CPU (test_generator_builds_every_case).
"""
from types import SimpleNamespace

import numpy as np
import pytest

import pyoracle
from dispatch_model import kernel_class
from frame_support import BOUND, frame_report, payload_report
from gpu_support import cu_count, dev

IDLE = 0xFFFFFFFF                       # ZRC4_IDLE_SLOT (include/zrc4.h)
SENT = 0xA5A5A5A5                       # prefill of every framing output
KINDS = ["A", "B", "C1", "C2", "C3", "D1", "D2", "D3", "E1", "E2", "F"]
K = {name: i + 1 for i, name in enumerate(KINDS)}          # 0: an ordinary block
PER_CASE = 8                            # every ingredient at least this often in a case


# ------------------------------------------------------------ the generator
def make_case(n, seed, bound=BOUND, maxp=8, idle=None, busy=None, marked=(), batch=None):
    """n receive blocks as onRecv sees them.  Returns a namespace with
      plain           the plaintext buffer (blocks at odd spacings, random gaps),
      inp             the device input: plain with each entry's fresh tail
                      [toff, toff + tlen) encrypted by that entry's oracle stream,
      off / len       the frame spans (whole blocks),
      toff / tlen     the crypt spans (the fresh tails),
      keys            uint8[n, 16], entry i's key (None when `batch` is given),
      batch           pyoracle.Batch(n), stream i advanced past entry i's tail,
      kind / masks    the ingredient of each entry, one boolean mask per ingredient,
      want            pyoracle.frame_scan over plain: npk, used, status, pkt_len.

    Blocks: proto4z packets of 6..64 bytes up to a target of 0..200 bytes
    (2 %: 1 000..3 000, past the 64-byte block loop and the window kernel's
    2 KiB chunk), usually cut 0..20 bytes short; an earlier iteration decrypted
    a random head of each.  Ingredients, each placed PER_CASE times in the case
    and once in every 256-entry chunk listed in `marked`:
      A   every byte decrypted earlier (tlen == 0, len > 0), >= 2 whole packets;
          also every entry of `idle` (a grouped batch's padding)
      B   an empty block (len == 0)
      C1-3 the decrypted head ends 1, 2, 3 bytes into a packet's length field
      D1  a length field below 6 (status 2)
      D2  a length field above bound (status 2)
      D3  a length field in (bound - used, bound] (status 1, proto4z.h:704-748)
      E1  1..5 bytes left after the last whole packet
      E2  a packet with its header whole and its body cut short
      F   more whole packets than max_packets
    `busy`: entries that must decrypt something (ordinary blocks, tlen >= 1).
    `batch`: continue these oracle streams instead of seeding fresh ones."""
    rng = np.random.default_rng([seed, n, bound])
    idle = np.zeros(n, bool) if idle is None else np.asarray(idle, bool)
    busy = np.zeros(n, bool) if busy is None else np.asarray(busy, bool)
    kind = np.zeros(n, np.int8)
    kind[idle] = K["A"]
    free = np.flatnonzero(~idle & ~busy)
    assert free.size >= PER_CASE * len(KINDS), "too few entries for the ingredients"
    kind[rng.permutation(free)[:PER_CASE * len(KINDS)]] = np.repeat(np.arange(1, len(KINDS) + 1), PER_CASE)
    for ch in marked:
        cc = free[(free // 256 == ch)]
        cc = cc[kind[cc] == 0]
        assert cc.size >= len(KINDS), f"chunk {ch} too small for one of each ingredient"
        kind[rng.permutation(cc)[:len(KINDS)]] = np.arange(1, len(KINDS) + 1)
    is_k = lambda *names: np.isin(kind, [K[x] for x in names])

    # packets: entry i takes pool[s[i] : s[i] + k[i]], the first k reaching its target
    n1, n2 = 1 << 16, 1 << 12
    pool = np.concatenate([rng.integers(6, 65, n1), rng.integers(6, 13, n2)]).astype(np.int64)
    cum = np.concatenate([[0], np.cumsum(pool)])
    target = rng.integers(0, 201, n)
    big = (rng.random(n) < 0.02) & (kind == 0)
    target[big] = rng.integers(1000, 3001, int(big.sum()))
    target[busy] = np.maximum(target[busy], 30)
    target[is_k("A")] = rng.integers(200, 301, int(is_k("A").sum()))
    target[is_k("B")] = 0
    mid = is_k("C1", "C2", "C3", "D1", "D2", "D3", "E1", "E2")
    target[mid] = rng.integers(140, 201, int(mid.sum()))
    target[is_k("F")] = 12 * (max(maxp, 1) + 2) + 20
    s = rng.integers(0, n1 - 600, n)
    s[is_k("F")] = n1 + rng.integers(0, n2 - 64, int(is_k("F").sum()))      # small packets: many in few bytes
    k = np.searchsorted(cum, cum[s] + target, side="left") - s
    e2 = is_k("E2")
    while (e2 & (pool[s + k - 1] == 6)).any():                              # E2 needs a body to cut
        k[e2 & (pool[s + k - 1] == 6)] -= 1
    total = cum[s + k] - cum[s]
    cut = np.where(rng.random(n) < 0.7, rng.integers(0, 21, n), 0)
    L = total - np.minimum(cut, total)
    last = np.where(k > 0, cum[s + np.maximum(k, 1) - 1] - cum[s], 0)       # start of the last packet
    plast = pool[s + np.maximum(k, 1) - 1]
    L[is_k("E1")] = (last + rng.integers(1, 6, n))[is_k("E1")]
    L[e2] = (last + 6 + np.floor(rng.random(n) * (plast - 6)).astype(np.int64))[e2]
    L = np.minimum(L, bound)

    p0 = pool[s]                                                           # length of packet 0
    u = rng.random(n)
    u[rng.random(n) < 0.2] = 0.0                                           # a wholly fresh block
    head = np.floor(L * u).astype(np.int64)
    head[is_k("A")] = L[is_k("A")]
    for c in (1, 2, 3):
        m = is_k(f"C{c}")
        head[m] = p0[m] + c
    head[busy] = np.minimum(head[busy], L[busy] - 1)
    assert (head <= L).all() and (L[busy] > head[busy]).all()

    gap = np.arange(n) % 5 + rng.integers(0, 4, n)
    off = 3 + np.concatenate([[0], np.cumsum(L + gap)[:-1]])
    plain = rng.integers(0, 256, int(off[-1] + L[-1]) + 64, dtype=np.uint8)

    # the length fields (the rest of every packet stays random bytes)
    ent = np.repeat(np.arange(n), k)
    j = np.arange(ent.size) - np.repeat(np.cumsum(k) - k, k)
    idx = s[ent] + j
    val = pool[idx].copy()
    pst = cum[idx] - cum[s[ent]]
    at1 = j == 1
    for name, draw in (("D1", lambda m: rng.choice([0, 3, 5], m)),
                       ("D2", lambda m: rng.choice([bound + 1, max(30000, bound + 7), 1 << 30, 0xFFFFFFFF], m)),
                       ("D3", lambda m: bound - np.floor(rng.random(m) * p0[ent[sel]]).astype(np.int64))):
        sel = at1 & (kind[ent] == K[name])
        assert sel.sum() == is_k(name).sum(), "every D block has a packet 1"
        val[sel] = draw(int(sel.sum()))
    for b in range(4):
        pos = off[ent] + pst + b
        ok = pos < off[ent] + L[ent]
        plain[pos[ok]] = (val[ok] >> (8 * b)) & 255

    off, ln = off.astype(np.uint64), L.astype(np.uint32)
    toff, tlen = (off + head.astype(np.uint64)), (L - head).astype(np.uint32)
    keys = None
    if batch is None:
        keys = rng.integers(0, 256, (n, 16), dtype=np.uint8)
        batch = pyoracle.Batch(n)
        batch.make_sbox(keys.reshape(-1), np.arange(n, dtype=np.uint64) * 16, np.full(n, 16, np.uint32))
    assert batch.n == n
    inp = plain.copy()
    batch.crypt(inp, toff, tlen, threads=8)
    cs = SimpleNamespace(n=n, bound=bound, maxp=maxp, plain=plain, inp=inp, off=off, len=ln, toff=toff, tlen=tlen,
                         keys=keys, batch=batch, kind=kind, masks={x: kind == K[x] for x in KINDS},
                         p0=p0, marked=tuple(marked), want=pyoracle.frame_scan(plain, off, ln, bound, maxp))
    check_case(cs)
    return cs


def _u32_at(buf, pos):
    pos = np.asarray(pos, np.int64)
    return sum(buf[pos + b].astype(np.int64) << (8 * b) for b in range(4))


def check_case(cs):
    """Every ingredient is there (PER_CASE times, and in every marked chunk)
    and the ORACLE's framing of the plaintext ends each one the way it was
    built to end."""
    npk, used, status, _ = (a.astype(np.int64) for a in cs.want)
    ln, tlen, off = cs.len.astype(np.int64), cs.tlen.astype(np.int64), cs.off.astype(np.int64)
    rest = ln - used
    for name, m in cs.masks.items():
        assert m.sum() >= PER_CASE, (name, int(m.sum()))
        for ch in cs.marked:
            assert m[256 * ch: 256 * (ch + 1)].any(), (name, ch)
    m = cs.masks
    assert ((tlen[m["A"]] == 0) & (ln[m["A"]] > 0) & (npk[m["A"]] >= 2)).all()
    assert ((ln[m["B"]] == 0) & (tlen[m["B"]] == 0) & (npk[m["B"]] == 0) & (used[m["B"]] == 0)
            & (status[m["B"]] == 1)).all()
    for c in (1, 2, 3):
        mc = m[f"C{c}"]
        # packet 0 is whole, packet 1's length field lies inside the block, the head ends c bytes into it
        assert ((ln - tlen)[mc] == cs.p0[mc] + c).all() and (used[mc] >= cs.p0[mc]).all()
        assert (ln[mc] >= cs.p0[mc] + 4).all() and (tlen[mc] > 0).all()
    for name, st in (("D1", 2), ("D2", 2), ("D3", 1)):
        md = m[name]
        assert ((status[md] == st) & (npk[md] == 1) & (used[md] == cs.p0[md])).all(), name
        f = _u32_at(cs.plain, off[md] + used[md])
        if name == "D1":
            assert (f < 6).all()
        elif name == "D2":
            assert (f > cs.bound).all()
        else:
            assert ((f > cs.bound - used[md]) & (f <= cs.bound)).all()
    assert ((status[m["E1"]] == 1) & (rest[m["E1"]] >= 1) & (rest[m["E1"]] <= 5)).all()
    me = m["E2"]
    f = _u32_at(cs.plain, off[me] + used[me])
    assert ((status[me] == 1) & (rest[me] >= 6) & (f > rest[me]) & (f <= cs.bound - used[me]) & (f >= 6)).all()
    assert (npk[m["F"]] > cs.maxp).all()


# --------------------------------------------------------------- the matrix
# id, entry point, first_slot, groups(cus), entries of the last group, class (kernel_class of
# tests/dispatch_model.py), kernel meant
MATRIX = [
    ("range_fs0_33g_half_kRange", "range", 0, lambda cus: 33, 77, "half", "crypt_half_kernel<kRange,true>"),
    ("range_fs0_halfCUs+1g_whole_kRange", "range", 0, lambda cus: cus // 2 + 1, 1, "whole",
     "crypt_kernel<kRange,true> (whole image)"),
    ("range_fs37_5g_whole_kRange_gathered", "range", 37, lambda cus: 5, 77, "whole",
     "crypt_kernel<kRange,true> (gathered columns)"),
    ("range_fs37_halfCUs+22g_whole_kRange_gathered", "range", 37, lambda cus: cus // 2 + 22, 77, "whole",
     "crypt_kernel<kRange,true> (gathered columns, XCD runs + tail)"),
    ("range_fs37_CUs+4g_stream_unaligned", "range", 37, lambda cus: cus + 4, 77, "stream",
     "crypt_stream_kernel<false,false,true>"),
    ("range_fs256_3g_win_kRange", "range", 256, lambda cus: 3, 77, "win", "crypt_win_kernel<kRange,true>"),
    ("grouped_40b_half_kGrouped", "grouped", 0, lambda cus: 40, 77, "half", "crypt_half_kernel<kGrouped,true>"),
    ("grouped_halfCUs+72b_whole_kGrouped", "grouped", 0, lambda cus: cus // 2 + 72, 77, "whole",
     "crypt_kernel<kGrouped,true>"),
    ("grouped_6b_win_kGrouped", "grouped", 0, lambda cus: 6, 77, "win", "crypt_win_kernel<kGrouped,true,false>"),
]
VARIANTS = [
    ("range_fs0_3g_win_kRange", "range", 0, lambda cus: 3, 77, "win", "crypt_win_kernel<kRange,true>"),
    ("grouped_6b_win_kGrouped", "grouped", 0, lambda cus: 6, 77, "win", "crypt_win_kernel<kGrouped,true,false>"),
]


def layout(spec, cus, seed):
    """Which slot each entry uses.  range: entry i -> slot first_slot + i, the
    last group ragged.  grouped: the zrc4_crypt_grouped contract -- bucket b
    holds slots of one group of an arena with 64 spare groups (groups in
    random order, slots in random entry positions), ~10 % of every bucket's
    entries are ZRC4_IDLE_SLOT padding, one whole bucket is idle, the last
    bucket is short.  Idle entries carry a frame block all the same."""
    name, mode, first_slot, groups, last, cls, kernel = spec
    g = groups(cus)
    n = (g - 1) * 256 + last
    rng = np.random.default_rng([seed, g])
    lay = SimpleNamespace(name=name, mode=mode, first_slot=first_slot, groups=g, n=n, cls=cls, kernel=kernel,
                          marked=(g - 1,) if last >= 64 else ())
    if mode == "range":
        lay.ids = None
        lay.slots = (first_slot + np.arange(n)).astype(np.int64)
        lay.idle = np.zeros(n, bool)
        lay.cap = -(-(first_slot + n) // 256) * 256 + 256
        return lay
    arena = g + 64
    lay.cap = 256 * arena
    lay.bucket_group = rng.permutation(arena)[:g]
    lay.spare = rng.permutation(np.setdiff1d(np.arange(arena), lay.bucket_group))
    lay.idle_bucket = 3 if g < 12 else 11
    ids = np.full(n, IDLE, np.int64)
    for b in range(g):
        cnt = min(256, n - 256 * b)
        if b == lay.idle_bucket:
            continue
        pos = rng.permutation(cnt)[max(1, round(0.1 * cnt)):]
        ids[256 * b + pos] = int(lay.bucket_group[b]) * 256 + rng.permutation(256)[:pos.size]
    lay.ids = ids
    lay.idle = ids == IDLE
    lay.slots = np.where(lay.idle, 0, ids)
    return lay


def test_kernel_class_follows_launch_crypt():
    """With 256 CUs every row of the matrix selects the kernel its id names."""
    for spec in MATRIX + VARIANTS:
        name, mode, first_slot, groups, last, cls, kernel = spec
        assert kernel_class(mode, first_slot, groups(256), 256) == cls, name
    assert [kernel_class("grouped", 0, g, 256) for g in (20, 100, 200)] == ["win", "half", "whole"]


def build_cases(spec, cus, seed, bound=BOUND, maxp=8):
    """The layout and the two calls' cases of one row: what the GPU tests
    launch and what the CPU generator test inspects."""
    lay = layout(spec, cus, seed)
    c1 = make_case(lay.n, seed, bound, maxp, idle=lay.idle, marked=lay.marked)
    c2 = make_case(lay.n, seed + 1000, bound, maxp, idle=lay.idle, marked=lay.marked, batch=c1.batch)
    return lay, c1, c2


# (seed, bound, max_packets) of test_fused_matrix and of the two parameter variants
RUNS = [(spec, 11, BOUND, 8) for spec in MATRIX] + [(spec, 12, BOUND, 0) for spec in VARIANTS] + \
       [(spec, 13, 512, 8) for spec in VARIANTS]


@pytest.mark.parametrize("spec,seed,bound,maxp", RUNS, ids=lambda v: v[0] if isinstance(v, tuple) else str(v))
def test_generator_builds_every_case(spec, seed, bound, maxp):
    """CPU: both calls' cases of every GPU run below, as built for 256 CUs.
    make_case asserts the ingredient counts and what the oracle makes of each
    ingredient (check_case); here pyoracle.frame_scan is also compared with
    the pure-Python restatement on every A..E block, the device input differs
    from the plaintext only inside the crypt spans, and decrypting it with a
    fresh copy of the streams gives the plaintext back."""
    lay, c1, c2 = build_cases(spec, 256, seed, bound, maxp)
    st0 = pyoracle.Batch(lay.n)                                           # the streams as seeded
    st0.make_sbox(c1.keys.reshape(-1), np.arange(lay.n, dtype=np.uint64) * 16, np.full(lay.n, 16, np.uint32))
    for cs in (c1, c2):
        assert (cs.tlen[lay.idle] == 0).all() and cs.masks["A"][lay.idle].all()
        assert (cs.len <= bound).all()
        if bound == BOUND:
            assert (cs.len > 2048).any(), "a block past the window kernel's 2 KiB chunk"
        inside = np.zeros(cs.plain.size + 1, np.int64)
        np.add.at(inside, cs.toff.astype(np.int64), 1)
        np.add.at(inside, cs.toff.astype(np.int64) + cs.tlen, -1)
        inside = np.cumsum(inside)[:-1]
        assert inside.max() <= 1, "crypt spans overlap"
        assert not (cs.inp != cs.plain)[inside == 0].any()
        back = cs.inp.copy()
        st0.crypt(back, cs.toff, cs.tlen, threads=8)                  # (c2 continues where c1 stopped)
        assert np.array_equal(back, cs.plain)
        npk, used, status, pk = cs.want
        sel = np.flatnonzero(np.isin(cs.kind, [K[x] for x in KINDS if x != "F"]))
        if sel.size > 600:                                            # (grouped padding: thousands of A blocks)
            sel = np.concatenate([np.flatnonzero(np.isin(cs.kind, [K[x] for x in KINDS[1:-1]])),
                                  np.flatnonzero(cs.masks["A"])[:400]])
        for e in sel:
            a = int(cs.off[e])
            pkts, u, st = pyoracle.py_frame_scan(cs.plain[a:a + int(cs.len[e])].tobytes(), bound)
            assert (len(pkts), u, st) == (int(npk[e]), int(used[e]), int(status[e])), (e, KINDS[cs.kind[e] - 1])
            if maxp:
                assert pkts[:maxp] == pk[e][:min(maxp, len(pkts))].tolist(), e


# ---------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch, cu_count(torch)


def _seed_arena(torch, lay, c1, seed):
    """A context of lay.cap slots, every slot seeded: the batch's slots with
    their entries' keys, the rest with keys of their own.  Returns it with the
    oracle's states of the arena as seeded."""
    from zsummerx_amd import Context
    rng = np.random.default_rng([seed, 77])
    live = ~lay.idle
    keys = rng.integers(0, 256, (lay.cap, 16), dtype=np.uint8)
    keys[lay.slots[live]] = c1.keys[live]
    koff = np.arange(lay.cap, dtype=np.uint64) * 16
    klen = np.full(lay.cap, 16, np.uint32)
    ob = pyoracle.Batch(lay.cap)
    ob.make_sbox(keys.reshape(-1), koff, klen)
    T = dev(torch)
    c = Context(0, lay.cap)
    c.ksa_range(0, T(klen.view(np.int32)), T(koff.view(np.int64)), T(keys.reshape(-1)))
    c.sync()
    return c, ob.states()


def _launch(torch, c, lay, cs, with_pk=True):
    """One fused call over case cs; returns the payload and the framing
    outputs as the device left them (every output prefilled with SENT)."""
    T = dev(torch)
    n, maxp = cs.n, cs.maxp
    sent = lambda k: T(np.full(max(1, k), SENT, np.uint32).view(np.int32))
    npk, used, status, pk = sent(n), sent(n), sent(n), sent(n * maxp)
    frame = {"off": T(cs.off.view(np.int64)), "len": T(cs.len.view(np.int32)), "bound": cs.bound,
             "max_packets": maxp, "npk": npk, "used": used, "status": status}
    if with_pk:
        frame["pkt_len"] = pk
    d = T(cs.inp)
    toff, tlen = T(cs.toff.view(np.int64)), T(cs.tlen.view(np.int32))
    if lay.mode == "range":
        c.crypt_range_frame(lay.first_slot, d, toff, tlen, frame)
    else:
        c.crypt_grouped_frame(d, toff, tlen, T(lay.ids.astype(np.uint32).view(np.int32)), frame)
    host = lambda t: t.cpu().numpy().view(np.uint32)
    return d, (lambda: (d.cpu().numpy(), host(npk), host(used), host(status), host(pk)[:n * maxp].reshape(n, maxp)))


def _want_pk(cs):
    """pkt_len as it must stand: the oracle's first min(npk, maxp) lengths of
    every row, SENT in the rest."""
    npk, _, _, pk = cs.want
    w = np.full((cs.n, cs.maxp), SENT, np.uint32)
    if cs.maxp:
        fill = np.arange(cs.maxp)[None, :] < np.minimum(npk, cs.maxp)[:, None]
        w[fill] = pk[:, :cs.maxp][fill]
    return w


def _state_report(c, lay, seeded, batch, ran, what):
    """'' when every slot of the arena is right: the batch's slots as the
    oracle streams stand, every other slot as it was seeded."""
    sb, x, y = (a.copy() for a in seeded)
    bs, bx, by = batch.states()
    sb[lay.slots[ran]], x[lay.slots[ran]], y[lay.slots[ran]] = bs[ran], bx[ran], by[ran]
    gsb, gx, gy = c.get_states(0, lay.cap)
    bad = np.flatnonzero((gsb != sb).any(axis=1) | (gx != x) | (gy != y))
    mine = np.zeros(lay.cap, bool)
    mine[lay.slots[ran]] = True
    if bad.size == 0:
        return ""
    return (f"{what}: states of {bad.size} slots differ, first {bad[:8].tolist()} "
            f"(slots of the batch: {mine[bad[:8]].tolist()}); x got {gx[bad[:4]].tolist()} "
            f"want {x[bad[:4]].tolist()}, y got {gy[bad[:4]].tolist()} want {y[bad[:4]].tolist()}, "
            f"S-box bytes differing {(gsb[bad[:4]] != sb[bad[:4]]).sum(axis=1).tolist()}")


def _run(torch, cus, spec, seed, bound=BOUND, maxp=8, with_pk=True):
    lay, c1, c2 = build_cases(spec, cus, seed, bound, maxp)
    assert kernel_class(lay.mode, lay.first_slot, lay.groups, cus) == lay.cls, \
        f"{lay.name}: {lay.groups} groups on {cus} CUs do not select {lay.kernel}"
    c, seeded = _seed_arena(torch, lay, c1, seed)
    errs = []                                   # everything one run can tell, then one assertion
    with c:
        for call, cs in enumerate((c1, c2)):
            what = f"{lay.name} ({lay.kernel}) call {call}"
            _, fetch = _launch(torch, c, lay, cs, with_pk)
            c.sync()
            got, npk, used, status, pk = fetch()
            msgs = [payload_report(got, cs.plain, cs.toff, cs.tlen)]
            msgs += [frame_report(w, g, nm) for w, g, nm in zip(cs.want[:3], (npk, used, status),
                                                                 ("npk", "used", "status"))]
            if with_pk:
                msgs.append(frame_report(_want_pk(cs), pk, "pkt_len"))
            errs += [f"{what}: {m}" for m in msgs if m]
        errs.append(_state_report(c, lay, seeded, c1.batch, ~lay.idle, f"{lay.name} ({lay.kernel}) after two calls"))
    errs = [m for m in errs if m]
    assert not errs, "\n".join(errs)


@pytest.mark.gpu
@pytest.mark.parametrize("spec", MATRIX, ids=lambda s: s[0])
def test_fused_matrix(built, gpu, spec):
    """Two fused calls in a row on the kernel the id names: the whole payload
    buffer (gaps included), npk / used / status / pkt_len of every entry
    (padding included; untouched pkt_len slots keep their prefill) and, after
    the second call, every state of the arena -- the batch's slots against the
    oracle streams, every other slot (below an unaligned first_slot, past the
    range's end, the unused slots of a bucket's group, the spare groups)
    against what it was seeded with."""
    torch, cus = gpu
    _run(torch, cus, spec, seed=11)


@pytest.mark.gpu
@pytest.mark.parametrize("spec", VARIANTS, ids=lambda s: s[0])
def test_fused_no_packet_lengths(built, gpu, spec):
    """max_packets = 0 with pkt_len omitted (include/zrc4.h: pkt_len may be
    NULL then): npk / used / status alone."""
    torch, cus = gpu
    _run(torch, cus, spec, seed=12, maxp=0, with_pk=False)


@pytest.mark.gpu
@pytest.mark.parametrize("spec", VARIANTS, ids=lambda s: s[0])
def test_fused_bound_512(built, gpu, spec):
    """bound = 512 with the blocks cut to 512 bytes: the long blocks now stop
    on ordinary packet lengths that pass bound - used."""
    torch, cus = gpu
    _run(torch, cus, spec, seed=13, bound=512)


# ------------------------------------------------- refusals, undeclared fused
def refusal_case(g, cls, cus):
    """A grouped batch of g buckets whose bucket 2 mixes two spare groups and
    whose bucket 5 names a slot twice.  Returns the layout, the case, the
    refused buckets' entries, the busy ones among them and the payload as it
    must stand after the call."""
    lay = layout((f"refusal_{g}b", "grouped", 0, lambda _: g, 77, cls, cls), cus, seed=21)
    rng = np.random.default_rng(2100 + g)
    H, H2, H3 = (int(v) for v in lay.spare[:3])
    ids = lay.ids
    ids[256 * 2: 256 * 3] = IDLE
    pos = rng.permutation(256)[:100]
    ids[256 * 2 + pos[:50]] = H * 256 + rng.permutation(256)[:50]
    ids[256 * 2 + pos[50:]] = H2 * 256 + rng.permutation(256)[:50]
    ids[256 * 5: 256 * 6] = IDLE
    pos = rng.permutation(256)[:42]
    lanes = rng.permutation(256)[:41]
    ids[256 * 5 + pos] = H3 * 256 + np.concatenate([lanes, lanes[:1]])    # lanes[0] named twice
    lay.idle = ids == IDLE
    refused = np.zeros(lay.n, bool)
    refused[256 * 2: 256 * 3] = True
    refused[256 * 5: 256 * 6] = True
    rb = refused & ~lay.idle                                             # busy entries of the refused buckets
    assert rb.sum() == 142
    cs = make_case(lay.n, 21, idle=lay.idle, busy=rb, marked=lay.marked)
    assert (cs.tlen[rb] > 0).all()
    # slots: every entry's own, but the twice-named slot is seeded once (by the later entry; it never runs)
    lay.slots = np.where(lay.idle, 0, ids)
    want = cs.plain.copy()                                              # refused busy spans stay ciphertext
    for e in np.flatnonzero(rb):
        a, z = int(cs.toff[e]), int(cs.toff[e]) + int(cs.tlen[e])
        want[a:z] = cs.inp[a:z]
    return lay, cs, refused, rb, want


@pytest.mark.parametrize("g,cls", [(20, "win"), (100, "half"), (200, "whole")])
def test_refusal_case_breaks_the_contract_as_meant(g, cls):
    """CPU: bucket 2's busy entries lie in exactly two groups, bucket 5's in
    one with one slot twice, no other bucket names those groups, every other
    bucket keeps the contract, and every refused busy entry has bytes to
    decrypt."""
    lay, cs, refused, rb, want = refusal_case(g, cls, 256)
    grp = np.where(lay.idle, -1, lay.ids // 256)
    b2, b5 = grp[512:768], grp[1280:1536]
    bad = set(b2[b2 >= 0]) | set(b5[b5 >= 0])
    assert len(set(b2[b2 >= 0])) == 2 and len(set(b5[b5 >= 0])) == 1 and len(bad) == 3
    s5 = lay.ids[1280:1536][b5 >= 0]
    assert s5.size == 42 and np.unique(s5).size == 41
    assert not (set(grp[~refused]) & bad) and not (set(lay.bucket_group) & bad)
    live = np.flatnonzero(~refused & ~lay.idle)
    assert np.unique(lay.ids[live]).size == live.size
    for b in range(g):
        gb = grp[256 * b: 256 * (b + 1)]
        if b not in (2, 5):
            assert len(set(gb[gb >= 0])) == (0 if b == lay.idle_bucket else 1), b
    assert (cs.tlen[rb] > 0).all() and (want != cs.plain).any()
    inside = np.zeros(want.size, bool)
    for e in np.flatnonzero(rb):
        inside[int(cs.toff[e]): int(cs.toff[e]) + int(cs.tlen[e])] = True
    assert not (want != cs.plain)[~inside].any() and np.array_equal(want[inside], cs.inp[inside])


@pytest.mark.gpu
@pytest.mark.parametrize("nb", ["20", "halfCUs-28", "CUs-56"])
def test_fused_refused_bucket_frames_nothing(built, gpu, nb):
    """include/zrc4.h, zrc4_crypt_grouped_frame on at most one bucket per CU
    (window, half-group, whole-group kernel): a refused bucket decrypts
    nothing, moves no state and never frames a busy entry over its
    undecrypted bytes.  Bucket 2 mixes 50 busy slots of spare group H with 50
    of spare group H2; bucket 5 names one slot of spare group H3 twice (among
    40 others of H3).  No other bucket names H, H2 or H3.  ZRC4_ERR_GROUP;
    every other bucket, idle entries included, is decrypted and framed as the
    oracle does it; every state of the arena is checked."""
    from zsummerx_amd import ZRC4Error
    torch, cus = gpu
    g = {"20": 20, "halfCUs-28": cus // 2 - 28, "CUs-56": cus - 56}[nb]
    cls = {"20": "win", "halfCUs-28": "half", "CUs-56": "whole"}[nb]
    assert kernel_class("grouped", 0, g, cus) == cls, f"{g} buckets on {cus} CUs are not the {cls} kernel's"
    lay, cs, refused, rb, want = refusal_case(g, cls, cus)
    c, seeded = _seed_arena(torch, lay, cs, 21)
    with c:
        _, fetch = _launch(torch, c, lay, cs)
        with pytest.raises(ZRC4Error) as ei:
            c.sync()
        assert ei.value.code == -7                                       # ZRC4_ERR_GROUP
        got, npk, used, status, pk = fetch()
        errs = [payload_report(got, want, cs.toff, cs.tlen)]
        framed = rb & ((npk != SENT) | (used != SENT) | (status != SENT) | (pk != SENT).any(axis=1))
        if framed.any():
            errs.append(f"a refused bucket framed its busy entries {np.flatnonzero(framed)[:8].tolist()} "
                        f"over their undecrypted bytes")
        keep = ~refused
        for w, gg, nm in zip(cs.want[:3] + (_want_pk(cs),), (npk, used, status, pk),
                             ("npk", "used", "status", "pkt_len")):
            msg = frame_report(w[keep], gg[keep], nm)
            errs.append(msg and f"entries outside buckets 2 and 5 (numbered among those): {msg}")
        errs.append(_state_report(c, lay, seeded, cs.batch, ~lay.idle & ~refused, "after the call"))
    errs = [f"{g} buckets ({cls}): {m}" for m in errs if m]
    assert not errs, "\n".join(errs)
