"""What the GPU parity tests share (numpy here, torch passed in or imported
inside the functions): a context seeded like its oracle batch, span layouts
with guard bytes, bucket tables, and the checks that follow every call.

  seeded        Context(0, cap) and pyoracle.Batch(cap) over the same random
                16-byte keys, with T, the host-array-to-device helper (dev()).
  layout        destination or source spans in entry order, guard bytes
                between them; span_index turns spans into byte indexes.
  buckets       the grouped calls' id tables: bucket b a random subset of one
                group in shuffled entry positions, ZRC4_IDLE_SLOT elsewhere.
  check_*       every state of the context against the oracle's, and a
                following crypt_range that continues every stream.

Every generator draws from the caller's numpy Generator in a fixed order; the
tests' cases are those draws, so the order is part of the interface.  Which
kernel family a call runs is stated in tests/dispatch_model.py, the framing
reports in tests/frame_support.py.
"""
import numpy as np
import pytest

import pyoracle
from zsummerx_amd import Context
from zsummerx_amd._capi import IDLE_SLOT

FILL = 0xA5        # prefill of every destination buffer
# the 16-byte units and the 2 KiB ring chunk of the window kernel
LONG = np.array([0, 1, 15, 16, 17, 63, 64, 65, 2047, 2048, 2049, 4100], dtype=np.uint32)
# head, blocks 0-3 of the A/B ping-pong, 16-byte pieces and the tail of the lane-per-stream kernels
SHORT = np.array([0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 250], dtype=np.uint32)
TAIL = 24          # bytes per slot of the following crypt_range


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def dev(torch):
    """T: a host array as a device tensor."""
    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()


def cu_count(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


# -- a seeded context and its oracle ------------------------------------------------

def oracle(seed_or_rng, cap):
    """pyoracle.Batch(cap) after KSA over random 16-byte keys (the generator's
    first draw), with the key tables."""
    rng = np.random.default_rng(seed_or_rng)
    keys = rng.integers(0, 256, 16 * cap, dtype=np.uint8)
    koff = np.arange(cap, dtype=np.uint64) * 16
    klen = np.full(cap, 16, dtype=np.uint32)
    ob = pyoracle.Batch(cap)
    ob.make_sbox(keys, koff, klen)
    return ob, keys, koff, klen


def seeded(torch, seed_or_rng, cap):
    """(c, ob, T): a context of cap slots seeded with oracle()'s keys."""
    ob, keys, koff, klen = oracle(seed_or_rng, cap)
    T = dev(torch)
    c = Context(0, cap)
    c.ksa_range(0, T(klen.view(np.int32)), T(koff.view(np.int64)), T(keys), stream=torch.cuda.current_stream())
    return c, ob, T


# -- spans ---------------------------------------------------------------------------

def layout(L, shift, cycle=3):
    """Spans in entry order, 1..cycle guard bytes (cycling) between them, the
    first at `shift`: offsets and the buffer size.  With cycle = 3 the gaps and
    either length list sum to an odd number of bytes modulo 16 per cycle, so
    the start misalignment of every list position walks through all of 0..15."""
    gap = 1 + (np.arange(L.size, dtype=np.uint64) % cycle)
    end = np.cumsum(L.astype(np.uint64) + gap)
    off = np.concatenate(([0], end[:-1])).astype(np.uint64) + np.uint64(shift)
    return off, int(end[-1]) + shift + 16


def span_index(off, L):
    """Indexes of every span byte."""
    L = L.astype(np.int64)
    start = np.cumsum(L) - L
    return np.repeat(off.astype(np.int64) - start, L) + np.arange(int(L.sum()), dtype=np.int64)


def disjoint(off, L):
    """No two of the spans [off, off + L) with L > 0 share a byte."""
    keep = L > 0
    o, l = off[keep].astype(np.int64), L[keep].astype(np.int64)
    order = np.argsort(o, kind="stable")
    o, l = o[order], l[order]
    return bool((o[1:] >= o[:-1] + l[:-1]).all())


def sources(rng, L, doff):
    """Sources of a grouped case: a third of the entries share one message (a
    prefix of it each), a third are congruent with their destination, the rest
    lie wherever the source layout puts them."""
    soff, ssize = layout(L, 11, cycle=5)
    kind = rng.integers(0, 3, L.size)
    cong = kind == 1
    soff[cong] += (doff[cong] - soff[cong]) % np.uint64(16)        # (may run into the next source: allowed)
    shared = ssize + 5
    soff[kind == 0] = shared
    ssize = shared + int(L.max()) + 16
    return soff, ssize


# -- buckets -------------------------------------------------------------------------

def buckets(rng, groups, fill=(1, 256)):
    """Bucket b: a random subset (fill[0]..fill[1] slots) of group groups[b] in
    shuffled entry positions, IDLE_SLOT elsewhere; groups[b] == IDLE_SLOT: an
    idle bucket.  Per bucket the draws are the count, the slots, the positions."""
    ids = np.full(256 * len(groups), IDLE_SLOT, dtype=np.uint32)
    for b, g in enumerate(groups):
        if g == IDLE_SLOT:
            continue
        k = int(rng.integers(fill[0], fill[1] + 1))
        slots = int(g) * 256 + rng.permutation(256)[:k]
        ids[256 * b + rng.permutation(256)[:k]] = slots
    return ids


SWEEP_CALLS, SWEEP_GROUPS = 10, 48


def sweep_call(rng):
    """One call of the multi-round sweep: 1-6 rounds over 1-40 valid buckets
    (distinct groups, each slot at most once, idle entries between), lengths
    0..300, any misalignment, sources shared / congruent / anywhere per
    entry-round.  Returns ids, groups, rounds and the round-major tables with
    both sizes."""
    rounds = int(rng.integers(1, 7))
    nb = int(rng.integers(1, 41))
    groups = rng.permutation(SWEEP_GROUPS)[:nb].astype(np.uint32)
    ids = buckets(rng, groups)
    n = ids.size
    L = rng.integers(0, 301, rounds * n).astype(np.uint32)
    L[rng.random(L.size) < 0.15] = 0
    gap = rng.integers(1, 18, L.size).astype(np.uint64)
    end = np.cumsum(L.astype(np.uint64) + gap)
    doff = np.concatenate(([0], end[:-1])).astype(np.uint64) + np.uint64(rng.integers(0, 16))
    order = rng.permutation(L.size)                      # spans of a slot's rounds lie anywhere, in any order
    doff_p = np.empty_like(doff)
    doff_p[order] = doff
    L_p = np.empty_like(L)
    L_p[order] = L
    size = int(end[-1]) + 32
    ssize = 4096 + 300
    soff = (rng.random(L.size) * (ssize - L_p.astype(np.int64))).astype(np.uint64)
    soff[rng.random(L.size) < 0.4] = int(rng.integers(0, 4096))
    some = rng.random(L.size) < 0.3
    adj = soff[some] + (doff_p[some] - soff[some]) % np.uint64(16)
    ok = adj + L_p[some].astype(np.uint64) <= ssize
    soff[np.flatnonzero(some)[ok]] = adj[ok]
    return ids, groups, rounds, L_p, doff_p, size, soff, ssize


# -- checks --------------------------------------------------------------------------

def assert_equal(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad[:8], int(bad.size), got[bad[:8]], want[bad[:8]])


def host(t):
    return t.cpu().numpy() if t.is_cuda else t.numpy()


def check_states(c, ob, cap):
    gsb, gx, gy = c.get_states(0, cap)
    osb, ox, oy = ob.states()
    bad = np.flatnonzero((gsb != osb).any(axis=1) | (gx != ox) | (gy != oy))
    assert bad.size == 0, bad[:8]


def check_continues(torch, c, ob, T, cap, rng, tail=TAIL):
    """Every state; then crypt_range of `tail` random bytes per slot of the whole
    context goes on where the oracle's streams are; then every state again."""
    check_states(c, ob, cap)
    s = torch.cuda.current_stream()
    data = rng.integers(0, 256, cap * tail, dtype=np.uint8)
    off = np.arange(cap, dtype=np.uint64) * tail
    L = np.full(cap, tail, dtype=np.uint32)
    want = data.copy()
    ob.crypt(want, off, L)
    pay = T(data)
    c.crypt_range(0, pay, T(off.view(np.int64)), T(L.view(np.int32)), stream=s)
    c.sync(s)
    bad = np.flatnonzero(pay.cpu().numpy() != want)
    assert bad.size == 0, ("following crypt_range", bad[:8] // tail, int(bad.size))
    check_states(c, ob, cap)
