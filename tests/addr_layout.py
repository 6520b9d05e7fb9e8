"""Where the bytes of a batched call sit in the address space (plain numpy).

Every batched entry point of include/zrc4.h takes one base pointer and 64-bit
per-entry offsets, and every `base + off` is computed modulo 2^64.  The helpers
here choose the addresses on purpose, for tests/test_gpu_addressing.py:

  the arena    one device allocation of ARENA_BYTES = 3 * 2^32 + 2 * M bytes
               (M = 64 MiB).  Wherever it starts, it holds three consecutive
               multiples of 2^32, A1 < A < A3, each at least M from both ends
               (lines()).  The tests place their spans around A.
  the windows  [X - WIN, X + WIN) around X = A1, A, A3 (WIN = 4 MiB): the only
               bytes ever filled and read back.  The windows at A1 and A3 are
               guards: a lost carry, or an offset cut to 32 bits, lands exactly
               2^32 below the right address, a spurious carry 2^32 above, so
               the likely slips show as a changed guard and not as a wild
               access.
  span_layout  entry k starts at A - s with 0 < s < len[k] (the straddler);
               the entries before it lie below A, the ones after it above,
               separated by the given gaps.
  base modes   the base pointer is a view arena[b:], the offsets are
               (address - base) mod 2^64 (offsets()):
                 low    the arena's start: every offset >= 2^32 + M
                 near   A - WIN: small offsets, only the address carries
                 at     A: entries below A have wrapped offsets
                 above  A + WIN: every offset wraps (the session engine's case,
                        engine/rc4_hooks_device.cpp: address minus base)
"""
import numpy as np

G4 = 1 << 32
M = 64 << 20
WIN = 4 << 20
ARENA_BYTES = 3 * G4 + 2 * M
MODES = ("low", "near", "at", "above")
SPLITS = (1, 15, 16, 17, 63, 64, 65, 100, -1)      # -1: len[k] - 1


def lines(start):
    """(A1, A, A3) of an arena that starts at address `start`."""
    a1 = -(-(start + M) // G4) * G4
    return a1, a1 + G4, a1 + 2 * G4


def base_of(mode, start):
    a = lines(start)[1]
    return {"low": start, "near": a - WIN, "at": a, "above": a + WIN}[mode]


def offsets(addr, base):
    """(addr - base) mod 2^64 as uint64 (pass .view(np.int64) to torch)."""
    return np.asarray(addr, np.int64).astype(np.uint64) - np.asarray([base], np.uint64)


def span_layout(length, gaps, k, s, a):
    """Absolute start addresses (int64) of spans of the given lengths: span k
    starts at a - s, span j + 1 starts gaps[j + 1] bytes after span j ends."""
    L = np.asarray(length, np.int64)
    g = np.asarray(gaps, np.int64)
    n = L.size
    assert 0 <= k < n and 0 < s < L[k], (k, s, int(L[k]))
    st = np.empty(n, np.int64)
    st[k] = a - s
    if k + 1 < n:
        st[k + 1:] = st[k] + np.cumsum(g[k + 1:]) + np.cumsum(L[k:-1])
    if k > 0:
        st[:k] = (st[k] - np.cumsum(g[1:k + 1][::-1]) - np.cumsum(L[:k][::-1]))[::-1]
    return st


def window_index(addr, a):
    """Index of absolute addresses into the host mirror of the three windows
    (A1's, A's, A3's, 2 * WIN bytes each, in that order)."""
    addr = np.asarray(addr, np.int64)
    w = (addr - a + G4 // 2) // G4                  # -1, 0, 1
    return addr - (a + w * G4) + WIN + (w + 1) * 2 * WIN


def ramp(length):
    """0 .. len[0]-1, 0 .. len[1]-1, ... (the byte indexes of every span)."""
    L = np.asarray(length, np.int64)
    return np.arange(int(L.sum()), dtype=np.int64) - np.repeat(np.cumsum(L) - L, L)


def span_bytes(start, length):
    """Every byte address of the spans, span after span."""
    return np.repeat(np.asarray(start, np.int64), np.asarray(length, np.int64)) + ramp(length)


def check_spans(start, length, a, straddler=True, window=True):
    """Spans are pairwise disjoint, (window) inside A's window, and (straddler)
    exactly one of them holds both a - 1 and a."""
    st = np.asarray(start, np.int64)
    L = np.asarray(length, np.int64)
    live = L > 0
    st, en = st[live], st[live] + L[live]
    order = np.argsort(st, kind="stable")
    st, en = st[order], en[order]
    assert (en[:-1] <= st[1:]).all(), "spans overlap"
    assert not window or st.size == 0 or (st[0] >= a - WIN and en[-1] <= a + WIN), "a span leaves the window"
    if straddler:
        assert int(((st <= a - 1) & (en > a)).sum()) == 1, "not exactly one span across the line"


def check_offsets(addr, mode, start, in_window=True):
    """The offsets of `addr` in `mode` give the addresses back modulo 2^64
    and, for addresses of A's window, have a nonzero high word in `low` mode,
    are small in `near` mode and >= 2^63 in `above` mode."""
    addr = np.asarray(addr, np.int64)
    base = base_of(mode, start)
    off = offsets(addr, base)
    back = off + np.asarray([base], np.uint64)          # wraps
    assert np.array_equal(back, addr.astype(np.uint64)), mode
    if mode == "low" and in_window:
        assert (off >> np.uint64(32) != 0).all() and (off >= np.uint64(G4 + M)).all()
    if mode == "near" and in_window:
        assert (off < np.uint64(2 * WIN)).all()
    if mode == "above" and in_window:
        assert (off >= np.uint64(1 << 63)).all()
    return off
