"""Failure reports of the framing tests (plain numpy): '' when the device's
output matches the oracle's, else enough to tell a stray store from a wrong
keystream after one failing run.  Shared by tests/test_frame_scan.py,
tests/test_gpu_fused_matrix.py and tests/test_gpu_addressing.py."""
import numpy as np

BOUND = 20480                           # the frame bound of the baseline shapes


def payload_report(got, want, off, ln):
    """'' when the buffers match; else the count of differing bytes, the
    first offsets and the sessions (entries) they fall in, with each one's
    [off, off + len) span -- enough to tell a stray store from a wrong
    keystream after one failing run (no reruns to reproduce)."""
    bad = np.flatnonzero(got != want)
    if bad.size == 0:
        return ""
    off = np.asarray(off, dtype=np.int64)
    ln = np.asarray(ln, dtype=np.int64)
    order = np.argsort(off, kind="stable")
    ent = order[np.clip(np.searchsorted(off[order], bad[:16], side="right") - 1, 0, len(off) - 1)]
    inside = (bad[:16] >= off[ent]) & (bad[:16] < off[ent] + ln[ent])
    sess = sorted(set(int(e) for e in ent))
    return (f"{bad.size} bytes differ; first offsets {bad[:16].tolist()}; entries {ent.tolist()} "
            f"(inside their span: {inside.tolist()}); {len(np.unique(ent))} distinct among the first 16; "
            f"spans {[(int(off[e]), int(off[e] + ln[e])) for e in sess[:4]]}; "
            f"got {got[bad[:8]].tolist()} want {want[bad[:8]].tolist()}")


def frame_report(w, g, name):
    """'' when a framing output matches; else where it differs."""
    w, g = np.asarray(w), np.asarray(g)
    if np.array_equal(w, g):
        return ""
    rows = np.flatnonzero((w != g).reshape(len(w), -1).any(axis=1))
    return (f"{name}: {rows.size} entries differ, first {rows[:8].tolist()}: "
            f"want {w[rows[:4]].tolist()} got {g[rows[:4]].tolist()}")
