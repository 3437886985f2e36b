"""The rule of rtk_amd/csrc/rtk_box_rule.h restated in numpy float32, for tests/test_box_cpu.py (against the header's driver) and
tests/test_gpu_box.py (against the kernel): every product, sum and difference is one float32 operation in the header's order.
Per query the count of its candidates, its full list in ascending primitive id, and the prefix a segment of a given room keeps."""
import numpy as np

F = np.float32
HALF = np.float32(0.5)


def live_np(lo, hi):
    """rule 1: [..., 3] float32 each -> bool [...]"""
    with np.errstate(invalid="ignore"):
        return ((lo - lo == 0) & (hi - hi == 0) & (lo <= hi)).all(-1)


def centre_np(lo, hi):
    with np.errstate(over="ignore", invalid="ignore"):
        return (lo + hi) * HALF, (hi - lo) * HALF


def _min(x, y):
    return np.where(y < x, y, x)


def _max(x, y):
    return np.where(y > x, y, x)


def boxes_touch_np(v0, v1, v2, lo, hi):
    """rule 2"""
    with np.errstate(invalid="ignore"):
        tlo, thi = _min(_min(v0, v1), v2), _max(_max(v0, v1), v2)
        return ((tlo <= hi) & (thi >= lo)).all(-1)


def _axis(ea, eb, w, ia, ib, ha, hb):
    """p_k = ea * w_k[ib] - eb * w_k[ia]; r = ha * |eb| + hb * |ea|"""
    p = [ea * wk[..., ib] - eb * wk[..., ia] for wk in w]
    r = ha * np.abs(eb) + hb * np.abs(ea)
    return ((p[0] > r) & (p[1] > r) & (p[2] > r)) | ((p[0] < -r) & (p[1] < -r) & (p[2] < -r))


def separated_np(v0, v1, v2, c, h):
    """rule 3: does one of the ten axes separate?"""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        w = [v0 - c, v1 - c, v2 - c]
        e = [v1 - v0, v2 - v1, v0 - v2]
        hx, hy, hz = h[..., 0], h[..., 1], h[..., 2]
        sep = np.zeros(np.broadcast(v0[..., 0], c[..., 0]).shape, bool)
        for ej in e:
            ex, ey, ez = ej[..., 0], ej[..., 1], ej[..., 2]
            sep = sep | _axis(ey, ez, w, 1, 2, hy, hz)           # unit_x X e
            sep = sep | _axis(ez, ex, w, 2, 0, hz, hx)           # unit_y X e
            sep = sep | _axis(ex, ey, w, 0, 1, hx, hy)           # unit_z X e
        e0, e1 = e[0], e[1]
        nx = e0[..., 1] * e1[..., 2] - e0[..., 2] * e1[..., 1]
        ny = e0[..., 2] * e1[..., 0] - e0[..., 0] * e1[..., 2]
        nz = e0[..., 0] * e1[..., 1] - e0[..., 1] * e1[..., 0]
        d = (nx * w[0][..., 0] + ny * w[0][..., 1]) + nz * w[0][..., 2]
        r = (hx * np.abs(nx) + hy * np.abs(ny)) + hz * np.abs(nz)
        return sep | (d > r) | (d < -r)


def candidate_np(v0, v1, v2, lo, hi):
    """rule 4, arrays that broadcast against each other, [..., 3] float32 -> bool [...]"""
    v0, v1, v2, lo, hi = (np.asarray(x, F) for x in (v0, v1, v2, lo, hi))
    c, h = centre_np(lo, hi)
    return live_np(lo, hi) & boxes_touch_np(v0, v1, v2, lo, hi) & ~separated_np(v0, v1, v2, c, h)


def skip_np(clo, chi, lo, hi):
    """rule 5"""
    with np.errstate(invalid="ignore"):
        return ((clo > hi) | (chi < lo)).any(-1)


class InBoxes:
    """counts uint32 [Q]; lists[i] = uint32 [count_i], ascending ids; kept[i] = the same cut to room[i] entries"""

    def __init__(self, counts, lists, kept):
        self.counts, self.lists, self.kept = counts, lists, kept


def brute_force_boxes(tris, prims, lo, hi, room=None):
    """tris [T, 3, 3] float32 with ids prims [T], lo / hi [Q, 3], room None or [Q] -> InBoxes"""
    tris = np.ascontiguousarray(tris, F).reshape(-1, 3, 3)
    prims = np.asarray(prims, np.uint32)
    lo, hi = np.ascontiguousarray(lo, F).reshape(-1, 3), np.ascontiguousarray(hi, F).reshape(-1, 3)
    Q, T = len(lo), len(tris)
    empty = np.zeros(0, np.uint32)
    if T == 0 or Q == 0:
        return InBoxes(np.zeros(Q, np.uint32), [empty] * Q, [empty] * Q)
    cand = candidate_np(tris[None, :, 0], tris[None, :, 1], tris[None, :, 2], lo[:, None, :], hi[:, None, :])
    counts = cand.sum(1).astype(np.uint32)
    lists, kept = [], []
    for i in range(Q):
        ids = np.sort(prims[np.nonzero(cand[i])[0]])
        lists.append(ids)
        kept.append(ids if room is None else ids[:int(room[i])])
    return InBoxes(counts, lists, kept)
