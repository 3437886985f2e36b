"""The rule of rtk_amd/csrc/rtk_closest_rule.h restated in numpy, for tests/test_closest_cpu.py (against the header's driver) and
tests/test_gpu_closest.py (against the kernel): every product, sum, difference and quotient is one operation of `dtype`, in the
header's order. With dtype float32 it states the expected bits; with float64 it is the yardstick of the accuracy statement."""
import numpy as np

NONE = 0xFFFFFFFF


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def tri_np(p, a, b, c, dtype=np.float32):
    """p, a, b, c broadcastable [..., 3] -> dist2, u, v [...], q [..., 3], region [...] (1 .. 7)"""
    p, a, b, c = (np.asarray(x, dtype) for x in (p, a, b, c))
    p, a, b, c = np.broadcast_arrays(p, a, b, c)
    one, zero = dtype(1), dtype(0)
    with np.errstate(all="ignore"):
        ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
        d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        e, g = d4 - d3, d5 - d6
        region = np.select([(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                            (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e >= 0) & (g >= 0)], [1, 2, 3, 4, 5, 6], 7)
        num = np.select([region == 3, region == 5, region == 6, region == 7], [d1, d2, e, np.broadcast_to(one, d1.shape)], zero).astype(dtype)
        den = np.select([region == 3, region == 5, region == 6, region == 7], [d1 - d3, d2 - d6, e + g, (va + vb) + vc], one).astype(dtype)
        t = num / den
        wb = np.select([region == 2, region == 3, region == 6, region == 7], [np.broadcast_to(one, t.shape), t, one - t, vb * t], zero).astype(dtype)
        wc = np.select([region == 4, region == 5, region == 6, region == 7], [np.broadcast_to(one, t.shape), t, t, vc * t], zero).astype(dtype)
        q = (a + ab * wb[..., None]) + ac * wc[..., None]
        m = np.where(b < a, b, a)
        lo = np.where(c < m, c, m)
        m = np.where(b > a, b, a)
        hi = np.where(c > m, c, m)
        q = np.where(q < lo, lo, np.where(q > hi, hi, q))
        d = p - q
        dist2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        u, v = (one - wb) - wc, wb
    assert dist2.dtype == dtype and u.dtype == dtype and v.dtype == dtype and q.dtype == dtype
    return dist2, u, v, q, region


def tri_box(a, b, c):
    """lo, hi of the rule's clamp (selects, as the header has them)"""
    m = np.where(b < a, b, a)
    lo = np.where(c < m, c, m)
    m = np.where(b > a, b, a)
    return lo, np.where(c > m, c, m)


def box_np(p, lo, hi, dtype=np.float32):
    p, lo, hi = (np.asarray(x, dtype) for x in (p, lo, hi))
    with np.errstate(all="ignore"):
        q = np.where(p < lo, lo, np.where(p > hi, hi, p))
        d = p - q
        bound = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert bound.dtype == dtype
    return bound


def better_np(dist2, prim, best2, best_prim):
    with np.errstate(invalid="ignore"):
        return (dist2 < best2) | ((dist2 == best2) & (prim < best_prim))


def brute_force(tris, prims, points, max2):
    """The answer by rules 1 and 3 over ALL triangles: tris [T, 3, 3] float32 with ids prims [T], points [Q, 3], max2 [Q] ->
    (records as the four uint32 words dist2, u, v, prim [Q, 4], points as words [Q, 3])."""
    tris = np.ascontiguousarray(tris, np.float32)
    prims = np.asarray(prims, np.uint32)
    points = np.ascontiguousarray(points, np.float32)
    max2 = np.ascontiguousarray(max2, np.float32)
    Q, T = len(points), len(tris)
    rec = np.zeros((Q, 4), np.uint32)
    rec[:, 0] = max2.view(np.uint32)
    rec[:, 3] = NONE
    out_pts = points.view(np.uint32).copy()
    if T == 0 or Q == 0:
        return rec, out_pts
    dist2, u, v, q, _ = tri_np(points[:, None, :], tris[None, :, 0], tris[None, :, 1], tris[None, :, 2])
    with np.errstate(invalid="ignore"):
        live = (max2 > 0) & np.isfinite(points).all(1)
        cand = (dist2 < max2[:, None]) & live[:, None]
    best = np.where(cand, dist2, np.float32(np.inf)).min(1)
    tie = cand & (dist2 == best[:, None])
    prim = np.where(tie, prims[None, :], np.uint32(NONE)).min(1)
    hit = np.nonzero(prim != NONE)[0]
    col = np.argsort(prims)[np.searchsorted(np.sort(prims), prim[hit])]
    rec[hit, 0] = dist2[hit, col].view(np.uint32)
    rec[hit, 1] = u[hit, col].view(np.uint32)
    rec[hit, 2] = v[hit, col].view(np.uint32)
    rec[hit, 3] = prim[hit]
    out_pts[hit] = q[hit, col].view(np.uint32)
    return rec, out_pts
