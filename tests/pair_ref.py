"""The rule of rtk_amd/csrc/rtk_pair_rule.h restated in numpy, for tests/test_pair_cpu.py (against the header's driver) and
tests/test_gpu_pair.py (against the kernel): every product, sum, difference and quotient is one operation of `dtype`, in the
header's order. With float32 it states the expected bits; with float64 it is the yardstick of the accuracy statement. One pair
(pair_np, arrays that broadcast), the box bound, and a brute force over a scene with filter, limit and tie rule."""
import numpy as np

from tests.closest_ref import tri_np
from tests.touch_ref import box_np, boxes_touch_np, cross_np, dot_np, live_np, shares_vertex_np

F = np.float32
NONE = 0xFFFFFFFF
FEATURE_NONE = 15
FEATURE_PIERCE = 16
SKIP_SHARED_VERTEX = 1


def _clamp(x, lo, hi):
    return np.where(x < lo, lo, np.where(x > hi, hi, x))


def _clamp01(x, dtype):
    return np.where(x < 0, dtype(0), np.where(x > 1, dtype(1), x))


def segments_np(p1, d1, a, p2, d2, e, dtype=F):
    """rule 2, an edge pair: -> s, t"""
    zero, one = dtype(0), dtype(1)
    r = p1 - p2
    f, c, b = dot_np(d2, r), dot_np(d1, r), dot_np(d1, d2)
    denom = a * e - b * b
    cross, epos, apos = denom > 0, e > 0, a > 0
    x0 = (b * f - c * e) / np.where(cross, denom, one)
    s0 = np.where(cross, _clamp01(x0, dtype), zero)
    y0 = (b * s0 + f) / np.where(epos, e, one)
    t0 = np.where(epos, y0, zero)
    low, high = ~epos | (t0 < 0), epos & (t0 > 1)
    x1 = np.where(low, -c, b - c) / np.where(apos, a, one)
    s1 = np.where(apos, _clamp01(x1, dtype), zero)
    s = np.where(low | high, s1, s0)
    t = np.where(low, zero, np.where(high, one, t0))
    return s.astype(dtype), t.astype(dtype)


def edge_weights_np(j, t, dtype=F):
    w, zero = dtype(1) - t, np.zeros_like(t)
    return ((w, t), (zero, w), (t, zero))[j]


def pierces_np(p, q, d, v, n, dtype=F):
    """rule 3, one edge against one triangle v [..., 3, 3] of normal n: -> pierces, t, (s0, s1, s2)"""
    dp, dq = dot_np(n, p - v[..., 0, :]), dot_np(n, q - v[..., 0, :])
    opposite = ((dp > 0) & (dq < 0)) | ((dp < 0) & (dq > 0))
    w = [v[..., k, :] - p for k in range(3)]
    s = [dot_np(d, cross_np(w[k], w[(k + 1) % 3])) for k in range(3)]
    inside = (((s[0] >= 0) & (s[1] >= 0) & (s[2] >= 0)) | ((s[0] <= 0) & (s[1] <= 0) & (s[2] <= 0))) & ((s[0] != 0) | (s[1] != 0) | (s[2] != 0))
    t = dp / np.where(opposite, dp - dq, dtype(1))
    return opposite & inside, t, s


class Pair:
    """dist2, u, v [...], qa, qb [..., 3], feature int [...] (0 .. 14, 15 none, 16 .. 21 pierced)"""

    def __init__(self, dist2, u, v, qa, qb, feature):
        self.dist2, self.u, self.v, self.qa, self.qb, self.feature = dist2, u, v, qa, qb, feature


def pair_np(a, b, dtype=F):
    """rules 2 and 3: a, b [..., 3, 3] that broadcast -> Pair"""
    a, b = np.asarray(a, dtype), np.asarray(b, dtype)
    shape = np.broadcast(a[..., 0, 0], b[..., 0, 0]).shape
    a, b = np.broadcast_to(a, shape + (3, 3)), np.broadcast_to(b, shape + (3, 3))
    zero, one = dtype(0), dtype(1)
    with np.errstate(all="ignore"):
        alo, ahi = box_np(a)
        blo, bhi = box_np(b)
        ea = [a[..., (i + 1) % 3, :] - a[..., i, :] for i in range(3)]
        eb = [b[..., (j + 1) % 3, :] - b[..., j, :] for j in range(3)]
        best = np.full(shape, np.inf, dtype)
        u, v = np.zeros(shape, dtype), np.zeros(shape, dtype)
        qa, qb = a[..., 0, :].copy(), b[..., 0, :].copy()
        feature = np.full(shape, FEATURE_NONE, np.int64)

        def take(k, d2, fu, fv, fa, fb):
            nonlocal best, u, v, qa, qb, feature
            win = d2 < best
            best, u, v = np.where(win, d2, best), np.where(win, fu, u), np.where(win, fv, v)
            qa, qb = np.where(win[..., None], fa, qa), np.where(win[..., None], fb, qb)
            feature = np.where(win, k, feature)

        for k in range(3):
            d2, fu, fv, q, _ = tri_np(a[..., k, :], b[..., 0, :], b[..., 1, :], b[..., 2, :], dtype)
            take(k, d2, fu, fv, a[..., k, :], q)
        for k in range(3):
            d2, _, _, q, _ = tri_np(b[..., k, :], a[..., 0, :], a[..., 1, :], a[..., 2, :], dtype)
            take(3 + k, d2, np.full(shape, one if k == 0 else zero, dtype), np.full(shape, one if k == 1 else zero, dtype), q, b[..., k, :])
        eaa, ebb = [dot_np(x, x) for x in ea], [dot_np(x, x) for x in eb]
        for i in range(3):
            for j in range(3):
                s, t = segments_np(a[..., i, :], ea[i], eaa[i], b[..., j, :], eb[j], ebb[j], dtype)
                fa = _clamp(a[..., i, :] + ea[i] * s[..., None], alo, ahi)
                fb = _clamp(b[..., j, :] + eb[j] * t[..., None], blo, bhi)
                g = fa - fb
                d2 = (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]
                fu, fv = edge_weights_np(j, t, dtype)
                take(6 + 3 * i + j, d2, fu, fv, fa, fb)
        # piercing overrides the features; the first edge in the order decides
        touch = boxes_touch_np(a, b)
        na, nb = cross_np(ea[0], ea[1]), cross_np(eb[0], eb[1])
        ilo, ihi = np.where(blo > alo, blo, alo), np.where(bhi < ahi, bhi, ahi)
        done = np.zeros(shape, bool)
        for k in range(6):
            i = k % 3
            if k < 3:
                p, q, d, tri, n = a[..., i, :], a[..., (i + 1) % 3, :], ea[i], b, nb
            else:
                p, q, d, tri, n = b[..., i, :], b[..., (i + 1) % 3, :], eb[i], a, na
            hit, t, s = pierces_np(p, q, d, tri, n, dtype)
            hit = hit & touch & ~done
            x = _clamp(p + d * t[..., None], ilo, ihi)
            if k < 3:
                total = (s[0] + s[1]) + s[2]
                total = np.where(hit, total, one)
                fu, fv = s[1] / total, s[2] / total
            else:
                fu, fv = edge_weights_np(i, t, dtype)
            best, u, v = np.where(hit, zero, best), np.where(hit, fu, u), np.where(hit, fv, v)
            qa, qb = np.where(hit[..., None], x, qa), np.where(hit[..., None], x, qb)
            feature = np.where(hit, FEATURE_PIERCE + k, feature)
            done = done | hit
    out = Pair(best.astype(dtype), u.astype(dtype), v.astype(dtype), qa.astype(dtype), qb.astype(dtype), feature)
    assert all(x.dtype == dtype for x in (out.dist2, out.u, out.v, out.qa, out.qb))
    return out


def box_bound_np(lo, hi, alo, ahi, dtype=F):
    """rule 6"""
    lo, hi, alo, ahi = (np.asarray(x, dtype) for x in (lo, hi, alo, ahi))
    with np.errstate(all="ignore"):
        x1, x2 = lo - ahi, alo - hi
        m = np.where(x2 > x1, x2, x1)
        g = np.where(dtype(0) > m, dtype(0), m)
        bound = (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]
    assert bound.dtype == dtype
    return bound


def brute_force_pairs(tris, prims, queries, max2=None, first_prim=None, flags=0, chunk=200000):
    """The answer by rules 1 to 5 over ALL records: tris [T, 3, 3] float32 with ids prims [T], queries [Q, 3, 3] (or [Q, 9]),
    max2 None (RTK_INF) or [Q], first_prim None or [Q] -> (records as the four uint32 words dist2, u, v, prim [Q, 4], the
    points on the query as words [Q, 3], the points on the scene as words [Q, 3])"""
    from rtk_amd.types import RTK_INF
    tris = np.ascontiguousarray(tris, F).reshape(-1, 3, 3)
    prims = np.asarray(prims, np.uint32)
    queries = np.ascontiguousarray(queries, F).reshape(-1, 3, 3)
    Q, T = len(queries), len(tris)
    max2 = np.full(Q, RTK_INF, F) if max2 is None else np.ascontiguousarray(max2, F)
    first = np.zeros(Q, np.uint32) if first_prim is None else np.asarray(first_prim, np.uint32)
    rec = np.zeros((Q, 4), np.uint32)
    rec[:, 0] = max2.view(np.uint32)
    rec[:, 3] = NONE
    pa = queries[:, 0, :].copy().view(np.uint32)
    pb = pa.copy()
    if T == 0 or Q == 0:
        return rec, pa, pb
    order = np.argsort(prims, kind="stable")
    rows = max(1, chunk // T)
    for at in range(0, Q, rows):
        sl = slice(at, min(at + rows, Q))
        a = queries[sl]
        r = pair_np(a[:, None], tris[None])
        with np.errstate(invalid="ignore"):
            ok = (live_np(a) & (max2[sl] > 0))[:, None] & (prims[None, :] >= first[sl, None]) & (r.dist2 < max2[sl, None])
        if flags & SKIP_SHARED_VERTEX:
            ok = ok & ~shares_vertex_np(a[:, None], tris[None])
        d = np.where(ok, r.dist2, F(np.inf))
        best = d.min(1)
        tie = ok & (d == best[:, None])
        prim = np.where(tie, prims[None, :], np.uint32(NONE)).min(1)
        hit = np.nonzero(prim != NONE)[0]
        col = order[np.searchsorted(prims[order], prim[hit])]
        rec[at + hit, 0] = r.dist2[hit, col].view(np.uint32)
        rec[at + hit, 1] = r.u[hit, col].view(np.uint32)
        rec[at + hit, 2] = r.v[hit, col].view(np.uint32)
        rec[at + hit, 3] = prim[hit]
        pa[at + hit] = r.qa[hit, col].view(np.uint32)
        pb[at + hit] = r.qb[hit, col].view(np.uint32)
    return rec, pa, pb
