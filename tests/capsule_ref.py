"""The rule of rtk_amd/csrc/rtk_capsule_rule.h restated in numpy, for tests/test_capsule_cpu.py (against the header's driver) and
tests/test_gpu_capsule.py (against the kernel): every product, sum, difference, quotient and square root is one operation of
`dtype`, in the header's order. With dtype float32 it states the expected bits; with float64 it is the yardstick of the accuracy
statement. Everything is evaluated for every (query, triangle) pair and selected afterwards: no early exit changes a value."""
import numpy as np

from tests.closest_ref import tri_box, tri_np
from tests.pair_ref import edge_weights_np, pierces_np, segments_np
from tests.sweep_ref import _entry, better_np, centre_np  # noqa: F401  (better_np: the sphere sweep's, used unchanged)
from tests.touch_ref import cross_np, dot_np

NONE = 0xFFFFFFFF
CP_NONE, CP_START, CP_FACE, CP_EDGE, CP_VERTEX, CP_FEATURES = 0, 1, 2, 10, 22, 28
ITEM_NONE, ITEM_PIERCE, ITEM_END0, ITEM_END1, ITEM_EDGE = 0, 1, 2, 3, 4
# indices into V = (a-, b-, c-, a+, b+, c+)
FACE_PICKS = ((0, 1, 2), (3, 4, 5), (1, 4, 0), (3, 0, 4), (2, 5, 1), (4, 1, 5), (0, 3, 2), (5, 2, 3))
EDGE_PICKS = ((0, 1), (1, 2), (2, 0), (3, 4), (4, 5), (5, 3), (0, 3), (1, 4), (2, 5), (0, 4), (1, 5), (2, 3))
_V = ("a-", "b-", "c-", "a+", "b+", "c+")
FEATURE_NAMES = ("none", "start") + tuple("face " + " ".join(_V[i] for i in f) for f in FACE_PICKS) \
    + tuple("edge " + " ".join(_V[i] for i in e) for e in EDGE_PICKS) + tuple("vertex " + v for v in _V)


def _clamp(x, lo, hi):
    return np.where(x < lo, lo, np.where(x > hi, hi, x))


class Query:
    """0. of the header: O, D, S, h, g, p0, p1 [..., 3]; tmin, tmax, r, r2, dd, live [...]"""

    def at(self, index):
        q = Query()
        for k, v in self.__dict__.items():
            setattr(q, k, v[index])
        return q

    def copy(self):
        q = Query()
        q.__dict__.update(self.__dict__)
        return q


def finish(q):
    """what 0. forms from O, D, tmin, tmax, r, h (again after a test has moved one of them)"""
    with np.errstate(all="ignore"):
        q.r2 = q.r * q.r
        q.dd = dot_np(q.D, q.D)
        q.S = q.O + q.D * q.tmin[..., None]
        q.g = q.r[..., None] + np.where(q.h < 0, -q.h, q.h)
        q.p0, q.p1 = q.S - q.h, q.S + q.h
    return q


def prepare(sweeps, dtype=np.float32):
    """sweeps: float32 [n, 12] (origin, direction, min_t, max_t, radius, half_axis) -> Query with leading shape [n]"""
    w = np.ascontiguousarray(sweeps, np.float32).reshape(-1, 12)
    q = Query()
    with np.errstate(all="ignore"):
        q.O, q.D, q.h = w[:, 0:3].astype(dtype), w[:, 3:6].astype(dtype), w[:, 9:12].astype(dtype)
        q.tmin, q.tmax, q.r = w[:, 6].astype(dtype), w[:, 7].astype(dtype), w[:, 8].astype(dtype)
        q.live = np.isfinite(w).all(1) & (w[:, 3:6] != 0).any(1) & (w[:, 8] >= 0) & (w[:, 6] <= w[:, 7])
    return finish(q)


def slab_np(q, lo, hi):
    """1.: the box [lo, hi] [..., 3] grown by g against the path -> (not empty, te)"""
    with np.errstate(all="ignore"):
        shape = np.broadcast(q.tmin, lo[..., 0]).shape
        t0, t1 = np.broadcast_to(q.tmin, shape), np.broadcast_to(q.tmax, shape)
        inside = np.ones(shape, bool)
        for k in range(3):
            l, h, d, o = lo[..., k] - q.g[..., k], hi[..., k] + q.g[..., k], q.D[..., k], q.O[..., k]
            zero = np.broadcast_to(d == 0, shape)
            tl, th = (l - o) / d, (h - o) / d
            tn, tf = np.where(d > 0, tl, th), np.where(d > 0, th, tl)
            t0 = np.where(zero, t0, np.where(tn > t0, tn, t0))
            t1 = np.where(zero, t1, np.where(tf < t1, tf, t1))
            inside = inside & (~zero | ((l <= o) & (o <= h)))
    assert t0.dtype == q.tmin.dtype
    return inside & (t0 <= t1), t0


class Contact:
    """dist2, u, v [...], qt, qa [..., 3], item int [...]"""


def distance_np(p0, p1, a, b, c, dtype=np.float32):
    """2. (ii): the distance walk of the segment [p0, p1] and the triangle (a, b, c), all [..., 3] that broadcast -> Contact"""
    p0, p1, a, b, c = np.broadcast_arrays(*(np.asarray(x, dtype) for x in (p0, p1, a, b, c)))
    shape = p0.shape[:-1]
    zero = dtype(0)
    with np.errstate(all="ignore"):
        x = p1 - p0
        slo, shi = np.where(p1 < p0, p1, p0), np.where(p1 > p0, p1, p0)
        lo, hi = tri_box(a, b, c)
        touch = ((lo <= shi) & (hi >= slo)).all(-1)
        v = (a, b, c)
        e = (b - a, c - b, a - c)
        best = np.full(shape, np.inf, dtype)
        fu, fv = np.zeros(shape, dtype), np.zeros(shape, dtype)
        qt, qa = a.copy(), p0.copy()
        item = np.full(shape, ITEM_NONE, np.int64)

        def take(k, d2, u, w, pt, pa):
            nonlocal best, fu, fv, qt, qa, item
            win = d2 < best
            best, fu, fv = np.where(win, d2, best), np.where(win, u, fu), np.where(win, w, fv)
            qt, qa = np.where(win[..., None], pt, qt), np.where(win[..., None], pa, qa)
            item = np.where(win, k, item)

        for k, p in enumerate((p0, p1)):
            d2, u, w, q, _ = tri_np(p, a, b, c, dtype)
            take(ITEM_END0 + k, d2, u, w, q, p)
        xx = dot_np(x, x)
        for j in range(3):
            s, t = segments_np(p0, x, xx, v[j], e[j], dot_np(e[j], e[j]), dtype)
            pa = _clamp(p0 + x * s[..., None], slo, shi)
            pb = _clamp(v[j] + e[j] * t[..., None], lo, hi)
            f = pa - pb
            d2 = (f[..., 0] * f[..., 0] + f[..., 1] * f[..., 1]) + f[..., 2] * f[..., 2]
            u, w = edge_weights_np(j, t, dtype)
            take(ITEM_EDGE + j, d2, u, w, pb, pa)
        # a pierce overrides the five
        n = cross_np(e[0], e[1])
        hit, t, s = pierces_np(p0, p1, x, np.stack([a, b, c], -2), n, dtype)
        hit = hit & touch
        at = _clamp(p0 + x * t[..., None], np.where(lo > slo, lo, slo), np.where(hi < shi, hi, shi))
        total = np.where(hit, (s[0] + s[1]) + s[2], dtype(1))
        best, fu, fv = np.where(hit, zero, best), np.where(hit, s[1] / total, fu), np.where(hit, s[2] / total, fv)
        qt, qa = np.where(hit[..., None], at, qt), np.where(hit[..., None], at, qa)
        item = np.where(hit, ITEM_PIERCE, item)
    r = Contact()
    r.dist2, r.u, r.v, r.qt, r.qa, r.item = best.astype(dtype), fu.astype(dtype), fv.astype(dtype), qt.astype(dtype), qa.astype(dtype), item
    return r


def tri_capsule_np(q, a, b, c, dtype=np.float32):
    """2.: q (made with the same dtype) broadcastable against a, b, c [..., 3] -> (feature [...] as the header's enum, t [...];
    t = max_t where the feature is none)"""
    a, b, c = (np.asarray(x, dtype) for x in (a, b, c))
    with np.errstate(all="ignore"):
        lo, hi = tri_box(a, b, c)
        ok, te = slab_np(q, lo, hi)
        shape = ok.shape
        start = distance_np(q.p0, q.p1, a, b, c, dtype).dist2 <= q.r2
        whole = q
        q = whole.copy()                         # (iii) is measured from the centre at te
        q.O = centre_np(whole, te)
        q.tmin, q.tmax = whole.tmin - te, whole.tmax - te
        in_range = lambda t: (q.tmin <= t) & (t <= q.tmax)
        feature = np.zeros(shape, np.int64)
        best = np.zeros(shape, dtype)

        def take(valid, t, code):
            nonlocal feature, best
            win = valid & ((feature == CP_NONE) | (t < best))
            feature = np.where(win, code, feature)
            best = np.where(win, t, best)

        V = (a - q.h, b - q.h, c - q.h, a + q.h, b + q.h, c + q.h)
        V = tuple(np.broadcast_to(x, shape + (3,)) for x in V)
        D = np.broadcast_to(q.D, shape + (3,))
        for i, (ia, ib, ic) in enumerate(FACE_PICKS):
            A, B, C = V[ia], V[ib], V[ic]
            ab, ac, ma = B - A, C - A, q.O - A
            n = cross_np(ab, ac)
            nn = dot_np(n, n)
            length = np.sqrt(nn)
            h0, hd = dot_np(n, ma), dot_np(n, D)
            hs = h0 + q.tmin * hd
            sr = np.where(hs < 0, -q.r, q.r)
            t = (sr * length - h0) / hd
            region = tri_np(centre_np(q, np.where(np.isfinite(t), t, 0).astype(dtype)), A, B, C, dtype)[4]
            take((nn > 0) & (hd != 0) & in_range(t) & (region == 7), t, CP_FACE + i)
        for i, (ip, iq) in enumerate(EDGE_PICKS):
            e, m = V[iq] - V[ip], q.O - V[ip]
            ee, nd, md = dot_np(e, e), dot_np(e, D), dot_np(e, m)
            Dp, mp = D - e * (nd / ee)[..., None], m - e * (md / ee)[..., None]
            A = dot_np(Dp, Dp)
            real, t = _entry(q, mp, Dp, A, dot_np(mp, Dp))
            w = md + t * nd
            take((ee > 0) & (A > 0) & real & (0 <= w) & (w <= ee) & in_range(t), t, CP_EDGE + i)
        for i in range(6):
            m = q.O - V[i]
            real, t = _entry(q, m, D, q.dd, dot_np(m, D))
            take(real & in_range(t), t, CP_VERTEX + i)

        q = whole
        time = te + best
        time = np.where(start, np.broadcast_to(q.tmin, shape), time)
        feature = np.where(start, CP_START, feature)
        feature = np.where(ok, feature, CP_NONE)
        time = np.where(te > time, te, time)
        feature = np.where(time > q.tmax, CP_NONE, feature)                  # (iv): a time beyond max_t is none
        t = np.where(feature != CP_NONE, time, np.broadcast_to(q.tmax, shape))
    assert t.dtype == dtype
    return feature, t


def record_np(q, t, a, b, c, dtype=np.float32):
    """the record: the distance walk at c(t) -> Contact"""
    with np.errstate(all="ignore"):
        ct = centre_np(q, t)
        return distance_np(ct - q.h, ct + q.h, a, b, c, dtype)


def brute_force(tris, prims, sweeps, mesh_of=None, filter=None, chunk=60000):
    """The answer over ALL triangles: tris [T, 3, 3] float32 with ids prims [T], sweeps float32 [Q, 12]; mesh_of [T]: the mesh
    index of each triangle; filter: dict with 'mesh_mask' (bools per mesh; meshes beyond it are not candidates) and / or
    'ignore_prim' (one id per query) -> (records as the four uint32 words t, u, v, prim [Q, 4], the points on the triangle as
    words [Q, 3], the points on the axis as words [Q, 3])."""
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 3, 3)
    prims = np.asarray(prims, np.uint32)
    sweeps = np.ascontiguousarray(sweeps, np.float32).reshape(-1, 12)
    Q, T = len(sweeps), len(tris)
    rec = np.zeros((Q, 4), np.uint32)
    rec[:, 0] = sweeps[:, 7].view(np.uint32)
    rec[:, 3] = NONE
    pts = sweeps[:, 0:3].copy().view(np.uint32)
    axs = pts.copy()
    if T == 0 or Q == 0:
        return rec, pts, axs
    filter = filter or {}
    order = np.argsort(prims, kind="stable")
    rows = max(1, chunk // T)
    for at in range(0, Q, rows):
        sl = slice(at, min(at + rows, Q))
        q = prepare(sweeps[sl])
        feature, t = tri_capsule_np(q.at((slice(None), None)), tris[None, :, 0], tris[None, :, 1], tris[None, :, 2])
        cand = (feature != CP_NONE) & q.live[:, None]
        if filter.get("mesh_mask") is not None:
            mask = np.asarray(filter["mesh_mask"], bool)
            mesh = np.asarray(mesh_of, np.int64)
            cand &= ((mesh < len(mask)) & mask[np.minimum(mesh, len(mask) - 1)])[None, :]
        if filter.get("ignore_prim") is not None:
            cand &= prims[None, :] != np.asarray(filter["ignore_prim"], np.uint32)[sl, None]
        best = np.where(cand, t, np.float32(np.inf)).min(1)
        tie = cand & (t == best[:, None])
        prim = np.where(tie, prims[None, :], np.uint32(NONE)).min(1)
        hit = np.nonzero(prim != NONE)[0]
        col = order[np.searchsorted(prims[order], prim[hit])]
        th = t[hit, col]
        r = record_np(q.at(hit), th, tris[col, 0], tris[col, 1], tris[col, 2])
        rec[at + hit, 0] = th.view(np.uint32)
        rec[at + hit, 1] = r.u.view(np.uint32)
        rec[at + hit, 2] = r.v.view(np.uint32)
        rec[at + hit, 3] = prim[hit]
        pts[at + hit] = np.ascontiguousarray(r.qt).view(np.uint32)
        axs[at + hit] = np.ascontiguousarray(r.qa).view(np.uint32)
    return rec, pts, axs
