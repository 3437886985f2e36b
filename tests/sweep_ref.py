"""The rule of rtk_amd/csrc/rtk_sweep_rule.h restated in numpy, for tests/test_sweep_cpu.py (against the header's driver) and
tests/test_gpu_sweep.py (against the kernel): every product, sum, difference, quotient and square root is one operation of
`dtype`, in the header's order. With dtype float32 it states the expected bits; with float64 it is the yardstick of the accuracy
statement. Everything is evaluated for every (query, triangle) pair and selected afterwards: no early exit changes a value."""
import numpy as np

from tests.closest_ref import tri_box, tri_np

NONE = 0xFFFFFFFF
SW_NONE, SW_START, SW_FACE, SW_EDGE_AB, SW_EDGE_BC, SW_EDGE_CA, SW_VERTEX_A, SW_VERTEX_B, SW_VERTEX_C = range(9)
FEATURE_NAMES = ("none", "start", "face", "edge ab", "edge bc", "edge ca", "vertex a", "vertex b", "vertex c")


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


class Query:
    """0. of the header: O, D, S [..., 3]; tmin, tmax, r, r2, dd, live [...]"""

    def at(self, index):
        q = Query()
        for k, v in self.__dict__.items():
            setattr(q, k, v[index])
        return q


def prepare(sweeps, dtype=np.float32):
    """sweeps: float32 [n, 9] (origin, direction, min_t, max_t, radius) -> Query with leading shape [n]"""
    w = np.ascontiguousarray(sweeps, np.float32).reshape(-1, 9)
    q = Query()
    with np.errstate(all="ignore"):
        q.O, q.D = w[:, 0:3].astype(dtype), w[:, 3:6].astype(dtype)
        q.tmin, q.tmax, q.r = w[:, 6].astype(dtype), w[:, 7].astype(dtype), w[:, 8].astype(dtype)
        q.r2 = q.r * q.r
        q.dd = _dot(q.D, q.D)
        q.S = q.O + q.D * q.tmin[:, None]
        q.live = np.isfinite(w).all(1) & (w[:, 3:6] != 0).any(1) & (w[:, 8] >= 0) & (w[:, 6] <= w[:, 7])
    return q


def centre_np(q, t):
    with np.errstate(all="ignore"):
        return q.O + q.D * t[..., None]


def slab_np(q, lo, hi):
    """1.: the box [lo, hi] [..., 3] grown by r against the path -> (not empty, te)"""
    with np.errstate(all="ignore"):
        shape = np.broadcast(q.tmin, lo[..., 0]).shape
        t0, t1 = np.broadcast_to(q.tmin, shape), np.broadcast_to(q.tmax, shape)
        inside = np.ones(shape, bool)
        for k in range(3):
            l, h, d, o = lo[..., k] - q.r, hi[..., k] + q.r, q.D[..., k], q.O[..., k]
            zero = np.broadcast_to(d == 0, shape)
            tl, th = (l - o) / d, (h - o) / d
            tn, tf = np.where(d > 0, tl, th), np.where(d > 0, th, tl)
            t0 = np.where(zero, t0, np.where(tn > t0, tn, t0))
            t1 = np.where(zero, t1, np.where(tf < t1, tf, t1))
            inside = inside & (~zero | ((l <= o) & (o <= h)))
    assert t0.dtype == q.tmin.dtype
    return inside & (t0 <= t1), t0


def _entry(q, m, D, A, B):
    """the time the path m + D * t (A = dot(D, D), B = dot(m, D)) enters the ball of radius r about 0, by its closest approach:
    t0 = -B / A, m0 = m + D * t0, disc = r2 - dot(m0, m0), t = t0 - sqrt(disc / A) -> (disc >= 0, t)"""
    t0 = -B / A
    m0 = m + D * t0[..., None]
    disc = q.r2 - _dot(m0, m0)
    return disc >= 0, t0 - np.sqrt(disc / A)


def tri_sweep_np(q, a, b, c, dtype=np.float32):
    """2.: q (made with the same dtype) broadcastable against a, b, c [..., 3] -> (feature [...] as the header's enum, t [...];
    t = max_t where the feature is none)"""
    a, b, c = (np.asarray(x, dtype) for x in (a, b, c))
    with np.errstate(all="ignore"):
        lo, hi = tri_box(a, b, c)
        ok, te = slab_np(q, lo, hi)
        shape = ok.shape
        dist2 = tri_np(q.S, a, b, c, dtype)[0]
        start = dist2 <= q.r2
        whole = q
        q = Query()                              # (iii) is measured from the centre at te
        q.__dict__.update(whole.__dict__)
        q.O = centre_np(whole, te)
        q.tmin, q.tmax = whole.tmin - te, whole.tmax - te
        in_range = lambda t: (q.tmin <= t) & (t <= q.tmax)
        feature = np.zeros(shape, np.int64)
        best = np.zeros(shape, dtype)

        def take(valid, t, code):
            nonlocal feature, best
            win = valid & ((feature == SW_NONE) | (t < best))
            feature = np.where(win, code, feature)
            best = np.where(win, t, best)

        ab, ac, ma = b - a, c - a, q.O - a
        n = np.stack([ab[..., 1] * ac[..., 2] - ab[..., 2] * ac[..., 1], ab[..., 2] * ac[..., 0] - ab[..., 0] * ac[..., 2],
                      ab[..., 0] * ac[..., 1] - ab[..., 1] * ac[..., 0]], -1)
        nn = _dot(n, n)
        length = np.sqrt(nn)
        h0, hd = _dot(n, ma), _dot(n, q.D)
        hs = h0 + q.tmin * hd
        sr = np.where(hs < 0, -q.r, q.r)
        t = (sr * length - h0) / hd
        region = tri_np(centre_np(q, np.where(np.isfinite(t), t, 0).astype(dtype)), a, b, c, dtype)[4]
        take((nn > 0) & (hd != 0) & in_range(t) & (region == 7), t, SW_FACE)

        mb, mc, bc, ca = q.O - b, q.O - c, c - b, a - c
        D = np.broadcast_to(q.D, ma.shape)
        for i, (e, m) in enumerate(((ab, ma), (bc, mb), (ca, mc))):
            ee, nd, md = _dot(e, e), _dot(e, D), _dot(e, m)
            Dp, mp = D - e * (nd / ee)[..., None], m - e * (md / ee)[..., None]
            A = _dot(Dp, Dp)
            real, t = _entry(q, mp, Dp, A, _dot(mp, Dp))
            w = md + t * nd
            take((ee > 0) & (A > 0) & real & (0 <= w) & (w <= ee) & in_range(t), t, SW_EDGE_AB + i)
        for i, m in enumerate((ma, mb, mc)):
            real, t = _entry(q, m, D, q.dd, _dot(m, D))
            take(real & in_range(t), t, SW_VERTEX_A + i)

        q = whole
        time = te + best
        time = np.where(start, np.broadcast_to(q.tmin, shape), time)
        feature = np.where(start, SW_START, feature)
        feature = np.where(ok, feature, SW_NONE)
        time = np.where(te > time, te, time)
        feature = np.where(time > q.tmax, SW_NONE, feature)                  # (iv): a time beyond max_t is none
        t = np.where(feature != SW_NONE, time, np.broadcast_to(q.tmax, shape))
    assert t.dtype == dtype
    return feature, t


def better_np(t, prim, best_t, best_prim):
    with np.errstate(invalid="ignore"):
        return (t < best_t) | ((t == best_t) & (prim < best_prim))


def brute_force(tris, prims, sweeps, mesh_of=None, filter=None):
    """The answer over ALL triangles: tris [T, 3, 3] float32 with ids prims [T], sweeps float32 [Q, 9]; mesh_of [T]: the mesh
    index of each triangle; filter: dict with 'mesh_mask' (bools per mesh; meshes beyond it are not candidates) and / or
    'ignore_prim' (one id per query) -> (records as the four uint32 words t, u, v, prim [Q, 4], contact points as words [Q, 3],
    centres as words [Q, 3])."""
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 3, 3)
    prims = np.asarray(prims, np.uint32)
    sweeps = np.ascontiguousarray(sweeps, np.float32).reshape(-1, 9)
    Q, T = len(sweeps), len(tris)
    rec = np.zeros((Q, 4), np.uint32)
    rec[:, 0] = sweeps[:, 7].view(np.uint32)
    rec[:, 3] = NONE
    pts = sweeps[:, 0:3].copy().view(np.uint32)
    ctr = pts.copy()
    if T == 0 or Q == 0:
        return rec, pts, ctr
    q = prepare(sweeps)
    feature, t = tri_sweep_np(q.at((slice(None), None)), tris[None, :, 0], tris[None, :, 1], tris[None, :, 2])
    cand = (feature != SW_NONE) & q.live[:, None]
    filter = filter or {}
    if filter.get("mesh_mask") is not None:
        mask = np.asarray(filter["mesh_mask"], bool)
        mesh_of = np.asarray(mesh_of, np.int64)
        cand &= ((mesh_of < len(mask)) & mask[np.minimum(mesh_of, len(mask) - 1)])[None, :]
    if filter.get("ignore_prim") is not None:
        cand &= prims[None, :] != np.asarray(filter["ignore_prim"], np.uint32)[:, None]
    best = np.where(cand, t, np.float32(np.inf)).min(1)
    tie = cand & (t == best[:, None])
    prim = np.where(tie, prims[None, :], np.uint32(NONE)).min(1)
    hit = np.nonzero(prim != NONE)[0]
    col = np.argsort(prims, kind="stable")[np.searchsorted(np.sort(prims), prim[hit])]
    th = t[hit, col]
    c = centre_np(q.at(hit), th)
    _, u, v, qq, _ = tri_np(c, tris[col, 0], tris[col, 1], tris[col, 2])
    rec[hit, 0] = th.view(np.uint32)
    rec[hit, 1] = u.view(np.uint32)
    rec[hit, 2] = v.view(np.uint32)
    rec[hit, 3] = prim[hit]
    pts[hit] = np.ascontiguousarray(qq).view(np.uint32)
    ctr[hit] = np.ascontiguousarray(c).view(np.uint32)
    return rec, pts, ctr
