"""Instanced worlds in numpy: the rules of rtk_amd/csrc/rtk_world_rule.h in the stated order (float64 for the inverse, rounded
once; float32 for the ray and the box), the fixtures of the GPU test and a float64 brute force over placed triangles."""
import numpy as np

F = np.float32
RTK_INF = F(3.402823e+38)
PRIM_NONE = 0xFFFFFFFF
WORLD_PAD = F(2.0 ** -11)
RAY_DTYPE = np.dtype([("origin", "<f4", (3,)), ("direction", "<f4", (3,)), ("min_t", "<f4"), ("max_t", "<f4")])


def place_np(m, v):
    """rtk_place_rule.h: ((m0 x + m1 y) + m2 z) + m3 per row, every operation in float32. m [..., 12], v [..., 3]."""
    m, v = np.asarray(m, F), np.asarray(v, F)
    with np.errstate(all="ignore"):
        return np.stack([((m[..., 4 * j] * v[..., 0] + m[..., 4 * j + 1] * v[..., 1]) + m[..., 4 * j + 2] * v[..., 2]) + m[..., 4 * j + 3]
                         for j in range(3)], -1)


def inverse_np(m):
    """rtk_world_inverse: m [n, 12] float32 -> (inv [n, 12] float32, live [n])."""
    m = np.asarray(m, F).reshape(-1, 12).astype(np.float64)
    a, b, c, T0, d, e, f, T1, g, h, i, T2 = [m[:, k] for k in range(12)]
    with np.errstate(all="ignore"):
        co = [e * i - f * h, c * h - b * i, b * f - c * e,
              f * g - d * i, a * i - c * g, c * d - a * f,
              d * h - e * g, b * g - a * h, a * e - b * d]
        det = (a * co[0] + b * co[3]) + c * co[6]
        out = np.zeros((m.shape[0], 12), np.float64)
        for j in range(3):
            r0, r1, r2 = co[3 * j] / det, co[3 * j + 1] / det, co[3 * j + 2] / det
            out[:, 4 * j], out[:, 4 * j + 1], out[:, 4 * j + 2] = r0, r1, r2
            out[:, 4 * j + 3] = -((r0 * T0 + r1 * T1) + r2 * T2)
        inv = out.astype(F)
    live = (det != 0) & np.isfinite(det) & np.isfinite(inv).all(1)
    return inv, live


def ray_np(inv, rays):
    """rtk_world_ray: inv [12], rays [n, 8] float32 -> [n, 8]."""
    inv, rays = np.asarray(inv, F), np.asarray(rays, F)
    out = rays.copy()
    out[:, 0:3] = place_np(inv, rays[:, 0:3])
    with np.errstate(all="ignore"):
        for j in range(3):
            out[:, 3 + j] = (inv[4 * j] * rays[:, 3] + inv[4 * j + 1] * rays[:, 4]) + inv[4 * j + 2] * rays[:, 5]
    return out


def box_np(root_lo, root_hi, m):
    """rtk_world_box: (lo [3], hi [3], finite)."""
    root_lo, root_hi, m = np.asarray(root_lo, F), np.asarray(root_hi, F), np.asarray(m, F)
    lo = hi = None
    for k in range(8):
        c = place_np(m, np.array([root_hi[0] if k & 1 else root_lo[0], root_hi[1] if k & 2 else root_lo[1], root_hi[2] if k & 4 else root_lo[2]], F))
        if k == 0:
            lo, hi = c.copy(), c.copy()
        else:
            lo = np.where(c < lo, c, lo)
            hi = np.where(c > hi, c, hi)
    B = S = F(0)
    for a in range(3):
        l, u, t = [x if not x < 0 else -x for x in (lo[a], hi[a], m[4 * a + 3])]
        B = l if l > B else B
        B = u if u > B else B
        S = t if t > S else S
    with np.errstate(all="ignore"):
        pad = WORLD_PAD * (B + S)
        lo, hi = (lo + -pad).astype(F), (hi + pad).astype(F)
    return lo, hi, bool(np.isfinite(lo).all() and np.isfinite(hi).all())


def margin_np(origin, bound):
    O = F(0)
    for a in range(3):
        v = origin[a] if not origin[a] < 0 else -origin[a]
        O = v if v > O else O
    with np.errstate(all="ignore"):
        return WORLD_PAD * (O + F(bound))


# ---------------------------------------------------------------------------- fixtures

def cube():
    """12 triangles, [-1, 1]^3"""
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], F)
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return np.array([[v[a], v[b], v[c]] for s in q for a, b, c in ((s[0], s[1], s[2]), (s[0], s[2], s[3]))], F)


def icosphere(level=2, radius=1.0):
    """20 * 4^level triangles on a sphere (level 2: 320)"""
    p = (1 + 5 ** 0.5) / 2
    v = np.array([[-1, p, 0], [1, p, 0], [-1, -p, 0], [1, -p, 0], [0, -1, p], [0, 1, p], [0, -1, -p], [0, 1, -p], [p, 0, -1], [p, 0, 1], [-p, 0, -1], [-p, 0, 1]], np.float64)
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    t = np.array([[v[a], v[b], v[c]] for a, b, c in f])
    for _ in range(level):
        a, b, c = t[:, 0], t[:, 1], t[:, 2]
        ab, bc, ca = (a + b) / 2, (b + c) / 2, (c + a) / 2
        t = np.concatenate([np.stack(x, 1) for x in ((a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca))])
    t = t / np.linalg.norm(t, axis=2, keepdims=True) * radius
    return t.astype(F)


def line_scene(n=2048):
    """n triangles across a line, each in a plane x = 100 * 0.997^k (100 down to 0.21, neighbours at least 6e-4 apart, so that
    their t stay apart in float) with the x axis through its inside: the spacing makes the tree deep, and a ray along the axis
    enters every box"""
    x = 100.0 * 0.997 ** np.arange(n)
    t = np.zeros((n, 3, 3))
    t[:, :, 0] = x[:, None]
    t[:, 0, 1:], t[:, 1, 1:], t[:, 2, 1:] = (-1, -1), (2, -1), (-1, 2)
    return t.astype(F)


def rotation(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def placement(A=None, T=(0, 0, 0)):
    m = np.zeros((3, 4))
    m[:, :3] = np.eye(3) if A is None else A
    m[:, 3] = T
    return m.reshape(12).astype(F)


def random_placements(n, rng, spread=40.0):
    """rotations with a uniform scale in [0.5, 2] (condition number 1), spread over a cube"""
    out = np.zeros((n, 12), F)
    for i in range(n):
        out[i] = placement(rotation(rng.standard_normal(3), rng.uniform(0, 2 * np.pi)) * rng.uniform(0.5, 2.0), rng.uniform(-spread, spread, 3))
    return out


def world_tris64(tris, m):
    """the placed triangles in float64 (the exact map of the float32 placement): [T, 3, 3]"""
    m = np.asarray(m, np.float64).reshape(3, 4)
    return tris.astype(np.float64) @ m[:, :3].T + m[:, 3]


def make_rays(placed, rng, n_hit=4096, n_miss=512):
    """placed: list of [T, 3, 3] float64 world triangles per live instance. n_hit rays aimed at inside points (barycentrics >= 0.1)
    from origins within 3 world extents of the centre, |d| in [0.5, 2]; n_miss rays that start outside and point away."""
    allv = np.concatenate([p.reshape(-1, 3) for p in placed])
    lo, hi = allv.min(0), allv.max(0)
    centre, R = (lo + hi) / 2, np.linalg.norm(hi - lo) / 2
    rays = np.zeros(n_hit + n_miss, RAY_DTYPE)
    which = rng.randint(0, len(placed), n_hit)
    for k in range(n_hit):
        t = placed[which[k]][rng.randint(len(placed[which[k]]))]
        w = rng.uniform(0.1, 1.0, 3)
        w = 0.1 + 0.7 * w / w.sum()
        p = w @ t
        d = rng.standard_normal(3)
        o = centre + d / np.linalg.norm(d) * R * rng.uniform(1.2, 3.0)
        rays["origin"][k] = o
        rays["direction"][k] = (p - o) / np.linalg.norm(p - o) * rng.uniform(0.5, 2.0)
    d = rng.standard_normal((n_miss, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays["origin"][n_hit:] = centre + d * R * 1.5
    rays["direction"][n_hit:] = d * rng.uniform(0.5, 2.0, (n_miss, 1))
    rays["max_t"] = RTK_INF
    return rays


def brute64(placed, rays):
    """float64 Moeller-Trumbore over every placed triangle an instance's box lets through: per ray the two smallest t with their
    (instance, triangle), as (t [n, 2], inst [n, 2], tri [n, 2]); inf / -1 where there is none. Instances whose box a ray's line
    misses (float64 slab test on a box grown by 1e-6 of its size) hold no candidate of it and are skipped."""
    o, d = rays["origin"].astype(np.float64), rays["direction"].astype(np.float64)
    n = len(rays)
    bt = np.full((n, 2), np.inf)
    bi = np.full((n, 2), -1, np.int64)
    bp = np.full((n, 2), -1, np.int64)
    with np.errstate(all="ignore"):
        rd = 1.0 / d
        for k, t in enumerate(placed):
            lo, hi = t.reshape(-1, 3).min(0), t.reshape(-1, 3).max(0)
            g = (hi - lo).max() * 1e-6 + 1e-12
            t0, t1 = (lo - g - o) * rd, (hi + g - o) * rd
            tn, tf = np.minimum(t0, t1).max(1), np.maximum(t0, t1).min(1)
            sel = np.flatnonzero((tn <= tf) & (tf >= 0))
            if not sel.size:
                continue
            e1, e2 = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
            for c0 in range(0, sel.size, 256):
                s = sel[c0:c0 + 256]
                pv = np.cross(d[s][:, None, :], e2[None])
                det = (pv * e1[None]).sum(2)
                tv = o[s][:, None, :] - t[None, :, 0]
                u = (tv * pv).sum(2) / det
                qv = np.cross(tv, e1[None])
                v = (d[s][:, None, :] * qv).sum(2) / det
                tt = (e2[None] * qv).sum(2) / det
                ok = (u >= 0) & (v >= 0) & (u + v <= 1) & (tt > 0) & (det != 0)
                tt = np.where(ok, tt, np.inf)
                for _ in range(2):
                    j = tt.argmin(1)
                    cand = tt[np.arange(s.size), j]
                    tt[np.arange(s.size), j] = np.inf
                    cat_t = np.concatenate([bt[s], cand[:, None]], 1)
                    cat_i = np.concatenate([bi[s], np.full((s.size, 1), k)], 1)
                    cat_p = np.concatenate([bp[s], j[:, None]], 1)
                    order = np.argsort(cat_t, 1, kind="stable")[:, :2]
                    rows = np.arange(s.size)[:, None]
                    bt[s], bi[s], bp[s] = cat_t[rows, order], cat_i[rows, order], cat_p[rows, order]
    bi[~np.isfinite(bt)] = -1
    bp[~np.isfinite(bt)] = -1
    return bt, bi, bp
