"""The rule of rtk_amd/csrc/rtk_boxsweep_rule.h restated in numpy, for tests/test_boxsweep_cpu.py (against the header's driver)
and tests/test_gpu_boxsweep.py (against the kernel): every product, sum, difference, quotient and square root is one operation of
`dtype`, in the header's order. With dtype float32 it states the expected bits; with float64 it is the yardstick of the accuracy
statement. Everything is evaluated for every (query, triangle) pair and selected afterwards: no early exit changes a value.
(tests/sweep_ref.py's slab_np grows a box by one radius on all axes and gives neither the exit time nor the axis: restated here.)"""
import numpy as np

from tests.closest_ref import tri_box, tri_np
from tests.sweep_ref import better_np  # noqa: F401  (3. of the header is the sphere rule's)

NONE = 0xFFFFFFFF
BS_NONE, BS_START, BS_BOX_X, BS_BOX_Y, BS_BOX_Z, BS_NORMAL, BS_EDGE = range(7)
BS_AXES = 15
AXIS_NAMES = ("none", "start", "box x", "box y", "box z", "normal") + tuple("%s x %s" % (e, j) for e in ("ab", "bc", "ca") for j in "xyz")


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def _cross(x, y):
    return np.stack([x[..., 1] * y[..., 2] - x[..., 2] * y[..., 1], x[..., 2] * y[..., 0] - x[..., 0] * y[..., 2],
                     x[..., 0] * y[..., 1] - x[..., 1] * y[..., 0]], -1)


def _min(x, y):
    return np.where(y < x, y, x)


def _max(x, y):
    return np.where(y > x, y, x)


class Query:
    """0. of the header: O, D, H [..., 3]; tmin, tmax, live [...]"""

    def at(self, index):
        q = Query()
        for k, v in self.__dict__.items():
            setattr(q, k, v[index])
        return q


def prepare(sweeps, dtype=np.float32):
    """sweeps: float32 [n, 11] (origin, direction, min_t, max_t, half) -> Query with leading shape [n]"""
    w = np.ascontiguousarray(sweeps, np.float32).reshape(-1, 11)
    q = Query()
    with np.errstate(all="ignore"):
        q.O, q.D, q.H = w[:, 0:3].astype(dtype), w[:, 3:6].astype(dtype), w[:, 8:11].astype(dtype)
        q.tmin, q.tmax = w[:, 6].astype(dtype), w[:, 7].astype(dtype)
        q.live = np.isfinite(w).all(1) & (w[:, 3:6] != 0).any(1) & (w[:, 8:11] >= 0).all(1) & (w[:, 6] <= w[:, 7])
    return q


def centre_np(q, t):
    with np.errstate(all="ignore"):
        return q.O + q.D * t[..., None]


def slab_np(q, lo, hi):
    """1.: the box [lo, hi] [..., 3] grown by H against the path -> (not empty, te, tx, axis)"""
    with np.errstate(all="ignore"):
        shape = np.broadcast(q.tmin, lo[..., 0]).shape
        t0, t1 = np.broadcast_to(q.tmin, shape), np.broadcast_to(q.tmax, shape)
        inside = np.ones(shape, bool)
        axis = np.full(shape, BS_START, np.int64)
        for k in range(3):
            l, h, d, o = lo[..., k] - q.H[..., k], hi[..., k] + q.H[..., k], q.D[..., k], q.O[..., k]
            zero = np.broadcast_to(d == 0, shape)
            tl, th = (l - o) / d, (h - o) / d
            tn, tf = np.where(d > 0, tl, th), np.where(d > 0, th, tl)
            win = ~zero & (tn > t0)
            t0 = np.where(win, tn, t0)
            axis = np.where(win, BS_BOX_X + k, axis)
            t1 = np.where(zero, t1, np.where(tf < t1, tf, t1))
            inside = inside & (~zero | ((l <= o) & (o <= h)))
    assert t0.dtype == q.tmin.dtype
    return inside & (t0 <= t1), t0, t1, axis


def tri_boxsweep_np(q, a, b, c, dtype=np.float32):
    """2.: q (made with the same dtype) broadcastable against a, b, c [..., 3] -> (axis [...] as the header's enum, t [...];
    t = max_t where the axis is none)"""
    a, b, c = (np.asarray(x, dtype) for x in (a, b, c))
    with np.errstate(all="ignore"):
        lo, hi = tri_box(a, b, c)
        ok, te, tx, axis = slab_np(q, lo, hi)
        shape = ok.shape
        Op = centre_np(q, te)
        w = [a - Op, b - Op, c - Op]
        ab, bc, ca, ac = b - a, c - b, a - c, c - a
        D, H = np.broadcast_to(q.D, w[0].shape), np.broadcast_to(q.H, w[0].shape)
        enter = np.zeros(shape, dtype)
        leave = tx - te
        some = np.ones(shape, bool)

        def one_axis(p, rb, s, code):
            nonlocal enter, leave, some, axis
            pmin, pmax = _min(_min(p[0], p[1]), p[2]), _max(_max(p[0], p[1]), p[2])
            still = s == 0
            some = some & ~(still & ((pmin > rb) | (pmax < -rb)))
            q0, q1 = (pmin - rb) / s, (pmax + rb) / s
            en, ex = np.where(s > 0, q0, q1), np.where(s > 0, q1, q0)
            win = ~still & (en > enter)
            enter = np.where(win, en, enter)
            axis = np.where(win, code, axis)
            leave = np.where(~still & (ex < leave), ex, leave)

        n = _cross(ab, ac)
        one_axis([_dot(n, wk) for wk in w], (np.abs(n[..., 0]) * H[..., 0] + np.abs(n[..., 1]) * H[..., 1]) + np.abs(n[..., 2]) * H[..., 2],
                 _dot(n, D), BS_NORMAL)
        for i, e in enumerate((ab, bc, ca)):
            for j in range(3):
                i1, i2 = (j + 1) % 3, (j + 2) % 3
                p = [e[..., i2] * wk[..., i1] - e[..., i1] * wk[..., i2] for wk in w]
                rb = np.abs(e[..., i2]) * H[..., i1] + np.abs(e[..., i1]) * H[..., i2]
                one_axis(p, rb, e[..., i2] * D[..., i1] - e[..., i1] * D[..., i2], BS_EDGE + 3 * i + j)
        time = te + enter
        time = np.where(te > time, te, time)
        has = ok & some & (enter <= leave) & ~(time > q.tmax)
        axis = np.where(has, axis, BS_NONE)
        t = np.where(has, time, np.broadcast_to(q.tmax, shape))
    assert t.dtype == dtype
    return axis, t


def normal_np(q, a, b, c, axis, dtype=np.float32):
    """the normal of 2.: q, a, b, c [n, ...], axis [n] -> [n, 3]"""
    a, b, c = (np.asarray(x, dtype) for x in (a, b, c))
    axis = np.asarray(axis, np.int64)
    with np.errstate(all="ignore"):
        zero = np.zeros(axis.shape, dtype)
        L = np.zeros(axis.shape + (3,), dtype)
        L = np.where((axis == BS_NORMAL)[:, None], _cross(b - a, c - a), L)
        for i, e in enumerate((b - a, c - b, a - c)):
            for j in range(3):
                i1, i2 = (j + 1) % 3, (j + 2) % 3
                comp = [zero, zero, zero]
                comp[i1], comp[i2] = e[..., i2], -e[..., i1]
                L = np.where((axis == BS_EDGE + 3 * i + j)[:, None], np.stack(comp, -1), L)
        length = np.sqrt(_dot(L, L))
        s = _dot(L, np.broadcast_to(q.D, L.shape))
        n = np.where((s > 0)[:, None], -L, L) / length[:, None]
        n = np.where(((length > 0) & (length <= np.finfo(np.float32).max))[:, None], n, dtype(0))
        for k in range(3):
            face = np.zeros(axis.shape + (3,), dtype)
            face[:, k] = np.where(q.D[..., k] > 0, dtype(-1), dtype(1))
            n = np.where((axis == BS_BOX_X + k)[:, None], face, n)
        n = np.where(((axis < BS_BOX_X) | (axis >= BS_AXES))[:, None], dtype(0), n)
    return n.astype(dtype)


def brute_force(tris, prims, sweeps, mesh_mask=None, ignore_prim=None, mesh_of=None):
    """The answer over ALL triangles: tris [T, 3, 3] float32 with ids prims [T], sweeps float32 [Q, 11]; mesh_mask: bools per mesh
    (meshes beyond it are not candidates) with mesh_of [T], the mesh index of each triangle; ignore_prim: one id per query ->
    (records as the four uint32 words t, u, v, prim [Q, 4], centres as words [Q, 3], normals as words [Q, 3])."""
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 3, 3)
    prims = np.asarray(prims, np.uint32)
    sweeps = np.ascontiguousarray(sweeps, np.float32).reshape(-1, 11)
    Q, T = len(sweeps), len(tris)
    rec = np.zeros((Q, 4), np.uint32)
    rec[:, 0] = sweeps[:, 7].view(np.uint32)
    rec[:, 3] = NONE
    ctr = sweeps[:, 0:3].copy().view(np.uint32)
    nrm = np.zeros((Q, 3), np.uint32)
    if T == 0 or Q == 0:
        return rec, ctr, nrm
    q = prepare(sweeps)
    axis, t = tri_boxsweep_np(q.at((slice(None), None)), tris[None, :, 0], tris[None, :, 1], tris[None, :, 2])
    cand = (axis != BS_NONE) & q.live[:, None]
    if mesh_mask is not None:
        mask = np.asarray(mesh_mask, bool)
        mesh_of = np.asarray(mesh_of, np.int64)
        cand &= ((mesh_of < len(mask)) & mask[np.minimum(mesh_of, len(mask) - 1)])[None, :]
    if ignore_prim is not None:
        cand &= prims[None, :] != np.asarray(ignore_prim, np.uint32)[:, None]
    best = np.where(cand, t, np.float32(np.inf)).min(1)
    tie = cand & (t == best[:, None])
    prim = np.where(tie, prims[None, :], np.uint32(NONE)).min(1)
    hit = np.nonzero(prim != NONE)[0]
    col = np.argsort(prims, kind="stable")[np.searchsorted(np.sort(prims), prim[hit])]
    th = t[hit, col]
    qh = q.at(hit)
    c = centre_np(qh, th)
    _, u, v, _, _ = tri_np(c, tris[col, 0], tris[col, 1], tris[col, 2])
    rec[hit, 0] = th.view(np.uint32)
    rec[hit, 1] = u.view(np.uint32)
    rec[hit, 2] = v.view(np.uint32)
    rec[hit, 3] = prim[hit]
    ctr[hit] = np.ascontiguousarray(c).view(np.uint32)
    nrm[hit] = np.ascontiguousarray(normal_np(qh, tris[col, 0], tris[col, 1], tris[col, 2], axis[hit, col])).view(np.uint32)
    return rec, ctr, nrm
