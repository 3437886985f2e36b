"""The rule of rtk_amd/csrc/rtk_obbsweep_rule.h restated in numpy, for tests/test_obbsweep_cpu.py (against the header's driver)
and tests/test_gpu_obbsweep.py (against the kernel): every product, sum, difference, quotient and square root is one operation of
`dtype`, in the header's order. With dtype float32 it states the expected bits; with float64 it is the yardstick of the accuracy
statement. Everything is evaluated for every (query, triangle) pair and selected afterwards: no early exit changes a value.
The slab is tests/boxsweep_ref.py's own, as the header's is rtk_boxsweep_rule.h's own, with the world reach g as its H."""
import numpy as np

from tests.boxsweep_ref import _cross, _dot, _max, _min, slab_np
from tests.closest_ref import tri_box, tri_np
from tests.sweep_ref import better_np  # noqa: F401  (3. of the header is the sphere rule's)

NONE = 0xFFFFFFFF
OS_NONE, OS_START, OS_U0, OS_U1, OS_U2, OS_NORMAL, OS_EDGE = range(7)
OS_UNNAMED = 15
OS_CODES = 16
ORTHO_TOL = 2.0 ** -10
AXIS_NAMES = ("none", "start", "u0", "u1", "u2", "normal") + tuple("%s x u%s" % (e, j) for e in ("ab", "bc", "ca") for j in "012") + ("unnamed",)


class Query:
    """0. of the header: O, D (scene), H = g, Dp = D', half, U [..., 3, 3] (rows are the axes); tmin, tmax, live [...]"""

    def at(self, index):
        q = Query()
        for k, v in self.__dict__.items():
            setattr(q, k, v[index])
        return q


def prepare(sweeps, dtype=np.float32):
    """sweeps: float32 [n, 20] (origin, direction, min_t, max_t, half, axes) -> Query with leading shape [n]. Liveness is decided
    in float32, whatever the dtype: it is a property of the query."""
    w = np.ascontiguousarray(sweeps, np.float32).reshape(-1, 20)
    q = Query()
    with np.errstate(all="ignore"):
        q.O, q.D, q.half = w[:, 0:3].astype(dtype), w[:, 3:6].astype(dtype), w[:, 8:11].astype(dtype)
        q.tmin, q.tmax = w[:, 6].astype(dtype), w[:, 7].astype(dtype)
        q.U = w[:, 11:20].reshape(-1, 3, 3).astype(dtype)
        q.Dp = np.stack([_dot(q.U[:, j], q.D) for j in range(3)], -1)
        q.H = (np.abs(q.U[:, 0]) * q.half[:, 0:1] + np.abs(q.U[:, 1]) * q.half[:, 1:2]) + np.abs(q.U[:, 2]) * q.half[:, 2:3]
        u = w[:, 11:20].reshape(-1, 3, 3)
        tol = np.float32(ORTHO_TOL)
        ortho = np.ones(len(w), bool)
        for j in range(3):
            ortho &= np.abs(_dot(u[:, j], u[:, j]) - np.float32(1)) <= tol
        for i, j in ((0, 1), (0, 2), (1, 2)):
            ortho &= np.abs(_dot(u[:, i], u[:, j])) <= tol
        q.live = np.isfinite(w).all(1) & (w[:, 3:6] != 0).any(1) & (w[:, 8:11] >= 0).all(1) & (w[:, 6] <= w[:, 7]) & ortho
    assert q.Dp.dtype == dtype and q.H.dtype == dtype
    return q


def centre_np(q, t):
    with np.errstate(all="ignore"):
        return q.O + q.D * t[..., None]


def obb_slab_np(q, lo, hi):
    """1.: the box [lo, hi] [..., 3] grown by g against the path -> (not empty, te, tx)"""
    return slab_np(q, lo, hi)[:3]


def _frame(q, w):
    return np.stack([_dot(q.U[..., j, :], w) for j in range(3)], -1)


def _primed(q, a, b, c):
    """(ok, te, tx, [wa', wb', wc']) of 2. (i) and (ii)"""
    lo, hi = tri_box(a, b, c)
    ok, te, tx = obb_slab_np(q, lo, hi)
    Op = centre_np(q, te)
    return ok, te, tx, [_frame(q, a - Op), _frame(q, b - Op), _frame(q, c - Op)]


def tri_obbsweep_np(q, a, b, c, dtype=np.float32):
    """2.: q (made with the same dtype) broadcastable against a, b, c [..., 3] -> (axis [...] as the header's enum, t [...];
    t = max_t where the axis is none)"""
    a, b, c = (np.asarray(x, dtype) for x in (a, b, c))
    with np.errstate(all="ignore"):
        ok, te, tx, w = _primed(q, a, b, c)
        shape = ok.shape
        ab, bc, ca, ac = w[1] - w[0], w[2] - w[1], w[0] - w[2], w[2] - w[0]
        D, H = np.broadcast_to(q.Dp, w[0].shape), np.broadcast_to(q.half, w[0].shape)
        enter = np.full(shape, -np.inf, dtype)
        leave = tx - te
        some = np.ones(shape, bool)
        axis = np.full(shape, OS_UNNAMED, np.int64)

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

        for j in range(3):
            one_axis([wk[..., j] for wk in w], H[..., j], D[..., j], OS_U0 + j)
        n = _cross(ab, ac)
        one_axis([_dot(n, wk) for wk in w], (np.abs(n[..., 0]) * H[..., 0] + np.abs(n[..., 1]) * H[..., 1]) + np.abs(n[..., 2]) * H[..., 2],
                 _dot(n, D), OS_NORMAL)
        for i, e in enumerate((ab, bc, ca)):
            for j in range(3):
                i1, i2 = (j + 1) % 3, (j + 2) % 3
                p = [e[..., i2] * wk[..., i1] - e[..., i1] * wk[..., i2] for wk in w]
                rb = np.abs(e[..., i2]) * H[..., i1] + np.abs(e[..., i1]) * H[..., i2]
                one_axis(p, rb, e[..., i2] * D[..., i1] - e[..., i1] * D[..., i2], OS_EDGE + 3 * i + j)
        after = _max(enter, dtype(0))
        time = te + after
        time = np.where(te > time, te, time)
        has = ok & some & (after <= leave) & ~(time > q.tmax)
        axis = np.where((enter <= 0) & (te == q.tmin), OS_START, axis)
        axis = np.where(has, axis, OS_NONE)
        t = np.where(has, time, np.broadcast_to(q.tmax, shape))
    assert t.dtype == dtype
    return axis, t


def normal_np(q, a, b, c, axis, dtype=np.float32):
    """the normal of 2.: q, a, b, c [n, ...], axis [n] -> [n, 3]"""
    a, b, c = (np.asarray(x, dtype) for x in (a, b, c))
    axis = np.asarray(axis, np.int64)
    with np.errstate(all="ignore"):
        _, _, _, w = _primed(q, a, b, c)
        zero = np.zeros(axis.shape, dtype)
        L = np.zeros(axis.shape + (3,), dtype)
        L = np.where((axis == OS_NORMAL)[:, None], _cross(w[1] - w[0], w[2] - w[0]), L)
        for i, e in enumerate((w[1] - w[0], w[2] - w[1], w[0] - w[2])):
            for j in range(3):
                i1, i2 = (j + 1) % 3, (j + 2) % 3
                comp = [zero, zero, zero]
                comp[i1], comp[i2] = e[..., i2], -e[..., i1]
                L = np.where((axis == OS_EDGE + 3 * i + j)[:, None], np.stack(comp, -1), L)
        Dp = np.broadcast_to(q.Dp, L.shape)
        s = _dot(L, Dp)
        for j in range(3):
            L = np.where((axis == OS_U0 + j)[:, None], np.eye(3, dtype=dtype)[j], L)
            s = np.where(axis == OS_U0 + j, Dp[..., j], s)
        U = np.broadcast_to(q.U, axis.shape + (3, 3))
        m = (L[..., 0:1] * U[..., 0, :] + L[..., 1:2] * U[..., 1, :]) + L[..., 2:3] * U[..., 2, :]
        length = np.sqrt(_dot(m, m))
        n = np.where((s > 0)[:, None], -m, m) / length[:, None]
        n = np.where(((length > 0) & (length <= np.finfo(np.float32).max))[:, None], n, dtype(0))
        n = np.where(((axis < OS_U0) | (axis >= OS_UNNAMED))[:, None], dtype(0), n)
    return n.astype(dtype)


def brute_force(tris, prims, sweeps, mesh_mask=None, ignore_prim=None, mesh_of=None):
    """The answer over ALL triangles: tris [T, 3, 3] float32 with ids prims [T], sweeps float32 [Q, 20]; mesh_mask: bools per mesh
    (meshes beyond it are not candidates) with mesh_of [T], the mesh index of each triangle; ignore_prim: one id per query ->
    (records as the four uint32 words t, u, v, prim [Q, 4], centres as words [Q, 3], normals as words [Q, 3])."""
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 3, 3)
    prims = np.asarray(prims, np.uint32)
    sweeps = np.ascontiguousarray(sweeps, np.float32).reshape(-1, 20)
    Q, T = len(sweeps), len(tris)
    rec = np.zeros((Q, 4), np.uint32)
    rec[:, 0] = sweeps[:, 7].view(np.uint32)
    rec[:, 3] = NONE
    ctr = sweeps[:, 0:3].copy().view(np.uint32)
    nrm = np.zeros((Q, 3), np.uint32)
    if T == 0 or Q == 0:
        return rec, ctr, nrm
    q = prepare(sweeps)
    axis, t = tri_obbsweep_np(q.at((slice(None), None)), tris[None, :, 0], tris[None, :, 1], tris[None, :, 2])
    cand = (axis != OS_NONE) & q.live[:, None]
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
