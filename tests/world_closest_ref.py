"""Closest points on an instanced world in numpy: the rule of rtk_amd/csrc/rtk_world_closest_rule.h in the stated order, float32
throughout -- the placed box, the placed triangle with tests/closest_ref.py's triangle routine on it, and the brute force over
(instance, primitive) with the tie rule and a filter -- and the queries of tests/test_gpu_world_closest.py."""
import numpy as np

from tests import closest_ref
from tests.world_ref import F, PRIM_NONE, RTK_INF, inverse_np, place_np

PAIRS = 1 << 21                              # (query, triangle) pairs evaluated at a time


def row_np(m, j, x, y, z):
    """rtk_place_row of row j: ((a x + b y) + c z) + d, every operation in float32"""
    with np.errstate(all="ignore"):
        return ((m[..., 4 * j] * x + m[..., 4 * j + 1] * y) + m[..., 4 * j + 2] * z) + m[..., 4 * j + 3]


def placed_box_np(m, lo, hi):
    """rtk_world_placed_box: m [..., 12], lo, hi [..., 3] -> (wlo, whi) [..., 3]: per world axis the row at the corner its signs
    choose, and at the opposite corner"""
    m, lo, hi = np.asarray(m, F), np.asarray(lo, F), np.asarray(hi, F)
    wlo, whi = [], []
    for j in range(3):
        neg = [m[..., 4 * j + a] < 0 for a in range(3)]
        up = [np.where(neg[a], lo[..., a], hi[..., a]) for a in range(3)]
        dn = [np.where(neg[a], hi[..., a], lo[..., a]) for a in range(3)]
        whi.append(row_np(m, j, *up))
        wlo.append(row_np(m, j, *dn))
    return np.stack(wlo, -1).astype(F), np.stack(whi, -1).astype(F)


def corners_box_np(m, lo, hi):
    """min / max over the eight corners placed by rtk_place_vertex, taken as rtk_world_box takes them (without its padding)"""
    m, lo, hi = np.asarray(m, F), np.asarray(lo, F), np.asarray(hi, F)
    wlo = whi = None
    for k in range(8):
        c = place_np(m, np.stack([hi[..., 0] if k & 1 else lo[..., 0], hi[..., 1] if k & 2 else lo[..., 1], hi[..., 2] if k & 4 else lo[..., 2]], -1))
        if k == 0:
            wlo, whi = c.copy(), c.copy()
        else:
            wlo, whi = np.where(c < wlo, c, wlo), np.where(c > whi, c, whi)
    return wlo, whi


def placed_tris(tris, m):
    """the records [T, 3, 3] of an instance under placement m [12], in float32 by the placement rule: what the flat twin's ingest holds"""
    return place_np(np.asarray(m, F), np.asarray(tris, F))


def live_instances(scene_tris, which, places):
    """bool [I]: the placement is invertible in float, the scene has triangles and its placed vertices are finite"""
    _, live = inverse_np(places)
    live = live.copy()
    for k in range(len(which)):
        t = scene_tris[which[k]]
        live[k] = live[k] and len(t) > 0 and bool(np.isfinite(placed_tris(t, places[k])).all())
    return live


def _instance_best(tris, points, max2):
    """closest_ref's brute force of one instance's placed triangles, in chunks: (record words [Q, 4], point words [Q, 3])"""
    rec = np.zeros((len(points), 4), np.uint32)
    pts = np.zeros((len(points), 3), np.uint32)
    step = max(1, PAIRS // max(1, len(tris)))
    prims = np.arange(len(tris), dtype=np.uint32)
    for c in range(0, len(points), step):
        rec[c:c + step], pts[c:c + step] = closest_ref.brute_force(tris, prims, points[c:c + step], max2[c:c + step])
    return rec, pts


def brute_force(scene_tris, which, places, points, max2, mask=None, ignore=None, live=None, prune=False):
    """The answer by the rule over every triangle of every live instance the filter lets through. scene_tris: list of [T, 3, 3]
    float32; which [I]; places [I, 12]; points [Q, 3]; max2 [Q]; mask: bool per instance (instances beyond it are out) or None;
    ignore: uint32 [Q] or None. -> (record words dist2 u v prim [Q, 4], instances uint32 [Q], point words [Q, 3]).
    prune: an instance is left out for a query when rtk_closest_box_bound of the box of its placed VERTICES (the theorem of
    rtk_closest_rule.h point 2, which tests/test_closest_cpu.py checks; not the placed box under test) is beyond the best dist2
    found so far -- the same answer, for the worlds whose plain brute force takes minutes."""
    points = np.ascontiguousarray(points, F)
    max2 = np.ascontiguousarray(max2, F)
    Q, I = len(points), len(which)
    live = live_instances(scene_tris, which, places) if live is None else live
    rec = np.zeros((Q, 4), np.uint32)
    rec[:, 0], rec[:, 3] = max2.view(np.uint32), PRIM_NONE
    inst = np.full(Q, PRIM_NONE, np.uint32)
    out_pts = points.view(np.uint32).copy()
    best2 = np.full(Q, np.inf, F)
    placed, bounds = {}, None
    allowed = np.zeros((Q, I), bool)
    for k in range(I):
        ok = bool(live[k]) and (mask is None or (k < len(mask) and bool(mask[k])))
        if ok:
            allowed[:, k] = True if ignore is None else (np.asarray(ignore, np.uint32) != k)
            placed[k] = placed_tris(scene_tris[which[k]], places[k])
    order = list(placed)
    if prune and order:
        bounds = np.full((Q, I), np.inf, F)
        for k in order:
            v = placed[k].reshape(-1, 3)
            bounds[:, k] = closest_ref.box_np(points, v.min(0), v.max(0))
        order.sort(key=lambda k: float(np.median(bounds[:, k])))
    for k in order:
        rows = allowed[:, k]
        if prune:
            with np.errstate(invalid="ignore"):
                rows = rows & ~(bounds[:, k] > best2)
        rows = np.flatnonzero(rows)
        if not rows.size:
            continue
        r, p = _instance_best(placed[k], points[rows], max2[rows])
        d2 = r[:, 0].view(F)
        hit = r[:, 3] != PRIM_NONE
        with np.errstate(invalid="ignore"):
            better = hit & ((d2 < best2[rows]) | ((d2 == best2[rows]) & (np.uint32(k) < inst[rows])))
        take = rows[better]
        rec[take], out_pts[take], inst[take], best2[take] = r[better], p[better], k, d2[better]
    return rec, inst, out_pts


# ---------------------------------------------------------------------------- the queries of the GPU test

def make_queries(scene_tris, which, places, rng, n_surface=2048, n_box=2048, n_miss=512, n_dead=64):
    """-> (points [n, 3], max2 [n]) float32: surface points of placed triangles pushed out along the normal by 1e-3 of the
    world's extent; uniform points in the world box grown by a half; queries with a max_dist small enough to miss (decided by
    the caller's brute force: a thousandth of the least distance of the same points); dead ones. In this order."""
    live = np.flatnonzero(live_instances(scene_tris, which, places))
    allv = np.concatenate([placed_tris(scene_tris[which[k]], places[k]).reshape(-1, 3) for k in live]).astype(np.float64)
    lo, hi = allv.min(0), allv.max(0)
    ext = float(np.linalg.norm(hi - lo))
    pts = np.zeros((n_surface, 3))
    for i in range(n_surface):
        k = live[rng.randint(len(live))]
        t = placed_tris(scene_tris[which[k]], places[k]).astype(np.float64)
        t = t[rng.randint(len(t))]
        w = rng.dirichlet((1, 1, 1))
        nrm = np.cross(t[1] - t[0], t[2] - t[0])
        pts[i] = w @ t + nrm / max(np.linalg.norm(nrm), 1e-300) * 1e-3 * ext
    box = rng.uniform(lo - 0.5 * (hi - lo), hi + 0.5 * (hi - lo), (n_box, 3))
    miss = rng.uniform(lo - 0.5 * (hi - lo), hi + 0.5 * (hi - lo), (n_miss, 3))
    dead = rng.uniform(lo, hi, (n_dead, 3)).astype(F)
    dead_max2 = np.full(n_dead, RTK_INF, F)
    half = n_dead // 2
    dead[np.arange(half), np.arange(half) % 3] = np.array([np.nan, np.inf, -np.inf], F)[(np.arange(half) // 3) % 3]
    dead_max2[half:] = np.array([np.nan, 0.0, -0.0, -1.0, -np.inf], F)[np.arange(n_dead - half) % 5]
    points = np.concatenate([pts, box, miss, dead]).astype(F)
    max2 = np.concatenate([np.full(n_surface + n_box, RTK_INF, F), np.zeros(n_miss, F), dead_max2])
    return points, max2
