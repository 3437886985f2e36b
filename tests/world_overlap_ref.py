"""The three overlap queries on an instanced world in numpy: the rule of rtk_amd/csrc/rtk_world_overlap_rule.h, float32
throughout. A record is placed by the placement rule (tests/world_ref.py), the shape's own candidate rule answers on the placed
vertices (tests/box_ref.py, tests/obb_ref.py, tests/touch_ref.py, unchanged), an entry is instance << 32 | prim and a list is
ascending; the brute force runs over (instance, record) with the world's filter. And the queries of
tests/test_gpu_world_overlap.py."""
import numpy as np

from tests import box_ref, obb_ref, touch_ref
from tests.world_closest_ref import live_instances, placed_tris
from tests.world_ref import F

SHAPES = ("box", "obb", "touch")
FLOATS = {"box": 6, "obb": 15, "touch": 9}
SKIP_SHARED_VERTEX = touch_ref.SKIP_SHARED_VERTEX
PAIRS = 1 << 20                              # (query, triangle) pairs evaluated at a time


def bounds_np(shape, q):
    """(qlo, qhi, live) of queries q [Q, FLOATS[shape]]: the axis-aligned bounds every skip compares against, and the shape's liveness"""
    q = np.ascontiguousarray(q, F).reshape(-1, FLOATS[shape])
    if shape == "box":
        return q[:, :3], q[:, 3:], box_ref.live_np(q[:, :3], q[:, 3:])
    if shape == "obb":
        _, qlo, qhi = obb_ref.reach_np(q)
        return qlo, qhi, obb_ref.live_np(q)
    a = q.reshape(-1, 3, 3)
    lo, hi = touch_ref.box_np(a)
    return lo, hi, touch_ref.live_np(a)


def candidate_np(shape, q, v, flags=0):
    """the shape's candidate rule for pairs: q [P, FLOATS], placed records v [P, 3, 3] -> bool [P]"""
    if shape == "box":
        return box_ref.candidate_np(v[:, 0], v[:, 1], v[:, 2], q[:, :3], q[:, 3:])
    if shape == "obb":
        return obb_ref.candidate_np(q, v[:, 0], v[:, 1], v[:, 2])
    return touch_ref.candidate_np(q.reshape(-1, 3, 3), v, flags=flags)


def keys_of(inst, prim):
    return (np.asarray(inst, np.uint64) << np.uint64(32)) | np.asarray(prim, np.uint64)


def decode(keys):
    keys = np.asarray(keys, np.uint64)
    return (keys >> np.uint64(32)).astype(np.uint32), (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)


class Answer:
    """counts uint32 [Q]; lists[i] = uint64 [count_i], ascending keys; instances[i] = how many instances query i has candidates in"""

    def __init__(self, counts, lists):
        self.counts, self.lists = counts, lists
        self.instances = np.array([len(np.unique(l >> np.uint64(32))) for l in lists], np.int64)

    def kept(self, room):
        return [l[:int(r)] for l, r in zip(self.lists, room)]

    def flat(self):
        return np.concatenate(self.lists + [np.zeros(0, np.uint64)])


def brute_force(shape, scene_tris, which, places, q, mask=None, ignore=None, flags=0, prune=False, live=None):
    """The answer by the rule over every record of every live instance the filter lets through. scene_tris: list of [T, 3, 3]
    float32; which [I]; places [I, 12]; q [Q, FLOATS[shape]]; mask: bool per instance (instances beyond it are out) or None;
    ignore: uint32 [Q] or None. prune: a pair is only evaluated where the placed record's own box touches the query's bounds --
    comparisons only, and a step of every shape's candidate rule, so the same answer -- for the worlds whose plain brute force
    takes minutes."""
    q = np.ascontiguousarray(q, F).reshape(-1, FLOATS[shape])
    Q = len(q)
    live = live_instances(scene_tris, which, places) if live is None else live
    qlo, qhi, qlive = bounds_np(shape, q)
    got_q, got_key = [np.zeros(0, np.int64)], [np.zeros(0, np.uint64)]
    for k in range(len(which)):
        if not live[k] or (mask is not None and not (k < len(mask) and bool(mask[k]))):
            continue
        rows = np.ones(Q, bool) if ignore is None else (np.asarray(ignore, np.uint32) != k)
        placed = placed_tris(scene_tris[which[k]], places[k])
        T = len(placed)
        if prune:
            vlo, vhi = placed.reshape(-1, 3).min(0), placed.reshape(-1, 3).max(0)
            with np.errstate(invalid="ignore"):
                rows = rows & qlive & ((vlo <= qhi) & (vhi >= qlo)).all(1)
        rows = np.flatnonzero(rows)
        step = max(1, PAIRS // max(1, T))
        for c in range(0, len(rows), step):
            r = rows[c:c + step]
            if prune:
                tlo, thi = placed.min(1), placed.max(1)
                with np.errstate(invalid="ignore"):
                    touch = ((tlo[None] <= qhi[r][:, None]) & (thi[None] >= qlo[r][:, None])).all(2)
                qi, ti = np.nonzero(touch)
            else:
                qi, ti = np.divmod(np.arange(len(r) * T), T)
            if not len(qi):
                continue
            ok = candidate_np(shape, q[r[qi]], placed[ti], flags)
            got_q.append(r[qi[ok]])
            got_key.append(keys_of(np.full(int(ok.sum()), k), ti[ok]))
    gq, gk = np.concatenate(got_q), np.concatenate(got_key)
    order = np.lexsort((gk, gq))
    gq, gk = gq[order], gk[order]
    counts = np.bincount(gq, minlength=Q).astype(np.uint32)
    lists = np.split(gk, np.cumsum(counts)[:-1]) if Q else []
    return Answer(counts, lists)


# ---------------------------------------------------------------------------- the queries of the tests

def random_rotations(n, rng):
    """[n, 3, 3] float32 whose rows are orthonormal to float accuracy (QR of a normal matrix, in float64)"""
    out = np.zeros((n, 3, 3))
    for i in range(n):
        out[i] = np.linalg.qr(rng.standard_normal((3, 3)))[0]
    return out


def make_queries(shape, scene_tris, which, places, rng, n_live, n_other, size):
    """-> q [n_live + n_other, FLOATS[shape]] float32. The live ones are built around a random record of a random live instance
    (instances drawn evenly, not by their triangle count), `size` setting their extent: a box and an oriented box that contain
    one of its placed vertices in their inside, a triangle that the record's centroid lies on and whose plane crosses the
    record's. Of the others half are not live (NaN, an infinity, lo > hi / a negative half, axes that are not orthonormal) and
    half lie ten extents outside the world."""
    live = np.flatnonzero(live_instances(scene_tris, which, places))
    placed = {k: placed_tris(scene_tris[which[k]], places[k]).astype(np.float64) for k in live}
    allv = np.concatenate([p.reshape(-1, 3) for p in placed.values()])
    wlo, whi = allv.min(0), allv.max(0)
    n = n_live + n_other
    q = np.zeros((n, FLOATS[shape]))
    rot = random_rotations(n, rng)
    for i in range(n):
        t = placed[live[rng.randint(len(live))]]
        t = t[rng.randint(len(t))]
        s = size * rng.uniform(0.5, 1.5)
        if i >= n_live + n_other // 2:
            t = t + (whi - wlo) * 10.0 + 100.0 * size                      # far outside: touches nothing
        if shape == "box":
            v = t[rng.randint(3)]
            q[i] = np.concatenate([v - s * rng.uniform(0.2, 1.0, 3), v + s * rng.uniform(0.2, 1.0, 3)])
        elif shape == "obb":
            v = t[rng.randint(3)]
            h = s * rng.uniform(0.3, 1.0, 3)
            centre = v + rot[i].T @ (h * rng.uniform(-0.5, 0.5, 3))          # the vertex is inside, at most half way out
            q[i] = np.concatenate([centre, h, rot[i].reshape(-1)])
        else:
            c = t.mean(0)
            nrm = np.cross(t[1] - t[0], t[2] - t[0])
            nrm = nrm / max(np.linalg.norm(nrm), 1e-300) if np.linalg.norm(nrm) > 0 else rot[i][0]
            tan = t[1] - t[0]
            tan = tan / max(np.linalg.norm(tan), 1e-300) if np.linalg.norm(tan) > 0 else rot[i][1]
            q[i] = np.concatenate([c + s * nrm + s * tan, c + s * nrm - s * tan, c - s * nrm])
    q = q.astype(F)
    dead = np.arange(n_live, n_live + n_other // 2)
    for j, i in enumerate(dead):
        kind = j % 4
        if kind == 0:
            q[i, j % FLOATS[shape]] = np.nan
        elif kind == 1:
            q[i, j % 3] = np.inf if j % 8 == 1 else -np.inf
        elif shape == "box":
            q[i, :3], q[i, 3:] = q[i, 3:].copy() + F(1.0), q[i, :3].copy()     # lo > hi
        elif shape == "obb":
            if kind == 2:
                q[i, 3 + j % 3] = -abs(q[i, 3 + j % 3]) - F(1e-3)               # a negative half
            else:
                q[i, 6:9] *= F(1.01)                                            # an axis that is not a unit vector
        else:
            q[i, 3 * (j % 3) + (j // 4) % 3] = np.nan
    return q


def shared_vertex_queries(scene_tris, which, places, rng, n):
    """-> q [n, 9] float32: query triangles whose vertex 0 HAS THE BITS of a placed vertex of a record of a random live instance,
    and which reach 1.7 times that record's two edges from it, pushed 0.1 off: they meet the records around that vertex,
    all of which share its position as the placement rule places it. What RTK_TOUCH_SKIP_SHARED_VERTEX is about."""
    live = np.flatnonzero(live_instances(scene_tris, which, places))
    q = np.zeros((n, 9), F)
    for i in range(n):
        k = live[rng.randint(len(live))]
        t = placed_tris(scene_tris[which[k]], places[k])
        t = t[rng.randint(len(t))]
        j = rng.randint(3)
        a, b, c = t[j], t[(j + 1) % 3], t[(j + 2) % 3]
        q[i] = np.concatenate([a, a + (b - a) * F(1.7) + F(0.1), a + (c - a) * F(1.7) - F(0.1)])
    return q
