"""The rule of rtk_amd/csrc/rtk_touch_rule.h restated in numpy float32, for tests/test_touch_cpu.py (against the header's driver)
and tests/test_gpu_touch.py (against the kernel): every product, sum and difference is one float32 operation in the header's
order. Per query the count of its candidates, its full list in ascending primitive id, and the prefix a segment of a given room
keeps. Also the query mix the GPU tests use, so that the CPU suite can check what it holds."""
import numpy as np

from tests.box_ref import skip_np  # noqa: F401  (rule 6 is the box rule's skip)

F = np.float32
SKIP_SHARED_VERTEX = 1


def live_np(a):
    """rule 1: a [..., 3, 3] float32 -> bool [...]"""
    with np.errstate(invalid="ignore"):
        return (a - a == 0).all((-1, -2))


def _min(x, y):
    return np.where(y < x, y, x)


def _max(x, y):
    return np.where(y > x, y, x)


def box_np(v):
    """componentwise min / max of the three vertices: v [..., 3, 3] -> lo, hi [..., 3]"""
    with np.errstate(invalid="ignore"):
        return _min(_min(v[..., 0, :], v[..., 1, :]), v[..., 2, :]), _max(_max(v[..., 0, :], v[..., 1, :]), v[..., 2, :])


def boxes_touch_np(a, b):
    """rule 2"""
    alo, ahi = box_np(a)
    tlo, thi = box_np(b)
    with np.errstate(invalid="ignore"):
        return ((tlo <= ahi) & (thi >= alo)).all(-1)


def cross_np(x, y):
    return np.stack([x[..., 1] * y[..., 2] - x[..., 2] * y[..., 1],
                     x[..., 2] * y[..., 0] - x[..., 0] * y[..., 2],
                     x[..., 0] * y[..., 1] - x[..., 1] * y[..., 0]], -1)


def dot_np(m, d):
    return (m[..., 0] * d[..., 0] + m[..., 1] * d[..., 1]) + m[..., 2] * d[..., 2]


def edges_np(v):
    return [v[..., 1, :] - v[..., 0, :], v[..., 2, :] - v[..., 1, :], v[..., 0, :] - v[..., 2, :]]


def axes_np(a, b):
    """rule 3: the seventeen axes in the rule's order, each [..., 3]"""
    ea, eb = edges_np(a), edges_np(b)
    na, nb = cross_np(ea[0], ea[1]), cross_np(eb[0], eb[1])
    return [na, nb] + [cross_np(ea[i], eb[j]) for i in range(3) for j in range(3)] + [cross_np(na, ea[i]) for i in range(3)] + [cross_np(nb, eb[j]) for j in range(3)]


def axis_separates_np(m, d1, d2, w):
    pa = [np.zeros((), F), dot_np(m, d1), dot_np(m, d2)]
    pb = [dot_np(m, wk) for wk in w]
    above = below = True
    for x in pb:
        for y in pa:
            above = above & (x > y)
            below = below & (x < y)
    return above | below


def separating_axes_np(a, b):
    """rule 3: a, b [..., 3, 3] float32 that broadcast -> uint32 [...], bit k set iff axis k separates"""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        a0 = a[..., 0, :]
        d1, d2 = a[..., 1, :] - a0, a[..., 2, :] - a0
        w = [b[..., k, :] - a0 for k in range(3)]
        bits = np.zeros(np.broadcast(a[..., 0, 0], b[..., 0, 0]).shape, np.uint32)
        for k, m in enumerate(axes_np(a, b)):
            bits = bits | (axis_separates_np(m, d1, d2, w).astype(np.uint32) << np.uint32(k))
        return bits


def shares_vertex_np(a, b):
    """rule 5: one of b's vertices equals one of a's on all three coordinates by float =="""
    with np.errstate(invalid="ignore"):
        shared = False
        for i in range(3):
            for j in range(3):
                shared = shared | (a[..., i, :] == b[..., j, :]).all(-1)
        return shared


def candidate_np(a, b, prim=0, first_prim=0, flags=0):
    """rule 4, arrays that broadcast against each other: a, b [..., 3, 3] float32 -> bool [...]"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    ok = live_np(a) & boxes_touch_np(a, b) & (separating_axes_np(a, b) == 0) & (np.asarray(prim) >= np.asarray(first_prim))
    if flags & SKIP_SHARED_VERTEX:
        ok = ok & ~shares_vertex_np(a, b)
    return ok


class Touching:
    """counts uint32 [Q]; lists[i] = uint32 [count_i], ascending ids; kept[i] = the same cut to room[i] entries"""

    def __init__(self, counts, lists, kept):
        self.counts, self.lists, self.kept = counts, lists, kept


def brute_force_touching(tris, prims, queries, first_prim=None, flags=0, room=None):
    """tris [T, 3, 3] float32 with ids prims [T], queries [Q, 3, 3] (or [Q, 9]), first_prim None or [Q] -> Touching"""
    tris = np.ascontiguousarray(tris, F).reshape(-1, 3, 3)
    prims = np.asarray(prims, np.uint32)
    queries = np.ascontiguousarray(queries, F).reshape(-1, 3, 3)
    Q, T = len(queries), len(tris)
    empty = np.zeros(0, np.uint32)
    if T == 0 or Q == 0:
        return Touching(np.zeros(Q, np.uint32), [empty] * Q, [empty] * Q)
    first = np.zeros(Q, np.uint32) if first_prim is None else np.asarray(first_prim, np.uint32)
    cand = candidate_np(queries[:, None], tris[None], prims[None, :], first[:, None], flags)
    counts = cand.sum(1).astype(np.uint32)
    lists, kept = [], []
    for i in range(Q):
        ids = np.sort(prims[np.nonzero(cand[i])[0]])
        lists.append(ids)
        kept.append(ids if room is None else ids[:int(room[i])])
    return Touching(counts, lists, kept)


# the parts of the query mix, in order: (name, number of queries)
MIX_PARTS = (("scene scale", 300), ("ten times the scene's scale", 200), ("the scene's own", 300), ("vertex on a vertex", 120),
             ("coplanar copies", 120), ("points", 80), ("segments", 80), ("huge and degenerate on purpose", 8), ("far away", 50),
             ("not live", 36))


def mix_slices():
    out, at = {}, 0
    for name, n in MIX_PARTS:
        out[name] = slice(at, at + n)
        at += n
    return out


def query_mix(tris, seed=31):
    """About 1300 query triangles [Q, 3, 3] float32 over a scene of few triangles, in the parts of MIX_PARTS: random triangles of
    the scene's scale and ten times it; the scene's own triangles; triangles with a vertex on a scene vertex and one float32 step
    off it; coplanar copies, shifted in their plane; points, segments; triangles that span the whole scene, and segments and
    points that do (a huge segment in the plane of nothing still meets every box, and its vanishing axes separate nothing);
    far away; NaN and +-inf members."""
    rng = np.random.RandomState(seed)
    tris = np.asarray(tris, F).reshape(-1, 3, 3)
    T = len(tris)
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    ext = hi - lo
    scale = float(np.abs(tris - tris.mean(1, keepdims=True)).max())          # the scene's triangles' own size
    parts = []
    # random triangles of the scene's scale, and ten times it
    for n, s in ((300, scale), (200, 10 * scale)):
        parts.append(rng.uniform(lo, hi, (n, 1, 3)) + rng.uniform(-s, s, (n, 3, 3)))
    # the scene's own triangles
    parts.append(tris[np.arange(300) % T])
    # a vertex on a scene vertex, and one float32 step either side of it on one axis: 40 x 3
    pick = tris[rng.permutation(T)[:40], rng.randint(0, 3, 40)]
    other = pick[:, None, :] + rng.uniform(-scale, scale, (40, 2, 3)).astype(F)
    for step in (-1, 0, 1):
        at = pick.copy()
        if step:
            at[:, 1] = np.nextafter(at[:, 1], F(step * np.inf))
        parts.append(np.concatenate([at[:, None, :], other], 1))
    # coplanar copies, shifted along an edge by part of its length: 40 x 3 shifts (0: the triangle itself)
    src = tris[rng.permutation(T)[:40]]
    for f in (0.0, 0.5, 3.0):
        parts.append(src + F(f) * (src[:, 1:2] - src[:, 0:1]))
    # points: at vertices, at centroids, anywhere
    verts = tris[rng.permutation(T)[:40], rng.randint(0, 3, 40)]
    cents = tris[rng.permutation(T)[:20]].astype(np.float64).mean(1)
    anywhere = rng.uniform(lo, hi, (20, 3))
    parts.append(np.repeat(np.concatenate([verts, cents, anywhere])[:, None, :], 3, 1))
    # segments: two equal vertices, and three collinear ones
    p, d = rng.uniform(lo, hi, (80, 3)), rng.uniform(-3 * scale, 3 * scale, (80, 3))
    seg = np.stack([p, p + d, p + d], 1)
    seg[40:, 2] = p[40:] + 0.5 * d[40:]
    parts.append(seg)
    # huge and degenerate on purpose: a triangle, two segments and a point cannot all meet everything, so all are tried and the
    # CPU suite asserts what the mix needs; a segment along the scene's diagonal, far longer than it, has nA = 0 and its edge
    # axes vanish with rounding, and a triangle of 1e30 swallows every difference
    mid = (lo + hi) * 0.5
    big = [np.stack([mid - 1e3 * ext, mid + 1e3 * ext, mid + 1e3 * ext]),
           np.stack([mid - 1e30, mid + 1e30, mid + 1e30]),
           np.stack([mid - 1e30, mid + 1e30, mid - 1e30 + 1e23]),
           np.stack([lo - 1e30 * np.array([1, 2, 3.0]), hi + 1e30 * np.array([3, 1, 2.0]), mid]),
           np.stack([lo - 3e38, hi + 3e38, mid]),
           np.stack([lo - ext, hi + ext, np.array([lo[0] - ext[0], hi[1] + ext[1], mid[2]])]),
           np.stack([mid - 3e38, mid + 3e38, mid + 3e38]),
           np.stack([lo, hi, hi])]
    parts.append(np.stack(big))
    # far away
    far = lo + ext * 1e3 * rng.choice([-1.0, 1.0], (50, 3))
    parts.append(far[:, None, :] + rng.uniform(-scale, scale, (50, 3, 3)))
    # NaN and +-inf members: one of the nine numbers of a triangle that otherwise spans the scene
    bad = np.tile(np.stack([lo - ext, hi + ext, mid])[None], (36, 1, 1)).astype(np.float64)
    for k in range(36):
        bad[k].reshape(-1)[k % 9] = [np.nan, np.inf, -np.inf, -np.nan][k // 9]
    parts.append(bad)
    with np.errstate(over="ignore"):
        out = np.concatenate(parts).astype(F)
    assert len(out) == sum(n for _, n in MIX_PARTS), len(out)
    return out
