"""The scenes that break a tree, cut down for brute force, and the queries that land on their ties: what
tests/test_gpu_queries_hostile_scenes.py runs every query family on. Everything here is numpy; the conditions on the scene set
and the non-vacuity figures are computed from the references alone (tests/test_hostile_scenes_cpu.py holds them on the CPU)."""
import functools

import numpy as np

from rtk_amd import synth
from rtk_amd.types import RTK_INF

F = np.float32
NONE = 0xFFFFFFFF
MIX_SEEDS = (15, 16, 10, 6)                  # _degenerate_mix seeds: 37 triangles; 300; 300, all on the x axis, 140 copies; 2500, 499 copies
STRIDES = {"tiny_cluster_plus_far_triangle": 40, "all_identical": 8, "line_along_x": 40, "huge_coordinates": 40, "two_distant_clusters": 40,
           "coplanar": 40, "flat_floor_grid": 40, "zero_area_row": 5, "geometric_chain": 3}
MAX_TRIANGLES = 2500
IDENTICAL = 600                              # copies of one record that all_identical keeps
BASE_QUERIES = 200                           # what a family's own mix is cut to; the three groups below add 96
GROUP = 32


@functools.lru_cache(maxsize=None)
def scenes():
    """name -> float32 [T, 3, 3], T <= 2500: four degenerate mixes and a strided subset of every adversarial scene"""
    from tests.test_gpu_build import _adversarial_scenes
    from tests.test_gpu_sizes import _degenerate_mix
    out = {}
    for seed in MIX_SEEDS:
        t = _degenerate_mix(seed).reshape(-1, 3, 3)
        assert len(t) in (37, 300, 2500), (seed, len(t))
        out["mix%d" % seed] = t
    for name, t in _adversarial_scenes().items():
        t = np.ascontiguousarray(t[::STRIDES[name]], F)
        out[name] = t[:IDENTICAL] if name == "all_identical" else t
    for t in out.values():
        t.setflags(write=False)
    return out


def copies(tris):
    """bool [T]: the record is in the scene more than once, bit for bit"""
    rows = np.ascontiguousarray(tris, F).reshape(len(tris), 9).view(np.uint32)
    _, inv, cnt = np.unique(rows, axis=0, return_inverse=True, return_counts=True)
    return cnt[inv.reshape(-1)] > 1


def extents(tris):
    return (tris.max(1) - tris.min(1)).max(1)


def zero_area(tris):
    t = tris.astype(np.float64)
    return np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1) == 0


def check_conditions(sc):
    """The conditions the issue puts on the scene set; returns which scenes hold each"""
    full = None
    held = {k: [] for k in "abcde"}
    for name, t in sc.items():
        assert t.dtype == F and t.shape[1:] == (3, 3) and 0 < len(t) <= MAX_TRIANGLES, (name, t.shape)
        e = extents(t)
        box = t.reshape(-1, 3).max(0) - t.reshape(-1, 3).min(0)
        if copies(t).sum() > 100:
            held["a"].append(name)
        if zero_area(t).any():
            held["b"].append(name)
        if (box == 0).sum() == 2:
            held["c"].append(name)
        if (e > 0).any() and e.max() / e[e > 0].min() > 1e6:
            held["d"].append(name)
        if np.abs(t).max() > 1e7:
            held["e"].append(name)
    for k, names in held.items():
        assert names, "no scene for condition (%s)" % k
    # the features a stride must keep
    from tests.test_gpu_build import _adversarial_scenes
    full = _adversarial_scenes()
    tiny = sc["tiny_cluster_plus_far_triangle"]
    assert tiny[0].tobytes() == full["tiny_cluster_plus_far_triangle"][0].tobytes() and tiny[0].min() >= 900 and np.abs(tiny[1:]).max() < 1
    two = sc["two_distant_clusters"]
    far = two[:, 0, 0] > 25
    assert 0.4 < far.mean() < 0.6 and not far[:len(two) // 2].any() and far[len(two) // 2:].all()
    assert copies(sc["all_identical"]).all() and len(sc["all_identical"]) == IDENTICAL
    assert (sc["coplanar"][:, :, 2] == F(0.5)).all() and (sc["flat_floor_grid"][:, :, 2] == F(0.25)).all()
    assert zero_area(sc["zero_area_row"]).all()
    return held


class Frame:
    """What the query groups need of a scene: its box, its copies, and the plane most of its flat triangles lie in"""

    def __init__(self, tris):
        self.tris = tris = np.asarray(tris, F)
        v = tris.reshape(-1, 3)
        self.lo, self.hi = v.min(0), v.max(0)
        self.ext = self.hi - self.lo
        self.size = float(self.ext.max())
        self.scale = float(np.abs(tris - tris.mean(1, keepdims=True)).max())
        dup = np.nonzero(copies(tris))[0]
        self.has_copies = len(dup) > 0
        self.tied = dup if self.has_copies else np.arange(len(tris))
        # the flat direction: the axis-aligned plane that holds the most triangles (a flat scene box: all of them); without
        # one, the low x face of the scene's box
        best = (0, 0, self.lo[0])
        for axis in range(3):
            flat = tris[(tris[:, :, axis] == tris[:, :1, axis]).all(1)][:, 0, axis]
            if len(flat):
                vals, cnt = np.unique(flat, return_counts=True)
                if cnt.max() > best[0]:
                    best = (int(cnt.max()), axis, vals[cnt.argmax()])
        self.in_plane, self.axis, self.plane = best
        self.other = [a for a in range(3) if a != self.axis]

    def far_points(self, n):
        """lo - 1e3 * ext and hi + 1e3 * ext, then the same on every proper subset of the axes"""
        out = []
        for k in range(n):
            m = np.array([1, 1, 1] if k < 2 else [(k // 2) >> a & 1 for a in range(3)], F)
            out.append(self.lo - F(1e3) * self.ext * m if k % 2 == 0 else self.hi + F(1e3) * self.ext * m)
        with np.errstate(over="ignore"):
            return np.array(out, F)

    def plane_points(self, rng, n):
        p = rng.uniform(self.lo - 0.05 * self.ext, self.hi + 0.05 * self.ext, (n, 3)).astype(F)
        p[:, self.axis] = self.plane
        return p

    def tied_vertices(self, rng, n):
        return self.tris[self.tied[rng.randint(0, len(self.tied), n)], rng.randint(0, 3, n)]


# (query, triangle) pairs a brute force may take, by what a pair costs in numpy: each case stays at a few seconds
PAIR_BUDGET = {"capsule": 300000, "pair": 400000, "near": 500000}


def base_queries(family, T):
    """how many rows of the family's own mix a scene of T triangles gets: 200, fewer where the reference is slow"""
    return int(min(BASE_QUERIES, max(GROUP, PAIR_BUDGET.get(family, 750000) // T - 3 * GROUP)))


def cut(mix, n=BASE_QUERIES):
    """every k-th row of a family's own mix: each of its parts in proportion"""
    return mix[::max(1, -(-len(mix) // n))]


def point_groups(tris, seed=1):
    """[96, 3]: on vertices of copied records, 1e3 extents away, in the flat direction's zero thickness"""
    f, rng = Frame(tris), np.random.RandomState(seed)
    return np.concatenate([f.tied_vertices(rng, GROUP), f.far_points(GROUP), f.plane_points(rng, GROUP)]).astype(F)


def triangle_groups(tris, seed=2):
    """[96, 3, 3]: scene records (copied ones where there are any), far away, inside the plane"""
    f, rng = Frame(tris), np.random.RandomState(seed)
    own = f.tris[f.tied[rng.randint(0, len(f.tied), GROUP)]]
    s = max(f.scale, 1e-3 * f.size)
    with np.errstate(over="ignore"):
        far = (f.far_points(GROUP)[:, None, :] + rng.uniform(-s, s, (GROUP, 3, 3))).astype(F)
    flat = (f.plane_points(rng, GROUP)[:, None, :] + rng.uniform(-s, s, (GROUP, 3, 3))).astype(F)
    flat[:, :, f.axis] = f.plane
    return np.concatenate([own, far, flat]).astype(F)


def box_groups(tris, seed=3):
    """(lo, hi) [96, 3] each: point boxes on vertices of copied records, scene-sized boxes 1e3 extents away, boxes of zero
    thickness in the plane"""
    f, rng = Frame(tris), np.random.RandomState(seed)
    v = f.tied_vertices(rng, GROUP)
    far = f.far_points(GROUP)
    c = f.plane_points(rng, GROUP)
    h = (rng.choice([0.02, 0.1, 0.5], (GROUP, 1)) * np.maximum(f.ext, 1e-3 * f.size)).astype(F)
    plo, phi = c - h, c + h
    plo[:, f.axis] = f.plane
    phi[:, f.axis] = f.plane
    with np.errstate(over="ignore"):
        return np.concatenate([v, far, plo]).astype(F), np.concatenate([v, far + f.ext, phi]).astype(F)


SWEEP_WIDTH = {"sphere": 9, "box": 11, "capsule": 12, "obb": 20}


def _shape(kind, rng, n, r):
    """the columns behind max_t of n sweeps whose shape has the size r[n] (0: a ray)"""
    s = np.zeros((n, SWEEP_WIDTH[kind] - 8), F)
    if kind == "sphere":
        s[:, 0] = r
    elif kind == "capsule":
        s[:, 0] = r
        s[:, 1:4] = rng.standard_normal((n, 3)) * r[:, None]
    else:
        s[:, 0:3] = rng.uniform(0.2, 1.0, (n, 3)) * r[:, None]
        if kind == "obb":
            from tests.test_gpu_obbsweep import quat_rows, rotations
            s[:, 3:12] = quat_rows(rotations(rng, n)).reshape(-1, 9)
    return s


def sweep_rows(kind, rng, o, d, r, min_t=0.0, max_t=RTK_INF):
    n = len(o)
    s = np.zeros((n, SWEEP_WIDTH[kind]), F)
    with np.errstate(over="ignore", invalid="ignore"):
        s[:, 0:3], s[:, 3:6] = o, d
    s[:, 6], s[:, 7] = min_t, max_t
    s[:, 8:] = _shape(kind, rng, n, np.asarray(r, np.float64))
    return s


def sweep_base(kind, tris, seed=4, n=BASE_QUERIES):
    """Where a family's own mix cannot be made of a scene (it asserts that it finds 80 hits through the box and 30 above a face:
    not so in a scene of points): paths from around the box to vertices, centroids and points of it, starts on the surface, and
    the family's rows that are not live"""
    f, rng = Frame(tris), np.random.RandomState(seed)
    ext = np.maximum(f.ext, 0.25 * f.size)
    k = max(n // 4, 12)
    pick = rng.randint(0, len(f.tris), 2 * k)
    target = np.concatenate([f.tris[pick[:k], rng.randint(0, 3, k)], f.tris[pick[k:]].astype(np.float64).mean(1), rng.uniform(f.lo, f.hi, (k, 3))])
    o = f.lo - ext + rng.uniform(0, 3, (3 * k, 3)) * ext
    r = rng.uniform(0, 1, 3 * k) ** 2 * 0.1 * f.size * (rng.uniform(0, 1, 3 * k) > 0.2)
    through = sweep_rows(kind, rng, o, target - o, r)
    start = f.tris[rng.randint(0, len(f.tris), k - 9), rng.randint(0, 3, k - 9)]
    on = sweep_rows(kind, rng, start, rng.standard_normal((k - 9, 3)) * f.size, rng.uniform(0, 0.05, k - 9) * f.size, min_t=rng.choice([0.0, -0.1], k - 9),
                    max_t=rng.choice([RTK_INF, 1.0], k - 9))
    bad = through[:9].copy()
    bad[np.arange(6), np.arange(6)] = np.array([np.nan, np.inf], F)[np.arange(6) // 3]
    bad[6, 3:6] = 0
    bad[7, 6], bad[7, 7] = 2.0, 1.0
    bad[8, 6] = np.nan
    return np.concatenate([through, on, bad]).astype(F)


def sweep_groups(kind, tris, seed=5):
    """[96, width]: paths that end on vertices of copied records (every copy at one t), starts 1e3 extents away aimed at the
    scene, paths that stay inside the plane"""
    f, rng = Frame(tris), np.random.RandomState(seed)
    ext = np.maximum(f.ext, 0.25 * f.size)
    v = f.tied_vertices(rng, GROUP)
    o = v + rng.choice([-1.0, 1.0], (GROUP, 3)) * ext * rng.uniform(0.5, 1.5, (GROUP, 3))
    small = rng.uniform(0, 0.02, GROUP) * f.size * (np.arange(GROUP) % 4 > 0)
    tied = sweep_rows(kind, rng, o, v - o, small)
    far = f.far_points(GROUP)
    aim = f.tris[rng.randint(0, len(f.tris), GROUP)].astype(np.float64).mean(1)
    away = sweep_rows(kind, rng, far, aim - far.astype(np.float64), small)
    a, b = f.plane_points(rng, GROUP), f.plane_points(rng, GROUP)
    a[:, f.other[0]] = (f.lo - 0.5 * ext)[f.other[0]]
    flat = sweep_rows(kind, rng, a, b - a, small * (np.arange(GROUP) % 2))
    flat[:, f.axis], flat[:, 3 + f.axis] = f.plane, 0
    return np.concatenate([tied, away, flat]).astype(F)


def sweep_live(kind, s):
    """rows that can hit at all: finite, a direction, a shape that is not negative, min_t <= max_t"""
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(np.delete(s, 7, 1)).all(1) & ~np.isnan(s[:, 7]) & (s[:, 3:6] != 0).any(1) & (s[:, 6] <= s[:, 7])
        shape = s[:, 8:9] if kind in ("sphere", "capsule") else s[:, 8:11]
        return ok & (shape >= 0).all(1)


def non_finite(tris):
    """the recipe of test_non_finite_vertices_do_not_break_the_build_or_the_traversal on a copy of tris [T, 3, 3]"""
    t = np.array(tris, F)
    k = np.arange(len(t))
    t[k % 97 == 0, 0, 0] = np.nan
    t[k % 101 == 1] = np.nan
    t[k % 103 == 2, 1, 2] = np.inf
    t[k % 107 == 3, 2, 1] = -np.inf
    return t


def non_finite_scenes():
    """name -> (hostile [T, 3, 3], its finite sibling)"""
    soup = synth.triangle_soup(1000, 0.05, seed=5).reshape(1000, 3, 3)
    mix = scenes()["mix16"]
    return {"soup1000": (non_finite(soup), soup), "mix16": (non_finite(mix), mix)}


def tied_winners(brute_force, tris, *args):
    """bool [Q] (callers pass the rows of the three groups: a lower bound of the batch's count is enough): two or more triangles at the winning dist2 or t. brute_force(tris, prims, *args)[0] is the record words with
    the primitive in column 3 (closest points, closest triangles, the sweeps): over the records in reverse order, ids still
    ascending, the lowest id at the winning value is another record exactly when the value has more than one."""
    T = len(tris)
    prims = np.arange(T, dtype=np.uint32)
    low = brute_force(tris, prims, *args)[0][:, 3]
    high = brute_force(np.ascontiguousarray(tris[::-1]), prims, *args)[0][:, 3]
    return (low != NONE) & (low != T - 1 - high.astype(np.int64))


def point_queries(tris, family):
    """closest: its own mix cut to 200 and the three groups without a limit. within: its own mix cut, and the groups with a
    radius of a tenth of the scene (vertices, plane) -- the far group keeps it and finds nothing, as it must."""
    from tests.test_gpu_closest import make_queries, query_mix
    g = point_groups(tris)
    if family == "closest":
        base = cut(query_mix(tris), base_queries(family, len(tris)))
        max2 = np.full(len(g), RTK_INF, F)
    else:
        from tests.test_gpu_within import within_mix
        base = cut(within_mix(tris), base_queries(family, len(tris)))
        size = Frame(tris).size
        max2 = np.full(len(g), F(0.1 * size) * F(0.1 * size), F)
    return np.concatenate([base, make_queries(g, max2)])


def box_queries(tris):
    from tests.test_gpu_box import box_mix, make_boxes
    return np.concatenate([cut(box_mix(tris)), make_boxes(*box_groups(tris))])


def triangle_queries(tris, family):
    """touch: its own mix cut to 200 and the three groups. pair, near: the same without the part that is huge on purpose, as
    their own files leave it out, and one squared limit per query drawn as they draw it, at the scene's size"""
    from tests.touch_ref import mix_slices, query_mix
    mix = query_mix(tris)
    if family == "touch":
        return np.concatenate([cut(mix), triangle_groups(tris)]), None
    from tests.test_gpu_pair import limits
    huge = mix_slices()["huge and degenerate on purpose"]
    q = np.concatenate([cut(np.concatenate([mix[:huge.start], mix[huge.stop:]]), base_queries(family, len(tris))), triangle_groups(tris)])
    return q, limits(np.random.RandomState(3), len(q), Frame(tris).size)


def sweep_queries(kind, tris):
    """-> (sweeps, whether the family's own mix could be made of this scene)"""
    import importlib
    mod = importlib.import_module({"sphere": "tests.test_gpu_sweep", "box": "tests.test_gpu_boxsweep", "capsule": "tests.test_gpu_capsule",
                                   "obb": "tests.test_gpu_obbsweep"}[kind])
    try:
        with np.errstate(all="ignore"):
            mix = mod.sweep_mix(tris)
        base, own = cut(mix[0] if isinstance(mix, tuple) else mix, base_queries(kind, len(tris))), True
    except (AssertionError, ValueError, IndexError):
        base, own = sweep_base(kind, tris, n=base_queries(kind, len(tris))), False
    return np.concatenate([base, sweep_groups(kind, tris)]).astype(F), own


def adversarial_rays(tris, n=1024):
    """The rays test_adversarial_distributions makes: from a cube around the scene, half of them aimed at centroids"""
    from rtk_amd.types import RAY_DTYPE
    t3 = np.asarray(tris, F).reshape(-1, 3, 3)
    lo, hi = t3.min(axis=(0, 1)).astype(np.float64), t3.max(axis=(0, 1)).astype(np.float64)
    ext = np.maximum(hi - lo, 0.25 * (hi - lo).max())
    u = synth.u01(9, 0, n * 6).reshape(n, 6).astype(np.float64)
    rays = np.zeros(n, RAY_DTYPE)
    org = lo - 0.5 * ext + 2.0 * ext * u[:, 0:3]
    tgt = lo + ext * u[:, 3:6]
    cent = t3.mean(axis=1).astype(np.float64)
    tgt[::2] = cent[(np.arange(n // 2) * 7919) % len(cent)]
    rays["origin"] = org.astype(F)
    rays["direction"] = (tgt - org).astype(F)
    rays["max_t"] = F(4.0)
    return rays
