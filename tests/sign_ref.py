"""The rule of rtk_amd/csrc/rtk_sign_rule.h restated in numpy, for tests/test_sign_cpu.py (against the header's driver) and
tests/test_gpu_sign.py (against the kernels): the table of pseudonormals and the sign in float32, operation by operation in the
header's order; a float64 brute-force distance; an analytic inside test for unions of axis-aligned boxes; and the meshes and
queries both tests use. Nothing here reads the library."""
import math

import numpy as np

from tests.closest_ref import NONE, _dot, brute_force, tri_np

F = np.float32
PIO2, PI = F(1.57079637), F(3.14159274)
COEF = [F(0.999977231), F(-0.332622826), F(0.193540394), F(-0.116426520), F(0.0526473969), F(-0.0117191551)]
RTK_INF = F(3.402823e+38)


def _cross(x, y):
    return np.stack([x[..., 1] * y[..., 2] - x[..., 2] * y[..., 1], x[..., 2] * y[..., 0] - x[..., 0] * y[..., 2],
                     x[..., 0] * y[..., 1] - x[..., 1] * y[..., 0]], -1)


def angle_np(y, x):
    """rtk_sign_angle in float32, case by case as the header states them"""
    y, x = np.broadcast_arrays(np.asarray(y, F), np.asarray(x, F))
    with np.errstate(all="ignore"):
        ay, ax = np.where(y < 0, F(0) - y, y), np.where(x < 0, F(0) - x, x)
        swap = ay > ax
        mx, mn = np.where(swap, ay, ax), np.where(swap, ax, ay)
        t = mn / mx
        s = t * t
        r = np.full(t.shape, COEF[5], F)
        for c in COEF[4::-1]:
            r = r * s + c
        r = r * t
        r = np.where(swap, PIO2 - r, r)
        r = np.where(x < 0, PI - r, r)
        r = np.where(y < 0, F(0) - r, r)
        r = np.where(mx == 0, F(0), r)
    assert r.dtype == F
    return r


def normals_np(tris):
    """tris [T, 3, 3] float32 -> raw cross n [T, 3], unit [T, 3], has [T], terms [T, 3 corners, 3]"""
    t = np.ascontiguousarray(tris, F)
    a, b, c = t[:, 0], t[:, 1], t[:, 2]
    with np.errstate(all="ignore"):
        n = _cross(b - a, c - a)
        ln = np.sqrt(_dot(n, n))
        unit = n / ln[:, None]
        has = (ln > 0) & (ln < np.inf)
        w = []
        for x, y, z in ((a, b, c), (b, c, a), (c, a, b)):
            e1, e2 = y - x, z - x
            k = _cross(e1, e2)
            w.append(angle_np(np.sqrt(_dot(k, k)), _dot(e1, e2)))
        terms = np.stack(w, 1)[:, :, None] * unit[:, None, :]
    assert n.dtype == F and unit.dtype == F and terms.dtype == F
    return n, unit, has, terms


def _place_ids(tris):
    """corner (prim, k) -> a place number; equal as numbers = same place, -0 = +0, a NaN corner is alone"""
    ids, seen = np.zeros((len(tris), 3), np.int64), {}
    for p in range(len(tris)):
        for k in range(3):
            v = tris[p, k]
            key = ("nan", p, k) if np.isnan(v).any() else tuple(float(x) + 0.0 for x in v)      # (-0.0 + 0.0 = +0.0)
            ids[p, k] = seen.setdefault(key, len(seen))
    return ids, len(seen)


def _sum_in_order(rows):
    if not rows:
        return np.zeros(3, F)
    s = rows[0].copy()
    for r in rows[1:]:
        s = s + r
    return s


def table_np(tris):
    """tris [T, 3, 3] float32 (prim = row) -> (table [T, 18] float32, the counts of rtk_dev_sign_info)"""
    tris = np.ascontiguousarray(tris, F)
    T = len(tris)
    _, unit, has, terms = normals_np(tris)
    ids, places = _place_ids(tris)
    corners = {}                                                             # place -> its corners in ascending (prim, k)
    for p in range(T):
        for k in range(3):
            corners.setdefault(int(ids[p, k]), []).append((p, k))
    table = np.zeros((T, 18), F)
    with np.errstate(all="ignore"):
        vsum = {pl: _sum_in_order([terms[p, k] for p, k in cs if has[p]]) for pl, cs in corners.items()}
        info = dict(boundary_sides=0, nonmanifold_sides=0, inconsistent_sides=0, degenerate_triangles=int((~has).sum()), places=places)
        for p in range(T):
            for k in range(3):
                table[p, 9 + 3 * k:12 + 3 * k] = vsum[int(ids[p, k])]
            for e, (i, j) in enumerate(((0, 1), (0, 2), (1, 2))):
                P, Q = int(ids[p, i]), int(ids[p, j])
                if P == Q:
                    table[p, 3 * e:3 * e + 3] = vsum[P]
                    continue
                rows, others, other_fwd, last = [], 0, False, -1
                for t, kp in corners[P]:
                    if t == last:
                        continue
                    last = t
                    kq = [k for k in range(3) if ids[t, k] == Q]
                    if not kq:
                        continue
                    if has[t]:
                        rows.append(unit[t])
                    if t != p:
                        others += 1
                        other_fwd = kq[0] == (kp + 1) % 3
                table[p, 3 * e:3 * e + 3] = _sum_in_order(rows)
                if others == 0:
                    info["boundary_sides"] += 1
                elif others >= 2:
                    info["nonmanifold_sides"] += 1
                elif other_fwd == (j == (i + 1) % 3):
                    info["inconsistent_sides"] += 1
    return table, info


REGION_AT = {1: 9, 2: 12, 3: 0, 4: 15, 5: 3, 6: 6}


def signed_np(tris, table, points, max2):
    """The answer of the closest rule over all records (prim = row), then the sign: (signed [Q] float32, records [Q, 4] uint32
    words, points [Q, 3] uint32 words, region [Q] (0 for a miss), shortcut [Q] bool: what the face normal alone would say)."""
    tris = np.ascontiguousarray(tris, F)
    points = np.ascontiguousarray(points, F)
    rec, pts = brute_force(tris, np.arange(len(tris), dtype=np.uint32), points, max2)
    Q = len(points)
    out, region, shortcut = np.full(Q, RTK_INF, F), np.zeros(Q, np.int64), np.zeros(Q, bool)
    hit = np.nonzero(rec[:, 3] != NONE)[0]
    if len(hit) == 0:
        return out, rec, pts, region, shortcut
    t = tris[rec[hit, 3]]
    p = points[hit]
    with np.errstate(all="ignore"):
        dist2, _, _, q, reg = tri_np(p, t[:, 0], t[:, 1], t[:, 2])
        n = _cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
        at = np.array([REGION_AT.get(int(r), 0) for r in reg])
        N = np.stack([table[rec[hit, 3], at + i] for i in range(3)], 1)
        N = np.where((reg == 7)[:, None], n, N)
        d = p - q
        s = _dot(d, N)
        r = np.sqrt(dist2)
        out[hit] = np.where(s < 0, F(0) - r, r)
        shortcut[hit] = _dot(d, n) < 0
    region[hit] = reg
    return out, rec, pts, region, shortcut


def distance64(tris, points):
    """float64 brute-force distance of each point from the mesh"""
    t = np.asarray(tris, np.float64)
    p = np.asarray(points, np.float64)
    with np.errstate(all="ignore"):
        d2 = tri_np(p[:, None, :], t[None, :, 0], t[None, :, 1], t[None, :, 2], dtype=np.float64)[0]
    return np.sqrt(np.nanmin(d2, 1))


# ---------------------------------------------------------------------------------------------- meshes

class Boxes:
    """A union of axis-aligned boxes given as filled cells of a grid with the planes xs, ys, zs: its surface is every cell face
    between a filled and an empty cell, two triangles each, wound outwards; all vertices are grid points, so there is no
    T-junction. inside(): the analytic test. tilt: a rotation (axis, angle) the whole shape is turned by; the grid and the
    analytic test stay in the shape's own frame (float64), the triangles are the turned grid points rounded to float32. With
    exact axis-aligned coordinates the face normal alone is never wrong (every doubtful dot product is exactly 0); turned,
    those products are +- a rounding error, which is what the pseudonormal is there for."""

    def __init__(self, xs, ys, zs, cells, tilt=None):
        self.R = np.eye(3)
        if tilt is not None:
            k = np.asarray(tilt[0], np.float64) / np.linalg.norm(tilt[0])
            K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
            self.R = np.eye(3) + math.sin(tilt[1]) * K + (1 - math.cos(tilt[1])) * K @ K
        self.g = [np.asarray(v, np.float64) for v in (xs, ys, zs)]
        self.occ = np.zeros([len(v) + 1 for v in self.g], bool)              # (a border of empty cells)
        for c in cells:
            self.occ[c[0] + 1, c[1] + 1, c[2] + 1] = True
        self.size = max(float(v[-1] - v[0]) for v in self.g)

    def local(self, v, snap=True):
        """world -> the shape's frame; snap: to the grid planes (for a vertex of the mesh)"""
        x = np.asarray(v, np.float64) @ self.R
        if snap:
            x = np.array([self.g[a][np.argmin(np.abs(self.g[a] - x[a]))] for a in range(3)])
        return x

    def inside(self, points):
        p = np.asarray(points, np.float64) @ self.R
        idx = [np.searchsorted(self.g[a], p[:, a], side="right") for a in range(3)]
        return self.occ[idx[0], idx[1], idx[2]]

    def triangles(self):
        out = []
        for i, j, k in np.argwhere(self.occ):
            lo = [self.g[0][i - 1], self.g[1][j - 1], self.g[2][k - 1]]
            hi = [self.g[0][i], self.g[1][j], self.g[2][k]]
            for axis in range(3):
                for side in (0, 1):
                    nb = [i, j, k]
                    nb[axis] += 1 if side else -1
                    if self.occ[tuple(nb)]:
                        continue
                    u, v = (axis + 1) % 3, (axis + 2) % 3
                    def pt(a, b):
                        x = [0.0, 0.0, 0.0]
                        x[axis] = hi[axis] if side else lo[axis]
                        x[u], x[v] = (hi[u] if a else lo[u]), (hi[v] if b else lo[v])
                        return x
                    quad = [pt(0, 0), pt(1, 0), pt(1, 1), pt(0, 1)]          # counter-clockwise seen from +axis
                    if not side:
                        quad = quad[::-1]
                    out += [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
        return (np.array(out, np.float64) @ self.R.T).astype(F)

    def kind_of_place(self, v):
        """'convex', 'saddle' (a corner that is not convex), 'convex edge', 'concave edge' or 'flat' for a vertex of the mesh"""
        v = self.local(v)
        idx = [int(np.searchsorted(self.g[a], v[a])) for a in range(3)]
        cube = self.occ[idx[0]:idx[0] + 2, idx[1]:idx[1] + 2, idx[2]:idx[2] + 2]
        for axis in range(3):
            a, b = np.take(cube, 0, axis), np.take(cube, 1, axis)
            if (a == b).all():                                               # the same on both sides of the point along this axis
                if any((np.take(a, 0, ax2) == np.take(a, 1, ax2)).all() for ax2 in range(2)):
                    return "flat"
                return "convex edge" if a.sum() == 1 else "concave edge"
        return "convex" if cube.sum() == 1 else "saddle"

    def kind_of_edge(self, v, w):
        """the kind of the segment between two grid points that the mesh has as an edge"""
        v, w = self.local(v), self.local(w)
        if (v != w).sum() != 1:
            return "flat"                                                    # (a quad's diagonal)
        axis = int(np.nonzero(v != w)[0][0])
        mid = (v + w) / 2
        idx = [int(np.searchsorted(self.g[a], mid[a])) for a in range(3)]
        sl = [slice(i, i + 2) for i in idx]
        sl[axis] = slice(idx[axis], idx[axis] + 1)
        four = self.occ[tuple(sl)].reshape(2, 2)
        n = int(four.sum())
        return "convex edge" if n == 1 else "concave edge" if n == 3 else "flat"


TILT = ((1.0, 2.0, 3.0), 0.7)


def l_prism(tilt=None):
    return Boxes([0.0, 1.0, 2.5], [0.0, 0.75, 2.0], [0.0, 1.25], [(0, 0, 0), (1, 0, 0), (0, 1, 0)], tilt)


def plus_shape(tilt=None):
    """a plus sign with thickness: the union of three boxes, a bar and the two stubs above and below its middle. (The plus of
    three bars along the three axes would not do: the region of space nearest to one of its inner corners is empty.)"""
    return Boxes([0.0, 1.0, 2.25, 3.0], [0.0, 0.75, 2.0, 3.25], [0.0, 1.5], [(0, 1, 0), (1, 1, 0), (2, 1, 0), (1, 0, 0), (1, 2, 0)], tilt)


def cube():
    return Boxes([-1.0, 1.0], [-1.0, 1.0], [-1.0, 1.0], [(0, 0, 0)]).triangles()


def tetrahedron():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F)
    return v[np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])]


def fan(n=200):
    """n triangles round one apex above a regular polygon: open below, the apex a vertex of valence n"""
    ang = (np.arange(n + 1) % n) * (2 * np.pi / n)
    rim = np.stack([np.cos(ang), np.sin(ang), np.zeros(n + 1)], 1).astype(F)
    apex = np.array([0.0, 0.0, 0.5], F)
    return np.stack([np.broadcast_to(apex, (n, 3)), rim[:-1], rim[1:]], 1)


def torus(nu=64, nv=32, R=2.0, r=0.75):
    """2 * nu * nv triangles, closed, wound outwards; every vertex position is computed once, so that neighbours share bits"""
    u, v = np.arange(nu) * (2 * np.pi / nu), np.arange(nv) * (2 * np.pi / nv)
    uu, vv = np.meshgrid(u, v, indexing="ij")
    p = np.stack([(R + r * np.cos(vv)) * np.cos(uu), (R + r * np.cos(vv)) * np.sin(uu), r * np.sin(vv)], -1).astype(F)
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    i1, j1 = (i + 1) % nu, (j + 1) % nv
    a, b, c, d = p[i, j], p[i1, j], p[i1, j1], p[i, j1]
    return np.concatenate([np.stack([a, b, c], 2).reshape(-1, 3, 3), np.stack([a, c, d], 2).reshape(-1, 3, 3)]).astype(F)


def torus_inside(points, R=2.0, r=0.75):
    p = np.asarray(points, np.float64)
    return (np.hypot(np.hypot(p[:, 0], p[:, 1]) - R, p[:, 2]) < r)


def defect_mesh():
    """a cube and four more records: a zero-area triangle (two equal vertices), one with all three vertices equal, one that has
    at -0.0 a vertex another has at +0.0, one with a NaN coordinate"""
    extra = np.array([[[1, 1, 1], [1, 1, 1], [2, 2, 1]], [[1, -1, 1], [1, -1, 1], [1, -1, 1]],
                      [[0.0, 3, 0], [1, 3, 0], [0, 4, 0]], [[-0.0, 3, -0.0], [0, 4, 0], [-1, 3, 0]], [[1, 1, 1], [np.nan, 0, 0], [3, 3, 3]]], F)
    return np.concatenate([cube(), extra])


def cpu_meshes():
    """name -> tris [T, 3, 3] float32: the meshes of the CPU test. Two meshes that meet are, as records, the concatenation."""
    L = l_prism().triangles()
    half = len(L) // 2
    c = cube()
    turned = c.copy()
    turned[3] = turned[3, [0, 2, 1]]
    edge3 = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[1, 0, 0], [0, 0, 0], [0, 0, 1]], [[0, 0, 0], [1, 0, 0], [0, -1, -1]]], F)
    top = (c[:, :, 2] == 1).all(1)
    return {"tetrahedron": tetrahedron(), "cube": c, "L prism": L, "L, vertices duplicated per face": L.copy(),
            "L as two meshes": np.concatenate([L[half:], L[:half]]), "single triangle": tetrahedron()[:1], "cube without a face": c[~top],
            "three triangles on one edge": edge3, "cube, one triangle turned": turned, "defects": defect_mesh(), "fan of 200": fan(200)}


# ---------------------------------------------------------------------------------------------- queries

CLASSES = ("face", "convex edge", "concave edge", "convex vertex", "saddle or concave vertex")


def _class_of(shape, tri, region):
    if region == 7:
        return "face"
    if region in (1, 2, 4):
        k = shape.kind_of_place(tri[{1: 0, 2: 1, 4: 2}[region]].astype(np.float64))
        return {"convex": "convex vertex", "saddle": "saddle or concave vertex", "flat": "face"}.get(k, k)
    i, j = {3: (0, 1), 5: (0, 2), 6: (1, 2)}[region]
    k = shape.kind_of_edge(tri[i], tri[j])
    return "face" if k == "flat" else k


def class_queries(shape, per_class, seed, min_rel=1e-3):
    """per_class queries of each of CLASSES round a Boxes shape: candidates are drawn near vertices, edges and faces (and on the
    grid lines through the saddle vertices, where alone such a vertex is the nearest feature, and near the concave edges), answered by the float32 reference,
    kept only if their float64 distance is at least min_rel of the shape's size, and sorted by the kind of the feature the
    answer lies on. Returns (points [5 * per_class, 3] float32, class index per point, region per point)."""
    rng = np.random.RandomState(seed)
    tris = shape.triangles()
    table, _ = table_np(tris)
    verts = np.unique(tris.reshape(-1, 3), axis=0).astype(np.float64)
    saddles = np.array([v for v in verts if shape.kind_of_place(v) == "saddle"])
    ends = np.concatenate([tris[:, [0, 1]], tris[:, [0, 2]], tris[:, [1, 2]]]).astype(np.float64)
    concave = np.array([e for e in ends if shape.kind_of_edge(e[0], e[1]) == "concave edge"])
    got = {c: [] for c in CLASSES}
    regs = {c: [] for c in CLASSES}
    known = {}
    for _ in range(60):
        if all(len(got[c]) >= per_class for c in CLASSES):
            break
        n = 3000
        t = tris[rng.randint(len(tris), size=n)].astype(np.float64)
        w = rng.dirichlet([1, 1, 1], n)
        on = {0: verts[rng.randint(len(verts), size=n)], 1: t[:, 0] + (t[:, 1] - t[:, 0]) * rng.uniform(0, 1, (n, 1)),
              2: (t * w[:, :, None]).sum(1), 3: saddles[rng.randint(len(saddles), size=n)]}
        ce = concave[rng.randint(len(concave), size=n)]
        on[4] = ce[:, 0] + (ce[:, 1] - ce[:, 0]) * rng.uniform(0, 1, (n, 1))
        d = rng.standard_normal((n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        axis_d = (np.eye(3)[rng.randint(3, size=n)] * rng.choice([-1.0, 1.0], (n, 1))) @ shape.R.T
        r = shape.size * 10.0 ** rng.uniform(-2.7, -0.5, (n, 1))
        for kind in range(5):
            p = (on[kind] + (axis_d if kind == 3 else d) * r).astype(F)
            keep = distance64(tris, p) >= min_rel * shape.size
            p = p[keep]
            _, rec, _, region, _ = signed_np(tris, table, p, np.full(len(p), RTK_INF, F))
            for x, pr, rg in zip(p, rec[:, 3], region):
                if (int(pr), int(rg)) not in known:
                    known[(int(pr), int(rg))] = _class_of(shape, tris[pr], int(rg))
                c = known[(int(pr), int(rg))]
                if len(got[c]) < per_class:
                    got[c].append(x); regs[c].append(int(rg))
    assert all(len(got[c]) == per_class for c in CLASSES), {c: len(got[c]) for c in CLASSES}
    return (np.array([x for c in CLASSES for x in got[c]], F), np.repeat(np.arange(len(CLASSES)), per_class),
            np.array([x for c in CLASSES for x in regs[c]]))
