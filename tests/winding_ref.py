"""The rule of rtk_amd/csrc/rtk_winding_rule.h restated in numpy, for tests/test_winding_cpu.py (against the header's driver) and
tests/test_gpu_winding.py (against the kernels): the triangle term, the far term, the accept test and a slot's moments in float32,
operation by operation in the header's order; a float64 brute-force winding number with numpy.arctan2; a float64 walk over a
table of moments read back from the device; and the meshes both tests use. Nothing here reads the library."""
import numpy as np

from tests.closest_ref import _dot
from tests.sign_ref import F, _cross, angle_np, cube

INV_4PI = F(0.0795774683)
R_UP = F(1.00000381)
NAN_BITS = 0x7FC00000
NONE, LEAF = 0xFFFFFFFF, 0x80000000


def triangle_np(p, a, b, c):
    """rtk_winding_triangle in float32; the arrays broadcast over their leading axes"""
    p, a, b, c = (np.asarray(x, F) for x in (p, a, b, c))
    with np.errstate(all="ignore"):
        A, B, C = a - p, b - p, c - p
        la, lb, lc = np.sqrt(_dot(A, A)), np.sqrt(_dot(B, B)), np.sqrt(_dot(C, C))
        num = _dot(A, _cross(B, C))
        den = la * lb * lc
        den = den + _dot(A, B) * lc
        den = den + _dot(A, C) * lb
        den = den + _dot(B, C) * la
        out = F(2) * angle_np(num, den) * INV_4PI
    assert out.dtype == F
    return out


def far_np(p, N, P):
    """rtk_winding_far in float32"""
    p, N, P = (np.asarray(x, F) for x in (p, N, P))
    with np.errstate(all="ignore"):
        d = P - p
        r2 = _dot(d, d)
        out = _dot(N, d) / (r2 * np.sqrt(r2)) * INV_4PI
    assert out.dtype == F
    return out


def accept_np(r2, beta, R):
    with np.errstate(all="ignore"):
        br = np.asarray(beta, F) * np.asarray(R, F)
        return np.asarray(r2, F) > br * br


def tri_moments_np(a, b, c):
    """rtk_winding_tri_moments: [..., 7] = area vector, area, area * centroid"""
    a, b, c = (np.asarray(x, F) for x in (a, b, c))
    with np.errstate(all="ignore"):
        k = _cross(b - a, c - a)
        n = F(0.5) * k
        area = F(0.5) * np.sqrt(_dot(k, k))
        g = (a + b + c) / F(3)
        out = np.concatenate([n, area[..., None], area[..., None] * g], -1)
    assert out.dtype == F
    return out


def slot_np(sums, lo, hi):
    """rtk_winding_slot: sums [7], the child's box -> [7] = N, P, R"""
    sums, lo, hi = (np.asarray(x, F) for x in (sums, lo, hi))
    with np.errstate(all="ignore"):
        c = lo * F(0.5) + hi * F(0.5)
        h = hi * F(0.5) - lo * F(0.5)
        P = sums[4:7] / sums[3] if (sums[3] > 0 and sums[3] < np.inf) else c
        e = P - c
        R = (np.sqrt(_dot(e, e)) + np.sqrt(_dot(h, h))) * R_UP
    return np.concatenate([sums[:3], P, [R]]).astype(F)


def brute32(tris, points):
    """the float32 sum of the triangle terms over all records in row order, starting from +0 (what RTK_WINDING_EXACT gives, up
    to the order of the sum)"""
    tris = np.ascontiguousarray(tris, F)
    w = np.zeros(len(points), F)
    for t in tris:
        w = w + triangle_np(points, t[0], t[1], t[2])
    return w


def brute64(tris, points):
    """float64 winding numbers with numpy.arctan2: the reference"""
    t = np.asarray(tris, np.float64)
    p = np.asarray(points, np.float64)
    out = np.zeros(len(p))
    for lo in range(0, len(p), 256):
        q = p[lo:lo + 256, None, :]
        A, B, C = t[None, :, 0] - q, t[None, :, 1] - q, t[None, :, 2] - q
        la, lb, lc = np.linalg.norm(A, axis=-1), np.linalg.norm(B, axis=-1), np.linalg.norm(C, axis=-1)
        num = (A * np.cross(B, C)).sum(-1)
        den = la * lb * lc + (A * B).sum(-1) * lc + (A * C).sum(-1) * lb + (B * C).sum(-1) * la
        out[lo:lo + 256] = (2.0 * np.arctan2(num, den)).sum(1) / (4.0 * np.pi)
    return out


def area_vector64(tris):
    t = np.asarray(tris, np.float64)
    k = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    return 0.5 * k.sum(0), 0.5 * np.linalg.norm(k, axis=1).sum()


def walk64(moments, points, beta, leaf_cost):
    """A float64 walk over a table read back from the device (moments [nodes, 8, 4] float32, the last row the child words):
    per point the number of triangle tests the accept test of the rule leaves, with leaf_cost(first_slot) -> triangles of the leaf."""
    m = np.asarray(moments, F)
    child = m[:, 7].view(np.uint32)
    N, P, R = m[:, 0:3].astype(np.float64), m[:, 3:6].astype(np.float64), m[:, 6].astype(np.float64)
    tests = np.zeros(len(points), np.int64)
    for i, p in enumerate(np.asarray(points, np.float64)):
        stack = [0]
        while stack:
            top = stack.pop()
            if top & LEAF:
                tests[i] += leaf_cost(top & 0x7FFFFFFF)
                continue
            for k in range(4):
                ref = int(child[top, k])
                if ref == NONE:
                    continue
                d = P[top, :, k] - p
                if d @ d > (beta * R[top, k]) ** 2:
                    continue
                stack.append(ref)
    return tests


# ---------------------------------------------------------------------------------------------- meshes

def icosphere(level=3, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """20 * 4^level triangles (1280 at level 3), closed, wound outwards; every vertex is computed once"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    verts = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, out = {}, []

        def middle(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                x = verts[i] + verts[j]
                verts.append(x / np.linalg.norm(x))
                mid[key] = len(verts) - 1
            return mid[key]
        for a, b, c in faces:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = out
    p = (np.array(verts) * radius + np.asarray(centre, np.float64)).astype(F)
    return p[np.array(faces)]


def open_cube():
    """the cube [-1, 1]^3 without its top (z = 1) face: ten triangles; the missing face's area vector is (0, 0, 4)"""
    c = cube()
    return c[~(c[:, :, 2] == 1).all(1)]


# ---------------------------------------------------------------------------------------------- fixtures and queries

def fixtures():
    """name -> (tris [T, 3, 3] float32, the shape's size): the closed torus, L and plus of tests/sign_ref.py (the two box shapes
    turned out of the axes), an icosphere of 1280 triangles and the cube without its top"""
    from tests.sign_ref import TILT, l_prism, plus_shape, torus
    L, plus = l_prism(TILT), plus_shape(TILT)
    return {"torus": (torus(64, 32), 5.5), "L": (L.triangles(), L.size), "plus": (plus.triangles(), plus.size),
            "icosphere": (icosphere(3), 2.0), "open cube": (open_cube(), 2.0)}


def query_points(tris, size, n, seed, keep_off=0.05):
    """n points uniform in the mesh's box grown by a quarter of the size on every side, none nearer than keep_off * size to any
    triangle by the float64 closest distance -- there the term is smooth and float64 is a meaningful reference"""
    from tests.sign_ref import distance64
    rng = np.random.RandomState(seed)
    v = np.asarray(tris, np.float64).reshape(-1, 3)
    lo, hi = v.min(0) - 0.25 * size, v.max(0) + 0.25 * size
    out = np.zeros((0, 3), F)
    while len(out) < n:
        p = rng.uniform(lo, hi, (2 * n, 3)).astype(F)
        out = np.concatenate([out, p[distance64(tris, p) >= keep_off * size]])
    return np.ascontiguousarray(out[:n])
