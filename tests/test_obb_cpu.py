"""Triangles that touch an oriented box without a GPU: the rule of rtk_amd/csrc/rtk_obb_rule.h, run by tests/obb_rule_driver.cpp
under the address and undefined-behaviour sanitizers, against numpy (tests/obb_ref.py): bit for bit on random inputs; on integer
inputs with all 48 signed-permutation axes, where every float32 operation of the rule is exact, against the same thirteen axes in
Python integers and against the triangle clipped against the box in fractions; the skip against the candidates; a host walk of a
small 4-wide tree in three child orders against brute force; the accuracy against the same rule in float64; and the parts of the
interface that need no device -- header text, symbols, argtypes, the refusals decided before any HIP call."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from tests.obb_ref import brute_force_obbs, candidate_np, live_np, reach_np, separated13_np, skip_np, to_frame_np
from tests.box_ref import boxes_touch_np
from tests.test_box_cpu import clipped_is_not_empty, enlarged, integer_cases, sat13_integers, split_segment
from tests.test_within_cpu import hexes, run_driver, small_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_BAD_ARG = -2
F = np.float32


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """The driver built against the rule headers alone (no HIP include path, -Wall -Werror, no FMA contraction as in the
    library) with both sanitizers. -O2 and -mfma: a compiler that were allowed to contract would do it here."""
    exe = str(tmp_path_factory.mktemp("obb_rule") / "obb_rule_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-mfma", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "rtk_amd", "csrc"), os.path.join(ROOT, "tests", "obb_rule_driver.cpp"), "-o", exe])
    return exe


def run_bulk(exe, v, q, clo, chi, tmp_path, name):
    """v [N, 3, 3], q [N, 15], clo / chi [N, 3], float32 -> (bits uint8 [N]: 1 live, 2 boxes touch, 4 separated, 8 skip;
    qlo and qhi words uint32 [N, 3] each)"""
    words = np.concatenate([v.reshape(-1, 9), q, clo, chi], 1).astype(F)
    assert words.shape[1] == 30
    path, out = str(tmp_path / (name + ".bin")), str(tmp_path / (name + ".out"))
    words.tofile(path)
    r = subprocess.run([exe, "-b", path, out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout == "ok\n", r.stdout[-200:] + r.stderr[-4000:]
    got = np.fromfile(out, np.uint32).reshape(-1, 7)
    assert len(got) == len(words)
    return got[:, 0].astype(np.uint8), got[:, 1:4], got[:, 4:7]


def numpy_bits(v, q, clo, chi):
    _, qlo, qhi = reach_np(q)
    bits = live_np(q) * 1 + boxes_touch_np(v[:, 0], v[:, 1], v[:, 2], qlo, qhi) * 2 + separated13_np(q, v[:, 0], v[:, 1], v[:, 2]) * 4 + skip_np(q, clo, chi) * 8
    assert ((bits & 7 == 3) == candidate_np(q, v[:, 0], v[:, 1], v[:, 2])).all()
    return bits.astype(np.uint8), qlo, qhi


def same_floats(words, x):
    """bit for bit, a NaN equal to any NaN"""
    x = np.ascontiguousarray(x, F)
    return ((words == x.view(np.uint32)) | (np.isnan(words.view(F)) & np.isnan(x))).all()


def quaternion_rows(rng, n):
    """rotations from random unit quaternions, converted in float64 and rounded once to float32: [n, 9], rows = axes"""
    from rtk_amd.api import obb_axes
    return obb_axes(rng.normal(size=(n, 4)), n).reshape(n, 9)


SIGNED_PERMUTATIONS = [np.array([[s[r] * (p[r] == c) for c in range(3)] for r in range(3)])
                       for p in itertools.permutations(range(3)) for s in itertools.product((1, -1), repeat=3)]


# ---------------------------------------------------------------------------------------------- random inputs

PER = 40000


def float_cases(seed=3, per=PER):
    """-> v [N, 3, 3], q [N, 15]. Five pairs of (triangle size, box size) with the box about a point of the triangle and a
    rotation of its own; then the same geometry with queries that are not live or whose axes are not a rotation"""
    rng = np.random.RandomState(seed)
    vs, qs = [], []
    for tri, box in ((1.0, 1.0), (1.0, 0.05), (0.05, 1.0), (1e3, 1e-3), (1e-3, 1e3)):
        centre = rng.uniform(-1, 1, (per, 1, 3)) * max(tri, box)
        v = centre + rng.uniform(-tri, tri, (per, 3, 3))
        bary = rng.dirichlet([1, 1, 1], per)
        mid = (v * bary[:, :, None]).sum(1) + rng.uniform(-1.5, 1.5, (per, 3)) * box
        half = rng.uniform(0, box, (per, 3)) * (rng.randint(0, 6, (per, 3)) != 0)          # a sixth of the extents are 0
        vs.append(v); qs.append(np.concatenate([mid, half, quaternion_rows(rng, per)], 1))
    # identity and signed-permutation axes
    v = rng.uniform(-1, 1, (per // 2, 3, 3))
    mid = v.mean(1) + rng.uniform(-0.5, 0.5, (per // 2, 3))
    axes = np.array([SIGNED_PERMUTATIONS[k % 48].reshape(9) for k in range(per // 2)], np.float64)
    vs.append(v); qs.append(np.concatenate([mid, rng.uniform(0, 0.5, (per // 2, 3)), axes], 1))
    # what the gate is for: NaN and infinite members, negative halves, scaled, sheared and zero axes, huge numbers
    m = per
    v = rng.uniform(-1, 1, (m, 3, 3)) * rng.choice([1.0, 1.0, 1e30, 3e38], (m, 1, 1))
    q = np.concatenate([v.mean(1) + rng.uniform(-0.3, 0.3, (m, 3)), rng.uniform(0, 0.5, (m, 3)), quaternion_rows(rng, m)], 1)
    kind = rng.randint(0, 10, m)
    rows = np.arange(m)
    col = rng.randint(0, 15, m)
    k0 = kind == 0
    q[rows[k0], col[k0]] = rng.choice([np.nan, np.inf, -np.inf], k0.sum())
    k1 = kind == 1
    q[rows[k1], 3 + col[k1] % 3] *= -1                                               # a negative half (or -0, which is legal)
    k2 = kind == 2
    q[k2, 6:] *= rng.choice([1.01, 0.99, 1.0004, 0.9996, 2.0, 1e20], (k2.sum(), 1))  # scaled, on both sides of the gate
    k3 = kind == 3
    q[k3, 6:9] += rng.choice([1e-4, 1e-3, 1e-2, 0.3], (k3.sum(), 1)) * q[k3, 9:12]   # sheared, on both sides of the gate
    k4 = kind == 4
    for j in range(3):
        z = k4 & (col % 3 == j)
        q[z, 6 + 3 * j:9 + 3 * j] = 0                                                # a zero axis
    k5 = kind == 5
    q[k5, 6:] = 0                                                                    # all axes zero
    k6 = kind == 6
    q[k6, 3:6] *= rng.choice([1e30, 3e38], (k6.sum(), 1))                            # a reach that overflows
    k7 = kind == 7
    q[k7, 0:3] *= 3e38
    vs.append(v); qs.append(q)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.concatenate(vs).astype(F), np.concatenate(qs).astype(F)


def test_random_inputs_equal_numpy_bit_for_bit(driver, tmp_path):
    v, q = float_cases()
    n = len(v)
    assert n >= 200000
    clo, chi = enlarged(np.random.RandomState(2), v)
    got, qlo_w, qhi_w = run_bulk(driver, v, q, clo, chi, tmp_path, "floats")
    ref, qlo, qhi = numpy_bits(v, q, clo, chi)
    bad = np.nonzero(got != ref)[0]
    assert len(bad) == 0, (len(bad), bad[:5], got[bad[:5]], ref[bad[:5]], v[bad[:2]], q[bad[:2]])
    assert same_floats(qlo_w, qlo) and same_floats(qhi_w, qhi)
    cand = (got & 7) == 3
    for k, name in enumerate(("1 / 1", "1 / 0.05", "0.05 / 1", "1e3 / 1e-3", "1e-3 / 1e3")):
        part = got[k * PER:(k + 1) * PER]
        print("%-12s candidates %5.1f %%, separated in the frame behind touching boxes %5.1f %%" % (name, 100 * ((part & 7) == 3).mean(), 100 * ((part & 7) == 7).mean()))
        assert 0.02 < ((part & 7) == 3).mean() < 0.98, name
        assert (part & 1).all(), name                                  # (rotations from float32-rounded quaternions pass the gate)
    assert ((got & 7) == 7).sum() > 5000
    perm = got[5 * PER:5 * PER + PER // 2]
    assert (perm & 1).all() and 0.02 < ((perm & 7) == 3).mean() < 0.98
    gate = got[5 * PER + PER // 2:]
    dead = (gate & 1) == 0
    print("the gate's cases: %d of %d not live" % (dead.sum(), len(gate)))
    assert 0.3 * len(gate) < dead.sum() < 0.8 * len(gate)
    # rule 4 never skips a box above a candidate
    assert not ((got & 8 != 0) & cand).any() and (got & 8 != 0).sum() > 0.1 * n


def test_the_gate_is_the_sweeps(driver, tmp_path):
    """Scaled and sheared axes on either side of the tolerance: live exactly where tests/obbsweep_ref.py's gate says, for queries
    that are finite and have half >= 0"""
    from tests import obbsweep_ref
    rng = np.random.RandomState(12)
    n = 20000
    axes = quaternion_rows(rng, n).astype(np.float64)
    axes *= 1 + rng.uniform(-2, 2, (n, 1)) * 2.0 ** -11
    axes[:, 0:3] += rng.uniform(-2, 2, (n, 1)) * 2.0 ** -10 * axes[:, 3:6]
    q = np.concatenate([rng.uniform(-1, 1, (n, 3)), rng.uniform(0, 1, (n, 3)), axes], 1).astype(F)
    v = rng.uniform(-1, 1, (n, 3, 3)).astype(F)
    got, _, _ = run_bulk(driver, v, q, v[:, 0], v[:, 0], tmp_path, "gate")
    live = (got & 1) != 0
    assert 0.2 * n < live.sum() < 0.8 * n
    assert (live == live_np(q)).all()
    # the sweep's own reference on a query with these axes: origin, direction, min_t, max_t, half, axes
    sweep = obbsweep_ref.prepare(np.concatenate([q[:, 0:3], np.tile(F([1, 0, 0]), (n, 1)), np.tile(F([0, 1]), (n, 1)), q[:, 3:6], q[:, 6:15]], 1).astype(F))
    assert (sweep.live == live).all()
    assert sweep.H.tobytes() == reach_np(q)[0].tobytes()             # (and the reach is the sweep's, bit for bit)


# ---------------------------------------------------------------------------------------------- integer inputs, 48 frames

def test_integer_inputs_in_all_48_frames_equal_the_exact_answers(driver, tmp_path):
    """The integer cases of tests/test_box_cpu.py (touching faces, corners on edges, degenerate triangles and boxes), doubled so
    that the box's centre is an integer, carried into the scene by each of the 48 signed permutations: the rule on the oriented
    query equals the thirteen axes in Python integers and the clipped triangle in fractions on the axis-aligned original"""
    v, lo, hi = integer_cases(seed=11, n=9600)
    n = len(v)
    c2, h2 = lo + hi, hi - lo                                        # the box in the frame, in half units: centre c2, half h2
    w = 2 * v - c2[:, None, :]                                       # the vertices in the frame, about the box's centre
    rng = np.random.RandomState(4)
    P = np.array([SIGNED_PERMUTATIONS[i % 48] for i in range(n)])    # rows = the box's axes in scene coordinates
    cs = rng.randint(-20, 21, (n, 3))
    vs = cs[:, None, :] + np.einsum("nji,nkj->nki", P, w)            # v_scene = centre + P^T w
    assert (np.einsum("nij,nkj->nki", P, vs - cs[:, None, :]) == w).all()
    assert np.abs(vs).max() < 256 and np.abs(w).max() <= 192
    q = np.concatenate([cs, h2, P.reshape(n, 9)], 1).astype(F)
    vf = vs.astype(F)
    clo, chi = enlarged(np.random.RandomState(1), vf)
    got, qlo_w, qhi_w = run_bulk(driver, vf, q, clo, chi, tmp_path, "integers")
    ref, qlo, qhi = numpy_bits(vf, q, clo, chi)
    assert (got == ref).all(), np.nonzero(got != ref)[0][:10]
    assert same_floats(qlo_w, qlo) and same_floats(qhi_w, qhi)
    assert (got & 1).all()
    # the reach of a signed permutation is the permuted half, exactly
    assert (qlo == cs - np.einsum("nji,nj->ni", np.abs(P), h2)).all() and (qhi == cs + np.einsum("nji,nj->ni", np.abs(P), h2)).all()
    cand = (got & 7) == 3
    want = np.array([sat13_integers(v[i], lo[i], hi[i]) for i in range(n)])
    bad = np.nonzero(cand != want)[0]
    assert len(bad) == 0, (len(bad), v[bad[:3]], lo[bad[:3]], hi[bad[:3]], P[bad[:3]])
    e0, e1 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 1]
    proper = np.cross(e0, e1).any(1)
    exact = np.array([clipped_is_not_empty(v[i], lo[i], hi[i]) for i in np.nonzero(proper)[0]])
    bad = np.nonzero(proper)[0][cand[proper] != exact]
    assert len(bad) == 0, (len(bad), v[bad[:3]], lo[bad[:3]], hi[bad[:3]], P[bad[:3]])
    print("integer cases %d: candidates %d, proper %d, degenerate candidates %d" % (n, cand.sum(), proper.sum(), (cand & ~proper).sum()))
    assert 0.15 * n < cand.sum() < 0.85 * n and (cand & ~proper).sum() > 200
    for k in range(48):                                              # every frame saw both answers
        assert cand[k::48].any() and not cand[k::48].all(), k
    touching = cand & ((v.min(1) == hi) | (v.max(1) == lo)).any(1)
    assert touching.sum() > 200
    assert ((h2 == 0).sum(1) == 3).sum() > 20 and ((h2 == 0).sum(1) == 1).sum() > 400
    assert not ((got & 8 != 0) & cand).any() and (got & 8 != 0).sum() > 0.1 * n


# ---------------------------------------------------------------------------------------------- tree

def walk_queries(rng, tris):
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    ext = hi - lo
    qs = []
    mid = rng.uniform(lo, hi, (60, 3))
    half = rng.choice([0.02, 0.1, 0.3], (60, 1)) * ext * rng.uniform(0.2, 1, (60, 3))
    qs.append(np.concatenate([mid, half, quaternion_rows(rng, 60)], 1))
    verts = tris[rng.permutation(len(tris))[:15], 1]
    qs.append(np.concatenate([verts, np.zeros((15, 3)), quaternion_rows(rng, 15)], 1))          # point boxes at vertices
    ident = np.tile(np.eye(3).reshape(1, 9), (15, 1))
    qs.append(np.concatenate([verts, np.zeros((15, 3)), ident], 1))
    qs.append(np.concatenate([np.tile((lo + hi) / 2, (2, 1)), np.tile(ext, (2, 1)), quaternion_rows(rng, 2)], 1))   # the whole scene
    dead = np.concatenate([np.tile((lo + hi) / 2, (4, 1)), np.tile(ext, (4, 1)), np.tile(np.eye(3).reshape(1, 9), (4, 1))], 1)
    dead[0, 0:3] = hi + 10 * ext                                     # far away
    dead[1, 4] = -1.0                                                # a negative half
    dead[2, 7] = np.nan
    dead[3, 6:] *= 1.01                                              # not orthonormal
    qs.append(dead)
    q = np.concatenate(qs).astype(F)
    room = rng.randint(0, 7, len(q))
    room[::7] = len(tris)                                            # room for the whole list
    return q, room


def test_host_walk_equals_brute_force_in_every_order(driver, tmp_path):
    """A soup under a random 4-wide tree, leaves of 1 to 5: count and kept prefix equal brute force bit for bit whichever way the
    children are visited"""
    rng = np.random.RandomState(5)
    tris = (rng.uniform(0, 1, (90, 1, 3)) + rng.uniform(-0.08, 0.08, (90, 3, 3))).astype(F)
    nodes, recs = small_tree(rng, tris, 5)
    assert len(nodes) > 8
    q, room = walk_queries(rng, tris)
    ref = brute_force_obbs(tris, np.arange(len(tris)), q, room)
    assert (ref.counts == 0).any() and (ref.counts > 6).any() and (ref.counts == 90).any() and (ref.counts[-4:] == 0).all()
    assert (ref.step1.sum(1) > ref.counts).any()                     # (the frame did decide)
    text = "n %d %s\nt %d %s\n" % (len(nodes), hexes(nodes), len(recs), hexes(recs))
    qwords = np.concatenate([q.view(np.uint32), room.astype(np.uint32)[:, None]], 1)
    for order in (0, 1, 2):
        out = run_driver(driver, text + "".join("q %d %s\n" % (order, hexes(w)) for w in qwords), len(qwords), tmp_path, "walk_%d" % order)
        for i, line in enumerate(out):
            want = ref.kept[i]
            seg = split_segment(line[2:], int(room[i]))
            assert int(line[0]) == ref.counts[i], (order, i)
            assert int(line[1]) == len(want), (order, i)
            assert seg[:len(want)].tobytes() == want.tobytes(), (order, i)
            assert (seg[len(want):] == 0x7e7e7e7e).all(), (order, i)
    # a scene without triangles: no candidates
    out = run_driver(driver, "n 0\nt 0\nq 0 %s\n" % hexes(qwords[0]), 1, tmp_path, "empty")
    assert out[0][:2] == ["0", "0"]


# ---------------------------------------------------------------------------------------------- accuracy

# measured by test_accuracy_against_float64 below (printed there); the assertion is at 2.5 times the measured worst, the
# project's convention. The rule header and the README state the same two numbers.
MEASURED_K = 1.29
MEASURED_DISAGREEMENTS = 37118
ASSERTED_K = 3.23                              # 2.5 * 1.29, rounded up


def axes16(q, v0, v1, v2):
    """The sixteen comparisons of the rule in the dtype of its inputs, in the rule's order of operations: -> (separates bool
    [..., 16], margin [..., 16]): the margin is by how much the axis separates (> 0) or keeps (<= 0), as a length: divided by the
    length of the axis where the axis is not a unit vector. Axes 0-2: step 1; 3-5: the box's own; 6-14: the edges; 15: the plane."""
    c, h = q[..., 0:3], q[..., 3:6]
    _, qlo, qhi = reach_np(q)
    tlo, thi = np.minimum(np.minimum(v0, v1), v2), np.maximum(np.maximum(v0, v1), v2)
    sep, mar = [], []
    for a in range(3):
        sep.append(~((tlo[..., a] <= qhi[..., a]) & (thi[..., a] >= qlo[..., a])))
        mar.append(np.maximum(tlo[..., a] - qhi[..., a], qlo[..., a] - thi[..., a]))
    p = [to_frame_np(q, v) for v in (v0, v1, v2)]
    for j in range(3):
        x, hj = [pk[..., j] for pk in p], h[..., j]
        sep.append(((x[0] > hj) & (x[1] > hj) & (x[2] > hj)) | ((x[0] < -hj) & (x[1] < -hj) & (x[2] < -hj)))
        mar.append(np.maximum(np.minimum(np.minimum(x[0], x[1]), x[2]) - hj, -hj - np.maximum(np.maximum(x[0], x[1]), x[2])))
    e = [p[1] - p[0], p[2] - p[1], p[0] - p[2]]
    with np.errstate(divide="ignore", invalid="ignore"):
        for ej in e:
            for ia, ib in ((1, 2), (2, 0), (0, 1)):
                ea, eb = ej[..., ia], ej[..., ib]
                x = [ea * pk[..., ib] - eb * pk[..., ia] for pk in p]
                r = h[..., ia] * np.abs(eb) + h[..., ib] * np.abs(ea)
                sep.append(((x[0] > r) & (x[1] > r) & (x[2] > r)) | ((x[0] < -r) & (x[1] < -r) & (x[2] < -r)))
                m = np.maximum(np.minimum(np.minimum(x[0], x[1]), x[2]) - r, -r - np.maximum(np.maximum(x[0], x[1]), x[2]))
                mar.append(m / np.sqrt(ea * ea + eb * eb))
        n = [e[0][..., 1] * e[1][..., 2] - e[0][..., 2] * e[1][..., 1], e[0][..., 2] * e[1][..., 0] - e[0][..., 0] * e[1][..., 2],
             e[0][..., 0] * e[1][..., 1] - e[0][..., 1] * e[1][..., 0]]
        d = (n[0] * p[0][..., 0] + n[1] * p[0][..., 1]) + n[2] * p[0][..., 2]
        r = (h[..., 0] * np.abs(n[0]) + h[..., 1] * np.abs(n[1])) + h[..., 2] * np.abs(n[2])
        sep.append((d > r) | (d < -r))
        mar.append((np.abs(d) - r) / np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]))
    return np.stack(sep, -1), np.stack(mar, -1)


def accuracy_cases(rng, per):
    """(triangle size, box size, where) at four scales; rotations from unit quaternions rounded to float32. A quarter of the boxes
    lie about a random point near the triangle. Random cases are rarely within a rounding of a threshold, so the others are
    contacts by construction, exact but for the rounding of the centre to float32: a vertex on a face of the box; a corner of
    the box on the triangle's plane with the box on one side of it; an edge of the box on an edge of the triangle with the box
    on one side of the plane the two edges span."""
    vs, qs = [], []
    for tri, box, where in ((1.0, 1.0, 1.0), (1.0, 0.05, 1.0), (0.05, 1.0, 1.0), (1.0, 0.3, 100.0)):
        centre = rng.uniform(-1, 1, (per, 1, 3)) * where
        v = centre + rng.uniform(-tri, tri, (per, 3, 3))
        bary = rng.dirichlet([1, 1, 1], per)
        half = rng.uniform(0.05 * box, box, (per, 3))
        rows = quaternion_rows(rng, per)
        U = rows.astype(np.float64).reshape(per, 3, 3)
        kind = rng.randint(0, 4, per)
        j = rng.randint(0, 3, per)
        at_j = np.arange(3)[None, :] == j[:, None]
        # the contact point on the triangle, and where on the box's surface it lies (in the box's frame)
        pt = (v * bary[:, :, None]).sum(1)
        pt[kind == 1] = v[kind == 1, 0]
        t = rng.uniform(0, 1, (per, 1))
        pt[kind == 3] = (v[:, 0] + t * (v[:, 1] - v[:, 0]))[kind == 3]
        inside = rng.uniform(-1, 1, (per, 3)) * half
        a = inside.copy()
        a[kind == 1] = np.where(at_j, rng.choice([-1.0, 1.0], (per, 1)) * half, inside)[kind == 1]
        n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
        flip = rng.choice([-1.0, 1.0], (per, 1))
        a[kind == 2] = (-np.sign(np.einsum("nij,nj->ni", U, n)) * flip * half)[kind == 2]
        d = np.cross(v[:, 1] - v[:, 0], U[np.arange(per), j])
        a[kind == 3] = np.where(at_j, inside, -np.sign(np.einsum("nij,nj->ni", U, d)) * flip * half)[kind == 3]
        mid = pt - np.einsum("nj,nji->ni", a, U)
        # ... and off the contact by nothing, or by up to 1, 4, 16 or 64 ulps of the largest coordinate: the band in which
        # float32 can get the answer wrong has to be probed from both sides, not only at its middle
        mid += rng.uniform(-1, 1, (per, 3)) * rng.choice([0.0, 1.0, 4.0, 16.0, 64.0], (per, 1)) * 2.0 ** -23 * np.abs(v).max((1, 2))[:, None]
        mid[kind == 0] = (pt + rng.uniform(-1.5, 1.5, (per, 3)) * box)[kind == 0]
        vs.append(v); qs.append(np.concatenate([mid, half, rows], 1))
    return np.concatenate(vs).astype(F), np.concatenate(qs).astype(F)


def test_accuracy_against_float64():
    """Over 1.2 million random (triangle, box, rotation) cases: wherever the float32 rule and the same rule in float64 disagree
    about candidate or not, every axis whose comparison came out differently has a float64 margin within K * 2^-23 of the
    largest coordinate magnitude involved. K is what this test measures; it is asserted at 2.5 times the measured worst."""
    rng = np.random.RandomState(77)
    total = disagree = 0
    worst = 0.0
    for chunk in range(6):
        v, q = accuracy_cases(rng, 50000)
        total += len(v)
        cand32 = candidate_np(q, v[:, 0], v[:, 1], v[:, 2])
        sep32, _ = axes16(q, v[:, 0], v[:, 1], v[:, 2])
        assert (live_np(q)).all() and (cand32 == ~sep32.any(-1)).all()             # (axes16 is the rule, comparison by comparison)
        q64, v64 = q.astype(np.float64), v.astype(np.float64)
        sep64, mar64 = axes16(q64, v64[:, 0], v64[:, 1], v64[:, 2])
        assert live_np(q64).all()
        cand64 = ~sep64.any(-1)
        bad = np.nonzero(cand32 != cand64)[0]
        disagree += len(bad)
        if len(bad) == 0:
            continue
        flipped = sep32[bad] != sep64[bad]
        gap = np.where(flipped, np.abs(mar64[bad]), 0.0).max(-1)                    # the largest margin a rounding had to cross
        _, qlo, qhi = reach_np(q64[bad])
        scale = np.maximum(np.abs(v64[bad]).max((1, 2)), np.maximum(np.abs(qlo).max(-1), np.abs(qhi).max(-1)))
        k = gap / scale / 2.0 ** -23
        worst = max(worst, float(k.max()))
    print("accuracy: %d cases, float32 and float64 disagree on %d, worst K = %.2f (asserted %s)" % (total, disagree, worst, ASSERTED_K))
    assert total >= 1000000 and disagree > 0
    assert worst <= ASSERTED_K, worst
    assert 2.5 * MEASURED_K <= ASSERTED_K < 2.5 * MEASURED_K + 0.01 and disagree > 10000


# ---------------------------------------------------------------------------------------------- the interface

def test_rule_header_includes_no_hip_and_states_its_rules():
    text = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_obb_rule.h")).read()
    assert [l.split()[1] for l in text.splitlines() if l.startswith("#include")] == ["<stdint.h>", '"rtk_closest_rule.h"', '"rtk_box_rule.h"']
    assert "hip_runtime" not in text and "__global__" not in text and "fmaf" not in text
    assert "rtk_box_boxes_touch(" in text and "rtk_box_separated(" in text and "rtk_box_skip(" in text
    flat = " ".join(text.replace("\n//", "\n").split())
    for word in ("0. LIVE", "1. BOXES", "2. THE FRAME", "3. CANDIDATE", "4. SKIP", "FLOAT RULE", "DEFINED BY IT", "IDENTITY AXES", "UP TO ROUNDING",
                 "ZERO-AREA", "WITHOUT VOLUME", "NON-FINITE", "NOTHING ELSE IS PROMISED", "NEVER SEPARATES", "WITHOUT A MARGIN", "ASCENDING PRIMITIVE ID",
                 "RTK_OBB_K = %.2f" % MEASURED_K, "RTK_OBB_DISAGREE = %d" % MEASURED_DISAGREEMENTS):
        assert word in flat, word
    # the sweep's header and the box rule are used or left alone, not changed: the tolerance is one number
    sweep = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_obbsweep_rule.h")).read()
    assert "rtk_obb_rule" not in sweep and "#define RTK_OBB_ORTHO_TOL 0.0009765625f" in sweep and "#define RTK_OBB_ORTHO_TOL 0.0009765625f" in text
    header = open(os.path.join(ROOT, "include", "rtk_amd.h")).read()
    section = header[header.index("/* ---- Triangles that touch an oriented box"):header.index("/* ---- Triangles that touch a triangle")]
    section = " ".join(section.replace("\n *", "\n").split())
    for word in ("rtk_obb_rule.h", "ARE NOT WRITTEN", "A SLOT THAT IS NOT LISTED IS NOT WRITTEN", "d_offsets[i] = i * k", "DETERMINISTIC", "NOTHING ELSE IS PROMISED",
                 "rtk_dev_trace_status", "rtk_mgpu_scene(m, i)", "CANNOT BE CULLED BY WHAT IT HAS KEPT", "ASCENDING PRIMITIVE ID", "touching counts", "2^-10"):
        assert word in section, word
    mk = open(os.path.join(ROOT, "rtk_amd", "csrc", "Makefile")).read()
    assert "rtk_obb_rule.h" in mk and "rtk_obb.hip" in mk and "rtk_overlap_walk.h" in mk
    # the shape's own calls in its file, what the three overlap shapes share in the walk
    kernel = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_obb.hip")).read()
    walk = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_overlap_walk.h")).read()
    assert "rtk_box_insert(" in walk and "rtk_obb_skip(" in kernel and "rtk_obb_candidate(" in kernel and "rtk_obb_prepare(" in kernel
    assert "kernel-resource-usage" in kernel and "scratch 0" in kernel and "OB_RESOURCES" in kernel
    layout = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_layout_check.h")).read()
    assert "static_assert(sizeof(rtk_obb_query) == 60" in layout
    dev = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_dev.h")).read()
    assert dev.index("int rtk_launch_box(") < dev.index("int rtk_launch_obb(") < dev.index("int rtk_launch_touch(")


def test_header_symbols_and_argtypes(api):
    from rtk_amd import types
    text = open(os.path.join(ROOT, "include", "rtk_amd.h")).read()
    for word in ("typedef struct rtk_obb_query { float centre[3], half[3], axes[9]; } rtk_obb_query;",
                 "int rtk_dev_triangles_in_obb_count(const rtk_dev_scene *ds, const rtk_obb_query *d_obbs, size_t num_queries,\n\tconst rtk_ray_list *list, uint32_t *d_counts, void *stream);",
                 "int rtk_dev_triangles_in_obb_all(const rtk_dev_scene *ds, const rtk_obb_query *d_obbs, size_t num_queries,\n\tconst rtk_ray_list *list, const uint64_t *d_offsets, uint32_t *d_prims, uint32_t *d_written /* may be NULL */, void *stream);",
                 "int rtk_dev_triangles_in_obb_counted(const rtk_dev_scene *ds, const rtk_obb_query *d_obbs, size_t num_queries,\n\tconst uint64_t *d_offsets, uint32_t *d_prims, uint32_t *d_counts_or_written, rtk_trace_counters *out);",
                 "uint32_t rtk_amd_obb_stack_entries(void);"):
        assert word in text, word
    assert text.index("/* ---- Triangles that touch a box") < text.index("/* ---- Triangles that touch an oriented box") < text.index("/* ---- Triangles that touch a triangle")
    dt = types.OBB_QUERY_DTYPE
    assert dt.itemsize == 60 and dt.names == ("centre", "half", "axes") and dt.fields["half"][1] == 12 and dt.fields["axes"][1] == 24

    class Query(C.Structure):
        _fields_ = [("centre", C.c_float * 3), ("half", C.c_float * 3), ("axes", C.c_float * 9)]
    assert C.sizeof(Query) == 60
    L = api.lib()
    for name in ("rtk_dev_triangles_in_obb_count", "rtk_dev_triangles_in_obb_all", "rtk_dev_triangles_in_obb_counted", "rtk_amd_obb_stack_entries"):
        assert name in api.RTK_AMD_H_SYMBOLS and hasattr(L, name), name
    assert L.rtk_dev_triangles_in_obb_count.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(api.RayList), C.c_void_p, C.c_void_p]
    assert L.rtk_dev_triangles_in_obb_all.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(api.RayList), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert L.rtk_dev_triangles_in_obb_counted.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(api.TraceCounters)]
    assert L.rtk_dev_triangles_in_obb_count.restype == C.c_int and L.rtk_dev_triangles_in_obb_all.restype == C.c_int
    assert L.rtk_dev_triangles_in_obb_counted.restype == C.c_int
    assert L.rtk_amd_obb_stack_entries.restype == C.c_uint32 and 1 <= L.rtk_amd_obb_stack_entries() <= 64
    for name in ("count_in_obbs_device", "in_obbs_all_device", "triangles_in_obbs_counted", "triangles_in_obbs", "occupancy_oriented", "occupancy"):
        assert callable(getattr(api.DeviceScene, name)), name


def test_query_arrays_on_the_host(api):
    """obb_query_array and oriented_grid need no device: shapes of half, matrices and quaternions, and the grid's cells"""
    q = api.obb_query_array(np.zeros((4, 3)), 0.5, np.eye(3))
    assert q.dtype == api.OBB_QUERY_DTYPE and (q["half"] == 0.5).all() and (q["axes"] == np.eye(3, dtype=F)).all()
    q = api.obb_query_array(np.ones((2, 3)), [1, 2, 3], [0, 0, np.sin(np.pi / 8), np.cos(np.pi / 8)])
    assert (q["half"] == F([1, 2, 3])).all() and live_np(q.view(F).reshape(2, 15)).all()
    assert np.allclose(q["axes"][0], [[np.sqrt(0.5), np.sqrt(0.5), 0], [-np.sqrt(0.5), np.sqrt(0.5), 0], [0, 0, 1]], atol=1e-7)
    with pytest.raises(api.RtkError):
        api.obb_query_array(np.zeros((4, 3)), [1, 2], np.eye(3))
    with pytest.raises(api.RtkError):
        api.oriented_grid([0, 0, 0], 1.0, np.eye(3), (2, 0, 2))
    # identity axes, a box of half (3, 2.5, 2) in 6 x 5 x 4 cells of half 0.5: every operation exact
    g = api.oriented_grid([1, 2, 3], [3, 2.5, 2], np.eye(3), (6, 5, 4))
    assert g.shape == (120,) and (g["half"] == 0.5).all() and (g["axes"] == np.eye(3, dtype=F)).all()
    want = np.stack(np.meshgrid(1 + np.arange(-2.5, 3), 2 + np.arange(-2.0, 2.5), 3 + np.arange(-1.5, 2), indexing="ij"), -1).reshape(-1, 3)
    assert (g["centre"] == want.astype(F)).all()
    # a turned box: the cells tile it (their corners reach the box's corners, neighbours are two half extents apart along an axis)
    quat = [0.3, -0.2, 0.5, 0.7]
    g = api.oriented_grid([1, 2, 3], [3, 2, 1], quat, (3, 2, 2))
    u = api.obb_axes(quat, 1)[0].astype(np.float64)
    cells = g["centre"].reshape(3, 2, 2, 3).astype(np.float64)
    assert np.allclose(cells[1, 0, 0] - cells[0, 0, 0], 2 * u[0], atol=1e-5) and np.allclose(cells[0, 1, 0] - cells[0, 0, 0], 2 * u[1], atol=1e-5)
    assert np.allclose(cells.reshape(-1, 3).mean(0), [1, 2, 3], atol=1e-5) and np.allclose(g["half"], [1, 1, 0.5])


def test_refusals_need_no_device(api):
    L = api.lib()
    buf = C.create_string_buffer(64)
    dummy = C.cast(buf, C.c_void_p)                                          # (what is refused is refused before the scene is looked at)
    count = C.cast(C.create_string_buffer(8), C.c_void_p)

    def ray_list(**kw):
        l = api.RayList()
        l.struct_size, l.flags, l.d_ids, l.d_count = C.sizeof(api.RayList), 0, None, count.value
        for k, v in kw.items():
            setattr(l, k, v)
        return l
    bad_lists = (ray_list(struct_size=8), ray_list(flags=1), ray_list(d_count=None))
    # count: scene, obbs, n, list, counts, stream
    for args in [(None, dummy, 4, None, dummy, None), (dummy, None, 4, None, dummy, None), (dummy, dummy, 4, None, None, None),
                 (dummy, dummy, 1 << 32, None, dummy, None), (dummy, dummy, 1 << 32, C.byref(ray_list()), dummy, None)] + \
                [(dummy, dummy, 4, C.byref(l), dummy, None) for l in bad_lists]:
        assert L.rtk_dev_triangles_in_obb_count(*args) == ERR_BAD_ARG, args
        assert "rtk_dev_triangles_in_obb_count:" in api.last_error()
    # fill: scene, obbs, n, list, offsets, prims, written, stream
    for args in [(None, dummy, 4, None, dummy, dummy, None, None), (dummy, None, 4, None, dummy, dummy, None, None),
                 (dummy, dummy, 4, None, None, dummy, None, None), (dummy, dummy, 4, None, dummy, None, dummy, None),
                 (dummy, dummy, 1 << 32, None, dummy, dummy, None, None)] + \
                [(dummy, dummy, 4, C.byref(l), dummy, dummy, None, None) for l in bad_lists]:
        assert L.rtk_dev_triangles_in_obb_all(*args) == ERR_BAD_ARG, args
        assert "rtk_dev_triangles_in_obb_all:" in api.last_error()
    # counted: scene, obbs, n, offsets, prims, counts or written, counters
    ctr = api.TraceCounters()
    for args in ((dummy, dummy, 4, None, None, dummy, None), (None, dummy, 4, None, None, dummy, C.byref(ctr)),
                 (dummy, None, 4, None, None, dummy, C.byref(ctr)), (dummy, dummy, 4, None, None, None, C.byref(ctr)),
                 (dummy, dummy, 4, dummy, None, None, C.byref(ctr)), (dummy, dummy, 1 << 32, None, None, dummy, C.byref(ctr))):
        assert L.rtk_dev_triangles_in_obb_counted(*args) == ERR_BAD_ARG, args
        assert "rtk_dev_triangles_in_obb_counted:" in api.last_error()
    # no queries: nothing to do, nothing launched
    assert L.rtk_dev_triangles_in_obb_count(dummy, None, 0, None, None, None) == 0
    assert L.rtk_dev_triangles_in_obb_count(dummy, dummy, 0, C.byref(ray_list()), dummy, None) == 0
    assert L.rtk_dev_triangles_in_obb_all(dummy, None, 0, None, None, None, None, None) == 0
    assert L.rtk_dev_triangles_in_obb_all(dummy, dummy, 0, C.byref(ray_list()), dummy, dummy, dummy, None) == 0
    ctr.rays = 7
    assert L.rtk_dev_triangles_in_obb_counted(dummy, None, 0, None, None, None, C.byref(ctr)) == 0 and ctr.rays == 0
