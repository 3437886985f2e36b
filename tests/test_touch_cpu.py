"""Triangles that touch a triangle without a GPU: the rule of rtk_amd/csrc/rtk_touch_rule.h, run by tests/touch_rule_driver.cpp
under the address and undefined-behaviour sanitizers, against numpy (tests/touch_ref.py): on integer inputs, where every float32
operation of the rule is exact, against the same seventeen axes in Python integers and against an independent exact answer (one
triangle clipped against the other's plane and three side half-spaces in fractions); on non-integer inputs bit for bit against
numpy, axis by axis; the skip against the candidates; the filter; a host walk of a small 4-wide tree in three child orders
against brute force; the parts of the interface that need no device -- header text, symbols, argtypes, the refusals decided
before any HIP call --; and what the query mix of the GPU tests holds."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from rtk_amd import synth
from tests.touch_ref import (SKIP_SHARED_VERTEX, MIX_PARTS, box_np, brute_force_touching, boxes_touch_np, candidate_np, live_np, mix_slices, query_mix,
                             separating_axes_np, shares_vertex_np, skip_np)
from tests.test_within_cpu import hexes, run_driver, small_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_BAD_ARG = -2
GUARD = 4                                     # entries on either side of the driver's segment
FILL = 0x7e7e7e7e


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """The driver built against the rule headers alone (no HIP include path, -Wall -Werror, no FMA contraction as in the
    library) with both sanitizers. -O2 and -mfma: a compiler that were allowed to contract would do it here."""
    exe = str(tmp_path_factory.mktemp("touch_rule") / "touch_rule_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-mfma", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "rtk_amd", "csrc"), os.path.join(ROOT, "tests", "touch_rule_driver.cpp"), "-o", exe])
    return exe


def run_bulk(exe, a, b, clo, chi, tmp_path, name, prim=None, first=None, flags=None):
    """a, b [N, 3, 3], clo, chi [N, 3] float32, prim / first / flags uint32 [N] or None (0) -> the driver's word per case,
    uint32 [N]: 1 live, 2 boxes touch, 4 skip, 8 the filter passes, bits 4 .. 20 the axes that separate"""
    n = len(a)
    words = np.zeros((n, 27), np.uint32)
    words[:, :24] = np.concatenate([a.reshape(n, 9), b.reshape(n, 9), clo, chi], 1).astype(np.float32).view(np.uint32)
    for k, x in enumerate((prim, first, flags)):
        if x is not None:
            words[:, 24 + k] = x
    path = str(tmp_path / (name + ".bin"))
    words.tofile(path)
    r = subprocess.run([exe, "-b", path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-200:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    assert lines[n] == "ok" and len(lines) == n + 2
    return np.array([int(x, 16) for x in lines[:n]], np.uint32)


def numpy_bits(a, b, clo, chi, prim=0, first=0, flags=0):
    alo, ahi = box_np(a)
    passes = (np.asarray(prim) >= np.asarray(first)) & ~((np.asarray(flags) & SKIP_SHARED_VERTEX != 0) & shares_vertex_np(a, b))
    bits = live_np(a) * 1 + boxes_touch_np(a, b) * 2 + skip_np(clo, chi, alo, ahi) * 4 + passes * 8
    return bits.astype(np.uint32) | separating_axes_np(a, b) << np.uint32(4)


def is_candidate(bits):
    return (bits & 0xb == 0xb) & (bits >> 4 == 0)


def enlarged(rng, v):
    """a box above each triangle: its own box, grown by nothing on some sides and by something on others"""
    with np.errstate(over="ignore", invalid="ignore"):
        grow = np.abs(v).max((1, 2))[:, None] * rng.choice([0.0, 0.0, 1e-6, 0.3], (len(v), 6)).astype(np.float32)
        return (v.min(1) - grow[:, :3]).astype(np.float32), (v.max(1) + grow[:, 3:]).astype(np.float32)


# ---------------------------------------------------------------------------------------------- integer inputs

KINDS = ("random", "coplanar", "shared vertex", "vertex on edge", "edge crosses edge", "A a point", "A a segment", "B a point",
         "B a segment", "identical", "both without area")


def integer_cases(seed=11, n=20000):
    """Pairs with integer coordinates in [-8, 8], of the kinds of KINDS: near each other so that they meet often; in one plane;
    with a common vertex; a vertex of B on the midpoint of an edge of A; an edge of each through one point; points and segments
    (two equal vertices, or three collinear ones) on either side and on both; the same triangle twice, vertices permuted."""
    rng = np.random.RandomState(seed)
    kind = rng.randint(0, len(KINDS), n)
    ca = rng.randint(-4, 5, (n, 1, 3))
    a = ca + rng.randint(-4, 5, (n, 3, 3))
    b = ca + rng.randint(-2, 3, (n, 1, 3)) + rng.randint(-4, 5, (n, 3, 3))
    k = kind == 1                                                   # one plane: one coordinate the same for all six vertices
    ax = rng.randint(0, 3, n)
    for x in range(3):
        m = k & (ax == x)
        a[m, :, x] = ca[m, :, x]; b[m, :, x] = ca[m, :, x]
    k = kind == 2                                                   # a common vertex
    rows = np.nonzero(k)[0]
    b[rows, rng.randint(0, 3, len(rows))] = a[rows, rng.randint(0, 3, len(rows))]
    k = kind == 3                                                   # b0 on the midpoint of A's edge 0
    d = rng.randint(-2, 3, (n, 3))
    a[k, 0] = np.clip(a[k, 0], -4, 4)                               # (so that nothing of the contact leaves [-8, 8])
    a[k, 1] = a[k, 0] + 2 * d[k]; b[k, 0] = a[k, 0] + d[k]
    k = kind == 4                                                   # A's edge 0 and B's edge 0 cross in p
    p, f = rng.randint(-4, 5, (n, 3)), rng.randint(-3, 4, (n, 3))
    d = rng.randint(-3, 4, (n, 3))
    a[k, 0] = p[k] - d[k]; a[k, 1] = p[k] + d[k]; b[k, 0] = p[k] - f[k]; b[k, 1] = p[k] + f[k]

    def flatten(v, m):
        """points, segments with two equal vertices, segments of three collinear vertices, a third each"""
        rows = np.nonzero(m)[0]
        how = rng.randint(0, 2, len(rows))
        v[rows[how == 0], 2] = v[rows[how == 0], 1]
        d = rng.randint(-2, 3, (len(rows), 3))
        r1 = rows[how == 1]
        v[r1, 1] = v[r1, 0] + d[how == 1]; v[r1, 2] = v[r1, 0] - 2 * d[how == 1]

    for v, pt, sg in ((a, 5, 6), (b, 7, 8)):
        k = kind == pt
        v[k, 1] = v[k, 0]; v[k, 2] = v[k, 0]
        flatten(v, kind == sg)
    # a point or a segment of A on B, half of the time: B's vertex, or the midpoint of B's doubled edge
    k = (kind == 5) & (rng.randint(0, 2, n) == 0)
    a[k] = b[k, 0:1]
    k = (kind == 7) & (rng.randint(0, 2, n) == 0)
    b[k] = a[k, 0:1]
    k = kind == 9
    rows = np.nonzero(k)[0]
    perm = np.array([[0, 1, 2], [1, 2, 0], [2, 1, 0]])[rng.randint(0, 3, len(rows))]
    b[rows] = a[rows[:, None], perm]
    k = kind == 10
    b[k] = a[k] + rng.randint(-1, 2, (n, 1, 3))[k]
    flatten(a, k); flatten(b, k)
    a, b = np.clip(a, -8, 8), np.clip(b, -8, 8)
    return a, b, kind


def cross_i(x, y):
    return [x[1] * y[2] - x[2] * y[1], x[2] * y[0] - x[0] * y[2], x[0] * y[1] - x[1] * y[0]]


def sub_i(x, y):
    return [x[0] - y[0], x[1] - y[1], x[2] - y[2]]


def dot_i(x, y):
    return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]


def sat17_integers(a, b, largest):
    """Rules 2 and 3 in Python integers -> (do the boxes touch, the axes that separate as a bit mask)"""
    a = [[int(x) for x in p] for p in a]
    b = [[int(x) for x in p] for p in b]
    touch = all(min(p[x] for p in b) <= max(p[x] for p in a) and max(p[x] for p in b) >= min(p[x] for p in a) for x in range(3))
    ea = [sub_i(a[1], a[0]), sub_i(a[2], a[1]), sub_i(a[0], a[2])]
    eb = [sub_i(b[1], b[0]), sub_i(b[2], b[1]), sub_i(b[0], b[2])]
    na, nb = cross_i(ea[0], ea[1]), cross_i(eb[0], eb[1])
    axes = [na, nb] + [cross_i(ea[i], eb[j]) for i in range(3) for j in range(3)] + [cross_i(na, e) for e in ea] + [cross_i(nb, e) for e in eb]
    da = [[0, 0, 0], sub_i(a[1], a[0]), sub_i(a[2], a[0])]
    db = [sub_i(p, a[0]) for p in b]
    bits = 0
    for k, m in enumerate(axes):
        pa, pb = [dot_i(m, d) for d in da], [dot_i(m, d) for d in db]
        largest[0] = max(largest[0], max(abs(x) for x in pa + pb + m))
        if min(pb) > max(pa) or max(pb) < min(pa):
            bits |= 1 << k
    return touch, bits


def clipped_is_not_empty(a, b):
    """a has area: b clipped against a's plane (both closed sides) and the three side half-spaces of a, in fractions: the two
    meet iff something is left"""
    a = [[int(x) for x in p] for p in a]
    poly = [[Fraction(int(x)) for x in p] for p in b]
    n = cross_i(sub_i(a[1], a[0]), sub_i(a[2], a[0]))
    planes = [(n, a[0]), ([-x for x in n], a[0])] + [(cross_i(n, sub_i(a[(i + 1) % 3], a[i])), a[i]) for i in range(3)]
    for m, at in planes:
        out = []
        for k in range(len(poly)):
            p, q = poly[k], poly[(k + 1) % len(poly)]
            dp, dq = dot_i(m, sub_i(p, at)), dot_i(m, sub_i(q, at))       # >= 0: inside
            if dp >= 0:
                out.append(p)
            if (dp > 0 and dq < 0) or (dp < 0 and dq > 0):
                t = dp / (dp - dq)
                out.append([p[i] + t * (q[i] - p[i]) for i in range(3)])
        poly = out
        if not poly:
            return False
    return True


def hull_of_collinear(v):
    """three collinear integer points -> the two ends of their segment (equal for a point)"""
    v = [[int(x) for x in p] for p in v]
    pairs = [(v[0], v[1]), (v[1], v[2]), (v[2], v[0])]
    return max(pairs, key=lambda pq: dot_i(sub_i(pq[1], pq[0]), sub_i(pq[1], pq[0])))


def segments_meet(a, b):
    """two closed segments (or points) with integer ends, exactly"""
    (p, q), (r, s) = hull_of_collinear(a), hull_of_collinear(b)
    d1, d2, w = sub_i(q, p), sub_i(s, r), sub_i(r, p)
    n = cross_i(d1, d2)
    nn = dot_i(n, n)
    if nn:
        if dot_i(w, n):
            return False
        t, u = dot_i(cross_i(w, d2), n), dot_i(cross_i(w, d1), n)       # times nn
        return 0 <= t <= nn and 0 <= u <= nn
    d = d1 if any(d1) else d2
    if not any(d):
        return p == r
    if any(cross_i(w, d)):
        return False
    i1, i2 = sorted((dot_i(p, d), dot_i(q, d))), sorted((dot_i(r, d), dot_i(s, d)))
    return i1[0] <= i2[1] and i2[0] <= i1[1]


def has_area(v):
    v = [[int(x) for x in p] for p in v]
    return any(cross_i(sub_i(v[1], v[0]), sub_i(v[2], v[0])))


def exact_meet(a, b):
    if has_area(a):
        return clipped_is_not_empty(a, b)
    if has_area(b):
        return clipped_is_not_empty(b, a)
    return segments_meet(a, b)


def test_integer_inputs_equal_the_exact_answers(driver, tmp_path):
    a, b, kind = integer_cases()
    n = len(a)
    af, bf = a.astype(np.float32), b.astype(np.float32)
    clo, chi = enlarged(np.random.RandomState(1), bf)
    got = run_bulk(driver, af, bf, clo, chi, tmp_path, "integers")
    ref = numpy_bits(af, bf, clo, chi)
    assert (got == ref).all(), np.nonzero(got != ref)[0][:10]
    assert (got & 1).all() and (got & 8).all()
    # the same seventeen axes in Python integers, axis by axis
    largest = [0]
    for i in range(n):
        touch, bits = sat17_integers(a[i], b[i], largest)
        assert touch == bool(got[i] & 2), (i, a[i], b[i])
        assert int(got[i]) >> 4 == bits, (i, a[i], b[i], hex(int(got[i]) >> 4), hex(bits))
    print("largest intermediate %d" % largest[0])
    assert largest[0] < 2 ** 24                                      # every float32 operation of the rule was exact
    cand = is_candidate(got)
    exact = np.array([exact_meet(a[i], b[i]) for i in range(n)])
    proper = np.array([has_area(a[i]) and has_area(b[i]) for i in range(n)])
    bad = np.nonzero(proper & (cand != exact))[0]
    assert len(bad) == 0, (len(bad), a[bad[:3]], b[bad[:3]])
    bad = np.nonzero(~proper & exact & ~cand)[0]                     # without area: never drops a pair that meets
    assert len(bad) == 0, (len(bad), a[bad[:3]], b[bad[:3]])
    print("integer pairs %d: candidates %d, exact %d, both with area %d, kept though apart %d" % (n, cand.sum(), exact.sum(), proper.sum(), (cand & ~exact).sum()))
    assert exact.sum() >= n // 5 and (~exact).sum() >= n // 5
    assert (cand & ~exact).sum() > 0                                 # (the superset is a proper one: the header's segment beside B)
    for k, name in enumerate(KINDS):
        part = kind == k
        assert part.sum() > n // 20, name
        assert (cand[part]).any() and (name in ("shared vertex", "vertex on edge", "edge crosses edge", "identical") or (~cand[part]).any()), name
    # each constructed contact is a contact and is kept (clipping to [-8, 8] moves none of them: their ranges stay inside)
    for name in ("shared vertex", "vertex on edge", "edge crosses edge", "identical"):
        part = kind == KINDS.index(name)
        assert exact[part].all() and cand[part].all(), name
    copl = kind == KINDS.index("coplanar")
    assert (proper & copl & cand).sum() > 100 and (proper & copl & ~cand).sum() > 100
    # coplanar pairs that only the six in-plane axes tell apart
    assert (((got[copl] >> 4) != 0) & ((got[copl] >> 4) & 0x7ff == 0)).any()
    # rule 6 never skips a box above a candidate
    assert not ((got & 4 != 0) & cand).any() and (got & 4 != 0).sum() > 0.05 * n


# ---------------------------------------------------------------------------------------------- non-integer inputs

PER = 30000                                   # cases per kind of the non-integer inputs


def float_cases(seed=3, per=PER):
    rng = np.random.RandomState(seed)
    As, Bs = [], []
    # four pairs of (size of A, size of B); a point of B lies near a point of A, so that the two meet often but not always
    for sa, sb in ((1.0, 1.0), (1.0, 0.05), (0.05, 1.0), (1e3, 1e-3)):
        centre = rng.uniform(-1, 1, (per, 1, 3)) * max(sa, sb)
        a = centre + rng.uniform(-sa, sa, (per, 3, 3))
        bary = rng.dirichlet([1, 1, 1], per)
        mid = (a * bary[:, :, None]).sum(1) + rng.uniform(-0.5, 0.5, (per, 3)) * min(sa, sb)
        b = rng.uniform(-sb, sb, (per, 3, 3))
        As.append(a); Bs.append(mid[:, None, :] + b - (b * rng.dirichlet([1, 1, 1], per)[:, :, None]).sum(1)[:, None, :])
    # near-coplanar pairs: B in A's plane but for a few ulps, overlapping or beside it
    a = rng.uniform(-1, 1, (per, 3, 3))
    wts = rng.uniform(-0.6, 1.2, (per, 3, 3))
    wts /= wts.sum(2, keepdims=True)
    b = np.einsum("nij,njk->nik", wts, a) + rng.choice([0.0, 1e-7, 1e-5], (per, 1, 1)) * rng.uniform(-1, 1, (per, 3, 3))
    As.append(a); Bs.append(b)
    # one float32 step either side of a contact: a vertex of B on a vertex of A, on an edge's midpoint, inside the face; then
    # that vertex moved by one step on one axis, up or down
    a = rng.uniform(-1, 1, (per, 3, 3)).astype(np.float32)
    where = rng.randint(0, 3, per)
    w = np.where(where[:, None] == 0, [1.0, 0.0, 0.0], np.where(where[:, None] == 1, [0.5, 0.5, 0.0], [0.25, 0.25, 0.5]))
    on = (a.astype(np.float64) * w[:, :, None]).sum(1).astype(np.float32)
    step = rng.randint(-1, 2, per)
    axis = rng.randint(0, 3, per)
    moved = on.copy()
    rows = np.arange(per)
    moved[rows, axis] = np.where(step == 0, on[rows, axis], np.nextafter(on[rows, axis], np.where(step > 0, np.inf, -np.inf).astype(np.float32)))
    b = np.concatenate([moved[:, None, :], moved[:, None, :] + rng.uniform(-1, 1, (per, 2, 3)).astype(np.float32)], 1)
    As.append(a); Bs.append(b)
    # slivers and exactly degenerate triangles on either side
    p, q = rng.uniform(-1, 1, (per, 3)), rng.uniform(-1, 1, (per, 3))
    t = rng.uniform(-0.5, 1.5, (per, 1))
    c = p + t * (q - p) + rng.choice([0.0, 1e-7, 1e-5], (per, 1)) * rng.uniform(-1, 1, (per, 3))
    thin = np.stack([p, q, c], 1)
    other = (p + rng.uniform(0, 1, (per, 1)) * (q - p))[:, None, :] + rng.uniform(-0.3, 0.3, (per, 3, 3))
    swap = rng.randint(0, 2, per).astype(bool)[:, None, None]
    As.append(np.where(swap, thin, other)); Bs.append(np.where(swap, other, thin))
    # denormals: everything within a few thousand ulps of zero
    tiny = np.float32(1e-45).astype(np.float64)
    As.append(rng.randint(-3000, 3000, (per // 2, 3, 3)) * tiny); Bs.append(rng.randint(-3000, 3000, (per // 2, 3, 3)) * tiny)
    # huge: products that overflow, infinities times zeros; queries and records with NaN and infinite members
    m = per // 2
    a = rng.uniform(-1, 1, (m, 3, 3)) * rng.choice([1.0, 1e15, 1e30, 3e38], (m, 1, 1))
    b = rng.uniform(-1, 1, (m, 3, 3)) * rng.choice([1.0, 1e15, 1e30, 3e38], (m, 1, 1))
    for v in (a, b):
        bad = np.nonzero(rng.randint(0, 8, m) == 0)[0]
        v.reshape(m, 9)[bad, rng.randint(0, 9, len(bad))] = rng.choice([np.nan, np.inf, -np.inf], len(bad))
    As.append(a); Bs.append(b)
    with np.errstate(over="ignore"):
        return np.concatenate(As).astype(np.float32), np.concatenate(Bs).astype(np.float32)


def test_non_integer_inputs_equal_numpy_bit_for_bit(driver, tmp_path):
    a, b = float_cases()
    n = len(a)
    assert n >= 200000
    clo, chi = enlarged(np.random.RandomState(2), b)
    rng = np.random.RandomState(4)
    prim, first, flags = rng.randint(0, 50, n), rng.randint(0, 50, n) * rng.randint(0, 2, n), rng.randint(0, 2, n)
    got = run_bulk(driver, a, b, clo, chi, tmp_path, "floats", prim, first, flags)
    ref = numpy_bits(a, b, clo, chi, prim, first, flags)
    bad = np.nonzero(got != ref)[0]
    assert len(bad) == 0, (len(bad), bad[:5], [hex(x) for x in got[bad[:5]]], [hex(x) for x in ref[bad[:5]]], a[bad[:2]], b[bad[:2]])
    cand = is_candidate(got | 8)                                     # (the rule without the filter)
    assert (is_candidate(got) == candidate_np(a, b, prim, first, 1) | (is_candidate(got) & (flags == 0))).all()
    names = ("1 / 1", "1 / 0.05", "0.05 / 1", "1e3 / 1e-3", "near-coplanar", "a step off a contact", "slivers")
    for k, name in enumerate(names):
        part = slice(k * PER, (k + 1) * PER)
        print("%-22s candidates %5.1f %%, separated behind touching boxes %5.1f %%" % (name, 100 * cand[part].mean(), 100 * ((got[part] & 2 != 0) & (got[part] >> 4 != 0)).mean()))
        assert 0.02 < cand[part].mean() < 0.98, name
    # every axis decided somewhere, and alone somewhere in the near-coplanar and stepped parts put together
    axes = got >> 4
    for k in range(17):
        assert (axes >> k & 1).sum() > 100, k
    # a step either side of a contact changes the answer in both directions
    part = slice(5 * PER, 6 * PER)
    assert cand[part].any() and (~cand[part]).any()
    # queries that are not live occurred, and so did NaN projections (an infinity times a zero, inf - inf) that separate nothing
    assert ((got & 1) == 0).sum() > 500
    huge = slice(n - PER // 2, n)
    assert ((got[huge] & 1 != 0) & (axes[huge] == 0)).any()
    # rule 6 never skips a box above a candidate
    assert not ((got & 4 != 0) & cand).any() and (got & 4 != 0).sum() > 0.05 * n


# ---------------------------------------------------------------------------------------------- the filter

def test_the_filter(driver, tmp_path):
    """first_prim at, below and above a candidate's id; skip_shared with +0 / -0 and with NaN coordinates"""
    a = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], np.float32)
    through = np.array([[1, 1, -1], [1, 1, 1], [2, 1, 1]], np.float32)           # pierces a, shares nothing
    shares = np.array([[0, 0, 0], [1, 1, 1], [2, 1, 1]], np.float32)             # vertex 0 is a's vertex 0
    minus = shares.copy(); minus[0] = [-0.0, 0.0, -0.0]                          # the same vertex with other zero signs
    near = shares.copy(); near[0, 0] = np.nextafter(np.float32(0), np.float32(1))
    nan_b = shares.copy(); nan_b[0, 1] = np.nan                                  # a NaN equals nothing
    a_nan = a.copy(); a_nan[0, 0] = np.nan
    b_same_nan = a_nan.copy()
    cases = [  # (A, B, prim, first, flags, passes)
        (a, through, 7, 7, 0, True), (a, through, 7, 6, 0, True), (a, through, 7, 8, 0, False), (a, through, 7, 0, 0, True),
        (a, through, 0xfffffffe, 0xffffffff, 0, False), (a, through, 0xffffffff, 0xffffffff, 0, True),
        (a, through, 7, 7, 1, True), (a, through, 7, 8, 1, False),
        (a, shares, 7, 0, 0, True), (a, shares, 7, 0, 1, False), (a, minus, 7, 0, 1, False), (a, near, 7, 0, 1, True),
        (a, nan_b, 7, 0, 1, True), (a, a, 7, 0, 1, False), (a, a[::-1].copy(), 7, 0, 1, False), (a, a, 7, 0, 0, True),
        (a_nan, b_same_nan, 7, 0, 1, False),      # (vertices 1 and 2 still equal)
        (a_nan, shares, 7, 0, 1, True),           # (the NaN vertex is the shared one: it equals nothing)
    ]
    A = np.stack([c[0] for c in cases]); B = np.stack([c[1] for c in cases])
    prim, first, flags = (np.array([c[k] for c in cases], np.uint32) for k in (2, 3, 4))
    clo, chi = enlarged(np.random.RandomState(0), np.nan_to_num(B))
    got = run_bulk(driver, A, B, clo, chi, tmp_path, "filter", prim, first, flags)
    assert ((got & 8 != 0) == np.array([c[5] for c in cases])).all(), got & 8
    assert (got == numpy_bits(A, B, clo, chi, prim, first, flags)).all()
    # the pairs do meet: what the filter passes is a candidate
    cand = is_candidate(got)
    assert cand[[0, 1, 3, 6, 8, 15]].all() and not cand[[2, 7, 9, 10, 13]].any()


# ---------------------------------------------------------------------------------------------- the walk

def split_segment(words, room):
    """the driver's dump -> the segment's words [room]; the guards must be untouched"""
    w = np.array([int(x, 16) for x in words], np.uint32)
    assert len(w) == GUARD + room + GUARD
    assert (w[:GUARD] == FILL).all() and (w[GUARD + room:] == FILL).all(), "a guard was written"
    return w[GUARD:GUARD + room]


def walk_queries(rng, tris):
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    ext = hi - lo
    q = [rng.uniform(lo, hi, (50, 1, 3)) + rng.choice([0.05, 0.2, 0.6], (50, 1, 1)) * rng.uniform(-1, 1, (50, 3, 3))]
    q.append(tris[rng.permutation(len(tris))[:20]])                                   # the scene's own
    verts = tris[rng.permutation(len(tris))[:10], 1]
    q.append(np.repeat(verts[:, None, :], 3, 1))                                      # points at vertices
    q.append(np.stack([np.stack([lo - ext, hi + ext, hi + ext]), np.stack([lo - 1e30, hi + 1e30, hi + 1e30])]))   # segments through everything
    q.append(np.stack([np.stack([hi + ext, hi + 2 * ext, hi + 3 * ext]), np.stack([lo, hi, hi * np.float32(np.nan)]), np.stack([lo, hi * np.float32(np.inf), hi])]))
    q = np.concatenate(q).astype(np.float32)
    room = rng.randint(0, 7, len(q))
    room[::7] = len(tris)                                            # room for the whole list
    first = rng.randint(0, len(tris), len(q)) * (rng.randint(0, 3, len(q)) == 0)
    flags = rng.randint(0, 2, len(q))
    return q, room, first.astype(np.uint32), flags.astype(np.uint32)


def test_host_walk_equals_brute_force_in_every_order(driver, tmp_path):
    """A soup under a random 4-wide tree, leaves of 1 to 5: count and kept prefix equal brute force bit for bit whichever way the
    children are visited, with and without the filter"""
    rng = np.random.RandomState(5)
    tris = (rng.uniform(0, 1, (90, 1, 3)) + rng.uniform(-0.08, 0.08, (90, 3, 3))).astype(np.float32)
    nodes, recs = small_tree(rng, tris, 5)
    assert len(nodes) > 8
    q, room, first, flags = walk_queries(rng, tris)
    counts, kept = [], []
    for fl in (0, 1):
        ref = brute_force_touching(tris, np.arange(len(tris)), q, first, fl, room)
        counts.append(ref.counts); kept.append(ref.kept)
    counts = np.where(flags == 1, counts[1], counts[0])
    kept = [kept[int(flags[i])][i] for i in range(len(q))]
    assert (counts == 0).any() and (counts > 6).any() and (counts > 80).any() and (counts[-3:] == 0).all()
    assert (counts[50:70][(flags[50:70] == 0) & (first[50:70] == 0)] >= 1).all()          # a triangle of the scene meets itself
    text = "n %d %s\nt %d %s\n" % (len(nodes), hexes(nodes), len(recs), hexes(recs))
    qwords = np.concatenate([q.reshape(-1, 9).view(np.uint32), room.astype(np.uint32)[:, None], first[:, None], flags[:, None]], 1)
    for order in (0, 1, 2):
        out = run_driver(driver, text + "".join("q %d %s\n" % (order, hexes(w)) for w in qwords), len(qwords), tmp_path, "walk_%d" % order)
        for i, line in enumerate(out):
            want = kept[i]
            seg = split_segment(line[2:], int(room[i]))
            assert int(line[0]) == counts[i], (order, i)
            assert int(line[1]) == len(want), (order, i)
            assert seg[:len(want)].tobytes() == want.tobytes(), (order, i)
            assert (seg[len(want):] == FILL).all(), (order, i)
    # a scene without triangles: no candidates
    out = run_driver(driver, "n 0\nt 0\nq 0 %s\n" % hexes(qwords[0]), 1, tmp_path, "empty")
    assert out[0][:2] == ["0", "0"]


# ---------------------------------------------------------------------------------------------- the interface

def test_rule_header_includes_no_hip_and_states_its_rules():
    text = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_touch_rule.h")).read()
    assert [l.split()[1] for l in text.splitlines() if l.startswith("#include")] == ['"rtk_box_rule.h"']
    assert "hip_runtime" not in text and "__global__" not in text and "fmaf" not in text
    assert "rtk_box_insert(" not in text.split("#pragma once")[1] and "rtk_box_skip(" not in text.split("#pragma once")[1]      # (used, not copied)
    text = " ".join(text.replace("\n//", "\n").split())              # (the comment's line breaks and slashes taken out)
    for word in ("1. LIVE", "2. BOXES", "3. SEVENTEEN AXES", "4. CANDIDATE", "5. FILTER", "6. SKIP", "7. INSERT", "CLOSED", "FLOAT RULE", "DEFINED BY IT",
                 "Touching counts", "NEVER LOSES A PAIR THAT MEETS", "THE EXACT ANSWER", "ZERO AREA", "NON-FINITE", "NOTHING ELSE IS PROMISED",
                 "NEVER SEPARATES", "WITHOUT A MARGIN", "ASCENDING PRIMITIVE ID", "always evaluated"):
        assert word in text, word
    for name in ("rtk_box_rule.h", "rtk_closest_rule.h"):
        assert "rtk_touch" not in open(os.path.join(ROOT, "rtk_amd", "csrc", name)).read()      # (used as they are, not changed)
    header = open(os.path.join(ROOT, "include", "rtk_amd.h")).read()
    section = header[header.index("/* ---- Triangles that touch a triangle"):header.index("/* ---- Every hit along a ray")]
    section = " ".join(section.replace("\n *", "\n").split())
    for word in ("rtk_touch_rule.h", "ARE NOT WRITTEN", "A SLOT THAT IS NOT LISTED IS NOT WRITTEN", "d_offsets[i] = i * k", "DETERMINISTIC", "NOTHING ELSE IS PROMISED",
                 "rtk_dev_trace_status", "rtk_mgpu_scene(m, i)", "CANNOT BE CULLED BY WHAT IT HAS KEPT", "ASCENDING PRIMITIVE ID", "touching counts",
                 "SEVENTEEN AXES", "indexed by query slot", "RTK_TOUCH_SKIP_SHARED_VERTEX", "unknown bit"):
        assert word in section, word
    mk = open(os.path.join(ROOT, "rtk_amd", "csrc", "Makefile")).read()
    assert "rtk_touch_rule.h" in mk and "rtk_touch.hip" in mk and "rtk_overlap_walk.h" in mk
    # the shape's own calls in its file, what the three overlap shapes share in the walk
    kernel = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_touch.hip")).read()
    walk = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_overlap_walk.h")).read()
    assert "rtk_box_insert(" in walk and "rtk_box_skip(" in kernel and "rtk_touch_candidate(" in kernel and "rtk_touch_live(" in kernel
    assert "kernel-resource-usage" in kernel and "scratch 0" in kernel and "LaunchScratch" in walk


def test_header_symbols_and_argtypes(api):
    from rtk_amd import types
    text = open(os.path.join(ROOT, "include", "rtk_amd.h")).read()
    for word in ("typedef struct rtk_tri_query { float v0[3], v1[3], v2[3]; } rtk_tri_query;",
                 "enum { RTK_TOUCH_SKIP_SHARED_VERTEX = 1u };",
                 "typedef struct rtk_touch_filter { uint32_t struct_size; uint32_t flags; const uint32_t *d_first_prim;",
                 "int rtk_dev_triangles_touching_count(const rtk_dev_scene *ds, const rtk_tri_query *d_tris, size_t num_queries,",
                 "int rtk_dev_triangles_touching_all(const rtk_dev_scene *ds, const rtk_tri_query *d_tris, size_t num_queries,",
                 "int rtk_dev_triangles_touching_counted(const rtk_dev_scene *ds, const rtk_tri_query *d_tris, size_t num_queries,",
                 "uint32_t rtk_amd_touch_stack_entries(void);"):
        assert word in text, word
    assert text.index("/* ---- Triangles that touch a box") < text.index("/* ---- Triangles that touch a triangle") < text.index("/* ---- Every hit along a ray")
    assert types.TRI_QUERY_DTYPE.itemsize == 36 and types.TRI_QUERY_DTYPE.names == ("v0", "v1", "v2") and types.TRI_QUERY_DTYPE.fields["v2"][1] == 24
    assert C.sizeof(api.TouchFilter) == 16 and api.TouchFilter.d_first_prim.offset == 8 and api.TOUCH_SKIP_SHARED_VERTEX == 1
    L = api.lib()
    for name in ("rtk_dev_triangles_touching_count", "rtk_dev_triangles_touching_all", "rtk_dev_triangles_touching_counted", "rtk_amd_touch_stack_entries"):
        assert name in api.RTK_AMD_H_SYMBOLS and hasattr(L, name), name
    F = C.POINTER(api.TouchFilter)
    assert L.rtk_dev_triangles_touching_count.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(api.RayList), F, C.c_void_p, C.c_void_p]
    assert L.rtk_dev_triangles_touching_all.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(api.RayList), F, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert L.rtk_dev_triangles_touching_counted.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, F, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(api.TraceCounters)]
    assert L.rtk_dev_triangles_touching_count.restype == C.c_int and L.rtk_dev_triangles_touching_all.restype == C.c_int
    assert L.rtk_dev_triangles_touching_counted.restype == C.c_int
    assert L.rtk_amd_touch_stack_entries.restype == C.c_uint32 and 1 <= L.rtk_amd_touch_stack_entries() <= 64
    for name in ("count_touching_device", "touching_all_device", "triangles_touching_counted", "triangles_touching", "triangles", "intersections",
                 "self_intersections"):
        assert callable(getattr(api.DeviceScene, name)), name


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

    def touch_filter(**kw):
        f = api.TouchFilter()
        f.struct_size, f.flags, f.d_first_prim = C.sizeof(api.TouchFilter), 0, None
        for k, v in kw.items():
            setattr(f, k, v)
        return f
    bad_lists = (ray_list(struct_size=8), ray_list(flags=1), ray_list(d_count=None))
    bad_filters = (touch_filter(struct_size=8), touch_filter(struct_size=0), touch_filter(flags=2), touch_filter(flags=0x80000001))
    good = C.byref(touch_filter(flags=1))
    # count: scene, triangles, n, list, filter, counts, stream
    for args in [(None, dummy, 4, None, None, dummy, None), (dummy, None, 4, None, None, dummy, None), (dummy, dummy, 4, None, good, None, None),
                 (dummy, dummy, 1 << 32, None, None, dummy, None), (dummy, dummy, 1 << 32, C.byref(ray_list()), good, dummy, None)] + \
                [(dummy, dummy, 4, C.byref(l), None, dummy, None) for l in bad_lists] + [(dummy, dummy, 4, None, C.byref(f), dummy, None) for f in bad_filters]:
        assert L.rtk_dev_triangles_touching_count(*args) == ERR_BAD_ARG, args
        assert "rtk_dev_triangles_touching_count:" in api.last_error()
    # fill: scene, triangles, n, list, filter, offsets, prims, written, stream
    for args in [(None, dummy, 4, None, None, dummy, dummy, None, None), (dummy, None, 4, None, None, dummy, dummy, None, None),
                 (dummy, dummy, 4, None, good, None, dummy, None, None), (dummy, dummy, 4, None, None, dummy, None, dummy, None),
                 (dummy, dummy, 1 << 32, None, None, dummy, dummy, None, None)] + \
                [(dummy, dummy, 4, C.byref(l), None, dummy, dummy, None, None) for l in bad_lists] + \
                [(dummy, dummy, 4, None, C.byref(f), dummy, dummy, None, None) for f in bad_filters]:
        assert L.rtk_dev_triangles_touching_all(*args) == ERR_BAD_ARG, args
        assert "rtk_dev_triangles_touching_all:" in api.last_error()
    # counted: scene, triangles, n, filter, offsets, prims, counts or written, counters
    ctr = api.TraceCounters()
    for args in [(dummy, dummy, 4, None, None, None, dummy, None), (None, dummy, 4, None, None, None, dummy, C.byref(ctr)),
                 (dummy, None, 4, None, None, None, dummy, C.byref(ctr)), (dummy, dummy, 4, good, None, None, None, C.byref(ctr)),
                 (dummy, dummy, 4, None, dummy, None, None, C.byref(ctr)), (dummy, dummy, 1 << 32, None, None, None, dummy, C.byref(ctr))] + \
                [(dummy, dummy, 4, C.byref(f), None, None, dummy, C.byref(ctr)) for f in bad_filters]:
        assert L.rtk_dev_triangles_touching_counted(*args) == ERR_BAD_ARG, args
        assert "rtk_dev_triangles_touching_counted:" in api.last_error()
    # no queries: nothing to do, nothing launched
    assert L.rtk_dev_triangles_touching_count(dummy, None, 0, None, None, None, None) == 0
    assert L.rtk_dev_triangles_touching_count(dummy, dummy, 0, C.byref(ray_list()), good, dummy, None) == 0
    assert L.rtk_dev_triangles_touching_all(dummy, None, 0, None, None, None, None, None, None) == 0
    assert L.rtk_dev_triangles_touching_all(dummy, dummy, 0, C.byref(ray_list()), good, dummy, dummy, dummy, None) == 0
    ctr.rays = 7
    assert L.rtk_dev_triangles_touching_counted(dummy, None, 0, None, None, None, None, C.byref(ctr)) == 0 and ctr.rays == 0


# ---------------------------------------------------------------------------------------------- the reference mix

def test_the_reference_has_empty_short_and_long_lists():
    """The query mix of tests/test_gpu_touch.py on its 300-triangle soup, through tests/touch_ref.py alone"""
    tris = synth.triangle_soup(300, 0.2, seed=5).reshape(300, 3, 3)
    q = query_mix(tris)
    n = len(q)
    assert 1200 <= n <= 1400 and n * 300 <= 500000 and n == sum(m for _, m in MIX_PARTS)
    ref = brute_force_touching(tris, np.arange(300), q)
    c = ref.counts
    print("queries %d, pairs %d, mean count %.2f, max %d, empty %.0f %%" % (n, int(c.sum()), c.mean(), c.max(), 100 * (c == 0).mean()))
    assert (c == 0).any() and (c == 1).any() and ((c > 1) & (c < 8)).any() and (c > 64).any() and (c == 300).sum() >= 1
    part = mix_slices()
    assert (c[part["scene scale"]] > 0).any() and (c[part["scene scale"]] == 0).any()
    assert (c[part["the scene's own"]] >= 1).all()                   # a triangle meets itself
    for i in range(300):
        assert i in ref.lists[part["the scene's own"].start + i]
    on = c[part["vertex on a vertex"]].reshape(3, 40)                # [a step below, on, a step above]
    assert (on[1] >= 1).all() and ((on[0] < on[1]) | (on[2] < on[1])).any()
    shifted = c[part["coplanar copies"]].reshape(3, 40)
    # (the copy itself always meets its source; shifted by half an edge it overlaps in exact arithmetic, but its vertices are
    # rounded off the plane and the float rule decides: most stay; shifted by three edges it is beside its source)
    assert (shifted[0] >= 1).all() and (shifted[1] >= 1).mean() > 0.8 and shifted[2].sum() < shifted[0].sum()
    assert (c[part["points"]][:40] >= 1).all()                       # a point on a vertex touches that triangle
    assert (c[part["segments"]] > 0).any()
    assert (c[part["huge and degenerate on purpose"]] == 300).any()
    assert (c[part["far away"]] == 0).all() and (c[part["not live"]] == 0).all()
    assert not live_np(q[part["not live"]]).any() and live_np(q[:part["not live"].start]).all()
