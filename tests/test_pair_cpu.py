"""Closest triangles without a GPU: the rule of rtk_amd/csrc/rtk_pair_rule.h, run by tests/pair_rule_driver.cpp under the address
and undefined-behaviour sanitizers, against numpy (tests/pair_ref.py): non-integer pairs bit for bit -- dist2, u, v, both points,
the winning feature, the piercing decision --; small integer pairs against an exact reference in fractions; the accuracy
statement against the same walk in float64; a host walk of a small 4-wide tree in four child orders against brute force; the
bound against the distance of everything inside a box; and the parts of the interface that need no device -- header text,
symbols, argtypes, the refusals decided before any HIP call."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from rtk_amd.types import RTK_INF
from tests.pair_ref import FEATURE_NONE, FEATURE_PIERCE, box_bound_np, brute_force_pairs, pair_np
from tests.test_touch_cpu import cross_i, dot_i, exact_meet, hull_of_collinear, integer_cases, sub_i
from tests.test_within_cpu import hexes, run_driver, small_tree
from tests.touch_ref import box_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_BAD_ARG = -2
NONE = 0xFFFFFFFF
# rtk_pair_rule.h's accuracy statement: measured over 8 million pairs (scripts/pair_accuracy.py), and what is asserted: about
# 2.5 times that, the margin rtk_closest_rule.h gives itself, because the sample is random and not worst case
ACCURACY_MEASURED = 1.47
ACCURACY_ASSERTED = 3.7


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """The driver built against the rule headers alone (no HIP include path, -Wall -Werror, no FMA contraction as in the
    library) with both sanitizers. -O2 and -mfma: a compiler that were allowed to contract would do it here."""
    exe = str(tmp_path_factory.mktemp("pair_rule") / "pair_rule_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-mfma", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "rtk_amd", "csrc"), os.path.join(ROOT, "tests", "pair_rule_driver.cpp"), "-o", exe])
    return exe


def run_bulk(exe, a, b, lo, hi, tmp_path, name):
    """a, b [N, 3, 3], lo, hi [N, 3] float32 -> (words uint32 [N, 10]: dist2 u v qa[3] qb[3] bound, feature [N], live [N])"""
    n = len(a)
    words = np.concatenate([a.reshape(n, 9), b.reshape(n, 9), lo, hi], 1).astype(np.float32).view(np.uint32)
    path = str(tmp_path / (name + ".bin"))
    words.tofile(path)
    r = subprocess.run([exe, "-b", path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-200:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    assert lines[n] == "ok" and len(lines) == n + 2
    rows = [l.split() for l in lines[:n]]
    return (np.array([[int(x, 16) for x in row[:10]] for row in rows], np.uint32), np.array([int(row[10]) for row in rows]),
            np.array([int(row[11]) for row in rows]))


def numpy_words(a, b, lo, hi):
    r = pair_np(a, b)
    alo, ahi = box_np(a)
    bound = box_bound_np(lo, hi, alo, ahi)
    return np.concatenate([r.dist2[:, None], r.u[:, None], r.v[:, None], r.qa, r.qb, bound[:, None]], 1), r


def same_words(got, want, what):
    """Bit for bit, except where the expected value is NaN: there only "it is NaN" is promised."""
    want = np.ascontiguousarray(want, np.float32)
    nan = np.isnan(want)
    assert (np.isnan(got.view(np.float32)) == nan).all(), what
    bad = (got != want.view(np.uint32)) & ~nan
    assert not bad.any(), (what, np.argwhere(bad)[:5], got[bad][:5], want.view(np.uint32)[bad][:5])


def enlarged(rng, v):
    """a box above each triangle: its own box, grown by nothing on some sides and by something on others"""
    lo, hi = box_np(v)
    with np.errstate(over="ignore", invalid="ignore"):
        grow = np.abs(v).max((1, 2))[:, None] * rng.choice([0.0, 0.0, 1e-6, 0.3, 2.0], (len(v), 6)).astype(np.float32)
        return (lo - grow[:, :3]).astype(np.float32), (hi + grow[:, 3:]).astype(np.float32)


# ---------------------------------------------------------------------------------------------- non-integer inputs

PER = 12000
FAMILIES = ("near", "far", "small against large", "parallel edges", "shared vertex", "shared edge", "A a segment", "A a point", "B a segment",
            "B a point", "both without area", "through each other", "coplanar", "denormal", "huge and non-finite")


def float_cases(seed=3, per=PER):
    rng = np.random.RandomState(seed)
    As, Bs = [], []

    def add(a, b):
        with np.errstate(over="ignore"):
            As.append(np.asarray(a, np.float64).astype(np.float32)); Bs.append(np.asarray(b, np.float64).astype(np.float32))

    def tri(scale=1.0, n=per):
        return rng.uniform(-1, 1, (n, 3, 3)) * scale
    add(tri(), tri() + rng.uniform(-1.5, 1.5, (per, 1, 3)))                                                   # near
    add(tri(), tri() + 20 * rng.choice([-1.0, 1.0], (per, 1, 3)) * rng.uniform(1, 2, (per, 1, 3)))             # far
    add(tri(), tri(0.03) + rng.uniform(-1, 1, (per, 1, 3)))                                                   # small against large
    a = tri()                                                                                                 # parallel edges
    b = tri() + rng.uniform(-1, 1, (per, 1, 3))
    f = rng.choice([1.0, -1.0, 0.5, 2.0, 0.3], (per, 1))
    b[:, 1] = b[:, 0] + f * (a[:, 1] - a[:, 0])
    add(a, b)
    a, b = tri().astype(np.float32), tri().astype(np.float32)                                                 # shared vertex
    rows = np.arange(per)
    b[rows, rng.randint(0, 3, per)] = a[rows, rng.randint(0, 3, per)]
    add(a, b)
    a, b = tri().astype(np.float32), tri().astype(np.float32)                                                 # shared edge
    b[:, 0] = a[:, 1]; b[:, 1] = a[:, 0]
    add(a, b)

    def flat(v, kind):
        """kind 0: two equal vertices; 1: three collinear ones; 2: a point"""
        v = v.copy()
        k0, k1, k2 = kind == 0, kind == 1, kind == 2
        v[k0, 2] = v[k0, 1]
        v[k1, 2] = v[k1, 0] + rng.uniform(-0.5, 1.5, (k1.sum(), 1)) * (v[k1, 1] - v[k1, 0])
        v[k2, 1] = v[k2, 0]; v[k2, 2] = v[k2, 0]
        return v
    shift = lambda: rng.uniform(-1, 1, (per, 1, 3)) * rng.choice([0.2, 1.0], (per, 1, 1))                     # noqa: E731
    add(flat(tri(), rng.randint(0, 2, per)), tri() + shift())                                                 # A a segment
    add(flat(tri(), np.full(per, 2)), tri() + shift())                                                        # A a point
    add(tri(), flat(tri(), rng.randint(0, 2, per)) + shift())                                                 # B a segment
    add(tri(), flat(tri(), np.full(per, 2)) + shift())                                                        # B a point
    add(flat(tri(), rng.randint(0, 3, per)), flat(tri(), rng.randint(0, 3, per)) + shift())                   # both without area
    a = tri()                                                                                                 # through each other
    w = rng.dirichlet([1, 1, 1], per)
    inside = (a * w[:, :, None]).sum(1)
    d = rng.uniform(-1, 1, (per, 3))
    b = np.stack([inside - d * rng.uniform(0.1, 1, (per, 1)), inside + d * rng.uniform(0.1, 1, (per, 1)), inside + rng.uniform(-1, 1, (per, 3))], 1)
    add(a, b)
    a = tri()                                                                                                 # coplanar, or nearly
    wts = rng.uniform(-0.6, 1.2, (per, 3, 3))
    wts /= wts.sum(2, keepdims=True)
    add(a, np.einsum("nij,njk->nik", wts, a) + rng.choice([0.0, 1e-7, 1e-5], (per, 1, 1)) * rng.uniform(-1, 1, (per, 3, 3)))
    tiny = np.float32(1e-45).astype(np.float64)                                                               # denormal
    add(rng.randint(-3000, 3000, (per, 3, 3)) * tiny, rng.randint(-3000, 3000, (per, 3, 3)) * tiny)
    a = tri() * rng.choice([1.0, 1e15, 1e30, 3e38], (per, 1, 1))                                              # huge and non-finite
    b = tri() * rng.choice([1.0, 1e15, 1e30, 3e38], (per, 1, 1))
    for v in (a, b):
        bad = np.nonzero(rng.randint(0, 8, per) == 0)[0]
        v.reshape(per, 9)[bad, rng.randint(0, 9, len(bad))] = rng.choice([np.nan, np.inf, -np.inf], len(bad))
    add(a, b)
    assert len(As) == len(FAMILIES)
    return np.concatenate(As), np.concatenate(Bs)


@pytest.fixture(scope="module")
def floats(driver, tmp_path_factory):
    """Every family once through the driver and through numpy"""
    a, b = float_cases()
    lo, hi = enlarged(np.random.RandomState(2), b)
    got, feature, live = run_bulk(driver, a, b, lo, hi, tmp_path_factory.mktemp("pair_floats"), "floats")
    want, ref = numpy_words(a, b, lo, hi)
    return a, b, got, feature, live, want, ref


def test_non_integer_inputs_equal_numpy_bit_for_bit(floats):
    a, b, got, feature, live, want, ref = floats
    assert len(a) == PER * len(FAMILIES)
    same_words(got, want, "dist2 u v qa qb bound")
    assert (feature == ref.feature).all(), np.nonzero(feature != ref.feature)[0][:10]
    with np.errstate(invalid="ignore"):
        assert (live == (a - a == 0).all((1, 2))).all()
    part = {name: slice(k * PER, (k + 1) * PER) for k, name in enumerate(FAMILIES)}
    finite = slice(0, part["huge and non-finite"].start)
    assert not np.isnan(ref.dist2[finite]).any() and (feature[finite] != FEATURE_NONE).all()
    # every feature wins somewhere, and every one of the six piercing edges decides somewhere
    seen = np.bincount(feature, minlength=22)
    print("features", seen)
    assert (seen[:15] > 50).all() and (seen[16:22] > 50).all()
    pierced = feature >= FEATURE_PIERCE
    assert (ref.dist2[pierced] == 0).all() and (got[pierced, 3:6] == got[pierced, 6:9]).all()
    for name, lo_share, hi_share in (("near", 0.02, 0.6), ("through each other", 0.9, 1.0), ("far", 0.0, 0.0), ("A a point", 0.0, 0.0), ("B a point", 0.0, 0.0),
                                     ("A a segment", 0.01, 0.5), ("B a segment", 0.01, 0.5)):
        share = pierced[part[name]].mean()
        print("%-20s pierced %5.1f %%" % (name, 100 * share))
        assert lo_share <= share <= hi_share, (name, share)
    # an edge pair decides where edges are parallel, and a vertex pair where a vertex is shared: the distance there is 0
    assert ((feature[part["parallel edges"]] >= 6) & (feature[part["parallel edges"]] < 15)).mean() > 0.2
    shared = ~pierced[part["shared vertex"]]
    assert (ref.dist2[part["shared vertex"]][shared] == 0).all() and shared.mean() > 0.2
    # u and v are the weights of b0 and b1 at qb: the point they give is qb, to rounding (the finite families)
    keep = np.nonzero(~np.isnan(ref.dist2[finite]) & (np.abs(b[finite]).reshape(-1, 9).max(1) > 1e-30))[0]
    u, v = ref.u[keep].astype(np.float64), ref.v[keep].astype(np.float64)
    bb = b[keep].astype(np.float64)
    at = bb[:, 0] * u[:, None] + bb[:, 1] * v[:, None] + bb[:, 2] * (1 - u - v)[:, None]
    scale = np.abs(bb).reshape(-1, 9).max(1)
    off = np.abs(at - ref.qb[keep]).max(1) / scale
    for name in FAMILIES[:-2]:
        rows = (keep >= part[name].start) & (keep < part[name].stop)
        print("%-20s qb against its weights: median %.3g, worst %.3g of the largest coordinate" % (name, np.median(off[rows]), off[rows].max()))
    # (where B has area and the pair is not nearly in one plane, the weights are well conditioned)
    for name in ("near", "far", "small against large", "through each other", "A a segment", "A a point"):
        rows = (keep >= part[name].start) & (keep < part[name].stop)
        assert np.median(off[rows]) < 1e-6 and (off[rows] < 1e-3).mean() > 0.999, name
    # the order matters: the first of equal features wins (a triangle against itself: every vertex feature gives 0, feature 0 stays)
    ints = np.random.RandomState(9).randint(-8, 9, (100, 3, 3)).astype(np.float32)      # (integers: nothing in one plane is pierced by rounding)
    same = pair_np(ints, ints)
    assert (same.feature == 0).all() and (same.dist2 == 0).all() and (same.u == 1).all() and (same.v == 0).all()


def test_the_bound_never_exceeds_the_distance(floats):
    """Random records under random enclosing boxes, pierced pairs included: bound <= dist2 wherever neither is a NaN, and never
    bound > dist2 (a NaN bound, inf - inf of a huge box, skips nothing). None may fail; a pierced pair's bound is 0."""
    a, b, got, feature, live, want, ref = floats
    bound = got[:, 9].view(np.float32)
    ok = ~np.isnan(ref.dist2)
    with np.errstate(invalid="ignore"):
        bad = np.nonzero(ok & ~np.isnan(bound) & ~(bound <= ref.dist2) | ok & (bound > ref.dist2))[0]
    assert len(bad) == 0, (len(bad), bad[:5], bound[bad[:5]], ref.dist2[bad[:5]])
    assert ok.sum() > 150000 and (bound[ok] > 0).mean() > 0.1 and (bound[ok] == ref.dist2[ok]).sum() > 0
    assert (bound[(feature >= FEATURE_PIERCE) & ~np.isnan(bound)] == 0).all() and (bound[:len(FAMILIES[:-1]) * PER][feature[:len(FAMILIES[:-1]) * PER] >= FEATURE_PIERCE] == 0).all()
    # and the record's own box, the bound the kernel skips a record by
    lo, hi = box_np(b)
    alo, ahi = box_np(a)
    own = box_bound_np(lo, hi, alo, ahi)
    with np.errstate(invalid="ignore"):
        fin = ok & ~np.isnan(bound) & ~np.isnan(own)
        assert (own[fin] <= ref.dist2[fin]).all() and (bound[fin] <= own[fin]).all() and not (own[ok] > ref.dist2[ok]).any()


# ---------------------------------------------------------------------------------------------- integer inputs

def seg_i(p, q):
    return [Fraction(int(x)) for x in p], [Fraction(int(x)) for x in q]


def point_segment2(x, p, q):
    d = sub_i(q, p)
    dd = dot_i(d, d)
    t = Fraction(0) if dd == 0 else max(Fraction(0), min(Fraction(1), Fraction(dot_i(sub_i(x, p), d)) / dd))
    w = [x[k] - (p[k] + t * d[k]) for k in range(3)]
    return dot_i(w, w)


def segment_segment2(p1, q1, p2, q2):
    """the squared distance of two closed segments, exactly: the four end points against the other segment, and the common
    perpendicular where it meets both inside"""
    best = min(point_segment2(p1, p2, q2), point_segment2(q1, p2, q2), point_segment2(p2, p1, q1), point_segment2(q2, p1, q1))
    d1, d2, r = sub_i(q1, p1), sub_i(q2, p2), sub_i(p1, p2)
    a, e, b, c, f = dot_i(d1, d1), dot_i(d2, d2), dot_i(d1, d2), dot_i(d1, r), dot_i(d2, r)
    den = a * e - b * b
    if den != 0:
        s, t = Fraction(b * f - c * e) / den, Fraction(a * f - b * c) / den
        if 0 < s < 1 and 0 < t < 1:
            w = [(p1[k] + s * d1[k]) - (p2[k] + t * d2[k]) for k in range(3)]
            best = min(best, dot_i(w, w))
    return best


def point_triangle2(x, v):
    best = min(point_segment2(x, v[k], v[(k + 1) % 3]) for k in range(3))
    n = cross_i(sub_i(v[1], v[0]), sub_i(v[2], v[0]))
    nn = dot_i(n, n)
    if nn != 0:
        w = sub_i(x, v[0])
        side = [dot_i(n, cross_i(sub_i(v[(k + 1) % 3], v[k]), sub_i(x, v[k]))) for k in range(3)]
        if all(s >= 0 for s in side):                                 # the foot of the perpendicular lies in the triangle
            h = dot_i(n, w)
            best = min(best, Fraction(h * h) / nn)
    return best


def exact_distance2(a, b):
    """two triangles (or segments, or points) with integer vertices: their squared distance as a fraction"""
    if exact_meet(a, b):
        return Fraction(0)
    a = [[Fraction(int(x)) for x in p] for p in a]
    b = [[Fraction(int(x)) for x in p] for p in b]
    best = min(min(point_triangle2(p, b) for p in a), min(point_triangle2(p, a) for p in b))
    for i in range(3):
        for j in range(3):
            best = min(best, segment_segment2(a[i], a[(i + 1) % 3], b[j], b[(j + 1) % 3]))
    return best


def crosses_properly(a, b):
    """does an edge of one go strictly through the interior of the other? (Python integers)"""
    a = [[int(x) for x in p] for p in a]
    b = [[int(x) for x in p] for p in b]
    for e, t in ((a, b), (b, a)):
        n = cross_i(sub_i(t[1], t[0]), sub_i(t[2], t[0]))
        for k in range(3):
            p, q = e[k], e[(k + 1) % 3]
            dp, dq = dot_i(n, sub_i(p, t[0])), dot_i(n, sub_i(q, t[0]))
            if not ((dp > 0 and dq < 0) or (dp < 0 and dq > 0)):
                continue
            d = sub_i(q, p)
            s = [dot_i(d, cross_i(sub_i(t[m], p), sub_i(t[(m + 1) % 3], p))) for m in range(3)]
            if all(x > 0 for x in s) or all(x < 0 for x in s):
                return True
    return False


def test_integer_inputs_against_an_exact_reference_in_fractions(driver, tmp_path):
    a, b, kind = integer_cases(seed=11, n=4000)
    n = len(a)
    af, bf = a.astype(np.float32), b.astype(np.float32)
    lo, hi = enlarged(np.random.RandomState(1), bf)
    got, feature, live = run_bulk(driver, af, bf, lo, hi, tmp_path, "integers")
    want, ref = numpy_words(af, bf, lo, hi)
    same_words(got, want, "integers")
    assert (feature == ref.feature).all() and live.all()
    dist2 = got[:, 0].view(np.float32)
    assert not np.isnan(dist2).any() and (feature != FEATURE_NONE).all()
    meet = np.array([exact_meet(a[i], b[i]) for i in range(n)])
    proper = np.array([crosses_properly(a[i], b[i]) for i in range(n)])
    assert proper.sum() > n // 20 and (~meet).sum() > n // 5 and (meet & ~proper).sum() > n // 20
    # every pair that crosses properly is pierced and has dist2 == 0.0 exactly; no disjoint pair has dist2 == 0; a pierced pair meets
    assert (feature[proper] >= FEATURE_PIERCE).all() and (dist2[proper] == 0).all()
    assert (dist2[~meet] > 0).all()
    assert meet[feature >= FEATURE_PIERCE].all()
    # sqrt(dist2) against the exact distance, on all of them
    exact = np.array([float(exact_distance2(a[i], b[i])) for i in range(n)]) ** 0.5
    mag = np.maximum(np.abs(a).reshape(n, 9).max(1), np.abs(b).reshape(n, 9).max(1)).astype(np.float64)
    err = np.abs(np.sqrt(dist2.astype(np.float64)) - exact)
    worst = (err / np.maximum(mag, 1)).max() * 2.0 ** 23
    print("integer pairs %d: meet %d, cross properly %d, worst error %.2f * 2^-23 of the largest coordinate" % (n, meet.sum(), proper.sum(), worst))
    assert (err <= ACCURACY_ASSERTED * 2.0 ** -23 * mag).all(), (worst, np.nonzero(err > ACCURACY_ASSERTED * 2.0 ** -23 * mag)[0][:5])
    assert (dist2[meet] < 1e-9).all()


# ---------------------------------------------------------------------------------------------- accuracy

def test_accuracy_against_float64():
    """|sqrt(dist2) - exact| <= ACCURACY_ASSERTED * 2^-23 of the largest coordinate magnitude involved, on random pairs at the
    five combinations of size and distance (the header's statement, measured by scripts/pair_accuracy.py over 8 million pairs;
    slivers and degenerate triangles are not part of it)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("pair_accuracy", os.path.join(ROOT, "scripts", "pair_accuracy.py"))
    acc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(acc)
    rng = np.random.RandomState(20250118)
    worst = 0.0
    for sp in acc.SCALE_PAIRS:
        a, b = acc.random_pairs(rng, 20000, *sp)
        w, pierced = acc.worst_error(a, b)
        print("scale pair %s: %d pairs, %.1f %% pierced, worst error %.2f * 2^-23 of the largest coordinate" % (sp, len(a), 100 * pierced, w))
        worst = max(worst, w)
    assert worst <= ACCURACY_ASSERTED
    text = " ".join(open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_pair_rule.h")).read().replace("\n//", "\n").split())
    assert "within %s * 2^-23" % ACCURACY_MEASURED in text and "asserts %s * 2^-23" % ACCURACY_ASSERTED in text
    assert 2.4 <= ACCURACY_ASSERTED / ACCURACY_MEASURED <= 2.6


# ---------------------------------------------------------------------------------------------- the walk

def torus_small(nu=6, nv=5, R=0.5, r=0.2, centre=(0.5, 0.5, 0.5)):
    u, v = np.meshgrid(np.arange(nu) * (2 * np.pi / nu), np.arange(nv) * (2 * np.pi / nv), indexing="ij")
    p = (np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], -1) + np.array(centre)).astype(np.float32)
    tris = []
    for i in range(nu):
        for j in range(nv):
            c = [p[i, j], p[(i + 1) % nu, j], p[(i + 1) % nu, (j + 1) % nv], p[i, (j + 1) % nv]]
            tris += [[c[0], c[1], c[2]], [c[0], c[2], c[3]]]
    return np.array(tris, np.float32)


def walk_scene(rng):
    """A soup, a small closed mesh, that mesh once more in place (equal dist2 under two ids: the lower must win), and a stack of
    parallel plates that one query pierces all at once (all dist2 0: the lowest id must win)"""
    soup = (rng.uniform(0, 1, (50, 1, 3)) + rng.uniform(-0.08, 0.08, (50, 3, 3))).astype(np.float32)
    mesh = torus_small()
    plates = np.array([[[1.5, -0.2, z], [2.1, -0.2, z], [1.8, 0.5, z]] for z in np.linspace(0.1, 0.9, 8)], np.float32)
    return np.concatenate([soup, mesh, plates, mesh]), len(soup), len(mesh), len(plates)


def walk_queries(rng, tris, n_soup, n_mesh, n_plates):
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    q = [rng.uniform(lo - 0.3, hi + 0.3, (40, 1, 3)) + rng.choice([0.02, 0.1, 0.4], (40, 1, 1)) * rng.uniform(-1, 1, (40, 3, 3))]
    q.append(tris[rng.permutation(len(tris))[:25]])                                   # the scene's own: distance 0 to themselves
    seg = rng.uniform(lo, hi, (12, 1, 3)) + rng.uniform(-0.3, 0.3, (12, 3, 3))
    seg[:, 2] = seg[:, 1]
    q.append(seg)                                                                     # segments
    q.append(np.repeat(rng.uniform(lo - 0.2, hi + 0.2, (12, 1, 3)), 3, 1))            # points
    q.append(np.array([[[1.8, 0.1, -0.5], [1.8, 0.1, 1.5], [1.85, 0.12, 1.5]],        # through every plate
                       [[1.8, 0.1, -0.5], [1.8, 0.1, 1.5], [1.8, 0.1, 1.5]]]))        # ... and a segment through every plate
    q.append(np.stack([np.stack([lo, hi, hi * np.float32(np.nan)]), np.stack([lo, hi * np.float32(np.inf), hi])]))      # not live
    q = np.concatenate(q).astype(np.float32)
    n = len(q)
    ext = float((hi - lo).max())
    max2 = (rng.choice([0.02, 0.1, 0.3, 1.0], n) * ext).astype(np.float32) ** 2
    max2[::3] = RTK_INF
    max2[1:40:8] = [0.0, -1.0, np.nan, 1e-45, -0.0]
    first = (rng.randint(0, len(tris), n) * (rng.randint(0, 3, n) == 0)).astype(np.uint32)
    flags = rng.randint(0, 2, n).astype(np.uint32)
    first[-4:-2] = 0; flags[-4:-2] = 0; max2[-4:-2] = RTK_INF
    return q, max2, first, flags


def test_host_walk_equals_brute_force_in_every_order(driver, tmp_path):
    rng = np.random.RandomState(5)
    tris, n_soup, n_mesh, n_plates = walk_scene(rng)
    nodes, recs = small_tree(rng, tris, 5)
    assert len(nodes) > 8
    q, max2, first, flags = walk_queries(rng, tris, n_soup, n_mesh, n_plates)
    prims = np.arange(len(tris))
    ref = [brute_force_pairs(tris, prims, q, max2, first, fl) for fl in (0, 1)]
    rec, pa, pb = (np.where((flags == 1)[:, None], ref[1][k], ref[0][k]) for k in range(3))
    hit = rec[:, 3] != NONE
    assert hit.sum() > 50 and (~hit).sum() >= 7 and not hit[-2:].any()
    # the through-everything queries pierce all eight plates and answer the lowest id of them
    first_plate = n_soup + n_mesh
    assert (rec[-4:-2, 3] == first_plate).all() and (rec[-4:-2, 0] == 0).all()
    allp = pair_np(q[-4:-2, None], tris[None, first_plate:first_plate + n_plates])
    assert (allp.dist2 == 0).all() and (allp.feature >= FEATURE_PIERCE).all()
    # the mesh stands twice in place: whoever answers with a mesh triangle answers with the lower id
    mesh_ids = rec[hit, 3][(rec[hit, 3] >= n_soup)]
    unfiltered = (first == 0) & hit
    assert (rec[unfiltered, 3] < first_plate + n_plates).all() and (mesh_ids >= n_soup).any()
    assert (rec[hit & (first > first_plate + n_plates), 3] >= first_plate + n_plates).any()      # (the copy answers once the filter hides the original)
    text = "n %d %s\nt %d %s\n" % (len(nodes), hexes(nodes), len(recs), hexes(recs))
    qwords = np.concatenate([q.reshape(-1, 9).view(np.uint32), max2.view(np.uint32)[:, None], first[:, None], flags[:, None]], 1)
    want = np.concatenate([rec, pa, pb], 1)
    evaluated = []
    for order in (0, 1, 2, 3):
        out = run_driver(driver, text + "".join("q %d %s\n" % (order, hexes(w)) for w in qwords), len(qwords), tmp_path, "walk_%d" % order)
        got = np.array([[int(x, 16) for x in line[:10]] for line in out], np.uint32)
        bad = np.nonzero((got != want).any(1))[0]
        assert len(bad) == 0, (order, bad[:5], got[bad[:3]], want[bad[:3]])
        evaluated.append(sum(int(line[10]) for line in out))
    print("records evaluated in slot order %d, reversed %d, drawn %d, nearest first %d of %d" % (tuple(evaluated) + (len(q) * len(tris),)))
    assert evaluated[3] < min(evaluated[:3]) and evaluated[3] < 0.25 * len(q) * len(tris)        # (the bound does cull)
    # a scene without triangles: a miss as stated
    out = run_driver(driver, "n 0\nt 0\nq 0 %s\n" % hexes(qwords[0]), 1, tmp_path, "empty")
    assert [int(x, 16) for x in out[0][:10]] == [int(qwords[0][9]), 0, 0, NONE] + [int(x) for x in qwords[0][:3]] * 2


# ---------------------------------------------------------------------------------------------- the interface

def test_rule_header_includes_no_hip_and_states_its_rules():
    text = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_pair_rule.h")).read()
    assert [l.split()[1] for l in text.splitlines() if l.startswith("#include")] == ['"rtk_touch_rule.h"']
    assert "hip_runtime" not in text and "__global__" not in text and "fmaf" not in text
    code = text.split("#pragma once")[1]
    for used in ("rtk_closest_triangle(", "rtk_closest_better(", "rtk_box_boxes_touch(", "rtk_touch_edges(", "rtk_touch_cross("):
        assert used in code, used
    assert "rtk_touch_separated" not in code and "rtk_touch_candidate" not in code                  # (not the seventeen axes)
    flat = " ".join(text.replace("\n//", "\n").split())
    for word in ("1. LIVE", "2. FIFTEEN FEATURE PAIRS", "3. PIERCING", "4. FILTER", "5. ANSWER", "6. BOX BOUND", "NOTHING IS EVER DECIDED BY 0 / 0", "no epsilon",
                 "THE FIRST IN THIS ORDER AMONG EQUAL ONES", "A NaN dist2 never wins", "STRICTLY OPPOSITE SIGNS", "not all three may be zero",
                 "BOXES TOUCH", "THE FIRST PIERCING EDGE IN THIS ORDER", "THE LOWEST PRIMITIVE ID", "WITHOUT A MARGIN", "bound <= dist2", "FLOAT RULE",
                 "DEFINED BY IT", "NON-FINITE", "NOTHING ELSE IS PROMISED", "part of the rule", "dist2 < max_dist2", "bound >= max_dist2", "rtk_touch_filter_passes"):
        assert word in flat, word
    for name in ("rtk_touch_rule.h", "rtk_box_rule.h", "rtk_closest_rule.h"):
        assert "rtk_pair" not in open(os.path.join(ROOT, "rtk_amd", "csrc", name)).read()        # (used as they are, not changed)
    header = open(os.path.join(ROOT, "include", "rtk_amd.h")).read()
    section = header[header.index("/* ---- Closest triangles"):header.index("/* ---- Every hit along a ray")]
    section = " ".join(section.replace("\n *", "\n").split())
    for word in ("rtk_pair_rule.h", "A SLOT THAT IS NOT LISTED IS NOT WRITTEN", "DETERMINISTIC", "NOTHING ELSE IS PROMISED", "rtk_dev_trace_status",
                 "rtk_mgpu_scene(m, i)", "THE LOWEST PRIMITIVE ID AMONG EQUAL dist2", "FIFTEEN FEATURE PAIRS", "PIERCING", "RTK_TOUCH_SKIP_SHARED_VERTEX",
                 "unknown bit", "vertex 0 as given", "rtk_dev_select_rays", "rtk_dev_expand_hits", "without a margin", "a segment", "NULL means RTK_INF"):
        assert word in section, word
    mk = open(os.path.join(ROOT, "rtk_amd", "csrc", "Makefile")).read()
    assert "rtk_pair_rule.h" in mk and "rtk_pair.hip" in mk
    kernel = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_pair.hip")).read()
    for used in ("rtk_pair_evaluate(", "rtk_pair_box_bound(", "rtk_pair_skip(", "rtk_pair_wins(", "rtk_touch_live(", "rtk_touch_filter_passes(", "LaunchScratch",
                 "kernel-resource-usage"):
        assert used in kernel, used
    for doc, word in (("README.md", "rtk_dev_closest_triangles"), ("INTEGRATION.md", "## Closest triangles"), ("DESIGN.md", "Closest triangles"),
                      (os.path.join("docs", "HISTORY.md"), "rtk_dev_closest_triangles")):
        assert word in open(os.path.join(ROOT, doc)).read(), doc


def test_header_symbols_and_argtypes(api):
    text = open(os.path.join(ROOT, "include", "rtk_amd.h")).read()
    for word in ("int rtk_dev_closest_triangles(const rtk_dev_scene *ds, const rtk_tri_query *d_tris, size_t num_queries,",
                 "int rtk_dev_closest_triangles_counted(const rtk_dev_scene *ds, const rtk_tri_query *d_tris, size_t num_queries,",
                 "uint32_t rtk_amd_pair_stack_entries(void);"):
        assert word in text, word
    assert text.index("/* ---- Triangles that touch a triangle") < text.index("/* ---- Closest triangles") < text.index("/* ---- Every hit along a ray")
    L = api.lib()
    for name in ("rtk_dev_closest_triangles", "rtk_dev_closest_triangles_counted", "rtk_amd_pair_stack_entries"):
        assert name in api.RTK_AMD_H_SYMBOLS and hasattr(L, name), name
    F = C.POINTER(api.TouchFilter)
    assert L.rtk_dev_closest_triangles.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(api.RayList), F, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_void_p]
    assert L.rtk_dev_closest_triangles_counted.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, F, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                            C.POINTER(api.TraceCounters)]
    assert L.rtk_dev_closest_triangles.restype == C.c_int and L.rtk_dev_closest_triangles_counted.restype == C.c_int
    assert L.rtk_amd_pair_stack_entries.restype == C.c_uint32 and 1 <= L.rtk_amd_pair_stack_entries() <= 64
    for name in ("closest_triangles_device", "closest_triangles_counted", "closest_triangles", "distance", "self_clearance"):
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
    # scene, triangles, n, list, filter, max_dist2, records, points on the query, points on the scene, stream
    for args in [(None, dummy, 4, None, None, None, dummy, None, None, None), (dummy, None, 4, None, None, None, dummy, None, None, None),
                 (dummy, dummy, 4, None, good, dummy, None, dummy, dummy, None), (dummy, dummy, 1 << 32, None, None, None, dummy, None, None, None),
                 (dummy, dummy, 1 << 32, C.byref(ray_list()), good, None, dummy, None, None, None)] + \
                [(dummy, dummy, 4, C.byref(l), None, None, dummy, None, None, None) for l in bad_lists] + \
                [(dummy, dummy, 4, None, C.byref(f), None, dummy, None, None, None) for f in bad_filters]:
        assert L.rtk_dev_closest_triangles(*args) == ERR_BAD_ARG, args
        assert "rtk_dev_closest_triangles:" in api.last_error()
    # counted: scene, triangles, n, filter, max_dist2, records, points, points, counters
    ctr = api.TraceCounters()
    for args in [(dummy, dummy, 4, None, None, dummy, None, None, None), (None, dummy, 4, None, None, dummy, None, None, C.byref(ctr)),
                 (dummy, None, 4, None, None, dummy, None, None, C.byref(ctr)), (dummy, dummy, 4, good, None, None, None, None, C.byref(ctr)),
                 (dummy, dummy, 1 << 32, None, None, dummy, None, None, C.byref(ctr))] + \
                [(dummy, dummy, 4, C.byref(f), None, dummy, None, None, C.byref(ctr)) for f in bad_filters]:
        assert L.rtk_dev_closest_triangles_counted(*args) == ERR_BAD_ARG, args
        assert "rtk_dev_closest_triangles_counted:" in api.last_error()
    # no queries: nothing to do, nothing launched
    assert L.rtk_dev_closest_triangles(dummy, None, 0, None, None, None, None, None, None, None) == 0
    assert L.rtk_dev_closest_triangles(dummy, dummy, 0, C.byref(ray_list()), good, dummy, dummy, dummy, dummy, None) == 0
    ctr.rays = 7
    assert L.rtk_dev_closest_triangles_counted(dummy, None, 0, None, None, None, None, None, C.byref(ctr)) == 0 and ctr.rays == 0
