"""Sphere sweeps without a GPU: the rule of rtk_amd/csrc/rtk_sweep_rule.h, run by tests/sweep_rule_driver.cpp under the address
and undefined-behaviour sanitizers, against numpy float32 arithmetic in the stated order (tests/sweep_ref.py), bit for bit; the
entry time of a box against the time of every triangle inside it; the accuracy statement against float64; and the parts of the
interface that need no device -- header text, symbols, struct sizes, argtypes, the refusals decided before any HIP call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.closest_ref import tri_box, tri_np
from tests.sweep_ref import (FEATURE_NAMES, SW_FACE, SW_NONE, SW_START, better_np, centre_np, prepare, slab_np, tri_sweep_np)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_BAD_ARG = -2
RTK_INF = np.float32(3.402823e+38)
# (triangle scale, distance of the start from the triangle, largest radius)
SCALES = [(1.0, 3.0, 0.3), (1.0, 3.0, 0.01), (1e-3, 1.0, 1e-3), (100.0, 300.0, 30.0), (1.0, 30.0, 1.0)]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """The driver built against the rule headers alone (no HIP include path, -Wall -Werror, no FMA contraction as in the library)
    with both sanitizers. -O2 and -mfma: a compiler that were allowed to contract would do it here."""
    exe = str(tmp_path_factory.mktemp("sweep_rule") / "sweep_rule_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-mfma", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "rtk_amd", "csrc"), os.path.join(ROOT, "tests", "sweep_rule_driver.cpp"), "-o", exe])
    return exe


def run_driver(exe, kind, words, tmp_path):
    """words uint32 [n, k] -> the driver's output lines as integers [n, m] (hexadecimal words first, then decimal flags)"""
    path = str(tmp_path / ("cases_%s.txt" % kind))
    with open(path, "w") as f:
        f.write("".join("%s %s\n" % (kind, " ".join("%x" % w for w in row)) for row in words.tolist()))
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    assert lines[len(words)] == "ok"
    hexes = {"q": 5, "b": 1, "t": 1, "c": 0, "s": 0}[kind]
    return np.array([[int(w, 16) if k < hexes else int(w) for k, w in enumerate(line.split())] for line in lines[:len(words)]], np.int64)


def same_bits(got, want):
    """Bit for bit, except where the expected value is NaN: there only "it is NaN" is promised."""
    got = np.ascontiguousarray(got, np.uint32)
    want = np.ascontiguousarray(want, np.float32)
    nan = np.isnan(want)
    assert (np.isnan(got.view(np.float32)) == nan).all()
    bad = (got != want.view(np.uint32)) & ~nan
    assert not bad.any(), (np.argwhere(bad)[:5], got[bad][:5], want.view(np.uint32)[bad][:5])


def make_sweeps(origin, direction, min_t, max_t, radius):
    n = len(origin)
    s = np.zeros((n, 9), np.float32)
    s[:, 0:3], s[:, 3:6] = origin, direction
    s[:, 6], s[:, 7], s[:, 8] = min_t, max_t, radius
    return s


def random_family(rng, n, tri_scale, dist, rmax):
    """Triangles of the given size about the origin; paths from `dist` away towards a point of the triangle's plane that lies
    inside the triangle or a little outside, lifted by up to two radii (so that the face, every edge, every vertex and a miss
    are met); a tenth start within the radius; max_t without a limit, beyond the contact or short of it."""
    t = (rng.standard_normal((n, 3, 3)) * tri_scale).astype(np.float32)
    w = rng.uniform(-0.7, 1.7, (n, 2))
    r = (rng.uniform(0, 1, n) ** 2 * rmax).astype(np.float32)
    aim = t[:, 0] + (t[:, 1] - t[:, 0]) * w[:, :1] + (t[:, 2] - t[:, 0]) * w[:, 1:] + rng.standard_normal((n, 3)) * r[:, None] * rng.uniform(0, 1.2, (n, 1))
    away = rng.standard_normal((n, 3))
    away /= np.linalg.norm(away, axis=1, keepdims=True)
    near = rng.uniform(0, 1, n) < 0.1
    o = aim + away * np.where(near, r * rng.uniform(0, 1.5, n), dist * rng.uniform(0.3, 1.5, n))[:, None]
    d = (aim - o) * rng.uniform(0.4, 2.5, (n, 1)) + rng.standard_normal((n, 3)) * 1e-3 * dist
    max_t = np.where(rng.uniform(0, 1, n) < 0.5, RTK_INF, rng.uniform(0.2, 4.0, n)).astype(np.float32)
    min_t = np.where(rng.uniform(0, 1, n) < 0.8, 0.0, rng.uniform(-1.0, 0.15, n)).astype(np.float32)
    return make_sweeps(o, d, min_t, max_t, r), t


def special_families(rng):
    """name -> (sweeps [n, 9], tris [n, 3, 3]) float32"""
    fam = {}
    n = 2000
    s, t = random_family(rng, n, 1.0, 3.0, 0.3)
    k = rng.uniform(-0.5, 1.5, (n, 1))
    t[:, 2] = (t[:, 0] + (t[:, 1] - t[:, 0]) * k + rng.standard_normal((n, 3)) * 10.0 ** rng.uniform(-8, -3, (n, 1))).astype(np.float32)
    fam["slivers"] = (s, t)
    s, t = random_family(rng, 600, 1.0, 3.0, 0.3)
    t[:, 1] = t[:, 0]
    fam["a=b"] = (s, t)
    s, t = random_family(rng, 600, 1.0, 3.0, 0.3)
    t[:, 1] = t[:, 0]; t[:, 2] = t[:, 0]
    fam["a=b=c"] = (s, t)
    # one or two direction components exactly zero: the containment branch of the slab routine
    s, t = random_family(rng, 1500, 1.0, 3.0, 0.5)
    zero = np.arange(1500) % 3
    s[np.arange(1500), 3 + zero] = 0.0
    s[np.arange(1500)[::2], 3 + (zero[::2] + 1) % 3] = 0.0
    s[::5, 3 + zero[::5]] = -0.0
    fam["axis-aligned directions"] = (s, t)
    s, t = random_family(rng, 1500, 1.0, 3.0, 0.5)
    s[np.arange(1500), 3 + np.arange(1500) % 3] = (rng.choice([-1.0, 1.0], 1500) * 10.0 ** rng.uniform(-45, -38, 1500)).astype(np.float32)
    fam["denormal direction components"] = (s, t)
    s, t = random_family(rng, 1500, 1.0, 3.0, 0.3)
    s[:, 8] = 0.0
    s[::7, 8] = -0.0
    fam["radius 0"] = (s, t)
    s, t = random_family(rng, 1000, 1.0, 0.3, 0.4)
    s[:, 7] = s[:, 6]
    fam["min_t = max_t"] = (s, t)
    # a start that already touches: the centre at min_t within the radius of a point of the triangle, or exactly on it
    s, t = random_family(rng, 1200, 1.0, 3.0, 0.3)
    w = rng.uniform(0, 1, (1200, 2)); w[w.sum(1) > 1] = 1 - w[w.sum(1) > 1]
    on = t[:, 0] + (t[:, 1] - t[:, 0]) * w[:, :1] + (t[:, 2] - t[:, 0]) * w[:, 1:]
    s[:, 6] = 0.0
    s[:, 0:3] = on + rng.standard_normal((1200, 3)) * (s[:, 8:9] * 0.5)
    s[::4, 0:3] = t[::4, 1]
    fam["a start that touches"] = (s, t)
    # paths parallel to an edge and to the face, at about one radius from it
    s, t = random_family(rng, 1500, 1.0, 3.0, 0.3)
    i = np.arange(1500)
    e = t[i, (i + 1) % 3] - t[i, i % 3]
    s[:, 3:6] = e * rng.uniform(-2, 2, (1500, 1))
    fam["parallel to an edge"] = (s, t)
    s, t = random_family(rng, 1500, 1.0, 3.0, 0.3)
    s[:, 3:6] = (t[:, 1] - t[:, 0]) * rng.uniform(-1, 1, (1500, 1)) + (t[:, 2] - t[:, 0]) * rng.uniform(-1, 1, (1500, 1))
    nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    s[:, 0:3] = t.mean(1) - s[:, 3:6] * 1.5 + nrm * s[:, 8:9] * rng.uniform(0.5, 1.5, (1500, 1))
    fam["parallel to the face"] = (s, t)
    # grazing: the path passes a vertex at a distance within a few ulps of the radius (discriminants around 0)
    s, t = random_family(rng, 3000, 1.0, 3.0, 0.3)
    i = np.arange(3000)
    v = t[i, i % 3].astype(np.float64)
    d = s[:, 3:6].astype(np.float64)
    side = np.cross(d, rng.standard_normal((3000, 3))); side /= np.linalg.norm(side, axis=1, keepdims=True)
    s[:, 0:3] = v - d * rng.uniform(0.5, 1.5, (3000, 1)) + side * (s[:, 8:9].astype(np.float64) * (1 + rng.uniform(-4e-7, 4e-7, (3000, 1))))
    s[:, 6], s[:, 7] = 0.0, RTK_INF
    fam["grazing"] = (s, t)
    # max_t at the float32 neighbour below the time, at it and above it (rows 0, 1, 2 mod 3), with min_t < 0: the entry time te
    # is then negative as a rule, max_t - te is larger than max_t, and its rounding admits feature times whose te + t lies
    # an ulp beyond max_t: 2. (iv) of the header makes them none
    s, t = random_family(rng, 12000, 1.0, 3.0, 0.3)
    s[:, 6], s[:, 7] = rng.uniform(-4.0, -0.5, 12000), RTK_INF
    f, time = tri_sweep_np(prepare(s), t[:, 0], t[:, 1], t[:, 2])
    s, t, time = s[f > SW_START][:1500], t[f > SW_START][:1500], time[f > SW_START][:1500]
    assert len(s) == 1500
    s[0::3, 7] = np.nextafter(time[0::3], np.float32(-np.inf))
    s[1::3, 7] = time[1::3]
    s[2::3, 7] = np.nextafter(time[2::3], np.float32(np.inf))
    fam["max_t around the time, min_t < 0"] = (s, t)
    # queries that are not live
    s, t = random_family(rng, 900, 1.0, 3.0, 0.3)
    bad = np.array([np.nan, np.inf, -np.inf], np.float32)
    s[np.arange(450), np.arange(450) % 9] = bad[(np.arange(450) // 9) % 3]
    s[450:600, 8] = -np.abs(s[450:600, 8]) - np.float32(1e-30)
    s[600:750, 3:6] = 0.0
    s[600:750:2, 4] = -0.0
    s[750:900, 7] = np.minimum(s[750:900, 7], 10.0)
    s[750:900, 6] = s[750:900, 7] + 1.0
    fam["not live"] = (s, t)
    return fam


@pytest.fixture(scope="module")
def cases():
    """Every family once: name -> (sweeps, tris, (feature, t) by numpy)"""
    rng = np.random.RandomState(20250219)
    fam = {"random %g %g %g" % sc: random_family(rng, 10000, *sc) for sc in SCALES}
    fam.update(special_families(rng))
    return {name: (s, t, tri_sweep_np(prepare(s), t[:, 0], t[:, 1], t[:, 2])) for name, (s, t) in fam.items()}


def test_rule_header_includes_no_hip_and_says_what_it_must():
    text = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_sweep_rule.h")).read()
    assert [l.split()[1] for l in text.splitlines() if l.startswith("#include")] == ["<stdint.h>", '"rtk_closest_rule.h"']
    for word in ("__fmul_rn", "__fadd_rn", "__fsub_rn", "__fdiv_rn", "__fsqrt_rn", "-ffp-contract=off", "fp contract(off)", "enormal", "NaN",
                 "CLOSED", "without a margin", "NOT rtk's watertight", "entry time <= time"):
        assert word in text, word
    mk = open(os.path.join(ROOT, "rtk_amd", "csrc", "Makefile")).read()
    assert "rtk_sweep_rule.h" in mk and "rtk_sweep.hip" in mk and "-fhip-fp32-correctly-rounded-divide-sqrt" in mk


def test_driver_matches_numpy_bit_for_bit(driver, cases, tmp_path):
    """The query constants, the time and the feature of every family; every feature, the start overlap and "none" are met"""
    seen = np.zeros(9, np.int64)
    for name, (s, t, (feature, time)) in cases.items():
        q = prepare(s)
        got = run_driver(driver, "q", s.view(np.uint32), tmp_path)
        same_bits(got[:, 0], q.r2); same_bits(got[:, 1], q.dd); same_bits(got[:, 2:5], q.S)
        assert (got[:, 5] == q.live).all(), name
        got = run_driver(driver, "t", np.concatenate([s, t.reshape(-1, 9)], 1).view(np.uint32), tmp_path)
        assert (got[:, 1] == feature).all(), (name, np.nonzero(got[:, 1] != feature)[0][:5])
        same_bits(got[:, 0], time)
        print("%-32s %s" % (name, np.bincount(feature, minlength=9)))
        has = feature != SW_NONE                                             # no time outside [min_t, max_t], whatever the family
        assert (s[has, 6] <= time[has]).all() and (time[has] <= s[has, 7]).all(), (name, np.nonzero(has & ~((s[:, 6] <= time) & (time <= s[:, 7])))[0][:5])
        if name.startswith("random"):
            seen += np.bincount(feature, minlength=9)
            assert q.live.all() and not np.isnan(time).any(), name
    assert (seen > 0).all(), dict(zip(FEATURE_NAMES, seen.tolist()))
    # what the special families are there for
    live = lambda name: prepare(cases[name][0]).live
    assert not live("not live").any() and live("radius 0").all() and live("denormal direction components").all()
    f = cases["a start that touches"][2][0]
    assert (f == SW_START).mean() > 0.9 and (f[::4] == SW_START).all()
    s, _, (f, time) = cases["min_t = max_t"]
    assert set(np.unique(f).tolist()) == {SW_NONE, SW_START}                 # (nothing but the start can happen in an interval of one point)
    assert (time == s[:, 7]).all()
    f = cases["a=b=c"][2][0]
    assert np.isin(f, [SW_NONE, SW_START, 6, 7, 8]).all() and (f >= 6).any()  # a point has no face and no edge
    f = cases["radius 0"][2][0]
    assert (f == SW_FACE).sum() > 50 and (f == SW_NONE).sum() > 50   # (a point meets the face or nothing, but for rounding)
    for name in ("axis-aligned directions", "denormal direction components", "slivers", "a=b", "parallel to an edge", "parallel to the face"):
        f, time = cases[name][2]
        assert (f != SW_NONE).sum() > 10 and (f == SW_NONE).sum() > 10 and not np.isnan(time).any(), name
    f = cases["parallel to the face"][2][0]
    assert (f >= 3).sum() > 50                                               # (beside a face the ball meets edges and vertices)
    f = cases["grazing"][2][0]
    assert 0.1 < (f != SW_NONE).mean() < 0.9                               # on both sides of a discriminant of 0
    s, _, (f, time) = cases["max_t around the time, min_t < 0"]
    assert (s[:, 6] < 0).all() and (f[0::3] == SW_NONE).all()                # below the time: none, also where max_t - te rounds up
    assert (f[1::3] != SW_NONE).sum() > 100 and (time[1::3] == s[1::3, 7]).all()    # at it: the closed interval keeps the hit (t = max_t either way)
    assert (f[2::3] != SW_NONE).sum() > 400 and (time[2::3][f[2::3] != SW_NONE] < s[2::3, 7][f[2::3] != SW_NONE]).all()
    # the order matters: dd summed the other way round differs somewhere (so the comparison can fail)
    q = prepare(cases["random 1 3 0.3"][0])
    assert (((q.D[:, 2] * q.D[:, 2] + q.D[:, 1] * q.D[:, 1]) + q.D[:, 0] * q.D[:, 0]) != q.dd).any()


def test_bound_never_exceeds_the_time(driver, cases, tmp_path):
    """The triangle's own box and random enlargements of it, for every live query: the box's entry time is <= the triangle's
    time, and an empty interval of the box means the triangle has none. None may fail."""
    rng = np.random.RandomState(7)
    total = 0
    for name, (s, t, (feature, time)) in cases.items():
        q = prepare(s)
        lo, hi = tri_box(t[:, 0], t[:, 1], t[:, 2])
        ext = np.maximum((hi - lo).max(1, keepdims=True), np.float32(1e-45))
        for grow in (0.0, 1e-6, 1e-2, 1.0, 30.0):
            with np.errstate(all="ignore"):
                blo = (lo - (rng.uniform(0, 1, lo.shape) * grow).astype(np.float32) * ext).astype(np.float32)
                bhi = (hi + (rng.uniform(0, 1, hi.shape) * grow).astype(np.float32) * ext).astype(np.float32)
            assert (blo <= lo).all() and (bhi >= hi).all()
            some, te = slab_np(q, blo, bhi)
            got = run_driver(driver, "b", np.concatenate([s, blo, bhi], 1).view(np.uint32), tmp_path)
            same_bits(got[:, 0], te)
            assert (got[:, 1] == some).all(), (name, grow)
            ok = q.live
            has = ok & (feature != SW_NONE)
            assert some[has].all(), (name, grow, int((~some[has]).sum()))                  # an empty box: no time below it
            assert (te[has] <= time[has]).all(), (name, grow, int((~(te[has] <= time[has])).sum()))
            assert not np.isnan(te[ok]).any()
            total += int(ok.sum())
    assert total > 300000


def test_better_than_and_skip(driver, tmp_path):
    f = np.array([0.0, -0.0, 1.0, -1.0, np.nextafter(np.float32(1), np.float32(2)), 1e-45, np.inf, np.nan, 3.402823e38], np.float32)
    prims = np.array([0, 1, 7, 0xFFFFFFFE, 0xFFFFFFFF], np.uint32)
    d, pr, b, bp = (x.reshape(-1) for x in np.meshgrid(f, prims, f, prims, indexing="ij"))
    words = np.stack([d.view(np.uint32), pr, b.view(np.uint32), bp], 1)
    got = run_driver(driver, "c", words, tmp_path)[:, 0]
    assert (got == better_np(d, pr, b, bp)).all()
    assert not got[np.isnan(d)].any()                                        # a NaN never beats anything
    assert got[(d == b) & (pr < bp)].all() and not got[(d == b) & (pr >= bp)].any()
    x, y = (v.reshape(-1) for v in np.meshgrid(f, f, indexing="ij"))
    got = run_driver(driver, "s", np.stack([x.view(np.uint32), y.view(np.uint32)], 1), tmp_path)[:, 0]
    with np.errstate(invalid="ignore"):
        assert (got == (x > y)).all()
    assert not got[np.isnan(x)].any() and not got[x == y].any()              # a NaN entry time descends, an equal one too


def _hit64(s, t, dr=0.0, dt=0.0, do=None):
    """float64, with the radius grown by dr, the interval widened by dt at both ends (negative: shrunk) and the origin moved by
    do: is there a time?"""
    q = prepare(s, np.float64)
    q.r = np.maximum(q.r + dr, 0.0)
    q.r2 = q.r * q.r
    q.tmin, q.tmax = q.tmin - dt, q.tmax + dt
    if do is not None:
        q.O = q.O + do
    q.S = q.O + q.D * q.tmin[:, None]
    return tri_sweep_np(q, t[:, 0], t[:, 1], t[:, 2], np.float64)[0] != SW_NONE


def test_accuracy_against_float64():
    """|t - t64| * |D| <= BOUND * 2^-23 * the largest coordinate magnitude involved (origin, triangle, centre at the contact), where
    float32 and float64 both take their time from a feature, on random families at five scales: 3 million pairs, of which about
    half a million have such a time. LEFT OUT, and not measured: slivers (smallest altitude below a hundredth of the longest
    edge), grazing contacts (the direction within 3 degrees of the tangent plane at the contact, where the time's condition
    number exceeds 20) and starts that overlap (their time is the start itself). Pairs whose two times come from different
    features (a contact within rounding of the border between a face, an edge and a vertex) are measured with the others, and
    counted: 52 of the 488320.
    The header's statement: measured 56.71. The asserted bound is that times 2.5, rounded up: 142.
    A pair on which float32 and float64 disagree about hit or none is counted apart. Such a pair is CLEAR if the float64 answer
    stays the same when the radius and both ends of the interval (in the path's units) move by d either way and when the origin
    moves by d along each axis either way, with d = BOUND * 2^-23 of the largest coordinate magnitude: the position error that
    the assertion above allows the float32 evaluation, whatever the radius and the triangle's size are. Then no discriminant,
    no interval test and no region test of the float64 evaluation is within that rounding of its threshold. (A radius below d
    is itself within rounding of the coordinates; there the smaller radius of the move is 0.) No clear pair may disagree.
    Measured: hit / none differs on 13 of the 3 million pairs, none of them clear."""
    BOUND = 142.0
    rng = np.random.RandomState(99)
    worst, evaluated, pairs, switched, disagree, disagree_clear = 0.0, 0, 0, 0, 0, 0
    for sc in SCALES:
        for _ in range(3):
            s, t = random_family(rng, 200000, *sc)
            f32, t32 = tri_sweep_np(prepare(s), t[:, 0], t[:, 1], t[:, 2])
            q = prepare(s, np.float64)
            T = t.astype(np.float64)
            f64, t64 = tri_sweep_np(q, T[:, 0], T[:, 1], T[:, 2], np.float64)
            c = centre_np(q, t64)
            mag = np.maximum(np.maximum(np.abs(q.O).max(1), np.abs(T).reshape(-1, 9).max(1)), np.where(f64 != SW_NONE, np.abs(c).max(1), 0))
            dlen = np.sqrt(q.dd)
            evaluated += len(s)
            # hit or none
            dis = np.nonzero((f32 != SW_NONE) != (f64 != SW_NONE))[0]
            if len(dis):
                d = mag[dis] * BOUND * 2.0 ** -23
                base = f64[dis] != SW_NONE
                moves = [dict(dr=-d, dt=-d / dlen[dis]), dict(dr=d, dt=d / dlen[dis])]
                moves += [dict(do=np.eye(3)[k] * d[:, None] * sign) for k in range(3) for sign in (-1.0, 1.0)]
                clear = np.all([_hit64(s[dis], T[dis], **m) == base for m in moves], 0)
                disagree += len(dis); disagree_clear += int(clear.sum())
            # the time
            e = np.stack([T[:, 1] - T[:, 0], T[:, 2] - T[:, 1], T[:, 0] - T[:, 2]], 1)
            area2 = np.linalg.norm(np.cross(e[:, 0], -e[:, 2]), axis=1)
            longest = np.linalg.norm(e, axis=2).max(1)
            sliver = area2 / longest < 0.01 * longest
            qq = tri_np(c, T[:, 0], T[:, 1], T[:, 2], np.float64)[3]
            normal = np.where((q.r > 0)[:, None], c - qq, np.cross(e[:, 0], -e[:, 2]))
            with np.errstate(all="ignore"):
                cos = np.abs((normal * q.D).sum(1)) / (np.linalg.norm(normal, axis=1) * dlen)
                both = (f32 > SW_START) & (f64 > SW_START) & ~sliver & (cos >= 0.05)
                use = both
                err = np.abs(t32.astype(np.float64) - t64) * dlen / mag
            pairs += int(use.sum()); switched += int((both & (f32 != f64)).sum())
            print("scales %s: %d pairs, worst error %.2f * 2^-23 of the largest coordinate; another feature on %d; hit / none differs on %d"
                  % (sc, int(use.sum()), err[use].max() * 2.0 ** 23, int((both & (f32 != f64)).sum()), len(dis)))
            worst = max(worst, err[use].max())
    print("worst %.2f * 2^-23 over %d pairs of %d; another feature on %d; hit / none differs on %d pairs, %d of them clear"
          % (worst * 2.0 ** 23, pairs, evaluated, switched, disagree, disagree_clear))
    assert evaluated >= 3000000 and pairs > 400000
    assert disagree_clear == 0
    assert worst <= BOUND * 2.0 ** -23


def test_header_symbols_sizes_and_argtypes(api):
    from rtk_amd import types
    text = open(os.path.join(ROOT, "include", "rtk_amd.h")).read()
    for word in ("typedef struct rtk_sphere_sweep { float origin[3], direction[3], min_t, max_t, radius; } rtk_sphere_sweep;",
                 "int rtk_dev_sweep_spheres(const rtk_dev_scene *ds, const rtk_sphere_sweep *d_sweeps, size_t num_sweeps, const rtk_ray_list *list,",
                 "int rtk_dev_sweep_spheres_any(", "int rtk_dev_sweep_spheres_counted(", "uint32_t rtk_amd_sweep_stack_entries(void);",
                 "LOWEST PRIMITIVE ID AMONG EQUAL TIMES", "NOT rtk's watertight ray test", "CLOSED interval", "d_after is refused"):
        assert word in text, word
    check = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_layout_check.h")).read()
    assert "sizeof(rtk_sphere_sweep) == 36" in check
    assert types.SPHERE_SWEEP_DTYPE.itemsize == 36 and types.SPHERE_SWEEP_DTYPE.names == ("origin", "direction", "min_t", "max_t", "radius")
    assert types.SPHERE_SWEEP_DTYPE.fields["min_t"][1] == 24 and types.SPHERE_SWEEP_DTYPE.fields["radius"][1] == 32
    L = api.lib()
    for name in ("rtk_dev_sweep_spheres", "rtk_dev_sweep_spheres_any", "rtk_dev_sweep_spheres_counted", "rtk_amd_sweep_stack_entries"):
        assert name in api.RTK_AMD_H_SYMBOLS and hasattr(L, name), name
    assert L.rtk_dev_sweep_spheres.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(api.RayList), C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.POINTER(api.DevFilter), C.c_void_p]
    assert L.rtk_dev_sweep_spheres_any.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(api.RayList), C.c_void_p, C.POINTER(api.DevFilter), C.c_void_p]
    assert L.rtk_dev_sweep_spheres_counted.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(api.DevFilter),
                                                        C.POINTER(api.TraceCounters)]
    assert L.rtk_dev_sweep_spheres.restype == C.c_int and L.rtk_dev_sweep_spheres_any.restype == C.c_int and L.rtk_dev_sweep_spheres_counted.restype == C.c_int
    assert L.rtk_amd_sweep_stack_entries.restype == C.c_uint32 and 1 <= L.rtk_amd_sweep_stack_entries() <= 64
    for name in ("sweep_spheres", "sweep_spheres_device", "sweep_spheres_any_device", "sweep_spheres_counted", "path_blocked"):
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

    def dev_filter(**kw):
        f = api.DevFilter()
        f.struct_size = C.sizeof(api.DevFilter)
        for k, v in kw.items():
            setattr(f, k, v)
        return f
    bad_lists = [C.byref(ray_list(struct_size=8)), C.byref(ray_list(flags=1)), C.byref(ray_list(d_count=None))]
    bad_filters = [C.byref(dev_filter(struct_size=16)), C.byref(dev_filter(d_after=dummy.value)), C.byref(dev_filter(d_mesh_mask=dummy.value))]
    # the closest form: (ds, sweeps, n, list, records, points, centres, filter, stream)
    for args in [(None, dummy, 4, None, dummy, None, None, None, None), (dummy, None, 4, None, dummy, None, None, None, None),
                 (dummy, dummy, 4, None, None, dummy, dummy, None, None), (dummy, dummy, 1 << 32, None, dummy, None, None, None, None),
                 (dummy, dummy, 1 << 32, C.byref(ray_list()), dummy, None, None, None, None)] \
            + [(dummy, dummy, 4, l, dummy, None, None, None, None) for l in bad_lists] \
            + [(dummy, dummy, 4, None, dummy, None, None, f, None) for f in bad_filters]:
        assert L.rtk_dev_sweep_spheres(*args) == ERR_BAD_ARG, args
        assert "rtk_dev_sweep_spheres:" in api.last_error()
    assert "d_after" in api.last_error() or "mesh mask" in api.last_error()
    assert L.rtk_dev_sweep_spheres(dummy, dummy, 4, None, dummy, None, None, bad_filters[1], None) == ERR_BAD_ARG and "d_after" in api.last_error()
    # the any-hit form: (ds, sweeps, n, list, blocked, filter, stream)
    for args in [(None, dummy, 4, None, dummy, None, None), (dummy, None, 4, None, dummy, None, None), (dummy, dummy, 4, None, None, None, None),
                 (dummy, dummy, 1 << 32, None, dummy, None, None)] + [(dummy, dummy, 4, l, dummy, None, None) for l in bad_lists] \
            + [(dummy, dummy, 4, None, dummy, f, None) for f in bad_filters]:
        assert L.rtk_dev_sweep_spheres_any(*args) == ERR_BAD_ARG, args
        assert "rtk_dev_sweep_spheres_any:" in api.last_error()
    # the counting form: (ds, sweeps, n, records, points, centres, filter, counters)
    ctr = api.TraceCounters()
    for args in [(dummy, dummy, 4, dummy, None, None, None, None), (None, dummy, 4, dummy, None, None, None, C.byref(ctr)),
                 (dummy, None, 4, dummy, None, None, None, C.byref(ctr)), (dummy, dummy, 4, None, None, None, None, C.byref(ctr)),
                 (dummy, dummy, 1 << 32, dummy, None, None, None, C.byref(ctr)), (dummy, dummy, 4, dummy, None, None, bad_filters[1], C.byref(ctr))]:
        assert L.rtk_dev_sweep_spheres_counted(*args) == ERR_BAD_ARG, args
        assert "rtk_dev_sweep_spheres_counted" in api.last_error()
    ctr.rays = 5
    assert L.rtk_dev_sweep_spheres_counted(dummy, None, 0, None, None, None, None, C.byref(ctr)) == 0 and ctr.rays == 0
    # no queries: nothing to do, nothing launched
    assert L.rtk_dev_sweep_spheres(dummy, None, 0, None, None, None, None, None, None) == 0
    assert L.rtk_dev_sweep_spheres(dummy, dummy, 0, C.byref(ray_list()), dummy, dummy, dummy, C.byref(dev_filter()), None) == 0
    assert L.rtk_dev_sweep_spheres_any(dummy, None, 0, None, None, None, None) == 0
