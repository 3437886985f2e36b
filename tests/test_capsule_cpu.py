"""Capsule sweeps without a GPU: the rule of rtk_amd/csrc/rtk_capsule_rule.h, run by tests/capsule_rule_driver.cpp under the
address and undefined-behaviour sanitizers, against numpy float32 arithmetic in the stated order (tests/capsule_ref.py), bit for
bit; the entry time of a box against the time of every triangle inside it; the accuracy statement against float64; the rows
without a half axis against the sphere sweep's reference; and the parts of the interface that need no device -- header text,
symbols, struct sizes, argtypes, the refusals decided before any HIP call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import sweep_ref
from tests.capsule_ref import (CP_EDGE, CP_FACE, CP_FEATURES, CP_NONE, CP_START, CP_VERTEX, FEATURE_NAMES, ITEM_EDGE, ITEM_END0, ITEM_END1,
                               ITEM_PIERCE, better_np, centre_np, distance_np, finish, prepare, record_np, slab_np, tri_capsule_np)
from tests.closest_ref import tri_box
from tests.test_sweep_cpu import SCALES, same_bits
from tests.test_sweep_cpu import random_family as sphere_family

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_BAD_ARG = -2
RTK_INF = np.float32(3.402823e+38)
# measured by test_accuracy_against_float64: 25.50; times 2.5, rounded up
BOUND = 64.0


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """The driver built against the rule headers alone (no HIP include path, -Wall -Werror, no FMA contraction as in the library)
    with both sanitizers. -O2 and -mfma: a compiler that were allowed to contract would do it here."""
    exe = str(tmp_path_factory.mktemp("capsule_rule") / "capsule_rule_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-mfma", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "rtk_amd", "csrc"), os.path.join(ROOT, "tests", "capsule_rule_driver.cpp"), "-o", exe])
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
    hexes = {"q": 14, "b": 1, "t": 1, "r": 9, "c": 0, "s": 0}[kind]
    return np.array([[int(w, 16) if k < hexes else int(w) for k, w in enumerate(line.split())] for line in lines[:len(words)]], np.int64)


def make_sweeps(origin, direction, min_t, max_t, radius, half):
    n = len(origin)
    s = np.zeros((n, 12), np.float32)
    s[:, 0:3], s[:, 3:6], s[:, 9:12] = origin, direction, half
    s[:, 6], s[:, 7], s[:, 8] = min_t, max_t, radius
    return s


def random_family(rng, n, tri_scale, dist, rmax):
    """tests/test_sweep_cpu.py's family with a half axis: triangles of the given size about the origin; a half axis in a random
    direction, up to four times the largest radius long; paths from `dist` away towards a point of the prism the triangle sweeps
    out along the half axis (inside the triangle or a little outside, anywhere along the axis or a little beyond), lifted by up
    to two radii, so that faces, edges, vertices and a miss are met; a tenth start within the radius; max_t without a limit,
    beyond the contact or short of it."""
    t = (rng.standard_normal((n, 3, 3)) * tri_scale).astype(np.float32)
    w = rng.uniform(-0.7, 1.7, (n, 2))
    r = (rng.uniform(0, 1, n) ** 2 * rmax).astype(np.float32)
    h = rng.standard_normal((n, 3))
    h *= (rng.uniform(0, 1, (n, 1)) ** 2 * 4.0 * rmax) / np.linalg.norm(h, axis=1, keepdims=True)
    aim = t[:, 0] + (t[:, 1] - t[:, 0]) * w[:, :1] + (t[:, 2] - t[:, 0]) * w[:, 1:] + h * rng.uniform(-1.3, 1.3, (n, 1)) \
        + rng.standard_normal((n, 3)) * r[:, None] * rng.uniform(0, 1.2, (n, 1))
    away = rng.standard_normal((n, 3))
    away /= np.linalg.norm(away, axis=1, keepdims=True)
    near = rng.uniform(0, 1, n) < 0.1
    o = aim + away * np.where(near, r * rng.uniform(0, 1.5, n), dist * rng.uniform(0.3, 1.5, n))[:, None]
    d = (aim - o) * rng.uniform(0.4, 2.5, (n, 1)) + rng.standard_normal((n, 3)) * 1e-3 * dist
    max_t = np.where(rng.uniform(0, 1, n) < 0.5, RTK_INF, rng.uniform(0.2, 4.0, n)).astype(np.float32)
    min_t = np.where(rng.uniform(0, 1, n) < 0.8, 0.0, rng.uniform(-1.0, 0.15, n)).astype(np.float32)
    return make_sweeps(o, d, min_t, max_t, r, h), t


def inside_points(rng, t):
    n = len(t)
    w = rng.uniform(0, 1, (n, 2)); w[w.sum(1) > 1] = 1 - w[w.sum(1) > 1]
    return t[:, 0] + (t[:, 1] - t[:, 0]) * w[:, :1] + (t[:, 2] - t[:, 0]) * w[:, 1:]


def special_families(rng):
    """name -> (sweeps [n, 12], tris [n, 3, 3]) float32"""
    fam = {}
    n = 1500
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
    s, t = random_family(rng, n, 1.0, 3.0, 0.5)
    zero = np.arange(n) % 3
    s[np.arange(n), 3 + zero] = 0.0
    s[np.arange(n)[::2], 3 + (zero[::2] + 1) % 3] = 0.0
    s[::5, 3 + zero[::5]] = -0.0
    fam["axis-aligned directions"] = (s, t)
    s, t = random_family(rng, n, 1.0, 3.0, 0.3)
    s[:, 8] = 0.0
    s[::7, 8] = -0.0
    fam["radius 0"] = (s, t)
    s, t = random_family(rng, n, 1.0, 3.0, 0.3)
    s[:, 9:12] = 0.0
    s[::7, 9:12] = -0.0
    fam["half_axis 0"] = (s, t)
    s, t = random_family(rng, 600, 1.0, 3.0, 0.3)
    s[:, 8:12] = 0.0
    fam["a point"] = (s, t)
    i = np.arange(n)
    s, t = random_family(rng, n, 1.0, 3.0, 0.3)
    s[:, 9:12] = (t[i, (i + 1) % 3] - t[i, i % 3]) * rng.uniform(-0.6, 0.6, (n, 1))
    fam["half_axis along an edge"] = (s, t)
    s, t = random_family(rng, n, 1.0, 3.0, 0.3)
    s[:, 9:12] = (t[:, 1] - t[:, 0]) * rng.uniform(-0.5, 0.5, (n, 1)) + (t[:, 2] - t[:, 0]) * rng.uniform(-0.5, 0.5, (n, 1))
    fam["half_axis in the plane"] = (s, t)
    s, t = random_family(rng, n, 1.0, 3.0, 0.3)
    s[:, 9:12] = s[:, 3:6] * rng.uniform(-0.2, 0.2, (n, 1))
    fam["half_axis along the direction"] = (s, t)
    s, t = random_family(rng, 1000, 1.0, 0.3, 0.4)
    s[:, 7] = s[:, 6]
    fam["min_t = max_t"] = (s, t)
    # starts that touch: the axis through the triangle (rows 0 mod 3), an end on the triangle (1 mod 3), within the radius (2 mod 3)
    s, t = random_family(rng, 1200, 1.0, 3.0, 0.3)
    on = inside_points(rng, t)
    s[:, 6] = 0.0
    s[0::3, 0:3] = on[0::3] + s[0::3, 9:12] * rng.uniform(-0.9, 0.9, (400, 1))
    s[1::3, 0:3] = on[1::3] + s[1::3, 9:12] * rng.choice([-1.0, 1.0], (400, 1))
    s[1::6, 9:12] = np.float32(0.25) * np.round(s[1::6, 9:12] * 8)                       # (exactly: an end that IS a vertex)
    s[1::6, 0:3] = t[1::6, 1] + s[1::6, 9:12]
    t[1::6] = np.float32(0.25) * np.round(t[1::6] * 4); s[1::6, 0:3] = t[1::6, 1] + s[1::6, 9:12]
    s[2::3, 0:3] = on[2::3] + s[2::3, 9:12] * rng.uniform(-1, 1, (400, 1)) + rng.standard_normal((400, 3)) * (s[2::3, 8:9] * 0.5)
    fam["a start that touches"] = (s, t)
    # paths parallel to an edge, and parallel to the face at about one radius from the prism
    s, t = random_family(rng, n, 1.0, 3.0, 0.3)
    s[:, 3:6] = (t[i, (i + 1) % 3] - t[i, i % 3]) * rng.uniform(-2, 2, (n, 1))
    fam["parallel to an edge"] = (s, t)
    s, t = random_family(rng, n, 1.0, 3.0, 0.3)
    s[:, 3:6] = (t[:, 1] - t[:, 0]) * rng.uniform(-1, 1, (n, 1)) + (t[:, 2] - t[:, 0]) * rng.uniform(-1, 1, (n, 1))
    nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    lift = np.abs((s[:, 9:12] * nrm).sum(1, keepdims=True)) + s[:, 8:9] * rng.uniform(0.5, 1.5, (n, 1))
    s[:, 0:3] = t.mean(1) - s[:, 3:6] * 1.5 + nrm * lift
    fam["parallel to the face"] = (s, t)
    # max_t at the float32 neighbour below the time, at it and above it (rows 0, 1, 2 mod 3), with min_t < 0: the entry time te
    # is then negative as a rule, and 2. (iv) of the header makes a time that rounds beyond max_t none
    s, t = random_family(rng, 12000, 1.0, 3.0, 0.3)
    s[:, 6], s[:, 7] = rng.uniform(-4.0, -0.5, 12000), RTK_INF
    f, time = tri_capsule_np(prepare(s), t[:, 0], t[:, 1], t[:, 2])
    s, t, time = s[f > CP_START][:1500], t[f > CP_START][:1500], time[f > CP_START][:1500]
    assert len(s) == 1500
    s[0::3, 7] = np.nextafter(time[0::3], np.float32(-np.inf))
    s[1::3, 7] = time[1::3]
    s[2::3, 7] = np.nextafter(time[2::3], np.float32(np.inf))
    fam["max_t around the time, min_t < 0"] = (s, t)
    # queries that are not live
    s, t = random_family(rng, 1050, 1.0, 3.0, 0.3)
    bad = np.array([np.nan, np.inf, -np.inf], np.float32)
    s[np.arange(600), np.arange(600) % 12] = bad[(np.arange(600) // 12) % 3]
    s[600:750, 8] = -np.abs(s[600:750, 8]) - np.float32(1e-30)
    s[750:900, 3:6] = 0.0
    s[750:900:2, 4] = -0.0
    s[900:1050, 7] = np.minimum(s[900:1050, 7], 10.0)
    s[900:1050, 6] = s[900:1050, 7] + 1.0
    fam["not live"] = (s, t)
    return fam


@pytest.fixture(scope="module")
def cases():
    """Every family once: name -> (sweeps, tris, (feature, t) by numpy)"""
    rng = np.random.RandomState(20250220)
    fam = {"random %g %g %g" % sc: random_family(rng, 10000, *sc) for sc in SCALES}
    fam.update(special_families(rng))
    return {name: (s, t, tri_capsule_np(prepare(s), t[:, 0], t[:, 1], t[:, 2])) for name, (s, t) in fam.items()}


def test_rule_header_includes_no_hip_and_says_what_it_must():
    text = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_capsule_rule.h")).read()
    assert [l.split()[1] for l in text.splitlines() if l.startswith("#include")] == ['"rtk_sweep_rule.h"', '"rtk_pair_rule.h"']
    assert "hip" not in text.replace("HIPCC", "").replace("HIP_DEVICE_COMPILE", "").replace("rtk_capsule.hip", "").lower()
    for word in ("THE RESULT DOES NOT DEPEND ON THE TREE", "LOWEST PRIMITIVE ID WINS AMONG EQUAL TIMES", "CLOSED interval", "WITHOUT A MARGIN",
                 "NOT rtk's watertight", "entry time <= time", "IS NOT PROMISED BIT-EQUAL", "THE FIRST AMONG EQUAL", "NaN", "enormal",
                 "NOTHING IS DECIDED BY", "PARALLEL", "rtk_sweep_edge", "rtk_sweep_vertex", "rtk_sweep_entry", "rtk_sweep_centre",
                 "rtk_closest_triangle", "rtk_pair_segments", "rtk_pair_edge_pierces", "rtk_sweep_better", "rtk_sweep_skip",
                 "%.2f * 2^-23" % 25.50, "%d * 2^-23" % BOUND):
        assert word in text, word
    # the feature order, as the numpy restatement has it
    order = [text.index(w) for w in ("FACES     2 .. 9: L, U, ab's two halves, bc's two, ca's two", "EDGES     10 .. 21",
                                     "L's three a- b-, b- c-, c- a-; U's three", "the three lateral ones a- a+, b- b+, c- c+; the three diagonals a- b+, b- c+, c- a+",
                                     "VERTICES  22 .. 27", "a-, b-, c-, a+, b+, c+")]
    assert order == sorted(order)
    assert "{ 0, 1, 2 }, { 3, 4, 5 }, { 1, 4, 0 }, { 3, 0, 4 }, { 2, 5, 1 }, { 4, 1, 5 }, { 0, 3, 2 }, { 5, 2, 3 }" in text
    assert "{ 0, 1 }, { 1, 2 }, { 2, 0 }, { 3, 4 }, { 4, 5 }, { 5, 3 }, { 0, 3 }, { 1, 4 }, { 2, 5 }, { 0, 4 }, { 1, 5 }, { 2, 3 }" in text
    mk = open(os.path.join(ROOT, "rtk_amd", "csrc", "Makefile")).read()
    assert "rtk_capsule_rule.h" in mk and "rtk_capsule.hip" in mk and "-fhip-fp32-correctly-rounded-divide-sqrt" in mk
    kernel = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_capsule.hip")).read()
    assert '#include "rtk_capsule_rule.h"' in kernel and "asm" not in kernel


def test_driver_matches_numpy_bit_for_bit(driver, cases, tmp_path):
    """The query constants, the time and the feature of every family, and the record at that time; every one of the 26 features,
    the start overlap and "none" decide somewhere, and so does every item of the distance walk"""
    seen = np.zeros(CP_FEATURES, np.int64)
    items = np.zeros(ITEM_EDGE + 3, np.int64)
    for name, (s, t, (feature, time)) in cases.items():
        q = prepare(s)
        got = run_driver(driver, "q", s.view(np.uint32), tmp_path)
        same_bits(got[:, 0], q.r2); same_bits(got[:, 1], q.dd); same_bits(got[:, 2:5], q.S); same_bits(got[:, 5:8], q.g)
        same_bits(got[:, 8:11], q.p0); same_bits(got[:, 11:14], q.p1)
        assert (got[:, 14] == q.live).all(), name
        tri_words = t.reshape(-1, 9).view(np.uint32)
        got = run_driver(driver, "t", np.concatenate([s.view(np.uint32), tri_words], 1), tmp_path)
        assert (got[:, 1] == feature).all(), (name, np.nonzero(got[:, 1] != feature)[0][:5], got[:, 1][got[:, 1] != feature][:5], feature[got[:, 1] != feature][:5])
        same_bits(got[:, 0], time)
        print("%-36s %s" % (name, np.bincount(feature, minlength=CP_FEATURES)))
        has = feature != CP_NONE                                             # no time outside [min_t, max_t], whatever the family
        assert (s[has, 6] <= time[has]).all() and (time[has] <= s[has, 7]).all(), name
        seen += np.bincount(feature, minlength=CP_FEATURES)
        if name.startswith("random"):
            assert q.live.all() and not np.isnan(time).any(), name
        # the record at the time (for "none": at max_t, where that is finite arithmetic all the same)
        r = record_np(q, time, t[:, 0], t[:, 1], t[:, 2])
        got = run_driver(driver, "r", np.concatenate([s.view(np.uint32), tri_words, time.view(np.uint32)[:, None]], 1), tmp_path)
        same_bits(got[:, 0], r.dist2); same_bits(got[:, 1], r.u); same_bits(got[:, 2], r.v)
        same_bits(got[:, 3:6], r.qt); same_bits(got[:, 6:9], r.qa)
        assert (got[:, 9] == r.item).all(), name
        items += np.bincount(r.item[has], minlength=len(items))
    print(dict(zip(FEATURE_NAMES, seen.tolist())), items)
    assert (seen > 0).all(), dict(zip(FEATURE_NAMES, seen.tolist()))
    assert (items[ITEM_PIERCE:] > 0).all(), items
    # what the special families are there for
    live = lambda name: prepare(cases[name][0]).live
    assert not live("not live").any() and (cases["not live"][0][:600] != cases["not live"][0][:600]).any()
    for name in ("radius 0", "half_axis 0", "half_axis along an edge", "half_axis in the plane", "half_axis along the direction"):
        f, time = cases[name][2]
        assert live(name).all() and (f > CP_START).sum() > 50 and (f == CP_NONE).sum() > 50 and not np.isnan(time).any(), name
    f, time = cases["a point"][2]                                            # (a point meets a face or nothing, but for rounding)
    assert live("a point").all() and (f > CP_START).sum() > 10 and (f == CP_NONE).sum() > 50 and not np.isnan(time).any()
    s, t, (f, time) = cases["a start that touches"]
    assert (f == CP_START).mean() > 0.9 and (f[0::3] == CP_START).all() and (f[1::6] == CP_START).all()
    at = distance_np(prepare(s).p0, prepare(s).p1, t[:, 0], t[:, 1], t[:, 2])
    assert (at.item[0::3] == ITEM_PIERCE).mean() > 0.9 and (at.dist2[0::3][at.item[0::3] == ITEM_PIERCE] == 0).all()
    assert (at.dist2[1::6] == 0).all() and np.isin(at.item[1::6], [ITEM_END0, ITEM_END1]).all()     # an end that is a vertex, exactly
    s, _, (f, time) = cases["min_t = max_t"]
    assert set(np.unique(f).tolist()) == {CP_NONE, CP_START}                 # (nothing but the start can happen in an interval of one point)
    assert (time == s[:, 7]).all()
    f = cases["a=b=c"][2][0]                                                 # a point swept along h is a segment: no face
    assert not np.isin(f, np.arange(CP_FACE, CP_EDGE)).any() and (f >= CP_EDGE).any()
    f = cases["half_axis 0"][2][0]                                           # L comes before U, an edge of L before its twins
    assert np.isin(f, [CP_NONE, CP_START, CP_FACE, CP_EDGE, CP_EDGE + 1, CP_EDGE + 2, CP_VERTEX, CP_VERTEX + 1, CP_VERTEX + 2]).all()
    for name in ("axis-aligned directions", "slivers", "a=b", "parallel to an edge", "parallel to the face"):
        f, time = cases[name][2]
        assert (f != CP_NONE).sum() > 10 and (f == CP_NONE).sum() > 10 and not np.isnan(time).any(), name
    s, _, (f, time) = cases["max_t around the time, min_t < 0"]
    assert (s[:, 6] < 0).all() and (f[0::3] == CP_NONE).all()                # below the time: none, also where max_t - te rounds up
    assert (f[1::3] != CP_NONE).sum() > 100 and (time[1::3] == s[1::3, 7]).all()    # at it: the closed interval keeps the hit
    assert (f[2::3] != CP_NONE).sum() > 400 and (time[2::3][f[2::3] != CP_NONE] < s[2::3, 7][f[2::3] != CP_NONE]).all()
    # a negative entry time is met
    s, t, _ = cases["max_t around the time, min_t < 0"]
    assert (slab_np(prepare(s), *tri_box(t[:, 0], t[:, 1], t[:, 2]))[1] < 0).sum() > 100
    # the order matters: g summed with the sign kept differs somewhere (so the comparison can fail)
    q = prepare(cases["random 1 3 0.3"][0])
    assert ((q.r[:, None] + q.h) != q.g).any()


def test_bound_never_exceeds_the_time(driver, cases, tmp_path):
    """The triangle's own box and random enlargements of it, for every live query: the box's entry time is <= the triangle's
    time, and an empty interval of the box means the triangle has none. Exactly: none may fail."""
    rng = np.random.RandomState(7)
    total = 0
    for name, (s, t, (feature, time)) in cases.items():
        q = prepare(s)
        lo, hi = tri_box(t[:, 0], t[:, 1], t[:, 2])
        ext = np.maximum((hi - lo).max(1, keepdims=True), np.float32(1e-45))
        own_some, own_te = slab_np(q, lo, hi)
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
            assert some[ok & own_some].all() and (te[ok & own_some] <= own_te[ok & own_some]).all(), (name, grow)   # the slab is monotone in the box
            has = ok & (feature != CP_NONE)
            assert some[has].all(), (name, grow, int((~some[has]).sum()))                  # an empty box: no time below it
            assert (te[has] <= time[has]).all(), (name, grow, int((~(te[has] <= time[has])).sum()))
            assert not np.isnan(te[ok]).any()
            total += int(ok.sum())
    assert total > 300000


def test_better_than_and_skip(driver, tmp_path):
    """rtk_sweep_better and rtk_sweep_skip as this rule uses them, through this rule's driver"""
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


def _moved(s, dtype, dr=0.0, dt=0.0, do=None):
    q = prepare(s, dtype)
    q.r = np.maximum(q.r + dr, 0.0)
    q.tmin, q.tmax = q.tmin - dt, q.tmax + dt
    if do is not None:
        q.O = q.O + do
    return finish(q)


def _hit64(s, t, **move):
    """float64, with the radius grown by dr, the interval widened by dt at both ends (negative: shrunk) and the origin moved by
    do: is there a time?"""
    return tri_capsule_np(_moved(s, np.float64, **move), t[:, 0], t[:, 1], t[:, 2], np.float64)[0] != CP_NONE


def _clear(s, T, d, dlen, hit64=_hit64):
    """tests/test_sweep_cpu.py's criterion: the float64 answer stays the same when the radius and both ends of the interval (in
    the path's units) move by d either way and when the origin moves by d along each axis either way"""
    base = hit64(s, T)
    moves = [dict(dr=-d, dt=-d / dlen), dict(dr=d, dt=d / dlen)]
    moves += [dict(do=np.eye(3)[k] * d[:, None] * sign) for k in range(3) for sign in (-1.0, 1.0)]
    return np.all([hit64(s, T, **m) == base for m in moves], 0)


def _is_sliver(T):
    """float64: tests/test_sweep_cpu.py's criterion, the triangle's smallest altitude below a hundredth of its longest edge"""
    e = np.stack([T[:, 1] - T[:, 0], T[:, 2] - T[:, 1], T[:, 0] - T[:, 2]], 1)
    area2 = np.linalg.norm(np.cross(e[:, 0], -e[:, 2]), axis=1)
    longest = np.linalg.norm(e, axis=2).max(1)
    return area2 / longest < 0.01 * longest


@pytest.fixture(scope="module")
def against_float64():
    """The 3 million random cases in float32 and in float64, evaluated once for the two tests below"""
    rng = np.random.RandomState(99)
    worst, evaluated, pairs, switched, disagree, disagree_clear = 0.0, 0, 0, 0, 0, 0
    left_out = {"slivers": 0, "grazing": 0, "starts": 0}
    for sc in SCALES:
        for _ in range(3):
            s, t = random_family(rng, 200000, *sc)
            f32, t32 = tri_capsule_np(prepare(s), t[:, 0], t[:, 1], t[:, 2])
            q = prepare(s, np.float64)
            T = t.astype(np.float64)
            f64, t64 = tri_capsule_np(q, T[:, 0], T[:, 1], T[:, 2], np.float64)
            c = centre_np(q, t64)
            ends = np.maximum(np.abs(c - q.h).max(1), np.abs(c + q.h).max(1))
            mag = np.maximum(np.maximum(np.abs(q.O).max(1), np.abs(T).reshape(-1, 9).max(1)), np.where(f64 != CP_NONE, ends, 0))
            dlen = np.sqrt(q.dd)
            evaluated += len(s)
            dis = np.nonzero((f32 != CP_NONE) != (f64 != CP_NONE))[0]
            if len(dis):
                clear = _clear(s[dis], T[dis], mag[dis] * BOUND * 2.0 ** -23, dlen[dis])
                disagree += len(dis); disagree_clear += int(clear.sum())
            sliver = _is_sliver(T)
            r = record_np(q, t64, T[:, 0], T[:, 1], T[:, 2], np.float64)
            normal = r.qa - r.qt
            with np.errstate(all="ignore"):
                cos = np.abs((normal * q.D).sum(1)) / (np.linalg.norm(normal, axis=1) * dlen)
                both = (f32 > CP_START) & (f64 > CP_START)
                use = both & ~sliver & (cos >= 0.05)
                err = np.abs(t32.astype(np.float64) - t64) * dlen / mag
            left_out["slivers"] += int((both & sliver).sum()); left_out["grazing"] += int((both & ~sliver & ~(cos >= 0.05)).sum())
            left_out["starts"] += int(((f32 == CP_START) | (f64 == CP_START)).sum())
            pairs += int(use.sum()); switched += int((use & (f32 != f64)).sum())
            print("scales %s: %d pairs, worst error %.2f * 2^-23 of the largest coordinate; another feature on %d; hit / none differs on %d"
                  % (sc, int(use.sum()), err[use].max() * 2.0 ** 23, int((use & (f32 != f64)).sum()), len(dis)))
            worst = max(worst, err[use].max())
    print("worst %.2f * 2^-23 over %d pairs of %d; left out %s; another feature on %d; hit / none differs on %d pairs, %d of them clear"
          % (worst * 2.0 ** 23, pairs, evaluated, left_out, switched, disagree, disagree_clear))
    return dict(worst=worst, evaluated=evaluated, pairs=pairs, disagree=disagree, clear=disagree_clear)


def test_accuracy_against_float64(against_float64):
    """|t - t64| * |D| <= BOUND * 2^-23 * the largest coordinate magnitude involved (origin, triangle, the capsule's two end points at
    the contact), where float32 and float64 both take their time from a feature, on the random families at the five scales of
    tests/test_sweep_cpu.py: 3 million cases, of which 0.72 million are measured. LEFT OUT, and not measured, as there:
    slivers (the triangle's smallest altitude below a hundredth of its longest edge; the prism's lateral faces are NOT looked
    at: a half axis down to nothing beside the edges is measured with the rest), grazing contacts (the direction within 3
    degrees of the tangent plane at the contact: the cosine between the direction and the contact normal -- the axis point minus
    the triangle point of the float64 record -- below 0.05) and starts that overlap (their time is the start itself). Each
    exclusion is counted and printed: 488, 4846 and 54495. Pairs whose two times come from different features are measured
    with the others, and counted: 228.
    The header's statement: measured 25.50. The asserted bound is that times 2.5, rounded up: 64."""
    r = against_float64
    assert r["evaluated"] >= 3000000 and r["pairs"] > 400000
    assert r["worst"] <= BOUND * 2.0 ** -23


def test_no_clear_pair_disagrees_with_float64(against_float64):
    """A pair on which float32 and float64 disagree about hit or none is CLEAR by the sphere test's criterion (_clear) with
    d = BOUND * 2^-23 of the largest coordinate magnitude. No clear pair may disagree. Measured: hit / none differs on none of
    the 3 million cases. (With the lateral faces named from the other end of the edge -- (p-, q-, q+) -- it differed on 18,
    17 of them clear: the rule header says under FACES why the corner a face is named from matters.)"""
    r = against_float64
    print("hit / none differs on %d, %d of them clear" % (r["disagree"], r["clear"]))
    assert r["clear"] == 0


def test_no_half_axis_against_the_sphere_reference():
    """half_axis == 0 against tests/sweep_ref.py on the sphere test's own families: the share of identical (feature class, time)
    rows is printed; where both have a time from a feature the times agree within the asserted accuracy bound (they are the
    same expressions: L is the triangle itself); hit / none may differ only on rows the clear criterion does not call clear."""
    rng = np.random.RandomState(5)
    rows = same = differ = differ_clear = 0
    for sc in SCALES:
        s9, t = sphere_family(rng, 40000, *sc)
        s = np.concatenate([s9, np.zeros((len(s9), 3), np.float32)], 1)
        fs, ts = sweep_ref.tri_sweep_np(sweep_ref.prepare(s9), t[:, 0], t[:, 1], t[:, 2])
        fc, tc = tri_capsule_np(prepare(s), t[:, 0], t[:, 1], t[:, 2])
        cls = np.where(fc >= CP_VERTEX, 2, np.where(fc >= CP_EDGE, 1, np.where(fc >= CP_FACE, 0, -1)))
        cls_s = np.where(fs >= sweep_ref.SW_VERTEX_A, 2, np.where(fs >= sweep_ref.SW_EDGE_AB, 1, np.where(fs >= sweep_ref.SW_FACE, 0, -1)))
        rows += len(s)
        same += int(((fs == sweep_ref.SW_NONE) == (fc == CP_NONE)).__and__((fs == sweep_ref.SW_START) == (fc == CP_START)).__and__(cls == cls_s)
                    .__and__(ts.view(np.uint32) == tc.view(np.uint32)).sum())
        both = (fs > sweep_ref.SW_START) & (fc > CP_START)
        q = prepare(s, np.float64)
        T = t.astype(np.float64)
        c = centre_np(q, tc.astype(np.float64))
        mag = np.maximum(np.maximum(np.abs(q.O).max(1), np.abs(T).reshape(-1, 9).max(1)), np.abs(c).max(1))
        dlen = np.sqrt(q.dd)
        err = np.abs(ts.astype(np.float64) - tc) * dlen / mag
        assert both.sum() > 1000 and (err[both] <= BOUND * 2.0 ** -23).all(), (sc, err[both].max() * 2.0 ** 23)
        dis = np.nonzero((fs != sweep_ref.SW_NONE) != (fc != CP_NONE))[0]
        if len(dis):
            differ += len(dis)
            differ_clear += int(_clear(s[dis], T[dis], mag[dis] * BOUND * 2.0 ** -23, dlen[dis]).sum())
    print("half_axis == 0 against the sphere reference: %d of %d rows identical (%.4f %%); hit / none differs on %d, %d of them clear"
          % (same, rows, 100.0 * same / rows, differ, differ_clear))
    assert differ_clear == 0


def test_header_symbols_sizes_and_argtypes(api):
    from rtk_amd import types
    text = open(os.path.join(ROOT, "include", "rtk_amd.h")).read()
    for word in ("typedef struct rtk_capsule_sweep { float origin[3], direction[3], min_t, max_t, radius, half_axis[3]; } rtk_capsule_sweep;",
                 "int rtk_dev_sweep_capsules(const rtk_dev_scene *ds, const rtk_capsule_sweep *d_sweeps, size_t num_sweeps, const rtk_ray_list *list,",
                 "int rtk_dev_sweep_capsules_any(", "int rtk_dev_sweep_capsules_counted(", "uint32_t rtk_amd_capsule_stack_entries(void);",
                 "half_axis == 0 IS NOT PROMISED", "A SLOT\n * THAT IS NOT LISTED IS NOT WRITTEN", "d_axis_points"):
        assert word in text, word
    section = text[text.index("---- Capsule sweeps"):text.index("uint32_t rtk_amd_capsule_stack_entries")]
    for word in ("LOWEST PRIMITIVE ID AMONG EQUAL TIMES", "NOT rtk's watertight ray test", "CLOSED interval", "d_after is refused",
                 "THE RESULT DOES NOT DEPEND ON THE TREE", "rtk_dev_trace_status", "num_sweeps == 0 is", "rtk_mgpu_scene(m, i)", "non-finite vertex coordinates",
                 "Asynchronous on `stream`"):
        assert word in section.replace("\n * ", " "), word
    check = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_layout_check.h")).read()
    assert "sizeof(rtk_capsule_sweep) == 48" in check and "offsetof(rtk_capsule_sweep, half_axis) == 36" in check
    dt = types.CAPSULE_SWEEP_DTYPE
    assert dt.itemsize == 48 and dt.names == ("origin", "direction", "min_t", "max_t", "radius", "half_axis")
    assert [dt.fields[k][1] for k in dt.names] == [0, 12, 24, 28, 32, 36]
    L = api.lib()
    for name in ("rtk_dev_sweep_capsules", "rtk_dev_sweep_capsules_any", "rtk_dev_sweep_capsules_counted", "rtk_amd_capsule_stack_entries"):
        assert name in api.RTK_AMD_H_SYMBOLS and hasattr(L, name), name
    assert L.rtk_dev_sweep_capsules.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(api.RayList), C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.POINTER(api.DevFilter), C.c_void_p]
    assert L.rtk_dev_sweep_capsules_any.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(api.RayList), C.c_void_p, C.POINTER(api.DevFilter), C.c_void_p]
    assert L.rtk_dev_sweep_capsules_counted.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(api.DevFilter),
                                                         C.POINTER(api.TraceCounters)]
    assert L.rtk_dev_sweep_capsules.restype == C.c_int and L.rtk_dev_sweep_capsules_any.restype == C.c_int and L.rtk_dev_sweep_capsules_counted.restype == C.c_int
    assert L.rtk_amd_capsule_stack_entries.restype == C.c_uint32 and 1 <= L.rtk_amd_capsule_stack_entries() <= 64
    for name in ("sweep_capsules", "sweep_capsules_device", "sweep_capsules_any_device", "sweep_capsules_counted", "capsule_path_blocked"):
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
    # the closest form: (ds, sweeps, n, list, records, points, axis_points, filter, stream)
    for args in [(None, dummy, 4, None, dummy, None, None, None, None), (dummy, None, 4, None, dummy, None, None, None, None),
                 (dummy, dummy, 4, None, None, dummy, dummy, None, None), (dummy, dummy, 1 << 32, None, dummy, None, None, None, None),
                 (dummy, dummy, 1 << 32, C.byref(ray_list()), dummy, None, None, None, None)] \
            + [(dummy, dummy, 4, l, dummy, None, None, None, None) for l in bad_lists] \
            + [(dummy, dummy, 4, None, dummy, None, None, f, None) for f in bad_filters]:
        assert L.rtk_dev_sweep_capsules(*args) == ERR_BAD_ARG, args
        assert "rtk_dev_sweep_capsules:" in api.last_error()
    assert L.rtk_dev_sweep_capsules(dummy, dummy, 4, None, dummy, None, None, bad_filters[1], None) == ERR_BAD_ARG and "d_after" in api.last_error()
    assert L.rtk_dev_sweep_capsules(dummy, dummy, 4, None, dummy, None, None, bad_filters[2], None) == ERR_BAD_ARG and "mesh mask" in api.last_error()
    # the any-hit form: (ds, sweeps, n, list, blocked, filter, stream)
    for args in [(None, dummy, 4, None, dummy, None, None), (dummy, None, 4, None, dummy, None, None), (dummy, dummy, 4, None, None, None, None),
                 (dummy, dummy, 1 << 32, None, dummy, None, None)] + [(dummy, dummy, 4, l, dummy, None, None) for l in bad_lists] \
            + [(dummy, dummy, 4, None, dummy, f, None) for f in bad_filters]:
        assert L.rtk_dev_sweep_capsules_any(*args) == ERR_BAD_ARG, args
        assert "rtk_dev_sweep_capsules_any:" in api.last_error()
    # the counting form: (ds, sweeps, n, records, points, axis_points, filter, counters)
    ctr = api.TraceCounters()
    for args in [(dummy, dummy, 4, dummy, None, None, None, None), (None, dummy, 4, dummy, None, None, None, C.byref(ctr)),
                 (dummy, None, 4, dummy, None, None, None, C.byref(ctr)), (dummy, dummy, 4, None, None, None, None, C.byref(ctr)),
                 (dummy, dummy, 1 << 32, dummy, None, None, None, C.byref(ctr)), (dummy, dummy, 4, dummy, None, None, bad_filters[1], C.byref(ctr))]:
        assert L.rtk_dev_sweep_capsules_counted(*args) == ERR_BAD_ARG, args
        assert "rtk_dev_sweep_capsules_counted" in api.last_error()
    ctr.rays = 5
    assert L.rtk_dev_sweep_capsules_counted(dummy, None, 0, None, None, None, None, C.byref(ctr)) == 0 and ctr.rays == 0
    # no queries: nothing to do, nothing launched
    assert L.rtk_dev_sweep_capsules(dummy, None, 0, None, None, None, None, None, None) == 0
    assert L.rtk_dev_sweep_capsules(dummy, dummy, 0, C.byref(ray_list()), dummy, dummy, dummy, C.byref(dev_filter()), None) == 0
    assert L.rtk_dev_sweep_capsules_any(dummy, None, 0, None, None, None, None) == 0
