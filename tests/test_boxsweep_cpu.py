"""Box sweeps without a GPU: the rule of rtk_amd/csrc/rtk_boxsweep_rule.h, run by tests/boxsweep_rule_driver.cpp under the address
and undefined-behaviour sanitizers, against numpy float32 arithmetic in the stated order (tests/boxsweep_ref.py), bit for bit; the
entry time of a box against the time of every triangle inside it; what the time means, by the static box rule of
tests/box_ref.py; the accuracy statement against float64; and the parts of the interface that need no device -- header text,
symbols, struct sizes, argtypes, the refusals decided before any HIP call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.box_ref import candidate_np
from tests.boxsweep_ref import (AXIS_NAMES, BS_AXES, BS_BOX_X, BS_BOX_Z, BS_EDGE, BS_NONE, BS_NORMAL, BS_START, better_np, centre_np, normal_np,
                                prepare, slab_np, tri_boxsweep_np)
from tests.closest_ref import tri_box
from tests.test_sweep_cpu import SCALES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_BAD_ARG = -2
RTK_INF = np.float32(3.402823e+38)
# |t - t64| * |D| in units of 2^-23 of the largest coordinate magnitude involved: what test_accuracy_against_float64 measured, and
# 2.5 times it, rounded up: the factor of the closest-point, closest-triangle and sphere-sweep statements
MEASURED = 1730.41
BOUND = 4327.0
# the same without grazing contacts (the motion within 3 degrees of the contact plane, where the time's condition number exceeds
# 20) and starts that overlap: what the sphere sweep's statement measures
MEASURED_STEEP = 31.96
BOUND_STEEP = 80.0


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """The driver built against the rule headers alone (no HIP include path, -Wall -Werror, no FMA contraction as in the library)
    with both sanitizers. -O2 and -mfma: a compiler that were allowed to contract would do it here."""
    exe = str(tmp_path_factory.mktemp("boxsweep_rule") / "boxsweep_rule_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-mfma", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "rtk_amd", "csrc"), os.path.join(ROOT, "tests", "boxsweep_rule_driver.cpp"), "-o", exe])
    return exe


def run_driver(exe, kind, words, tmp_path):
    """words uint32 [n, k] -> the driver's output lines as integers [n, m] (hexadecimal words first, then decimal numbers)"""
    path = str(tmp_path / ("cases_%s.txt" % kind))
    with open(path, "w") as f:
        f.write("".join("%s %s\n" % (kind, " ".join("%x" % w for w in row)) for row in words.tolist()))
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    assert lines[len(words)] == "ok"
    hexes = {"q": 3, "b": 2, "t": 4, "c": 0, "s": 0}[kind]
    return np.array([[int(w, 16) if k < hexes else int(w) for k, w in enumerate(line.split())] for line in lines[:len(words)]], np.int64)


def same_bits(got, want):
    """Bit for bit, except where the expected value is NaN: there only "it is NaN" is promised."""
    got = np.ascontiguousarray(got, np.uint32)
    want = np.ascontiguousarray(want, np.float32)
    nan = np.isnan(want)
    assert (np.isnan(got.view(np.float32)) == nan).all()
    bad = (got != want.view(np.uint32)) & ~nan
    assert not bad.any(), (np.argwhere(bad)[:5], got[bad][:5], want.view(np.uint32)[bad][:5])


def make_sweeps(origin, direction, min_t, max_t, half):
    n = len(origin)
    s = np.zeros((n, 11), np.float32)
    s[:, 0:3], s[:, 3:6], s[:, 8:11] = origin, direction, half
    s[:, 6], s[:, 7] = min_t, max_t
    return s


def random_family(rng, n, tri_scale, dist, hmax):
    """tests/test_sweep_cpu.py's family with three half extents in the place of the radius, each drawn as its radii are; a
    seventh of the boxes are exactly 0 on one, two or all three axes. Triangles of the given size about the origin; paths from
    `dist` away towards a point of the triangle's plane inside the triangle or a little outside, lifted by up to two of the
    largest half extent; a tenth start within it; max_t without a limit, beyond the contact or short of it."""
    t = (rng.standard_normal((n, 3, 3)) * tri_scale).astype(np.float32)
    w = rng.uniform(-0.7, 1.7, (n, 2))
    h = (rng.uniform(0, 1, (n, 3)) ** 2 * hmax).astype(np.float32)
    flat = np.nonzero(rng.uniform(0, 1, n) < 1.0 / 7.0)[0]
    keep = rng.randint(0, 3, len(flat))                                      # how many axes keep their extent: 2, 1 or none
    order = np.argsort(rng.uniform(0, 1, (len(flat), 3)), 1)
    for k in range(3):
        h[flat, order[:, k]] = np.where(k < keep, h[flat, order[:, k]], 0.0)
    r = h.max(1)
    aim = t[:, 0] + (t[:, 1] - t[:, 0]) * w[:, :1] + (t[:, 2] - t[:, 0]) * w[:, 1:] + rng.standard_normal((n, 3)) * r[:, None] * rng.uniform(0, 1.2, (n, 1))
    away = rng.standard_normal((n, 3))
    away /= np.linalg.norm(away, axis=1, keepdims=True)
    near = rng.uniform(0, 1, n) < 0.1
    o = aim + away * np.where(near, r * rng.uniform(0, 1.5, n), dist * rng.uniform(0.3, 1.5, n))[:, None]
    d = (aim - o) * rng.uniform(0.4, 2.5, (n, 1)) + rng.standard_normal((n, 3)) * 1e-3 * dist
    max_t = np.where(rng.uniform(0, 1, n) < 0.5, RTK_INF, rng.uniform(0.2, 4.0, n)).astype(np.float32)
    min_t = np.where(rng.uniform(0, 1, n) < 0.8, 0.0, rng.uniform(-1.0, 0.15, n)).astype(np.float32)
    return make_sweeps(o, d, min_t, max_t, h), t


def times(s, t):
    return tri_boxsweep_np(prepare(s), t[:, 0], t[:, 1], t[:, 2])


def special_families(rng):
    """name -> (sweeps [n, 11], tris [n, 3, 3]) float32"""
    fam = {}
    n = 2000
    s, t = random_family(rng, n, 1.0, 3.0, 0.3)
    k = rng.uniform(-0.5, 1.5, (n, 1))
    t[:, 2] = (t[:, 0] + (t[:, 1] - t[:, 0]) * k + rng.standard_normal((n, 3)) * 10.0 ** rng.uniform(-8, -3, (n, 1))).astype(np.float32)
    fam["slivers"] = (s, t)
    s, t = random_family(rng, 600, 1.0, 3.0, 0.3)
    t[:, 1] = t[:, 0]
    fam["a=b"] = (s, t)
    s, t = random_family(rng, 3000, 1.0, 3.0, 0.3)
    t[:, 1] = t[:, 0]; t[:, 2] = t[:, 0]
    fam["a=b=c"] = (s, t)
    # triangles in an axis plane: the normal is an axis of the box and nine of the ten other axes are that axis again or zero
    s, t = random_family(rng, 1500, 1.0, 3.0, 0.3)
    i = np.arange(1500)
    t[i, 1, i % 3] = t[i, 0, i % 3]; t[i, 2, i % 3] = t[i, 0, i % 3]
    fam["in an axis plane"] = (s, t)
    # one or two direction components exactly zero: the containment branch of the slab routine, and s == 0 on edge axes
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
    s[:, 8:11] = 0.0
    s[::7, 8] = -0.0
    fam["half 0"] = (s, t)
    s, t = random_family(rng, 1000, 1.0, 0.3, 0.4)
    s[:, 7] = s[:, 6]
    fam["min_t = max_t"] = (s, t)
    # a start that already overlaps: the centre at min_t on a point of the triangle, or off it by less than the half extents
    s, t = random_family(rng, 1200, 1.0, 3.0, 0.3)
    w = rng.uniform(0, 1, (1200, 2)); w[w.sum(1) > 1] = 1 - w[w.sum(1) > 1]
    on = t[:, 0] + (t[:, 1] - t[:, 0]) * w[:, :1] + (t[:, 2] - t[:, 0]) * w[:, 1:]
    s[:, 6] = 0.0
    s[:, 0:3] = on + rng.uniform(-0.9, 0.9, (1200, 3)) * s[:, 8:11]
    s[::4, 0:3] = t[::4, 1]
    fam["a start that overlaps"] = (s, t)
    # paths parallel to an edge and to the face: s == 0, or a rounding of it, on the axes across them
    s, t = random_family(rng, 1500, 1.0, 3.0, 0.3)
    i = np.arange(1500)
    e = t[i, (i + 1) % 3] - t[i, i % 3]
    s[:, 3:6] = e * rng.uniform(-2, 2, (1500, 1))
    fam["parallel to an edge"] = (s, t)
    s, t = random_family(rng, 1500, 1.0, 3.0, 0.3)
    s[:, 3:6] = (t[:, 1] - t[:, 0]) * rng.uniform(-1, 1, (1500, 1)) + (t[:, 2] - t[:, 0]) * rng.uniform(-1, 1, (1500, 1))
    nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    s[:, 0:3] = t.mean(1) - s[:, 3:6] * 1.5 + nrm * s[:, 8:11].max(1, keepdims=True) * rng.uniform(0.0, 1.5, (1500, 1))
    fam["parallel to the face"] = (s, t)
    # max_t at the float32 neighbour below the time, at it and above it (rows 0, 1, 2 mod 3), for min_t = 0 and for min_t < 0:
    # with a negative entry time te, tx - te is larger than max_t and its rounding admits times an ulp beyond max_t
    for name, lo_t in (("max_t around the time", None), ("max_t around the time, min_t < 0", -4.0)):
        s, t = random_family(rng, 12000, 1.0, 3.0, 0.3)
        s[:, 6], s[:, 7] = (0.0 if lo_t is None else rng.uniform(lo_t, -0.5, 12000)), RTK_INF
        axis, time = times(s, t)
        s, t, time = s[axis > BS_START][:1500], t[axis > BS_START][:1500], time[axis > BS_START][:1500]
        assert len(s) == 1500
        s[0::3, 7] = np.nextafter(time[0::3], np.float32(-np.inf))
        s[1::3, 7] = time[1::3]
        s[2::3, 7] = np.nextafter(time[2::3], np.float32(np.inf))
        fam[name] = (s, t)
    # queries that are not live
    s, t = random_family(rng, 1100, 1.0, 3.0, 0.3)
    bad = np.array([np.nan, np.inf, -np.inf], np.float32)
    s[np.arange(550), np.arange(550) % 11] = bad[(np.arange(550) // 11) % 3]
    s[np.arange(550, 700), 8 + np.arange(150) % 3] = -np.abs(s[np.arange(550, 700), 8 + np.arange(150) % 3]) - np.float32(1e-30)
    s[700:850, 3:6] = 0.0
    s[700:850:2, 4] = -0.0
    s[850:1100, 7] = np.minimum(s[850:1100, 7], 10.0)
    s[850:1100, 6] = s[850:1100, 7] + 1.0
    fam["not live"] = (s, t)
    return fam


@pytest.fixture(scope="module")
def cases():
    """Every family once: name -> (sweeps, tris, (axis, t) by numpy)"""
    rng = np.random.RandomState(20250311)
    fam = {"random %g %g %g" % sc: random_family(rng, 10000, *sc) for sc in SCALES}
    fam.update(special_families(rng))
    return {name: (s, t, times(s, t)) for name, (s, t) in fam.items()}


def test_rule_header_includes_no_hip_and_says_what_it_must():
    text = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_boxsweep_rule.h")).read()
    assert [l.split()[1] for l in text.splitlines() if l.startswith("#include")] == ["<stdint.h>", '"rtk_closest_rule.h"', '"rtk_sweep_rule.h"']
    for word in ("__fmul_rn", "__fadd_rn", "__fsub_rn", "__fdiv_rn", "__fsqrt_rn", "-ffp-contract=off", "fp contract(off)", "enormal", "NaN",
                 "CLOSED", "without a margin", "NOT rtk's watertight", "entry time <= time", "FROM THE CENTRE AT te",
                 "%.2f * 2^-23" % MEASURED, "%d * 2^-23" % BOUND):
        assert word in text, word
    mk = open(os.path.join(ROOT, "rtk_amd", "csrc", "Makefile")).read()
    assert "rtk_boxsweep_rule.h" in mk and "rtk_boxsweep.hip" in mk and "-fhip-fp32-correctly-rounded-divide-sqrt" in mk
    drv = open(os.path.join(ROOT, "tests", "boxsweep_rule_driver.cpp")).read()
    assert [l.split()[1] for l in drv.splitlines() if l.startswith("#include")][0] == '"rtk_boxsweep_rule.h"' and "hip" not in drv.lower()


def test_driver_matches_numpy_bit_for_bit(driver, cases, tmp_path):
    """The query, the time, the winning axis and the normal of every family; every axis, the start overlap and "none" are met"""
    seen = np.zeros(BS_AXES, np.int64)
    for name, (s, t, (axis, time)) in cases.items():
        q = prepare(s)
        got = run_driver(driver, "q", s.view(np.uint32), tmp_path)
        same_bits(got[:, 0:3], centre_np(q, q.tmin))
        assert (got[:, 3] == q.live).all(), name
        got = run_driver(driver, "t", np.concatenate([s, t.reshape(-1, 9)], 1).view(np.uint32), tmp_path)
        assert (got[:, 4] == axis).all(), (name, np.nonzero(got[:, 4] != axis)[0][:5], got[got[:, 4] != axis][:5], axis[got[:, 4] != axis][:5])
        same_bits(got[:, 0], time)
        normal = normal_np(q, t[:, 0], t[:, 1], t[:, 2], axis)
        same_bits(got[:, 1:4], normal)
        print("%-34s %s" % (name, np.bincount(axis, minlength=BS_AXES)))
        has = axis != BS_NONE                                                # no time outside [min_t, max_t], whatever the family
        assert (s[has, 6] <= time[has]).all() and (time[has] <= s[has, 7]).all(), (name, np.nonzero(has & ~((s[:, 6] <= time) & (time <= s[:, 7])))[0][:5])
        # the normal: zeros for none and start, otherwise of unit length or zeros, against the motion, never a NaN where live
        assert not np.isnan(normal[q.live]).any(), name
        assert (normal[axis <= BS_START] == 0).all()
        length = np.linalg.norm(normal.astype(np.float64), axis=1)
        assert (((np.abs(length - 1) < 1e-6) | (length == 0))[q.live]).all(), name
        assert ((normal[q.live].astype(np.float64) * s[q.live, 3:6]).sum(1)[length[q.live] > 0] < 0).all(), name
        box = (axis >= BS_BOX_X) & (axis <= BS_BOX_Z)
        assert (np.abs(normal[box]).sum(1) == 1).all() and (normal[box] != 0).sum() == box.sum()
        if name.startswith("random"):
            seen += np.bincount(axis, minlength=BS_AXES)
            assert q.live.all() and not np.isnan(time).any(), name
            assert (length[axis > BS_START] > 0).all(), name
            assert 0.05 < has.mean() < 0.6, (name, has.mean())
    assert (seen > 0).all(), dict(zip(AXIS_NAMES, seen.tolist()))
    # what the special families are there for
    live = lambda name: prepare(cases[name][0]).live
    assert not live("not live").any() and live("half 0").all() and live("denormal direction components").all()
    f = cases["a start that overlaps"][2][0]
    assert (f == BS_START).mean() > 0.9 and (f[::4] == BS_START).all()
    s, _, (f, time) = cases["min_t = max_t"]
    assert set(np.unique(f).tolist()) == {BS_NONE, BS_START}                 # (nothing but the start can happen in an interval of one point)
    assert (time == s[:, 7]).all() and (f == BS_START).sum() > 20
    f = cases["a=b=c"][2][0]
    assert np.isin(f, [BS_NONE, BS_START, 2, 3, 4]).all() and (f >= 2).sum() > 10   # a point has no normal and no edge: the box's faces alone
    f = cases["in an axis plane"][2][0]
    assert (f != BS_NONE).sum() > 50 and (f >= BS_EDGE).sum() > 10 and (f == BS_NORMAL).sum() < 0.1 * (f != BS_NONE).sum()    # (its normal is a box axis, which comes first, but for rounding)
    f = cases["half 0"][2][0]
    assert (f == BS_NORMAL).sum() > 50 and (f == BS_NONE).sum() > 50       # (a point meets the face or nothing, but for rounding)
    for name in ("axis-aligned directions", "denormal direction components", "slivers", "a=b", "parallel to an edge", "parallel to the face"):
        f, time = cases[name][2]
        assert (f != BS_NONE).sum() > 10 and (f == BS_NONE).sum() > 10 and not np.isnan(time).any(), name
    for name in ("max_t around the time", "max_t around the time, min_t < 0"):
        s, _, (f, time) = cases[name]
        assert (f[0::3] == BS_NONE).all(), name                              # below the time: none, also where tx - te rounds up
        assert (f[1::3] != BS_NONE).sum() > 100 and (time[1::3] == s[1::3, 7]).all()    # at it: the closed interval keeps the hit (t = max_t either way)
        assert (f[2::3] != BS_NONE).sum() > 400 and (time[2::3][f[2::3] != BS_NONE] < s[2::3, 7][f[2::3] != BS_NONE]).all()
    assert (cases["max_t around the time, min_t < 0"][0][:, 6] < 0).all()
    # the order matters: a projection summed the other way round differs somewhere (so the comparison can fail)
    s, t = cases["random 1 3 0.3"][:2]
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]).astype(np.float32)
    d = s[:, 3:6]
    assert (((n[:, 2] * d[:, 2] + n[:, 1] * d[:, 1]) + n[:, 0] * d[:, 0]) != ((n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2])).any()


def test_bound_never_exceeds_the_time(driver, cases, tmp_path):
    """The triangle's own box and random enlargements of it, equal to it on some faces, for every live query: the box's entry
    time is <= the triangle's time, its exit time >= the triangle's box's, and an empty interval of the box means the triangle
    has none. None may fail."""
    rng = np.random.RandomState(7)
    total = with_time = 0
    for name, (s, t, (axis, time)) in cases.items():
        q = prepare(s)
        lo, hi = tri_box(t[:, 0], t[:, 1], t[:, 2])
        own = slab_np(q, lo, hi)
        ext = np.maximum((hi - lo).max(1, keepdims=True), np.float32(1e-45))
        for grow in (0.0, 1e-6, 1e-4, 1e-2, 0.3, 1.0, 1.0, 30.0):
            with np.errstate(all="ignore"):
                keep_lo, keep_hi = rng.uniform(0, 1, lo.shape) < 0.3, rng.uniform(0, 1, hi.shape) < 0.3      # faces that stay the triangle's
                blo = (lo - (rng.uniform(0, 1, lo.shape) * grow * ~keep_lo).astype(np.float32) * ext).astype(np.float32)
                bhi = (hi + (rng.uniform(0, 1, hi.shape) * grow * ~keep_hi).astype(np.float32) * ext).astype(np.float32)
            assert (blo <= lo).all() and (bhi >= hi).all()
            some, te, tx, face = slab_np(q, blo, bhi)
            got = run_driver(driver, "b", np.concatenate([s, blo, bhi], 1).view(np.uint32), tmp_path)
            same_bits(got[:, 0], te); same_bits(got[:, 1], tx)
            assert (got[:, 2] == face).all() and (got[:, 3] == some).all(), (name, grow)
            ok = q.live
            has = ok & (axis != BS_NONE)
            assert some[has].all(), (name, grow, int((~some[has]).sum()))                  # an empty box: no time below it
            assert (te[has] <= time[has]).all(), (name, grow, int((~(te[has] <= time[has])).sum()))
            assert (some | ~own[0])[ok].all() and (te <= own[1])[ok & own[0]].all() and (tx >= own[2])[ok & own[0]].all()
            assert not np.isnan(te[ok]).any()
            total += int(ok.sum()); with_time += int(has.sum())
    print("boxes %d, of them above a triangle with a time %d" % (total, with_time))
    assert total > 300000 and with_time >= 100000


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


def driver_times(exe, s, t, tmp_path):
    """(axis, t) of 2. for every (sweep, triangle) row BY THE HEADER, through the driver's binary mode -- and the same bits as numpy"""
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "times.bin")
    np.concatenate([s, t.reshape(-1, 9)], 1).astype(np.float32).view(np.uint32).tofile(src)
    r = subprocess.run([exe, "--binary", src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = np.fromfile(dst, np.uint32).reshape(-1, 5)
    assert len(got) == len(s)
    axis, time = got[:, 4].astype(np.int64), got[:, 0].copy().view(np.float32)
    want_axis, want_time = times(s, t)
    assert (axis == want_axis).all()
    same_bits(got[:, 0], want_time)
    return axis, time


def test_what_the_time_means_by_the_static_box_rule(driver, tmp_path):
    """Independent of swept axes: tests/box_ref.py's rule for "a box touches a triangle" (rtk_dev_triangles_in_box) on the family of
    scale 1 with half extents up to 0.3, the times taken from the header through the driver. Where the sweep has a time later
    than min_t: the box at c(t) with its half extents grown by tol touches the triangle, and the box a little earlier does not.
    tol is the position error that the accuracy statement allows, BOUND * 2^-23 of the largest coordinate magnitude involved.
    "A little earlier", where every half extent is at least tol: at c(t - delta) with delta = 2 * tol / |D|, the half extents
    shrunk by tol. In exact arithmetic that is a time before the contact even where t is late by tol / |D|, so the true boxes
    are apart there, the shrunk ones by tol and more -- a thousand times the rounding of the static rule.
    Where a half extent is below tol (flat boxes, needles, points: they cannot be shrunk): the box as it is, at c(t - delta) with
    delta = (tol + g / cos) / |D|, g = 64 * 2^-23 of the largest coordinate magnitude and cos the cosine between the motion and
    the axis that gives the time in float64. Before the contact the gap along that unit axis grows by |D| * cos per unit of time,
    so the true box is apart from the triangle by g and more there, sixty-four ulps of the largest coordinate, where the static
    rule's own rounding is a few. (Cases that have no time from an axis in float64 are left out of this half: they are the ones
    test_accuracy_against_float64 counts as disagreeing.)"""
    rng = np.random.RandomState(31)
    s, t = random_family(rng, 100000, 1.0, 3.0, 0.3)
    axis, time = driver_times(driver, s, t, tmp_path)
    q = prepare(s, np.float64)
    use = (axis > BS_START) & (time > s[:, 6])
    assert use.sum() > 15000
    s, t, time, q = s[use], t[use].astype(np.float64), time[use].astype(np.float64), q.at(use)
    c = centre_np(q, time)
    mag = np.maximum(np.maximum(np.abs(q.O).max(1), np.abs(t).reshape(-1, 9).max(1)), (np.abs(c) + q.H).max(1))
    tol = BOUND * 2.0 ** -23 * mag
    dlen = np.sqrt((q.D * q.D).sum(1))
    F = np.float32
    grown = (q.H + tol[:, None]).astype(F)
    at = candidate_np(t[:, 0], t[:, 1], t[:, 2], c.astype(F) - grown, c.astype(F) + grown)
    assert at.all(), (int((~at).sum()), np.nonzero(~at)[0][:5])
    # before the time: boxes that can be shrunk
    thick = (q.H >= tol[:, None]).all(1)
    before = centre_np(q, time - 2.0 * tol / dlen)
    shrunk = np.maximum(q.H - tol[:, None], 0.0).astype(F)
    touches = candidate_np(t[:, 0], t[:, 1], t[:, 2], before.astype(F) - shrunk, before.astype(F) + shrunk)
    assert thick.sum() > 10000 and not touches[thick].any(), (int(touches[thick].sum()), np.nonzero(touches & thick)[0][:5])
    # ... and those that cannot: flat boxes, needles, points, as they are
    axis64 = tri_boxsweep_np(q, t[:, 0], t[:, 1], t[:, 2], np.float64)[0]
    normal = normal_np(q, t[:, 0], t[:, 1], t[:, 2], axis64, np.float64)
    cos = np.abs((normal * q.D).sum(1)) / dlen
    thin = ~thick & (axis64 > BS_START) & (cos > 0)
    with np.errstate(divide="ignore"):
        delta = (tol + 64.0 * 2.0 ** -23 * mag / cos) / dlen
    before = centre_np(q, time - np.where(thin, delta, 0.0))
    half = q.H.astype(F)
    touches = candidate_np(t[:, 0], t[:, 1], t[:, 2], before.astype(F) - half, before.astype(F) + half)
    flat = thin & (q.H == 0).any(1)
    print("times %d; before the time: %d boxes shrunk, %d as they are (%d of them flat on an axis), %d left out" % (
        len(s), int(thick.sum()), int(thin.sum()), int(flat.sum()), int((~thick & ~thin).sum())))
    assert thin.sum() > 2500 and flat.sum() > 1500 and (~thick & ~thin).sum() < 20
    assert not touches[thin].any(), (int(touches[thin].sum()), np.nonzero(touches & thin)[0][:5])


def _hit64(s, t, dh=0.0, dt=0.0, do=None):
    """float64, with the half extents grown by dh, the interval widened by dt at both ends (negative: shrunk) and the origin
    moved by do: is there a time?"""
    q = prepare(s, np.float64)
    q.H = np.maximum(q.H + np.asarray(dh)[..., None], 0.0)
    q.tmin, q.tmax = q.tmin - dt, q.tmax + dt
    if do is not None:
        q.O = q.O + do
    return tri_boxsweep_np(q, t[:, 0], t[:, 1], t[:, 2], np.float64)[0] != BS_NONE


def test_accuracy_against_float64(driver, tmp_path):
    """|t - t64| * |D| <= BOUND * 2^-23 * the largest coordinate magnitude involved (origin, triangle, the box's faces at the
    contact), on EVERY case that has a time in float32 and in float64 -- starts that overlap, slivers and grazing contacts
    included --, 600 000 cases at each of the five scales, the float32 side of every one computed BY THE HEADER through the
    driver (and the same bits as the numpy reference); at least 5 % of every family have one (the float64 rule alone gives
    9.8 % to 39 %: a smaller share would mean that the float rule loses hits).
    The header's statement: MEASURED = 1730.41, reached by a grazing contact (the motion 0.01 degrees off the triangle's plane: the
    time's condition number is 5000, and the error times the cosine stays below 7); the asserted bound is that times 2.5,
    rounded up: BOUND = 4327. Without grazing contacts (cosine below 0.05) and starts that overlap, as the sphere sweep's
    statement is measured: MEASURED_STEEP = 31.96, asserted at 2.5 times it, 80.
    Measured: hit / none differs on 419 of the 3 million cases, none of them clear.
    A case on which float32 and float64 disagree about hit or none is counted apart. Such a case is CLEAR if the float64 answer
    stays the same when all half extents and both ends of the interval (in the path's units) move by d either way and when the
    origin moves by d along each axis either way, with d = BOUND * 2^-23 of the largest coordinate magnitude: the position
    error that the assertion above allows the float32 evaluation. Then no comparison of the float64 evaluation is within that
    rounding of its threshold. No clear case may disagree."""
    rng = np.random.RandomState(99)
    worst, steep_worst, steep_pairs, evaluated, pairs, disagree, disagree_clear = 0.0, 0.0, 0, 0, 0, 0, 0
    for sc in SCALES:
        fam_pairs = fam_n = 0
        fam_worst = 0.0
        for _ in range(3):
            s, t = random_family(rng, 200000, *sc)
            f32, t32 = driver_times(driver, s, t, tmp_path)                  # the header's bits, not the reference's
            q = prepare(s, np.float64)
            T = t.astype(np.float64)
            f64, t64 = tri_boxsweep_np(q, T[:, 0], T[:, 1], T[:, 2], np.float64)
            c = centre_np(q, t64)
            mag = np.maximum(np.maximum(np.abs(q.O).max(1), np.abs(T).reshape(-1, 9).max(1)), np.where(f64 != BS_NONE, (np.abs(c) + q.H).max(1), 0))
            dlen = np.sqrt((q.D * q.D).sum(1))
            evaluated += len(s); fam_n += len(s)
            dis = np.nonzero((f32 != BS_NONE) != (f64 != BS_NONE))[0]
            if len(dis):
                d = mag[dis] * BOUND * 2.0 ** -23
                base = f64[dis] != BS_NONE
                moves = [dict(dh=-d, dt=-d / dlen[dis]), dict(dh=d, dt=d / dlen[dis])]
                moves += [dict(do=np.eye(3)[k] * d[:, None] * sign) for k in range(3) for sign in (-1.0, 1.0)]
                clear = np.all([_hit64(s[dis], T[dis], **m) == base for m in moves], 0)
                disagree += len(dis); disagree_clear += int(clear.sum())
            both = (f32 != BS_NONE) & (f64 != BS_NONE)
            err = np.abs(t32.astype(np.float64) - t64) * dlen / mag
            pairs += int(both.sum()); fam_pairs += int(both.sum())
            fam_worst = max(fam_worst, err[both].max())
            normal = normal_np(q, T[:, 0], T[:, 1], T[:, 2], f64, np.float64)
            steep = both & (f32 > BS_START) & (f64 > BS_START) & (np.abs((normal * q.D).sum(1)) >= 0.05 * dlen)
            steep_pairs += int(steep.sum())
            steep_worst = max(steep_worst, err[steep].max())
        print("scales %s: %d of %d have a time in both (%.1f %%), worst error %.2f * 2^-23 of the largest coordinate"
              % (sc, fam_pairs, fam_n, 100.0 * fam_pairs / fam_n, fam_worst * 2.0 ** 23))
        assert fam_n >= 600000 and fam_pairs >= 0.05 * fam_n, sc
        worst = max(worst, fam_worst)
    print("worst %.2f * 2^-23 over %d cases of %d; hit / none differs on %d cases, %d of them clear"
          % (worst * 2.0 ** 23, pairs, evaluated, disagree, disagree_clear))
    print("without grazing contacts and starts that overlap: worst %.2f * 2^-23 over %d cases" % (steep_worst * 2.0 ** 23, steep_pairs))
    assert disagree_clear == 0
    assert worst <= BOUND * 2.0 ** -23
    assert steep_pairs > 400000 and steep_worst <= BOUND_STEEP * 2.0 ** -23


def test_header_symbols_sizes_and_argtypes(api):
    from rtk_amd import types
    text = open(os.path.join(ROOT, "include", "rtk_amd.h")).read()
    for word in ("typedef struct rtk_box_sweep { float origin[3], direction[3], min_t, max_t, half[3]; } rtk_box_sweep;",
                 "int rtk_dev_sweep_boxes(const rtk_dev_scene *ds, const rtk_box_sweep *d_sweeps, size_t num_sweeps, const rtk_ray_list *list,",
                 "int rtk_dev_sweep_boxes_any(", "int rtk_dev_sweep_boxes_counted(", "uint32_t rtk_amd_boxsweep_stack_entries(void);",
                 "LOWEST PRIMITIVE ID AMONG EQUAL TIMES", "NOT rtk's watertight ray test", "CLOSED interval", "d_after is refused", "Box sweeps", "NOT NECESSARILY A POINT OF CONTACT",
                 "float *d_centres /* may be NULL */, float *d_normals /* may be NULL */", "never a NaN"):
        assert word in text, word
    assert text.index("---- Sphere sweeps") < text.index("---- Box sweeps") < text.index("---- Every hit along a ray")
    check = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_layout_check.h")).read()
    assert "sizeof(rtk_box_sweep) == 44" in check
    assert types.BOX_SWEEP_DTYPE.itemsize == 44 and types.BOX_SWEEP_DTYPE.names == ("origin", "direction", "min_t", "max_t", "half")
    assert types.BOX_SWEEP_DTYPE.fields["min_t"][1] == 24 and types.BOX_SWEEP_DTYPE.fields["half"][1] == 32 and types.BOX_SWEEP_DTYPE.fields["half"][0].shape == (3,)
    L = api.lib()
    for name in ("rtk_dev_sweep_boxes", "rtk_dev_sweep_boxes_any", "rtk_dev_sweep_boxes_counted", "rtk_amd_boxsweep_stack_entries"):
        assert name in api.RTK_AMD_H_SYMBOLS and hasattr(L, name), name
    assert L.rtk_dev_sweep_boxes.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(api.RayList), C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.POINTER(api.DevFilter), C.c_void_p]
    assert L.rtk_dev_sweep_boxes_any.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(api.RayList), C.c_void_p, C.POINTER(api.DevFilter), C.c_void_p]
    assert L.rtk_dev_sweep_boxes_counted.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(api.DevFilter),
                                                        C.POINTER(api.TraceCounters)]
    assert L.rtk_dev_sweep_boxes.restype == C.c_int and L.rtk_dev_sweep_boxes_any.restype == C.c_int and L.rtk_dev_sweep_boxes_counted.restype == C.c_int
    assert L.rtk_amd_boxsweep_stack_entries.restype == C.c_uint32 and 1 <= L.rtk_amd_boxsweep_stack_entries() <= 64
    for name in ("sweep_boxes", "sweep_boxes_device", "sweep_boxes_any_device", "sweep_boxes_counted", "box_path_blocked"):
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
    # the closest form: (ds, sweeps, n, list, records, centres, normals, filter, stream)
    for args in [(None, dummy, 4, None, dummy, None, None, None, None), (dummy, None, 4, None, dummy, None, None, None, None),
                 (dummy, dummy, 4, None, None, dummy, dummy, None, None), (dummy, dummy, 1 << 32, None, dummy, None, None, None, None),
                 (dummy, dummy, 1 << 32, C.byref(ray_list()), dummy, None, None, None, None)] \
            + [(dummy, dummy, 4, l, dummy, None, None, None, None) for l in bad_lists] \
            + [(dummy, dummy, 4, None, dummy, None, None, f, None) for f in bad_filters]:
        assert L.rtk_dev_sweep_boxes(*args) == ERR_BAD_ARG, args
        assert "rtk_dev_sweep_boxes:" in api.last_error()
    assert "d_after" in api.last_error() or "mesh mask" in api.last_error()
    assert L.rtk_dev_sweep_boxes(dummy, dummy, 4, None, dummy, None, None, bad_filters[1], None) == ERR_BAD_ARG and "d_after" in api.last_error()
    # the any-hit form: (ds, sweeps, n, list, blocked, filter, stream)
    for args in [(None, dummy, 4, None, dummy, None, None), (dummy, None, 4, None, dummy, None, None), (dummy, dummy, 4, None, None, None, None),
                 (dummy, dummy, 1 << 32, None, dummy, None, None)] + [(dummy, dummy, 4, l, dummy, None, None) for l in bad_lists] \
            + [(dummy, dummy, 4, None, dummy, f, None) for f in bad_filters]:
        assert L.rtk_dev_sweep_boxes_any(*args) == ERR_BAD_ARG, args
        assert "rtk_dev_sweep_boxes_any:" in api.last_error()
    # the counting form: (ds, sweeps, n, records, centres, normals, filter, counters)
    ctr = api.TraceCounters()
    for args in [(dummy, dummy, 4, dummy, None, None, None, None), (None, dummy, 4, dummy, None, None, None, C.byref(ctr)),
                 (dummy, None, 4, dummy, None, None, None, C.byref(ctr)), (dummy, dummy, 4, None, None, None, None, C.byref(ctr)),
                 (dummy, dummy, 1 << 32, dummy, None, None, None, C.byref(ctr)), (dummy, dummy, 4, dummy, None, None, bad_filters[1], C.byref(ctr))]:
        assert L.rtk_dev_sweep_boxes_counted(*args) == ERR_BAD_ARG, args
        assert "rtk_dev_sweep_boxes_counted" in api.last_error()
    ctr.rays = 5
    assert L.rtk_dev_sweep_boxes_counted(dummy, None, 0, None, None, None, None, C.byref(ctr)) == 0 and ctr.rays == 0
    # no queries: nothing to do, nothing launched
    assert L.rtk_dev_sweep_boxes(dummy, None, 0, None, None, None, None, None, None) == 0
    assert L.rtk_dev_sweep_boxes(dummy, dummy, 0, C.byref(ray_list()), dummy, dummy, dummy, C.byref(dev_filter()), None) == 0
    assert L.rtk_dev_sweep_boxes_any(dummy, None, 0, None, None, None, None) == 0
