"""Oriented box sweeps without a GPU: the rule of rtk_amd/csrc/rtk_obbsweep_rule.h, run by tests/obbsweep_rule_driver.cpp under the
address and undefined-behaviour sanitizers, against numpy float32 arithmetic in the stated order (tests/obbsweep_ref.py), bit for
bit; the entry time of a box against the time of every triangle inside it; what the time means, by the static box rule of
tests/box_ref.py in the box's frame; the accuracy statement against float64; the axis-aligned rule on signed-permutation axes;
and the parts of the interface that need no device -- header text, symbols, struct sizes, argtypes, the refusals decided before
any HIP call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import boxsweep_ref
from tests.box_ref import candidate_np
from tests.closest_ref import tri_box
from tests.obbsweep_ref import (AXIS_NAMES, ORTHO_TOL, OS_CODES, OS_EDGE, OS_NONE, OS_NORMAL, OS_START, OS_U0, OS_U2, OS_UNNAMED, centre_np, normal_np,
                                obb_slab_np, prepare, tri_obbsweep_np)
from tests.test_boxsweep_cpu import BOUND as BOX_BOUND
from tests.test_boxsweep_cpu import random_family as box_family
from tests.test_sweep_cpu import SCALES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_BAD_ARG = -2
RTK_INF = np.float32(3.402823e+38)
# |t - t64| * |D| in units of 2^-23 of the largest coordinate magnitude involved: what test_accuracy_against_float64 measured, and
# 2.5 times it, rounded up: the factor of the closest-point, closest-triangle and the other sweeps' statements
MEASURED = 726.86
BOUND = 1818.0
# the same without grazing contacts (cosine between the motion and the contact normal below 0.05) and starts that overlap
MEASURED_STEEP = 41.09
BOUND_STEEP = 103.0


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """The driver built against the rule headers alone (no HIP include path, -Wall -Werror, no FMA contraction as in the library)
    with both sanitizers. -O2 and -mfma: a compiler that were allowed to contract would do it here."""
    exe = str(tmp_path_factory.mktemp("obbsweep_rule") / "obbsweep_rule_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-mfma", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "rtk_amd", "csrc"), os.path.join(ROOT, "tests", "obbsweep_rule_driver.cpp"), "-o", exe])
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
    hexes = {"q": 9, "b": 2, "t": 4}[kind]
    return np.array([[int(w, 16) if k < hexes else int(w) for k, w in enumerate(line.split())] for line in lines[:len(words)]], np.int64)


def same_bits(got, want):
    """Bit for bit, except where the expected value is NaN: there only "it is NaN" is promised."""
    got = np.ascontiguousarray(got, np.uint32)
    want = np.ascontiguousarray(want, np.float32)
    nan = np.isnan(want)
    assert (np.isnan(got.view(np.float32)) == nan).all()
    bad = (got != want.view(np.uint32)) & ~nan
    assert not bad.any(), (np.argwhere(bad)[:5], got[bad][:5], want.view(np.uint32)[bad][:5])


def quat_rows(q):
    """unit quaternions (x, y, z, w) [n, 4] -> [n, 3, 3] float64 whose ROWS are the images of the unit vectors: the box's axes"""
    q = np.asarray(q, np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    x, y, z, w = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                  2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)
    return R.transpose(0, 2, 1)


def with_axes(box_sweeps, axes):
    """float32 [n, 11] box sweeps and axes [n, 3, 3] -> float32 [n, 20]"""
    return np.concatenate([np.asarray(box_sweeps, np.float32), np.asarray(axes, np.float64).reshape(-1, 9).astype(np.float32)], 1)


def signed_permutations(rng, n):
    """[n, 3, 3] signed permutation matrices (identity among them: every fifth), and the permutation perm [n, 3] with row j = +-unit(perm[j])"""
    perm = np.argsort(rng.uniform(0, 1, (n, 3)), 1)
    sign = rng.choice([-1.0, 1.0], (n, 3))
    perm[::5] = np.arange(3)
    sign[::5] = 1.0
    U = np.zeros((n, 3, 3))
    for j in range(3):
        U[np.arange(n), j, perm[:, j]] = sign[:, j]
    return U, perm


def random_family(rng, n, tri_scale, dist, hmax):
    """tests/test_boxsweep_cpu.py's family (triangles of the given size, paths from `dist` away towards them, half extents up to
    hmax, a seventh of the boxes flat on one, two or three axes, a tenth of the starts within reach) with a rotation per query
    from a random unit quaternion, made in float64 and rounded once to float32"""
    s, t = box_family(rng, n, tri_scale, dist, hmax)
    return with_axes(s, quat_rows(rng.standard_normal((n, 4)))), t


def times(s, t):
    return tri_obbsweep_np(prepare(s), t[:, 0], t[:, 1], t[:, 2])


def special_families(rng):
    """name -> (sweeps [n, 20], tris [n, 3, 3]) float32"""
    fam = {}
    s, t = random_family(rng, 3000, 1.0, 3.0, 0.3)
    s[:, 11:20] = signed_permutations(rng, 3000)[0].reshape(-1, 9)
    s[::7, 11:20] = -np.abs(s[::7, 11:20])                                   # (-0 among the zeros, -1 on the diagonal or off it)
    fam["identity and signed permutations"] = (s, t)
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
    # triangles in a face plane of the box: spanned by two of its axes, so that the normal is the third axis again (up to rounding)
    s, t = random_family(rng, 1500, 1.0, 3.0, 0.3)
    i = np.arange(1500)
    U = s[:, 11:20].reshape(-1, 3, 3).astype(np.float64)
    e1, e2 = U[i, (i + 1) % 3], U[i, (i + 2) % 3]
    base = t[:, 0].astype(np.float64)
    c1, c2 = rng.standard_normal((2, 1500, 2, 1))
    t[:, 1] = base + e1 * c1[:, 0] + e2 * c1[:, 1]
    t[:, 2] = base + e1 * c2[:, 0] + e2 * c2[:, 1]
    fam["in a face plane of the box"] = (s, t)
    # the motion along one or two of the box's own axes: D' has zeros or roundings of them, the s == 0 branch of the box axes
    s, t = random_family(rng, 1500, 1.0, 3.0, 0.5)
    U = s[:, 11:20].reshape(-1, 3, 3).astype(np.float64)
    dlen = np.linalg.norm(s[:, 3:6], axis=1, keepdims=True)
    s[:, 3:6] = U[i, i % 3] * dlen * rng.choice([-1.0, 1.0], (1500, 1))
    s[::2, 3:6] += (U[i, (i + 1) % 3] * dlen * rng.uniform(-1, 1, (1500, 1)))[::2]
    s[::3, 11:20] = signed_permutations(rng, 500)[0].reshape(-1, 9)           # ... exactly zero with exact axes
    fam["along the box's axes"] = (s, t)
    s, t = random_family(rng, 1500, 1.0, 3.0, 0.5)
    zero = np.arange(1500) % 3
    s[np.arange(1500), 3 + zero] = 0.0
    s[np.arange(1500)[::2], 3 + (zero[::2] + 1) % 3] = 0.0
    s[::5, 3 + zero[::5]] = -0.0
    fam["axis-aligned directions"] = (s, t)
    s, t = random_family(rng, 1500, 1.0, 3.0, 0.5)
    s[np.arange(1500), 3 + np.arange(1500) % 3] = (rng.choice([-1.0, 1.0], 1500) * 10.0 ** rng.uniform(-45, -38, 1500)).astype(np.float32)
    s[1000:, 3:6] = (rng.choice([-1.0, 1.0], (500, 3)) * 10.0 ** rng.uniform(-45, -38, (500, 3))).astype(np.float32)      # all of D denormal: D' may vanish
    s[1000:, 0:3] = t[1000:].mean(1) + rng.uniform(-0.5, 0.5, (500, 3))
    s[1000:, 6] = np.where(rng.uniform(0, 1, 500) < 0.5, 0.0, -1e37)
    fam["denormal direction components"] = (s, t)
    s, t = random_family(rng, 2100, 1.0, 3.0, 0.3)
    s[:700, 8:11] = 0.0
    s[:700:7, 8] = -0.0
    k = np.arange(700)
    s[700 + k, 8 + k % 3] = 0.0                                             # flat on one axis
    s[1400 + k, 8 + k % 3] = 0.0; s[1400 + k, 8 + (k + 1) % 3] = 0.0          # a segment
    fam["half 0"] = (s, t)
    s, t = random_family(rng, 1000, 1.0, 0.3, 0.4)
    s[:, 7] = s[:, 6]
    fam["min_t = max_t"] = (s, t)
    # a start that already overlaps: the centre at min_t on a point of the triangle, or off it by less than the half extents along the box's axes
    s, t = random_family(rng, 1200, 1.0, 3.0, 0.3)
    w = rng.uniform(0, 1, (1200, 2)); w[w.sum(1) > 1] = 1 - w[w.sum(1) > 1]
    on = t[:, 0] + (t[:, 1] - t[:, 0]) * w[:, :1] + (t[:, 2] - t[:, 0]) * w[:, 1:]
    U = s[:, 11:20].reshape(-1, 3, 3).astype(np.float64)
    s[:, 6] = 0.0
    s[:, 0:3] = on + np.einsum("nj,njk->nk", rng.uniform(-0.9, 0.9, (1200, 3)) * s[:, 8:11], U)
    s[::4, 0:3] = t[::4, 1]
    fam["a start that overlaps"] = (s, t)
    s, t = random_family(rng, 1500, 1.0, 3.0, 0.3)
    i = np.arange(1500)
    e = t[i, (i + 1) % 3] - t[i, i % 3]
    s[:, 3:6] = e * rng.uniform(-2, 2, (1500, 1))
    fam["parallel to an edge"] = (s, t)
    # max_t at the float32 neighbour below the time, at it and above it (rows 0, 1, 2 mod 3), for min_t = 0 and for min_t < 0:
    # with a negative entry time te, tx - te is larger than max_t and its rounding admits times an ulp beyond max_t
    for name, lo_t in (("max_t around the time", None), ("max_t around the time, min_t < 0", -4.0)):
        s, t = random_family(rng, 12000, 1.0, 3.0, 0.3)
        s[:, 6], s[:, 7] = (0.0 if lo_t is None else rng.uniform(lo_t, -0.5, 12000)), RTK_INF
        axis, time = times(s, t)
        s, t, time = s[axis > OS_START][:1500], t[axis > OS_START][:1500], time[axis > OS_START][:1500]
        assert len(s) == 1500
        s[0::3, 7] = np.nextafter(time[0::3], np.float32(-np.inf))
        s[1::3, 7] = time[1::3]
        s[2::3, 7] = np.nextafter(time[2::3], np.float32(np.inf))
        fam[name] = (s, t)
    # queries that are not live: rows 0 .. 1199 a NaN or an infinity in every field, then negative half extents, a zero
    # direction, min_t > max_t, and from 1700 on axes that fail the gate
    s, t = random_family(rng, 2300, 1.0, 3.0, 0.3)
    bad = np.array([np.nan, np.inf, -np.inf], np.float32)
    s[np.arange(1200), np.arange(1200) % 20] = bad[(np.arange(1200) // 20) % 3]
    s[np.arange(1200, 1350), 8 + np.arange(150) % 3] = -np.abs(s[np.arange(1200, 1350), 8 + np.arange(150) % 3]) - np.float32(1e-30)
    s[1350:1500, 3:6] = 0.0
    s[1350:1500:2, 4] = -0.0
    s[1500:1700, 7] = np.minimum(s[1500:1700, 7], 10.0)
    s[1500:1700, 6] = s[1500:1700, 7] + 1.0
    U = s[1700:, 11:20].reshape(-1, 3, 3).astype(np.float64)
    k = np.arange(600)
    kind = k % 6
    U[kind == 0, k[kind == 0] % 3] *= 2.0                                    # scaled
    U[kind == 1, k[kind == 1] % 3] = 0.0                                     # a zero axis
    U[kind == 2, 1] = U[kind == 2, 0]                                        # the same axis twice
    U[kind == 3, 2] += 0.1 * U[kind == 3, 0]                                 # sheared
    U[kind == 4] = rng.standard_normal(((kind == 4).sum(), 3, 3))            # garbage
    U[kind == 5] *= 1e20                                                     # dots that overflow
    s[1700:, 11:20] = U.reshape(-1, 9)
    fam["not live"] = (s, t)
    # axes around the gate: a row's length, or the dot of a pair, a little inside and a little outside 2^-10 (rows 0, 1 mod 2)
    s, t = random_family(rng, 1200, 1.0, 3.0, 0.3)
    U = s[:, 11:20].reshape(-1, 3, 3).astype(np.float64)
    k = np.arange(1200)
    off = np.where(k % 2 == 0, 0.98, 1.02) * ORTHO_TOL * np.where((k // 2) % 2 == 0, 1.0, -1.0)
    longer = (k // 4) % 2 == 0
    U[k[longer], (k[longer] // 8) % 3] *= np.sqrt(1.0 + off[longer])[:, None]
    j = (k // 8) % 3
    U[k[~longer], j[~longer]] += U[k[~longer], (j[~longer] + 1) % 3] * off[~longer, None]
    s[:, 11:20] = U.reshape(-1, 9)
    fam["around the gate"] = (s, t)
    return fam


@pytest.fixture(scope="module")
def cases():
    """Every family once: name -> (sweeps, tris, (axis, t) by numpy)"""
    rng = np.random.RandomState(20250611)
    fam = {"random %g %g %g" % sc: random_family(rng, 10000, *sc) for sc in SCALES}
    fam.update(special_families(rng))
    return {name: (s, t, times(s, t)) for name, (s, t) in fam.items()}


def test_rule_header_includes_no_hip_and_says_what_it_must():
    text = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_obbsweep_rule.h")).read()
    assert [l.split()[1] for l in text.splitlines() if l.startswith("#include")] == ["<stdint.h>", '"rtk_closest_rule.h"', '"rtk_sweep_rule.h"',
                                                                                       '"rtk_boxsweep_rule.h"']
    for word in ("__fmul_rn", "__fadd_rn", "__fsub_rn", "__fdiv_rn", "__fsqrt_rn", "-ffp-contract=off", "fp contract(off)", "enormal", "NaN",
                 "CLOSED", "without a margin", "NOT rtk's watertight", "entry time <= time", "FROM THE CENTRE AT te", "RTK_OBB_ORTHO_TOL = 2^-10",
                 "UP TO ROUNDING, NOT bit for bit", "THE QUERY", "THE BOUND", "THE BOX AND ONE TRIANGLE", "THE NORMAL", "BETTER THAN and SKIP", "ACCURACY",
                 "%.2f * 2^-23" % MEASURED, "%d * 2^-23" % BOUND, "%.2f * 2^-23" % MEASURED_STEEP, "%d * 2^-23" % BOUND_STEEP):
        assert word in text, word
    assert BOUND == np.ceil(2.5 * MEASURED) and BOUND_STEEP == np.ceil(2.5 * MEASURED_STEEP)
    mk = open(os.path.join(ROOT, "rtk_amd", "csrc", "Makefile")).read()
    assert "rtk_obbsweep_rule.h" in mk and "rtk_obbsweep.hip" in mk and "-fhip-fp32-correctly-rounded-divide-sqrt" in mk
    drv = open(os.path.join(ROOT, "tests", "obbsweep_rule_driver.cpp")).read()
    assert [l.split()[1] for l in drv.splitlines() if l.startswith("#include")][0] == '"rtk_obbsweep_rule.h"' and "hip" not in drv.lower()
    # the axis-aligned rule is used as it stands
    assert "rtk_boxsweep_slab(Q.S" in text and "rtk_boxsweep_axis(" in text and "rtk_boxsweep_edge(Q.F" in text


def test_driver_matches_numpy_bit_for_bit(driver, cases, tmp_path):
    """The query (liveness, D', g), the time, the winning axis and the normal of every family; every axis, the start overlap and
    "none" are met"""
    seen = np.zeros(OS_CODES, np.int64)
    for name, (s, t, (axis, time)) in cases.items():
        q = prepare(s)
        got = run_driver(driver, "q", s.view(np.uint32), tmp_path)
        same_bits(got[:, 0:3], centre_np(q, q.tmin))
        same_bits(got[:, 3:6], q.Dp)
        same_bits(got[:, 6:9], q.H)
        assert (got[:, 9] == q.live).all(), (name, np.nonzero(got[:, 9] != q.live)[0][:5])
        got = run_driver(driver, "t", np.concatenate([s, t.reshape(-1, 9)], 1).view(np.uint32), tmp_path)
        assert (got[:, 4] == axis).all(), (name, np.nonzero(got[:, 4] != axis)[0][:5], got[got[:, 4] != axis][:5], axis[got[:, 4] != axis][:5])
        same_bits(got[:, 0], time)
        normal = normal_np(q, t[:, 0], t[:, 1], t[:, 2], axis)
        same_bits(got[:, 1:4], normal)
        print("%-34s %s" % (name, np.bincount(axis, minlength=OS_CODES)))
        has = (axis != OS_NONE) & q.live                                     # no time outside [min_t, max_t], whatever the family
        assert (s[has, 6] <= time[has]).all() and (time[has] <= s[has, 7]).all(), (name, np.nonzero(has & ~((s[:, 6] <= time) & (time <= s[:, 7])))[0][:5])
        assert (time[axis == OS_START] == s[axis == OS_START, 6]).all()
        # the normal: zeros for none and start, otherwise of unit length or zeros, against the motion, never a NaN where live
        assert not np.isnan(normal[q.live]).any(), name
        assert (normal[(axis <= OS_START) | (axis == OS_UNNAMED)] == 0).all()
        length = np.linalg.norm(normal.astype(np.float64), axis=1)
        assert (((np.abs(length - 1) < 1e-6) | (length == 0))[q.live]).all(), name
        assert ((normal[q.live].astype(np.float64) * s[q.live, 3:6]).sum(1)[length[q.live] > 0] < 1e-6 * np.linalg.norm(s[q.live, 3:6], axis=1)[length[q.live] > 0]).all(), name
        box = (axis >= OS_U0) & (axis <= OS_U2) & q.live
        u = s[:, 11:20].reshape(-1, 3, 3)[np.arange(len(s)), np.clip(axis - OS_U0, 0, 2)]
        assert (np.abs(np.abs((normal[box].astype(np.float64) * u[box]).sum(1)) - 1) < 2e-3).all(), name     # (a box axis: the row itself, to the gate's tolerance)
        if name.startswith("random"):
            seen += np.bincount(axis, minlength=OS_CODES)
            assert q.live.all() and not np.isnan(time).any(), name
            assert (length[axis > OS_START] > 0).all(), name
            assert 0.05 < has.mean() < 0.6, (name, has.mean())
            assert ((normal.astype(np.float64) * s[:, 3:6]).sum(1)[length > 0] < 0).all(), name
    assert (seen[:OS_UNNAMED] > 0).all(), dict(zip(AXIS_NAMES, seen.tolist()))
    # what the special families are there for
    live = lambda name: prepare(cases[name][0]).live
    assert not live("not live").any() and live("half 0").all() and live("identity and signed permutations").all()
    assert live("denormal direction components").all()
    f = cases["denormal direction components"][2][0]
    print("denormal directions: %d unnamed" % (f == OS_UNNAMED).sum())
    g = live("around the gate")
    assert g[0::2].all() and not g[1::2].any()                               # 2 % inside the gate, 2 % outside
    f = cases["a start that overlaps"][2][0]
    assert (f == OS_START).mean() > 0.9 and (f[::4] == OS_START).all()
    s, _, (f, time) = cases["min_t = max_t"]
    assert set(np.unique(f).tolist()) == {OS_NONE, OS_START}                 # (nothing but the start can happen in an interval of one point)
    assert (time == s[:, 7]).all() and (f == OS_START).sum() > 20
    f = cases["a=b=c"][2][0]
    assert np.isin(f, [OS_NONE, OS_START, 2, 3, 4]).all() and (f >= 2).sum() > 10   # a point has no normal and no edge: the box's faces alone
    f = cases["in a face plane of the box"][2][0]
    assert (f != OS_NONE).sum() > 50 and (f >= OS_EDGE).sum() > 10
    s, _, (f, _) = cases["half 0"]
    assert (f[:700] == OS_NORMAL).sum() > 30 and (f == OS_NONE).sum() > 50 and (f[700:] > OS_NORMAL).sum() > 20
    f = cases["identity and signed permutations"][2][0]
    assert (np.bincount(f, minlength=OS_CODES)[OS_START:OS_UNNAMED] > 0).all()
    for name in ("axis-aligned directions", "denormal direction components", "slivers", "a=b", "parallel to an edge", "along the box's axes"):
        f, time = cases[name][2]
        assert (f != OS_NONE).sum() > 10 and (f == OS_NONE).sum() > 10 and not np.isnan(time).any(), name
    for name in ("max_t around the time", "max_t around the time, min_t < 0"):
        s, _, (f, time) = cases[name]
        assert (f[0::3] == OS_NONE).all(), name                              # below the time: none, also where tx - te rounds up
        assert (f[1::3] != OS_NONE).sum() > 100 and (time[1::3] == s[1::3, 7]).all()    # at it: the closed interval keeps the hit (t = max_t either way)
        assert (f[2::3] != OS_NONE).sum() > 400 and (time[2::3][f[2::3] != OS_NONE] < s[2::3, 7][f[2::3] != OS_NONE]).all()
    s, t, _ = cases["max_t around the time, min_t < 0"]
    assert (s[:, 6] < 0).all()
    q = prepare(s)
    te = obb_slab_np(q, *tri_box(t[:, 0], t[:, 1], t[:, 2]))[1]
    assert (te < 0).sum() > 100                                              # negative entry times


def test_bound_never_exceeds_the_time(driver, cases, tmp_path):
    """The triangle's own box and random enlargements of it, equal to it on some faces, for every live query: the box's entry
    time is <= the triangle's time, its exit time >= the triangle's box's, and an empty interval of the box means the triangle
    has none. None may fail."""
    rng = np.random.RandomState(7)
    total = with_time = 0
    for name, (s, t, (axis, time)) in cases.items():
        q = prepare(s)
        lo, hi = tri_box(t[:, 0], t[:, 1], t[:, 2])
        own = obb_slab_np(q, lo, hi)
        ext = np.maximum((hi - lo).max(1, keepdims=True), np.float32(1e-45))
        for grow in (0.0, 1e-6, 1e-4, 1e-2, 0.3, 1.0, 1.0, 30.0, 1e6):
            with np.errstate(all="ignore"):
                keep_lo, keep_hi = rng.uniform(0, 1, lo.shape) < 0.3, rng.uniform(0, 1, hi.shape) < 0.3      # faces that stay the triangle's
                blo = (lo - (rng.uniform(0, 1, lo.shape) * grow * ~keep_lo).astype(np.float32) * ext).astype(np.float32)
                bhi = (hi + (rng.uniform(0, 1, hi.shape) * grow * ~keep_hi).astype(np.float32) * ext).astype(np.float32)
            assert (blo <= lo).all() and (bhi >= hi).all()
            some, te, tx = obb_slab_np(q, blo, bhi)
            got = run_driver(driver, "b", np.concatenate([s, blo, bhi], 1).view(np.uint32), tmp_path)
            same_bits(got[:, 0], te); same_bits(got[:, 1], tx)
            assert (got[:, 2] == some).all(), (name, grow)
            ok = q.live
            has = ok & (axis != OS_NONE)
            assert some[has].all(), (name, grow, int((~some[has]).sum()))                  # an empty box: no time below it
            assert (te[has] <= time[has]).all(), (name, grow, int((~(te[has] <= time[has])).sum()))
            assert (some | ~own[0])[ok].all() and (te <= own[1])[ok & own[0]].all() and (tx >= own[2])[ok & own[0]].all()
            assert not np.isnan(te[ok]).any()
            total += int(ok.sum()); with_time += int(has.sum())
    print("boxes %d, of them above a triangle with a time %d" % (total, with_time))
    assert total > 300000 and with_time >= 100000


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


def _magnitude(q, T, c=None):
    """the largest coordinate magnitude involved: origin, triangle, and (where given) the centre at the contact plus the reach g"""
    mag = np.maximum(np.abs(q.O).max(1), np.abs(T).reshape(-1, 9).max(1))
    return mag if c is None else np.maximum(mag, (np.abs(c) + q.H).max(1))


def test_what_the_time_means_by_the_static_box_rule(driver, tmp_path):
    """Independent of swept axes: path and triangle taken into the box's frame in float64 (x -> U x, the rows as given), where
    the box is axis-aligned, then tests/box_ref.py's rule for "a box touches a triangle" (rtk_dev_triangles_in_box), on the
    family of scale 1 with half extents up to 0.3, the times taken from the header through the driver. Where the sweep has a
    time later than min_t: the box at c(t) with its half extents grown by tol touches the triangle, and the box a little
    earlier does not. tol is the position error that the accuracy statement allows, BOUND * 2^-23 of the largest coordinate
    magnitude involved.
    "A little earlier", where every half extent is at least tol: at c(t - delta) with delta = 2 * tol / |D|, the half extents
    shrunk by tol. Where a half extent is below tol (flat boxes, needles, points: they cannot be shrunk): the box as it is, at
    c(t - delta) with delta = (tol + g / cos) / |D|, g = 64 * 2^-23 of the largest coordinate magnitude and cos the cosine
    between the motion and the axis that gives the time in float64: before the contact the gap along that unit axis grows by
    |D| * cos per unit of time, so the true box is apart from the triangle by g and more there. (Cases that have no time from
    an axis in float64 are left out of this half: test_accuracy_against_float64 counts them as disagreeing.)"""
    rng = np.random.RandomState(31)
    s, t = random_family(rng, 100000, 1.0, 3.0, 0.3)
    axis, time = driver_times(driver, s, t, tmp_path)
    q = prepare(s, np.float64)
    use = (axis > OS_START) & (time > s[:, 6])
    assert use.sum() > 15000
    s, t, time, q = s[use], t[use].astype(np.float64), time[use].astype(np.float64), q.at(use)
    c = centre_np(q, time)
    tol = BOUND * 2.0 ** -23 * _magnitude(q, t, c)
    dlen = np.sqrt((q.D * q.D).sum(1))
    F = np.float32
    into = lambda x: np.einsum("njk,nk->nj", q.U, x)                         # scene -> the box's frame
    # (measured from the centre before the rotation, so that the float32 static rule sees numbers of the box's size)
    rel = lambda centre: [into(t[:, k] - centre).astype(F) for k in range(3)]
    grown = (q.half + tol[:, None]).astype(F)
    at = candidate_np(*rel(c), -grown, grown)
    assert at.all(), (int((~at).sum()), np.nonzero(~at)[0][:5])
    # before the time: boxes that can be shrunk
    thick = (q.half >= tol[:, None]).all(1)
    shrunk = np.maximum(q.half - tol[:, None], 0.0).astype(F)
    touches = candidate_np(*rel(centre_np(q, time - 2.0 * tol / dlen)), -shrunk, shrunk)
    assert thick.sum() > 10000 and not touches[thick].any(), (int(touches[thick].sum()), np.nonzero(touches & thick)[0][:5])
    # ... and those that cannot: flat boxes, needles, points, as they are
    axis64 = tri_obbsweep_np(q, t[:, 0], t[:, 1], t[:, 2], np.float64)[0]
    normal = normal_np(q, t[:, 0], t[:, 1], t[:, 2], axis64, np.float64)
    cos = np.abs((normal * q.D).sum(1)) / dlen
    thin = ~thick & (axis64 > OS_START) & (cos > 0)
    with np.errstate(divide="ignore"):
        delta = (tol + 64.0 * 2.0 ** -23 * _magnitude(q, t, c) / cos) / dlen
    half = q.half.astype(F)
    touches = candidate_np(*rel(centre_np(q, time - np.where(thin, delta, 0.0))), -half, half)
    flat = thin & (q.half == 0).any(1)
    print("times %d; before the time: %d boxes shrunk, %d as they are (%d of them flat on an axis), %d left out" % (
        len(s), int(thick.sum()), int(thin.sum()), int(flat.sum()), int((~thick & ~thin).sum())))
    assert thin.sum() > 2500 and flat.sum() > 1500 and (~thick & ~thin).sum() < 20
    assert not touches[thin].any(), (int(touches[thin].sum()), np.nonzero(touches & thin)[0][:5])


def _hit64(s, t, dh=0.0, dt=0.0, do=None):
    """float64, with the half extents grown by dh, the interval widened by dt at both ends (negative: shrunk) and the origin
    moved by do: is there a time?"""
    q = prepare(s, np.float64)
    q.half = np.maximum(q.half + np.asarray(dh)[..., None], 0.0)
    q.H = (np.abs(q.U[:, 0]) * q.half[:, 0:1] + np.abs(q.U[:, 1]) * q.half[:, 1:2]) + np.abs(q.U[:, 2]) * q.half[:, 2:3]
    q.tmin, q.tmax = q.tmin - dt, q.tmax + dt
    if do is not None:
        q.O = q.O + do
    return tri_obbsweep_np(q, t[:, 0], t[:, 1], t[:, 2], np.float64)[0] != OS_NONE


def _clear(s, T, mag, dlen, f64, bound):
    """the box sweep test's definition: the float64 answer stays the same when all half extents and both ends of the interval (in
    the path's units) move by d either way and when the origin moves by d along each axis either way, d = bound * 2^-23 * mag"""
    d = mag * bound * 2.0 ** -23
    base = f64 != OS_NONE
    moves = [dict(dh=-d, dt=-d / dlen), dict(dh=d, dt=d / dlen)]
    moves += [dict(do=np.eye(3)[k] * d[:, None] * sign) for k in range(3) for sign in (-1.0, 1.0)]
    return np.all([_hit64(s, T, **m) == base for m in moves], 0)


def test_accuracy_against_float64(driver, tmp_path):
    """|t - t64| * |D| <= BOUND * 2^-23 * the largest coordinate magnitude involved (origin, triangle, the centre at the contact
    plus the box's reach), on EVERY case that has a time in float32 and in float64 -- starts that overlap, slivers and grazing
    contacts included --, 600 000 cases at each of the five scales, rotations from random unit quaternions, the float32 side of
    every one computed BY THE HEADER through the driver (and the same bits as the numpy reference); at least 5 % of every
    family have one. MEASURED is the worst figure met, BOUND 2.5 times it, rounded up; MEASURED_STEEP / BOUND_STEEP the same
    without grazing contacts (cosine between motion and normal below 0.05) and starts that overlap.
    A case on which float32 and float64 disagree about hit or none is counted apart; no CLEAR one (see _clear) may disagree."""
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
            f64, t64 = tri_obbsweep_np(q, T[:, 0], T[:, 1], T[:, 2], np.float64)
            c = centre_np(q, t64)
            mag = np.where(f64 != OS_NONE, _magnitude(q, T, c), _magnitude(q, T))
            dlen = np.sqrt((q.D * q.D).sum(1))
            evaluated += len(s); fam_n += len(s)
            dis = np.nonzero((f32 != OS_NONE) != (f64 != OS_NONE))[0]
            if len(dis):
                clear = _clear(s[dis], T[dis], mag[dis], dlen[dis], f64[dis], BOUND)
                disagree += len(dis); disagree_clear += int(clear.sum())
            both = (f32 != OS_NONE) & (f64 != OS_NONE)
            err = np.abs(t32.astype(np.float64) - t64) * dlen / mag
            pairs += int(both.sum()); fam_pairs += int(both.sum())
            fam_worst = max(fam_worst, err[both].max())
            normal = normal_np(q, T[:, 0], T[:, 1], T[:, 2], f64, np.float64)
            steep = both & (f32 > OS_START) & (f64 > OS_START) & (np.abs((normal * q.D).sum(1)) >= 0.05 * dlen)
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


def test_against_the_axis_aligned_rule(driver, tmp_path):
    """Axes that are a signed permutation of the unit vectors, row j = +-unit(perm[j]): the same box is the axis-aligned one with
    H[perm[j]] = half[j]. Every case with a time under both rules: the two times differ by no more than the sum of the two
    asserted bounds; no CLEAR case (by the larger of the two bounds) disagrees about hit or none."""
    rng = np.random.RandomState(5)
    n_both = n_dis = n_face = n_same_face = 0
    for sc in SCALES:
        sb, t = box_family(rng, 100000, *sc)
        U, perm = signed_permutations(rng, len(sb))
        s = with_axes(sb, U)
        for j in range(3):
            s[:, 8 + j] = sb[np.arange(len(sb)), 8 + perm[:, j]]
        q32 = prepare(s)
        assert q32.live.all() and (q32.H == sb[:, 8:11]).all()               # (the reach is the axis-aligned box's, exactly)
        f_obb, t_obb = driver_times(driver, s, t, tmp_path)
        f_box, t_box = boxsweep_ref.tri_boxsweep_np(boxsweep_ref.prepare(sb), t[:, 0], t[:, 1], t[:, 2])
        q = prepare(s, np.float64)
        T = t.astype(np.float64)
        f64, t64 = tri_obbsweep_np(q, T[:, 0], T[:, 1], T[:, 2], np.float64)
        mag = np.where(f64 != OS_NONE, _magnitude(q, T, centre_np(q, t64)), _magnitude(q, T))
        dlen = np.sqrt((q.D * q.D).sum(1))
        both = (f_obb != OS_NONE) & (f_box != boxsweep_ref.BS_NONE)
        err = np.abs(t_obb.astype(np.float64) - t_box.astype(np.float64)) * dlen / mag
        print("scales %s: %d with a time under both rules, worst difference %.2f * 2^-23" % (sc, both.sum(), err[both].max() * 2.0 ** 23))
        assert both.sum() > 5000 and err[both].max() <= (BOUND + BOX_BOUND) * 2.0 ** -23
        dis = np.nonzero((f_obb != OS_NONE) != (f_box != boxsweep_ref.BS_NONE))[0]
        if len(dis):
            assert not _clear(s[dis], T[dis], mag[dis], dlen[dis], f64[dis], max(BOUND, BOX_BOUND)).any()
        n_both += int(both.sum()); n_dis += len(dis)
        # a contact that both rules give to a face of the box: the same face
        face = both & (f_obb >= OS_U0) & (f_obb <= OS_U2) & (f_box >= boxsweep_ref.BS_BOX_X) & (f_box <= boxsweep_ref.BS_BOX_Z)
        n_face += int(face.sum()); n_same_face += int((perm[face, f_obb[face] - OS_U0] == f_box[face] - boxsweep_ref.BS_BOX_X).sum())
    print("%d with a time under both, %d disagree (none clear); %d on a face of the box under both, %d on the same one" % (n_both, n_dis, n_face, n_same_face))
    assert n_face > 1000 and n_same_face > 0.99 * n_face


def test_header_symbols_sizes_and_argtypes(api):
    from rtk_amd import types
    text = open(os.path.join(ROOT, "include", "rtk_amd.h")).read()
    for word in ("typedef struct rtk_obb_sweep { float origin[3], direction[3], min_t, max_t, half[3], axes[9]; } rtk_obb_sweep;",
                 "int rtk_dev_sweep_obbs(const rtk_dev_scene *ds, const rtk_obb_sweep *d_sweeps, size_t num_sweeps, const rtk_ray_list *list,",
                 "int rtk_dev_sweep_obbs_any(", "int rtk_dev_sweep_obbs_counted(", "uint32_t rtk_amd_obbsweep_stack_entries(void);",
                 "LOWEST PRIMITIVE ID AMONG EQUAL TIMES", "CLOSED interval", "d_after is refused", "---- Oriented box sweeps", "NOT NECESSARILY A POINT OF CONTACT",
                 "THE AXES ARE ORTHONORMAL TO WITHIN 2^-10", "UP TO ROUNDING, NOT BIT FOR BIT", "never a NaN"):
        assert word in text, word
    assert "an oriented box is not offered" not in text.lower() and "not offered" not in text[text.index("---- Box sweeps"):text.index("---- Capsule sweeps")]
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "oriented box is not offered" not in integ.lower() and "Oriented box sweeps" in integ and "rtk_dev_sweep_obbs" in integ
    assert text.index("---- Box sweeps") < text.index("---- Capsule sweeps") < text.index("---- Oriented box sweeps") < text.index("---- Every hit along a ray")
    check = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_layout_check.h")).read()
    assert "sizeof(rtk_obb_sweep) == 80" in check
    assert types.OBB_SWEEP_DTYPE.itemsize == 80 and types.OBB_SWEEP_DTYPE.names == ("origin", "direction", "min_t", "max_t", "half", "axes")
    assert types.OBB_SWEEP_DTYPE.fields["half"][1] == 32 and types.OBB_SWEEP_DTYPE.fields["axes"][1] == 44 and types.OBB_SWEEP_DTYPE.fields["axes"][0].shape == (3, 3)
    L = api.lib()
    for name in ("rtk_dev_sweep_obbs", "rtk_dev_sweep_obbs_any", "rtk_dev_sweep_obbs_counted", "rtk_amd_obbsweep_stack_entries"):
        assert name in api.RTK_AMD_H_SYMBOLS and hasattr(L, name), name
    assert L.rtk_dev_sweep_obbs.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(api.RayList), C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.POINTER(api.DevFilter), C.c_void_p]
    assert L.rtk_dev_sweep_obbs_any.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(api.RayList), C.c_void_p, C.POINTER(api.DevFilter), C.c_void_p]
    assert L.rtk_dev_sweep_obbs_counted.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(api.DevFilter),
                                                       C.POINTER(api.TraceCounters)]
    assert L.rtk_dev_sweep_obbs.restype == C.c_int and L.rtk_dev_sweep_obbs_any.restype == C.c_int and L.rtk_dev_sweep_obbs_counted.restype == C.c_int
    assert L.rtk_amd_obbsweep_stack_entries.restype == C.c_uint32 and 1 <= L.rtk_amd_obbsweep_stack_entries() <= 64
    for name in ("sweep_obbs", "sweep_obbs_device", "sweep_obbs_any_device", "sweep_obbs_counted", "obb_path_blocked"):
        assert callable(getattr(api.DeviceScene, name)), name
    # the rotation argument of the numpy conveniences: matrices (rows are the axes) and quaternions (x, y, z, w), one or one per query
    rng = np.random.RandomState(3)
    quat = rng.standard_normal((7, 4))
    rows = quat_rows(quat)
    got = api.obb_axes(quat * 3.0, 7)                                        # (normalised in float64)
    assert got.dtype == np.float32 and got.shape == (7, 3, 3) and np.abs(got - rows).max() < 2.0 ** -24     # (rounded once, from float64)
    assert prepare(with_axes(np.ones((7, 11), np.float32), got)).live.all()
    rows32 = rows.astype(np.float32)
    assert api.obb_axes(rows, 7).tobytes() == rows32.tobytes() and api.obb_axes(rows[0], 7).tobytes() == np.repeat(rows32[:1], 7, 0).tobytes()
    assert api.obb_axes(quat[0], 7).tobytes() == np.repeat(got[:1], 7, 0).tobytes()
    assert api.obb_axes([0, 0, 0, 1], 2).tobytes() == np.repeat(np.eye(3, dtype=np.float32)[None], 2, 0).tobytes()
    z90 = api.obb_axes([0, 0, np.sqrt(0.5), np.sqrt(0.5)], 1)[0]             # a quarter turn about z takes x to y: the first axis is +y
    assert np.allclose(z90, [[0, 1, 0], [-1, 0, 0], [0, 0, 1]], atol=1e-7)
    with pytest.raises(api.RtkError):
        api.obb_axes(np.zeros((7, 5)), 7)


def test_refusals_need_no_device(api):
    L = api.lib()
    buf = C.create_string_buffer(128)
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
        assert L.rtk_dev_sweep_obbs(*args) == ERR_BAD_ARG, args
        assert "rtk_dev_sweep_obbs:" in api.last_error()
    assert "d_after" in api.last_error() or "mesh mask" in api.last_error()
    assert L.rtk_dev_sweep_obbs(dummy, dummy, 4, None, dummy, None, None, bad_filters[1], None) == ERR_BAD_ARG and "d_after" in api.last_error()
    # the any-hit form: (ds, sweeps, n, list, blocked, filter, stream)
    for args in [(None, dummy, 4, None, dummy, None, None), (dummy, None, 4, None, dummy, None, None), (dummy, dummy, 4, None, None, None, None),
                 (dummy, dummy, 1 << 32, None, dummy, None, None)] + [(dummy, dummy, 4, l, dummy, None, None) for l in bad_lists] \
            + [(dummy, dummy, 4, None, dummy, f, None) for f in bad_filters]:
        assert L.rtk_dev_sweep_obbs_any(*args) == ERR_BAD_ARG, args
        assert "rtk_dev_sweep_obbs_any:" in api.last_error()
    # the counting form: (ds, sweeps, n, records, centres, normals, filter, counters)
    ctr = api.TraceCounters()
    for args in [(dummy, dummy, 4, dummy, None, None, None, None), (None, dummy, 4, dummy, None, None, None, C.byref(ctr)),
                 (dummy, None, 4, dummy, None, None, None, C.byref(ctr)), (dummy, dummy, 4, None, None, None, None, C.byref(ctr)),
                 (dummy, dummy, 1 << 32, dummy, None, None, None, C.byref(ctr)), (dummy, dummy, 4, dummy, None, None, bad_filters[1], C.byref(ctr))]:
        assert L.rtk_dev_sweep_obbs_counted(*args) == ERR_BAD_ARG, args
        assert "rtk_dev_sweep_obbs_counted" in api.last_error()
    ctr.rays = 5
    assert L.rtk_dev_sweep_obbs_counted(dummy, None, 0, None, None, None, None, C.byref(ctr)) == 0 and ctr.rays == 0
    # no queries: nothing to do, nothing launched
    assert L.rtk_dev_sweep_obbs(dummy, None, 0, None, None, None, None, None, None) == 0
    assert L.rtk_dev_sweep_obbs(dummy, dummy, 0, C.byref(ray_list()), dummy, dummy, dummy, C.byref(dev_filter()), None) == 0
    assert L.rtk_dev_sweep_obbs_any(dummy, None, 0, None, None, None, None) == 0
