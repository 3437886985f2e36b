"""Closest points on an instanced world without a GPU: the rule of rtk_amd/csrc/rtk_world_closest_rule.h, run by
tests/world_closest_rule_driver.cpp (built plain and once more under the address and undefined-behaviour sanitizers, the flags of
tests/test_world_cpu.py), against numpy in the stated order (tests/world_closest_ref.py), bit for bit: the placed box equals numpy
and the min / max over the eight placed corners, every placed point lies in the placed box and no bound exceeds a dist2 below
it -- the exactness claim, with no exception allowed --, the driver's brute force equals the reference's; and the symbols,
argtypes and refusals of the interface that need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import world_closest_ref as R
from tests import world_ref
from tests.test_world_cpu import ERR_BAD_ARG, _hex, placements_under_test, run_driver
from tests.world_ref import F, PRIM_NONE, RTK_INF, placement, rotation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if request.param == "sanitized" else []
    exe = str(tmp_path_factory.mktemp("world_closest_rule_" + request.param) / "world_closest_rule_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-mfma", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + extra +
                          ["-I" + os.path.join(ROOT, "rtk_amd", "csrc"), os.path.join(ROOT, "tests", "world_closest_rule_driver.cpp"), "-o", exe])
    return exe


def placements():
    """[n, 12] float32: the live placements of tests/test_world_cpu.py (rotations, scales 1e-3 to 1e3, a mirror, denormal
    translations) and, for the box, what an inverse would refuse but a box must still take: shears, zero entries and zero rows in
    the matrix, negative zeros, mirrors in every axis, denormal entries"""
    rng = np.random.RandomState(17)
    out = [c[1] for c in placements_under_test() if c[2]]
    shear = np.array([[1, 0.7, -0.3], [0, 1, 2.5], [0, 0, 1]])
    out += [placement(shear, (1, -2, 3)), placement(shear.T @ np.diag([-2.0, 0.5, 1e3]), (0, 0, 0)),
            placement(np.diag([-1.0, -1.0, -1.0]), (5, 5, 5)), placement(np.array([[0, 1, 0], [0, 0, -1], [1, 0, 0]]), (-1, 0, 1)),
            placement(np.array([[1, 2, 3], [0, 0, 0], [4, 5, 6]]), (1, 2, 3)), placement(np.zeros((3, 3)), (7, 8, 9)),
            placement(np.array([[-0.0, 1, 0], [1, -0.0, 0], [0, 0, -0.0]]), (0, 0, 0)),
            placement(np.eye(3) * 1e-42, (1e-40, 0, 1e-44)), placement(rotation([1, 1, 1], 1.0) * 1e-3, (1e3, -1e3, 0))]
    for _ in range(60):
        A = rng.standard_normal((3, 3)) * rng.choice([1e-3, 1.0, 1e3])
        A[rng.uniform(size=(3, 3)) < 0.2] = 0
        out.append(placement(A, np.abs(rng.choice([0, 1]) * rng.uniform(-100, 100, 3)) * rng.choice([-1, 1], 3) + 0.0))      # (+ 0.0: no translation of -0)
    return np.array(out, F)


def random_boxes(n, rng):
    """(lo, hi) [n, 3]: sizes 1e-3 to 1e3, a tenth flat in an axis, some denormal"""
    scale = (10.0 ** rng.uniform(-3, 3, (n, 1)))
    c = rng.uniform(-4, 4, (n, 3)) * scale
    e = rng.uniform(0, 1, (n, 3)) * scale
    e[rng.uniform(size=(n, 3)) < 0.1] = 0
    lo, hi = (c - e).astype(F), (c + e).astype(F)
    den = rng.uniform(size=n) < 0.02
    lo[den], hi[den] = (lo[den] * F(1e-42)).astype(F), (hi[den] * F(1e-42)).astype(F)
    return np.minimum(lo, hi), np.maximum(lo, hi)


def test_rule_header_includes_only_the_two_rule_headers():
    text = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_world_closest_rule.h")).read()
    assert [l.split()[1] for l in text.splitlines() if l.startswith("#include")] == ['"rtk_world_rule.h"', '"rtk_closest_rule.h"']
    assert "hip/" not in text and "math.h" not in text and "<cmath>" not in text
    for word in ("THE PLACED TRIANGLE", "THE PLACED BOX", "WHY IT IS EXACT", "monotone", "THE TOP TREE", "BETTER THAN", "FORWARD", "No HIP, no libm",
                 "ACROSS INSTANCES IS DECIDED", "without a\n//    margin", "DESIGN.md 3.23.1"):
        assert word in text, word
    drv = open(os.path.join(ROOT, "tests", "world_closest_rule_driver.cpp")).read()
    assert [l.split()[1] for l in drv.splitlines() if l.startswith("#include") and '"' in l] == ['"rtk_world_closest_rule.h"']
    mk = open(os.path.join(ROOT, "rtk_amd", "csrc", "Makefile")).read()
    for name in ("rtk_world_closest.hip", "rtk_world_closest_rule.h", "rtk_world_internal.h", "rtk_world.hip", "rtk_world_rule.h"):
        assert name in mk, name
    # the world object is defined once, in the internal header both walks include
    for name, n in (("rtk_world_internal.h", 1), ("rtk_world.hip", 0), ("rtk_world_closest.hip", 0)):
        assert open(os.path.join(ROOT, "rtk_amd", "csrc", name)).read().count("struct rtk_dev_world {") == n, name


def test_placed_box_equals_numpy_and_the_eight_corners(driver, tmp_path):
    rng = np.random.RandomState(23)
    P = placements()
    n = 100000
    m = P[rng.randint(0, len(P), n)]
    m[:len(P)] = P                                                           # every placement at least once
    lo, hi = random_boxes(n, rng)
    rows = np.concatenate([m, lo, hi], 1)
    got = np.array(run_driver(driver, ["b " + _hex(r) for r in rows], tmp_path, "box"), np.uint32)
    corners = np.array(run_driver(driver, ["k " + _hex(r) for r in rows], tmp_path, "corners"), np.uint32)
    wlo, whi = R.placed_box_np(m, lo, hi)
    want = np.concatenate([wlo, whi], 1)
    assert np.isfinite(want).all() and got.shape == (n, 6)
    assert (got == want.view(np.uint32)).all()
    clo, chi = R.corners_box_np(m, lo, hi)
    assert (corners == np.concatenate([clo, chi], 1).view(np.uint32)).all()
    # the claim: the six rows are the extremes of the eight corners. As values everywhere; as bits except the sign of a zero,
    # which can be another corner's only under a translation of -0 (no placement here has one: bit for bit then)
    assert (got.view(F) == corners.view(F)).all()
    assert (got == corners).all()
    assert (wlo <= whi).all()
    assert ((m[:, 0] < 0) | (m[:, 5] < 0) | (m[:, 10] < 0)).mean() > 0.2 and (lo == hi).any(1).mean() > 0.1
    with np.errstate(all="ignore"):
        assert (np.abs(lo) < F(1.2e-38)).all(1).sum() > 100                  # denormal boxes
    # a translation of -0: equal as values, and the signs of the zeros are the only difference there can be
    mz = placement(np.array([[0, 0, 0], [0, 1, 0], [0, 0, 0]]), (-0.0, -0.0, -0.0))
    row = np.concatenate([mz, [-1, -1, -1], [1, 1, 1]]).astype(F)
    a = np.array(run_driver(driver, ["b " + _hex(row)], tmp_path, "zero_b"), np.uint32)
    b = np.array(run_driver(driver, ["k " + _hex(row)], tmp_path, "zero_k"), np.uint32)
    assert (a.view(F) == b.view(F)).all() and ((a ^ b) & 0x7fffffff == 0).all()


def test_containment_and_the_bound_without_exception(driver, tmp_path):
    """A million random points inside random boxes, under every placement: each placed point lies inside the placed box, and
    rtk_closest_box_bound of the placed box is at most the dist2 of a triangle of such points"""
    P = placements()
    rounds = -(-1000000 // (3 * len(P))) + 1
    lines = []
    for k, m in enumerate(P):
        scale = np.array([10.0 ** ((k % 7) - 3)], F)
        lines.append("c %s %d %d %s" % (_hex(m), 1000 + k, rounds, _hex(scale)))
    got = run_driver(driver, lines, tmp_path, "contain")
    assert 3 * rounds * len(P) >= 1000000
    # (run_driver reads its output as hexadecimal words: zero is zero)
    assert [g for g in got if g != [0, 0]] == []
    # the same in numpy on a sample: placed points against the placed box
    rng = np.random.RandomState(29)
    n = 20000
    m = P[rng.randint(0, len(P), n)]
    lo, hi = random_boxes(n, rng)
    t = rng.uniform(0, 1, (n, 3)).astype(F)
    with np.errstate(all="ignore"):
        x = np.clip((lo + (hi - lo) * t).astype(F), lo, hi)
    wlo, whi = R.placed_box_np(m, lo, hi)
    w = world_ref.place_np(m, x)
    assert ((w >= wlo) & (w <= whi)).all()


def small_world():
    rng = np.random.RandomState(31)
    scenes = [world_ref.cube(), world_ref.icosphere(1)]
    which = np.array([0, 1, 0, 1, 0, 0], np.uint32)
    places = world_ref.random_placements(6, rng, 3.0)
    places[2] = placement(np.diag([-1.0, 2.0, 0.5]) @ rotation([1, 2, 3], 0.4), (1, 0, -1))
    places[4] = placement(np.array([[1, 2, 3], [1, 2, 3], [0, 0, 1]]), (0, 0, 0))      # singular: dead
    places[5] = places[0]                                                               # an exact duplicate: ties go to instance 0
    return scenes, which, places


def test_driver_brute_force_equals_the_reference(driver, tmp_path):
    scenes, which, places = small_world()
    rng = np.random.RandomState(37)
    points, max2 = R.make_queries(scenes, which, places, rng, 150, 150, 40, 30)
    unlimited, _, _ = R.brute_force(scenes, which, places, points[300:340], np.full(40, RTK_INF, F))
    max2[300:340] = unlimited[:, 0].view(F) * F(1e-6)
    mask = np.array([True, True, True, False, True, True])
    ignore = rng.randint(0, 7, len(points)).astype(np.uint32)
    ignore[::5] = PRIM_NONE
    live = R.live_instances(scenes, which, places)
    assert live.tolist() == [True, True, True, True, False, True]
    for use_mask, use_ignore in ((False, False), (True, True)):
        want = R.brute_force(scenes, which, places, points, max2, mask if use_mask else None, ignore if use_ignore else None)
        pruned = R.brute_force(scenes, which, places, points, max2, mask if use_mask else None, ignore if use_ignore else None, prune=True)
        assert all((a == b).all() for a, b in zip(want, pruned))                 # (the pruned form the GPU test uses on its large worlds)
        lines = ["s %d %s" % (len(t), _hex(t)) for t in scenes]
        lines += ["i %d %d %s" % (which[k], int(live[k] and (not use_mask or mask[k])), _hex(places[k])) for k in range(len(which))]
        ign = ignore if use_ignore else np.full(len(points), PRIM_NONE, np.uint32)
        lines += ["q %s %x" % (_hex(np.concatenate([points[i], max2[i:i + 1]])), ign[i]) for i in range(len(points))]
        got = np.array(run_driver(driver, lines, tmp_path, "world%d" % use_mask), np.uint32)
        rec, inst, pts = want
        bad = (got[:, [0, 1, 2, 3]] != rec).any(1) | (got[:, 4] != inst) | (got[:, 5:8] != pts).any(1)
        assert not bad.any(), (np.flatnonzero(bad)[:5], got[bad][:3], rec[bad][:3], inst[bad][:3])
        hit = rec[:, 3] != PRIM_NONE
        assert hit[:300].all() and not hit[300:].any() and (inst[~hit] == PRIM_NONE).all()
        assert (rec[~hit, 0] == max2[~hit].view(np.uint32)).all() and (pts[~hit] == points[~hit].view(np.uint32)).all()
        if not use_mask:
            assert (inst != 5).all() and (inst == 0).sum() > 20                 # the duplicate never wins


def test_header_symbols_and_argtypes(api):
    text = open(os.path.join(ROOT, "include", "rtk_amd.h")).read()
    for word in ("int rtk_dev_world_closest_points(const rtk_dev_world *w, const rtk_point_query *d_queries, size_t num_queries,",
                 "int rtk_dev_world_closest_points_counted(const rtk_dev_world *w, const rtk_point_query *d_queries, size_t num_queries,",
                 "uint32_t rtk_amd_world_closest_stack_entries(void);", "THE LOWEST INSTANCE NUMBER", "FLAT PLACED TWIN", "FORWARD placement"):
        assert word in text, word
    assert "other query kinds on a world are not there yet" not in text
    assert "not there yet" not in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    L = api.lib()
    for name in ("rtk_dev_world_closest_points", "rtk_dev_world_closest_points_counted"):
        assert name in api.RTK_AMD_H_SYMBOLS and getattr(L, name).restype == C.c_int, name
    assert len(L.rtk_dev_world_closest_points.argtypes) == 9 and len(L.rtk_dev_world_closest_points_counted.argtypes) == 8
    assert L.rtk_amd_world_closest_stack_entries() > 0 and "rtk_amd_world_closest_stack_entries" in api.RTK_AMD_H_SYMBOLS
    for name in ("closest_points_device", "closest_points_counted", "closest_points"):
        assert callable(getattr(api.DeviceWorld, name)), name
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md", "docs/HISTORY.md"):
        assert "rtk_dev_world_closest_points" in open(os.path.join(ROOT, doc)).read(), doc


def test_refusals_need_no_device(api):
    L = api.lib()
    dummy = C.cast(C.create_string_buffer(64), C.c_void_p)                   # (what is refused is refused before the world is looked at)
    count = C.cast(C.create_string_buffer(8), C.c_void_p)

    def ray_list(**kw):
        l = api.RayList()
        l.struct_size, l.flags, l.d_ids, l.d_count = C.sizeof(api.RayList), 0, None, count.value
        for k, v in kw.items():
            setattr(l, k, v)
        return C.byref(l)

    def filt(**kw):
        f = api.WorldFilter()
        f.struct_size = C.sizeof(api.WorldFilter)
        for k, v in kw.items():
            setattr(f, k, v)
        return C.byref(f)
    #            world  queries n  list  filter records instances points stream
    for args in ((None, dummy, 4, None, None, dummy, None, None, None), (dummy, None, 4, None, None, dummy, None, None, None),
                 (dummy, dummy, 4, None, None, None, None, None, None),
                 (dummy, dummy, 4, ray_list(struct_size=8), None, dummy, None, None, None), (dummy, dummy, 4, ray_list(flags=1), None, dummy, None, None, None),
                 (dummy, dummy, 4, ray_list(d_count=None), None, dummy, None, None, None), (dummy, dummy, 1 << 32, None, None, dummy, None, None, None),
                 (dummy, dummy, 1 << 32, ray_list(), None, dummy, None, None, None),
                 (dummy, dummy, 4, None, filt(struct_size=16), dummy, None, None, None), (dummy, dummy, 4, None, filt(flags=1), dummy, None, None, None),
                 (dummy, dummy, 4, None, filt(d_instance_mask=dummy.value, instance_mask_bits=0), dummy, None, None, None)):
        assert L.rtk_dev_world_closest_points(*args) == ERR_BAD_ARG, args
        assert "rtk_dev_world_closest_points" in api.last_error()
    # no queries: nothing to do, nothing launched (the world is not even looked at)
    assert L.rtk_dev_world_closest_points(dummy, None, 0, None, None, None, None, None, None) == 0
    assert L.rtk_dev_world_closest_points(dummy, None, 0, ray_list(), filt(), None, None, None, None) == 0
    ctr = api.TraceCounters()
    assert L.rtk_dev_world_closest_points_counted(dummy, dummy, 0, None, dummy, None, None, C.byref(ctr)) == 0
    assert L.rtk_dev_world_closest_points_counted(dummy, dummy, 4, None, dummy, None, None, None) == ERR_BAD_ARG
    assert "NULL counters" in api.last_error()
    assert L.rtk_dev_world_closest_points_counted(None, dummy, 4, None, dummy, None, None, C.byref(ctr)) == ERR_BAD_ARG
    assert "rtk_dev_world_closest_points_counted" in api.last_error()
