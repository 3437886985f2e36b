"""Winding numbers without a GPU: the rule of rtk_amd/csrc/rtk_winding_rule.h, run by tests/winding_rule_driver.cpp (built plain
and once more under the address and undefined-behaviour sanitizers), against numpy float32 arithmetic in the stated order
(tests/winding_ref.py), bit for bit; the float32 sum against the float64 one on the fixtures of the GPU test; and the parts of the
interface that need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import winding_ref
from tests.winding_ref import F, accept_np, brute32, brute64, far_np, fixtures, query_points, slot_np, tri_moments_np, triangle_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_BAD_ARG = -2
# the ceiling the exact form is held to (500 x below the 0.5 that decides inside); the float32 sum on the CPU is held to it too
EXACT_CEILING = 1e-3


def _build(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp(name) / "winding_rule_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-mfma", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + extra +
                          ["-I" + os.path.join(ROOT, "rtk_amd", "csrc"), os.path.join(ROOT, "tests", "winding_rule_driver.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    """The driver built against the header alone (no HIP include path, -Wall -Werror, no FMA contraction as in the library):
    once as it is and once with both sanitizers, the flags of tests/test_sign_cpu.py. Every test below runs with each."""
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if request.param == "sanitized" else []
    return _build(tmp_path_factory, "winding_rule_" + request.param, extra)


def _hex(row):
    return " ".join("%x" % w for w in np.ascontiguousarray(row, F).view(np.uint32).ravel().tolist())


def run_driver(exe, lines, tmp_path, name):
    path = str(tmp_path / (name + ".txt"))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = r.stdout.split("\n")
    assert out[-2] == "ok"
    return out[:-2]


def same_bits(got, want):
    """Bit for bit, except where the expected value is NaN: there only "it is NaN" is promised."""
    got = np.ascontiguousarray(got, np.uint32)
    want = np.ascontiguousarray(want, F)
    nan = np.isnan(want)
    assert (np.isnan(got.view(F)) == nan).all()
    bad = (got != want.view(np.uint32)) & ~nan
    assert not bad.any(), (np.argwhere(bad)[:5], got[bad][:5], want.view(np.uint32)[bad][:5])


def special_cases():
    """(p, a, b, c): a point on a corner, on an edge, in the face plane outside and inside the triangle, and zero-area triangles"""
    a, b, c = [0, 0, 0], [2, 0, 0], [0, 2, 0]
    tri = [a, b, c]
    rows = [([0, 0, 0], *tri), ([2, 0, 0], *tri), ([0, 2, 0], *tri),                     # on each corner
            ([1, 0, 0], *tri), ([0, 0.5, 0], *tri), ([1, 1, 0], *tri),                   # on each edge
            ([3, 3, 0], *tri), ([-1, -1, 0], *tri), ([5, 0, 0], *tri),                   # in the plane, outside
            ([0.5, 0.5, 0], *tri),                                                        # in the plane, inside: the jump, 1/2
            ([0.5, 0.5, 1], a, b, b), ([0.5, 0.5, 1], a, a, a), ([0.3, 0.2, 1], a, [1, 1, 1], [2, 2, 2]),   # zero area: b = c, a = b = c, collinear
            ([1, 0, 0], a, b, b), ([0.5, 0.5, 1e-3], *tri), ([0.5, 0.5, -1e-3], *tri)]
    return np.array(rows, F)


def test_rule_header_includes_no_hip_and_says_what_it_must():
    text = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_winding_rule.h")).read()
    assert [l.split()[1] for l in text.splitlines() if l.startswith("#include")] == ["<stdint.h>", '"rtk_sign_rule.h"']
    assert "hip/" not in text and "math.h" not in text and "atan2f" not in text and "atanf" not in text
    for word in ("TRIANGLE TERM", "FAR TERM", "ACCEPT TEST", "MOMENTS OF A CHILD SLOT", "rtk_sign_angle", "RTK_SIGN_SQRT", "0x3da2f983",
                 "IN SLOT ORDER", "FROM THE BOX", "not the exact maximum", "THE ORDER OF THE SUMS FOLLOWS THE TREE", "WHAT IS PROMISED",
                 "NOT PROMISED BIT FOR BIT ACROSS TREES", "ON A CORNER", "DEGENERATE", "fp contract(off)", "No HIP, no libm"):
        assert word in text, word
    drv = open(os.path.join(ROOT, "tests", "winding_rule_driver.cpp")).read()
    assert [l.split()[1] for l in drv.splitlines() if l.startswith("#include") and '"' in l] == ['"rtk_winding_rule.h"']
    mk = open(os.path.join(ROOT, "rtk_amd", "csrc", "Makefile")).read()
    assert "rtk_winding_rule.h" in mk and "rtk_winding.hip" in mk


def test_terms_match_numpy_bit_for_bit(driver, tmp_path):
    """The triangle term and the far term over random triangles and points at four scales, and the special places: a point on a
    corner, on an edge, in the face plane, and zero-area triangles. The special values are also stated outright."""
    rng = np.random.RandomState(1)
    rows = [special_cases().reshape(-1, 12)]
    for scale in (1.0, 1e-3, 1e3, 37.0):
        t = rng.uniform(-1, 1, (400, 4, 3)) * scale
        t[200:, 0] = t[200:, 1:].mean(1) + rng.standard_normal((200, 3)) * 0.05 * scale          # near the triangle
        rows.append(t.reshape(-1, 12))
    rows = np.concatenate(rows).astype(F)
    got = run_driver(driver, ["t " + _hex(r) for r in rows], tmp_path, "tri")
    want = triangle_np(rows[:, 0:3], rows[:, 3:6], rows[:, 6:9], rows[:, 9:12])
    same_bits([int(x, 16) for x in got], want)
    sp = want[:len(special_cases())]
    assert (sp[:3].view(np.uint32) == 0).all()                               # on a corner: +0
    assert (sp[6:9] == 0).all() and (sp[10:12] == 0).all()                   # in the plane outside; two or three equal corners: exactly 0
    assert abs(sp[12]) < 1e-6                                                # three distinct corners on a line: 0 up to the rounding of num
    assert abs(abs(sp[9]) - 0.5) < 1e-6                                      # in the plane inside: the jump
    assert abs(sp[14] + 0.5) < 2e-3 and abs(sp[15] - 0.5) < 2e-3             # just above (outward side: behind the face, -1/2), just below
    # Against float64, for the points drawn apart from their triangle (the first 200 of each scale; next to a triangle den is a
    # difference of nearly equal numbers and its float rounding, not the arctangent, sets the error). The budget: the angle's
    # asserted error, 2 * 3.64e-6 / (4 pi) = 5.8e-7, and as much again for the rounding of num and den.
    k = np.arange(len(rows)) - len(special_cases())
    apart = (k >= 0) & (k % 400 < 200)
    ref = np.array([brute64(r[3:].reshape(1, 3, 3), r[None, :3])[0] for r in rows[apart]])
    err = np.abs(want[apart] - ref).max()
    print("triangle term against float64, %d pairs apart: worst %.3e" % (apart.sum(), err))
    assert err <= 2 * (2 * 3.64e-6 / (4 * np.pi))

    f = rng.uniform(-1, 1, (600, 3, 3)).astype(F)
    f[:, 2] = f[:, 0] + rng.standard_normal((600, 3)) * rng.choice([0.1, 3.0, 100.0], (600, 1))
    f[0, 2] = f[0, 0]                                                        # P == p: 0 / 0, a NaN (never taken: the accept test is false there)
    got = run_driver(driver, ["f " + _hex(r) for r in f.reshape(-1, 9)], tmp_path, "far")
    same_bits([int(x, 16) for x in got], far_np(f[:, 0], f[:, 1], f[:, 2]))


def test_accept_test(driver, tmp_path):
    """r2 > (beta * R)^2; false for a NaN R, a NaN r2 and for beta * R that overflows (also when only its square does)."""
    cases = [(5.0, 2.0, 1.0, 1), (4.0, 2.0, 1.0, 0), (3.9, 2.0, 1.0, 0), (1.0, 2.0, 0.0, 1), (0.0, 2.0, 0.0, 0),
             (1e30, 2.0, np.nan, 0), (np.nan, 2.0, 1.0, 0), (3e38, 2.0, 3e38, 0), (3e38, 2.0, 1e20, 0), (np.inf, 2.0, 3e38, 0),
             (1e30, 2.0, np.inf, 0), (17.0, 4.0, 1.0, 1), (16.0, 4.0, 1.0, 0), (np.inf, 2.0, 1.0, 1)]
    arr = np.array([c[:3] for c in cases], F)
    got = run_driver(driver, ["c " + _hex(r) for r in arr], tmp_path, "accept")
    assert [int(x) for x in got] == [c[3] for c in cases]
    assert accept_np(arr[:, 0], arr[:, 1], arr[:, 2]).astype(int).tolist() == [c[3] for c in cases]


def test_moments_match_numpy_bit_for_bit(driver, tmp_path):
    rng = np.random.RandomState(2)
    t = rng.uniform(-3, 3, (300, 3, 3)).astype(F)
    t[0, 1] = t[0, 0]                                                        # zero area
    got = run_driver(driver, ["m " + _hex(r) for r in t.reshape(-1, 9)], tmp_path, "moments")
    want = tri_moments_np(t[:, 0], t[:, 1], t[:, 2])
    same_bits([[int(x, 16) for x in l.split()] for l in got], want)
    # a slot from sums and a box: the weighted centre, and the box's centre when the area is 0, infinite or a NaN; R covers the box from P
    lo, hi = t.min(1), t.max(1)
    sums = want.copy()
    sums[1, 3] = 0.0; sums[2, 3] = np.inf; sums[3, 3] = np.nan
    got = run_driver(driver, ["s " + _hex(np.concatenate([s, l, h])) for s, l, h in zip(sums, lo, hi)], tmp_path, "slots")
    want_slots = np.array([slot_np(s, l, h) for s, l, h in zip(sums, lo, hi)])
    same_bits([[int(x, 16) for x in l.split()] for l in got], want_slots)
    for k in (1, 2, 3):
        assert (want_slots[k, 3:6] == (lo[k] * F(0.5) + hi[k] * F(0.5))).all()
    corners = np.stack([np.where(np.array(m)[None, :], hi, lo) for m in np.ndindex(2, 2, 2)], 1).astype(np.float64)      # [T, 8, 3]
    reach = np.linalg.norm(corners - want_slots[:, None, 3:6].astype(np.float64), axis=2).max(1)
    assert (want_slots[:, 6] >= reach).all() and (want_slots[:, 6] >= 0).all()


@pytest.fixture(scope="module")
def sums():
    """name -> (tris, points, float32 sum in row order, float64 sum): 200 points per fixture, none within 5 % of the size of the surface"""
    out = {}
    for k, (name, (tris, size)) in enumerate(fixtures().items()):
        pts = query_points(tris, size, 200, 40 + k)
        out[name] = (tris, pts, brute32(tris, pts), brute64(tris, pts))
    return out


def test_float32_sum_agrees_with_float64_on_the_fixtures(driver, sums, tmp_path):
    """The driver's sum is numpy's, bit for bit; and it is the float64 sum within the ceiling the exact form is held to. The known
    values: 1 inside and 0 outside the closed shapes."""
    for name, (tris, pts, w32, w64) in sums.items():
        lines = ["w %d" % len(tris)] + [_hex(r) for r in tris.reshape(-1, 9)] + ["q " + _hex(p) for p in pts[:50]]
        got = run_driver(driver, lines, tmp_path, "sum_" + name.replace(" ", "_"))
        same_bits([int(x, 16) for x in got], w32[:50])
        err = np.abs(w32.astype(np.float64) - w64).max()
        print("%s: %d triangles, float32 sum against float64: worst %.3e" % (name, len(tris), err))
        assert err <= EXACT_CEILING, (name, err)
        if name != "open cube":
            assert np.abs(w64 - np.round(w64)).max() < 1e-9 and set(np.round(w64).astype(int)) == {0, 1}, name
        else:
            assert ((w64 > 0.01) & (w64 < 0.99)).any()


def test_known_values_in_float64():
    """the reference itself: 5/6 at the centre of the cube without a face, 2 inside two nested spheres, -1 inside a flipped one"""
    centre = np.zeros((1, 3))
    assert abs(brute64(winding_ref.open_cube(), centre)[0] - 5.0 / 6.0) < 1e-12
    ico = winding_ref.icosphere(3)
    assert len(ico) == 1280
    assert abs(brute64(np.concatenate([ico, winding_ref.icosphere(3, 2.0)]), centre)[0] - 2.0) < 1e-9
    assert abs(brute64(ico[:, [0, 2, 1]], centre)[0] + 1.0) < 1e-9
    n, area = winding_ref.area_vector64(winding_ref.open_cube())
    assert np.allclose(n, [0, 0, -4]) and abs(area - 20.0) < 1e-12


def test_header_symbols_sizes_and_argtypes(api):
    text = open(os.path.join(ROOT, "include", "rtk_amd.h")).read()
    for word in ("typedef struct rtk_winding_opts { uint32_t struct_size; uint32_t flags; float beta; } rtk_winding_opts;", "#define RTK_WINDING_EXACT 1u",
                 "int rtk_dev_scene_prepare_winding(const rtk_dev_scene *ds, rtk_dev_winding_info *out /* may be NULL */, void *stream);",
                 "int rtk_dev_scene_winding_moments(const rtk_dev_scene *ds, float *d_out, void *stream);",
                 "int rtk_dev_winding_numbers(const rtk_dev_scene *ds, const rtk_point_query *d_queries, size_t num_queries,",
                 "int rtk_dev_winding_numbers_counted(const rtk_dev_scene *ds, const rtk_point_query *d_queries, size_t num_queries,",
                 "uint32_t rtk_amd_winding_stack_entries(void);", "max_dist2 of an rtk_point_query IS NOT READ", "0x7fc00000",
                 "A SLOT THAT IS NOT\n * LISTED IS NOT WRITTEN", "Works as it is on rtk_mgpu_scene(m, i)", "NOT promised bit for bit across trees"):
        assert word in text, word
    layout = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_layout_check.h")).read()
    assert "sizeof(rtk_dev_winding_info) == 56" in layout and "sizeof(rtk_winding_opts) == 12" in layout
    assert "sizeof(DevWinding) == 128" in open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_dev.h")).read()
    assert C.sizeof(api.WindingInfo) == 56 and C.sizeof(api.WindingOpts) == 12
    assert [k for k, _ in api.WindingInfo._fields_] == ["nodes", "table_bytes", "table_ms", "total_area_vector", "total_area"]
    assert api.WindingInfo.table_ms.offset == 16 and api.WindingInfo.total_area.offset == 48 and api.WindingOpts.beta.offset == 8
    L = api.lib()
    for name in ("rtk_dev_scene_prepare_winding", "rtk_dev_scene_winding_moments", "rtk_dev_winding_numbers", "rtk_dev_winding_numbers_counted"):
        assert name in api.RTK_AMD_H_SYMBOLS and hasattr(L, name) and getattr(L, name).restype == C.c_int, name
    assert L.rtk_amd_winding_stack_entries() >= 1 and "rtk_amd_winding_stack_entries" in api.RTK_AMD_H_SYMBOLS
    assert L.rtk_dev_winding_numbers.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(api.RayList), C.POINTER(api.WindingOpts), C.c_void_p, C.c_void_p]
    for name in ("prepare_winding", "winding_moments", "winding_numbers_device", "winding_numbers_counted", "winding_numbers", "contains_winding"):
        assert callable(getattr(api.DeviceScene, name)), name
    doc = api.DeviceScene.contains_winding.__doc__
    assert "-1" in doc and '"outside"' in doc and "contains_signed" in doc and "holes" in doc
    mem = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_scene_mem.h")).read()
    assert "rtk_scene_winding_table (rtk_winding.hip)" in mem and "num_nodes * 128" in mem


def test_refusals_need_no_device(api):
    L = api.lib()
    dummy = C.cast(C.create_string_buffer(64), C.c_void_p)                   # (what is refused is refused before the scene is looked at)
    count = C.cast(C.create_string_buffer(8), C.c_void_p)

    def ray_list(**kw):
        l = api.RayList()
        l.struct_size, l.flags, l.d_ids, l.d_count = C.sizeof(api.RayList), 0, None, count.value
        for k, v in kw.items():
            setattr(l, k, v)
        return l

    def opts(**kw):
        o = api.make_winding_opts()
        for k, v in kw.items():
            setattr(o, k, v)
        return C.byref(o)
    #            scene  queries n  list  opts  winding stream
    for args in ((None, dummy, 4, None, None, dummy, None), (dummy, None, 4, None, None, dummy, None), (dummy, dummy, 4, None, None, None, None),
                 (dummy, dummy, 4, C.byref(ray_list(struct_size=8)), None, dummy, None), (dummy, dummy, 4, C.byref(ray_list(flags=1)), None, dummy, None),
                 (dummy, dummy, 4, C.byref(ray_list(d_count=None)), None, dummy, None), (dummy, dummy, 1 << 32, None, None, dummy, None),
                 (dummy, dummy, 4, None, opts(struct_size=8), dummy, None), (dummy, dummy, 4, None, opts(struct_size=16), dummy, None),
                 (dummy, dummy, 4, None, opts(beta=-1.0), dummy, None), (dummy, dummy, 4, None, opts(beta=float("nan")), dummy, None),
                 (dummy, dummy, 4, None, opts(flags=2), dummy, None), (dummy, dummy, 0, None, opts(beta=-2.0), dummy, None)):
        assert L.rtk_dev_winding_numbers(*args) == ERR_BAD_ARG, args
        assert "rtk_dev_winding_numbers" in api.last_error()
    # no queries: nothing to do, nothing launched, no table made (the scene is not even looked at)
    assert L.rtk_dev_winding_numbers(dummy, None, 0, None, None, None, None) == 0
    assert L.rtk_dev_winding_numbers(dummy, dummy, 0, C.byref(ray_list()), opts(beta=0.0), dummy, None) == 0
    ctr = api.TraceCounters()
    assert L.rtk_dev_winding_numbers_counted(dummy, dummy, 0, None, dummy, C.byref(ctr)) == 0
    assert L.rtk_dev_winding_numbers_counted(dummy, dummy, 4, None, dummy, None) == ERR_BAD_ARG
    assert L.rtk_dev_winding_numbers_counted(dummy, dummy, 4, None, None, C.byref(ctr)) == ERR_BAD_ARG
    assert L.rtk_dev_scene_prepare_winding(None, None, None) == ERR_BAD_ARG and "rtk_dev_scene_prepare_winding" in api.last_error()
    assert L.rtk_dev_scene_winding_moments(None, dummy, None) == ERR_BAD_ARG and L.rtk_dev_scene_winding_moments(dummy, None, None) == ERR_BAD_ARG
    assert "rtk_dev_scene_winding_moments" in api.last_error()
