"""Signed distances without a GPU: the rule of rtk_amd/csrc/rtk_sign_rule.h, run by tests/sign_rule_driver.cpp under the address
and undefined-behaviour sanitizers, against numpy float32 arithmetic in the stated order (tests/sign_ref.py), bit for bit -- the
table of pseudonormals, the counts and the sign; the arctangent against float64; the sign against an analytic inside test where
the face normal alone fails; and the parts of the interface that need no device."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from tests import sign_ref
from tests.sign_ref import CLASSES, F, RTK_INF, angle_np, class_queries, cpu_meshes, l_prism, plus_shape, signed_np, table_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_BAD_ARG = -2
ANGLE_ERROR_MEASURED = 1.82e-06         # rad: what the header's comment states; twice this is asserted


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """The driver built against the header alone (no HIP include path, -Wall -Werror, no FMA contraction as in the library)
    with both sanitizers: the flags of tests/test_closest_cpu.py."""
    exe = str(tmp_path_factory.mktemp("sign_rule") / "sign_rule_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-mfma", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "rtk_amd", "csrc"), os.path.join(ROOT, "tests", "sign_rule_driver.cpp"), "-o", exe])
    return exe


def _hex(rows):
    return "".join(" ".join("%x" % w for w in row) + "\n" for row in np.ascontiguousarray(rows, F).view(np.uint32).tolist())


def run_mesh(exe, tris, queries, tmp_path, name="mesh"):
    """tris [T, 3, 3], queries [Q, 4] (point, max_dist2) -> (table words [T, 18], info dict, per query [signed, dist2, prim, region])"""
    path = str(tmp_path / (name.replace(" ", "_").replace(",", "") + ".txt"))
    with open(path, "w") as f:
        f.write("m %d\n" % len(tris) + _hex(tris.reshape(-1, 9)))
        f.write("".join("q " + l + "\n" for l in _hex(queries).splitlines()))
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    T, Q = len(tris), len(queries)
    assert lines[T + 1 + Q] == "ok"
    table = np.array([[int(w, 16) for w in l.split()] for l in lines[:T]], np.uint32).reshape(T, 18)
    info = dict(zip(("boundary_sides", "nonmanifold_sides", "inconsistent_sides", "degenerate_triangles", "places"), map(int, lines[T].split()[1:])))
    ans = np.array([[int(w, 16) if k < 3 else int(w) for k, w in enumerate(l.split())] for l in lines[T + 1:T + 1 + Q]], np.int64).reshape(Q, 4)
    return table, info, ans


def same_bits(got, want):
    """Bit for bit, except where the expected value is NaN: there only "it is NaN" is promised."""
    got = np.ascontiguousarray(got, np.uint32)
    want = np.ascontiguousarray(want, F)
    nan = np.isnan(want)
    assert (np.isnan(got.view(F)) == nan).all()
    bad = (got != want.view(np.uint32)) & ~nan
    assert not bad.any(), (np.argwhere(bad)[:5], got[bad][:5], want.view(np.uint32)[bad][:5])


def queries_round(tris, n, seed):
    """points in and round the mesh's box, and a few that cannot be answered"""
    rng = np.random.RandomState(seed)
    fin = tris[np.isfinite(tris).all((1, 2))].reshape(-1, 3)
    lo, hi = fin.min(0), fin.max(0)
    q = np.zeros((n, 4), F)
    q[:, :3] = rng.uniform(lo - 0.5 * (hi - lo) - 0.1, hi + 0.5 * (hi - lo) + 0.1, (n, 3))
    q[: n // 4, :3] = fin[rng.randint(len(fin), size=n // 4)] + rng.standard_normal((n // 4, 3)) * 0.05      # near the vertices
    q[:, 3] = RTK_INF
    q[-1, 3] = 1e-6; q[-2, 3] = 0.0; q[-3, 0] = np.nan; q[-4, 3] = np.nan; q[-5, 1] = np.inf
    return q


def test_rule_header_includes_no_hip_and_says_what_it_must():
    text = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_sign_rule.h")).read()
    assert [l.split()[1] for l in text.splitlines() if l.startswith("#include")] == ["<stdint.h>", '"rtk_closest_rule.h"']
    assert "hip/" not in text and "math.h" not in text
    for word in ("__fmul_rn", "-ffp-contract=off", "fp contract(off)", "enormal", "NaN", "-0 equals +0", "SAME PLACE", "HAS NO NORMAL",
                 "STARTING FROM THE FIRST TERM", "ascending prim order", "No libm", "NOT normalised", "INSIDE iff s < 0", "WHAT IS PROMISED",
                 "closed, consistently wound, non-self-intersecting", "open or inconsistently wound", "region picks N",
                 "%.2e rad" % ANGLE_ERROR_MEASURED, "__builtin_sqrtf"):
        assert word in text, word
    drv = open(os.path.join(ROOT, "tests", "sign_rule_driver.cpp")).read()
    assert [l.split()[1] for l in drv.splitlines() if l.startswith("#include") and '"' in l] == ['"rtk_sign_rule.h"']
    mk = open(os.path.join(ROOT, "rtk_amd", "csrc", "Makefile")).read()
    assert "rtk_sign_rule.h" in mk and "rtk_sign.hip" in mk and "-fhip-fp32-correctly-rounded-divide-sqrt" in mk


def test_tables_counts_and_signs_match_numpy_bit_for_bit(driver, tmp_path):
    """Every mesh of the list: the table, the five counts, and signed / dist2 / prim / region of queries round it."""
    infos = {}
    for k, (name, tris) in enumerate(cpu_meshes().items()):
        want_table, want_info = table_np(tris)
        q = queries_round(tris, 300, 100 + k)
        table, info, ans = run_mesh(driver, tris, q, tmp_path, name)
        same_bits(table, want_table)
        assert info == want_info, (name, info, want_info)
        signed, rec, _, region, _ = signed_np(tris, want_table, q[:, :3], q[:, 3])
        same_bits(ans[:, 0], signed)
        same_bits(ans[:, 1], rec[:, 0].view(F))
        assert (ans[:, 2] == rec[:, 3]).all() and (ans[:, 3] == region).all(), name
        miss = rec[:, 3] == sign_ref.NONE
        assert miss[-5:].all() and (signed[miss].view(np.uint32) == RTK_INF.view(np.uint32)).all() and (ans[miss, 3] == 0).all()
        infos[name] = info
    # the counts stated outright
    for name in ("tetrahedron", "cube", "L prism", "L, vertices duplicated per face", "L as two meshes"):
        i = infos[name]
        assert (i["boundary_sides"], i["nonmanifold_sides"], i["inconsistent_sides"], i["degenerate_triangles"]) == (0, 0, 0, 0), (name, i)
    assert infos["cube"]["places"] == 8 and infos["L prism"]["places"] == 16 and infos["tetrahedron"]["places"] == 4
    assert infos["single triangle"]["boundary_sides"] == 3
    assert infos["cube without a face"]["boundary_sides"] == 4 and infos["cube without a face"]["nonmanifold_sides"] == 0
    assert infos["three triangles on one edge"]["nonmanifold_sides"] == 3
    assert infos["cube, one triangle turned"]["inconsistent_sides"] == 6 and infos["cube, one triangle turned"]["boundary_sides"] == 0
    assert infos["defects"]["degenerate_triangles"] == 3
    assert infos["fan of 200"]["places"] == 201 and infos["fan of 200"]["boundary_sides"] == 200
    # welding is by place: the -0.0 vertex and the +0.0 vertex of the defect mesh are one place (their rows are equal), the NaN
    # corner is alone, and the degenerate records still carry their neighbours' sums
    tris = cpu_meshes()["defects"]
    table, _ = table_np(tris)
    assert (table[14, 9:12].view(np.uint32) == table[15, 9:12].view(np.uint32)).all() and np.signbit(tris[15, 0, 0]) and not np.signbit(tris[14, 0, 0])
    assert (table[12, 9:12] == table[12, 12:15]).all() and np.abs(table[12, 9:12]).sum() > 0                 # a = b of the zero-area record: the cube's corner
    assert (table[16, 12:15] == 0).all()                                                                      # the NaN corner: nothing to sum


def test_angle_against_float64(driver, tmp_path):
    """|rtk_sign_angle - math.atan2| over ratios 2^-20 .. 2^20 in steps of 2^(1/8), four magnitudes of x, all sign combinations,
    and the exact zeros; the driver equals numpy bit for bit. Measured, stated in the header, asserted at twice that."""
    ratio = 2.0 ** (np.arange(-160, 161) / 8.0)
    ys, xs = [], []
    for x0 in (1.0, 3.0, 2.0 ** -10, 1.7 * 2.0 ** 10):
        for sy in (1.0, -1.0):
            for sx in (1.0, -1.0):
                ys.append(sy * ratio * x0); xs.append(np.full(len(ratio), sx * x0))
    zeros = [(0.0, 1.0), (0.0, -1.0), (1.0, 0.0), (-1.0, 0.0), (0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0), (2.5, 0.0), (0.0, 7.0)]
    y = np.concatenate(ys + [np.array([z[0] for z in zeros])]).astype(F)
    x = np.concatenate(xs + [np.array([z[1] for z in zeros])]).astype(F)
    want = angle_np(y, x)
    path = str(tmp_path / "angles.txt")
    with open(path, "w") as f:
        f.write("".join("a %x %x\n" % (a, b) for a, b in zip(y.view(np.uint32).tolist(), x.view(np.uint32).tolist())))
    r = subprocess.run([driver, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    got = np.array([int(l, 16) for l in r.stdout.split()[:len(y)]], np.uint32)
    assert (got == want.view(np.uint32)).all()
    exact = np.array([math.atan2(float(a), float(b)) for a, b in zip(y, x)])
    err = np.abs(want.astype(np.float64) - exact)
    err[(y == 0) & (x == 0)] = 0.0                                           # ((0, 0) is 0 by the rule whatever the zeros' signs; atan2 says +-pi for some)
    print("rtk_sign_angle: worst absolute error %.3e rad over %d pairs" % (err.max(), len(y)))
    assert err.max() <= 2 * ANGLE_ERROR_MEASURED and 2 * ANGLE_ERROR_MEASURED <= 1e-5
    assert err.max() >= 0.5 * ANGLE_ERROR_MEASURED                          # (the stated figure is this grid's, not a guess)
    # the exact cases, as bits
    bits = lambda a, b: int(angle_np(F(a), F(b)).view(np.uint32))
    assert bits(0.0, 1.0) == 0 and bits(0.0, 7.0) == 0 and bits(0.0, 0.0) == 0 and bits(-0.0, -0.0) == 0
    assert bits(1.0, 0.0) == 0x3FC90FDB and bits(2.5, 0.0) == 0x3FC90FDB and bits(0.0, -1.0) == 0x40490FDB


@pytest.fixture(scope="module")
def class_cases():
    """name -> (shape, tris, table, points, class, region): 2000 queries per class round the L and the plus, both turned out of
    the axes (sign_ref.Boxes says why)"""
    out = {}
    for name, shape, seed in (("L", l_prism(sign_ref.TILT), 11), ("plus", plus_shape(sign_ref.TILT), 12)):
        tris = shape.triangles()
        table, info = table_np(tris)
        assert (info["boundary_sides"], info["nonmanifold_sides"], info["inconsistent_sides"], info["degenerate_triangles"]) == (0, 0, 0, 0)
        pts, cls, reg = class_queries(shape, 2000, seed)
        out[name] = (shape, tris, table, pts, cls, reg)
    return out


def test_sign_is_right_where_the_face_normal_is_not(driver, class_cases, tmp_path):
    """2000 queries per class (face, convex edge, concave edge, convex vertex, saddle or concave vertex) round the L prism and the
    plus of three boxes, none nearer than 1e-3 of the shape's size in float64 and none left out afterwards: the driver's sign is
    the analytic inside test's for every one. The inputs are worth it: at least a fifth end in a region other than 7, both
    sides are met, and the face normal alone gets some of them wrong."""
    for name, (shape, tris, table, pts, cls, _) in class_cases.items():
        assert len(pts) == 2000 * len(CLASSES)
        assert (sign_ref.distance64(tris, pts) >= 1e-3 * shape.size).all()
        inside = shape.inside(pts)
        signed, rec, _, region, shortcut = signed_np(tris, table, pts, np.full(len(pts), RTK_INF, F))
        q = np.concatenate([pts, np.full((len(pts), 1), RTK_INF, F)], 1)
        _, _, ans = run_mesh(driver, tris, q, tmp_path, "classes " + name)
        same_bits(ans[:, 0], signed)
        got_inside = ans[:, 0].astype(np.uint32).view(F) < 0
        wrong = np.nonzero(got_inside != inside)[0]
        assert len(wrong) == 0, (name, len(wrong), pts[wrong[:5]], region[wrong[:5]])
        print(name, "regions", np.bincount(region, minlength=8)[1:], "inside", int(inside.sum()), "of", len(pts),
              "face-normal shortcut wrong", int((shortcut != inside).sum()),
              "per class inside", [int(inside[cls == c].sum()) for c in range(len(CLASSES))])
        assert (region != 7).mean() >= 0.2
        assert inside.mean() >= 0.1 and (~inside).mean() >= 0.1
        assert (shortcut != inside).sum() >= 1
        assert inside[cls == CLASSES.index("concave edge")].all() and not inside[cls == CLASSES.index("convex edge")].any()


def test_header_symbols_sizes_and_argtypes(api):
    text = open(os.path.join(ROOT, "include", "rtk_amd.h")).read()
    for word in ("typedef struct rtk_dev_sign_info {", "int rtk_dev_scene_prepare_signs(const rtk_dev_scene *ds, rtk_dev_sign_info *out /* may be NULL */, void *stream);",
                 "int rtk_dev_scene_pseudonormals(const rtk_dev_scene *ds, float *d_out, void *stream);",
                 "int rtk_dev_signed_distances(const rtk_dev_scene *ds, const rtk_point_query *d_queries, size_t num_queries, const rtk_ray_list *list,",
                 "closed = boundary_sides == 0 && nonmanifold_sides == 0 && inconsistent_sides == 0", "WELDED BY PLACE", "A SLOT THAT IS\n * NOT LISTED IS NOT WRITTEN",
                 "Works as it is on rtk_mgpu_scene(m, i)", "RTK_AMD_ERR_UNSUPPORTED for a scene that does not hold exactly"):
        assert word in text, word
    assert "sizeof(rtk_dev_sign_info) == 56" in open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_layout_check.h")).read()
    assert C.sizeof(api.SignInfo) == 56
    assert [k for k, _ in api.SignInfo._fields_] == ["boundary_sides", "nonmanifold_sides", "inconsistent_sides", "degenerate_triangles", "places", "table_bytes", "table_ms"]
    assert api.SignInfo.table_ms.offset == 48 and isinstance(api.SignInfo().as_dict()["table_ms"], float)
    L = api.lib()
    for name in ("rtk_dev_scene_prepare_signs", "rtk_dev_scene_pseudonormals", "rtk_dev_signed_distances"):
        assert name in api.RTK_AMD_H_SYMBOLS and hasattr(L, name) and getattr(L, name).restype == C.c_int, name
    assert L.rtk_dev_scene_prepare_signs.argtypes == [C.c_void_p, C.POINTER(api.SignInfo), C.c_void_p]
    assert L.rtk_dev_scene_pseudonormals.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p]
    assert L.rtk_dev_signed_distances.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(api.RayList), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    for name in ("prepare_signs", "pseudonormals", "signed_distances_device", "signed_distances", "contains_signed"):
        assert callable(getattr(api.DeviceScene, name)), name
    mem = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_scene_mem.h")).read()
    assert "rtk_scene_pseudonormals (rtk_sign.hip)" in mem and "num_prims * 72" in mem


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
    #            scene  queries n  list  records points signed stream
    for args in ((None, dummy, 4, None, dummy, None, dummy, None), (dummy, None, 4, None, dummy, None, dummy, None),
                 (dummy, dummy, 4, None, dummy, None, None, None), (dummy, dummy, 4, None, None, None, None, None),
                 (dummy, dummy, 4, C.byref(ray_list(struct_size=8)), dummy, None, dummy, None), (dummy, dummy, 4, C.byref(ray_list(flags=1)), dummy, None, dummy, None),
                 (dummy, dummy, 4, C.byref(ray_list(d_count=None)), dummy, None, dummy, None),
                 (dummy, dummy, 1 << 32, None, dummy, None, dummy, None), (dummy, dummy, 1 << 32, C.byref(ray_list()), None, None, dummy, None)):
        assert L.rtk_dev_signed_distances(*args) == ERR_BAD_ARG, args
        assert "rtk_dev_signed_distances" in api.last_error()
    # no queries: nothing to do, nothing launched, no table made (the scene is not even looked at)
    assert L.rtk_dev_signed_distances(dummy, None, 0, None, None, None, None, None) == 0
    assert L.rtk_dev_signed_distances(dummy, dummy, 0, C.byref(ray_list()), dummy, dummy, dummy, None) == 0
    assert L.rtk_dev_scene_prepare_signs(None, None, None) == ERR_BAD_ARG and "rtk_dev_scene_prepare_signs" in api.last_error()
    assert L.rtk_dev_scene_pseudonormals(None, dummy, None) == ERR_BAD_ARG and L.rtk_dev_scene_pseudonormals(dummy, None, None) == ERR_BAD_ARG
    assert "rtk_dev_scene_pseudonormals" in api.last_error()
