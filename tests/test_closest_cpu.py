"""Closest points without a GPU: the rule of rtk_amd/csrc/rtk_closest_rule.h, run by tests/closest_rule_driver.cpp under the
address and undefined-behaviour sanitizers, against numpy float32 arithmetic in the stated order (tests/closest_ref.py), bit for
bit; the bound of a box against the distance of every triangle inside it; the accuracy statement against float64; and the parts
of the interface that need no device -- header text, symbols, struct sizes, argtypes, the refusals decided before any HIP call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.closest_ref import better_np, box_np, tri_box, tri_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_BAD_ARG = -2
SCALE_PAIRS = [(1.0, 1.0), (1e-3, 1.0), (1.0, 1e-3), (100.0, 1.0), (1e-3, 1e-3)]      # (triangle scale, point offset scale)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """The driver built against the header alone (no HIP include path, -Wall -Werror, no FMA contraction as in the library)
    with both sanitizers. -O2 and -mfma: a compiler that were allowed to contract would do it here."""
    exe = str(tmp_path_factory.mktemp("closest_rule") / "closest_rule_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-mfma", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "rtk_amd", "csrc"), os.path.join(ROOT, "tests", "closest_rule_driver.cpp"), "-o", exe])
    return exe


def run_driver(exe, kind, words, tmp_path):
    """words uint32 [n, k] -> the driver's output lines as integers [n, m] (hexadecimal words; the region and flags decimal)"""
    path = str(tmp_path / ("cases_%s.txt" % kind))
    with open(path, "w") as f:
        f.write("".join("%s %s\n" % (kind, " ".join("%x" % w for w in row)) for row in words.tolist()))
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    assert lines[len(words)] == "ok"
    hexes = 6 if kind == "t" else 1 if kind == "b" else 0
    return np.array([[int(w, 16) if k < hexes else int(w) for k, w in enumerate(line.split())] for line in lines[:len(words)]], np.int64)


def same_bits(got, want):
    """Bit for bit, except where the expected value is NaN: there only "it is NaN" is promised."""
    got = np.ascontiguousarray(got, np.uint32)
    want = np.ascontiguousarray(want, np.float32)
    nan = np.isnan(want)
    assert (np.isnan(got.view(np.float32)) == nan).all()
    bad = (got != want.view(np.uint32)) & ~nan
    assert not bad.any(), (np.argwhere(bad)[:5], got[bad][:5], want.view(np.uint32)[bad][:5])


def random_family(rng, n, tri_scale, off_scale):
    """Triangles of the given size about the origin; points at the given distance from a point of the triangle's plane that lies
    inside the triangle or a little outside (so that every region is met)"""
    t = (rng.standard_normal((n, 3, 3)) * tri_scale).astype(np.float32)
    w = rng.uniform(-0.6, 1.6, (n, 2))
    on = t[:, 0] + (t[:, 1] - t[:, 0]) * w[:, :1] + (t[:, 2] - t[:, 0]) * w[:, 1:]
    p = (on + rng.standard_normal((n, 3)) * off_scale).astype(np.float32)
    return p, t


def special_families(rng):
    """name -> (p [n, 3], tris [n, 3, 3]) float32"""
    fam = {}
    n = 3000
    # near-collinear slivers: c almost on the line ab
    p, t = random_family(rng, n, 1.0, 0.3)
    s = rng.uniform(-0.5, 1.5, (n, 1))
    t[:, 2] = (t[:, 0] + (t[:, 1] - t[:, 0]) * s + rng.standard_normal((n, 3)) * 10.0 ** rng.uniform(-8, -3, (n, 1))).astype(np.float32)
    fam["slivers"] = (p, t)
    for name, (i, j) in (("a=b", (1, 0)), ("a=c", (2, 0)), ("b=c", (2, 1))):
        p, t = random_family(rng, 500, 1.0, 1.0)
        t[:, i] = t[:, j]
        fam[name] = (p, t)
    p, t = random_family(rng, 500, 1.0, 1.0)
    t[:, 1] = t[:, 0]; t[:, 2] = t[:, 0]
    fam["a=b=c"] = (p, t)
    p, t = random_family(rng, 900, 1.0, 1.0)
    p[:] = t[np.arange(900), np.arange(900) % 3]
    fam["point at a vertex"] = (p, t)
    p, t = random_family(rng, 900, 1.0, 1.0)
    k, s = np.arange(900) % 3, rng.uniform(0, 1, (900, 1)).astype(np.float32)
    p[:] = t[np.arange(900), k] + (t[np.arange(900), (k + 1) % 3] - t[np.arange(900), k]) * s
    fam["point on an edge"] = (p, t)
    fam["point in the plane"] = random_family(rng, 2000, 1.0, 0.0)
    p, t = random_family(rng, 2000, 1.0, 1.0)
    fam["denormal coordinates"] = ((p * np.float32(1e-38)).astype(np.float32) * np.float32(1e-2), (t * np.float32(1e-38)).astype(np.float32) * np.float32(1e-2))
    p, t = random_family(rng, 1000, 1.0, 1.0)
    fam["denormal triangle, normal point"] = (p, (t * np.float32(1e-38)).astype(np.float32) * np.float32(1e-3))
    return fam


@pytest.fixture(scope="module")
def cases():
    """Every family once: name -> (p, tris), and the numpy answers to them"""
    rng = np.random.RandomState(20250117)
    fam = {"random %g %g" % sp: random_family(rng, 10000, *sp) for sp in SCALE_PAIRS}
    fam.update(special_families(rng))
    p, t = random_family(rng, 600, 1.0, 1.0)
    bad = np.array([np.nan, np.inf, -np.inf], np.float32)
    p[np.arange(600), np.arange(600) % 3] = bad[(np.arange(600) // 3) % 3]
    fam["non-finite point"] = (p, t)
    return {name: (p, t, tri_np(p, t[:, 0], t[:, 1], t[:, 2])) for name, (p, t) in fam.items()}


def test_rule_header_includes_no_hip_and_says_what_it_must():
    text = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_closest_rule.h")).read()
    assert [l.split()[1] for l in text.splitlines() if l.startswith("#include")] == ["<stdint.h>"]
    for word in ("__fmul_rn", "__fadd_rn", "__fsub_rn", "__fdiv_rn", "-ffp-contract=off", "fp contract(off)", "enormal", "NaN", "bound <= dist2"):
        assert word in text, word
    mk = open(os.path.join(ROOT, "rtk_amd", "csrc", "Makefile")).read()
    assert "rtk_closest_rule.h" in mk and "rtk_closest.hip" in mk and "-fhip-fp32-correctly-rounded-divide-sqrt" in mk


def test_driver_matches_numpy_bit_for_bit(driver, cases, tmp_path):
    """dist2, u, v, q and the region of every family, and every one of the seven regions is met"""
    seen = set()
    for name, (p, t, (dist2, u, v, q, region)) in cases.items():
        words = np.concatenate([p, t.reshape(-1, 9)], 1).astype(np.float32).view(np.uint32)
        got = run_driver(driver, "t", words, tmp_path)
        assert (got[:, 6] == region).all(), name
        same_bits(got[:, 0], dist2); same_bits(got[:, 1], u); same_bits(got[:, 2], v); same_bits(got[:, 3:6], q)
        if name.startswith("random"):
            seen |= set(np.unique(region).tolist())
            assert not np.isnan(dist2).any(), name
    assert seen == {1, 2, 3, 4, 5, 6, 7}
    # what the special families are there for
    assert (cases["a=b=c"][2][4] == 1).all() and not np.isnan(cases["a=b=c"][2][0]).any()
    p, t, (dist2, _, _, _, _) = cases["point at a vertex"]                  # (b and c are a + ab * 1 and a + ac * 1, rounded: 0 or tiny)
    assert (dist2[::3] == 0).all() and (np.sqrt(dist2) <= 16 * 2.0 ** -23 * np.abs(t).reshape(-1, 9).max(1)).all()
    assert (cases["denormal coordinates"][2][0] >= 0).all()
    # ... and the regions they exist to probe: a point made on an edge lands in an edge case or, by the rounding of its own
    # construction, a hair inside the face or at an end of the edge -- all three edge cases are met, and most points are theirs;
    # a point of the plane that lies inside the triangle is the face's; slivers meet every edge case and the face
    region = cases["point on an edge"][2][4]
    print("point on an edge: cases", np.bincount(region, minlength=8)[1:])
    assert {3, 5, 6} <= set(np.unique(region).tolist()) and np.isin(region, [3, 5, 6]).mean() > 0.5
    region = cases["point in the plane"][2][4]
    print("point in the plane: cases", np.bincount(region, minlength=8)[1:])
    assert set(np.unique(region).tolist()) == {1, 2, 3, 4, 5, 6, 7} and (region == 7).mean() > 0.1
    assert {3, 5, 6, 7} <= set(np.unique(cases["slivers"][2][4]).tolist())
    # (two equal vertices: an edge case can divide 0 by 0; such a triangle answers NaN and is never the nearest -- the rule as it is)
    assert np.isnan(cases["a=b"][2][0]).any()
    p, _, (dist2, _, _, _, _) = cases["non-finite point"]
    assert np.isnan(dist2[np.isnan(p).any(1)]).all()                         # a NaN in p: a NaN dist2
    assert (np.isnan(dist2) | np.isinf(dist2)).all()                         # an infinity in p: NaN or +inf, never a finite distance
    # the order matters: the same dot products summed the other way round differ somewhere (so the comparison can fail)
    p, t, (dist2, _, _, _, _) = cases["random 1 1"]
    d = p - tri_np(p, t[:, 0], t[:, 1], t[:, 2])[3]
    assert (((d[:, 2] * d[:, 2] + d[:, 1] * d[:, 1]) + d[:, 0] * d[:, 0]) != dist2).any()


def test_bound_never_exceeds_the_distance(driver, cases, tmp_path):
    """The triangle's own box and random enlargements of it: bound <= dist2 wherever dist2 is not a NaN. None may fail."""
    rng = np.random.RandomState(7)
    total = 0
    for name, (p, t, (dist2, _, _, _, _)) in cases.items():
        lo, hi = tri_box(t[:, 0], t[:, 1], t[:, 2])
        ext = np.maximum((hi - lo).max(1, keepdims=True), np.float32(1e-45))
        for grow in (0.0, 1e-6, 1e-2, 1.0, 30.0):
            with np.errstate(all="ignore"):
                blo = (lo - (rng.uniform(0, 1, lo.shape) * grow).astype(np.float32) * ext).astype(np.float32)
                bhi = (hi + (rng.uniform(0, 1, hi.shape) * grow).astype(np.float32) * ext).astype(np.float32)
            assert (blo <= lo).all() and (bhi >= hi).all()
            want = box_np(p, blo, bhi)
            got = run_driver(driver, "b", np.concatenate([p, blo, bhi], 1).view(np.uint32), tmp_path)
            same_bits(got[:, 0], want)
            ok = ~np.isnan(dist2)
            with np.errstate(invalid="ignore"):
                assert (want[ok] <= dist2[ok]).all(), (name, grow, int((~(want[ok] <= dist2[ok])).sum()))
            total += int(ok.sum())
    assert total > 300000


def test_better_than_and_skip(driver, tmp_path):
    f = np.array([0.0, -0.0, 1.0, np.nextafter(np.float32(1), np.float32(2)), 1e-45, np.inf, np.nan, 3.402823e38], np.float32)
    prims = np.array([0, 1, 7, 0xFFFFFFFE, 0xFFFFFFFF], np.uint32)
    d, pr, b, bp = (x.reshape(-1) for x in np.meshgrid(f, prims, f, prims, indexing="ij"))
    words = np.stack([d.view(np.uint32), pr, b.view(np.uint32), bp], 1)
    got = run_driver(driver, "c", words, tmp_path)[:, 0]
    assert (got == better_np(d, pr, b, bp)).all()
    assert not got[np.isnan(d)].any()                                        # a NaN never beats anything
    x, y = (v.reshape(-1) for v in np.meshgrid(f, f, indexing="ij"))
    got = run_driver(driver, "s", np.stack([x.view(np.uint32), y.view(np.uint32)], 1), tmp_path)[:, 0]
    with np.errstate(invalid="ignore"):
        assert (got == (x > y)).all()
    assert not got[np.isnan(x)].any() and not got[x == y].any()              # a NaN bound descends, an equal bound too


def test_accuracy_against_float64(cases):
    """|sqrt(dist2) - exact| <= 16 * 2^-23 * the largest coordinate magnitude involved, on the random families (the header's
    statement: measured 6.3 * 2^-23 over 8 million pairs; slivers and degenerate triangles are not part of it)."""
    worst = 0.0
    for sp in SCALE_PAIRS:
        p, t, (dist2, _, _, _, _) = cases["random %g %g" % sp]
        exact = np.sqrt(tri_np(p, t[:, 0], t[:, 1], t[:, 2], dtype=np.float64)[0])
        mag = np.maximum(np.abs(p).max(1), np.abs(t).reshape(-1, 9).max(1)).astype(np.float64)
        err = np.abs(np.sqrt(dist2.astype(np.float64)) - exact) / mag
        print("scale pair %s: worst error %.2f * 2^-23 of the largest coordinate" % (sp, err.max() * 2.0 ** 23))
        worst = max(worst, err.max())
    assert worst <= 16 * 2.0 ** -23


def test_header_symbols_sizes_and_argtypes(api):
    from rtk_amd import types
    text = open(os.path.join(ROOT, "include", "rtk_amd.h")).read()
    for word in ("typedef struct rtk_point_query { float x, y, z, max_dist2; } rtk_point_query;",
                 "typedef struct rtk_closest_record { float dist2, u, v; uint32_t prim; } rtk_closest_record;",
                 "int rtk_dev_closest_points(const rtk_dev_scene *ds, const rtk_point_query *d_queries, size_t num_queries,",
                 "uint32_t rtk_amd_closest_stack_entries(void);", "NOTHING ELSE IS PROMISED", "LOWEST PRIMITIVE ID"):
        assert word in text, word
    check = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_layout_check.h")).read()
    assert "sizeof(rtk_point_query) == 16" in check and "sizeof(rtk_closest_record) == 16" in check
    assert types.POINT_QUERY_DTYPE.itemsize == 16 and types.CLOSEST_RECORD_DTYPE.itemsize == 16
    assert types.CLOSEST_RECORD_DTYPE.names == ("dist2", "u", "v", "prim") and types.POINT_QUERY_DTYPE.fields["max_dist2"][1] == 12
    L = api.lib()
    assert "rtk_dev_closest_points" in api.RTK_AMD_H_SYMBOLS and "rtk_amd_closest_stack_entries" in api.RTK_AMD_H_SYMBOLS
    assert "rtk_dev_closest_points_counted" in api.RTK_AMD_H_SYMBOLS and "int rtk_dev_closest_points_counted(" in text
    assert L.rtk_dev_closest_points_counted.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(api.TraceCounters)]
    assert L.rtk_dev_closest_points.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(api.RayList), C.c_void_p, C.c_void_p, C.c_void_p]
    assert L.rtk_dev_closest_points.restype == C.c_int
    assert L.rtk_amd_closest_stack_entries.restype == C.c_uint32 and 1 <= L.rtk_amd_closest_stack_entries() <= 64
    assert callable(api.DeviceScene.closest_points) and callable(api.DeviceScene.closest_points_device)


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
    for args in ((None, dummy, 4, None, dummy, None, None), (dummy, None, 4, None, dummy, None, None), (dummy, dummy, 4, None, None, None, None),
                 (dummy, dummy, 4, C.byref(ray_list(struct_size=8)), dummy, None, None), (dummy, dummy, 4, C.byref(ray_list(flags=1)), dummy, None, None),
                 (dummy, dummy, 4, C.byref(ray_list(d_count=None)), dummy, None, None),
                 (dummy, dummy, 1 << 32, None, dummy, None, None), (dummy, dummy, 1 << 32, C.byref(ray_list()), dummy, None, None)):
        assert L.rtk_dev_closest_points(*args) == ERR_BAD_ARG, args
        assert "rtk_dev_closest_points" in api.last_error()
    ctr = api.TraceCounters()
    for args in ((dummy, dummy, 4, dummy, None, None), (None, dummy, 4, dummy, None, C.byref(ctr)), (dummy, None, 4, dummy, None, C.byref(ctr)),
                 (dummy, dummy, 4, None, None, C.byref(ctr)), (dummy, dummy, 1 << 32, dummy, None, C.byref(ctr))):
        assert L.rtk_dev_closest_points_counted(*args) == ERR_BAD_ARG, args
        assert "rtk_dev_closest_points" in api.last_error()
    assert L.rtk_dev_closest_points_counted(dummy, None, 0, None, None, C.byref(ctr)) == 0 and ctr.rays == 0
    # no queries: nothing to do, nothing launched
    assert L.rtk_dev_closest_points(dummy, None, 0, None, None, None, None) == 0
    assert L.rtk_dev_closest_points(dummy, dummy, 0, C.byref(ray_list()), dummy, dummy, None) == 0
