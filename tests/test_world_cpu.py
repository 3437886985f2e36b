"""Instanced worlds without a GPU: the rules of rtk_amd/csrc/rtk_world_rule.h, run by tests/world_rule_driver.cpp (built plain and
once more under the address and undefined-behaviour sanitizers), against numpy in the stated order (tests/world_ref.py), bit for
bit: the inverse in float64 rounded once, the ray and the box in float32; and every refusal of the interface that needs no
device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import world_ref
from tests.world_ref import F, box_np, inverse_np, margin_np, placement, ray_np, rotation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_BAD_ARG = -2


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    """The driver built against the rule headers alone (no HIP include path, -Wall -Werror, no FMA contraction as in the
    library): once as it is and once with both sanitizers, the flags of tests/test_winding_cpu.py."""
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if request.param == "sanitized" else []
    exe = str(tmp_path_factory.mktemp("world_rule_" + request.param) / "world_rule_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-mfma", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + extra +
                          ["-I" + os.path.join(ROOT, "rtk_amd", "csrc"), os.path.join(ROOT, "tests", "world_rule_driver.cpp"), "-o", exe])
    return exe


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
    return [[int(x, 16) for x in l.split()] for l in out[:-2]]


def same_bits(got, want):
    """Bit for bit, except where the expected value is NaN: there only "it is NaN" is promised."""
    got = np.ascontiguousarray(got, np.uint32)
    want = np.ascontiguousarray(want, F)
    nan = np.isnan(want)
    assert (np.isnan(got.view(F)) == nan).all()
    bad = (got != want.view(np.uint32)) & ~nan
    assert not bad.any(), (np.argwhere(bad)[:5], got[bad][:5], want.view(np.uint32)[bad][:5])


def placements_under_test():
    """(name, m, live): identity, a rotation with translation, non-uniform scale, a mirror, singular ones, NaN / inf entries,
    denormal entries, and random well-conditioned ones"""
    rng = np.random.RandomState(3)
    R = rotation([1, 2, 3], 0.7)
    zero_row = placement(np.array([[1, 2, 3], [0, 0, 0], [4, 5, 6]]), (1, 2, 3))
    equal_rows = placement(np.array([[1, 2, 3], [1, 2, 3], [4, 5, 7]]), (1, 2, 3))
    nan = placement(R, (1, 2, 3)); nan[5] = np.nan
    inf = placement(R, (1, 2, 3)); inf[0] = np.inf
    inf_t = placement(R, (np.inf, 2, 3))
    den = placement(np.eye(3) * 1e-42, (1e-40, 0, 1e-44))            # denormal entries: the inverse overflows float
    den_t = placement(R, (1e-41, -1e-43, 1e-45))                     # denormal translation only: live
    huge = placement(np.eye(3) * 1e-30, (1, 2, 3))                   # 1e30 fits float: live
    cases = [("identity", placement(), True), ("rotation", placement(R, (10, -20, 30)), True),
             ("scale", placement(np.diag([0.5, 3.0, 10.0]), (1, 2, 3)), True), ("mirror", placement(np.diag([-1.0, 1.0, 1.0]) @ R, (4, 5, 6)), True),
             ("zero row", zero_row, False), ("equal rows", equal_rows, False), ("nan", nan, False), ("inf", inf, False), ("inf translation", inf_t, False),
             ("denormal", den, False), ("denormal translation", den_t, True), ("tiny scale", huge, True), ("zero", np.zeros(12, F), False)]
    for k in range(200):
        A = rotation(rng.standard_normal(3), rng.uniform(0, 6.28)) @ np.diag(rng.uniform(0.1, 10.0, 3)) @ rotation(rng.standard_normal(3), rng.uniform(0, 6.28))
        cases.append(("random %d" % k, placement(A * rng.choice([1e-3, 1.0, 1e3]), rng.uniform(-100, 100, 3)), True))
    return cases


def test_rule_header_includes_no_hip_and_says_what_it_must():
    text = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_world_rule.h")).read()
    assert [l.split()[1] for l in text.splitlines() if l.startswith("#include")] == ["<stdint.h>", '"rtk_place_rule.h"']
    assert "hip/" not in text and "math.h" not in text
    for word in ("THE INVERSE", "THE RAY", "THE BOX", "THE PADDING", "THE MARGIN", "EACH ROUNDED TO FLOAT ONCE", "ARE COPIED", "NOT RENORMALISED",
                 "DEAD", "RTK_WORLD_PAD 0x1p-11f", "fp contract(off)", "No HIP, no libm", "DESIGN.md 3.23"):
        assert word in text, word
    drv = open(os.path.join(ROOT, "tests", "world_rule_driver.cpp")).read()
    assert [l.split()[1] for l in drv.splitlines() if l.startswith("#include") and '"' in l] == ['"rtk_world_rule.h"']
    mk = open(os.path.join(ROOT, "rtk_amd", "csrc", "Makefile")).read()
    assert "rtk_world_rule.h" in mk and "rtk_world.hip" in mk


def test_inverse_matches_numpy_bit_for_bit(driver, tmp_path):
    cases = placements_under_test()
    m = np.array([c[1] for c in cases], F)
    got = run_driver(driver, ["i " + _hex(r) for r in m], tmp_path, "inverse")
    inv, live = inverse_np(m)
    assert [g[0] for g in got] == live.astype(int).tolist()
    assert live.tolist() == [c[2] for c in cases], [c[0] for c, l in zip(cases, live) if c[2] != l]
    same_bits([g[1:] for g, l in zip(got, live) if l], inv[live])
    # the inverse is one: A * inv(A) = 1 within float rounding times the condition number, for the random placements
    for (name, mm, _), iv in zip(cases, inv):
        if name.startswith("random"):
            A, B = mm.reshape(3, 4)[:, :3].astype(np.float64), iv.reshape(3, 4)[:, :3].astype(np.float64)
            assert np.abs(A @ B - np.eye(3)).max() <= 1e-4, name
            assert np.abs(A @ iv.reshape(3, 4)[:, 3] + mm.reshape(3, 4)[:, 3]).max() <= 1e-4 * 100 * 10, name
    assert (inv[0] == placement()).all()                                     # the identity's inverse is the identity, bit for bit


def test_ray_matches_numpy_bit_for_bit(driver, tmp_path):
    rng = np.random.RandomState(4)
    cases = [c for c in placements_under_test() if c[2]]
    inv, _ = inverse_np(np.array([c[1] for c in cases], F))
    rays = np.zeros((len(cases), 8), F)
    rays[:, 0:3] = rng.uniform(-50, 50, (len(cases), 3))
    rays[:, 3:6] = rng.standard_normal((len(cases), 3))
    rays[:, 6], rays[:, 7] = 1e-3, world_ref.RTK_INF
    rays[0, 3:6] = (0, 0, 1)                                                 # an axis-aligned direction
    rays[1, 0:3] = (np.inf, 0, np.nan)                                       # NaN results: only that they are NaN
    got = run_driver(driver, ["r " + _hex(np.concatenate([i, r])) for i, r in zip(inv, rays)], tmp_path, "ray")
    want = np.array([ray_np(i, r[None])[0] for i, r in zip(inv, rays)])
    same_bits(got, want)
    assert (want[:, 6] == rays[:, 6]).all() and (want[:, 7] == rays[:, 7]).all()      # min_t, max_t: copied
    # the direction is not renormalised: under a scale of 3 along an axis it shrinks by 3
    iv, _ = inverse_np(placement(np.diag([3.0, 3.0, 3.0])))
    out = ray_np(iv[0], np.array([[0, 0, 0, 0, 0, 1, 0, 1]], F))
    assert abs(out[0, 5] - 1 / 3) < 1e-7


def test_box_and_margin_match_numpy_bit_for_bit(driver, tmp_path):
    rng = np.random.RandomState(5)
    cases = [c for c in placements_under_test() if c[2]]
    lines, want = [], []
    for k, (name, m, _) in enumerate(cases):
        lo = rng.uniform(-5, 0, 3).astype(F)
        hi = (lo + rng.uniform(0, 7, 3)).astype(F)
        if k == 0:
            lo, hi = np.array([-1, -1, -1], F), np.array([1, 1, 1], F)
        lines.append("b " + _hex(np.concatenate([lo, hi, m])))
        want.append(box_np(lo, hi, m))
    lines.append("b " + _hex(np.concatenate([[-2, -2, -2], [2, 2, 2], placement(np.eye(3) * 3e38, (0, 0, 0))])))          # overflows: not finite
    want.append(box_np([-2, -2, -2], [2, 2, 2], placement(np.eye(3) * 3e38, (0, 0, 0))))
    got = run_driver(driver, lines, tmp_path, "box")
    assert [g[0] for g in got] == [int(w[2]) for w in want] and not want[-1][2]
    same_bits([g[1:] for g in got[:-1]], [np.concatenate([w[0], w[1]]) for w in want[:-1]])
    # the unit cube under the identity: padded by 2^-11 * (1 + 0) on every side; and every box contains its exact corners
    assert (want[0][0] == F(-1) - F(2.0 ** -11)).all() and (want[0][1] == F(1) + F(2.0 ** -11)).all()
    org = rng.uniform(-100, 100, (50, 3)).astype(F)
    org[0] = (np.nan, -3, 2)
    bounds = rng.uniform(0, 500, 50).astype(F)
    got = run_driver(driver, ["g " + _hex(np.concatenate([o, [b]])) for o, b in zip(org, bounds)], tmp_path, "margin")
    same_bits([g[0] for g in got], [margin_np(o, b) for o, b in zip(org, bounds)])
    assert margin_np(org[0], F(10)) == F(2.0 ** -11) * F(13)                 # a NaN coordinate is not the largest


def test_header_symbols_sizes_and_argtypes(api):
    text = open(os.path.join(ROOT, "include", "rtk_amd.h")).read()
    for word in ("typedef struct rtk_dev_world rtk_dev_world;", "rtk_dev_world *rtk_dev_world_create(rtk_dev_scene *const *scenes, size_t num_scenes,",
                 "int rtk_dev_world_update(rtk_dev_world *w, const rtk_placement *placements, void *stream);",
                 "int rtk_dev_world_rebuild(rtk_dev_world *w, void *stream);", "int rtk_dev_world_get_info(const rtk_dev_world *w, rtk_dev_world_info *out);",
                 "void rtk_dev_world_free(rtk_dev_world *w);", "int rtk_dev_world_trace_rays(const rtk_dev_world *w, const rtk_ray *d_rays, size_t n, const rtk_ray_list *list,",
                 "int rtk_dev_world_trace_rays_any(", "int rtk_dev_world_trace_rays_counted(", "uint32_t rtk_amd_world_stack_entries(void);",
                 "FREEING A SCENE THAT A LIVE WORLD NAMES IS THE CALLER'S ERROR", "MUST BE FOLLOWED BY", "rtk_dev_world_update BEFORE THE NEXT TRACE",
                 "THE RECORD IS THAT OF ONE OF THEM", "NOT RENORMALISED"):
        assert word in text, word
    layout = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_layout_check.h")).read()
    assert "sizeof(DevWorldInstance) == 64" in layout and "sizeof(rtk_dev_world_info) == 64" in layout and "sizeof(rtk_world_filter) == 32" in layout
    assert C.sizeof(api.WorldInfo) == 64 and C.sizeof(api.WorldFilter) == 32
    assert api.WorldInfo.top_max_depth.offset == 40 and api.WorldInfo.build_ms.offset == 48 and api.WorldFilter.d_ignore_instance.offset == 24
    L = api.lib()
    for name in ("rtk_dev_world_update", "rtk_dev_world_rebuild", "rtk_dev_world_get_info", "rtk_dev_world_trace_rays", "rtk_dev_world_trace_rays_any",
                 "rtk_dev_world_trace_rays_counted", "rtk_dev_world_trace_status"):
        assert name in api.RTK_AMD_H_SYMBOLS and hasattr(L, name) and getattr(L, name).restype == C.c_int, name
    assert L.rtk_amd_world_stack_entries() == 16 and "rtk_amd_world_stack_entries" in api.RTK_AMD_H_SYMBOLS
    for name in ("create", "update", "rebuild", "info", "free", "trace_device", "trace_any_device", "trace_counted", "trace", "trace_any"):
        assert callable(getattr(api.DeviceWorld, name)), name
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        assert "rtk_dev_world" in open(os.path.join(ROOT, doc)).read(), doc


def test_refusals_need_no_device(api):
    L = api.lib()
    # (a scene is looked at only for its device number, the first word: two zeroed buffers are two scenes on device 0)
    bufs = [C.create_string_buffer(64) for _ in range(3)]
    scenes = (C.c_void_p * 3)(*[C.cast(b, C.c_void_p) for b in bufs])
    which = (C.c_uint32 * 4)(0, 1, 2, 1)
    place = (api.Placement * 4)()

    def create(s=scenes, ns=3, w=which, p=place, n=4):
        return L.rtk_dev_world_create(s, ns, w, p, n)
    for bad in (dict(s=None), dict(w=None), dict(p=None), dict(ns=0), dict(n=0), dict(n=1 << 31), dict(n=1 << 40)):
        assert not create(**bad), bad
        assert "rtk_dev_world_create" in api.last_error()
    assert not create(w=(C.c_uint32 * 4)(0, 1, 3, 1)) and "names scene 3 of 3" in api.last_error()
    assert not create(s=(C.c_void_p * 3)(scenes[0], None, scenes[2])) and "scene 1 is NULL" in api.last_error()
    C.cast(bufs[2], C.POINTER(C.c_int))[0] = 1                               # scenes on different devices
    assert not create() and "a world is on one device" in api.last_error()
    C.cast(bufs[2], C.POINTER(C.c_int))[0] = 0

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
    #            world  rays   n  list  filter records instances stream
    for args in ((None, dummy, 4, None, None, dummy, None, None), (dummy, None, 4, None, None, dummy, None, None), (dummy, dummy, 4, None, None, None, None, None),
                 (dummy, dummy, 4, ray_list(struct_size=8), None, dummy, None, None), (dummy, dummy, 4, ray_list(flags=1), None, dummy, None, None),
                 (dummy, dummy, 4, ray_list(d_count=None), None, dummy, None, None), (dummy, dummy, 1 << 32, None, None, dummy, None, None),
                 (dummy, dummy, 1 << 32, ray_list(), None, dummy, None, None),
                 (dummy, dummy, 4, None, filt(struct_size=16), dummy, None, None), (dummy, dummy, 4, None, filt(flags=1), dummy, None, None),
                 (dummy, dummy, 4, None, filt(d_instance_mask=dummy.value, instance_mask_bits=0), dummy, None, None)):
        assert L.rtk_dev_world_trace_rays(*args) == ERR_BAD_ARG, args
        assert "rtk_dev_world_trace_rays" in api.last_error()
        any_args = args[:5] + (args[5], args[7])
        assert L.rtk_dev_world_trace_rays_any(*any_args) == ERR_BAD_ARG, any_args
        assert "rtk_dev_world_trace_rays_any" in api.last_error()
    # no rays: nothing to do, nothing launched (the world is not even looked at)
    assert L.rtk_dev_world_trace_rays(dummy, None, 0, None, None, None, None, None) == 0
    assert L.rtk_dev_world_trace_rays_any(dummy, None, 0, ray_list(), filt(), None, None) == 0
    ctr = api.TraceCounters()
    assert L.rtk_dev_world_trace_rays_counted(dummy, dummy, 0, None, dummy, None, C.byref(ctr)) == 0
    assert L.rtk_dev_world_trace_rays_counted(dummy, dummy, 4, None, dummy, None, None) == ERR_BAD_ARG
    assert L.rtk_dev_world_trace_rays_counted(None, dummy, 4, None, dummy, None, C.byref(ctr)) == ERR_BAD_ARG
    for fn, args in ((L.rtk_dev_world_update, (None, None, None)), (L.rtk_dev_world_rebuild, (None, None)), (L.rtk_dev_world_get_info, (None, None)),
                     (L.rtk_dev_world_get_info, (dummy, None)), (L.rtk_dev_world_trace_status, (None, None))):
        assert fn(*args) == ERR_BAD_ARG
        assert "rtk_dev_world" in api.last_error()
    assert L.rtk_dev_world_top_scene(None) is None
    L.rtk_dev_world_free(None)
