"""Placed meshes without a GPU: the rule of rtk_amd/csrc/rtk_place_rule.h, run by tests/place_rule_driver.cpp under the address
and undefined-behaviour sanitizers, against numpy float32 arithmetic in the stated order, bit for bit; and the parts of the
interface that need no device -- header text, symbols, sizeof(rtk_placement), argtypes, the refusals decided before any HIP call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from rtk_amd.types import MeshSet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_BAD_ARG, ERR_UNSUPPORTED = -2, -6
PLACED_SYMBOLS = ["rtk_dev_scene_build_placed", "rtk_dev_scene_refit_placed", "rtk_dev_scene_refit_meshes_placed",
                  "rtk_mgpu_build_placed", "rtk_mgpu_refit_placed", "rtk_mgpu_refit_meshes_placed"]


def place_np(m, v):
    """The rule in numpy: m float32 [..., 12] (or [..., 3, 4]), v [..., 3] float32 or float64 -> float32 [..., 3]. Every product and
    every sum is one float32 operation, in the order the header states."""
    m = np.asarray(m, np.float32)
    m = m.reshape(m.shape[:-2] + (12,)) if m.shape[-2:] == (3, 4) else m
    v = np.asarray(v).astype(np.float32)
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    with np.errstate(all="ignore"):
        out = [((m[..., 4 * r] * x + m[..., 4 * r + 1] * y) + m[..., 4 * r + 2] * z) + m[..., 4 * r + 3] for r in range(3)]
    out = np.stack(out, -1)
    assert out.dtype == np.float32
    return out


def run_driver(exe, m, v):
    """m [n, 12] float32, v [n, 3] float32 or float64 -> the driver's result bits, uint32 [n, 3]."""
    m = np.ascontiguousarray(m, np.float32)
    f64 = v.dtype == np.float64
    mw, vw = m.view(np.uint32), np.ascontiguousarray(v).view(np.uint64 if f64 else np.uint32)
    text = "".join("%s %s %s\n" % ("d" if f64 else "f", " ".join("%x" % w for w in mw[i]), " ".join("%x" % w for w in vw[i])) for i in range(len(m)))
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    assert lines[len(m)] == "ok"
    return np.array([[int(w, 16) for w in line.split()] for line in lines[:len(m)]], np.uint64).astype(np.uint32).reshape(-1, 3)


def same_bits(got, want):
    """Bit for bit, except where the expected value is NaN: there only "it is NaN" is promised."""
    got_f, want_f = got.view(np.float32), want.view(np.float32)
    nan = np.isnan(want_f)
    assert (np.isnan(got_f) == nan).all()
    bad = (got != want.view(np.uint32)) & ~nan
    assert not bad.any(), (np.argwhere(bad)[:5], got[bad][:5], want.view(np.uint32)[bad][:5])


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """The driver built against the header alone (no HIP include path, -Wall -Werror, no FMA contraction as in the library)
    with both sanitizers. -O2 and -mfma: a compiler that were allowed to contract would do it here."""
    exe = str(tmp_path_factory.mktemp("place_rule") / "place_rule_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-mfma", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "rtk_amd", "csrc"), os.path.join(ROOT, "tests", "place_rule_driver.cpp"), "-o", exe])
    return exe


def test_rule_header_includes_no_hip_and_says_what_it_must():
    text = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_place_rule.h")).read()
    assert [l.split()[1] for l in text.splitlines() if l.startswith("#include")] == ["<stdint.h>"]
    assert "__fmul_rn" in text and "__fadd_rn" in text and "-ffp-contract=off" in text
    assert "-0" in text and "0 * inf" in text and "NaN" in text and "enormal" in text


def test_library_flags_keep_the_rule():
    """No contraction on either side, nothing that flushes f32 denormals on the device."""
    mk = open(os.path.join(ROOT, "rtk_amd", "csrc", "Makefile")).read()
    flags = mk[mk.index("FLAGS   :="):mk.index("LLVMBIN")]
    assert "-ffp-contract=off" in flags and "-fno-fast-math" in flags
    assert "flush-denormals" not in mk and "-ffast-math" not in mk and "-Ofast" not in mk and "-cl-denorms-are-zero" not in mk
    assert "rtk_place_rule.h" in mk


def test_random_cases(driver):
    rng = np.random.RandomState(20240611)
    n = 4000
    m = (rng.standard_normal((n, 12)) * np.exp(rng.uniform(-6, 6, (n, 12)))).astype(np.float32)
    v = (rng.standard_normal((n, 3)) * np.exp(rng.uniform(-6, 6, (n, 3)))).astype(np.float32)
    want = place_np(m, v)
    same_bits(run_driver(driver, m, v), want)
    # the order matters: the same cases summed in double and rounded once differ somewhere (so the comparison can fail)
    once = ((m.astype(np.float64).reshape(n, 3, 4)[:, :, :3] * v.astype(np.float64)[:, None, :]).sum(-1) + m.reshape(n, 3, 4)[:, :, 3]).astype(np.float32)
    assert (once.view(np.uint32) != want.view(np.uint32)).any()
    # rows whose products cancel: where a fused multiply-add would show
    a = rng.standard_normal((n, 1)).astype(np.float32)
    m2 = m.copy()
    m2[:, 0::4], m2[:, 1::4] = a, -a
    v2 = v.copy()
    v2[:, 1] = v2[:, 0] * np.float32(1.0000001)
    same_bits(run_driver(driver, m2, v2), place_np(m2, v2))


def test_double_vertices_are_made_float_first(driver):
    rng = np.random.RandomState(7)
    n = 2000
    m = rng.standard_normal((n, 12)).astype(np.float32)
    v = rng.standard_normal((n, 3)) * np.exp(rng.uniform(-20, 20, (n, 3)))
    v[:8] = 1e-42 * rng.standard_normal((8, 3))                    # doubles that become float denormals
    want = place_np(m, v)
    same_bits(run_driver(driver, m, v), want)
    wide = ((m.astype(np.float64).reshape(n, 3, 4)[:, :, :3] * v[:, None, :]).sum(-1) + m.reshape(n, 3, 4)[:, :, 3]).astype(np.float32)
    assert (wide.view(np.uint32) != want.view(np.uint32)).any()


def fixed_cases():
    ident = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)
    tiny, inf, nan, big = np.float32(1e-30), np.float32(np.inf), np.float32(np.nan), np.float32(3e38)
    den = np.float32(1e-40)                                           # a denormal
    assert 0 < den < np.finfo(np.float32).tiny
    cases = [
        (ident, [0.0, 0.0, 0.0]), (ident, [-0.0, -0.0, -0.0]), (ident, [-0.0, 1.0, -2.0]), (-ident, [0.0, -0.0, 3.0]),
        (ident, [den, -den, 3 * den]), (ident * np.float32(0.5), [den, -den, 3 * den]),
        # results in the denormal range: scale 1e-30 on coordinates 1e-10
        (ident * tiny, [1e-10, -2e-10, 3.5e-10]), (ident * tiny, [1e-10, 1e-12, 1e-15]),
        (np.array([tiny, tiny, tiny, 0, tiny, -tiny, tiny, den, 0, 0, tiny, -den], np.float32), [1e-10, 2e-10, -3e-10]),
        # overflow to +inf and -inf, in a product and in a sum
        (ident * big, [2.0, -2.0, 1.0]), (np.array([1, 1, 0, 0, -1, -1, 0, 0, 1, 0, 0, big], np.float32), [big, big, big]),
        # inf and NaN: 0 * inf is NaN, so the identity turns an infinite coordinate into NaNs in the other rows
        (ident, [inf, 1.0, 2.0]), (ident, [1.0, -inf, 2.0]), (ident, [nan, 1.0, 2.0]),
        (np.array([inf, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), [1.0, 2.0, 3.0]), (np.array([inf, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), [0.0, 2.0, 3.0]),
        (np.array([1, 0, 0, nan, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), [1.0, 2.0, 3.0]),
        (np.array([1, 0, 0, inf, 0, 1, 0, -inf, 0, 0, 1, 0], np.float32), [-inf, inf, 3.0]),
    ]
    m = np.stack([np.asarray(c[0], np.float32) for c in cases])
    v = np.array([c[1] for c in cases], np.float32)
    return m, v


def test_fixed_cases(driver):
    m, v = fixed_cases()
    want = place_np(m, v)
    w = want.view(np.uint32)
    # the list does hold what it claims to: -0 -> +0 under the identity, denormal results, both infinities, NaNs
    assert v.view(np.uint32)[1, 0] == 0x80000000 and w[1, 0] == 0
    tiny = np.finfo(np.float32).tiny
    assert ((np.abs(want[6:9]) > 0) & (np.abs(want[6:9]) < tiny)).any(1).all()
    assert np.isposinf(want[9:11]).any() and np.isneginf(want[9:11]).any()
    assert np.isnan(want[11, 1]) and np.isnan(want[11, 2]) and np.isposinf(want[11, 0])
    assert np.isnan(want[15, 0]) and np.isnan(want[17]).any()
    same_bits(run_driver(driver, m, v), want)


def test_symbols_header_and_argtypes(api):
    header = open(os.path.join(ROOT, "include", "rtk_amd.h")).read()
    L = api.lib()
    for name in PLACED_SYMBOLS:
        assert name in api.RTK_AMD_H_SYMBOLS and hasattr(L, name) and name + "(" in header
    assert "typedef struct rtk_placement { float m[12]; } rtk_placement;" in header
    assert "rtk_dev_scene *rtk_dev_scene_build_placed(const rtk_scene_desc *desc, const rtk_placement *placements);" in header
    assert "int rtk_dev_scene_refit_placed(rtk_dev_scene *ds, const rtk_scene_desc *desc, const rtk_placement *placements, void *stream);" in header
    assert "int rtk_mgpu_refit_placed(rtk_mgpu *m, const rtk_scene_desc *desc, const rtk_placement *placements);" in header
    assert "sizeof(rtk_placement) == 48" in open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_layout_check.h")).read()
    from rtk_amd import types
    assert C.sizeof(types.Placement) == 48
    P, D, U = C.POINTER(types.Placement), C.POINTER(types.SceneDesc), C.POINTER(C.c_uint32)
    assert L.rtk_dev_scene_build_placed.argtypes == [D, P] and L.rtk_dev_scene_build_placed.restype == C.c_void_p
    assert L.rtk_dev_scene_refit_placed.argtypes == [C.c_void_p, D, P, C.c_void_p] and L.rtk_dev_scene_refit_placed.restype == C.c_int
    assert L.rtk_dev_scene_refit_meshes_placed.argtypes == [C.c_void_p, D, P, U, C.c_size_t, C.c_void_p]
    assert L.rtk_mgpu_build_placed.argtypes == [C.c_void_p, D, P] and L.rtk_mgpu_refit_placed.argtypes == [C.c_void_p, D, P]
    assert L.rtk_mgpu_refit_meshes_placed.argtypes == [C.c_void_p, D, P, U, C.c_size_t]
    import inspect
    assert "placements" in inspect.signature(api.DeviceScene.build).parameters
    assert list(inspect.signature(api.DeviceScene.refit).parameters)[1:] == ["meshes", "only", "placements"]


def test_placement_array_shapes():
    from rtk_amd.types import placement_array
    a = np.arange(24, dtype=np.float64).reshape(2, 3, 4)
    for form in (a, a.reshape(2, 12), a.tolist()):
        out = placement_array(form, 2)
        assert out.dtype == np.float32 and out.shape == (2, 12) and out.flags["C_CONTIGUOUS"] and (out.reshape(-1) == np.arange(24)).all()
    with pytest.raises(ValueError):
        placement_array(a, 3)


def test_null_arguments_are_refused_without_a_gpu(api):
    from rtk_amd import types
    L = api.lib()
    ms = MeshSet([dict(positions=np.zeros((3, 3), np.float32))])
    pl = (types.Placement * 1)()
    ids = (C.c_uint32 * 1)(0)
    dummy = C.cast(C.create_string_buffer(8), C.c_void_p)         # (NULL arguments are looked at before the scene is)
    assert not L.rtk_dev_scene_build_placed(C.byref(ms.desc), None)
    assert "rtk_dev_scene_build_placed" in api.last_error() and "placements" in api.last_error()
    assert not L.rtk_dev_scene_build_placed(None, pl)
    for args in ((None, C.byref(ms.desc), pl, None), (dummy, None, pl, None), (dummy, C.byref(ms.desc), None, None)):
        assert L.rtk_dev_scene_refit_placed(*args) == ERR_BAD_ARG
        assert "rtk_dev_scene_refit_placed" in api.last_error()
    for args in ((None, C.byref(ms.desc), pl, ids, 1, None), (dummy, None, pl, ids, 1, None), (dummy, C.byref(ms.desc), None, ids, 1, None),
                 (dummy, C.byref(ms.desc), pl, None, 1, None)):
        assert L.rtk_dev_scene_refit_meshes_placed(*args) == ERR_BAD_ARG
        assert "rtk_dev_scene_refit_meshes_placed" in api.last_error()
    assert L.rtk_mgpu_build_placed(None, C.byref(ms.desc), pl) == ERR_BAD_ARG
    assert L.rtk_mgpu_build_placed(dummy, C.byref(ms.desc), None) == ERR_BAD_ARG and "rtk_mgpu_build_placed" in api.last_error()
    assert L.rtk_mgpu_refit_placed(None, C.byref(ms.desc), pl) == ERR_BAD_ARG and "rtk_mgpu_refit_placed" in api.last_error()
    assert L.rtk_mgpu_refit_placed(dummy, C.byref(ms.desc), None) == ERR_BAD_ARG
    assert L.rtk_mgpu_refit_meshes_placed(None, C.byref(ms.desc), pl, ids, 1) == ERR_BAD_ARG and "rtk_mgpu_refit_meshes_placed" in api.last_error()
    assert L.rtk_mgpu_refit_meshes_placed(dummy, C.byref(ms.desc), None, ids, 1) == ERR_BAD_ARG
    # a position callback takes no placement: refused with its own code before a device is asked for
    ms._arr[0].position_cb = 1
    assert L.rtk_mgpu_build_placed(dummy, C.byref(ms.desc), pl) == ERR_UNSUPPORTED and "callback" in api.last_error()
