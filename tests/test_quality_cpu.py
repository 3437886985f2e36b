"""CPU tests of rtk_dev_scene_quality: exported, declared, bound, and refusing bad arguments on the host before HIP is
touched (no GPU here)."""
import ctypes as C
import os

from rtk_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTK_AMD_ERR_BAD_ARG = -2
# sizeof(rtk_dev_scene_quality_info): two 32-bit words, two 64-bit counts, nine doubles (the static_assert in
# rtk_amd/csrc/rtk_layout_check.h holds the same number)
QUALITY_INFO_BYTES = 96


def _lib():
    if not os.path.exists(api.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return api.lib()


def test_quality_symbol_is_exported_declared_and_bound():
    L = _lib()
    header = open(os.path.join(ROOT, "include", "rtk_amd.h")).read()
    assert hasattr(L, "rtk_dev_scene_quality"), "librtk_amd.so does not export rtk_dev_scene_quality"
    assert "rtk_dev_scene_quality(" in header, "rtk_amd.h does not declare rtk_dev_scene_quality"
    assert "rtk_dev_scene_quality" in api.RTK_AMD_H_SYMBOLS
    assert hasattr(api.DeviceScene, "quality")


def test_structure_size_matches_the_header():
    assert C.sizeof(api.SceneQuality) == QUALITY_INFO_BYTES
    check = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_layout_check.h")).read()
    assert "sizeof(rtk_dev_scene_quality_info) == %d" % QUALITY_INFO_BYTES in check
    # field for field what the header declares, in its order
    header = open(os.path.join(ROOT, "include", "rtk_amd.h")).read()
    body = header[header.index("typedef struct rtk_dev_scene_quality_info {"):header.index("} rtk_dev_scene_quality_info;")]
    declared = [ln.split(";")[0].split()[-1] for ln in body.splitlines()[1:] if ";" in ln]
    assert declared == [k for k, _ in api.SceneQuality._fields_]
    assert api.SceneQuality.measure_ms.offset == QUALITY_INFO_BYTES - 8


def test_bad_arguments_are_refused_without_a_gpu():
    L = _lib()
    q = api.SceneQuality()
    q.struct_size = C.sizeof(api.SceneQuality)
    assert L.rtk_dev_scene_quality(None, C.byref(q), None) == RTK_AMD_ERR_BAD_ARG
    assert "rtk_dev_scene_quality" in api.last_error()
    # (NULL `out` and the size are looked at before the scene is: any non-NULL handle will do)
    dummy = C.create_string_buffer(8)
    assert L.rtk_dev_scene_quality(C.cast(dummy, C.c_void_p), None, None) == RTK_AMD_ERR_BAD_ARG
    assert "rtk_dev_scene_quality" in api.last_error()
    for size in (0, 8, C.sizeof(api.SceneQuality) - 1):
        q = api.SceneQuality()
        q.struct_size = size
        assert L.rtk_dev_scene_quality(C.cast(dummy, C.c_void_p), C.byref(q), None) == RTK_AMD_ERR_BAD_ARG
        assert "rtk_dev_scene_quality" in api.last_error() and "struct_size" in api.last_error()
        assert q.struct_size == size and q.sah_cost == 0.0       # (nothing written)
