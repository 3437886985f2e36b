"""rtk_dev_scene_split_leaves without a GPU: the partition rule of one leaf (rtk_amd/csrc/rtk_split_rule.h) run by
tests/split_rule_driver.cpp under the address and undefined-behaviour sanitizers, and the parts of the interface that need no
device -- the symbols, the Python mirror of rtk_dev_split_info, the refusals that are decided before any HIP call."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_BAD_ARG = -2


@pytest.fixture(scope="module")
def driver_output(tmp_path_factory):
    """The driver built against the header alone (no HIP include path, -Wall -Werror, no FMA contraction as in the library)
    with both sanitizers, and run once."""
    exe = str(tmp_path_factory.mktemp("split_rule") / "split_rule_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "rtk_amd", "csrc"), os.path.join(ROOT, "tests", "split_rule_driver.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


def test_rule_header_includes_no_hip():
    includes = [l.split()[1] for l in open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_split_rule.h")) if l.startswith("#include")]
    assert includes == ["<stdint.h>"]


def test_rule_over_every_leaf(driver_output):
    """Every count 1 .. 63 at max_leaf 1, 3, 4, 62, 63, identical triangles, the geometric line, NaN / inf: the driver's own
    assertions (permutation, leaf sizes, two children or more, the depth cap, the counting entry point, a second run)."""
    lines = driver_output.splitlines()
    assert lines[-1] == "ok" and "FAIL" not in driver_output
    assert "scattered: 315 leaves" in lines and "non-finite: 20 leaves" in lines


def test_geometric_line_stays_within_the_cap(driver_output):
    """The case a free surface-area sweep answers with one triangle per level: 63 triangles at max_leaf 1 would be 62 levels."""
    got = {int(m.group(1)): (int(m.group(2)), int(m.group(3))) for m in re.finditer(r"geometric: max_leaf (\d+) -> (\d+) levels, cap (\d+)", driver_output)}
    assert set(got) == {1, 3, 4, 62, 63}
    # 2 * ceil(log4(63 / max_leaf)): 63 -> 3, 21 -> 3, 15.75 -> 2, 1.02 -> 1, 1 -> 0
    assert {k: v[1] for k, v in got.items()} == {1: 6, 3: 6, 4: 4, 62: 2, 63: 0}
    for levels, cap in got.values():
        assert levels <= cap


def test_symbols_are_listed_and_exported(api):
    assert "rtk_dev_scene_split_leaves" in api.RTK_AMD_H_SYMBOLS and "rtk_mgpu_split_leaves" in api.RTK_AMD_H_SYMBOLS
    header = open(os.path.join(ROOT, "include", "rtk_amd.h")).read()
    assert "int rtk_dev_scene_split_leaves(rtk_dev_scene *ds, uint32_t max_leaf, rtk_dev_split_info *out" in header
    assert "int rtk_mgpu_split_leaves(rtk_mgpu *m, uint32_t max_leaf);" in header
    L = api.lib()
    assert L.rtk_dev_scene_split_leaves.argtypes == [C.c_void_p, C.c_uint32, C.POINTER(api.SplitInfo), C.c_void_p]
    assert L.rtk_mgpu_split_leaves.argtypes == [C.c_void_p, C.c_uint32]
    assert callable(api.DeviceScene.split_leaves)


def test_split_info_mirrors_the_header(api):
    """sizeof(SplitInfo) and the field order against the struct the header declares (rtk_layout_check.h asserts 48 bytes
    at compile time)."""
    header = open(os.path.join(ROOT, "include", "rtk_amd.h")).read()
    body = re.search(r"typedef struct rtk_dev_split_info \{(.*?)\} rtk_dev_split_info;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    size, names = 0, []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, rest = decl.split(None, 1)
        width = {"uint32_t": 4, "uint64_t": 8, "double": 8}[ctype]
        for name in rest.split(","):
            size = (size + width - 1) // width * width + width
            names.append(name.strip())
    assert size == 48 and C.sizeof(api.SplitInfo) == 48
    assert [k for k, _ in api.SplitInfo._fields_] == names
    assert "sizeof(rtk_dev_split_info) == 48" in open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_layout_check.h")).read()


def test_refusals_need_no_gpu(api):
    """ds NULL, max_leaf > 63, a struct_size that is too small: RTK_AMD_ERR_BAD_ARG before any HIP call (none of them looks at
    the scene, so a handle that is no scene is enough here)."""
    L = api.lib()
    info = api.SplitInfo()
    info.struct_size = C.sizeof(api.SplitInfo)
    assert L.rtk_dev_scene_split_leaves(None, 3, C.byref(info), None) == ERR_BAD_ARG
    assert "NULL" in api.last_error()
    not_a_scene = C.create_string_buffer(64)
    handle = C.cast(not_a_scene, C.c_void_p)
    assert L.rtk_dev_scene_split_leaves(handle, 64, C.byref(info), None) == ERR_BAD_ARG
    assert "max_leaf 64" in api.last_error()
    assert L.rtk_dev_scene_split_leaves(handle, 0xFFFFFFFF, None, None) == ERR_BAD_ARG
    info.struct_size = C.sizeof(api.SplitInfo) - 4
    assert L.rtk_dev_scene_split_leaves(handle, 3, C.byref(info), None) == ERR_BAD_ARG
    assert "struct_size" in api.last_error()
    assert L.rtk_mgpu_split_leaves(None, 3) == ERR_BAD_ARG
    assert L.rtk_mgpu_split_leaves(handle, 64) == ERR_BAD_ARG
    with pytest.raises(api.RtkError):
        api.DeviceScene.split_leaves(object(), 64)
