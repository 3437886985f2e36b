"""rtk_dev_scene_rebuild without a GPU: the symbols, the Python mirror of rtk_dev_rebuild_info, the refusals that are decided
before any HIP call, and the ledger's adopt_all (how a rebuilt tree's allocations change owners) run by
tests/rebuild_ledger_driver.cpp under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_BAD_ARG = -2


def test_symbols_are_listed_and_exported(api):
    assert "rtk_dev_scene_rebuild" in api.RTK_AMD_H_SYMBOLS and "rtk_mgpu_rebuild" in api.RTK_AMD_H_SYMBOLS
    header = open(os.path.join(ROOT, "include", "rtk_amd.h")).read()
    assert "int rtk_dev_scene_rebuild(rtk_dev_scene *ds, rtk_dev_rebuild_info *out /* may be NULL */, void *stream);" in header
    assert "int rtk_mgpu_rebuild(rtk_mgpu *m);" in header
    L = api.lib()
    assert L.rtk_dev_scene_rebuild.argtypes == [C.c_void_p, C.POINTER(api.RebuildInfo), C.c_void_p]
    assert L.rtk_dev_scene_rebuild.restype is C.c_int
    assert L.rtk_mgpu_rebuild.argtypes == [C.c_void_p] and L.rtk_mgpu_rebuild.restype is C.c_int
    assert callable(api.DeviceScene.rebuild)


def test_rebuild_info_mirrors_the_header(api):
    """sizeof(RebuildInfo) and the field order against the struct the header declares (rtk_layout_check.h asserts 40 bytes
    at compile time)."""
    header = open(os.path.join(ROOT, "include", "rtk_amd.h")).read()
    body = re.search(r"typedef struct rtk_dev_rebuild_info \{(.*?)\} rtk_dev_rebuild_info;", header, re.S).group(1)
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
    assert names == ["struct_size", "key_bits", "nodes_before", "nodes_after", "max_depth_before", "max_depth_after", "rebuild_ms"]
    assert size == 40 and C.sizeof(api.RebuildInfo) == 40
    assert [k for k, _ in api.RebuildInfo._fields_] == names
    assert "sizeof(rtk_dev_rebuild_info) == 40" in open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_layout_check.h")).read()


def test_refusals_need_no_gpu(api):
    """ds NULL and a struct_size that is too small: RTK_AMD_ERR_BAD_ARG before any HIP call and before the scene is looked at
    (a handle that is no scene is enough here); rtk_mgpu_rebuild(NULL) likewise."""
    L = api.lib()
    info = api.RebuildInfo()
    info.struct_size = C.sizeof(api.RebuildInfo)
    assert L.rtk_dev_scene_rebuild(None, C.byref(info), None) == ERR_BAD_ARG
    assert "rtk_dev_scene_rebuild" in api.last_error() and "NULL" in api.last_error()
    assert L.rtk_dev_scene_rebuild(None, None, None) == ERR_BAD_ARG
    not_a_scene = C.create_string_buffer(64)
    handle = C.cast(not_a_scene, C.c_void_p)
    info.struct_size = C.sizeof(api.RebuildInfo) - 4
    assert L.rtk_dev_scene_rebuild(handle, C.byref(info), None) == ERR_BAD_ARG
    assert "struct_size" in api.last_error()
    info.struct_size = 0
    assert L.rtk_dev_scene_rebuild(handle, C.byref(info), None) == ERR_BAD_ARG
    assert L.rtk_mgpu_rebuild(None) == ERR_BAD_ARG
    assert "rtk_mgpu_rebuild" in api.last_error()


def test_forget_slots_is_a_flag_of_its_own():
    """RTK_FORGET_SLOTS shares no bit with the two older flags and is acted on in rtk_scene_forget_derived alone."""
    dev_h = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_dev.h")).read()
    flags = {name: int(value) for name, value in re.findall(r"#define (RTK_FORGET_[A-Z]+) (\d+)u", dev_h)}
    assert set(flags) == {"RTK_FORGET_BOXES", "RTK_FORGET_TREE", "RTK_FORGET_SLOTS"}
    assert sorted(flags.values()) == [1, 2, 4]
    csrc = os.path.join(ROOT, "rtk_amd", "csrc")
    tests = {f: open(os.path.join(csrc, f)).read().count("& RTK_FORGET_SLOTS") for f in os.listdir(csrc) if f.endswith((".hip", ".h", ".cpp"))}
    assert {f for f, k in tests.items() if k} == {"rtk_capi.hip"}


def test_ledger_adopt_all(tmp_path):
    """The driver's own assertions: entries change ledgers with their counted figures, the giver is left empty, every
    pointer is freed exactly once by its new owner. Built against the header alone, run once under both sanitizers
    with leak detection on."""
    exe = str(tmp_path / "rebuild_ledger_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "rtk_amd", "csrc"), os.path.join(ROOT, "tests", "rebuild_ledger_driver.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and r.stderr == "" and r.stdout.splitlines()[-1] == "ok", r.stdout[-2000:] + r.stderr[-4000:]
