"""The three overlap queries on an instanced world without a GPU: the rule of rtk_amd/csrc/rtk_world_overlap_rule.h, run by
tests/world_overlap_rule_driver.cpp (built plain and once more as a stand-alone program under the address and
undefined-behaviour sanitizers), against numpy (tests/world_overlap_ref.py), bit for bit in counts and lists for all three
shapes; the 64-bit insert against a sort; the skip, which never removes a candidate from the walk of a two-level hierarchy,
however its leaves are ordered; and the symbols, argtypes and refusals of the interface that need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import world_overlap_ref as R
from tests.test_gpu_world import TRIS, case
from tests.test_world_cpu import ERR_BAD_ARG, _hex, run_driver
from tests.world_ref import F, PRIM_NONE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LETTER = {"box": "b", "obb": "o", "touch": "t"}


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if request.param == "sanitized" else []
    exe = str(tmp_path_factory.mktemp("world_overlap_rule_" + request.param) / "world_overlap_rule_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-mfma", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"] + extra +
                          ["-I" + os.path.join(ROOT, "rtk_amd", "csrc"), os.path.join(ROOT, "tests", "world_overlap_rule_driver.cpp"), "-o", exe])
    return exe


def world_lines(which, places, live, mask=None):
    lines = ["s %d %s" % (len(t), _hex(t)) for t in TRIS]
    return lines + ["i %d %d %s" % (which[k], int(live[k] and (mask is None or mask[k])), _hex(places[k])) for k in range(len(which))]


def parse(rows):
    """driver lines -> (counts, lists of uint64 keys)"""
    counts = np.array([r[0] for r in rows], np.uint32)
    lists = [R.keys_of(r[1::2], r[2::2]) if len(r) > 1 else np.zeros(0, np.uint64) for r in rows]
    return counts, lists


_WORLDS = {}


def world(name):
    """(which, places, live, {shape: queries}): 160 live queries and 32 others per shape, shared by the tests"""
    if name not in _WORLDS:
        which, places = case(name)
        live = R.live_instances(TRIS, which, places)
        rng = np.random.RandomState(53)
        _WORLDS[name] = (which, places, live, {s: R.make_queries(s, TRIS, which, places, rng, 160, 32, 0.4) for s in R.SHAPES})
    return _WORLDS[name]


def test_rule_header_is_for_the_host_and_the_device():
    text = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_world_overlap_rule.h")).read()
    assert [l.split()[1] for l in text.splitlines() if l.startswith("#include")] == ['"rtk_world_closest_rule.h"', '"rtk_box_rule.h"', '"rtk_obb_rule.h"', '"rtk_touch_rule.h"']
    assert "hip/" not in text and "math.h" not in text and "<cmath>" not in text
    for word in ("THE PLACED TRIANGLE", "THE SKIP", "WHY NO MARGIN IS NEEDED", "ALL THREE SKIPS ARE COMPARISONS", "No condition number", "THE ENTRY AND THE ORDER",
                 "((uint64_t)instance << 32) | prim", "ASCENDING KEY", "THE INSERT", "LIVENESS", "DEAD INSTANCES", "FILTER", "TREE INDEPENDENCE", "No HIP, no libm",
                 "FORWARD", "DESIGN.md 3.23.2"):
        assert word in text, word
    drv = open(os.path.join(ROOT, "tests", "world_overlap_rule_driver.cpp")).read()
    assert [l.split()[1] for l in drv.splitlines() if l.startswith("#include") and '"' in l] == ['"rtk_world_overlap_rule.h"']
    kernel = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_world_overlap.hip")).read()
    for word in ("rtk_world_overlap_rule.h", "rtk_world_overlap_insert(", "rtk_world_overlap_place(", "rtk_world_placed_box(", "rtk_world_launch(", "WO_RESOURCES",
                 "scratch 0", "rtk_box_shape.h", "rtk_obb_shape.h", "rtk_touch_shape.h"):
        assert word in kernel, word
    mk = open(os.path.join(ROOT, "rtk_amd", "csrc", "Makefile")).read()
    for name in ("rtk_world_overlap.hip", "rtk_world_overlap_rule.h", "rtk_box_shape.h", "rtk_obb_shape.h", "rtk_touch_shape.h"):
        assert name in mk, name
    # each Shape is defined once, in the header its scene walk and the world's walk include
    for shape, stem in (("Box", "rtk_box"), ("Obb", "rtk_obb"), ("Touch", "rtk_touch")):
        assert open(os.path.join(ROOT, "rtk_amd", "csrc", stem + "_shape.h")).read().count("struct %s {" % shape) == 1
        assert "struct %s {" % shape not in open(os.path.join(ROOT, "rtk_amd", "csrc", stem + ".hip")).read()
        assert '#include "%s_shape.h"' % stem in open(os.path.join(ROOT, "rtk_amd", "csrc", stem + ".hip")).read()


@pytest.mark.parametrize("name", ["special", "two"])
def test_driver_equals_the_reference_bit_for_bit(driver, tmp_path, name):
    which, places, live, queries = world(name)
    rng = np.random.RandomState(59)
    assert live.all()
    for shape in R.SHAPES:
        q = queries[shape]
        ignore = rng.randint(0, len(which) + 1, len(q)).astype(np.uint32)
        ignore[::3] = PRIM_NONE
        mask = np.ones(len(which), bool)
        mask[-1] = False
        for use_filter, flags in ((False, 0), (True, 1 if shape == "touch" else 0)):
            want = R.brute_force(shape, TRIS, which, places, q, mask if use_filter else None, ignore if use_filter else None, flags)
            pruned = R.brute_force(shape, TRIS, which, places, q, mask if use_filter else None, ignore if use_filter else None, flags, prune=True)
            assert (want.counts == pruned.counts).all() and (want.flat() == pruned.flat()).all()      # (the pruned form the GPU test uses)
            ign = ignore if use_filter else np.full(len(q), PRIM_NONE, np.uint32)
            lines = world_lines(which, places, live, mask if use_filter else None)
            lines += ["q %s %x %x -1 %s" % (LETTER[shape], ign[i], flags, _hex(q[i])) for i in range(len(q))]
            counts, lists = parse(run_driver(driver, lines, tmp_path, "%s_%s_%d" % (name, shape, use_filter)))
            assert (counts == want.counts).all(), (shape, np.flatnonzero(counts != want.counts)[:5])
            assert all((a == b).all() for a, b in zip(lists, want.lists)), shape
            if not use_filter:
                assert (want.counts[:160] > 0).all() and (want.counts[160:] == 0).all(), shape      # built to hit; not live or far away
                assert all((np.diff(l.astype(np.int64)) > 0).all() for l in lists)
            # room: the first min(count, room) entries
            for room in (0, 1, 3):
                rows = ["q %s %x %x %d %s" % (LETTER[shape], ign[i], flags, room, _hex(q[i])) for i in range(0, len(q), 4)]
                c2, l2 = parse(run_driver(driver, world_lines(which, places, live, mask if use_filter else None) + rows, tmp_path, "room"))
                assert (c2 == want.counts[::4]).all() and all((a == b[:room]).all() and len(a) == min(room, len(b)) for a, b in zip(l2, want.lists[::4]))


@pytest.mark.parametrize("name", ["special", "two"])
def test_shared_vertices_are_compared_on_the_placed_vertices(driver, tmp_path, name):
    """Query triangles with a vertex that has the bits of a placed vertex: with RTK_TOUCH_SKIP_SHARED_VERTEX the driver's brute
    force and its walk leave out the records around that vertex, without it they list them -- as the reference says"""
    which, places, live, _ = world(name)
    q = R.shared_vertex_queries(TRIS, which, places, np.random.RandomState(67), 120)
    plain = R.brute_force("touch", TRIS, which, places, q)
    skipped = R.brute_force("touch", TRIS, which, places, q, flags=R.SKIP_SHARED_VERTEX)
    # from the reference alone: the flag removes candidates from every query and adds none
    assert (plain.counts > skipped.counts).all() and all(np.isin(b, a).all() for a, b in zip(plain.lists, skipped.lists))
    assert int(skipped.counts.sum()) > 0
    for flags, want in ((0, plain), (R.SKIP_SHARED_VERTEX, skipped)):
        for kind, last in (("q", -1), ("w", 0), ("w", 3)):
            lines = world_lines(which, places, live) + ["%s t %x %x %d %s" % (kind, PRIM_NONE, flags, last, _hex(q[i])) for i in range(len(q))]
            counts, lists = parse(run_driver(driver, lines, tmp_path, "shared_%s_%d_%d" % (kind, flags, last)))
            assert (counts == want.counts).all(), (kind, flags, np.flatnonzero(counts != want.counts)[:5])
            assert all((a == b).all() for a, b in zip(lists, want.lists)), (kind, flags)


def test_insert_keeps_the_first_of_the_sorted_set(driver, tmp_path):
    rng = np.random.RandomState(61)
    lines, want = [], []
    for trial in range(300):
        K = int(rng.randint(0, 40))
        # distinct keys; a third of the streams differ only in the instance half, a third only in the prim half
        hi = rng.randint(0, 1 << 31, K).astype(np.uint64) if trial % 3 else rng.randint(0, 4, K).astype(np.uint64)
        lo = rng.randint(0, 1 << 32, K).astype(np.uint64) if trial % 3 != 1 else np.full(K, 7, np.uint64)
        keys = np.unique((hi << np.uint64(32)) | lo)
        keys = keys[rng.permutation(len(keys))]                                # any arrival order
        if trial % 5 == 0:
            keys = np.sort(keys)[::-1] if trial % 10 else np.sort(keys)      # descending: every key displaces; ascending: none does
        for room in (0, 1, 3, len(keys) + 5):
            lines.append("n %d %d %s" % (room, len(keys), " ".join("%x %x" % (int(k) >> 32, int(k) & 0xffffffff) for k in keys)))
            want.append((room, np.sort(keys)[:room]))
    got = run_driver(driver, lines, tmp_path, "insert")
    untouched = 0x7e7e7e7e7e7e7e7e
    for row, (room, first) in zip(got, want):
        buf = R.keys_of(row[1::2], row[2::2])
        assert row[0] == len(first) and len(buf) == room + 4
        assert (buf[:len(first)] == first).all() and (buf[len(first):] == np.uint64(untouched)).all(), (room, first, buf)


@pytest.mark.parametrize("name", ["special", "two"])
def test_the_skip_never_removes_a_candidate(driver, tmp_path, name):
    """The walk of a two-level hierarchy made by the driver -- the proxy box as it is, the scene's root box and leaves of four
    records through the placed box -- reaches every candidate of the brute force, for every order of its leaves"""
    which, places, live, queries = world(name)
    for shape in R.SHAPES:
        q = queries[shape]
        want = R.brute_force(shape, TRIS, which, places, q)
        assert int(want.counts.sum()) > 500
        for seed in (0, 1, 2):
            lines = world_lines(which, places, live) + ["w %s %x 0 %d %s" % (LETTER[shape], PRIM_NONE, seed, _hex(q[i])) for i in range(len(q))]
            counts, lists = parse(run_driver(driver, lines, tmp_path, "walk_%s_%d" % (shape, seed)))
            assert (counts == want.counts).all(), (shape, seed, np.flatnonzero(counts != want.counts)[:5])
            assert all((a == b).all() for a, b in zip(lists, want.lists)), (shape, seed)


WORLD_CALLS = [stem + tail for stem in ("rtk_dev_world_triangles_in_box", "rtk_dev_world_triangles_in_obb", "rtk_dev_world_triangles_touching")
               for tail in ("_count", "_all", "_counted")]


def test_header_symbols_and_argtypes(api):
    text = open(os.path.join(ROOT, "include", "rtk_amd.h")).read()
    for word in ["int %s(const rtk_dev_world *w, const rtk_" % name for name in WORLD_CALLS] + \
                ["uint32_t rtk_amd_world_overlap_stack_entries(void);", "OVERLAPS ON A WORLD", "((uint64_t)instance << 32) | prim", "ASCENDING ENTRY",
                 "FLAT PLACED TWIN", "uint32_t touch_flags", "rtk_world_overlap_rule.h", "A SLOT THAT IS NOT LISTED IS NOT WRITTEN", "DESIGN.md 3.23.2"]:
        assert word in text, word
    assert "overlaps, pairs and sweeps still take one rtk_dev_scene" not in text
    L = api.lib()
    for name in WORLD_CALLS + ["rtk_amd_world_overlap_stack_entries"]:
        assert name in api.RTK_AMD_H_SYMBOLS and hasattr(L, name), name
    wf, rl, tc = C.POINTER(api.WorldFilter), C.POINTER(api.RayList), C.POINTER(api.TraceCounters)
    v = C.c_void_p
    assert L.rtk_dev_world_triangles_in_box_count.argtypes == [v, v, C.c_size_t, rl, wf, v, v]
    assert L.rtk_dev_world_triangles_in_obb_all.argtypes == [v, v, C.c_size_t, rl, wf, v, v, v, v]
    assert L.rtk_dev_world_triangles_in_box_counted.argtypes == [v, v, C.c_size_t, wf, v, v, v, tc]
    assert L.rtk_dev_world_triangles_touching_count.argtypes == [v, v, C.c_size_t, rl, wf, C.c_uint32, v, v]
    assert L.rtk_dev_world_triangles_touching_all.argtypes == [v, v, C.c_size_t, rl, wf, C.c_uint32, v, v, v, v]
    assert L.rtk_dev_world_triangles_touching_counted.argtypes == [v, v, C.c_size_t, wf, C.c_uint32, v, v, v, tc]
    assert L.rtk_amd_world_overlap_stack_entries() > 0
    for shape in ("in_box", "in_obb", "touching"):
        for name in ("triangles_%s_count_device", "triangles_%s_all_device", "triangles_%s_counted", "triangles_%s"):
            assert callable(getattr(api.DeviceWorld, name % shape)), name % shape
    from rtk_amd import types
    e = np.array([(5 << 32) | 9], np.uint64).view(types.WORLD_ENTRY_DTYPE)
    assert e["instance"][0] == 5 and e["prim"][0] == 9
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        assert "rtk_dev_world_triangles_in_box" in open(os.path.join(ROOT, doc)).read(), doc


def test_refusals_need_no_device(api):
    L = api.lib()
    dummy = C.cast(C.create_string_buffer(64), C.c_void_p)                   # (what is refused is refused before the world is looked at)
    count = C.cast(C.create_string_buffer(8), C.c_void_p)
    ctr = api.TraceCounters()

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

    for stem in ("rtk_dev_world_triangles_in_box", "rtk_dev_world_triangles_in_obb", "rtk_dev_world_triangles_touching"):
        flags = (0,) if stem.endswith("touching") else ()
        fn_count, fn_all, fn_counted = (getattr(L, stem + tail) for tail in ("_count", "_all", "_counted"))

        def refused(fn, name, *args):
            assert fn(*args) == ERR_BAD_ARG, (name, args)
            assert name in api.last_error(), (name, api.last_error())
        # a NULL world, by each door; NULL queries or outputs with n != 0
        refused(fn_count, stem + "_count", None, dummy, 4, None, None, *flags, dummy, None)
        refused(fn_all, stem + "_all", None, dummy, 4, None, None, *flags, dummy, dummy, None, None)
        refused(fn_counted, stem + "_counted", None, dummy, 4, None, *flags, None, None, dummy, C.byref(ctr))
        refused(fn_count, stem + "_count", dummy, None, 4, None, None, *flags, dummy, None)
        refused(fn_count, stem + "_count", dummy, dummy, 4, None, None, *flags, None, None)
        refused(fn_all, stem + "_all", dummy, dummy, 4, None, None, *flags, None, dummy, None, None)
        refused(fn_all, stem + "_all", dummy, dummy, 4, None, None, *flags, dummy, None, None, None)
        refused(fn_counted, stem + "_counted", dummy, dummy, 4, None, *flags, dummy, None, dummy, C.byref(ctr))
        refused(fn_counted, stem + "_counted", dummy, dummy, 4, None, *flags, None, None, dummy, None)
        assert "NULL counters" in api.last_error()
        # a bad list, a bad filter, too many queries
        for l in (ray_list(struct_size=8), ray_list(flags=1), ray_list(d_count=None)):
            refused(fn_count, stem + "_count", dummy, dummy, 4, l, None, *flags, dummy, None)
            refused(fn_all, stem + "_all", dummy, dummy, 4, l, None, *flags, dummy, dummy, None, None)
        for f in (filt(struct_size=16), filt(flags=1), filt(d_instance_mask=dummy.value, instance_mask_bits=0)):
            refused(fn_count, stem + "_count", dummy, dummy, 4, None, f, *flags, dummy, None)
            refused(fn_counted, stem + "_counted", dummy, dummy, 4, f, *flags, None, None, dummy, C.byref(ctr))
        refused(fn_count, stem + "_count", dummy, dummy, 1 << 32, None, None, *flags, dummy, None)
        refused(fn_all, stem + "_all", dummy, dummy, 1 << 32, ray_list(), None, *flags, dummy, dummy, None, None)
        # no queries: nothing to do, nothing launched (the world is not even looked at)
        assert fn_count(dummy, None, 0, None, None, *flags, None, None) == 0
        assert fn_all(dummy, None, 0, ray_list(), filt(), *flags, None, None, None, None) == 0
        assert fn_counted(dummy, None, 0, None, *flags, None, None, None, C.byref(ctr)) == 0
    # an unknown bit of touch_flags, by each door
    stem = "rtk_dev_world_triangles_touching"
    for bad in (2, 0x80000000, 3):
        assert L.rtk_dev_world_triangles_touching_count(dummy, dummy, 4, None, None, bad, dummy, None) == ERR_BAD_ARG
        assert stem + "_count" in api.last_error() and "touch_flags" in api.last_error()
        assert L.rtk_dev_world_triangles_touching_all(dummy, dummy, 4, None, None, bad, dummy, dummy, None, None) == ERR_BAD_ARG
        assert stem + "_all" in api.last_error()
        assert L.rtk_dev_world_triangles_touching_counted(dummy, dummy, 4, None, bad, None, None, dummy, C.byref(ctr)) == ERR_BAD_ARG
        assert stem + "_counted" in api.last_error()
