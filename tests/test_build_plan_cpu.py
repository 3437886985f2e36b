"""What the host decides in a device build between the kernels (rtk_amd/csrc/rtk_build_plan.h), checked without a GPU:
tests/build_plan_driver.cpp is built by the host compiler against that header alone, with -fsanitize=address,undefined, and
answers a table of cases as a child process.

What is expected was written down by reading the build as it was before these decisions moved into the header (plan_meshes,
plan_build, read_build_knobs, alloc_node_estimate, run_collapse and run_stages of rtk_build.hip), not by running the new code.
Every index and position buffer of a mesh case is allocated with exactly the bytes expected here, and the driver reads
[0, ibytes) and [0, pbytes) as the upload would: a plan one byte too long, or a scan of the indices that reads past the last
triple, is a heap overflow the address sanitizer reports."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DEFAULT, F32, F64, REAL, U16, U32 = 0, 1, 2, 3, 4, 5          # rtk_type
ERR_UNSUPPORTED = -6
KNOB_VARS = ["BUILD_TIMING", "BUILD_HOSTTIME", "MAX_LEAF", "SORT_PACKED", "KEY_BITS", "BUILD_DIRECT", "FUSED_EMIT", "TILE_COLLAPSE_MIN", "TOP_CAP",
             "NODE_ESTIMATE_DIV", "KEEP_WORKSPACE", "KEY_REBUILD", "SAH_CN", "SAH_CT"]
KNOB_DEFAULTS = dict(timing=0, host_time=0, max_leaf=3, sort_packed=1, key_bits=0, direct=1, fused_emit=1, tile_min=3 << 19, top_cap=0xffffffff, est_div=0,
                     keep_workspace=1, key_rebuild=1, max_leaf_fn=3, cost_node=0.5, cost_tri=1.0)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("build_plan") / "build_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "rtk_amd", "csrc"),
                           os.path.join(ROOT, "tests", "build_plan_driver.cpp"), "-o", exe])
    return exe


def run(driver, commands, env=None):
    """The driver's answers to `commands`, one list of words each; the run ends clean under the sanitizers."""
    full = {k: v for k, v in os.environ.items() if not k.startswith("RTK_AMD_")}
    full.update(env or {})
    r = subprocess.run([driver], input="".join(c + "\n" for c in commands), capture_output=True, text=True, timeout=120, env=full)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(commands)
    return [line.split() for line in lines]


def test_plan_header_includes_no_hip():
    includes = [l.split()[1] for l in open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_build_plan.h")) if l.startswith("#include")]
    assert includes == ['"rtk.h"', '"rtk_amd.h"', '"rtk_build_layout.h"', "<stddef.h>", "<stdint.h>", "<stdio.h>", "<stdlib.h>", "<algorithm>", "<vector>"]


# ---------------------------------------------------------------------------------------------- mesh plans

def mesh(nt, idx=0, pos=F32, istride=0, pstride=0, idev=0, pdev=0, vcount=None, itype=None, cbs=0, no_positions=False):
    """One mesh of a case. idx: 0 implicit, 1 u16, 2 u32; index value number k is (7 k) mod vcount."""
    return dict(nt=nt, idx=idx, pos=pos, istride=istride, pstride=pstride, idev=idev, pdev=pdev, vcount=vcount or max(3 * nt, 1),
                itype=(itype if itype is not None else (0, U16, U32)[idx]), cbs=cbs, no_positions=no_positions)


def index_extent(m):
    """bytes of the index buffer: the last triple ends (nt - 1) strides in, 6 or 12 bytes long"""
    step = m["istride"] or (6 if m["idx"] == 1 else 12)
    return (m["nt"] - 1) * step + (6 if m["idx"] == 1 else 12)


def expected_plan(m, n):
    """(host, f64, idx_kind, pstride, istride, pbytes, ibytes, pos_dev, idx_dev) as plan_meshes of the parent left them"""
    if m["nt"] == 0:
        return (0, 0, 0, 0, 0, 0, 0, 0, 0)
    if m["cbs"] or n < 2:
        return (1, 0, 0, 0, 0, 0, 0, 0, 0)
    f64 = int(m["pos"] == F64)
    pstride = m["pstride"] or (24 if f64 else 12)
    max_vertex = 3 * m["nt"] - 1
    istride = ibytes = 0
    if m["idx"]:
        istride = m["istride"] or (6 if m["idx"] == 1 else 12)
        if not m["idev"]:
            if not m["pdev"]:
                max_vertex = max((7 * k) % m["vcount"] for k in range(3 * m["nt"]))
            ibytes = index_extent(m)
    pbytes = 0 if m["pdev"] else max_vertex * pstride + (24 if f64 else 12)
    return (0, f64, m["idx"], pstride, istride, pbytes, ibytes, m["pdev"], m["idev"] if m["idx"] else 0)


def meshes_command(meshes, placed=0, n=None):
    n = sum(m["nt"] for m in meshes) if n is None else n
    words = ["meshes", n, placed, len(meshes)]
    for m in meshes:
        palloc = -1 if m["no_positions"] else (expected_plan(m, n)[5] if not (m["cbs"] or n < 2 or m["nt"] == 0) else 0)
        words += [m["nt"], m["idx"], m["itype"], m["istride"], index_extent(m) if m["idx"] else 0, m["idev"], m["vcount"], m["pos"], m["pstride"], palloc, m["pdev"], m["cbs"]]
    return " ".join(str(w) for w in words)


def parse_plans(words, count):
    bar = words.index("|")
    assert bar == 2 + 10 * count, words
    return [tuple(int(w) for w in words[2 + 10 * k: 12 + 10 * k]) for k in range(count)]


FILLER = mesh(2)        # two implicit float triangles: keeps a one-triangle mesh out of the scene of fewer than two
ISTRIDES = {0: [0], 1: [0, 6, 8, 10], 2: [0, 12, 16, 20]}         # default, explicit tight, padded (even / multiples of 4: the values are read in place)
PSTRIDES = {F32: [0, 12, 16, 28], F64: [0, 24, 32, 40]}
HOST_CASES = [mesh(nt, idx, pos, istride, pstride, vcount=vcount)
              for idx in (0, 1, 2) for pos in (F32, F64) for istride in ISTRIDES[idx] for pstride in PSTRIDES[pos] for nt in (1, 2, 129)
              for vcount in ((3 * nt, 5) if idx else (None,))]


def test_mesh_plans_of_host_buffers(driver):
    """implicit / u16 / u32 indices x f32 / f64 positions x default, tight and padded strides x 1, 2 and 129 triangles; where the mesh
    is indexed, the largest index is once 3 nt - 1 (a permutation of all vertices) and once 4 (fewer, or for one triangle more, vertices
    than 3 nt)"""
    answers = run(driver, [meshes_command([m, FILLER]) for m in HOST_CASES])
    for m, words in zip(HOST_CASES, answers):
        assert words[:2] == ["1", "0"], (m, words)
        got = parse_plans(words, 2)
        assert got[0] == expected_plan(m, m["nt"] + 2) + (1,), m
        assert got[1] == (0, 0, 0, 12, 0, 6 * 12, 0, 0, 0, 1), m


def test_mesh_plan_extents_spelled_out(driver):
    """a few of the above by hand: ibytes = (nt - 1) * istride + 6 | 12, pbytes = max_vertex * pstride + 12 | 24"""
    cases = [(mesh(129, 1, F32, vcount=387), (0, 0, 1, 12, 6, 386 * 12 + 12, 128 * 6 + 6, 0, 0)),
             (mesh(129, 1, F64, istride=10, pstride=40, vcount=5), (0, 1, 1, 40, 10, 4 * 40 + 24, 128 * 10 + 6, 0, 0)),
             (mesh(2, 2, F32, istride=20, pstride=16, vcount=6), (0, 0, 2, 16, 20, 5 * 16 + 12, 20 + 12, 0, 0)),
             (mesh(1, 2, F64, vcount=5), (0, 1, 2, 24, 12, 4 * 24 + 24, 12, 0, 0)),
             (mesh(129, 0, F64, pstride=32), (0, 1, 0, 32, 0, 386 * 32 + 24, 0, 0, 0))]
    for (m, want), words in zip(cases, run(driver, [meshes_command([m, FILLER]) for m, _ in cases])):
        assert expected_plan(m, m["nt"] + 2) == want
        assert parse_plans(words, 2)[0] == want + (1,)


def test_position_types_that_mean_float(driver):
    for pos, words in zip((DEFAULT, REAL, F32), run(driver, [meshes_command([mesh(2, 1, pos)]) for pos in (DEFAULT, REAL, F32)])):
        assert parse_plans(words, 1)[0][:4] == (0, 0, 1, 12), pos
    # RTK_TYPE_DEFAULT on an index buffer means 32-bit indices
    words, = run(driver, [meshes_command([mesh(2, 2, F32, itype=DEFAULT)])])
    assert parse_plans(words, 1)[0] == (0, 0, 2, 12, 12, 5 * 12 + 12, 24, 0, 0, 1)


def test_device_buffers_are_not_read_and_not_copied(driver):
    """Both extents are zero for what the callable reports as device memory; with positions on the device the indices are not scanned
    (max_vertex stays 3 nt - 1 and is not needed), with both there nothing is. The device buffers of the driver are one byte long."""
    cases = [mesh(nt, idx, pos, idev=idev, pdev=1, vcount=5) for nt in (1, 2, 129) for idx in (0, 1, 2) for pos in (F32, F64) for idev in ((0, 1) if idx else (0,))]
    for m, words in zip(cases, run(driver, [meshes_command([m, FILLER]) for m in cases])):
        want = expected_plan(m, m["nt"] + 2)
        assert want[5] == 0 and want[7] == 1 and (want[6] == 0) == (m["idev"] == 1 or m["idx"] == 0)
        assert parse_plans(words, 2)[0] == want + (1,), m


REFUSALS = [
    ("bad position type", [mesh(2, pos=U16)], 0, 0, "rtk_dev_scene_build: mesh 0: bad position type 4"),
    ("bad position type in the second mesh", [FILLER, mesh(2, pos=7)], 0, 0, "rtk_dev_scene_build: mesh 1: bad position type 7"),
    ("bad index type", [mesh(2, 2, itype=F32)], 0, 0, "rtk_dev_scene_build: mesh 0: bad index type 1"),
    ("no positions", [mesh(2, no_positions=True)], 0, 0, "rtk_dev_scene_build: mesh 0 has no positions"),
    ("device indices over host positions", [mesh(2, 1, idev=1, pdev=0)], 0, 0, "rtk_dev_scene_build: mesh 0 has device indices but host positions"),
    ("a position callback together with placements", [FILLER, mesh(2, cbs=1)], 1, ERR_UNSUPPORTED,
     "rtk_dev_scene_build_placed: mesh 1: a position callback gives world positions, it takes no placement"),
]


def test_refusals(driver):
    """Each with the text the build reports; a code of its own only where the parent's plan_meshes set one (the placement refusal)."""
    for (name, meshes, placed, rc, text), words in zip(REFUSALS, run(driver, [meshes_command(m, placed) for _, m, placed, _, _ in REFUSALS])):
        assert words[:3] == ["0", str(rc), "|"], name
        assert " ".join(words[3:]) == text, name


def test_what_is_not_refused(driver):
    HOST = (1, 0, 0, 0, 0, 0, 0, 0, 0, 1)
    SKIPPED = (0, 0, 0, 0, 0, 0, 0, 0, 0, 1)
    cases = [
        # callbacks mean host decode, whatever the buffers say (bad types and missing positions included); an index callback takes a placement
        ([mesh(2, cbs=1, pos=7, no_positions=True), FILLER], 0, [HOST, (0, 0, 0, 12, 0, 72, 0, 0, 0, 1)]),
        ([mesh(2, 2, cbs=2, itype=F32), FILLER], 0, [HOST, (0, 0, 0, 12, 0, 72, 0, 0, 0, 1)]),
        ([mesh(2, cbs=3)], 0, [HOST]),
        ([mesh(2, cbs=2)], 1, [HOST]),
        # fewer than two triangles in the scene: every mesh is decoded on the host, and a mesh without positions passes the plan
        ([mesh(1, 1, F64)], 0, [HOST]),
        ([mesh(0), mesh(1, no_positions=True), mesh(0)], 0, [SKIPPED, HOST, SKIPPED]),
        # empty meshes are skipped before anything of theirs is looked at
        ([mesh(0, pos=7), mesh(0, 2, itype=F32), FILLER], 0, [SKIPPED, SKIPPED, (0, 0, 0, 12, 0, 72, 0, 0, 0, 1)]),
        ([], 0, []),
    ]
    for (meshes, placed, want), words in zip(cases, run(driver, [meshes_command(m, placed) for m, placed, _ in cases])):
        assert words[:2] == ["1", "0"], meshes
        assert parse_plans(words, len(meshes)) == want, meshes


def test_mesh_base(driver):
    got = run(driver, ["base 0", "base 3 5 0 7", "base 2 %d 1" % (0x3ffffff0 - 2), "base 2 %d 1" % (0x3ffffff0 - 1), "base 1 %d" % (1 << 40)])
    assert got == [["1", "0"], ["1", "0", "5", "5", "12"], ["1", "0", str(0x3ffffff0 - 2), str(0x3ffffff0 - 1)],
                   ["0", "0", str(0x3ffffff0 - 1), str(0x3ffffff0)], ["0", "0", str(1 << 40)]]


# ---------------------------------------------------------------------------------------------- the build plan

NS = [2, 3, 65536, 65537, 2 ** 24 - 1, 2 ** 24, 0x3fffffef]
PLAN_CASES = [(n, force, packed_knob, key_bits, tile_min, top_cap) for n in NS for force in (0, 40) for packed_knob in (1, 0) for key_bits in (0, 8, 32)
              for tile_min in (3 << 19, 0, 1 << 62) for top_cap in (0xffffffff, 0, 1, 5000)]


def expected_build_plan(n, force, packed_knob, key_bits, tile_min, top_cap):
    lg = (n - 1).bit_length()                         # ceil(log2 n)
    bits = min(max((lg + 8 + 7) // 8 * 8, 24), 40)
    bits = key_bits or force or bits                  # the knob over force_bits over the width from n
    tiles = (n + 1023) // 1024
    return (int(n < 2 ** 24 and packed_knob), bits, tiles, int(tiles > 1 and n >= tile_min), min(n // 2, top_cap))


def test_build_plan(driver):
    got = run(driver, ["plan %d %d %d %d %d %d" % c for c in PLAN_CASES])
    for c, words in zip(PLAN_CASES, got):
        assert tuple(int(w) for w in words) == expected_build_plan(*c), c


def test_key_widths_spelled_out():
    widths = {n: expected_build_plan(n, 0, 1, 0, 3 << 19, 0xffffffff)[1] for n in NS}
    assert widths == {2: 24, 3: 24, 65536: 24, 65537: 32, 2 ** 24 - 1: 32, 2 ** 24: 32, 0x3fffffef: 40}
    assert expected_build_plan(3 << 19, 0, 1, 0, 3 << 19, 0xffffffff)[3] == 1 and expected_build_plan((3 << 19) - 1, 0, 1, 0, 3 << 19, 0xffffffff)[3] == 0
    assert expected_build_plan(1024, 0, 1, 0, 0, 0xffffffff)[2:4] == (1, 0) and expected_build_plan(1025, 0, 1, 0, 0, 0xffffffff)[2:4] == (2, 1)


def test_build_plan_at_the_tile_thresholds(driver):
    cases = [(n, 0, 1, 0, tile_min, 0xffffffff) for n, tile_min in (((3 << 19) - 1, 3 << 19), (3 << 19, 3 << 19), (1024, 0), (1025, 0), (1025, 1025), (1025, 1026))]
    for c, words in zip(cases, run(driver, ["plan %d %d %d %d %d %d" % c for c in cases])):
        assert tuple(int(w) for w in words) == expected_build_plan(*c), c


# ---------------------------------------------------------------------------------------------- the three rules

def test_first_node_capacity(driver):
    cases = [(n, div) for n in NS + [8191, 8192] for div in (0, -3, 1, 2, 7, 100000)]
    for (n, div), words in zip(cases, run(driver, ["estimate %d %d" % c for c in cases])):
        assert int(words[0]) == (n // div + 16 if div > 0 else n // 2 + 4096), (n, div)


def test_narrow_key_verdict(driver):
    """packed, fewer than 40 bits, and more than an eighth of the sorted neighbours equal: the border is equal * 8 == n"""
    cases = [(packed, bits, equal, n) for packed in (1, 0) for bits in (24, 32, 40) for n in (8, 1000, 1001, 2 ** 24 - 1, 0x3fffffef)
             for equal in sorted({0, max(n // 8 - 1, 0), n // 8, n // 8 + 1, n - 1})]
    for (packed, bits, equal, n), words in zip(cases, run(driver, ["narrow %d %d %d %d" % c for c in cases])):
        assert int(words[0]) == int(bool(packed) and bits < 40 and equal * 8 > n), (packed, bits, equal, n)
    assert run(driver, ["narrow 1 32 125 1000", "narrow 1 32 126 1000"]) == [["0"], ["1"]]


def test_big_levels(driver):
    """2, and one more for every power-of-four multiple of COLLAPSE_SMALL_JOBS (64) that is still below jobs_hint"""
    hints = sorted({h for k in range(0, 14) for h in (64 * 4 ** k - 1, 64 * 4 ** k, 64 * 4 ** k + 1)} | {0, 1, 2, 16, 0x3fffffef, 16 * ((0x3fffffef + 1023) // 1024)})
    for hint, words in zip(hints, run(driver, ["levels %d" % h for h in hints])):
        want = 2
        c = 64
        while c < hint:
            want += 1
            c *= 4
        assert int(words[0]) == want, hint
    assert run(driver, ["levels 64", "levels 65", "levels 256", "levels 257"]) == [["2"], ["3"], ["3"], ["4"]]


# ---------------------------------------------------------------------------------------------- knobs

def knobs(driver, env):
    words, = run(driver, ["knobs"], {"RTK_AMD_" + k: v for k, v in env.items()})
    return {k: float(v) if "cost" in k else int(v) for k, v in (w.split("=") for w in words)}


def want_knobs(**changed):
    return dict(KNOB_DEFAULTS, **changed)


def test_knob_defaults(driver):
    assert knobs(driver, {}) == KNOB_DEFAULTS


KNOB_CASES = [
    # set at all
    ("BUILD_TIMING", "", dict(timing=1)), ("BUILD_TIMING", "0", dict(timing=1)), ("BUILD_TIMING", "1", dict(timing=1)), ("BUILD_TIMING", "no", dict(timing=1)),
    # only when it reads as non-zero
    ("BUILD_HOSTTIME", "", {}), ("BUILD_HOSTTIME", "0", {}), ("BUILD_HOSTTIME", "1", dict(host_time=1)), ("BUILD_HOSTTIME", "yes", {}), ("BUILD_HOSTTIME", "7", dict(host_time=1)),
    # 1 .. 63, default 3 (the empty string is the default)
    ("MAX_LEAF", "", {}), ("MAX_LEAF", "0", dict(max_leaf=1, max_leaf_fn=1)), ("MAX_LEAF", "1", dict(max_leaf=1, max_leaf_fn=1)), ("MAX_LEAF", "8", dict(max_leaf=8, max_leaf_fn=8)),
    ("MAX_LEAF", "63", dict(max_leaf=63, max_leaf_fn=63)), ("MAX_LEAF", "64", dict(max_leaf=63, max_leaf_fn=63)), ("MAX_LEAF", "100000", dict(max_leaf=63, max_leaf_fn=63)),
    ("MAX_LEAF", "2.9", dict(max_leaf=2, max_leaf_fn=2)),
    # 8, 16, 24, 32, 40 and nothing else
    ("KEY_BITS", "", {}), ("KEY_BITS", "0", {}), ("KEY_BITS", "1", {}), ("KEY_BITS", "7", {}), ("KEY_BITS", "12", {}), ("KEY_BITS", "48", {}), ("KEY_BITS", "-8", {}),
    ("KEY_BITS", "8", dict(key_bits=8)), ("KEY_BITS", "16", dict(key_bits=16)), ("KEY_BITS", "24", dict(key_bits=24)), ("KEY_BITS", "32", dict(key_bits=32)), ("KEY_BITS", "40", dict(key_bits=40)),
    # read per build; the empty string reads as 0
    ("TILE_COLLAPSE_MIN", "", dict(tile_min=0)), ("TILE_COLLAPSE_MIN", "0", dict(tile_min=0)), ("TILE_COLLAPSE_MIN", "1", dict(tile_min=1)),
    ("TILE_COLLAPSE_MIN", "4000000000000", dict(tile_min=4000000000000)), ("TILE_COLLAPSE_MIN", "-1", dict(tile_min=2 ** 64 - 1)),
    ("TOP_CAP", "", dict(top_cap=0)), ("TOP_CAP", "0", dict(top_cap=0)), ("TOP_CAP", "1", dict(top_cap=1)), ("TOP_CAP", "-1", dict(top_cap=0xffffffff)),
    ("NODE_ESTIMATE_DIV", "", {}), ("NODE_ESTIMATE_DIV", "0", {}), ("NODE_ESTIMATE_DIV", "1", dict(est_div=1)), ("NODE_ESTIMATE_DIV", "-3", dict(est_div=-3)),
    ("NODE_ESTIMATE_DIV", "1000000", dict(est_div=1000000)),
    # the cost constants: the empty string is the default, 0 is 0
    ("SAH_CN", "", {}), ("SAH_CN", "0", dict(cost_node=0.0)), ("SAH_CN", "1", dict(cost_node=1.0)), ("SAH_CN", "0.25", dict(cost_node=0.25)), ("SAH_CN", "1e6", dict(cost_node=1e6)),
    ("SAH_CT", "", {}), ("SAH_CT", "0", dict(cost_tri=0.0)), ("SAH_CT", "1", {}), ("SAH_CT", "2.5", dict(cost_tri=2.5)),
]
# "set it to 0 to turn it off": off for 0 and, as it has always been, for the empty string and for anything that does not read as a number
UNLESS_ZERO = dict(SORT_PACKED="sort_packed", BUILD_DIRECT="direct", FUSED_EMIT="fused_emit", KEEP_WORKSPACE="keep_workspace", KEY_REBUILD="key_rebuild")
KNOB_CASES += [(var, text, {} if on else {field: 0}) for var, field in UNLESS_ZERO.items() for text, on in (("", 0), ("0", 0), ("1", 1), ("2", 1), ("-1", 1), ("off", 0), ("00", 0))]


@pytest.mark.parametrize("var,text,changed", KNOB_CASES, ids=["%s=%s" % (v, t or "empty") for v, t, _ in KNOB_CASES])
def test_knob(driver, var, text, changed):
    assert var in KNOB_VARS
    assert knobs(driver, {var: text}) == want_knobs(**changed)


def test_every_variable_has_cases():
    for var in KNOB_VARS:
        assert {"", "0", "1"} <= {t for v, t, _ in KNOB_CASES if v == var}, var


def test_build_direct_is_read_once_per_process(driver):
    """... and every other variable per build"""
    got = run(driver, ["knobs", "setenv RTK_AMD_BUILD_DIRECT 0", "setenv RTK_AMD_FUSED_EMIT 0", "setenv RTK_AMD_MAX_LEAF 5", "knobs"])
    first, second = (dict(w.split("=") for w in words) for words in (got[0], got[4]))
    assert (first["direct"], first["fused_emit"], first["max_leaf"]) == ("1", "1", "3")
    assert (second["direct"], second["fused_emit"], second["max_leaf"]) == ("1", "0", "5")
    got = run(driver, ["knobs", "setenv RTK_AMD_BUILD_DIRECT 1", "knobs"], {"RTK_AMD_BUILD_DIRECT": "0"})
    assert [dict(w.split("=") for w in words)["direct"] for words in (got[0], got[2])] == ["0", "0"]
