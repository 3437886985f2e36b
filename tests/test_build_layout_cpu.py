"""Where the temporaries of a device build lie in the build workspace (rtk_amd/csrc/rtk_build_layout.h), checked without a GPU:
tests/build_layout_driver.cpp is built by the host compiler against that header alone and answers a table of cases.

What is expected was written down by reading the build as it was before the carve (rtk_dev_scene_build's `need` sum and its
sequence of Arena::take calls), not by running the new code: every buffer's extent is its element size times its count, the
buffers follow one another in the order they were taken, each on a 256-byte step, and the whole is never larger than the old
`need`. In tile mode the n-node region is shared by five pieces (the nodes above the tiles, their tile-root and level words,
a word per binary node, the tiles' root lists) that must not overlap and must end inside n * sizeof(DevNode)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZEOF = dict(InTri=48, BinNode=32, Climb=12, LevelState=32, MeshSrc=16, DevNode=128)
REFIT_TILE, COLLAPSE_BLOCK, COLLAPSE_RING = 1024, 256, 64
SIZES = [0, 1, 255, 256, 257, 12 * 10 ** 6]
# (index bytes, position bytes) of every mesh: none, one mesh with every size in either place, three meshes
MESH_SETS = [[]] + [[(SIZES[k], SIZES[(k + 1) % 6])] for k in range(6)] + [[(0, 1), (255, 256), (257, 12 * 10 ** 6)], [(12 * 10 ** 6, 0), (256, 255), (1, 257)]]
NS = [2, 3, 1023, 1024, 1025, 4096, 4097, 2 ** 24 - 1, 2 ** 24, 0x3fffffef]
CASES = [(n, packed, tile_mode, top_cap) for n in NS for packed in (1, 0) for tile_mode in ((0, 1) if n >= 1025 else (0,)) for top_cap in (n // 2, 2)]


def sort_words(n):
    """rtk_sort_scratch_words: 256 histogram words per 4096 keys, one sum per 4096 of those, 16 more"""
    hist = 256 * ((n + 4095) // 4096)
    return hist + (hist + 4095) // 4096 + 16


def padded(b):
    return ((b if b else 1) + 255) & ~255


def need_before(n, meshes):
    """The workspace size rtk_dev_scene_build asked for before the carve (its `need`), term by term. A mesh contributed its two
    padded upload sizes if it reached the device decode at all; one that uploads nothing is counted as if it had not (the smaller sum)."""
    m1 = len(meshes) + 1
    need = sum(padded(p) + padded(i) for i, p in meshes if i or p) + 64 * 256
    need += padded(n * SIZEOF["InTri"]) + padded(n * 12) + padded(m1 * SIZEOF["MeshSrc"])
    need += 2 * padded(n * 8) + 2 * padded(n * 4)
    need += padded(sort_words(n) * 4) + padded(64) + padded(m1 * 8)
    need += 2 * padded(n * 8) + padded(n * 12) + padded(n * 16) + padded(n * 4) + padded(16)
    need += padded(n * SIZEOF["BinNode"])
    need += padded(n * 16) + 2 * padded(n * 4) + padded((n + COLLAPSE_BLOCK - 1) // COLLAPSE_BLOCK * 4) + padded(SIZEOF["LevelState"] * COLLAPSE_RING)
    need += padded(n * SIZEOF["DevNode"])
    need += 4 * padded((n // REFIT_TILE + 4) * 4) + padded(16) + padded(n * 4)
    return need


def extents(n, packed, tile_mode, meshes):
    """(name, bytes) of every buffer a build takes, in the order it took them; bytes = element size x count"""
    tiles1 = (n + REFIT_TILE - 1) // REFIT_TILE + 1
    out = [("in_tris", SIZEOF["InTri"] * n), ("cent", 4 * 3 * n), ("bounds", 4 * 16)]
    for m, (i, p) in enumerate(meshes):
        out += [("idx%d" % m, i)] * bool(i) + [("pos%d" % m, p)] * bool(p)
    out += [("keys_a", 8 * n), ("keys_b", 8 * n)]
    if not packed:
        out += [("vals_a", 4 * n), ("vals_b", 4 * n)]
    out += [("sort_scratch", 4 * sort_words(n)), ("mesh_src", SIZEOF["MeshSrc"] * (len(meshes) + 1))]
    out += [("lr", 8 * n), ("range", 8 * n), ("climbers", SIZEOF["Climb"] * n), ("half", 8 * 2 * n), ("arrive", 4 * n), ("root", 4 * 4), ("bin", SIZEOF["BinNode"] * n)]
    out += [("tile_count", 4 * tiles1), ("tile_base", 4 * tiles1), ("depth_word", 4 * 4)]
    if tile_mode:
        out += [("area", 4 * n)]
    out += [("tile_nclimb", 4 * tiles1), ("nodes_tmp", SIZEOF["DevNode"] * n), ("tile_nroots", 4 * tiles1)]
    out += [("jobs", 4 * n), ("dec", 16 * n), ("info", 4 * n), ("sums", 4 * ((n + COLLAPSE_BLOCK - 1) // COLLAPSE_BLOCK)), ("ring", SIZEOF["LevelState"] * COLLAPSE_RING)]
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """The driver built against the header only (no HIP include path, -Wall -Werror)."""
    exe = str(tmp_path_factory.mktemp("build_layout") / "build_layout_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "rtk_amd", "csrc"),
                           os.path.join(ROOT, "tests", "build_layout_driver.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def answers(driver):
    """The driver run once over all cases."""
    exe = driver
    keys = [case + (k,) for case in CASES for k in range(len(MESH_SETS))]
    text = "".join("%d %d %d %d %d %d %s\n" % (n, packed, tile_mode, top_cap, sort_words(n), len(MESH_SETS[k]), " ".join("%d %d" % ip for ip in MESH_SETS[k]))
                   for n, packed, tile_mode, top_cap, k in keys)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(keys)
    return {key: {k: int(v) for k, v in (w.split("=") for w in line.split())} for key, line in zip(keys, lines)}


def test_layout_header_includes_no_hip():
    includes = [l.split()[1] for l in open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_build_layout.h")) if l.startswith("#include")]
    assert includes == ["<stddef.h>", "<stdint.h>", "<vector>"]


def test_the_header_and_the_test_agree_on_the_sizes():
    text = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_build_layout.h")).read()
    for name, size in SIZEOF.items():
        assert "#define RTK_BUILD_SIZEOF_%s %du" % (name.upper(), size) in text
    for name, value in (("REFIT_TILE", REFIT_TILE), ("COLLAPSE_BLOCK", COLLAPSE_BLOCK), ("COLLAPSE_RING", COLLAPSE_RING)):
        assert "#define RTK_BUILD_%s %du" % (name, value) in text


@pytest.mark.parametrize("n,packed,tile_mode,top_cap", CASES, ids=["n%d-%s-%s-cap%d" % (n, "packed" if p else "pairs", "tiles" if t else "levels", c) for n, p, t, c in CASES])
def test_layout(answers, n, packed, tile_mode, top_cap):
    for k, meshes in enumerate(MESH_SETS):
        got = answers[(n, packed, tile_mode, top_cap, k)]
        assert got["ok"] == 1
        total = got["bytes"]
        bufs = extents(n, packed, tile_mode, meshes)
        # every buffer the build has is placed, the others are not
        absent = (set(["vals_a", "vals_b"]) if packed else set()) | (set() if tile_mode else set(["area", "top_refs", "top_level", "root_info", "root_list"]))
        absent |= {"idx%d" % m for m, (i, p) in enumerate(meshes) if not i} | {"pos%d" % m for m, (i, p) in enumerate(meshes) if not p}
        assert {name for name, off in got.items() if off == -1} == absent
        # on 256-byte steps, in the order the build took them, none reaching into the next, all inside `bytes`: with the extents
        # in Python's integers, so that a sum cut to 32 bits in the header would show (48 n alone is past 2^35 at the top size)
        end = 0
        for name, size in bufs:
            off = got[name]
            assert off % 256 == 0, name
            assert off >= end, name
            end = off + size
        assert end <= total
        assert total >= sum(size for _, size in bufs)
        assert total <= need_before(n, meshes)
        if tile_mode:
            base, region = got["nodes_tmp"], SIZEOF["DevNode"] * n
            pieces = [("nodes_tmp", SIZEOF["DevNode"] * top_cap, 128), ("top_refs", 16 * top_cap, 16), ("top_level", 4 * top_cap, 4), ("root_info", 8 * n, 256), ("root_list", 4 * n, 4)]
            end = base
            for name, size, align in pieces:
                assert got[name] % align == 0 and got[name] >= end, name
                end = got[name] + size
            assert end <= base + region


def test_a_top_capacity_the_region_cannot_hold_is_refused(driver):
    """More nodes above the tiles than n / 2: the five pieces would not fit n nodes' worth of workspace, and the carve says so."""
    r = subprocess.run([driver], input="4097 1 1 4000 %d 0\n4097 1 1 2048 %d 0\n" % (sort_words(4097), sort_words(4097)), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert [line.split()[0] for line in r.stdout.splitlines()] == ["ok=0", "ok=1"]
