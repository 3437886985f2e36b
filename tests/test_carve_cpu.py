"""Tables that share one allocation (rtk_amd/csrc/rtk_carve.h), checked without a GPU: tests/carve_driver.cpp is built by the host
compiler against that header alone, with -fsanitize=address,undefined, and carves the lists of piece sizes it reads. What is
expected is a model kept here: the chains of padded sizes as the sites wrote them out by hand before the header existed (every
piece on a 256-byte step, a piece of 0 bytes still one step), and the sums the ledger was given beside them."""
import itertools
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [0, 1, 4, 255, 256, 257, 4096, 3 << 30]
NODES = [1, 2, 63, 64, 65, 1023, 1024, 1025, 10000]


def padded(b):
    return ((b or 1) + 255) & ~255


def model(pieces):
    """offsets, bytes, counted: offset k is the sum of the padded sizes before it"""
    offsets, at = [], 0
    for p in pieces:
        offsets.append(at)
        at += padded(p)
    return offsets + [at, sum(pieces)]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("carve") / "carve_driver")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "rtk_amd", "csrc"), os.path.join(ROOT, "tests", "carve_driver.cpp"), "-o", exe])
    return exe


def carve(driver, lists):
    """[offsets + [bytes, counted]] of the lists, from one clean run of the driver"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([driver], input="".join(" ".join(str(p) for p in l) + "\n" for l in lists), capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-4000:]
    out = [[int(w) for w in line.split()] for line in r.stdout.splitlines()]
    assert len(out) == len(lists)
    return out


def test_header_includes_no_hip():
    includes = [l.split()[1] for l in open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_carve.h")) if l.startswith("#include")]
    assert includes == ["<stddef.h>"]


def test_piece_lists(driver):
    """Lengths 0 to 8 over SIZES: every list up to length 3, every list of one repeated size, and 300 drawn ones per longer length."""
    rng = random.Random(1)
    lists = [list(l) for n in range(4) for l in itertools.product(SIZES, repeat=n)]
    for n in range(4, 9):
        lists += [[s] * n for s in SIZES]
        lists += [[rng.choice(SIZES) for _ in range(n)] for _ in range(300)]
    got = carve(driver, lists)
    for l, g in zip(lists, got):
        assert g == model(l), l
    assert got[0] == [0, 0]                                    # no piece: nothing to allocate
    assert carve(driver, [[0], [0, 0]]) == [[0, 256, 0], [0, 256, 512, 0]]      # a piece of 0 bytes still takes one step


@pytest.mark.parametrize("sort_words", [0, 1, 1024, 65537])
def test_refit_schedule(driver, sort_words):
    """The six temporaries of a refit's schedule (heights, the changed word, two key arrays, the sort's scratch, level starts) lie
    where schedule_tmp put them when it summed the padded sizes itself."""
    lists = [[n * 4, 4, n * 8, n * 8, sort_words * 4, (n + 2) * 4] for n in NODES]
    for n, g in zip(NODES, carve(driver, lists)):
        o_changed = padded(n * 4)
        o_ka = o_changed + padded(4)
        o_kb = o_ka + padded(n * 8)
        o_sort = o_kb + padded(n * 8)
        o_ls = o_sort + padded(sort_words * 4)
        total = o_ls + padded((n + 2) * 4)
        assert g[:7] == [0, o_changed, o_ka, o_kb, o_sort, o_ls, total], n


@pytest.mark.parametrize("heights,meshes", [(1, 1), (7, 3), (40, 1000)])
def test_partial_refit_tables(driver, heights, meshes):
    """The eight tables of a refit of some meshes, nt = 3 n triangles: the offsets as make_partial_tables summed them, and counted
    as it typed the sum for the ledger: n * 12 + nt * 8 + (nb + 1) * 4 + (heights + 1) * 4 + (meshes + 1) * sizeof(RefitRange)."""
    range_bytes, dirty_block = 8, 1024
    lists = []
    for n in NODES:
        nt, nb = 3 * n, (n + dirty_block - 1) // dirty_block
        lists.append([n * 4, nt * 4, nt * 4, n * 4, n * 4, (nb + 1) * 4, (heights + 1) * 4, (meshes + 1) * range_bytes])
    for n, g in zip(NODES, carve(driver, lists)):
        nt, nb = 3 * n, (n + dirty_block - 1) // dirty_block
        o_slot_node = padded(n * 4)
        o_mesh_slots = o_slot_node + padded(nt * 4)
        o_dirty = o_mesh_slots + padded(nt * 4)
        o_list = o_dirty + padded(n * 4)
        o_block = o_list + padded(n * 4)
        o_list_start = o_block + padded((nb + 1) * 4)
        o_ranges = o_list_start + padded((heights + 1) * 4)
        total = o_ranges + padded((meshes + 1) * range_bytes)
        assert g[:9] == [0, o_slot_node, o_mesh_slots, o_dirty, o_list, o_block, o_list_start, o_ranges, total], n
        assert g[9] == n * 12 + nt * 8 + (nb + 1) * 4 + (heights + 1) * 4 + (meshes + 1) * range_bytes, n
