"""The ledger of a scene's device allocations (rtk_amd/csrc/rtk_scene_mem.h), checked without a GPU: tests/scene_mem_driver.cpp
is built by the host compiler against that header alone, with -fsanitize=address,undefined, and runs lists of commands with
malloc / free as the allocator. What is expected is a model kept here: the live entries and their counted figures. The run
ends clean under the address sanitizer with leak detection on: nothing the ledger was given is leaked or freed twice."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (allocated, counted) of six entries: equal, counted 0 (the constants block), more allocated than counted, nothing allocated
SIZES = [(128, 128), (16, 0), (256, 200), (1, 1), (4096, 4095), (0, 7)]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("scene_mem") / "scene_mem_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "rtk_amd", "csrc"), os.path.join(ROOT, "tests", "scene_mem_driver.cpp"), "-o", exe])
    return exe


def run(driver, commands):
    """[(ret, counted, allocs, frees)] of the commands, from one clean run of the driver"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([driver], input="".join(c + "\n" for c in commands), capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-4000:]
    out = [tuple(int(w) for w in line.split()) for line in r.stdout.splitlines()]
    assert len(out) == len(commands)
    return out


def test_header_includes_no_hip():
    includes = [l.split()[1] for l in open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_scene_mem.h")) if l.startswith("#include")]
    assert includes == ["<stddef.h>", "<stdint.h>", "<mutex>", "<vector>"]


def test_own_then_release_in_every_order(driver):
    """1 to 6 entries, every order of giving them back: after every step counted() is the sum over the live entries, every
    release finds its entry, and each pointer is freed exactly once."""
    commands, expect = [], []
    allocs = frees = 0
    for n in range(1, 7):
        for order in itertools.permutations(range(n)):
            commands.append("new")
            expect.append((0, 0, allocs, frees))
            live = {}
            for k in range(n):
                commands.append("own %d %d" % SIZES[k])
                allocs += 1
                live[k] = SIZES[k][1]
                expect.append((k, sum(live.values()), allocs, frees))
            for k in order:
                commands.append("release %d" % k)
                frees += 1
                del live[k]
                expect.append((1, sum(live.values()), allocs, frees))
    assert run(driver, commands) == expect


def test_release_of_what_is_not_owned_changes_nothing(driver):
    got = run(driver, ["own 64 64", "own 32 10", "foreign", "release null", "release 2", "release 0", "release 0", "counted", "release 1", "release 1", "release null"])
    assert got == [(0, 64, 1, 0), (1, 74, 2, 0), (2, 74, 2, 0),
                   (0, 74, 2, 0), (0, 74, 2, 0),                # NULL, a pointer of somebody else's
                   (1, 10, 2, 1), (0, 10, 2, 1), (0, 10, 2, 1),  # the second release of the same pointer
                   (1, 0, 2, 2), (0, 0, 2, 2), (0, 0, 2, 2)]


def test_a_failing_allocator_records_nothing(driver):
    got = run(driver, ["own 64 64", "fail 1", "own 128 128", "counted", "release_all", "fail 0", "own 8 8", "release 2"])
    assert got == [(0, 64, 1, 0), (0, 64, 1, 0), (-1, 64, 2, 0), (0, 64, 2, 0), (0, 0, 2, 1), (0, 0, 2, 1), (2, 8, 3, 1), (1, 0, 3, 2)]


def test_adopt_then_release(driver):
    # (adopted memory is not the allocator's call, but it is the ledger's to free)
    got = run(driver, ["adopt 100 40", "own 10 10", "release 0", "release 0", "adopt 50 0", "counted", "release 2", "release 1"])
    assert got == [(0, 40, 0, 0), (1, 50, 1, 0), (1, 10, 1, 1), (0, 10, 1, 1), (2, 10, 1, 1), (0, 10, 1, 1), (1, 10, 1, 2), (1, 0, 1, 3)]


def test_release_all_twice_and_the_destructor(driver):
    got = run(driver, ["own 64 64", "adopt 8 3", "own 16 0", "release_all", "release_all", "release 0", "own 5 5", "adopt 6 6", "new", "counted"])
    assert got == [(0, 64, 1, 0), (1, 67, 1, 0), (2, 67, 2, 0), (0, 0, 2, 3), (0, 0, 2, 3), (0, 0, 2, 3),
                   (3, 5, 3, 3), (4, 11, 3, 3), (0, 0, 3, 5), (0, 0, 3, 5)]       # (a ledger that goes away frees what it still has)


def test_counted_zero_and_counted_apart_from_allocated(driver):
    got = run(driver, ["own 16 0", "counted", "own 4096 100", "own 100 4096", "release 0", "release 2", "release 1"])
    assert got == [(0, 0, 1, 0), (0, 0, 1, 0), (1, 100, 2, 0), (2, 4196, 3, 0), (1, 4196, 3, 1), (1, 100, 3, 2), (1, 0, 3, 3)]


def test_leak_detection_is_on(driver):
    """The proof rests on it: an entry taken out of the ledger's hands without being freed (the driver's `leak`) fails the run."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([driver], input="leak\n", capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode != 0 and "LeakSanitizer" in r.stderr
