"""The owner of a scene's launch scratch (rtk_amd/csrc/rtk_launch_scratch.h), checked without a GPU: tests/launch_scratch_driver.cpp
is built by the host compiler against that header alone, with -fsanitize=address,undefined, and runs lists of commands with
malloc / free as the allocator and a counting "wait for the stream". What is expected is a model kept here: the sets by stream,
each buffer's capacity, and what every command makes the hooks do, in order. The run ends clean under the address sanitizer
with leak detection on: nothing a set was given is leaked or freed twice."""
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_OOM = 0, -3
BUFFERS = ("sort", "entries", "leftover", "select")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("launch_scratch") / "launch_scratch_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "rtk_amd", "csrc"),
                           os.path.join(ROOT, "tests", "launch_scratch_driver.cpp"), "-o", exe])
    return exe


def run(driver, commands):
    """[(ret, nonnull, capacity, entries, events, allocs, frees, waits, pinned_frees)] of the commands, from one clean run"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([driver], input="".join(c + "\n" for c in commands), capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-4000:]
    out = []
    for line in r.stdout.splitlines():
        w = line.split()
        out.append(tuple(int(x) for x in w[:4]) + (w[4],) + tuple(int(x) for x in w[5:]))
    assert len(out) == len(commands)
    return out


class Model:
    """What the header has to do, written down independently: sets by stream in the order they were made; of each buffer
    whether it holds memory and its capacity; the hooks' calls of each command as a string (w f a c p)."""

    def __init__(self):
        self.fail = False
        self.allocs = self.frees = self.waits = self.pinned = 0
        self.made = 0
        self.sets = {}      # stream -> dict(number, verdict, entries, bufs = {name: [held, capacity]})

    def _grow(self, buf, need):
        ev = ""
        if buf[1] >= need:
            return OK, ev
        if buf[0]:
            ev += "wf"
            self.waits += 1
            self.frees += 1
        buf[0], buf[1] = False, 0
        ev += "a"
        self.allocs += 1
        if self.fail:
            return ERR_OOM, ev
        buf[0], buf[1] = True, need
        return OK, ev

    def _free_set(self, s):
        ev = "f"                                                    # the counter words
        self.frees += 1
        if s["verdict"]:
            ev += "p"
            self.pinned += 1
        for name in ("spill",) + BUFFERS:
            if s["bufs"][name][0]:
                ev += "f"
                self.frees += 1
        return ev

    def step(self, command):
        w = command.split()
        ret, named, entries, ev = 0, None, 0, ""
        if w[0] == "new":
            for s in sorted(self.sets.values(), key=lambda s: s["number"]):
                ev += self._free_set(s)
            self.sets = {}
        elif w[0] == "fail":
            self.fail = w[1] != "0"
        elif w[0] == "get":
            s = self.sets.get(w[1])
            if s is None:
                ev += "c"
                if not self.fail:
                    s = self.sets[w[1]] = dict(number=self.made, verdict=False, entries=0, bufs={n: [False, 0] for n in ("spill",) + BUFFERS})
                    self.made += 1
            ret = s["number"] if s else -1
        elif w[0] == "find":
            ret = self.sets[w[1]]["number"] if w[1] in self.sets else -1
        elif w[0] == "drop":
            if w[1] in self.sets:
                ev += self._free_set(self.sets.pop(w[1]))
        elif w[0] == "verdict":
            self.sets[w[1]]["verdict"] = True
        elif w[0] == "grow":
            named = self.sets[w[1]]["bufs"][w[2]]
            ret, ev = self._grow(named, int(w[3]))
        elif w[0] == "spill":
            s = self.sets[w[1]]
            named, lanes, per_lane = s["bufs"]["spill"], int(w[2]), int(w[3])
            if not (named[1] >= lanes and s["entries"] >= per_lane):
                named[1] = s["entries"] = 0
                ret, ev = self._grow(named, lanes)
                if ret == OK:
                    s["entries"] = per_lane
            entries = s["entries"]
        return (ret, int(named[0]) if named else 0, named[1] if named else 0, entries, ev or "-", self.allocs, self.frees, self.waits, self.pinned)


def check(driver, commands):
    model = Model()
    expect = [model.step(c) for c in commands]
    got = run(driver, commands + ["new"])[:-1]          # (the last `new` empties the collection: the run ends without a leak)
    assert got == expect
    return got


def test_header_includes_no_hip():
    includes = [l.split()[1] for l in open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_launch_scratch.h")) if l.startswith("#include")]
    assert includes == ['"rtk_amd.h"', "<stddef.h>", "<stdint.h>", "<vector>"]


def test_grow_keeps_waits_frees_allocates_in_that_order(driver):
    got = check(driver, ["get 1", "grow 1 sort 100 1600", "grow 1 sort 100 1600", "grow 1 sort 7 112", "grow 1 sort 101 1616", "grow 1 leftover 0 0",
                         "grow 1 leftover 64 64", "grow 1 entries 3 1536", "grow 1 select 10 10", "grow 1 select 11 11"])
    ev = [g[4] for g in got]
    assert ev[1] == "a"                                   # a first grow with no old area: no wait
    assert ev[2] == "-" and ev[3] == "-"                  # enough capacity: no allocation, no wait
    assert ev[4] == "wfa" and got[4][2] == 101            # over an old area: one wait, then one free, then one allocation
    assert ev[5] == "-" and got[5][1:3] == (0, 0)         # nothing needed: nothing made
    assert ev[6] == "a" and ev[9] == "wfa"
    assert got[-1][5:8] == (6, 2, 2)


def test_a_failing_allocator_leaves_the_buffer_empty(driver):
    got = check(driver, ["get 1", "grow 1 sort 10 160", "fail 1", "grow 1 sort 20 320", "grow 1 sort 5 80", "fail 0", "grow 1 sort 5 80", "grow 1 sort 5 80",
                         "fail 1", "spill 1 256 4", "fail 0", "spill 1 256 4"])
    assert got[3][:5] == (ERR_OOM, 0, 0, 0, "wfa")        # the old area is gone, nothing took its place
    assert got[4][:5] == (ERR_OOM, 0, 0, 0, "a")          # capacity 0: even a smaller need asks the allocator again
    assert got[6][:5] == (OK, 1, 5, 0, "a") and got[7][4] == "-"
    assert got[9][:5] == (ERR_OOM, 0, 0, 0, "a") and got[11][:5] == (OK, 1, 256, 4, "a")


def test_the_spill_pair_is_remade_when_either_measure_is_short(driver):
    got = check(driver, ["get 1", "spill 1 512 6", "spill 1 512 6", "spill 1 256 3", "spill 1 513 6", "spill 1 513 2", "spill 1 100 7", "spill 1 100 7",
                         "spill 1 101 7", "spill 1 101 8"])
    assert [g[4] for g in got[1:]] == ["a", "-", "-", "wfa", "-", "wfa", "-", "wfa", "wfa"]
    assert [g[2:4] for g in got[1:]] == [(512, 6), (512, 6), (512, 6), (513, 6), (513, 6), (100, 7), (100, 7), (101, 7), (101, 8)]


def test_sets_by_stream(driver):
    got = check(driver, ["find 1", "get 1", "get 1", "get 2", "find 2", "find 3", "get 0", "grow 1 sort 4 64", "grow 2 sort 4 64", "grow 2 select 8 8",
                         "spill 2 64 2", "verdict 2", "grow 0 entries 1 512", "drop 2", "find 2", "find 1", "find 0", "drop 2", "get 2", "drop 3", "new", "find 1"])
    assert [g[0] for g in got[:7]] == [-1, 0, 0, 1, 1, -1, 2]        # twice the same set, another stream another set; NULL is a stream
    assert got[13][4] == "fpfff" and got[13][6] - got[12][6] == 4 and got[13][8] == 1      # counter words, verdict, spill, sort, select: each once
    assert [g[0] for g in got[14:17]] == [-1, 0, 2] and got[17][4] == "-"
    assert got[18][0] == 3 and got[18][4] == "c"                     # a set of its own again, with nothing of the old one
    assert got[20][4] == "fffff" and got[21][0] == -1                # destruction: the counter words of three sets, one sort, one entry list


def test_a_set_whose_counter_words_cannot_be_had_is_not_entered(driver):
    got = check(driver, ["fail 1", "get 5", "find 5", "fail 0", "find 5", "get 5", "find 5"])
    assert [g[0] for g in got] == [0, -1, -1, 0, -1, 0, 0] and got[1][4] == "c" and got[5][4] == "c"


def test_random_commands_against_the_model(driver):
    rng = random.Random(20240)
    commands, live = [], set()
    for _ in range(3000):
        s = rng.randrange(4)
        k = rng.random()
        if k < 0.02:
            commands.append("new")
            live.clear()
        elif k < 0.08:
            commands.append("fail %d" % rng.randrange(2))
        elif k < 0.2 or s not in live:
            commands += ["fail 0", "get %d" % s]
            live.add(s)
        elif k < 0.25:
            commands.append("drop %d" % s)
            live.discard(s)
        elif k < 0.3:
            commands.append("find %d" % rng.randrange(5))
        elif k < 0.75:
            need = rng.randrange(0, 40)
            commands.append("grow %d %s %d %d" % (s, rng.choice(BUFFERS), need, need * 16))
        else:
            commands.append("spill %d %d %d" % (s, 64 * rng.randrange(1, 5), rng.randrange(1, 5)))
    check(driver, commands)


def test_leak_detection_is_on(driver):
    """The proof rests on it: memory nobody frees (the driver's `leak`) fails the run."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([driver], input="leak\n", capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode != 0 and "LeakSanitizer" in r.stderr
