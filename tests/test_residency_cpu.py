"""The residency cache of the host-pointer calls (rtk_amd/csrc/rtk_residency.h), checked without a GPU: tests/residency_driver.cpp
is built by the host compiler against that header alone, with -fsanitize=address,undefined, and runs lists of commands with
malloc / free of a numbered dummy as "upload" and "free a device copy". Blobs are allocated at exactly their size: a hash that
reads past the end of one fails the run. What is expected is a model kept here, with the hashes recomputed in Python (64-bit
masks): which copy every lookup answers with, what was made and freed by each command. The run ends clean with leak detection on."""
import os
import re
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
STRIPE = 4096
HEADER = 56                     # sizeof(rtk_scene); size_in_bytes is its u64 at offset 24
SIZES = [64, 255, 256, 4095, 4096, 4097, 3 * 4096 + 5, 3 * 4096 + 8]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("residency") / "residency_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "rtk_amd", "csrc"),
                           os.path.join(ROOT, "tests", "residency_driver.cpp"), "-o", exe])
    return exe


def run(driver, commands):
    """[(ret, made, freed, sorted events)] of the commands, from one clean run"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([driver], input="".join(c + "\n" for c in commands), capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-4000:]
    out = []
    for line in r.stdout.splitlines():
        w = line.split()
        out.append((int(w[0]), int(w[1]), int(w[2]), sorted(re.findall(r"u|[fv]\d+", w[3]))))
    assert len(out) == len(commands)
    return out


def hash_words(data, h):
    n8 = len(data) // 8
    for (w,) in struct.iter_unpack("<Q", bytes(data[:n8 * 8])):
        h = ((h ^ w) * 0x9e3779b97f4a7c15) & M64
        h ^= h >> 29
    for b in data[n8 * 8:]:
        h = ((h ^ b) * 0x100000001b3) & M64
    return h


class Model:
    """What the header has to do, written down independently. Entries by (blob, device): the copy's number, the size, the head
    hash, the stripe hashes and which stripe the next lookup re-checks. (Maps are not ordered: events are compared sorted.)"""

    def __init__(self):
        self.blobs, self.entries = {}, {}
        self.made = self.freed = 0
        self.fail = False

    @staticmethod
    def size_of(blob):
        return struct.unpack_from("<Q", blob, 24)[0]

    def head(self, blob):
        h = hash_words(blob[:HEADER], 0xcbf29ce484222325)
        return hash_words(blob[128:256], h) if 256 <= self.size_of(blob) <= 1 << 48 else h

    def stripe(self, blob, size, k):
        return hash_words(blob[k * STRIPE:min((k + 1) * STRIPE, size)], k * STRIPE)

    def fill(self, key, number):
        blob = self.blobs[key[0]]
        size = self.size_of(blob)
        stripes = [self.stripe(blob, size, k) for k in range((size + STRIPE - 1) // STRIPE)] if 256 <= size <= 1 << 48 else []
        self.entries[key] = dict(number=number, size=size, head=self.head(blob), stripes=stripes, next=0)

    def drop_address(self, b):
        ev = []
        for key in [k for k in self.entries if k[0] == b]:
            ev.append("f%d" % self.entries.pop(key)["number"])
            self.freed += 1
        return ev

    def step(self, command):
        w = command.split()
        cmd, b = w[0], int(w[1]) if len(w) > 1 else 0
        x, y = (int(w[2]) if len(w) > 2 else 0), (int(w[3]) if len(w) > 3 else 0)
        ret, ev = 0, []
        if cmd == "blob":
            blob = bytearray((i * 131 + y * 31 + (i >> 8)) & 255 for i in range(x))
            struct.pack_into("<Q", blob, 24, x)
            self.blobs[b] = blob
        elif cmd == "poke":
            self.blobs[b][x] = y
        elif cmd == "setsize":
            struct.pack_into("<Q", self.blobs[b], 24, x)
        elif cmd == "lookup":
            blob, key = self.blobs[b], (b, x)
            e = self.entries.get(key)
            if e is not None:
                same = e["size"] == self.size_of(blob) and e["head"] == self.head(blob)
                if same and e["stripes"]:
                    k = e["next"]
                    e["next"] = (k + 1) % len(e["stripes"])
                    same = self.stripe(blob, e["size"], k) == e["stripes"][k]
                if same:
                    return (e["number"], self.made, self.freed, [])
                ev.append("f%d" % e["number"])
                self.freed += 1
                del self.entries[key]
            ev.append("u")
            ret = -1
            if not self.fail:
                ret = self.made
                self.made += 1
                self.fill(key, ret)
        elif cmd == "adopt":
            ret = self.made
            self.made += 1
            ev += self.drop_address(b)
            self.fill((b, x), ret)
        elif cmd == "forget":
            ev += self.drop_address(b)
        elif cmd == "each":
            ev += ["v%d" % e["number"] for e in self.entries.values()]
            ret = len(ev)
        elif cmd == "fail":
            self.fail = b != 0
        elif cmd == "unblob":
            del self.blobs[b]
        return (ret, self.made, self.freed, sorted(ev))


def check(driver, commands):
    model = Model()
    expect = [model.step(c) for c in commands]
    tidy = ["forget %d" % b for b in model.blobs] + ["unblob %d" % b for b in model.blobs]     # the run ends without a leak
    got = run(driver, commands + tidy)[:len(commands)]
    assert got == expect
    return got


def test_header_includes_no_hip():
    includes = [l.split()[1] for l in open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_residency.h")) if l.startswith("#include")]
    assert includes == ['"rtk.h"', "<string.h>", "<algorithm>", "<functional>", "<mutex>", "<unordered_map>", "<vector>"]


@pytest.mark.parametrize("size", SIZES)
def test_an_edit_in_stripe_j_is_noticed_on_lookup_j_of_the_rotation(driver, size):
    """Lookups are counted from the fill; lookup number i re-checks stripe i mod (number of stripes). A byte that only its stripe
    covers (outside header and root node) is edited right after a fill and, wrapping, some lookups into the rotation."""
    stripes = (size + STRIPE - 1) // STRIPE if size >= 256 else 0
    flipped = lambda offset: ((offset * 131 + 7 * 31 + (offset >> 8)) & 255) ^ 255
    if not stripes:                                     # header only: nothing behind the header is looked at, or read
        got = check(driver, ["blob 1 %d 7" % size, "lookup 1 0", "poke 1 60 %d" % flipped(60), "lookup 1 0", "lookup 1 0"])
        assert [g[0] for g in got[3:]] == [0, 0] and got[-1][1:3] == (1, 0)
    for j in range(stripes):
        # stripe 0: between the header and the root node; the last stripe: its last byte (of a tail of 1, 5 or 8 bytes)
        offset = 60 if j == 0 else size - 1 if j == stripes - 1 else j * STRIPE + 300
        assert j * STRIPE <= offset < min((j + 1) * STRIPE, size) and not (offset < HEADER or 128 <= offset < 256)
        for before in (0, j + 1, stripes + 2):          # lookups already done since the fill when the byte changes
            commands = ["blob 1 %d 7" % size, "lookup 1 0"] + ["lookup 1 0"] * before + ["poke 1 %d %d" % (offset, flipped(offset))]
            wait = (j - before) % stripes               # further lookups that still answer with the old copy
            commands += ["lookup 1 0"] * (wait + 2)
            got = check(driver, commands)
            answers = [g[0] for g in got[3 + before:]]
            assert answers == [0] * wait + [1, 1], (size, j, before, answers)
            assert got[3 + before + wait][3] == ["f0", "u"]          # the old copy freed exactly once, a new one made
            assert got[-1][1:3] == (2, 1)


@pytest.mark.parametrize("size", SIZES)
def test_header_root_and_size_are_checked_on_every_lookup(driver, size):
    commands = ["blob 1 %d 3" % size, "lookup 1 0", "lookup 1 0", "poke 1 9 200", "lookup 1 0", "lookup 1 0"]      # a header byte
    expect = [0, 0, 1, 1]
    if size >= 256:
        commands += ["lookup 1 0", "poke 1 255 200", "lookup 1 0", "poke 1 128 201", "lookup 1 0", "lookup 1 0"]   # the root's last and first byte
        expect += [1, 2, 3, 3]
    last = expect[-1]
    commands += ["setsize 1 %d" % (size - 1), "lookup 1 0", "lookup 1 0", "setsize 1 %d" % size, "lookup 1 0"]     # (255: the root is no longer hashed, nor read)
    expect += [last + 1, last + 1, last + 2]
    got = check(driver, commands)
    answers = [g[0] for c, g in zip(commands, got) if c.startswith("lookup")]
    assert answers == expect
    assert got[-1][1:3] == (last + 3, last + 2)          # every mismatch freed one copy and made one


def test_adopt_replaces_every_device_and_forget_drops_them(driver):
    got = check(driver, ["blob 1 8200 1", "blob 2 300 2", "lookup 1 0", "lookup 1 1", "lookup 1 2", "lookup 2 0", "each",
                         "adopt 1 1", "each", "lookup 1 1", "lookup 1 0", "each", "forget 1", "each", "forget 1", "lookup 2 0", "forget 2", "each"])
    assert got[6][0] == 4 and got[6][3] == ["v0", "v1", "v2", "v3"]                   # every live copy once
    assert got[7][0] == 4 and got[7][3] == ["f0", "f1", "f2"]                        # the address's copies on all devices, not blob 2's
    assert got[8][3] == ["v3", "v4"] and got[9][0] == 4 and got[9][3] == []           # exactly one installed, and it answers
    assert got[10][0] == 5 and got[10][3] == ["u"]                                  # another device: its own upload
    assert got[12][3] == ["f4", "f5"] and got[13][3] == ["v3"] and got[14][3] == []   # forget frees all, installs none; twice is nothing
    assert got[15][0] == 3 and got[17][0] == 0 and got[17][1:3] == (6, 6)


def test_a_failed_upload_leaves_no_entry(driver):
    got = check(driver, ["blob 1 4097 5", "fail 1", "lookup 1 0", "each", "lookup 1 0", "fail 0", "lookup 1 0", "lookup 1 0",
                         "poke 1 4096 9", "fail 1", "lookup 1 0", "lookup 1 0", "each", "fail 0", "lookup 1 0", "each"])
    assert [g[0] for g in got[2:5]] == [-1, 0, -1] and got[2][3] == ["u"] and got[4][3] == ["u"]
    assert got[6][0] == 0 and got[7][0] == 0
    # the tail stripe (one byte) changed: lookup 1 since the fill re-checks stripe 1, frees the copy, and the upload fails
    assert got[10][0] == -1 and got[10][3] == ["f0", "u"] and got[11][0] == -1 and got[11][3] == ["u"] and got[12][0] == 0
    assert got[14][0] == 1 and got[15][3] == ["v1"] and got[15][1:3] == (2, 1)


def test_leak_detection_is_on(driver):
    """The proof rests on it: memory nobody frees (the driver's `leak`) fails the run."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([driver], input="leak\n", capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode != 0 and "LeakSanitizer" in r.stderr
