"""The launch plan of LISTED batches (rtk_dev_trace_rays*_listed: TraceRequest::listed, rtk_amd/csrc/rtk_trace_plan.h), checked
without a GPU by tests/trace_plan_listed_driver.cpp, the existing plan driver with the two new inputs.

What a listed batch is, whatever the options say: no image (no hint taken, no look asked for, the image defaults of refill_min
and node_exit never taken), no packet kernel, no entry lists, no re-ordering pre-pass, always dealt from the queues (the host does
not know how many rays are traced: the counter reset and a persistent grid even for one workgroup's worth), grid and spill area
sized by num_rays. The assembly per-lane kernels take it exactly when they take the plain batch of that size that has no image
hint, no SORT_RAYS and no STATIC (the three things a listed batch ignores) -- and their listed forms are loaded.

An unlisted request must plan exactly as before: the old driver, which does not know the field, and the new one with listed
left alone and with listed=0 answer the old test's whole table alike, word for word."""
import itertools
import os
import subprocess

import pytest

from .test_trace_plan_cpu import CASES as UNLISTED_CASES
from .test_trace_plan_cpu import EXACT_NODES, NO_ASM, ROOT, SORT_RAYS, STATIC

SIZES = [1, 256, 257, 1 << 20, (1 << 26) + 1]
FLAGS = [0, SORT_RAYS, STATIC, NO_ASM, SORT_RAYS | STATIC | NO_ASM, EXACT_NODES]


def hint_for(n):
    """an image hint that matches n (whole 64x64-pixel blocks where n allows it: what the packet kernels would take), or None"""
    if n == 1 << 20:
        return 1024, 1024
    if n == 256:
        return 16, 16
    return None


def listed_cases():
    out = []
    for n, f, any_hit, filtered, hinted in itertools.product(SIZES, FLAGS, (0, 1), (0, 1), (0, 1)):
        hint = hint_for(n)
        if hinted and not hint:
            continue
        given = dict(n=n, struct_size=28, flags=f, any_hit=any_hit, filtered=filtered, listed=1)
        if hinted:
            given.update(image_width=hint[0], image_height=hint[1])
        # the plain batch it is measured against: the same size and scene, without what a listed batch ignores
        plain = dict(n=n, struct_size=28, flags=f & ~(SORT_RAYS | STATIC), any_hit=any_hit, filtered=filtered)
        out.append(("n=%d flags=%d any=%d filt=%d hint=%d" % (n, f, any_hit, filtered, hinted), given, plain))
    return out


LISTED = listed_cases()
EXTRA = [
    ("listed, no options block", dict(n=1 << 20, listed=1), dict(n=1 << 20)),
    ("listed, the listed kernels not loaded", dict(n=1 << 20, listed=1, lane_listed_loaded=0), dict(n=1 << 20, lane_loaded=0)),
    ("listed, only the listed kernels loaded", dict(n=1 << 20, listed=1, lane_loaded=0), dict(n=1 << 20)),
    ("listed, 2^26 rays", dict(n=1 << 26, listed=1), dict(n=1 << 26)),
    ("listed, refill_min and node_exit given", dict(n=1 << 20, listed=1, struct_size=28, image_width=1024, image_height=1024, refill_min=5, node_exit=7),
     dict(n=1 << 20, struct_size=28, refill_min=5, node_exit=7)),
    ("listed, blocks_per_cu 2", dict(n=1 << 20, listed=1, struct_size=28, blocks_per_cu=2), dict(n=1 << 20, struct_size=28, blocks_per_cu=2)),
    ("listed, a looked-at image is not taken", dict(n=16384, listed=1, look_w=128, look_h=128), dict(n=16384)),
    ("listed, big leaves, any hit", dict(n=1 << 20, listed=1, any_hit=1, big_leaf_fraction=0.05), dict(n=1 << 20, any_hit=1, big_leaf_fraction=0.05)),
    ("listed, a deep stack", dict(n=1 << 20, listed=1, stack_entries=512), dict(n=1 << 20, stack_entries=512)),
]


def build(tmp, source):
    exe = str(tmp / os.path.splitext(source)[0])
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "rtk_amd", "csrc"), os.path.join(ROOT, "tests", source), "-o", exe])
    return exe


def ask(exe, cases):
    text = "".join(" ".join("%s=%r" % kv for kv in given.items()) + "\n" for given in cases)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    return [{k: int(v) for k, v in (w.split("=") for w in line.split())} for line in lines]


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("trace_plan_listed")
    return build(tmp, "trace_plan_driver.cpp"), build(tmp, "trace_plan_listed_driver.cpp")


@pytest.fixture(scope="module")
def answers(drivers):
    cases = LISTED + EXTRA
    got = ask(drivers[1], [g for _, g, _ in cases])
    plain = ask(drivers[1], [p for _, _, p in cases])
    return {name: (g, p) for (name, _, _), g, p in zip(cases, got, plain)}


def test_the_sizes_and_flags_of_the_table():
    assert {g["n"] for _, g, _ in LISTED} == set(SIZES)
    assert any(g.get("image_width") for _, g, _ in LISTED) and any(g["flags"] & SORT_RAYS for _, g, _ in LISTED)
    assert any(g["flags"] & STATIC for _, g, _ in LISTED) and any(g["flags"] & NO_ASM for _, g, _ in LISTED) and any(g["filtered"] for _, g, _ in LISTED)


@pytest.mark.parametrize("name", [c[0] for c in LISTED + EXTRA])
def test_listed_plan(answers, name):
    got, plain = answers[name]
    given = dict((c[0], c[1]) for c in LISTED + EXTRA)[name]
    n = given["n"]
    assert got["error"] == 0 and got["look"] == 0
    assert got["packet"] == 0 and got["hot"] == 0 and got["entries"] == 0 and got["sort_rays"] == 0 and got["hot_grid"] == 0
    assert got["image_w"] == 0 and got["image_h"] == 0 and got["tile_blocks"] == 0
    assert got["dynamic"] == 1
    # never the image defaults (64 / 24): what was given, or the plain defaults
    assert got["refill_min"] == (given.get("refill_min") or 8) and got["node_exit"] == (given.get("node_exit") or 32)
    # the assembly kernels: as for the plain batch of this size, and never with filters
    want_lane = plain["lane_hot"]
    if name == "listed, only the listed kernels loaded":
        want_lane = 1
    assert got["lane_hot"] == want_lane
    if given.get("filtered"):
        assert got["lane_hot"] == 0
    if n <= 256 or n > 1 << 26 or given.get("flags", 0) & NO_ASM:
        assert got["lane_hot"] == 0
    assert got["variant"] == plain["variant"] == got["variant_of"] and got["qn"] == plain["qn"]
    # grid and spill area by num_rays: a persistent grid (256 CUs x occupancy 4, or blocks_per_cu), no more workgroups than n has
    blocks_needed = (n + 255) // 256
    per_cu = min(given.get("blocks_per_cu") or 4, 4)
    assert got["grid"] == min(256 * per_cu, blocks_needed)
    assert got["lane_grid"] == (min(256 * 5, blocks_needed) if got["lane_hot"] else 0)
    assert got["spill_lanes"] == max(got["grid"], got["lane_grid"]) * 256
    assert got["lds_entries"] == 15 and got["spill_cap"] == given.get("stack_entries", 40) - 15


def test_unlisted_requests_plan_as_before(drivers):
    """The old driver fills TraceRequest field by field and has never heard of `listed`: its answers over the old test's table are
    the plan with the field at its default. The new driver with the field left alone, and with listed=0, must give the same words."""
    old_exe, new_exe = drivers
    given = [g for _, g, _ in UNLISTED_CASES]
    old = ask(old_exe, given)
    assert ask(new_exe, given) == old
    assert ask(new_exe, [dict(g, listed=0) for g in given]) == old
    assert ask(new_exe, [dict(g, lane_listed_loaded=0) for g in given]) == old
    # ... and the field does change the plan where it is set: the table is not blind to it
    changed = sum(a != b for a, b in zip(ask(new_exe, [dict(g, listed=1) for g in given]), old))
    assert changed > len(given) // 3
