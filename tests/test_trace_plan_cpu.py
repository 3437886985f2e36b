"""Which kernels a trace launch runs (rtk_amd/csrc/rtk_trace_plan.h), checked without a GPU: tests/trace_plan_driver.cpp is
built by the host compiler against that header alone and answers a table of cases.

The expected values were written down by reading rtk_launch_trace as it was before the decision moved into plan_trace (the
chain of conditions on the options, the image, the scene and the loaded kernels), not by running the new code. "kernel" is
the number RTK_AMD_LOG_PATH prints as "beam": -1 the C++ packet kernel, 0 rtk_packet_hot, 1 rtk_packet_beam,
2 rtk_packet_beam2, 3 rtk_packet_count2, 4 rtk_packet_any2. It says which hand-written kernel WOULD run; it does run where
"hot" is 1, and the C++ packet kernel takes the whole batch where "packet" is 1 and "hot" is 0.

The scene of every case unless it says otherwise: built (compressed nodes there), 200000 nodes, 1000000 triangles, 40 stack
entries, |planes| <= 100, no big leaves, 256 CUs; every hand-written kernel loaded (7 / 8 / 7 workgroups per CU for
rtk_packet_hot / _beam / _beam2, 5 for rtk_lane_hot); 4 workgroups per CU of the C++ kernel."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STATIC, NO_PACKET, SORT_RAYS, EXACT_NODES, NO_ASM, NO_ENTRIES, NO_BEAM, ONE_TILE_BEAM, NO_DETECT = 1, 2, 4, 8, 16, 32, 64, 128, 256
ERR_UNSUPPORTED = -6
CPP, HOT, BEAM, BEAM2, COUNT2, ANY2 = -1, 0, 1, 2, 3, 4
ALL, NO_BEAM2, ONLY_HOT, NO_COUNT2, NO_ANY2 = 31, 31 - 4, 1, 31 - 8, 31 - 16      # "loaded": bit k = kernel k


def flags(f, **more):
    return dict(struct_size=28, flags=f, **more)


def image(w, h, f=0, **more):
    return dict(n=w * h, struct_size=28, flags=f, image_width=w, image_height=h, **more)


def want(*parts, **more):
    return {k: v for part in parts + (more,) for k, v in part.items()}


# the four ways a batch is traced, as the plan spells them
LANE_HOT = dict(packet=0, hot=0, lane_hot=1)
VARIANT = dict(packet=0, hot=0, lane_hot=0)
PACKET_HOT = dict(packet=1, hot=1, lane_hot=0)
PACKET_CPP = dict(packet=1, hot=0, lane_hot=0)
IMAGE_DEFAULTS = dict(refill_min=64, node_exit=24)

CASES = [
    # --- plain batches: 1e6 rays = 3907 workgroups' worth; persistent grids of 256 CUs x 4 (C++) and x 5 (assembly)
    ("plain closest hit", dict(), want(LANE_HOT, dynamic=1, image_w=0, qn=1, variant=8, entries=0, sort_rays=0, tile_blocks=0, refill_min=8, node_exit=32,
                                       grid=1024, lane_grid=1280, lds_entries=15, spill_cap=25, spill_lanes=1280 * 256, error=0, look=0)),
    ("plain any hit", dict(any_hit=1), want(LANE_HOT, variant=9)),
    ("EXACT_NODES", flags(EXACT_NODES), want(VARIANT, qn=0, variant=0, grid=1024, spill_lanes=1024 * 256)),
    ("NO_ASM", flags(NO_ASM), want(VARIANT, qn=1, variant=8)),
    ("STATIC", flags(STATIC), want(VARIANT, dynamic=0, variant=8, grid=3907)),
    ("SORT_RAYS", flags(SORT_RAYS), want(LANE_HOT, sort_rays=1, variant=8)),
    ("SORT_RAYS in a block too short to hold flags", dict(struct_size=8, flags=SORT_RAYS), want(LANE_HOT, sort_rays=0, o_flags=0)),
    ("one workgroup", dict(n=256), want(VARIANT, dynamic=0, grid=1, variant=8)),
    ("one workgroup and a ray", dict(n=257), want(LANE_HOT, dynamic=1, grid=2, lane_grid=2)),
    ("no compressed nodes", dict(has_qnodes=0), want(VARIANT, qn=0, variant=0)),
    ("QNODES=0", dict(QNODES=0), want(VARIANT, qn=0, variant=0)),
    ("LANE_ASM=0", dict(LANE_ASM=0), want(VARIANT, qn=1, variant=8)),
    ("lane kernels not loaded", dict(lane_loaded=0), want(VARIANT, variant=8)),
    ("LANE_LDS=12", dict(LANE_LDS=12), want(LANE_HOT, lds_entries=12, spill_cap=28)),
    ("blocks_per_cu 2", flags(0, blocks_per_cu=2), want(LANE_HOT, grid=512, lane_grid=1280)),
    ("blocks_per_cu above what fits", flags(0, blocks_per_cu=9), dict(grid=1024)),
    ("refill_min and node_exit given", flags(0, refill_min=100, node_exit=70), want(LANE_HOT, refill_min=64, node_exit=64, o_refill_given=1)),
    ("a stack that fits LDS", dict(stack_entries=15), want(LANE_HOT, spill_cap=0)),
    ("a stack of 512", dict(stack_entries=512), want(VARIANT, spill_cap=497)),
    ("2^27 rays", dict(n=1 << 27), want(VARIANT, variant=8)),
    ("filtered", dict(filtered=1), want(VARIANT, variant=12)),
    ("filtered any hit, exact nodes", dict(filtered=1, any_hit=1, struct_size=28, flags=EXACT_NODES), want(VARIANT, variant=5)),
    ("collect", dict(collect=1), want(VARIANT, variant=17, qn=1)),
    ("collect, exact nodes", dict(collect=1, struct_size=28, flags=EXACT_NODES), want(VARIANT, variant=16)),
    ("counted", dict(counted=1), want(VARIANT, variant=10)),
    # --- images with a hint: 1024 x 1024 = 4096 workgroups' worth
    ("image 1024x1024", image(1024, 1024), want(PACKET_HOT, IMAGE_DEFAULTS, kernel=BEAM2, entries=1, tile_blocks=1, image_w=1024, image_h=1024, variant=18,
                                                 dynamic=1, grid=1024, hot_grid=1792, lds_entries=16, spill_cap=24, spill_lanes=1024 * 256, sort_rays=0, look=0)),
    ("image, ONE_TILE_BEAM", image(1024, 1024, ONE_TILE_BEAM), want(PACKET_HOT, kernel=BEAM, entries=1, hot_grid=2048)),
    ("image, NO_BEAM", image(1024, 1024, NO_BEAM), want(PACKET_HOT, kernel=HOT, entries=1, hot_grid=1792)),
    ("image, NO_ASM", image(1024, 1024, NO_ASM), want(PACKET_CPP, kernel=BEAM2, entries=1, tile_blocks=1, variant=18)),
    ("image, NO_ENTRIES", image(1024, 1024, NO_ENTRIES), want(PACKET_HOT, kernel=BEAM2, entries=0)),
    ("image, NO_PACKET", image(1024, 1024, NO_PACKET), want(VARIANT, IMAGE_DEFAULTS, image_w=1024, tile_blocks=1, entries=0, variant=8, lds_entries=15)),
    ("image, SORT_RAYS", image(1024, 1024, SORT_RAYS), want(PACKET_HOT, sort_rays=0)),
    ("image, refill_min and node_exit given", image(1024, 1024, 0, refill_min=8, node_exit=32), want(PACKET_HOT, refill_min=8, node_exit=32)),
    ("image, rtk_packet_beam2 not loaded", dict(image(1024, 1024), loaded=NO_BEAM2), want(PACKET_HOT, kernel=BEAM, hot_grid=2048)),
    ("image, only rtk_packet_hot loaded", dict(image(1024, 1024), loaded=ONLY_HOT), want(PACKET_HOT, kernel=HOT)),
    ("image, nothing loaded", dict(image(1024, 1024), loaded=0), want(PACKET_CPP, kernel=HOT, entries=1)),
    ("image, PACKET_BEAM=1", dict(image(1024, 1024), PACKET_BEAM=1), want(PACKET_HOT, kernel=BEAM)),
    ("image, PACKET_BEAM=0", dict(image(1024, 1024), PACKET_BEAM=0), want(PACKET_HOT, kernel=HOT)),
    ("image, PACKET_BEAM=1 and NO_BEAM", dict(image(1024, 1024, NO_BEAM), PACKET_BEAM=1), want(PACKET_HOT, kernel=HOT)),
    ("image, PACKET_ASM=0", dict(image(1024, 1024), PACKET_ASM=0), want(PACKET_CPP, kernel=BEAM2, entries=1)),
    ("image, PACKET_ENTRIES=0", dict(image(1024, 1024), PACKET_ENTRIES=0), want(PACKET_HOT, entries=0)),
    ("image, TILE_BLOCKS=0", dict(image(1024, 1024), TILE_BLOCKS=0), want(PACKET_CPP, tile_blocks=0, entries=0)),
    ("image, HOT_BLOCKS_PER_CU=3", dict(image(1024, 1024), HOT_BLOCKS_PER_CU=3), want(PACKET_HOT, hot_grid=768)),
    ("image 72x72", image(72, 72), want(PACKET_CPP, IMAGE_DEFAULTS, image_w=72, tile_blocks=0, entries=0, variant=18, grid=21)),
    ("image 64x128", image(64, 128), want(PACKET_CPP, tile_blocks=1, entries=1, grid=32)),
    ("image 128x64", image(128, 64), want(PACKET_HOT, tile_blocks=1, entries=1, hot_grid=32)),
    ("image 100x100: not whole 8x8 tiles", image(100, 100), want(LANE_HOT, image_w=0, refill_min=8, node_exit=32)),
    ("image hint of another batch", dict(image(1024, 1024), n=1000000), want(LANE_HOT, image_w=0)),
    ("image hint in a block too short to hold it", dict(image(1024, 1024), struct_size=8), want(LANE_HOT, image_w=0, look=1)),
    ("any-hit image", image(1024, 1024, any_hit=1), want(PACKET_HOT, kernel=ANY2, entries=1, variant=18, hot_grid=1792)),
    ("any-hit image, rtk_packet_any2 not loaded", dict(image(1024, 1024, any_hit=1), loaded=NO_ANY2), want(PACKET_CPP, kernel=CPP, entries=1)),
    ("any-hit image, ONE_TILE_BEAM", image(1024, 1024, ONE_TILE_BEAM, any_hit=1), want(PACKET_CPP, kernel=CPP)),
    ("any-hit image, ANY_PACKETS=0", dict(image(1024, 1024, any_hit=1), ANY_PACKETS=0), want(VARIANT, image_w=1024, variant=9, kernel=BEAM2)),
    ("any-hit image 72x72", image(72, 72, any_hit=1), want(VARIANT, image_w=72, variant=9)),
    ("any-hit image 64x128", image(64, 128, any_hit=1), want(VARIANT, variant=9)),
    ("any-hit image, STATIC", image(1024, 1024, STATIC, any_hit=1), want(VARIANT, variant=9, dynamic=0)),
    ("any-hit image, counted", image(1024, 1024, any_hit=1, counted=1), want(VARIANT, variant=11)),
    ("filtered image", image(1024, 1024, filtered=1), want(VARIANT, variant=12, image_w=1024, entries=0)),
    ("collect image", image(1024, 1024, collect=1), want(VARIANT, variant=17)),
    ("counted image", image(1024, 1024, counted=1), want(PACKET_CPP, variant=19, entries=1, kernel=BEAM2)),
    ("packet-counted image", image(1024, 1024, pk_counted=1), want(PACKET_HOT, kernel=COUNT2, hot_grid=1792, error=0)),
    ("packet-counted, rtk_packet_count2 not loaded", dict(image(1024, 1024, pk_counted=1), loaded=NO_COUNT2), dict(error=ERR_UNSUPPORTED, has_message=1)),
    ("packet-counted, rtk_packet_beam2 not loaded", dict(image(1024, 1024, pk_counted=1), loaded=NO_BEAM2), dict(error=ERR_UNSUPPORTED, has_message=1)),
    ("packet-counted, ONE_TILE_BEAM", image(1024, 1024, ONE_TILE_BEAM, pk_counted=1), dict(error=ERR_UNSUPPORTED, has_message=1)),
    ("packet-counted image 72x72", image(72, 72, pk_counted=1), dict(error=ERR_UNSUPPORTED, has_message=1)),
    ("packet-counted, no image", dict(pk_counted=1), dict(error=ERR_UNSUPPORTED, has_message=1)),
    # --- the scene
    ("image, 65 stack entries", dict(image(1024, 1024), stack_entries=65), want(VARIANT, image_w=1024, variant=8, spill_cap=50)),
    ("image, 64 stack entries", dict(image(1024, 1024), stack_entries=64), want(PACKET_HOT, spill_cap=48)),
    ("image, |planes| up to 2^19", dict(image(1024, 1024), bound_abs=524288), want(PACKET_CPP, entries=0)),
    ("plain, |planes| up to 2^19", dict(bound_abs=524288), want(LANE_HOT)),
    ("plain, |planes| up to 2^60", dict(bound_abs=2.0 ** 60), want(VARIANT)),
    ("image, no nodes", dict(image(1024, 1024), num_nodes=0), want(PACKET_HOT, entries=0)),
    ("image, big leaves", dict(image(1024, 1024), big_leaf_fraction=0.05), want(PACKET_HOT, kernel=BEAM2)),
    ("image, big leaves, ONE_TILE_BEAM", dict(image(1024, 1024, ONE_TILE_BEAM), big_leaf_fraction=0.05), want(PACKET_CPP, kernel=BEAM)),
    ("image, big leaves, NO_BEAM", dict(image(1024, 1024, NO_BEAM), big_leaf_fraction=0.05), want(PACKET_CPP, kernel=HOT)),
    ("any-hit image, big leaves", dict(image(1024, 1024, any_hit=1), big_leaf_fraction=0.05), want(PACKET_HOT, kernel=ANY2)),
    ("plain any hit, big leaves", dict(any_hit=1, big_leaf_fraction=0.05), want(VARIANT, variant=9)),
    ("plain closest hit, big leaves", dict(big_leaf_fraction=0.05), want(LANE_HOT)),
    ("2^31 bytes of compressed nodes", dict(num_nodes=1 << 25), want(VARIANT)),
    ("2^31 bytes of triangles", dict(num_tris=44739243), want(VARIANT)),
    # --- no hint: is the batch looked at, and what becomes of the verdict
    ("look: 16384 rays, no options", dict(n=16384), dict(look=1)),
    ("look: empty options", dict(n=16384, struct_size=28), dict(look=1)),
    ("look: any hit", dict(n=16384, any_hit=1), dict(look=1)),
    ("look: NO_DETECT", dict(n=16384, struct_size=28, flags=NO_DETECT), dict(look=0)),
    ("look: NO_DETECT in a block too short to hold flags", dict(n=16384, struct_size=8, flags=NO_DETECT), dict(look=1)),
    ("look: NO_PACKET", dict(n=16384, struct_size=28, flags=NO_PACKET), dict(look=0)),
    ("look: SORT_RAYS", dict(n=16384, struct_size=28, flags=SORT_RAYS), dict(look=0)),
    ("look: STATIC", dict(n=16384, struct_size=28, flags=STATIC), dict(look=0)),
    ("look: 16000 rays", dict(n=16000), dict(look=0)),
    ("look: 12288 rays", dict(n=12288), dict(look=0)),
    ("look: 2^30 + 4096 rays", dict(n=(1 << 30) + 4096), dict(look=0)),
    ("look: a filter", dict(n=16384, filtered=1), dict(look=0)),
    ("look: a filter with nothing set", dict(n=16384, has_filter=1), dict(look=0, variant=8)),
    ("look: collect", dict(n=16384, collect=1), dict(look=0)),
    ("look: counted", dict(n=16384, counted=1), dict(look=0)),
    ("look: packet-counted", dict(n=16384, pk_counted=1), dict(look=0)),
    ("look: a hint", image(128, 128), dict(look=0)),
    ("look: 65 stack entries", dict(n=16384, stack_entries=65), dict(look=0)),
    ("look: DETECT_IMAGE=0", dict(n=16384, DETECT_IMAGE=0), dict(look=0)),
    ("found 128x128", dict(n=16384, look_w=128, look_h=128), want(PACKET_HOT, IMAGE_DEFAULTS, image_w=128, image_h=128, kernel=BEAM2, entries=1, tile_blocks=1, hot_grid=64)),
    ("found 128x128, refill_min given", dict(n=16384, look_w=128, look_h=128, struct_size=28, refill_min=8, node_exit=32), want(PACKET_HOT, IMAGE_DEFAULTS)),
    ("found 64x256: one block per row", dict(n=16384, look_w=64, look_h=256), want(LANE_HOT, image_w=0, refill_min=8, node_exit=32)),
    ("found 256x72: not whole blocks", dict(n=18432, look_w=256, look_h=72), want(LANE_HOT, image_w=0)),
    ("found any-hit 128x128", dict(n=16384, any_hit=1, look_w=128, look_h=128), want(PACKET_HOT, kernel=ANY2)),
    # --- the options block at every length that adds a field
    ("options of 0 bytes", dict(struct_size=0, flags=511, image_width=1024, image_height=512, refill_min=100, blocks_per_cu=3, node_exit=70),
     dict(o_flags=0, o_image_w=0, o_image_h=0, o_refill_min=0, o_refill_given=0, o_blocks_per_cu=0, o_node_exit=0)),
    ("options of 8 bytes", dict(struct_size=8, flags=511, image_width=1024, image_height=512, refill_min=100, blocks_per_cu=3, node_exit=70),
     dict(o_flags=0, o_image_w=0, o_image_h=0, o_refill_min=0, o_refill_given=0, o_blocks_per_cu=0, o_node_exit=0)),
    ("options of 16 bytes", dict(struct_size=16, flags=511, image_width=1024, image_height=512, refill_min=100, blocks_per_cu=3, node_exit=70),
     dict(o_flags=511, o_image_w=1024, o_image_h=512, o_refill_min=0, o_refill_given=0, o_blocks_per_cu=0, o_node_exit=0)),
    ("options of 24 bytes", dict(struct_size=24, flags=511, image_width=1024, image_height=512, refill_min=100, blocks_per_cu=3, node_exit=70),
     dict(o_flags=511, o_image_w=1024, o_image_h=512, o_refill_min=64, o_refill_given=1, o_blocks_per_cu=3, o_node_exit=0)),
    ("options of 28 bytes", dict(struct_size=28, flags=511, image_width=1024, image_height=512, refill_min=100, blocks_per_cu=3, node_exit=70),
     dict(o_flags=511, o_image_w=1024, o_image_h=512, o_refill_min=64, o_refill_given=1, o_blocks_per_cu=3, o_node_exit=64)),
    ("no options", dict(), dict(o_flags=0, o_image_w=0, o_refill_min=0, o_refill_given=0, o_blocks_per_cu=0, o_node_exit=0)),
    ("options of 28 bytes, small values", dict(struct_size=28, refill_min=5, node_exit=7), dict(o_refill_min=5, o_refill_given=1, o_node_exit=7, refill_min=5, node_exit=7)),
]


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """The driver built against the header only (no HIP include path, -Wall -Werror) and run once over all cases."""
    exe = str(tmp_path_factory.mktemp("trace_plan") / "trace_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "rtk_amd", "csrc"), os.path.join(ROOT, "tests", "trace_plan_driver.cpp"), "-o", exe])
    text = "".join(" ".join("%s=%r" % kv for kv in given.items()) + "\n" for _, given, _ in CASES)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(CASES)
    return {name: {k: int(v) for k, v in (w.split("=") for w in line.split())} for (name, _, _), line in zip(CASES, lines)}


def test_plan_header_includes_no_hip():
    includes = [l.split()[1] for l in open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_trace_plan.h")) if l.startswith("#include")]
    assert includes == ['"rtk_amd.h"', "<stddef.h>", "<stdint.h>"]


def test_case_names_are_unique():
    assert len({name for name, _, _ in CASES}) == len(CASES)


@pytest.mark.parametrize("name,given,expected", CASES, ids=[c[0] for c in CASES])
def test_plan(answers, name, given, expected):
    got = answers[name]
    assert {k: got[k] for k in expected} == expected
    if got["error"] == 0:
        # the occupancy is asked for the variant the plan then names; one path at most; the assembly packet kernel only with the packet path
        assert got["variant_of"] == got["variant"]
        assert got["packet"] + got["lane_hot"] <= 1 and got["hot"] <= got["packet"]
        assert (got["hot_grid"] > 0) == bool(got["hot"]) and (got["lane_grid"] > 0) == bool(got["lane_hot"])
