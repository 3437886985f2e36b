"""GPU tests of rtk_dev_scene_quality: the SAH cost of a device scene's tree, measured on the device.

The yardstick is the exported blob walked in numpy float64 with the header's area formula,
2 * (dx*dy + dy*dz + dz*dx), dx = (double)max - (double)min. TOLERANCE, derived and not measured: both sides add the same
double terms (every area is formed by the same operations in the same order, so term for term they are equal) in different
orders; with n <= 2e4 non-negative terms the two sums differ by at most about n * 2^-53 ~ 2e-12 relative. The tests assert
1e-9 relative on the sums and on what is derived from them, and exact equality on the counters. Everything that compares
the device with itself (two calls, a refit there and back, a twin scene, a replica) asserts bit identity."""
import ctypes as C

import numpy as np
import pytest

from rtk_amd import synth
from rtk_amd.types import MeshSet

pytestmark = pytest.mark.gpu

REL = 1e-9
COST_NODE, COST_TRI = 0.5, 1.0                      # the builder's constants (rtk_sah_costs)
SUMS = ("root_area", "inner_area", "leaf_area", "leaf_area_triangles")
DERIVED = ("node_visits", "triangle_tests", "sah_cost")
COUNTERS = ("nonfinite_boxes", "inner_children", "leaf_children")
RESULT_BYTES = 88                                   # everything in front of measure_ms


def deform(pos, k, ext=None):
    """Every vertex moved by a smooth, seed-free function of its position (shared vertices stay shared): a sine
    displacement of 3 % * k of the scene extent, computed in float64 and cast back. k = 0 is the input itself."""
    if k == 0:
        return pos.copy()
    p = np.asarray(pos, np.float64)
    if ext is None:
        ext = np.asarray(pos).max(0) - np.asarray(pos).min(0) if len(p) else np.ones(3)     # (in the positions' own format)
    ext = np.where(np.asarray(ext, np.float64) > 0, ext, 1.0)
    d = np.stack([np.sin(3.1 * p[:, 1] / ext[1] + 1.0), np.sin(2.3 * p[:, 2] / ext[2] + 2.0), np.sin(2.9 * p[:, 0] / ext[0] + 3.0)], axis=1)
    return (p + 0.03 * k * ext * d).astype(pos.dtype)


def _area(lo, hi):
    d = np.asarray(hi, np.float64) - np.asarray(lo, np.float64)
    return 2.0 * (d[0] * d[1] + d[1] * d[2] + d[2] * d[0])


def blob_quality(blob):
    """What rtk_dev_scene_quality must report for the tree in this blob, and the leaves met on the way as (triangle count,
    triangle index of the first record). Walks from the root node at byte 128: 24 floats of boxes [axis][min|max][slot],
    four 64-bit child words at byte 96 (bit 0: a leaf, whose first 64-bit word holds its count in the low 6 bits); an
    empty slot has min > max."""
    b = np.ascontiguousarray(blob).view(np.uint8).reshape(-1)
    inner, leaf, leaf_tris, leaves = [], [], [], []
    nonfinite = inner_children = leaf_children = 0
    root_area = 0.0
    stack = [128]
    with np.errstate(invalid="ignore", over="ignore"):
        while stack:
            at = stack.pop()
            box = b[at:at + 96].view(np.float32).reshape(3, 2, 4)
            ptr = b[at + 96:at + 128].view(np.uint64)
            used = [k for k in range(4) if not (box[:, 0, k] > box[:, 1, k]).all()]
            if at == 128 and used:
                root_area = float(_area(np.fmin.reduce(box[:, 0, used], axis=1), np.fmax.reduce(box[:, 1, used], axis=1)))
            for k in used:
                a = float(_area(box[:, 0, k], box[:, 1, k]))
                p = int(ptr[k])
                if p & 1:
                    at_leaf = p ^ 1
                    count = int(b[at_leaf:at_leaf + 8].view(np.uint64)[0]) & 63
                    leaves.append((count, int(b[at_leaf + 12:at_leaf + 16].view(np.uint32)[0])))
                    leaf_children += 1
                    if np.isfinite(a):
                        leaf.append(a)
                        leaf_tris.append(a * float(count))
                    else:
                        nonfinite += 1
                else:
                    stack.append(p)
                    inner_children += 1
                    if np.isfinite(a):
                        inner.append(a)
                    else:
                        nonfinite += 1
    want = dict(nonfinite_boxes=nonfinite, inner_children=inner_children, leaf_children=leaf_children, root_area=root_area,
                inner_area=float(np.sum(np.asarray(inner, np.float64))), leaf_area=float(np.sum(np.asarray(leaf, np.float64))),
                leaf_area_triangles=float(np.sum(np.asarray(leaf_tris, np.float64))), node_visits=0.0, triangle_tests=0.0, sah_cost=0.0)
    if np.isfinite(root_area) and root_area != 0.0:
        want["node_visits"] = 1.0 + want["inner_area"] / root_area
        want["triangle_tests"] = want["leaf_area_triangles"] / root_area
        want["sah_cost"] = COST_NODE * want["node_visits"] + COST_TRI * want["triangle_tests"]
    return want, leaves


def raw_quality(api, handle, stream=None):
    q = api.SceneQuality()
    q.struct_size = C.sizeof(api.SceneQuality)
    assert api.lib().rtk_dev_scene_quality(handle, C.byref(q), stream) == 0, api.last_error()
    return q


def bits(q):
    """every result byte of the structure (measure_ms, the last field, is a wall time)"""
    assert type(q).measure_ms.offset == RESULT_BYTES
    return bytes(q)[:RESULT_BYTES]


def sums_bits(q):
    return bytes(q)[:RESULT_BYTES - 8]               # ... without sah_cost_at_build, which is the scene's memory, not a sum


def check_against(got, want, what):
    print("%s: device %s" % (what, {k: got[k] for k in COUNTERS + SUMS + DERIVED}))
    print("%s: numpy  %s" % (what, {k: want[k] for k in COUNTERS + SUMS + DERIVED}))
    for k in COUNTERS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in SUMS + DERIVED:
        assert abs(got[k] - want[k]) <= REL * abs(want[k]), (what, k, got[k], want[k])


@pytest.fixture(scope="module")
def config1(api):
    """The config-1 scene (10 000 triangles, about 4.6k nodes: many workgroups' worth plus a ragged tail), what numpy makes
    of a device build of it, and the device's own answer for that build: made once, read by every case."""
    v0 = synth.scene_for_config(1)
    ds = api.DeviceScene.build([dict(positions=v0)])
    want, leaves = blob_quality(ds.export_blob())
    q = raw_quality(api, ds.handle)
    return dict(v0=v0, want=want, leaves=leaves, bits=sums_bits(q), sah_cost=q.sah_cost)


def test_against_the_blob(api, config1):
    ds = api.DeviceScene.build([dict(positions=config1["v0"])])
    ok, c0 = ds.validate()
    assert ok, c0
    bytes_before = ds.info()["total_device_bytes"]
    got = ds.quality()
    check_against(got, config1["want"], "config 1")
    info = ds.info()
    assert got["inner_children"] == info["num_nodes"] - 1
    assert sum(count for count, _ in config1["leaves"]) == info["num_triangles"] == 10_000
    assert got["leaf_children"] == len(config1["leaves"]) and got["nonfinite_boxes"] == 0
    assert got["sah_cost"] == COST_NODE * got["node_visits"] + COST_TRI * got["triangle_tests"]
    assert got["sah_cost_at_build"] == got["sah_cost"] and got["ratio"] == 1.0 and got["measure_ms"] > 0.0
    # no scene bit changes
    ok, c1 = ds.validate()
    assert ok and c1["content_hash"] == c0["content_hash"]
    # the first call made the scene's records and result slot; no later call allocates
    bytes_first = info["total_device_bytes"]
    assert bytes_before < bytes_first <= bytes_before + (1 << 17)
    ds.quality()
    assert ds.info()["total_device_bytes"] == bytes_first


def test_determinism_and_baseline(api, config1):
    v0 = config1["v0"]
    ds = api.DeviceScene.build([dict(positions=v0)])
    a, b = raw_quality(api, ds.handle), raw_quality(api, ds.handle)
    assert bits(a) == bits(b)
    assert sums_bits(a) == config1["bits"]                     # (another build of the same input: the same bits)
    assert a.sah_cost_at_build == a.sah_cost and b.sah_cost_at_build == b.sah_cost and a.sah_cost > 0.0
    ds.refit([dict(positions=v0)])
    c = raw_quality(api, ds.handle)
    assert bits(c) == bits(a)                                  # every sum, and the cost the scene remembers
    # a scene whose first measurement comes after a refit never learns what it cost when it was built
    late = api.DeviceScene.build([dict(positions=v0)])
    late.refit([dict(positions=v0)])
    q = late.quality()
    assert q["sah_cost_at_build"] == 0.0 and q["ratio"] is None
    assert q["sah_cost"] == a.sah_cost
    assert late.quality()["sah_cost_at_build"] == 0.0


def test_it_sees_a_ruined_tree(api, config1):
    """Every triangle takes another triangle's place: the topology now groups triangles that lie all over the scene, nearly
    every inner box spans it, node_visits approaches num_nodes. The factor 2 is a floor, orders of magnitude below that."""
    v0 = config1["v0"]
    n = len(v0) // 3
    perm = np.random.RandomState(7).permutation(n)
    v1 = np.ascontiguousarray(v0.reshape(n, 3, 3)[perm].reshape(-1, 3))
    ds = api.DeviceScene.build([dict(positions=v0)])
    q0 = ds.quality()
    ds.refit([dict(positions=v1)])
    q1 = ds.quality()
    fresh = api.DeviceScene.build([dict(positions=v1)])
    qf = fresh.quality()
    rays = synth.rays_incoherent(16384)
    nodes_refitted = ds.trace_counted(rays)[1]["nodes"]
    nodes_fresh = fresh.trace_counted(rays)[1]["nodes"]
    print("ruined tree: sah_cost at build %.3f, refitted %.3f (ratio %.1f, node_visits %.1f of %d nodes), fresh build %.3f (refitted / fresh %.1f); "
          "nodes fetched by 16384 incoherent rays: refitted %d, fresh %d (%.1fx)"
          % (q0["sah_cost"], q1["sah_cost"], q1["ratio"], q1["node_visits"], ds.info()["num_nodes"], qf["sah_cost"], q1["sah_cost"] / qf["sah_cost"],
             nodes_refitted, nodes_fresh, nodes_refitted / nodes_fresh))
    assert q1["sah_cost_at_build"] == q0["sah_cost"]
    assert q1["sah_cost"] > 2 * q1["sah_cost_at_build"] and q1["ratio"] > 2
    assert qf["sah_cost"] < 0.5 * q1["sah_cost"]
    assert nodes_refitted > nodes_fresh
    ds.refit([dict(positions=v0)])
    back = raw_quality(api, ds.handle)
    assert sums_bits(back) == config1["bits"] and back.sah_cost_at_build == q0["sah_cost"]


def test_smooth_deformation(api, config1):
    v0 = config1["v0"]
    ds = api.DeviceScene.build([dict(positions=v0)])
    ds.refit([dict(positions=deform(v0, 3))])
    got = ds.quality()
    want, _ = blob_quality(ds.export_blob())
    check_against(got, want, "deform(v0, 3)")
    assert got["sah_cost"] != config1["sah_cost"]              # (the refit moved something)


def test_partial_refit_twin(api, config1):
    tri = config1["v0"].reshape(-1, 3, 3)
    parts = [np.ascontiguousarray(p.reshape(-1, 3)) for p in np.array_split(tri, 4)]
    ext = config1["v0"].max(0) - config1["v0"].min(0)
    moved = deform(parts[1], 2, ext)
    a = api.DeviceScene.build([dict(positions=p) for p in parts])
    b = api.DeviceScene.build([dict(positions=p) for p in parts])
    qa0, qb0 = raw_quality(api, a.handle), raw_quality(api, b.handle)
    assert bits(qa0) == bits(qb0)
    a.refit([None, dict(positions=moved), None, None], only=[1])
    print("partial refit: %d of %d nodes remade" % (a.last_refit_nodes(), a.info()["num_nodes"]))
    b.refit([dict(positions=parts[0]), dict(positions=moved), dict(positions=parts[2]), dict(positions=parts[3])])
    qa, qb = raw_quality(api, a.handle), raw_quality(api, b.handle)
    assert bits(qa) == bits(qb) and sums_bits(qa) != sums_bits(qa0)


def test_big_leaves(api, oracle, config1):
    """The oracle's SAH build has leaves of up to 63 triangles: leaf_area_triangles is more than leaf_area here (device
    builds make about one triangle per leaf)."""
    ds = api.DeviceScene.upload(oracle.build_scene([dict(positions=config1["v0"])]))
    got = ds.quality()
    want, leaves = blob_quality(ds.export_blob())
    assert max(count for count, _ in leaves) > 3 and sum(count for count, _ in leaves) == 10_000
    check_against(got, want, "oracle blob")
    assert got["leaf_area_triangles"] > 1.5 * got["leaf_area"]
    assert got["sah_cost_at_build"] == got["sah_cost"]         # (an upload is a beginning too)


@pytest.mark.parametrize("n", [1, 2, 5, 64, 257])
def test_small_shapes(api, n):
    """A root with a single leaf child; fewer nodes than one workgroup covers in a trip (128); one such trip plus a tail."""
    ds = api.DeviceScene.build([dict(positions=synth.triangle_soup(n, 0.5, seed=17))])
    got = ds.quality()
    want, leaves = blob_quality(ds.export_blob())
    assert sum(count for count, _ in leaves) == n
    check_against(got, want, "%d triangles" % n)
    assert got["sah_cost"] > 0.0


def test_degenerate_root(api):
    ds = api.DeviceScene.build([dict(positions=np.full((3, 3), 0.25, np.float32))])
    q = raw_quality(api, ds.handle)
    assert q.root_area == 0.0 and q.node_visits == 0.0 and q.triangle_tests == 0.0 and q.sah_cost == 0.0
    assert q.leaf_children == 1 and q.inner_children == 0 and q.nonfinite_boxes == 0
    assert q.inner_area == 0.0 and q.leaf_area == 0.0


def test_no_triangles(api):
    ds = api.DeviceScene.build([dict(positions=np.zeros((0, 3), np.float32))])
    q = raw_quality(api, ds.handle)
    assert bytes(q)[4:RESULT_BYTES] == bytes(RESULT_BYTES - 4) and q.struct_size == C.sizeof(api.SceneQuality)


def test_non_finite(api, config1):
    """NaN positions, as test_gpu_refit.test_non_finite_positions_and_back gives them: one lone NaN vertex (the box of its
    leaf stays finite: fminf / fmaxf skip a NaN while the union has another member) and one whole NaN triangle that has its
    leaf to itself (found in the build's blob), whose box is NaN. That box is counted and left out; everything reported is
    finite. (No inf: an inf travels up to the root, whose area the call reports as it is.)"""
    v0 = config1["v0"]
    alone = [t for count, t in config1["leaves"] if count == 1]
    assert alone
    t = alone[len(alone) // 2]
    bad = v0.copy()
    bad[3 * t:3 * t + 3] = np.nan
    bad[3 * ((t + 1000) % (len(v0) // 3)) + 1] = np.nan
    ds = api.DeviceScene.build([dict(positions=v0)])
    q0 = raw_quality(api, ds.handle)
    ds.refit([dict(positions=bad)])
    q = ds.quality()
    print("non-finite: %s" % q)
    assert q["nonfinite_boxes"] > 0
    assert all(np.isfinite(v) for k, v in q.items() if isinstance(v, float))
    assert q["inner_children"] == q0.inner_children and q["leaf_children"] == q0.leaf_children
    assert q["sah_cost"] > 0.0
    ds.refit([dict(positions=v0)])
    back = raw_quality(api, ds.handle)
    assert back.nonfinite_boxes == 0 and bits(back) == bits(q0) and sums_bits(back) == config1["bits"]


def test_beside_a_trace(api, config1):
    import torch
    ds = api.DeviceScene.build([dict(positions=config1["v0"])])
    rays = synth.rays_incoherent(65536)
    n = len(rays)
    d_rays = api.to_device(rays)
    alone = ds.trace_device(d_rays, n).cpu().numpy().tobytes()
    tracing, measuring = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(tracing):
        d_rec = ds.trace_device(d_rays, n)                     # queued, not waited for
    q = raw_quality(api, ds.handle, C.c_void_p(measuring.cuda_stream))
    assert api.lib().rtk_dev_trace_status(ds.handle, C.c_void_p(tracing.cuda_stream)) == 0, api.last_error()
    assert d_rec.cpu().numpy().tobytes() == alone
    assert sums_bits(q) == config1["bits"]


def test_replicas_agree(api, config1):
    """rtk_mgpu_scene(m, i) is an ordinary scene: two slots on device 0 give the single scene's bytes."""
    L = api.lib()
    m = L.rtk_mgpu_create((C.c_int * 2)(0, 0), 2)
    assert m
    try:
        ms = MeshSet([dict(positions=config1["v0"])])
        assert L.rtk_mgpu_build(m, C.byref(ms.desc)) == 0, api.last_error()
        q = [raw_quality(api, L.rtk_mgpu_scene(m, i)) for i in range(2)]
        assert bits(q[0]) == bits(q[1]) and sums_bits(q[0]) == config1["bits"]
        assert q[0].sah_cost_at_build == q[0].sah_cost
    finally:
        L.rtk_mgpu_destroy(m)
