"""rtk_dev_scene_split_leaves on the GPU: big leaves of an uploaded blob become small subtrees, in place.

The authority everywhere is the oracle walking the blob EXPORTED AFTER the split: the reference's group-of-four rule applies
to the new leaves, so t, u, v and ids are compared bit for bit against that. Against the trace from before the split only
hit / miss and t within the project's 1e-5 can be asked (other groups of four, and ties between equal t go to another id).

The depth cap is the contract's: a leaf of K triangles becomes at most 2 * ceil(log4(K / max_leaf)) node levels."""
import ctypes as C

import numpy as np
import pytest

from rtk_amd import synth
from rtk_amd.types import HIT_RECORD_DTYPE
from tests.util import compare_hits, compare_hits_struct, load_golden

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF


def _as_blob(oracle, arr):
    b = oracle._aligned_bytes(arr.size)
    b[:] = arr
    return oracle.Blob(b)


def _level_cap(count, max_leaf):
    d, cap = 0, max_leaf
    while cap < count:
        cap *= 4
        d += 1
    return 2 * d


def _blob_tree(buf):
    """(leaf sizes, deepest node level, number of nodes) of a blob, parsed here (nodes of 96 bytes of
    boxes and four 64-bit child offsets from byte 128 on, bit 0 = leaf, the leaf's count in the low six bits of its first word;
    an empty slot has an inverted box)."""
    buf = np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
    leaves, deepest, nodes, todo = [], 0, 0, [(128, 1)]
    while todo:
        off, level = todo.pop()
        nodes += 1
        deepest = max(deepest, level)
        box = np.frombuffer(buf, "<f4", 24, off).reshape(3, 2, 4)
        child = np.frombuffer(buf, "<u8", 4, off + 96)
        for k in range(4):
            if not (box[:, 0, k] <= box[:, 1, k]).all():
                continue
            p = int(child[k])
            if p & 1:
                cnt = int(np.frombuffer(buf, "<u8", 1, p ^ 1)[0]) & 0x3F
                if cnt:
                    leaves.append(cnt)
            else:
                todo.append((p, level + 1))
    return leaves, deepest, nodes


def _valid(ds):
    ok, c = ds.validate()
    assert ok, c
    return c


def _exact_against_exported_blob(oracle, ds, rays, what, opts=None):
    """records of `ds` against the oracle on the blob exported from it now: mask, ids, t, u, v bit for bit"""
    blob = _as_blob(oracle, ds.export_blob())
    rec = ds.trace(rays, opts=opts, full=False)
    oh, om = oracle.trace(blob, rays)
    gm = rec["prim"] != NONE
    assert (gm == om).all(), what
    base = ds.mesh_base()
    assert (rec["prim"][gm] == base[oh["mesh_index"][om].astype(np.int64)] + oh["triangle_index"][om]).all(), what
    assert (rec["t"][gm] == oh["t"][om]).all() and (rec["u"][gm] == oh["u"][om]).all() and (rec["v"][gm] == oh["v"][om]).all(), what
    return blob, rec


def _one_leaf_blob(oracle, tris):
    return oracle.leaf_chain_blobs(np.asarray(tris, np.float32).reshape(-1, 3, 3), chunk=63)[0]


@pytest.fixture(scope="module")
def soup63():
    return synth.triangle_soup(63, 0.3, seed=41)


@pytest.mark.parametrize("max_leaf", [3, 1, 62, 63])
def test_one_leaf_of_63_triangles(api, oracle, soup63, max_leaf):
    blob = _one_leaf_blob(oracle, soup63)
    ds = api.DeviceScene.upload(blob)
    assert ds.info()["num_triangles"] == 63 and ds.info()["num_nodes"] == 1
    rays = synth.rays_config1(4096)
    before = ds.trace(rays, full=False)
    hash_before = _valid(ds)["content_hash"]
    order_before = ds.primitive_order().copy()
    s = ds.split_leaves(max_leaf)
    c = _valid(ds)
    assert c["triangles_checked"] == 63
    assert s["max_leaf"] == max_leaf and s["largest_leaf_before"] == 63 and s["max_depth_before"] == 1
    info = ds.info()
    if max_leaf == 63:
        # nothing to split: no bit changes
        assert s["leaves_split"] == 0 and s["nodes_added"] == 0 and c["content_hash"] == hash_before
        assert info["num_nodes"] == 1 and info["max_depth"] == 1 and s["largest_leaf_after"] == 63
        assert (ds.primitive_order() == order_before).all()
    else:
        assert s["leaves_split"] == 1 and s["nodes_added"] >= 1 and c["content_hash"] != hash_before
        assert info["num_nodes"] == 1 + s["nodes_added"] and info["node_bytes"] == 128 * info["num_nodes"]
        assert s["largest_leaf_after"] <= max_leaf
        assert sorted(ds.primitive_order()) == sorted(order_before)
    exported, rec = _exact_against_exported_blob(oracle, ds, rays, "one leaf, max_leaf %d" % max_leaf)
    assert oracle.validate_blob(exported)[0] == 0
    leaves, deepest, nodes = _blob_tree(exported.data)
    assert sum(leaves) == 63 and max(leaves) <= max_leaf and nodes == info["num_nodes"]
    cap = _level_cap(63, max_leaf)
    assert deepest == info["max_depth"] == s["max_depth_after"] and deepest <= 1 + cap
    assert info["stack_entries"] == 3 * info["max_depth"] + 1
    # against the trace from before the split: the same rays hit, t within 1e-5
    gm, bm = rec["prim"] != NONE, before["prim"] != NONE
    assert (gm == bm).all() and bm.sum() > 100
    assert np.allclose(rec["t"][gm], before["t"][bm], rtol=1e-5, atol=0)
    # a second call with the same limit has nothing to do
    s2 = ds.split_leaves(max_leaf)
    assert s2["leaves_split"] == 0 and s2["nodes_added"] == 0 and _valid(ds)["content_hash"] == c["content_hash"]


@pytest.fixture(scope="module")
def cfg1_blob(oracle):
    return oracle.build_scene([dict(positions=synth.scene_for_config(1))])


def test_mixed_leaf_sizes(api, oracle, golden_dir, cfg1_blob):
    """The oracle's own build of the 10k-triangle scene (leaves of 4 to 63), split at 0 = the device builder's 3."""
    ds = api.DeviceScene.upload(cfg1_blob)
    before = ds.info()
    frame = synth.rays_pinhole(128, 128)
    fopts = api.make_opts(image=(128, 128))
    _, pk_before = ds.trace_packet_counted(frame, fopts)
    s = ds.split_leaves(0)
    assert s["max_leaf"] == 3 and s["leaves_split"] > 100 and 3 < s["largest_leaf_before"] <= 63 and s["largest_leaf_after"] <= 3
    c = _valid(ds)
    assert c["triangles_checked"] == 10000
    info = ds.info()
    assert info["num_nodes"] == before["num_nodes"] + s["nodes_added"] and info["node_bytes"] == 128 * info["num_nodes"]
    assert info["max_depth"] == s["max_depth_after"] and s["max_depth_before"] == before["max_depth"]
    assert info["max_depth"] <= before["max_depth"] + _level_cap(s["largest_leaf_before"], 3)
    assert info["stack_entries"] == 3 * info["max_depth"] + 1 and info["total_device_bytes"] > before["total_device_bytes"]
    assert info["num_triangles"] == 10000
    rays = synth.rays_config1(65536)
    exported = _as_blob(oracle, ds.export_blob())
    assert oracle.validate_blob(exported)[0] == 0
    leaves, deepest, nodes = _blob_tree(exported.data)
    assert sum(leaves) == 10000 and max(leaves) <= 3 and nodes == info["num_nodes"] and deepest == info["max_depth"]
    hits, mask, rec = ds.trace(rays)
    oh, om = oracle.trace(exported, rays)
    st = compare_hits(mask, hits["mesh_index"], hits["triangle_index"], hits["t"], hits["u"], hits["v"],
                      om, oh["mesh_index"], oh["triangle_index"], oh["t"], oh["u"], oh["v"], "split blob vs oracle on the exported blob")
    assert st["bit_exact"] == 1.0
    assert (hits["vertex"]["index"][mask] == oh["vertex"]["index"][om]).all()
    compare_hits_struct(hits, mask, load_golden(golden_dir, "cfg1_full.npz"), "split blob vs reference fixture")
    # what the leaf size decides: the hand-written packet kernel keeps its tiles, tests fewer triangles, and any-hit frames
    # run on it
    prec, pk_after = ds.trace_packet_counted(frame, fopts)
    assert pk_after["tiles_handed_back"] <= pk_before["tiles_handed_back"]
    assert pk_after["triangle_group_tests"] < pk_before["triangle_group_tests"]
    foh, fom = oracle.trace(exported, frame)
    assert ((prec["prim"] != NONE) == fom).all() and (prec["t"][fom] == foh["t"][fom]).all()
    assert (ds.trace_any(frame, opts=fopts) == fom).all()


def test_identity_and_filters(api, oracle):
    """A random multi-mesh scene through the CPU task builder, uploaded and split: the full rtk_hit (mesh, triangle, the three
    vertices and their indices) and the device filters against the oracle on the exported blob."""
    from tests.util import random_mixed_scene
    desc, keep, tris, mesh_index, tri_index, vidx = random_mixed_scene(3)
    L = api.lib()
    assert L.rtk_amd_set_builder(1) == 0
    try:
        scene = L.rtk_build_scene(C.byref(desc))
    finally:
        L.rtk_amd_set_builder(0)
    assert scene, api.last_error()
    try:
        ds = api.DeviceScene.upload(_as_blob(oracle, api.scene_bytes(scene)))
    finally:
        api.free_scene(scene)
    s = ds.split_leaves(0)
    assert s["leaves_split"] > 0 and s["largest_leaf_after"] <= 3
    c = _valid(ds)
    assert c["triangles_checked"] == len(tris)
    assert sorted(ds.primitive_order()) == list(range(len(tris)))
    exported = _as_blob(oracle, ds.export_blob())
    assert oracle.validate_blob(exported)[0] == 0
    rays = synth.rays_config1(8192, seed=23)
    hits, mask, plain = ds.trace(rays)
    oh, om = oracle.trace(exported, rays)
    assert (mask == om).all() and mask.sum() > 100
    for k in ("mesh_index", "triangle_index", "t", "u", "v"):
        assert (hits[k][mask] == oh[k][om]).all(), k
    assert (hits["vertex"]["index"][mask] == oh["vertex"]["index"][om]).all()
    assert (hits["vertex"]["position"][mask] == oh["vertex"]["position"][om]).all()
    # ... and they are the caller's triangles
    base = ds.mesh_base()
    prim = (base[hits["mesh_index"][mask].astype(np.int64)] + hits["triangle_index"][mask]).astype(np.int64)
    assert (plain["prim"][mask] == prim).all()
    assert (np.sort(hits["vertex"]["index"][mask], axis=1) == np.sort(vidx[prim], axis=1)).all()

    def check(rec, fh, fm, what):
        gm = rec["prim"] != NONE
        assert (gm == fm).all(), what
        assert (rec["prim"][gm] == base[fh["mesh_index"][fm].astype(np.int64)] + fh["triangle_index"][fm]).all(), what
        assert (rec["t"][gm] == fh["t"][fm]).all() and (rec["u"][gm] == fh["u"][fm]).all(), what

    num_meshes = len(base) - 1
    vis = [m % 2 == 0 for m in range(num_meshes)]
    check(ds.trace_filtered(rays, mesh_mask=vis), *oracle.trace_filtered(exported, rays, mesh_mask=vis), "mesh mask")
    hit = plain["prim"] != NONE
    pm = np.where(hit, np.searchsorted(base, np.where(hit, plain["prim"], 0), side="right") - 1, NONE).astype(np.uint32)
    pt = np.where(hit, plain["prim"] - base[np.where(hit, pm, 0).astype(np.int64)], 0).astype(np.uint32)
    check(ds.trace_filtered(rays, ignore_prim=plain["prim"].copy()), *oracle.trace_filtered(exported, rays, ignore=(pm, pt)), "ignore")
    check(ds.trace_filtered(rays, after=plain), *oracle.trace_filtered(exported, rays, after=(plain["t"], pm, pt)), "after")


def _degenerate(kind, oracle):
    if kind == "identical":
        one = np.array([[0.2, 0.2, 0.5], [0.8, 0.3, 0.5], [0.4, 0.9, 0.6]], np.float32)
        return _one_leaf_blob(oracle, np.repeat(one[None], 63, axis=0))
    x = np.ldexp(np.float32(1.0), np.arange(63) - 40).astype(np.float32)
    tris = np.zeros((63, 3, 3), np.float32)
    tris[:, :, 0] = x[:, None]
    tris[:, 1, 0] *= np.float32(1.01)
    tris[:, 1, 1] = np.float32(0.01) * x
    tris[:, 2, 2] = np.float32(0.01) * x
    tris = tris[(np.arange(63) * 29) % 63]                      # (slot order is not the line's order)
    blob = _one_leaf_blob(oracle, tris)
    if kind == "nonfinite":
        # the blob's boxes stay finite (the leaf is not an empty slot to the loader); the vertices behind them do not
        vo = int(np.frombuffer(blob.data, "<u8", 1, 48)[0])
        v = blob.data[vo:vo + 16 * 189].view("<f4").reshape(189, 4)
        v[5, 0] = np.nan
        v[40, 1] = np.inf
        v[100, 2] = -np.inf
        v[101, 0] = np.float32(3.0e38)
    return blob


@pytest.mark.parametrize("kind", ["identical", "geometric", "nonfinite"])
@pytest.mark.parametrize("max_leaf", [1, 3])
def test_degenerate_leaves(api, oracle, kind, max_leaf):
    ds = api.DeviceScene.upload(_degenerate(kind, oracle))
    assert ds.info()["num_triangles"] == 63
    s = ds.split_leaves(max_leaf)
    assert s["leaves_split"] == 1 and s["largest_leaf_after"] <= max_leaf
    assert sorted(ds.primitive_order()) == list(range(63))
    info = ds.info()
    assert info["max_depth"] == s["max_depth_after"] <= 1 + _level_cap(63, max_leaf)
    assert info["num_nodes"] == 1 + s["nodes_added"] and s["nodes_added"] <= 62
    if kind == "identical":
        assert (ds.primitive_order() == np.arange(63)).all()    # every cost ties: slot order survives
    if kind != "nonfinite":
        c = _valid(ds)
        assert c["triangles_checked"] == 63
        _exact_against_exported_blob(oracle, ds, synth.rays_config1(2048), kind)


def test_refit_around_a_split(api, oracle):
    """Two meshes. Refit, split, refit: exact boxes everywhere; the refit of one mesh after a split leaves the bits the full
    refit leaves (schedule and tables are made anew for the longer tree)."""
    a = synth.triangle_soup(4000, 0.08, seed=7)
    b = synth.triangle_soup(800, 0.08, seed=8) + np.float32(0.1)
    blob = oracle.build_scene([dict(positions=a), dict(positions=b)])
    b2 = (b * np.float32(1.05)).astype(np.float32)
    ds = api.DeviceScene.upload(blob)
    ds.refit([dict(positions=a), dict(positions=b)])              # (a schedule exists before the split)
    ds.refit([None, dict(positions=b)], only=[1])                 # (and the tables of the partial refit)
    bytes_with_tables = ds.info()["total_device_bytes"]
    s = ds.split_leaves(0)
    assert s["leaves_split"] > 0
    assert _valid(ds)["loose_boxes"] == 0
    assert ds.info()["total_device_bytes"] != bytes_with_tables
    ds.refit([dict(positions=a), dict(positions=b2)])
    c_full = _valid(ds)
    assert c_full["loose_boxes"] == 0 and c_full["nodes_checked"] == ds.info()["num_nodes"]
    assert ds.last_refit_nodes() == ds.info()["num_nodes"]
    other = api.DeviceScene.upload(blob)
    other.split_leaves(0)
    other.refit([dict(positions=a), dict(positions=b)])
    other.refit([None, dict(positions=b2)], only=[1])
    assert 0 < other.last_refit_nodes() < other.info()["num_nodes"]
    c_part = _valid(other)
    assert c_part["content_hash"] == c_full["content_hash"] and c_part["loose_boxes"] == 0
    rays = synth.rays_config1(8192)
    assert ds.trace(rays, full=False).tobytes() == other.trace(rays, full=False).tobytes()
    _exact_against_exported_blob(oracle, ds, rays, "refit after a split")


def test_quality_around_a_split(api, cfg1_blob):
    ds = api.DeviceScene.upload(cfg1_blob)
    q0 = ds.quality()
    assert q0["sah_cost_at_build"] == q0["sah_cost"] > 0
    ds.split_leaves(0)
    q1 = ds.quality()
    assert q1["triangle_tests"] < q0["triangle_tests"] and q1["node_visits"] > q0["node_visits"]
    # the old tree's cost is forgotten; this measurement, made before any refit, is the new one
    assert q1["sah_cost_at_build"] == q1["sah_cost"] != q0["sah_cost"]
    assert ds.quality()["sah_cost_at_build"] == q1["sah_cost"]
    # a scene that had a refit before the split has no cost "at build", as before
    tris = synth.scene_for_config(1)
    ds2 = api.DeviceScene.upload(cfg1_blob)
    ds2.refit([dict(positions=tris)])
    ds2.split_leaves(0)
    assert ds2.quality()["sah_cost_at_build"] == 0.0


def test_determinism_and_no_ops(api, oracle, cfg1_blob):
    a, b = api.DeviceScene.upload(cfg1_blob), api.DeviceScene.upload(cfg1_blob)
    sa, sb = a.split_leaves(0), b.split_leaves(0)
    ca, cb = _valid(a), _valid(b)
    assert ca["content_hash"] == cb["content_hash"]
    assert {k: v for k, v in sa.items() if k != "split_ms"} == {k: v for k, v in sb.items() if k != "split_ms"}
    assert (a.primitive_order() == b.primitive_order()).all()
    assert a.export_blob().tobytes() == b.export_blob().tobytes()
    # the replicas of a multi-GPU context
    L = api.lib()
    m = L.rtk_mgpu_create((C.c_int * 2)(0, 0), 2)
    assert m
    try:
        assert L.rtk_mgpu_split_leaves(m, 0) == -2                          # (no scene yet)
        assert L.rtk_mgpu_upload(m, C.c_void_p(cfg1_blob.ptr)) == 0, api.last_error()
        handles = [L.rtk_mgpu_scene(m, i) for i in range(2)]
        assert L.rtk_mgpu_split_leaves(m, 0) == 0, api.last_error()
        assert [L.rtk_mgpu_scene(m, i) for i in range(2)] == handles
        for h in handles:
            c = api.SceneCheck()
            assert L.rtk_dev_scene_validate(h, C.byref(c)) == 0, api.last_error()
            assert c.content_hash == ca["content_hash"]
        rays = synth.rays_config1(16384)
        got = np.zeros(len(rays), HIT_RECORD_DTYPE)
        assert L.rtk_mgpu_trace_rays(m, rays.ctypes.data, len(rays), got.ctypes.data, None) == 0, api.last_error()
        assert got.tobytes() == a.trace(rays, full=False).tobytes()
    finally:
        L.rtk_mgpu_destroy(m)
    # a device-built scene has nothing to split
    built = api.DeviceScene.build([dict(positions=synth.scene_for_config(1))])
    h0 = _valid(built)["content_hash"]                                      # (the validator makes the side arrays: counted from here on)
    before = built.info()
    s = built.split_leaves(0)
    assert s["leaves_split"] == 0 and s["nodes_added"] == 0 and s["largest_leaf_before"] <= 3
    assert _valid(built)["content_hash"] == h0 and built.info() == before
    # a scene without triangles
    empty = api.DeviceScene.build([dict(positions=np.zeros((0, 3), np.float32))])
    assert empty.split_leaves(0)["leaves_split"] == 0
