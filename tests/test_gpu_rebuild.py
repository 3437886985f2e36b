"""rtk_dev_scene_rebuild / rtk_mgpu_rebuild on the GPU: the device builder's tree over the triangles a scene holds now, under the
same handle.

The yardstick throughout is DeviceScene.build of the same positions: the rebuilt scene must be that scene bit for bit -- the
validator's content hash (every box, child word and triangle record), the slot order, the shape figures. Where hits are
checked, the authority is the oracle walking the blob exported after the rebuild (same tree: bit-exact)."""
import ctypes as C

import numpy as np
import pytest

from rtk_amd import synth
from rtk_amd.types import HIT_RECORD_DTYPE, MeshSet
from tests.test_gpu_refit import _all_paths_vs_oracle, _as_blob, deform

pytestmark = pytest.mark.gpu

ERR_BAD_ARG, ERR_UNSUPPORTED = -2, -6


def _valid(ds):
    ok, c = ds.validate()
    assert ok, c
    assert c["box_violations"] == 0 and c["compressed_node_errors"] == 0 and c["loose_boxes"] == 0, c
    return c


def _shape(ds):
    i = ds.info()
    return i["num_nodes"], i["max_depth"], i["stack_entries"], i["num_triangles"], i["node_bytes"]


def _info(ds):
    """info() without the one figure that describes a call, not the scene"""
    return {k: v for k, v in ds.info().items() if k != "build_ms"}


def _same_scene(rebuilt, fresh, what=""):
    """rebuilt is the scene `fresh` is: hash, slot order, shape; both validate with exact boxes"""
    assert _shape(rebuilt) == _shape(fresh), what
    assert (rebuilt.primitive_order() == fresh.primitive_order()).all(), what
    cr, cf = _valid(rebuilt), _valid(fresh)
    assert cr["content_hash"] == cf["content_hash"], what
    for k in ("nodes_checked", "leaves_checked", "triangles_checked"):
        assert cr[k] == cf[k], (what, k)
    return cr


def _soup(n, seed=17):
    return synth.triangle_soup(max(n, 1), 0.1 if n > 100 else 0.5, seed=seed)[:3 * n]


# ---------------------------------------------------------------------------------------------- 1 equal to a fresh build

def _build_refit_rebuild(api, n):
    v0 = _soup(n)
    v2 = deform(v0, 2)
    ds = api.DeviceScene.build([dict(positions=v0)])
    handle = ds.handle.value
    build_ms = ds.info()["build_ms"]
    ds.refit([dict(positions=v2)])
    before = ds.info()
    r = ds.rebuild()
    after = ds.info()                                        # (right after: nothing derived has been made yet)
    fresh = api.DeviceScene.build([dict(positions=v2)])
    assert after["total_device_bytes"] == fresh.info()["total_device_bytes"]
    assert ds.handle.value == handle and after["build_ms"] == build_ms
    assert r["nodes_before"] == before["num_nodes"] and r["nodes_after"] == after["num_nodes"]
    assert r["max_depth_before"] == before["max_depth"] and r["max_depth_after"] == after["max_depth"]
    assert r["rebuild_ms"] > 0.0 and r["key_bits"] in (24, 32, 40, 63)
    _same_scene(ds, fresh, "n = %d" % n)
    return ds, fresh, v2


@pytest.mark.parametrize("n", [2, 3, 4, 1023, 1024, 1025, 3000])
def test_equal_to_a_fresh_build(api, n):
    """build(V0), refit(deform(V0, 2)), rebuild() against build(deform(V0, 2)), at sizes on the borders of the refit tile of
    1024 triangles and over three tiles."""
    ds, fresh, v2 = _build_refit_rebuild(api, n)
    rays = synth.rays_config1(4096)
    assert ds.trace(rays, full=False).tobytes() == fresh.trace(rays, full=False).tobytes()


@pytest.mark.parametrize("knob,value", [("RTK_AMD_TILE_COLLAPSE_MIN", "0"), ("RTK_AMD_SORT_PACKED", "0"), ("RTK_AMD_NODE_ESTIMATE_DIV", "16"),
                                        ("RTK_AMD_FUSED_EMIT", "0")])
def test_equal_under_the_builders_knobs(api, monkeypatch, knob, value):
    """The same at 3000 triangles with the tile collapse, the (key, index) pair sort, a node estimate that is too small and
    the emit pass of its own: the knobs are read per build, by the rebuild as by the fresh build."""
    monkeypatch.setenv(knob, value)
    ds, fresh, _ = _build_refit_rebuild(api, 3000)
    if knob == "RTK_AMD_SORT_PACKED":
        assert ds.rebuild()["key_bits"] == 63
    if knob == "RTK_AMD_TILE_COLLAPSE_MIN":
        # the smallest size with two refit tiles: the tiles' run of node numbers ends at first_top, which is not 0 here and
        # arrives with the rest of the tree's record (the validator is given it: _same_scene)
        ds, fresh, _ = _build_refit_rebuild(api, 1025)
        i_rebuilt, i_fresh = _info(ds), _info(fresh)
        print("rebuilt", i_rebuilt, "fresh", i_fresh)
        assert i_rebuilt == i_fresh


# ---------------------------------------------------------------------------------------------- 2 indexed and mixed meshes

def _grid_mesh(side, z, dtype=np.float32):
    """(side x side vertices on a wavy sheet, two triangles per cell as uint16 indices): every inner vertex is shared by six"""
    u, v = np.meshgrid(np.linspace(0.05, 0.95, side), np.linspace(0.05, 0.95, side), indexing="ij")
    pos = np.stack([u, v, z + 0.05 * np.sin(7 * u) * np.cos(5 * v)], axis=-1).reshape(-1, 3).astype(dtype)
    i, j = np.meshgrid(np.arange(side - 1), np.arange(side - 1), indexing="ij")
    a = (i * side + j).reshape(-1)
    idx = np.concatenate([np.stack([a, a + side, a + 1], 1), np.stack([a + 1, a + side, a + side + 1], 1)]).astype(np.uint16)
    return pos, idx


def test_indexed_and_mixed_meshes(api, oracle):
    """u16 indices over shared vertices next to implicit indices over float64 positions: after refit and rebuild the scene is
    the fresh build of the float32 casts, and the full rtk_hit carries the caller's vertex indices and the current positions."""
    ga, ia = _grid_mesh(40, 0.45)
    sb = (synth.triangle_soup(1500, 0.08, seed=5).astype(np.float64) * 0.9 + 0.05)
    ga2 = deform(ga, 2)
    sb2 = deform(sb, 2)
    ds = api.DeviceScene.build([dict(positions=ga, indices=ia), dict(positions=sb)])
    ds.refit([dict(positions=ga2, indices=ia), dict(positions=sb2)])
    ds.rebuild()
    after = ds.info()
    fresh = api.DeviceScene.build([dict(positions=ga2.astype(np.float32), indices=ia), dict(positions=sb2.astype(np.float32))])
    assert after["total_device_bytes"] == fresh.info()["total_device_bytes"] and after["num_meshes"] == 2
    assert (ds.mesh_base() == fresh.mesh_base()).all()
    _same_scene(ds, fresh, "indexed + f64")
    _all_paths_vs_oracle(api, oracle, ds, [ga2, sb2], rays_scale=4)


# ---------------------------------------------------------------------------------------------- 3 a blob gets the device tree

@pytest.fixture(scope="module")
def cfg1_blob(oracle):
    return oracle.build_scene([dict(positions=synth.scene_for_config(1))])


@pytest.fixture(scope="module")
def cfg1_fresh(api):
    """(content hash, slot order, shape, info() right after the build, the validator's counts) of DeviceScene.build of the
    config 1 triangles: made once"""
    fresh = api.DeviceScene.build([dict(positions=synth.scene_for_config(1))])
    info = _info(fresh)
    c = _valid(fresh)
    return c["content_hash"], fresh.primitive_order().copy(), _shape(fresh), info, c


@pytest.mark.parametrize("split_first", [False, True])
def test_blob_gets_the_device_tree(api, oracle, cfg1_blob, cfg1_fresh, split_first):
    tris = synth.scene_for_config(1)
    ds = api.DeviceScene.upload(cfg1_blob)
    if split_first:
        assert ds.split_leaves(0)["leaves_split"] > 0
    uploaded = ds.info()
    r = ds.rebuild()
    rebuilt = _info(ds)                                      # (right after: nothing derived has been made yet)
    assert r["nodes_before"] == uploaded["num_nodes"] and r["nodes_after"] == rebuilt["num_nodes"]
    want_hash, want_order, want_shape, want_info, want_counts = cfg1_fresh
    # Every figure of info() is the fresh build's. One of them is so by its own rule: a blob's vertex indices are staged in input
    # order for the side arrays made later (12 bytes per triangle, rtk_scene_mem.h), which a build from implicit indices never
    # holds; that difference is exact and the only one.
    print("rebuilt", rebuilt, "fresh", want_info)
    assert rebuilt["total_device_bytes"] == want_info["total_device_bytes"] + 12 * rebuilt["num_triangles"]
    assert dict(rebuilt, total_device_bytes=want_info["total_device_bytes"]) == want_info
    assert _shape(ds) == want_shape and (ds.primitive_order() == want_order).all()
    c = _valid(ds)                                           # (first_split is back to 0: the validator holds every node to the builder's numbering)
    assert c == want_counts
    assert c["content_hash"] == want_hash and c["triangles_checked"] == 10000
    _all_paths_vs_oracle(api, oracle, ds, [tris], rays_scale=4)
    # a second rebuild of what is now a device tree changes no bit
    ds.rebuild()
    assert _valid(ds)["content_hash"] == want_hash


# ---------------------------------------------------------------------------------------------- 4 clustered scene

def test_clustered_scene_is_rebuilt_with_wide_keys(api):
    """The input of test_gpu_build.test_clustered_scene_is_rebuilt_with_wide_keys: more than an eighth of the sorted
    neighbours share a 32-bit code, so the rebuild, like the build, runs once more with 40 bits."""
    n = 200_000
    dense = (synth.triangle_soup(n, 0.03, seed=31).reshape(-1, 3) * np.float32(0.01) + np.float32(0.495)).astype(np.float32)
    far = np.array([[-1, -1, -1], [-1, -1, -0.99], [-1, -0.99, -1], [2, 2, 2], [2, 2, 2.01], [2, 2.01, 2]], np.float32)
    tris = np.ascontiguousarray(np.concatenate([dense, far]))
    ds = api.DeviceScene.build([dict(positions=tris)])
    want = _valid(ds)["content_hash"]
    order = ds.primitive_order().copy()
    r = ds.rebuild()
    assert r["key_bits"] == 40
    c = _valid(ds)
    assert c["content_hash"] == want and c["triangles_checked"] == n + 2
    assert (ds.primitive_order() == order).all()


# ---------------------------------------------------------------------------------------------- 5 the loop goes on

def test_the_loop_goes_on(api):
    a = synth.triangle_soup(2500, 0.08, seed=7)
    b = synth.triangle_soup(600, 0.08, seed=8) + np.float32(0.1)
    a2, b2 = deform(a, 2), deform(b, 2)
    b3 = (b2 * np.float32(1.05)).astype(np.float32)
    ds = api.DeviceScene.build([dict(positions=a), dict(positions=b)])
    q_built = ds.quality()
    ds.refit([dict(positions=a2), dict(positions=b2)])
    q_moved = ds.quality()
    assert q_moved["sah_cost_at_build"] == q_built["sah_cost"]
    ds.rebuild()
    fresh = api.DeviceScene.build([dict(positions=a2), dict(positions=b2)])
    q_fresh = fresh.quality()
    q = ds.quality()
    print("sah_cost: built %.6g, after the refit %.6g, after the rebuild %.6g" % (q_built["sah_cost"], q_moved["sah_cost"], q["sah_cost"]))
    # never refitted again: this measurement is the new tree's cost at build, bit for bit the fresh build's first
    assert q["sah_cost"] == q_fresh["sah_cost"] and q["sah_cost_at_build"] == q_fresh["sah_cost_at_build"] == q_fresh["sah_cost"]
    assert ds.quality()["sah_cost_at_build"] == q["sah_cost"]
    h = _valid(ds)["content_hash"]
    assert h == _valid(fresh)["content_hash"]
    # a refit to where the triangles are changes no bit; then the ratio has a baseline again
    ds.refit([dict(positions=a2), dict(positions=b2)])
    assert _valid(ds)["content_hash"] == h
    assert ds.quality()["sah_cost_at_build"] == q["sah_cost"]
    # a refit of one mesh leaves the bits the full refit leaves (schedule and tables are made anew for the new tree)
    fresh.refit([dict(positions=a2), dict(positions=b3)])
    ds.refit([None, dict(positions=b3)], only=[1])
    assert 0 < ds.last_refit_nodes() < ds.info()["num_nodes"]
    c_part, c_full = _valid(ds), _valid(fresh)
    assert c_part["content_hash"] == c_full["content_hash"] != h
    # a second rebuild right after the first changes no bit
    ds.rebuild()
    h2 = _valid(ds)["content_hash"]
    order2 = ds.primitive_order().copy()
    ds.rebuild()
    assert _valid(ds)["content_hash"] == h2 and (ds.primitive_order() == order2).all()
    rays = synth.rays_config1(8192)
    again = api.DeviceScene.build([dict(positions=a2), dict(positions=b3)])
    assert ds.trace(rays, full=False).tobytes() == again.trace(rays, full=False).tobytes()
    assert api.lib().rtk_dev_trace_status(ds.handle, None) == 0


# ---------------------------------------------------------------------------------------------- 6 no-ops and refusals

@pytest.mark.parametrize("n", [0, 1])
def test_tiny_scenes_are_left_alone(api, n):
    v = _soup(n) if n else np.zeros((0, 3), np.float32)
    ds = api.DeviceScene.build([dict(positions=v)])
    ok, c0 = ds.validate()
    assert ok
    before = ds.info()
    r = ds.rebuild()
    assert r["nodes_before"] == r["nodes_after"] == before["num_nodes"] and r["key_bits"] == 0
    ok, c = ds.validate()
    assert ok and c["content_hash"] == c0["content_hash"] and ds.info() == before


def _leaves(buf):
    """[(offset of the leaf header, count)] of a blob's leaves (nodes from byte 128 on, 96 bytes of boxes and
    four 64-bit child offsets, bit 0 = leaf; the count in the low six bits of the leaf's first word)"""
    out, todo = [], [128]
    while todo:
        off = todo.pop()
        box = np.frombuffer(buf, "<f4", 24, off).reshape(3, 2, 4)
        child = np.frombuffer(buf, "<u8", 4, off + 96)
        for k in range(4):
            if (box[:, 0, k] <= box[:, 1, k]).all():
                p = int(child[k])
                if p & 1:
                    out.append((p ^ 1, int(np.frombuffer(buf, "<u8", 1, p ^ 1)[0]) & 0x3F))
                else:
                    todo.append(p)
    return out


def _refused(api, ds):
    ok0, c0 = ds.validate()
    before, order = ds.info(), ds.primitive_order().copy()
    info = api.RebuildInfo()
    info.struct_size = C.sizeof(api.RebuildInfo)
    assert api.lib().rtk_dev_scene_rebuild(ds.handle, C.byref(info), None) == ERR_UNSUPPORTED
    why = api.last_error()
    ok, c = ds.validate()
    assert (ok, c) == (ok0, c0) and ds.info() == before and (ds.primitive_order() == order).all()
    return why


def test_not_one_record_per_primitive_is_refused(api, oracle, cfg1_blob):
    """Two blobs that upload and do not hold one record per primitive. (1) A leaf's count lowered by one (a leaf whose count
    is not 1 mod 4, so that the mesh table behind its triangles stays where it is): 9999 records for 10000 ids, refused on
    the host. (2) One triangle of a leaf given its neighbour's id: 10000 records, one id twice and one never, counted by the
    staging pass. Either way -6, and no bit of the scene changes."""
    data = np.array(cfg1_blob.data, copy=True)
    off, cnt = next((o, c) for o, c in _leaves(data) if c >= 2 and c % 4 != 1)
    ids = data[off + 8:off + 8 + 8 * cnt].view("<u4")[1::2]
    assert 9999 not in ids[-2:]                              # (the largest id stays: the number of primitives does)
    short = data.copy()
    short[off:off + 8].view("<u8")[0] -= 1
    ds = api.DeviceScene.upload(_as_blob(oracle, short))
    assert ds.info()["num_triangles"] == 9999
    assert "9999 triangle records for 10000 primitives" in _refused(api, ds)
    twice = data.copy()
    twice[off + 8:off + 8 + 8 * cnt].view("<u4")[2 * cnt - 1] = ids[cnt - 2]
    ds = api.DeviceScene.upload(_as_blob(oracle, twice))
    assert ds.info()["num_triangles"] == 10000
    assert "1 of 10000 primitives" in _refused(api, ds)
    # (and the blob as it came is rebuilt: the refusals above are the edits', not the scene's)
    good = api.DeviceScene.upload(_as_blob(oracle, data))
    good.rebuild()
    _valid(good)


# ---------------------------------------------------------------------------------------------- 7 replicas

def test_replicas(api):
    v0 = _soup(3000, seed=23)
    v2 = deform(v0, 2)
    want = _valid(api.DeviceScene.build([dict(positions=v2)]))["content_hash"]
    L = api.lib()
    m = L.rtk_mgpu_create((C.c_int * 2)(0, 0), 2)
    assert m
    try:
        assert L.rtk_mgpu_rebuild(m) == ERR_BAD_ARG                        # (no scene yet)
        ms0, ms2 = MeshSet([dict(positions=v0)]), MeshSet([dict(positions=v2)])
        assert L.rtk_mgpu_build(m, C.byref(ms0.desc)) == 0, api.last_error()
        handles = [L.rtk_mgpu_scene(m, i) for i in range(2)]
        assert L.rtk_mgpu_refit(m, C.byref(ms2.desc)) == 0, api.last_error()
        assert L.rtk_mgpu_rebuild(m) == 0, api.last_error()
        assert [L.rtk_mgpu_scene(m, i) for i in range(2)] == handles       # (the handles the host holds stay valid)
        for h in handles:
            c = api.SceneCheck()
            assert L.rtk_dev_scene_validate(h, C.byref(c)) == 0, api.last_error()
            assert c.content_hash == want and c.loose_boxes == 0
        rays = synth.rays_config1(16384)
        got = np.zeros(len(rays), HIT_RECORD_DTYPE)
        assert L.rtk_mgpu_trace_rays(m, rays.ctypes.data, len(rays), got.ctypes.data, None) == 0, api.last_error()
        assert got.tobytes() == api.DeviceScene.build([dict(positions=v2)]).trace(rays, full=False).tobytes()
    finally:
        L.rtk_mgpu_destroy(m)
