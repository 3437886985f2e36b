"""GPU tests of rtk_dev_scene_refit / rtk_mgpu_refit: new vertex positions for a finished device scene, in place.

The yardsticks: the device validator (every box the exact union of what is below it: loose_boxes == 0), its content hash
(boxes, child words, triangle records: a bit-level check of every box), the oracle walking the blob exported AFTER the
refit (same tree: bit-exact), and the oracle's own SAH build of the moved geometry (another tree: ids exact, t/u/v 1e-5)."""
import ctypes as C

import numpy as np
import pytest

from rtk_amd import synth
from rtk_amd.types import HIT_RECORD_DTYPE, MeshSet, RAY_DTYPE
from tests.util import compare_hits, load_golden

pytestmark = pytest.mark.gpu

ERROR_COUNTS = ("box_violations", "bad_references", "leaf_format_errors", "triangles_missing", "triangles_duplicated",
                "nodes_unreachable", "nodes_shared", "primitive_id_errors", "compressed_node_errors")


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


def _as_blob(oracle, arr):
    b = oracle._aligned_bytes(arr.size)
    b[:] = arr
    return oracle.Blob(b)


def _vs_oracle(hits, mask, ohits, omask, what):
    st = compare_hits(mask, hits["mesh_index"], hits["triangle_index"], hits["t"], hits["u"], hits["v"],
                      omask, ohits["mesh_index"], ohits["triangle_index"], ohits["t"], ohits["u"], ohits["v"], what)
    assert st["bit_exact"] == 1.0, what
    return st


def _records_vs_oracle(rec, ohits, omask, mesh_base, what):
    hit = rec["prim"] != 0xFFFFFFFF
    assert (hit == omask).all(), what
    want = mesh_base[ohits["mesh_index"][omask]] + ohits["triangle_index"][omask]
    assert (rec["prim"][hit] == want).all(), what
    for k in ("t", "u", "v"):
        assert rec[k][hit].tobytes() == ohits[k][omask].tobytes(), what + " " + k


def _all_paths_vs_oracle(api, oracle, ds, positions_of_mesh, rays_scale=1):
    """Every path that reads different data, bit-exact against the oracle on the blob exported now. positions_of_mesh[m]:
    the vertex array the scene was last given for mesh m (the full hit must carry THOSE positions under the caller's indices)."""
    blob = _as_blob(oracle, ds.export_blob())
    assert oracle.validate_blob(blob)[0] == 0
    mesh_base = ds.mesh_base()
    step = rays_scale
    # packet kernels: an image batch with the hint (128-byte nodes + order words)
    img = synth.rays_pinhole(256, 256)
    rec = ds.trace(img, opts=api.make_opts(image=(256, 256)), full=False)
    ohits, omask = oracle.trace(blob, img)
    _records_vs_oracle(rec, ohits, omask, mesh_base, "image batch")
    # per-lane assembly on compressed nodes; exact nodes; C++ kernels
    inc = synth.rays_incoherent(65536)[::step]
    ohits, omask = oracle.trace(blob, inc)
    for name, opts in (("per-lane", None), ("exact nodes", api.make_opts(exact_nodes=True)), ("no asm", api.make_opts(no_asm=True))):
        _records_vs_oracle(ds.trace(inc, opts=opts, full=False), ohits, omask, mesh_base, name)
    # any-hit
    sh = synth.rays_shadow(65536)[::step]
    _, smask = oracle.trace(blob, sh)
    assert (ds.trace_any(sh) == smask).all()
    # expansion to the full rtk_hit: the NEW positions under the caller's vertex indices
    c1 = synth.rays_config1(65536)[::step]
    hits, mask, _ = ds.trace(c1)
    ohits, omask = oracle.trace(blob, c1)
    _vs_oracle(hits, mask, ohits, omask, "full hits")
    assert (hits["vertex"]["index"][mask] == ohits["vertex"]["index"][omask]).all()
    assert hits["vertex"]["position"][mask].tobytes() == ohits["vertex"]["position"][omask].tobytes()
    for m, pos in enumerate(positions_of_mesh):
        sel = mask & (hits["mesh_index"] == m)
        if sel.any():
            want = np.asarray(pos)[hits["vertex"]["index"][sel]].astype(np.float32)
            assert (hits["vertex"]["position"][sel] == want).all()
    assert api.lib().rtk_dev_trace_status(ds.handle, None) == 0
    return blob


def _tree_shape(ds):
    i = ds.info()
    return ds.primitive_order().tobytes(), i["num_nodes"], i["max_depth"], i["stack_entries"], i["num_triangles"]


def _valid(ds):
    ok, c = ds.validate()
    assert ok, c
    assert c["box_violations"] == 0 and c["compressed_node_errors"] == 0 and c["loose_boxes"] == 0, c
    return c


def test_identity_refit_changes_no_bit(api, oracle):
    """build(V0), refit(V0): the hash (every box, child word and triangle record), the exported blob and the records are
    what they were."""
    v0 = synth.scene_for_config(1)
    ds = api.DeviceScene.build([dict(positions=v0)])
    c0 = _valid(ds)
    blob0 = ds.export_blob().tobytes()
    rays = synth.rays_config1(65536)
    rec0 = ds.trace(rays, full=False).tobytes()
    inc0 = ds.trace(synth.rays_incoherent(65536), full=False).tobytes()
    shape0 = _tree_shape(ds)
    assert ds.last_refit_ms() == 0.0
    ds.refit([dict(positions=v0)])
    assert ds.last_refit_ms() > 0.0
    c = _valid(ds)
    assert c["content_hash"] == c0["content_hash"] and c["nodes_checked"] == c0["nodes_checked"]
    assert ds.export_blob().tobytes() == blob0
    assert ds.trace(rays, full=False).tobytes() == rec0
    assert ds.trace(synth.rays_incoherent(65536), full=False).tobytes() == inc0
    assert _tree_shape(ds) == shape0


def test_there_and_back(api):
    v0 = synth.scene_for_config(1)
    ds = api.DeviceScene.build([dict(positions=v0)])
    h0 = _valid(ds)["content_hash"]
    ds.refit([dict(positions=deform(v0, 1))])
    h1 = _valid(ds)["content_hash"]
    assert h1 != h0                       # (the refit is not a no-op)
    ds.refit([dict(positions=v0)])
    assert _valid(ds)["content_hash"] == h0


def test_moved_geometry_same_tree(api, oracle):
    v0 = synth.scene_for_config(1)
    v1 = deform(v0, 1)
    ds = api.DeviceScene.build([dict(positions=v0)])
    shape0 = _tree_shape(ds)
    ds.refit([dict(positions=v1)])
    _valid(ds)
    assert _tree_shape(ds) == shape0
    _all_paths_vs_oracle(api, oracle, ds, [v1])


def test_moved_geometry_other_tree(api, oracle):
    """The refitted scene against the oracle's own SAH build of V1 (a different BVH): hit/miss and ids exact, t/u/v to the
    project's 1e-5 (430 of the 45 658 hits differ in the last bits of t between two oracle trees through the group-of-four
    rule). Two trees can disagree on a near-tie, so this (scene, rays, deformation) is one where two DIFFERENT oracle
    trees of V1 -- the SAH blob and the brute-force leaf chain -- agree on every mask and id; that is asserted first."""
    v0 = synth.scene_for_config(1)
    v1 = deform(v0, 1)
    rays = synth.rays_config1(65536)
    sah = oracle.build_scene([dict(positions=v1)])
    ohits, omask = oracle.trace(sah, rays)
    chits, cmask = oracle.trace_chain(oracle.leaf_chain_blobs(v1.reshape(-1, 3, 3)), rays)
    assert int(omask.sum()) == 45658
    assert (omask == cmask).all() and (ohits["triangle_index"][omask] == chits["triangle_index"][cmask]).all()
    ds = api.DeviceScene.build([dict(positions=v0)])
    ds.refit([dict(positions=v1)])
    hits, mask, _ = ds.trace(rays)
    compare_hits(mask, hits["mesh_index"], hits["triangle_index"], hits["t"], hits["u"], hits["v"],
                 omask, ohits["mesh_index"], ohits["triangle_index"], ohits["t"], ohits["u"], ohits["v"], "refit vs oracle build of V1")


@pytest.mark.parametrize("n,spread", [(0, 0.5), (2, 0.5), (3, 0.5), (1023, 0.1), (1024, 0.1), (1025, 0.1), (10_000, 0.05),
                                      (1_000_000, 0.02), (1_600_000, 0.02)])
def test_sizes(api, oracle, n, spread):
    """Identity, there and back, moved geometry at sizes that straddle the builder's boundaries (the refit tile of 1024;
    from about 1.5 M triangles on the tile collapse numbers the nodes in two runs)."""
    v0 = synth.triangle_soup(max(n, 1), spread, seed=17)[:3 * n]
    v1 = deform(v0, 1)
    ds = api.DeviceScene.build([dict(positions=v0)])
    c0 = _valid(ds)
    shape0 = _tree_shape(ds)
    blob0 = ds.export_blob().tobytes() if n <= 10_000 else None
    ds.refit([dict(positions=v0)])
    c = _valid(ds)
    assert c["content_hash"] == c0["content_hash"] and c["triangles_checked"] == n
    if blob0 is not None:
        assert ds.export_blob().tobytes() == blob0
    ds.refit([dict(positions=v1)])
    c1 = _valid(ds)
    assert _tree_shape(ds) == shape0
    if n:
        assert c1["content_hash"] != c0["content_hash"]
    if n:
        _all_paths_vs_oracle(api, oracle, ds, [v1], rays_scale=1 if n <= 10_000 else 8)
    else:
        assert (ds.trace(synth.rays_config1(2048), full=False)["prim"] == 0xFFFFFFFF).all()
    ds.refit([dict(positions=v0)])
    assert _valid(ds)["content_hash"] == c0["content_hash"]


@pytest.mark.parametrize("kind", ["numpy_f32", "numpy_f64", "torch_f32", "torch_f64", "strided_f32", "strided_f64"])
def test_position_inputs(api, oracle, kind):
    """The same positions through every form a position buffer may take: identity, moved geometry on the same tree
    (bit for bit the scene a plain float32 host array gives, and every trace path against the oracle), and back."""
    import torch
    v0 = synth.scene_for_config(1)
    v1 = deform(v0, 1)
    ref = api.DeviceScene.build([dict(positions=v0)])
    ref.refit([dict(positions=v1)])
    want = _valid(ref)["content_hash"]
    ds = api.DeviceScene.build([dict(positions=v0)])
    h0 = _valid(ds)["content_hash"]
    shape0 = _tree_shape(ds)
    dt = np.float64 if kind.endswith("f64") else np.float32

    def refit(v):
        if kind.startswith("numpy"):
            ds.refit([dict(positions=v.astype(dt))])
        elif kind.startswith("torch"):
            t = torch.from_numpy(v.astype(dt)).cuda()
            ds.refit([dict(positions=t)])
            assert t.cpu().numpy().tobytes() == v.astype(dt).tobytes()        # (read, not written)
        else:
            wide = np.full((len(v), 5), 7.0, dt)                              # x y z and two words nobody may read as positions
            wide[:, :3] = v
            ms = MeshSet([dict(positions=np.ascontiguousarray(wide[:, :3]))])
            ms._keep.append(wide)
            ms._arr[0].position.data = wide.ctypes.data
            ms._arr[0].position.stride = wide.strides[0]
            ds.refit(ms)
    refit(v0)
    assert _valid(ds)["content_hash"] == h0
    refit(v1)
    assert _valid(ds)["content_hash"] == want and want != h0
    assert _tree_shape(ds) == shape0
    _all_paths_vs_oracle(api, oracle, ds, [v1])
    refit(v0)
    assert _valid(ds)["content_hash"] == h0


def _edge_meshes(golden_dir):
    g = load_golden(golden_dir, "edge_cases.npz")
    t0 = g["tris"][g["mesh"] == 0].reshape(-1, 3)
    t1 = g["tris"][g["mesh"] == 1].reshape(-1, 3)
    p0, inv0 = np.unique(t0, axis=0, return_inverse=True)
    p1, inv1 = np.unique(t1, axis=0, return_inverse=True)
    return g, (p0.astype(np.float64), inv0.reshape(-1, 3).astype(np.uint16)), (p1.astype(np.float32), inv1.reshape(-1, 3).astype(np.uint32))


@pytest.mark.parametrize("where", ["host", "device"])
def test_indexed_multi_mesh(api, oracle, golden_dir, where):
    """u16 + float64 and u32 + float32 in one scene (both position formats in one launch); the triangles keep the vertex
    indices the scene recorded, so the refit is given positions only."""
    import torch
    g, (p0, i0), (p1, i1) = _edge_meshes(golden_dir)
    rays = np.ascontiguousarray(g["rays"]).view(RAY_DTYPE).reshape(-1)
    allp = np.concatenate([p0, p1.astype(np.float64)])
    ext = allp.max(0) - allp.min(0)
    ds = api.DeviceScene.build([dict(positions=p0, indices=i0), dict(positions=p1, indices=i1)])
    c0 = _valid(ds)
    shape0 = _tree_shape(ds)
    q0, q1 = deform(p0, 1, ext), deform(p1, 1, ext)
    assert q0.dtype == np.float64 and q1.dtype == np.float32
    if where == "host":
        new = [dict(positions=q0, indices=i0), dict(positions=q1, indices=i1)]
    else:
        new = [dict(positions=torch.from_numpy(q0).cuda(), indices=i0), dict(positions=torch.from_numpy(q1).cuda(), indices=i1)]
    ds.refit(new)
    c1 = _valid(ds)
    assert c1["content_hash"] != c0["content_hash"] and _tree_shape(ds) == shape0
    assert list(ds.mesh_base()) == [0, 8, 10]
    blob = _as_blob(oracle, ds.export_blob())
    hits, mask, _ = ds.trace(rays)
    ohits, omask = oracle.trace(blob, rays)
    _vs_oracle(hits, mask, ohits, omask, "indexed multi-mesh after refit")
    assert mask.any()
    assert (hits["vertex"]["index"][mask] == ohits["vertex"]["index"][omask]).all()
    for m, (q, idx) in enumerate(((q0, i0), (q1, i1))):
        sel = mask & (hits["mesh_index"] == m)
        for r in np.nonzero(sel)[0]:
            assert set(hits["vertex"]["index"][r]) == set(idx[hits["triangle_index"][r]])
        assert (hits["vertex"]["position"][sel] == q[hits["vertex"]["index"][sel]].astype(np.float32)).all()
    # the same scene as a build of the moved meshes sees it: the other tree
    other = oracle.build_scene([dict(positions=q0, indices=i0), dict(positions=q1, indices=i1)])
    bh, bm = oracle.trace(other, rays)
    assert (bm == mask).all()
    # and back
    ds.refit([dict(positions=p0, indices=i0), dict(positions=p1, indices=i1)])
    assert _valid(ds)["content_hash"] == c0["content_hash"]


def test_uploaded_blob_with_big_leaves(api, oracle):
    """An uploaded blob (the oracle's SAH build: leaves of 4 ... 63 triangles, boxes that need not be exact unions) is
    refitted like a device-built scene; afterwards its boxes ARE exact."""
    v0 = synth.scene_for_config(1)
    v1 = deform(v0, 1)
    ds = api.DeviceScene.upload(oracle.build_scene([dict(positions=v0)]))
    ok, c = ds.validate()
    assert ok, c
    shape0 = _tree_shape(ds)
    ds.refit([dict(positions=v1)])
    _valid(ds)
    assert _tree_shape(ds) == shape0
    _all_paths_vs_oracle(api, oracle, ds, [v1])


def test_non_finite_positions_and_back(api):
    """NaN / inf vertices: the refit treats them as a build does (fminf / fmaxf skip a NaN unless every member of the union
    is one -- the leaf of an all-NaN triangle gets a NaN box, which the validator reports for a build too; an inf
    travels up to the root), so the validator's verdict and its error counts are those of a BUILD of the same input
    (the two trees differ, so node and leaf totals and the hash are not compared); traces end without a stack error;
    finite positions next frame bring back the build's bits and the compressed nodes."""
    v0 = synth.scene_for_config(1)
    bad = v0.copy()
    bad[5, 0] = np.nan
    bad[3001] = np.nan
    bad[12000:12003] = np.nan          # a whole triangle
    bad[7777, 1] = np.inf
    bad[20001, 2] = -np.inf
    only_triangle = v0.copy()
    only_triangle[12000:12003] = np.nan    # (no inf anywhere: the compressed nodes stay in use, and are checked)
    ds = api.DeviceScene.build([dict(positions=v0)])
    h0 = _valid(ds)["content_hash"]
    inc = synth.rays_incoherent(65536)
    inc0 = ds.trace(inc, full=False).tobytes()
    # Which nodes a launch reads is visible in its visit counts, not in its records: the compressed boxes are a little
    # larger than the exact ones, so rays enter more of them.
    def visits(opts=None):             # (per-ray counts: they do not depend on how the rays were dealt to the waves)
        c = ds.trace_counted(inc, opts=opts)[1]
        return tuple(c[k] for k in ("rays", "nodes", "leaves", "triangles", "hits"))
    visits_q, visits_exact = visits(), visits(api.make_opts(exact_nodes=True))
    assert visits_q != visits_exact and visits_q[4] == visits_exact[4]
    for positions in (only_triangle, bad):
        okb, cb = api.DeviceScene.build([dict(positions=positions)]).validate()
        ds.refit([dict(positions=positions)])
        ok, c = ds.validate()
        assert ok == okb
        for k in ERROR_COUNTS + ("loose_boxes", "triangles_checked"):
            assert c[k] == cb[k], (k, c, cb)
    # (an inf plane does not fit the 8-bit grid: the default launch and the exact-nodes one now read the same nodes)
    assert visits() == visits(api.make_opts(exact_nodes=True))
    L = api.lib()
    for rays, opts in ((synth.rays_config1(65536), None), (inc, None), (synth.rays_pinhole(256, 256), api.make_opts(image=(256, 256)))):
        ds.trace(rays, opts=opts, full=False)
        assert L.rtk_dev_trace_status(ds.handle, None) == 0, api.last_error()
    ds.refit([dict(positions=v0)])
    assert _valid(ds)["content_hash"] == h0
    assert ds.trace(inc, full=False).tobytes() == inc0
    # ... and the launch reads the compressed nodes again (after the inf it was on its exact nodes)
    assert visits() == visits_q and visits(api.make_opts(exact_nodes=True)) == visits_exact


def test_refusals_leave_the_scene_alone(api):
    v0 = synth.scene_for_config(1)
    ds = api.DeviceScene.build([dict(positions=v0)])
    h0 = _valid(ds)["content_hash"]
    L = api.lib()

    def rc_of(ms):
        return L.rtk_dev_scene_refit(ds.handle, C.byref(ms.desc), None)
    assert rc_of(MeshSet([dict(positions=v0), dict(positions=v0[:3])])) == -2          # RTK_AMD_ERR_BAD_ARG: mesh count
    assert "meshes" in api.last_error()
    assert rc_of(MeshSet([dict(positions=v0[:-3])])) == -2                             # triangle count
    assert "triangles" in api.last_error()
    ms = MeshSet([dict(positions=v0)])
    ms._arr[0].position.type = 77
    assert rc_of(ms) == -2                                                             # unknown position type
    ms = MeshSet([dict(positions=v0)])
    ms._arr[0].position_cb = 1                                                         # (never called: refused before)
    assert rc_of(ms) == -6                                                             # RTK_AMD_ERR_UNSUPPORTED
    assert "callback" in api.last_error()
    with pytest.raises(api.RtkError):
        ds.refit([dict(positions=v0[:-3])])
    assert ds.last_refit_ms() == 0.0
    assert _valid(ds)["content_hash"] == h0


def test_virtual_shards(api):
    """rtk_mgpu_refit: three slots on device 0; every replica ends up as the single scene's refit."""
    v0 = synth.scene_for_config(1)
    v1 = deform(v0, 1)
    single = api.DeviceScene.build([dict(positions=v0)])
    single.refit([dict(positions=v1)])
    want = _valid(single)["content_hash"]
    L = api.lib()
    m = L.rtk_mgpu_create((C.c_int * 3)(0, 0, 0), 3)
    assert m
    try:
        ms0, ms1 = MeshSet([dict(positions=v0)]), MeshSet([dict(positions=v1)])
        assert L.rtk_mgpu_refit(m, C.byref(ms1.desc)) == -2                # (no scene yet)
        assert L.rtk_mgpu_build(m, C.byref(ms0.desc)) == 0, api.last_error()
        handles = [L.rtk_mgpu_scene(m, i) for i in range(3)]
        assert L.rtk_mgpu_refit(m, C.byref(ms1.desc)) == 0, api.last_error()
        assert [L.rtk_mgpu_scene(m, i) for i in range(3)] == handles       # (the handles the host holds stay valid)
        for i in range(3):
            c = api.SceneCheck()
            assert L.rtk_dev_scene_validate(handles[i], C.byref(c)) == 0, api.last_error()
            assert c.content_hash == want and c.loose_boxes == 0
        rays = synth.rays_config1(65536)
        got = np.zeros(len(rays), HIT_RECORD_DTYPE)
        assert L.rtk_mgpu_trace_rays(m, rays.ctypes.data, len(rays), got.ctypes.data, None) == 0, api.last_error()
        assert got.tobytes() == single.trace(rays, full=False).tobytes()
    finally:
        L.rtk_mgpu_destroy(m)


def test_two_streams_before_and_after(api, oracle):
    """A scene traced on two streams before the refit (two scratch sets exist) gives the new scene's records on both."""
    import torch
    v0 = synth.scene_for_config(1)
    v1 = deform(v0, 1)
    ds = api.DeviceScene.build([dict(positions=v0)])
    img = synth.rays_pinhole(256, 256)
    opts = api.make_opts(image=(256, 256))
    inc = synth.rays_incoherent(65536)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]

    def on_streams():
        out = []
        for s in streams:
            with torch.cuda.stream(s):
                out.append((ds.trace(img, opts=opts, full=False).tobytes(), ds.trace(inc, full=False).tobytes()))
            s.synchronize()
        return out
    before = on_streams()
    assert before[0] == before[1]
    torch.cuda.synchronize()
    ds.refit([dict(positions=v1)])
    after = on_streams()
    assert after[0] == after[1] and after[0] != before[0]
    blob = _as_blob(oracle, ds.export_blob())
    mesh_base = ds.mesh_base()
    for rays, raw in ((img, after[0][0]), (inc, after[0][1])):
        ohits, omask = oracle.trace(blob, rays)
        _records_vs_oracle(np.frombuffer(raw, HIT_RECORD_DTYPE), ohits, omask, mesh_base, "after the refit, on a stream that traced before it")
