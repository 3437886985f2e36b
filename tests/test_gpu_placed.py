"""GPU tests of the placed calls (rtk_dev_scene_build_placed, _refit_placed, _refit_meshes_placed and their rtk_mgpu forms): rest-pose
meshes plus a 3 x 4 matrix per mesh.

The yardstick is the TWIN: the rule of rtk_amd/csrc/rtk_place_rule.h applied in numpy (tests/test_place_cpu.py: place_np, which
that file ties to the header on the CPU) to every vertex of every mesh, as tightly packed float32 positions with the same index
buffers, sent through the unplaced sibling in the same process. The contract is bit identity, so nothing here has a tolerance."""
import ctypes as C

import numpy as np
import pytest

from rtk_amd import synth
from rtk_amd.types import HIT_DTYPE, HIT_RECORD_DTYPE, MeshSet
from tests.test_place_cpu import place_np

pytestmark = pytest.mark.gpu

ERR_BAD_ARG, ERR_UNSUPPORTED = -2, -6


def rot(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


def mat(linear, t):
    return np.concatenate([np.asarray(linear, np.float64), np.asarray(t, np.float64).reshape(3, 1)], 1).astype(np.float32)


ROT_TRANS = mat(rot([1, 2, 3], 0.7), [0.25, -0.5, 1.0])
SCALE_SHEAR = mat([[1.5, 0.3, 0.0], [0.0, 0.6, -0.2], [0.1, 0.0, 2.5]], [0.0, 0.125, -0.25])
REFLECT = mat(np.diag([-1.0, 1.0, 1.0]) @ rot([0, 1, 0], 0.3), [1.0, 0.0, 0.0])


def twin_of(meshes, placements):
    """Every mesh with float32 positions = the rule on every vertex of its buffer; indices as they are."""
    out = []
    for m, pl in zip(meshes, placements):
        p = m["positions"]
        p = p.cpu().numpy() if hasattr(p, "data_ptr") else np.asarray(p)
        t = dict(m)
        t["positions"] = np.ascontiguousarray(place_np(np.asarray(pl, np.float32).reshape(12), p[:, :3]))
        out.append(t)
    return out


def fingerprint(ds, finite=True):
    """Everything the contract names: validator counts and content hash, primitive order, exported blob, info without build_ms."""
    ok, c = ds.validate()
    if finite:
        assert ok and c["box_violations"] == 0 and c["loose_boxes"] == 0 and c["compressed_node_errors"] == 0, c
    info = ds.info()
    info.pop("build_ms")
    return dict(ok=ok, check=c, order=ds.primitive_order().tobytes(), blob=ds.export_blob().tobytes(), info=info)


def assert_same(a, b):
    for k in ("ok", "check", "info"):
        assert a[k] == b[k], (k, a[k], b[k])
    assert a["order"] == b["order"] and a["blob"] == b["blob"]


def padded(pos, dtype, words=5):
    """positions in a buffer of `words` numbers per vertex, of which only the first three are coordinates"""
    wide = np.full((len(pos), words), 7.0, dtype)
    wide[:, :3] = pos
    return wide


def set_stride(ms, i, wide):
    ms._keep.append(wide)
    ms._arr[i].position.data = wide.ctypes.data
    ms._arr[i].position.stride = wide.strides[0]


def test_build_equals_twin_three_formats(api):
    """F32 implicit (1 triangle), F64 + u16 + padded stride (65), F32 + u32 in device memory (1025): the edges of a wave and of
    the ingest's workgroup. A rotation with a translation, a non-uniform scale with shear, a reflection."""
    import torch
    rng = np.random.RandomState(3)
    p0 = synth.triangle_soup(1, 0.3, seed=5)
    p1 = rng.uniform(0, 1, (40, 3))
    i1 = rng.randint(0, 40, (65, 3)).astype(np.uint16)
    p2 = rng.uniform(0, 1, (700, 3)).astype(np.float32)
    i2 = rng.randint(0, 700, (1025, 3)).astype(np.int32)
    d_p2, d_i2 = torch.from_numpy(p2).cuda(), torch.from_numpy(i2).cuda()
    placements = np.stack([ROT_TRANS, SCALE_SHEAR, REFLECT])
    meshes = [dict(positions=p0), dict(positions=p1, indices=i1), dict(positions=d_p2, indices=d_i2)]
    ms = MeshSet(meshes)
    set_stride(ms, 1, padded(p1, np.float64))
    A = api.DeviceScene.build(ms, placements=placements)
    assert d_p2.cpu().numpy().tobytes() == p2.tobytes()               # (read, not written)
    tw = twin_of(meshes, placements)
    tw[2] = dict(positions=torch.from_numpy(tw[2]["positions"]).cuda(), indices=d_i2)
    B = api.DeviceScene.build(tw)
    fa, fb = fingerprint(A), fingerprint(B)
    assert fa["info"]["num_triangles"] == 1 + 65 + 1025 and fa["info"]["num_meshes"] == 3
    assert_same(fa, fb)
    # (12, ) rows instead of (3, 4) matrices, and the unplaced call is not the placed one
    assert_same(fingerprint(api.DeviceScene.build(ms, placements=placements.reshape(3, 12))), fb)
    assert fingerprint(api.DeviceScene.build(ms))["check"]["content_hash"] != fa["check"]["content_hash"]


def test_build_equals_twin_where_the_twin_is_gathered_in_place(api):
    """All meshes implicit float32 (host, device, padded stride): the twin's build gathers them in place from the caller's buffers
    (DIRECT), the placed build stages them; the same scene."""
    import torch
    v = synth.triangle_soup(3000, 0.05, seed=11)
    parts = [v[:3 * 1024], v[3 * 1024:3 * 1089], v[3 * 1089:]]
    placements = np.stack([REFLECT, ROT_TRANS, SCALE_SHEAR])
    d = torch.from_numpy(parts[1]).cuda()
    meshes = [dict(positions=parts[0]), dict(positions=d), dict(positions=parts[2])]
    ms = MeshSet(meshes)
    set_stride(ms, 2, padded(parts[2], np.float32, 4))
    A = api.DeviceScene.build(ms, placements=placements)
    B = api.DeviceScene.build(twin_of(meshes, placements))
    assert_same(fingerprint(A), fingerprint(B))


def test_host_decoded_meshes(api):
    """What the host decodes and places itself: a scene of one triangle, and a mesh whose indices come from a callback."""
    p = synth.triangle_soup(1, 0.3, seed=9)
    A = api.DeviceScene.build([dict(positions=p)], placements=SCALE_SHEAR[None])
    B = api.DeviceScene.build(twin_of([dict(positions=p)], [SCALE_SHEAR]))
    assert_same(fingerprint(A), fingerprint(B))
    rng = np.random.RandomState(5)
    pos = rng.uniform(0, 1, (50, 3))
    idx = rng.randint(0, 50, (200, 3)).astype(np.uint32)
    CB = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.c_size_t, C.c_size_t)

    def index_cb(user, mesh, out, offset, count):
        for k in range(3 * count):
            out[k] = int(idx.reshape(-1)[3 * offset + k])
    cb = CB(index_cb)
    other = synth.triangle_soup(100, 0.1, seed=2)
    ms = MeshSet([dict(positions=pos, indices=idx), dict(positions=other)])
    ms._arr[0].index.data = None
    ms._arr[0].index_cb = C.cast(cb, C.c_void_p)
    placements = np.stack([ROT_TRANS, REFLECT])
    A = api.DeviceScene.build(ms, placements=placements)
    B = api.DeviceScene.build(twin_of([dict(positions=pos, indices=idx), dict(positions=other)], placements))
    assert_same(fingerprint(A), fingerprint(B))


# ---- instances: one 500-triangle mesh, eight entries

REST = synth.triangle_soup(500, 0.15, seed=21)


def ring(phase, scale=0.3):
    """eight placements that put the unit-cube mesh, shrunk, near the eight corners of the unit cube, each turned its own way"""
    out = []
    for k in range(8):
        centre = np.array([k & 1, (k >> 1) & 1, (k >> 2) & 1], np.float64) * 0.6 + 0.2
        linear = scale * rot([1 + k, 2, 3 - k], 0.4 * k + phase)      # (about the middle of the rest pose's cube)
        out.append(mat(linear, centre - linear @ np.full(3, 0.5) + 0.02 * np.sin(phase + k)))
    return np.stack(out)


def instance_scenes(api, placements):
    meshes = [dict(positions=REST)] * 8                                # (eight entries, one buffer)
    ms = MeshSet(meshes)
    assert len({ms._arr[k].position.data for k in range(8)}) == 1
    A = api.DeviceScene.build(ms, placements=placements)
    B = api.DeviceScene.build(twin_of(meshes, placements))
    return meshes, A, B


def test_instances(api):
    placements = ring(0.0)
    meshes, A, B = instance_scenes(api, placements)
    assert_same(fingerprint(A), fingerprint(B))
    rays = synth.rays_pinhole(64, 64)
    placed = [place_np(placements[k].reshape(12), REST) for k in range(8)]
    for opts in (api.make_opts(image=(64, 64)), None):
        ha, ma, ra = A.trace(rays, opts=opts)
        hb, mb, rb = B.trace(rays, opts=opts)
        assert ra.tobytes() == rb.tobytes() and ha.tobytes() == hb.tobytes() and (ma == mb).all()
        assert ma.sum() > 100 and len(set(ha["mesh_index"][ma])) >= 2     # (the frame does see more than one instance)
        # the hit is the ENTRY's: its mesh number, its triangle, its vertex numbers, the placed positions the scene holds
        mesh, tri = ha["mesh_index"][ma].astype(np.int64), ha["triangle_index"][ma].astype(np.int64)
        assert (ra["prim"][ma] == 500 * mesh + tri).all()
        for c in range(3):
            assert (ha["vertex"]["index"][ma][:, c] == 3 * tri + c).all()
            want = np.stack([placed[m][3 * t + c] for m, t in zip(mesh, tri)])
            assert ha["vertex"]["position"][ma][:, c].tobytes() == want.tobytes()


def test_refit_placed_and_refit_meshes_placed(api):
    p0 = ring(0.0)
    meshes, A, B = instance_scenes(api, p0)
    num_nodes = A.info()["num_nodes"]
    h0 = fingerprint(A)["check"]["content_hash"]
    # all eight
    p1 = ring(0.5)
    A.refit(meshes, placements=p1)
    B.refit(twin_of(meshes, p1))
    fa, fb = fingerprint(A), fingerprint(B)
    assert_same(fa, fb)
    assert fa["check"]["content_hash"] != h0 and A.last_refit_nodes() == B.last_refit_nodes() == num_nodes and A.last_refit_ms() > 0.0
    # two of the eight, the others without positions; entries of unlisted meshes are not read (NaN would show)
    p2 = p1.copy()
    p2[[1, 6]] = ring(1.1)[[1, 6]]
    given = np.full_like(p2, np.nan)
    given[[1, 6]] = p2[[1, 6]]
    A.refit([meshes[k] if k in (1, 6) else None for k in range(8)], only=[1, 6], placements=given)
    tw = twin_of(meshes, p2)
    B.refit([tw[k] if k in (1, 6) else None for k in range(8)], only=[1, 6])
    fa, fb = fingerprint(A), fingerprint(B)
    assert_same(fa, fb)
    assert 0 < A.last_refit_nodes() == B.last_refit_nodes() < num_nodes
    # ... which is also what the full placed refit of all eight gives
    Cs = api.DeviceScene.build(twin_of(meshes, p0))
    Cs.refit(meshes, placements=p2)
    fc = fingerprint(Cs)                                              # (its info differs: it never made the per-mesh tables)
    assert fc["check"] == fa["check"] and fc["blob"] == fa["blob"] and fc["order"] == fa["order"]
    # three of the eight: above the quarter, the full passes
    p3 = p2.copy()
    p3[[0, 3, 5]] = ring(2.0)[[0, 3, 5]]
    A.refit([meshes[k] if k in (0, 3, 5) else None for k in range(8)], only=[0, 3, 5], placements=p3)
    tw = twin_of(meshes, p3)
    B.refit([tw[k] if k in (0, 3, 5) else None for k in range(8)], only=[0, 3, 5])
    assert_same(fingerprint(A), fingerprint(B))
    assert A.last_refit_nodes() == B.last_refit_nodes() == num_nodes
    # nothing listed: no bit, no work
    h = fingerprint(A)["check"]["content_hash"]
    A.refit([None] * 8, only=[], placements=p3)
    assert A.last_refit_nodes() == 0 and fingerprint(A)["check"]["content_hash"] == h
    # nothing is remembered: a plain refit takes its positions as given
    A.refit(meshes)
    B.refit(meshes)
    assert_same(fingerprint(A), fingerprint(B))


@pytest.mark.parametrize("fmt", ["f32_host", "f64_host_strided", "f64_device"])
def test_refit_placed_position_formats(api, fmt):
    """The refit's own gather (float / double / both in one launch), host-resident positions staged raw and placed on the device."""
    import torch
    v = synth.triangle_soup(2000, 0.05, seed=4)
    parts = [v[:3 * 700], v[3 * 700:3 * 1400], v[3 * 1400:]]
    base = [dict(positions=p) for p in parts]
    placements = np.stack([ROT_TRANS, SCALE_SHEAR, REFLECT])
    A, B = api.DeviceScene.build(base), api.DeviceScene.build(base)
    dt = np.float32 if fmt.startswith("f32") else np.float64
    rest = [p.astype(dt) for p in parts]
    rest[2] = rest[2].astype(np.float32)                              # (with f64 elsewhere: both formats in one launch)
    given = [dict(positions=torch.from_numpy(r).cuda()) if fmt.endswith("device") else dict(positions=r) for r in rest]
    ms = MeshSet(given)
    if fmt.endswith("strided"):
        set_stride(ms, 0, padded(rest[0], dt))
    A.refit(ms, placements=placements)
    B.refit(twin_of([dict(positions=r) for r in rest], placements))
    assert_same(fingerprint(A), fingerprint(B))
    # the listed form of the same kernels
    A.refit(ms, only=[0], placements=placements[::-1])
    B.refit([twin_of([dict(positions=rest[0])], [placements[2]])[0], None, None], only=[0])
    assert_same(fingerprint(A), fingerprint(B))


def test_denormals_are_kept_on_the_device(api):
    """Coordinates of 1e-10 under a scale of 1e-30: the positions the scene holds are numpy's denormals, not zeros."""
    rest = (synth.triangle_soup(200, 0.2, seed=8) * np.float32(1e-10)).astype(np.float32)
    pl = mat(np.diag([1e-30, 1e-30, 1e-30]), [0, 0, 0])[None]
    want = place_np(pl[0].reshape(12), rest)
    tiny = np.finfo(np.float32).tiny
    assert ((want != 0) & (np.abs(want) < tiny)).mean() > 0.9
    A = api.DeviceScene.build([dict(positions=rest)], placements=pl)
    B = api.DeviceScene.build([dict(positions=want)])
    assert_same(fingerprint(A, finite=False), fingerprint(B, finite=False))
    # every triangle's full hit, from a record that names it
    rec = np.zeros(200, HIT_RECORD_DTYPE)
    rec["t"], rec["u"], rec["v"], rec["prim"] = 1.0, 0.25, 0.25, np.arange(200)
    d_hits, d_mask = A.expand_device(api.to_device(rec), 200)
    hits = d_hits.cpu().numpy().view(HIT_DTYPE)
    assert d_mask.cpu().numpy().all() and (hits["triangle_index"] == np.arange(200)).all()
    assert hits["vertex"]["position"].tobytes() == want.reshape(200, 3, 3).tobytes()
    # and through the refit's gather
    A.refit([dict(positions=(rest * np.float32(0.5)).astype(np.float32))], placements=pl)
    d_hits, _ = A.expand_device(api.to_device(rec), 200)
    want2 = place_np(pl[0].reshape(12), (rest * np.float32(0.5)).astype(np.float32))
    assert ((want2 != 0) & (np.abs(want2) < tiny)).mean() > 0.9
    assert d_hits.cpu().numpy().view(HIT_DTYPE)["vertex"]["position"].tobytes() == want2.reshape(200, 3, 3).tobytes()


def test_non_finite_placements(api):
    """An inf entry (0 * inf: NaN) and a NaN entry: the calls succeed, and the validator counts what it counts for the twin."""
    v = synth.triangle_soup(1500, 0.05, seed=6)
    parts = [v[:3 * 500].copy(), v[3 * 500:3 * 1000], v[3 * 1000:]]
    parts[0][::7, 1] = 0.0                                            # (0 * inf)
    meshes = [dict(positions=p) for p in parts]
    placements = np.stack([ROT_TRANS, SCALE_SHEAR, REFLECT])
    placements[0, 0, 1] = np.inf
    placements[2, 1, 3] = np.nan
    tw = twin_of(meshes, placements)
    assert np.isnan(tw[0]["positions"]).any() and np.isnan(tw[2]["positions"][:, 1]).all() and np.isfinite(tw[1]["positions"]).all()

    def counts(ds):
        ok, c = ds.validate()
        c.pop("content_hash")                                         # (the payload of a NaN is not promised)
        return ok, c
    A = api.DeviceScene.build(meshes, placements=placements)
    B = api.DeviceScene.build(tw)
    assert counts(A) == counts(B) and A.info()["num_nodes"] == B.info()["num_nodes"]
    good = api.DeviceScene.build(meshes, placements=np.stack([ROT_TRANS, SCALE_SHEAR, REFLECT]))
    good2 = api.DeviceScene.build(twin_of(meshes, [ROT_TRANS, SCALE_SHEAR, REFLECT]))
    good.refit(meshes, placements=placements)
    good2.refit(tw)
    assert counts(good) == counts(good2)
    good.refit(meshes, only=[2], placements=placements)
    good2.refit([None, None, tw[2]], only=[2])
    assert counts(good) == counts(good2) and good.last_refit_nodes() == good2.last_refit_nodes()


def test_refusals_leave_the_scene_alone(api):
    L = api.lib()
    v = synth.triangle_soup(1200, 0.05, seed=12)
    parts = [v[:3 * 400], v[3 * 400:3 * 800], v[3 * 800:]]
    full = [dict(positions=p) for p in parts]
    placements = np.stack([ROT_TRANS, SCALE_SHEAR, REFLECT])
    ds = api.DeviceScene.build(full, placements=placements)
    h0 = fingerprint(ds)["check"]["content_hash"]
    ptr, keep = api.placement_ptr(placements, 3)
    ids = (C.c_uint32 * 1)(1)

    def both(ms, pl):
        return (L.rtk_dev_scene_refit_placed(ds.handle, C.byref(ms.desc), pl, None),
                L.rtk_dev_scene_refit_meshes_placed(ds.handle, C.byref(ms.desc), pl, ids, 1, None))
    assert both(MeshSet(full), None) == (ERR_BAD_ARG, ERR_BAD_ARG)                                  # NULL placements
    ms = MeshSet(full)
    ms._arr[1].position_cb = 1                                                                      # (never called: refused before)
    assert both(ms, ptr) == (ERR_UNSUPPORTED, ERR_UNSUPPORTED) and "callback" in api.last_error()
    assert both(MeshSet(full[:2] + [dict(positions=parts[2][:-3])]), ptr) == (ERR_BAD_ARG, ERR_BAD_ARG)   # a wrong triangle count
    assert "triangles" in api.last_error()
    assert both(MeshSet(full[:2]), ptr) == (ERR_BAD_ARG, ERR_BAD_ARG)                               # a wrong mesh count
    ms = MeshSet(full)
    ms._arr[1].position.data = None
    assert both(ms, ptr) == (ERR_BAD_ARG, ERR_BAD_ARG) and "no positions" in api.last_error()
    assert L.rtk_dev_scene_refit_meshes_placed(ds.handle, C.byref(MeshSet(full).desc), ptr, (C.c_uint32 * 1)(3), 1, None) == ERR_BAD_ARG
    assert ds.last_refit_ms() == 0.0 and ds.last_refit_nodes() == 0
    assert fingerprint(ds)["check"]["content_hash"] == h0
    # the build: no scene, and the reason
    ms = MeshSet(full)
    ms._arr[1].position_cb = 1
    assert not L.rtk_dev_scene_build_placed(C.byref(ms.desc), ptr) and "callback" in api.last_error()
    assert not L.rtk_dev_scene_build_placed(C.byref(MeshSet(full).desc), None) and "placements" in api.last_error()
    m = L.rtk_mgpu_create((C.c_int * 1)(0), 1)
    try:
        assert L.rtk_mgpu_build_placed(m, C.byref(ms.desc), ptr) == ERR_UNSUPPORTED
        assert L.rtk_mgpu_refit_placed(m, C.byref(MeshSet(full).desc), ptr) == ERR_BAD_ARG          # (no scene yet)
    finally:
        L.rtk_mgpu_destroy(m)
    with pytest.raises(ValueError):
        api.DeviceScene.build(full, placements=placements[:2])
    with pytest.raises(api.RtkError):
        ds.refit(full[:2], placements=placements[:2])


def test_the_loop(api):
    """build_placed -> quality -> refit_placed -> rebuild: the rebuilt scene is the twin's build of the last placed positions, and
    total_device_bytes of a placed build is the twin's (nothing of a placement is kept)."""
    p0, p1 = ring(0.0), ring(2.5, scale=0.45)
    meshes, A, B = instance_scenes(api, p0)
    assert A.info()["total_device_bytes"] == B.info()["total_device_bytes"]
    q0 = A.quality()
    assert q0["sah_cost"] == B.quality()["sah_cost"]
    A.refit(meshes, placements=p1)
    assert A.quality()["ratio"] is not None
    A.rebuild()
    fresh = api.DeviceScene.build(twin_of(meshes, p1))
    fa, ff = fingerprint(A), fingerprint(fresh)
    assert fa["check"] == ff["check"] and fa["order"] == ff["order"] and fa["blob"] == ff["blob"]
    assert fa["info"]["num_nodes"] == ff["info"]["num_nodes"] and fa["info"]["max_depth"] == ff["info"]["max_depth"]


def test_virtual_shards(api):
    """rtk_mgpu_build_placed, then rtk_mgpu_refit_meshes_placed, on two slots of device 0: both replicas are the single scene."""
    L = api.lib()
    p0 = ring(0.0)
    p1 = p0.copy()
    p1[[2, 7]] = ring(0.9)[[2, 7]]
    meshes, A, _ = instance_scenes(api, p0)
    want0 = fingerprint(A)["check"]["content_hash"]
    some = api.mesh_set_of_some([meshes[k] if k in (2, 7) else None for k in range(8)], A.mesh_base())
    A.refit(some, only=[2, 7], placements=p1)
    want1 = fingerprint(A)["check"]["content_hash"]
    assert want1 != want0
    m = L.rtk_mgpu_create((C.c_int * 2)(0, 0), 2)
    assert m
    try:
        ms = MeshSet(meshes)
        ptr0, keep0 = api.placement_ptr(p0, 8)
        ptr1, keep1 = api.placement_ptr(p1, 8)
        assert L.rtk_mgpu_build_placed(m, C.byref(ms.desc), ptr0) == 0, api.last_error()
        handles = [L.rtk_mgpu_scene(m, i) for i in range(2)]

        def hashes():
            out = []
            for h in handles:
                c = api.SceneCheck()
                assert L.rtk_dev_scene_validate(h, C.byref(c)) == 0, api.last_error()
                out.append(int(c.content_hash))
            return out
        assert hashes() == [want0, want0]
        ids = (C.c_uint32 * 2)(2, 7)
        assert L.rtk_mgpu_refit_meshes_placed(m, C.byref(some.desc), ptr1, ids, 2) == 0, api.last_error()
        assert [L.rtk_mgpu_scene(m, i) for i in range(2)] == handles
        assert hashes() == [want1, want1]
        assert [L.rtk_dev_scene_last_refit_nodes(h) for h in handles] == [A.last_refit_nodes()] * 2
        assert L.rtk_mgpu_refit_placed(m, C.byref(ms.desc), ptr0) == 0, api.last_error()
        assert hashes() == [want0, want0]
    finally:
        L.rtk_mgpu_destroy(m)
