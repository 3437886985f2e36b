"""GPU tests of rtk_dev_scene_refit_meshes / rtk_mgpu_refit_meshes: new positions for SOME meshes of a device scene.

The yardstick is the TWIN scene. The device build is deterministic, so the same input is built twice: scene A gets
refit(only=ids) with new positions for the listed meshes, scene B the full refit with those positions for the listed
meshes and the positions A holds for the rest. The contract is bit identity, so nothing here has a tolerance: validator
counts and content hash, the exported blob, hit records on every path that reads different data, and the two things hits
cannot see -- the child order words (step counts of the packet kernel) and the compressed nodes (visit counts of the
per-lane kernel). Once per module A is also tied to the oracle walking A's own exported blob. How many nodes a call
remade (last_refit_nodes) is checked against a count made here, in Python, from the exported blob."""
import ctypes as C

import numpy as np
import pytest

from rtk_amd import synth
from rtk_amd.types import HIT_RECORD_DTYPE, MeshSet, RAY_DTYPE
from tests.test_gpu_refit import _all_paths_vs_oracle, _as_blob, _edge_meshes, _records_vs_oracle, _valid, deform

pytestmark = pytest.mark.gpu

# rtk_amd.h: above this share of the scene's triangles in the listed meshes the full box and finish passes run
FULL_PASSES_ABOVE = 0.25


def by_slab(v, k):
    """The soup cut into k meshes of (almost) equal size along x: compact meshes."""
    tri = np.asarray(v).reshape(-1, 3, 3)
    order = np.argsort(tri[:, :, 0].mean(1), kind="stable")
    return [np.ascontiguousarray(tri[part].reshape(-1, 3)) for part in np.array_split(order, k)]


def round_robin(v, k):
    """Triangle i goes to mesh i % k: every mesh is everywhere."""
    tri = np.asarray(v).reshape(-1, 3, 3)
    return [np.ascontiguousarray(tri[m::k].reshape(-1, 3)) for m in range(k)]


def extent(parts):
    allp = np.concatenate([np.asarray(p, np.float64) for p in parts if len(p)]) if any(len(p) for p in parts) else np.zeros((1, 3))
    return allp.max(0) - allp.min(0)


def nodes_above(blob_bytes, listed):
    """(nodes whose subtree holds a triangle of a listed mesh, all nodes), from the blob alone. Node: 24 floats of boxes and
    four 64-bit child words at byte 96 (bit 0: leaf; an inverted box: empty slot). Leaf: a 64-bit word with the count in
    its low 6 bits, count rounded up to 4 records of 8 bytes (byte 3: local mesh), then the table local mesh -> mesh."""
    b = np.frombuffer(blob_bytes, np.uint8)
    listed = set(int(m) for m in listed)
    touched, total = 0, 0
    stack = [(128, False)]
    result = {}
    while stack:
        at, done = stack.pop()
        words = b[at + 96:at + 128].view(np.uint64)
        lo, hi = b[at:at + 16].view(np.float32), b[at + 16:at + 32].view(np.float32)
        kids = [int(words[k]) for k in range(4) if lo[k] <= hi[k]]
        if not done:
            stack.append((at, True))
            stack.extend((c, False) for c in kids if not c & 1)
            continue
        hit = False
        for c in kids:
            if not c & 1:
                hit = hit or result[c]
                continue
            leaf = c ^ 1
            n = int(b[leaf:leaf + 8].view(np.uint64)[0]) & 0x3f
            n4 = (n + 3) & ~3
            recs = b[leaf + 8:leaf + 8 + 8 * n4].reshape(-1, 8)
            table = leaf + 8 + 8 * n4
            hit = hit or any(int(b[table + 4 * int(recs[t, 3]):table + 4 * int(recs[t, 3]) + 4].view(np.uint32)[0]) in listed for t in range(n))
        result[at] = hit
        total += 1
        touched += 1 if hit else 0
    return touched, total


def same_scene(api, A, B, rays_scale=1, finite=True):
    """A and B are the same scene, bit for bit, as far as anything can tell."""
    if finite:
        ca, cb = _valid(A), _valid(B)
    else:
        (oka, ca), (okb, cb) = A.validate(), B.validate()
        assert oka == okb
    assert ca == cb, (ca, cb)                                   # (every count, nodes_checked and content_hash among them)
    assert A.export_blob().tobytes() == B.export_blob().tobytes()
    assert A.info()["num_nodes"] == B.info()["num_nodes"]
    img, iopts = synth.rays_pinhole(256, 256), api.make_opts(image=(256, 256))
    inc = synth.rays_incoherent(65536)[::rays_scale]
    sh = synth.rays_shadow(65536)[::rays_scale]
    assert A.trace(img, opts=iopts, full=False).tobytes() == B.trace(img, opts=iopts, full=False).tobytes()
    for opts in (None, api.make_opts(exact_nodes=True), api.make_opts(no_asm=True)):
        assert A.trace(inc, opts=opts, full=False).tobytes() == B.trace(inc, opts=opts, full=False).tobytes()
    assert (A.trace_any(sh) == B.trace_any(sh)).all()
    # order words: the packet kernel's own step counts; compressed nodes: what the per-lane kernel visits
    def packet_counted(ds):
        try:
            return ds.trace_packet_counted(img, iopts)
        except api.RtkError:
            # (a scene whose bound is not finite is not given to the assembly packet kernel: then neither twin is)
            assert not finite
            return None
    a, b = packet_counted(A), packet_counted(B)
    assert (a is None) == (b is None)
    if a is not None:
        (ra, pa), (rb, pb) = a, b
        assert ra.tobytes() == rb.tobytes()
        for k in ("node_steps", "triangles_fetched", "triangle_group_tests"):
            assert pa[k] == pb[k], (k, pa, pb)
    (ra, la), (rb, lb) = A.trace_counted(inc), B.trace_counted(inc)
    assert ra.tobytes() == rb.tobytes()
    for k in ("nodes", "leaves", "triangles"):
        assert la[k] == lb[k], (k, la, lb)
    assert api.lib().rtk_dev_trace_status(A.handle, None) == 0


class Twin:
    """Scene A and what it has been given so far; move() gives A a per-mesh refit and returns a fresh twin B."""

    def __init__(self, api, meshes, upload=None):
        self.api, self.base, self.cur, self.upload = api, [dict(m) for m in meshes], [dict(m) for m in meshes], upload
        self.A = self.make()
        i = self.A.info()
        self.shape = (self.A.primitive_order().tobytes(), i["num_nodes"], i["max_depth"], i["stack_entries"], i["num_triangles"], i["num_meshes"])
        self.num_nodes, self.num_tris = i["num_nodes"], i["num_triangles"]

    def make(self):
        return self.api.DeviceScene.upload(self.upload) if self.upload is not None else self.api.DeviceScene.build(self.base)

    def move(self, new, check_nodes=True, exact_before=True, compare=True, finite=True, rays_scale=1):
        """new: {mesh id: positions}. A.refit(only=...), unlisted meshes passed as None; B: a new scene + the full refit."""
        for m, p in new.items():
            self.cur[m] = dict(self.cur[m], positions=p)
        self.A.refit([self.cur[m] if m in new else None for m in range(len(self.cur))], only=list(new))
        assert self.A.last_refit_ms() > 0.0
        B = self.make()
        B.refit(self.cur)
        assert B.last_refit_nodes() == self.num_nodes
        i = self.A.info()
        assert (self.A.primitive_order().tobytes(), i["num_nodes"], i["max_depth"], i["stack_entries"], i["num_triangles"], i["num_meshes"]) == self.shape
        if check_nodes:
            listed_tris = sum(int(self.A.mesh_base()[m + 1] - self.A.mesh_base()[m]) for m in new)
            touched, total = nodes_above(self.A.export_blob().tobytes(), new)
            assert total == self.num_nodes
            full = not exact_before or listed_tris > FULL_PASSES_ABOVE * self.num_tris
            assert self.A.last_refit_nodes() == (self.num_nodes if full else touched), (touched, total, listed_tris)
            if not full and len(new) * 4 <= len(self.cur) and self.num_tris >= 10_000 and getattr(self, "compact", False):
                assert touched < total // 2                       # (the work did follow the moved part)
        if compare:
            same_scene(self.api, self.A, B, rays_scale=rays_scale, finite=finite)
        return B


def soup_twin(api, cut, k, n=None, spread=None):
    v0 = synth.scene_for_config(1) if n is None else synth.triangle_soup(max(n, 1), spread, seed=17)[:3 * n]
    parts = cut(v0, k)
    tw = Twin(api, [dict(positions=p) for p in parts])
    tw.parts, tw.ext, tw.compact = parts, extent(parts), cut is by_slab
    return tw


_oracle_done = []


@pytest.mark.parametrize("cut", [by_slab, round_robin], ids=["slabs", "round_robin"])
@pytest.mark.parametrize("ids", [(5,), (2, 9, 14), tuple(range(16))], ids=["one", "three", "all"])
def test_soup_in_16_meshes(api, oracle, cut, ids):
    tw = soup_twin(api, cut, 16)
    assert tw.A.last_refit_nodes() == 0
    tw.move({m: deform(tw.parts[m], 1, tw.ext) for m in ids})
    if not _oracle_done:
        # once per module: A against the reference's walk of A's own blob, every path, bit-exact
        _all_paths_vs_oracle(api, oracle, tw.A, [m["positions"] for m in tw.cur])
        _oracle_done.append(True)


def test_against_the_oracle(api, oracle):
    """A after a per-mesh refit against the oracle walking A's exported blob (whatever order the tests ran in)."""
    tw = soup_twin(api, by_slab, 16)
    tw.move({3: deform(tw.parts[3], 2, tw.ext)}, compare=False)
    _all_paths_vs_oracle(api, oracle, tw.A, [m["positions"] for m in tw.cur])


def test_sequence_on_one_scene(api):
    tw = soup_twin(api, by_slab, 16)
    h0 = _valid(tw.A)["content_hash"]
    tw.move({2: deform(tw.parts[2], 1, tw.ext)})
    h1 = _valid(tw.A)["content_hash"]
    assert h1 != h0
    tw.move({2: tw.parts[2]})
    assert _valid(tw.A)["content_hash"] == h0                   # (mesh 2 back, nothing else moved: the build's bits)
    tw.move({2: deform(tw.parts[2], 1, tw.ext)})
    tw.move({5: deform(tw.parts[5], 1, tw.ext)})
    tw.move({2: tw.parts[2]})
    tw.move({9: deform(tw.parts[9], 2, tw.ext)})
    # the empty call: no bit, no work
    h = _valid(tw.A)["content_hash"]
    tw.A.refit([None] * 16, only=[])
    assert tw.A.last_refit_nodes() == 0 and _valid(tw.A)["content_hash"] == h
    # an id that repeats counts once
    tw.A.refit([tw.cur[m] if m == 9 else None for m in range(16)], only=[9, 9, 9])
    assert _valid(tw.A)["content_hash"] == h and 0 < tw.A.last_refit_nodes() < tw.num_nodes


@pytest.mark.parametrize("n,spread", [(8, 0.5), (1023, 0.1), (1024, 0.1), (1025, 0.1), (10_000, 0.05), (1_000_000, 0.02), (1_600_000, 0.02)])
def test_sizes(api, n, spread):
    """Sizes that straddle the builder's boundaries (the refit tile of 1024; from about 1.5 M triangles on the tile
    collapse numbers the nodes in two runs), 8 slab meshes, one moved -- then back."""
    tw = soup_twin(api, by_slab, 8, n, spread)
    h0 = _valid(tw.A)["content_hash"]
    big = n > 10_000
    tw.move({3: deform(tw.parts[3], 1, tw.ext)}, check_nodes=not big, rays_scale=8 if big else 1)
    assert _valid(tw.A)["content_hash"] != h0
    if big:
        assert 0 < tw.A.last_refit_nodes() < tw.num_nodes // 4
    tw.A.refit([dict(positions=tw.parts[3]) if m == 3 else None for m in range(8)], only=[3])
    assert _valid(tw.A)["content_hash"] == h0


@pytest.mark.parametrize("share", [None, "0", "1"], ids=["default", "share0", "share1"])
def test_first_call_ever_is_a_placed_refit_of_one_f64_host_mesh(api, monkeypatch, share):
    """The first refit a scene sees lists one mesh, host-resident doubles, with a placement: the schedule's temporaries, those of
    the per-mesh tables, the staged positions and the placement table all take their turn in ONE loan of the workspace. With the
    dirty set (the default share, and 1) and with the full passes (0) the scene is, byte for byte, what the full placed refit of
    a twin makes of the same inputs. 10 000 triangles: heights with a launch of their own and a run of small ones. (Both scenes
    are built through the identity, so every other mesh has gone through the one rule on both sides.)"""
    from tests.test_gpu_placed import ROT_TRANS
    if share is None:
        monkeypatch.delenv("RTK_AMD_REFIT_MESHES_SHARE", raising=False)
    else:
        monkeypatch.setenv("RTK_AMD_REFIT_MESHES_SHARE", share)
    parts = by_slab(synth.triangle_soup(10_000, 0.05, seed=17), 16)
    meshes = [dict(positions=p) for p in parts]
    placements = np.tile(np.eye(3, 4, dtype=np.float32), (16, 1, 1))
    A, B = api.DeviceScene.build(meshes, placements=placements), api.DeviceScene.build(meshes, placements=placements)
    assert A.last_refit_nodes() == 0 and A.export_blob().tobytes() == B.export_blob().tobytes()
    num_nodes = A.info()["num_nodes"]
    moved = dict(positions=deform(parts[5], 1, extent(parts)).astype(np.float64))
    placements[5] = ROT_TRANS
    given = np.full_like(placements, np.nan)                    # (entries of unlisted meshes are not read)
    given[5] = ROT_TRANS
    A.refit([moved if m == 5 else None for m in range(16)], only=[5], placements=given)
    B.refit([moved if m == 5 else meshes[m] for m in range(16)], placements=placements)
    assert A.export_blob().tobytes() == B.export_blob().tobytes()
    assert _valid(A) == _valid(B)
    assert B.last_refit_nodes() == num_nodes
    assert A.last_refit_nodes() == num_nodes if share == "0" else 0 < A.last_refit_nodes() < num_nodes


def test_nothing_to_move(api):
    """A scene without triangles, and a listed mesh without triangles: fine, and no bit changes."""
    none = np.zeros((0, 3), np.float32)
    ds = api.DeviceScene.build([dict(positions=none)])
    h = ds.validate()[1]["content_hash"]
    ds.refit([dict(positions=none)], only=[0])
    assert ds.validate()[1]["content_hash"] == h and ds.last_refit_nodes() == 0
    v0 = synth.scene_for_config(1)
    ds = api.DeviceScene.build([dict(positions=v0), dict(positions=none)])
    h = _valid(ds)["content_hash"]
    blob = ds.export_blob().tobytes()
    ds.refit([None, dict(positions=none)], only=[1])
    assert _valid(ds)["content_hash"] == h and ds.export_blob().tobytes() == blob and ds.last_refit_nodes() == 0
    # ... next to one that does move
    tw = Twin(api, [dict(positions=v0[:15000]), dict(positions=none), dict(positions=v0[15000:])])
    tw.move({1: none, 2: deform(v0[15000:], 1)}, check_nodes=False)
    assert tw.A.last_refit_nodes() == tw.num_nodes              # (half the scene: the full passes)


@pytest.mark.parametrize("kind", ["numpy_f32", "numpy_f64", "torch_f32", "torch_f64", "strided_f32", "strided_f64", "mixed"])
def test_position_inputs(api, kind):
    """The listed mesh's positions in every form a position buffer may take; unlisted meshes with position.data = NULL."""
    import torch
    tw = soup_twin(api, by_slab, 16)
    dt = np.float64 if kind.endswith("f64") else np.float32
    ids = (4, 11) if kind == "mixed" else (4,)
    new = {m: deform(tw.parts[m], 1, tw.ext) for m in ids}
    keep = []

    def entry(m):
        if m not in new:
            return None
        v = new[m].astype(np.float64 if kind == "mixed" and m == 11 else dt)
        if kind.startswith("torch"):
            t = torch.from_numpy(v).cuda()
            keep.append((t, v))
            return dict(positions=t)
        return dict(positions=v)
    ms = api.mesh_set_of_some([entry(m) for m in range(16)], tw.A.mesh_base())
    if kind.startswith("strided"):
        wide = np.full((len(new[4]), 5), 7.0, dt)                 # x y z and two words nobody may read as positions
        wide[:, :3] = new[4]
        ms._keep.append(wide)
        ms._arr[4].position.data = wide.ctypes.data
        ms._arr[4].position.stride = wide.strides[0]
    for m in range(16):
        assert (ms._arr[m].position.data is None) == (m not in new)
    tw.A.refit(ms, only=list(ids))
    for t, v in keep:
        assert t.cpu().numpy().tobytes() == v.tobytes()         # (read, not written)
    for m in ids:
        tw.cur[m] = dict(positions=new[m])
    B = tw.make()
    B.refit(tw.cur)
    same_scene(api, tw.A, B)
    assert 0 < tw.A.last_refit_nodes() < tw.num_nodes


@pytest.mark.parametrize("where", ["host", "device"])
def test_indexed_meshes_that_share_vertices(api, oracle, golden_dir, where):
    """The u16 + float64 / u32 + float32 fixture: one mesh moved, then the other, then both (mixed formats in one launch)."""
    import torch
    g, (p0, i0), (p1, i1) = _edge_meshes(golden_dir)
    allp = np.concatenate([p0, p1.astype(np.float64)])
    ext = allp.max(0) - allp.min(0)
    tw = Twin(api, [dict(positions=p0, indices=i0), dict(positions=p1, indices=i1)])
    put = (lambda a: torch.from_numpy(a).cuda()) if where == "device" else (lambda a: a)
    q0, q1 = deform(p0, 1, ext), deform(p1, 1, ext)
    for new in ({0: q0}, {1: q1}, {0: p0, 1: deform(p1, 2, ext)}):
        for m, p in new.items():
            tw.cur[m] = dict(tw.cur[m], positions=p)
        tw.A.refit([dict(tw.cur[m], positions=put(tw.cur[m]["positions"])) if m in new else None for m in range(2)], only=list(new))
        B = tw.make()
        B.refit(tw.cur)
        ca, cb = _valid(tw.A), _valid(B)
        assert ca == cb
        assert tw.A.export_blob().tobytes() == B.export_blob().tobytes()
        rays = np.ascontiguousarray(g["rays"]).view(RAY_DTYPE).reshape(-1)
        ha, ma, ra = tw.A.trace(rays)
        hb, mb, rb = B.trace(rays)
        assert ra.tobytes() == rb.tobytes() and ha.tobytes() == hb.tobytes() and ma.any()
    blob = _as_blob(oracle, tw.A.export_blob())
    ohits, omask = oracle.trace(blob, rays)
    _records_vs_oracle(ra, ohits, omask, tw.A.mesh_base(), "indexed meshes after per-mesh refits")


def test_uploaded_blob(api, oracle):
    """An uploaded blob's boxes need not be exact unions: the first per-mesh call remakes every box (and says so), the
    second one only what moved."""
    tw0 = soup_twin(api, by_slab, 16)
    blob = oracle.build_scene([dict(positions=p) for p in tw0.parts])
    tw = Twin(api, [dict(positions=p) for p in tw0.parts], upload=blob)
    tw.compact = True
    ok, c = tw.A.validate()
    assert ok, c
    tw.move({6: deform(tw0.parts[6], 1, tw0.ext)}, exact_before=False)
    assert tw.A.last_refit_nodes() == tw.num_nodes and _valid(tw.A)["loose_boxes"] == 0
    # (the twin of the second call: upload, full refit -- move() makes it from the cumulative positions)
    tw.move({10: deform(tw0.parts[10], 1, tw0.ext)})
    assert 0 < tw.A.last_refit_nodes() < tw.num_nodes // 2


def test_non_finite_positions_and_back(api):
    """NaN and inf in a vertex of a listed mesh: the scene leaves its compressed nodes as after a full refit, and comes back."""
    tw = soup_twin(api, by_slab, 16)
    inc = synth.rays_incoherent(65536)

    def visits(ds, opts=None):
        c = ds.trace_counted(inc, opts=opts)[1]
        return tuple(c[k] for k in ("rays", "nodes", "leaves", "triangles", "hits"))
    visits_q, visits_exact = visits(tw.A), visits(tw.A, api.make_opts(exact_nodes=True))
    assert visits_q != visits_exact
    h0 = _valid(tw.A)["content_hash"]
    nan = tw.parts[7].copy()
    nan[100, 1] = np.nan
    B = tw.move({7: nan}, finite=False, check_nodes=False)
    inf = tw.parts[7].copy()
    inf[100, 2] = np.inf
    B = tw.move({7: inf}, finite=False, check_nodes=False)
    assert visits(tw.A) == visits(tw.A, api.make_opts(exact_nodes=True)) == visits(B)      # (on its exact nodes, like the twin)
    # another mesh moves while the inf is still there: the scene starts on its exact nodes
    B = tw.move({2: deform(tw.parts[2], 1, tw.ext)}, finite=False, check_nodes=False)
    assert visits(tw.A) == visits(tw.A, api.make_opts(exact_nodes=True))
    tw.move({7: tw.parts[7]}, check_nodes=False)
    tw.move({2: tw.parts[2]})
    assert _valid(tw.A)["content_hash"] == h0
    assert visits(tw.A) == visits_q and visits(tw.A, api.make_opts(exact_nodes=True)) == visits_exact
    assert api.lib().rtk_dev_trace_status(tw.A.handle, None) == 0


def test_refusals_leave_the_scene_alone(api):
    tw = soup_twin(api, by_slab, 4)
    ds, parts = tw.A, tw.parts
    h0 = _valid(ds)["content_hash"]
    L = api.lib()

    def rc_of(ms, ids):
        a = (C.c_uint32 * max(len(ids), 1))(*ids)
        return L.rtk_dev_scene_refit_meshes(ds.handle, C.byref(ms.desc), a, len(ids), None)
    full = [dict(positions=p) for p in parts]
    assert rc_of(MeshSet(full), [4]) == -2                                              # RTK_AMD_ERR_BAD_ARG: id out of range
    assert "rtk_dev_scene_refit_meshes" in api.last_error() and "mesh id" in api.last_error()
    assert rc_of(MeshSet(full[:3]), [0]) == -2                                          # mesh count
    assert "meshes" in api.last_error()
    assert rc_of(MeshSet(full[:3] + [dict(positions=parts[3][:-3])]), [0]) == -2        # triangle count of an UNLISTED mesh
    assert "triangles" in api.last_error()
    ms = MeshSet(full)
    ms._arr[1].position_cb = 1                                                          # (never called: refused before)
    assert rc_of(ms, [1]) == -6                                                         # RTK_AMD_ERR_UNSUPPORTED
    assert "callback" in api.last_error()
    ms = MeshSet(full)
    ms._arr[1].position.data = None
    assert rc_of(ms, [0, 1]) == -2                                                      # listed mesh without positions
    assert "no positions" in api.last_error()
    ms = MeshSet(full)
    ms._arr[2].position.type = 77
    assert rc_of(ms, [2]) == -2                                                         # unknown position type
    assert L.rtk_dev_scene_refit_meshes(ds.handle, C.byref(MeshSet(full).desc), None, 1, None) == -2
    with pytest.raises(api.RtkError):
        ds.refit(full, only=[7])
    assert ds.last_refit_ms() == 0.0 and ds.last_refit_nodes() == 0
    assert _valid(ds)["content_hash"] == h0
    # what is NOT refused: the same oddities in meshes that are not listed
    ms = MeshSet(full)
    ms._arr[1].position_cb = 1
    ms._arr[2].position.data = None
    ms._arr[3].position.type = 77
    assert rc_of(ms, [0]) == 0, api.last_error()
    assert _valid(ds)["content_hash"] == h0


def test_virtual_shards(api):
    """rtk_mgpu_refit_meshes: three slots on device 0; every replica ends up as the single scene's."""
    tw = soup_twin(api, by_slab, 16)
    new = {m: deform(tw.parts[m], 1, tw.ext) for m in (1, 8)}
    tw.move(new, compare=False)
    want = _valid(tw.A)["content_hash"]
    L = api.lib()
    m = L.rtk_mgpu_create((C.c_int * 3)(0, 0, 0), 3)
    assert m
    try:
        ms0 = MeshSet(tw.base)
        ms1 = api.mesh_set_of_some([tw.cur[k] if k in new else None for k in range(16)], tw.A.mesh_base())
        ids = (C.c_uint32 * 2)(1, 8)
        assert L.rtk_mgpu_refit_meshes(m, C.byref(ms1.desc), ids, 2) == -2          # (no scene yet)
        assert L.rtk_mgpu_build(m, C.byref(ms0.desc)) == 0, api.last_error()
        handles = [L.rtk_mgpu_scene(m, i) for i in range(3)]
        assert L.rtk_mgpu_refit_meshes(m, C.byref(ms1.desc), ids, 2) == 0, api.last_error()
        assert [L.rtk_mgpu_scene(m, i) for i in range(3)] == handles
        for i in range(3):
            c = api.SceneCheck()
            assert L.rtk_dev_scene_validate(handles[i], C.byref(c)) == 0, api.last_error()
            assert c.content_hash == want and c.loose_boxes == 0
            assert L.rtk_dev_scene_last_refit_nodes(handles[i]) == tw.A.last_refit_nodes()
        rays = synth.rays_config1(65536)
        got = np.zeros(len(rays), HIT_RECORD_DTYPE)
        assert L.rtk_mgpu_trace_rays(m, rays.ctypes.data, len(rays), got.ctypes.data, None) == 0, api.last_error()
        assert got.tobytes() == tw.A.trace(rays, full=False).tobytes()
    finally:
        L.rtk_mgpu_destroy(m)


def test_two_streams_before_and_after(api, oracle):
    """A scene traced on two streams before the per-mesh refit gives the new scene's records on both."""
    import torch
    tw = soup_twin(api, by_slab, 16)
    ds = tw.A
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
    tw.move({m: deform(tw.parts[m], 2, tw.ext) for m in (6, 7, 8)}, compare=False)
    after = on_streams()
    assert after[0] == after[1] and after[0] != before[0]
    blob = _as_blob(oracle, ds.export_blob())
    for rays, raw in ((img, after[0][0]), (inc, after[0][1])):
        ohits, omask = oracle.trace(blob, rays)
        _records_vs_oracle(np.frombuffer(raw, HIT_RECORD_DTYPE), ohits, omask, ds.mesh_base(), "after the per-mesh refit, on a stream that traced before it")
