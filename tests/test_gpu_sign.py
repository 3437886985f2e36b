"""GPU tests of rtk_dev_signed_distances and the table of pseudonormals behind it. The bar everywhere: the table, the counts and
the signed distances are bit for bit what numpy float32 gives by the rule of rtk_amd/csrc/rtk_sign_rule.h (tests/sign_ref.py)
over the scene's triangle records, whatever tree is above them; records and points are byte for byte rtk_dev_closest_points'.
Outputs are pre-filled with 0x7e and carry a tail that must stay untouched."""
import ctypes as C

import numpy as np
import pytest

from rtk_amd.types import POINT_QUERY_DTYPE
from tests import sign_ref
from tests.sign_ref import CLASSES, F, RTK_INF, class_queries, cpu_meshes, fan, l_prism, plus_shape, signed_np, table_np, torus, torus_inside

pytestmark = pytest.mark.gpu

TAIL, FILL = 5, 0x7e7e7e7e
ERR_UNSUPPORTED = -6
COUNTS = ("boundary_sides", "nonmanifold_sides", "inconsistent_sides", "degenerate_triangles", "places")


def mesh_of(tris):
    return dict(positions=np.ascontiguousarray(tris.reshape(-1, 3), F))


def indexed(tris, rng):
    """the same triangles with every vertex duplicated per face under shuffled indices: welding can only be by place"""
    pos = tris.reshape(-1, 3)
    perm = rng.permutation(len(pos))
    inv = np.argsort(perm)
    return dict(positions=np.ascontiguousarray(pos[perm], F), indices=np.ascontiguousarray(inv.reshape(-1, 3), np.uint32))


def make_queries(points, max2=RTK_INF):
    q = np.zeros(len(points), POINT_QUERY_DTYPE)
    q["point"] = points
    q["max_dist2"] = max2
    return q


def table_words(ds):
    return ds.pseudonormals().cpu().numpy().view(np.uint32)


def same_table(got_words, want):
    want = np.ascontiguousarray(want, F)
    nan = np.isnan(want)
    assert (np.isnan(got_words.view(F)) == nan).all()
    assert ((got_words == want.view(np.uint32)) | nan).all(), np.argwhere((got_words != want.view(np.uint32)) & ~nan)[:5]


def run(api, ds, queries, n=None, records=True, points=True, count=None, ids=None):
    """-> (signed words [n + TAIL], record words [n + TAIL, 4] or None, point words [n + TAIL, 3] or None)"""
    import torch
    n = len(queries) if n is None else n
    d_q = api.to_device(queries) if len(queries) else torch.zeros(16, dtype=torch.uint8, device="cuda")
    d_sg = torch.full((n + TAIL,), 0, dtype=torch.int32, device="cuda").fill_(FILL).view(torch.float32)
    d_rec = torch.full(((n + TAIL) * 16,), 0x7e, dtype=torch.uint8, device="cuda") if records else None
    d_pts = torch.full(((n + TAIL) * 12,), 0x7e, dtype=torch.uint8, device="cuda") if points else None
    d_count = torch.tensor([count], dtype=torch.int64, device="cuda") if count is not None else None
    d_ids = torch.from_numpy(np.ascontiguousarray(ids, np.int64)).cuda() if ids is not None else None
    ds.signed_distances_device(d_q, n, d_rec, d_pts, d_sg, count=d_count, ids=d_ids, want_records=records, want_points=points)
    assert api.lib().rtk_dev_trace_status(ds.handle, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0, api.last_error()
    sg = d_sg.view(torch.int32).cpu().numpy().view(np.uint32)
    rec = d_rec.cpu().numpy().view(np.uint32).reshape(n + TAIL, 4) if records else None
    pts = d_pts.cpu().numpy().view(np.uint32).reshape(n + TAIL, 3) if points else None
    assert (sg[n:] == FILL).all() and (rec is None or (rec[n:] == FILL).all()) and (pts is None or (pts[n:] == FILL).all()), "written beyond num_queries"
    return sg, rec, pts


def closest(api, ds, queries):
    d_rec, d_pts = ds.closest_points_device(api.to_device(queries), len(queries))
    return d_rec.cpu().numpy().view(np.uint32).reshape(-1, 4), d_pts.cpu().numpy().view(np.uint32).reshape(-1, 3)


def check(api, ds, tris, points, max2=RTK_INF, table=None):
    """the whole batch against the reference over `tris` (prim = row) and against rtk_dev_closest_points; returns signed floats"""
    table = table_np(tris)[0] if table is None else table
    q = make_queries(points, max2)
    want, want_rec, want_pts, _, _ = signed_np(tris, table, q["point"], q["max_dist2"])
    sg, rec, pts = run(api, ds, q)
    n = len(q)
    assert (sg[:n] == want.view(np.uint32)).all(), np.argwhere(sg[:n] != want.view(np.uint32))[:5]
    crec, cpts = closest(api, ds, q)
    assert (rec[:n] == crec).all() and (pts[:n] == cpts).all() and (rec[:n] == want_rec).all() and (pts[:n] == want_pts).all()
    miss = want_rec[:, 3] == sign_ref.NONE
    assert (sg[:n][miss] == RTK_INF.view(np.uint32)).all()
    return sg[:n].view(F)


def test_table_equals_the_reference(api):
    """Bit for bit, with the counts: the L, the L with duplicated vertices under other indices, the L as two meshes that meet, the
    defect mesh, the fan of 200 (a run longer than a wave) and a 64 x 32 torus -- 12288 corners, three tiles of the sort's 4096
    (SORT_TILE in rtk_sort.hip: num_units = (n + SORT_TILE - 1) / SORT_TILE decides between one workgroup and several)."""
    rng = np.random.RandomState(5)
    L = l_prism().triangles()
    half = len(L) // 2
    cases = {"L": ([mesh_of(L)], L), "L duplicated": ([indexed(L, rng)], L), "L two meshes": ([mesh_of(L[half:]), indexed(L[:half], rng)], np.concatenate([L[half:], L[:half]])),
             "defects": ([mesh_of(cpu_meshes()["defects"])], cpu_meshes()["defects"]), "fan": ([mesh_of(fan(200))], fan(200)),
             "torus": ([mesh_of(torus(64, 32))], torus(64, 32))}
    for name, (meshes, tris) in cases.items():
        ds = api.DeviceScene.build(meshes)
        want, info = table_np(tris)
        got = ds.prepare_signs()
        assert {k: got[k] for k in COUNTS} == info, (name, got, info)
        assert got["table_bytes"] == 72 * len(tris) and got["table_ms"] > 0 and got["closed"] == (name in ("L", "L duplicated", "L two meshes", "torus"))
        same_table(table_words(ds), want)
    assert len(torus(64, 32)) == 4096 and 3 * 4096 > 2 * 4096                # (more than one tile of the sort, and a partial last one is the fan's)


@pytest.fixture(scope="module")
def shapes():
    out = {}
    for name, shape, seed in (("L", l_prism(sign_ref.TILT), 21), ("plus", plus_shape(sign_ref.TILT), 22)):
        tris = shape.triangles()
        pts, cls, _ = class_queries(shape, 300, seed)
        out[name] = (shape, tris, table_np(tris)[0], pts)
    return out


def test_sign_equals_the_reference_and_the_truth(api, shapes):
    """300 queries per class round the turned L and plus: signed bit for bit, records and points byte for byte the closest call's,
    and the side is the analytic one. A random mix round the torus the same, with misses (a limit, a NaN)."""
    for name, (shape, tris, table, pts) in shapes.items():
        ds = api.DeviceScene.build([mesh_of(tris)])
        sg = check(api, ds, tris, pts, table=table)
        assert ((sg < 0) == shape.inside(pts)).all(), name
    tris = torus(64, 32)
    ds = api.DeviceScene.build([mesh_of(tris)])
    rng = np.random.RandomState(3)
    pts = rng.uniform(-3.2, 3.2, (1500, 3)).astype(F) * np.array([1, 1, 0.4], F)
    max2 = np.full(len(pts), RTK_INF, F)
    max2[:200] = 0.01
    pts[200, 0] = np.nan; pts[201, 2] = np.inf; max2[202] = np.nan; max2[203] = 0.0
    sg = check(api, ds, tris, pts, max2)
    assert (sg[200:204].view(np.uint32) == RTK_INF.view(np.uint32)).all() and (sg[:200] == RTK_INF).any() and (sg[:200] != RTK_INF).any()
    far = np.abs(np.hypot(np.hypot(pts[:, 0], pts[:, 1]) - 2.0, pts[:, 2]) - 0.75) > 0.05      # (the mesh is inscribed in the torus: leave its skin out)
    ok = far & (sg != RTK_INF) & np.isfinite(pts).all(1)
    assert ok.sum() > 800 and ((sg < 0)[ok] == torus_inside(pts)[ok]).all()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_sizes(api, shapes, n):
    shape, tris, table, pts = shapes["L"]
    ds = api.DeviceScene.build([mesh_of(tris)])
    if n == 0:
        before = ds.info()["total_device_bytes"]
        run(api, ds, make_queries(pts[:0]))
        assert ds.info()["total_device_bytes"] == before                     # no queries: the table is not made
        return
    check(api, ds, tris, pts[np.arange(n) % len(pts)], table=table)


def test_lists_null_outputs_and_two_launches(api, shapes):
    shape, tris, table, pts = shapes["plus"]
    ds = api.DeviceScene.build([mesh_of(tris)])
    q = make_queries(pts[:500])
    want = signed_np(tris, table, q["point"], q["max_dist2"])[0].view(np.uint32)
    full, rec0, pts0 = run(api, ds, q)
    again, rec1, pts1 = run(api, ds, q)
    assert (full == again).all() and (rec0 == rec1).all() and (pts0 == pts1).all() and (full[:500] == want).all()
    # NULL d_records (the scratch set's array) and NULL d_points
    sg, rec, p = run(api, ds, q, records=False, points=False)
    assert rec is None and p is None and (sg == full).all()
    sg, rec, p = run(api, ds, q, records=False)
    assert (sg == full).all() and (p == pts0).all()
    # lists: a slot that is not listed is not written; an id may repeat; the count is clamped
    ids = np.array([7, 3, 3, 499, 0, 250, 7], np.int64)
    for count, use in ((len(ids), ids), (4, ids[:4]), (0, ids[:0])):
        sg, rec, p = run(api, ds, q, count=count, ids=ids)
        listed = np.zeros(500 + TAIL, bool)
        listed[use] = True
        assert (sg[listed] == full[listed]).all() and (sg[~listed] == FILL).all()
        assert (rec[listed] == rec0[listed]).all() and (rec[~listed] == FILL).all() and (p[~listed] == FILL).all()
    sg, _, _ = run(api, ds, q, count=100)                                    # ids NULL: the first 100
    assert (sg[:100] == full[:100]).all() and (sg[100:] == FILL).all()


def test_the_tree_does_not_matter(api, oracle, shapes):
    """Device build, CPU-builder upload, after split_leaves, after rebuild, and a build from the triangles in another order with
    the ids mapped back: the same table bytes and the same signed bytes; a split and a rebuild do not make the table again."""
    from oracle import pyoracle
    tris = torus(64, 32)
    rng = np.random.RandomState(9)
    pts = rng.uniform(-3.2, 3.2, (700, 3)).astype(F) * np.array([1, 1, 0.4], F)
    q = make_queries(pts)
    built = api.DeviceScene.build([mesh_of(tris)])
    want_table, want_sg = table_words(built), run(api, built, q)[0]
    same_table(want_table, table_np(tris)[0])
    up = api.DeviceScene.upload(pyoracle.build_scene([mesh_of(tris)]))
    assert (table_words(up) == want_table).all() and (run(api, up, q)[0] == want_sg).all()
    for ds, step in ((up, lambda d: d.split_leaves(2)), (up, lambda d: d.rebuild()), (built, lambda d: d.rebuild())):
        step(ds)
        assert ds.prepare_signs()["table_ms"] == 0                           # kept: made from positions, indexed by primitive
        assert (table_words(ds) == want_table).all() and (run(api, ds, q)[0] == want_sg).all()
    perm = rng.permutation(len(tris))
    other = api.DeviceScene.build([mesh_of(tris[perm])])
    got = table_words(other)
    # The sums of a place are taken in the order of the primitive ids (the rule), so the same triangles under another numbering
    # may round a sum differently: in the numpy reference itself 4033 of this torus's 4096 rows, mapped back, differ from the
    # first numbering's, by at most 9.5e-7. Byte equality with the ids mapped back is therefore not what the rule gives; the
    # renumbered scene is held to the reference over ITS records, bit for bit, to the same distances and to the same sides.
    same_table(got, table_np(tris[perm])[0])
    back = np.empty_like(got)
    back[perm] = got
    assert np.abs(back.view(F) - want_table.view(F)).max() <= 4 * 2.0 ** -23 * 8      # (sums of at most 8 terms below pi in size)
    sg = run(api, other, q)[0][:len(q)].view(F)
    far = np.abs(np.hypot(np.hypot(pts[:, 0], pts[:, 1]) - 2.0, pts[:, 2]) - 0.75) > 0.05
    assert ((sg < 0)[far] == (want_sg[:len(q)].view(F) < 0)[far]).all() and (np.abs(sg) == np.abs(want_sg[:len(q)].view(F))).all()


def test_a_refit_drops_the_table_and_the_ledger_counts_it(api, shapes):
    """total_device_bytes grows by exactly 72 * num_prims at the first call and not at the second; a scene never asked keeps
    its figure. A refit to the mirrored copy (every winding turned) drops the table: the figure falls by table_bytes, the signs
    flip, the next prepare_signs reports a making. The same through refit_meshes on the two-mesh L."""
    L = l_prism().triangles()
    half = len(L) // 2
    mirrored = (L * np.array([-1, 1, 1], F)).astype(F)
    pts = class_queries(l_prism(), 40, 31)[0]
    q = make_queries(pts)
    for meshes, moved, only in (([mesh_of(L)], [mesh_of(mirrored)], None), ([mesh_of(L[:half]), mesh_of(L[half:])], [mesh_of(mirrored[:half]), mesh_of(mirrored[half:])], [0, 1])):
        ds = api.DeviceScene.build(meshes)
        never = api.DeviceScene.build(meshes)
        ok, _ = ds.validate()                                                # (a device build makes its side arrays on first use: made here, not counted below)
        never.validate()
        ds.refit(meshes, only=only)                                          # (... and a first refit its schedule: counted too, and kept)
        never.refit(meshes, only=only)
        base =ds.info()["total_device_bytes"]
        first = run(api, ds, q)[0][:len(q)].view(F)
        assert ds.info()["total_device_bytes"] == base + 72 * len(L)
        run(api, ds, q)
        info = ds.prepare_signs()
        assert ds.info()["total_device_bytes"] == base + 72 * len(L) and info["table_bytes"] == 72 * len(L) and info["table_ms"] == 0
        assert never.info()["total_device_bytes"] == base
        ds.refit(moved, only=only)
        assert ds.info()["total_device_bytes"] == base
        mq = make_queries(pts * np.array([-1, 1, 1], F))
        flipped = run(api, ds, mq)[0][:len(q)].view(F)
        assert ds.info()["total_device_bytes"] == base + 72 * len(L)
        assert (np.abs(flipped) == np.abs(first)).all() and ((flipped < 0) != (first < 0)).all()
        ds.refit(moved, only=only)
        assert ds.prepare_signs()["table_ms"] > 0


@pytest.fixture(scope="module")
def cfg1_blob(oracle):
    from rtk_amd import synth
    return oracle.build_scene([dict(positions=synth.scene_for_config(1))])


def test_a_blob_that_names_a_primitive_twice_is_refused(api, oracle, cfg1_blob):
    """the blob of tests/test_gpu_rebuild.py's refusal: one triangle of a leaf given its neighbour's id. -6, nothing allocated."""
    from tests.test_gpu_rebuild import _as_blob, _leaves
    import torch
    data = np.array(cfg1_blob.data, copy=True)
    off, cnt = next((o, c) for o, c in _leaves(data) if c >= 2 and c % 4 != 1)
    ids = data[off + 8:off + 8 + 8 * cnt].view("<u4")[1::2]
    twice = data.copy()
    twice[off + 8:off + 8 + 8 * cnt].view("<u4")[2 * cnt - 1] = ids[cnt - 2]
    ds = api.DeviceScene.upload(_as_blob(oracle, twice))
    before = ds.info()
    info = api.SignInfo()
    assert api.lib().rtk_dev_scene_prepare_signs(ds.handle, C.byref(info), None) == ERR_UNSUPPORTED and "one triangle record per primitive" in api.last_error()
    buf = torch.zeros(64, dtype=torch.uint8, device="cuda")
    assert api.lib().rtk_dev_signed_distances(ds.handle, C.c_void_p(buf.data_ptr()), 1, None, None, None, C.c_void_p(buf.data_ptr()), None) == ERR_UNSUPPORTED
    assert api.lib().rtk_dev_scene_pseudonormals(ds.handle, C.c_void_p(buf.data_ptr()), None) == ERR_UNSUPPORTED
    assert ds.info() == before
    good = api.DeviceScene.upload(_as_blob(oracle, data))                    # (the blob as it came is served)
    assert good.prepare_signs()["table_bytes"] == 72 * good.info()["num_triangles"]


def test_contains_signed_and_signed_distances_on_the_cube(api):
    """the eight points just inside the cube's corners and the eight just outside, through the Python interface"""
    ds = api.DeviceScene.build([mesh_of(sign_ref.cube())])
    corners = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], F)
    pts = np.concatenate([corners * F(0.99), corners * F(1.01)])
    inside = ds.contains_signed(pts).cpu().numpy()
    assert inside[:8].all() and not inside[8:].any()
    signed, prim, closest_pts = ds.signed_distances(pts)
    signed, prim, closest_pts = signed.cpu().numpy(), prim.cpu().numpy(), closest_pts.cpu().numpy()
    assert np.allclose(signed[:8], -0.01, atol=1e-6) and np.allclose(signed[8:], 0.01 * np.sqrt(3), atol=1e-6)
    assert ((prim >= 0) & (prim < 12)).all() and np.allclose(closest_pts[8:], corners)
    signed, prim, _ = ds.signed_distances(pts, max_dist=0.005)
    assert (signed.cpu().numpy() == RTK_INF).all() and (prim.cpu().numpy() == -1).all()
    assert ds.prepare_signs()["closed"] and ds.prepare_signs()["places"] == 8
