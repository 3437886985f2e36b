"""GPU tests of rtk_dev_closest_points. The bar everywhere: records and points are bit for bit what numpy float32 brute force
gives by the rule of rtk_amd/csrc/rtk_closest_rule.h (tests/closest_ref.py) over the triangle records the scene holds at that
moment -- read back through rtk_dev_expand_hits, so they are the scene's own --, whatever tree is above them. Outputs are
pre-filled with 0x7e and carry a tail that must stay untouched. The base scene is a 300-triangle soup; every brute force stays
below half a million (point, triangle) pairs."""
import ctypes as C

import numpy as np
import pytest

from rtk_amd import synth
from rtk_amd.types import CLOSEST_RECORD_DTYPE, HIT_DTYPE, HIT_RECORD_DTYPE, POINT_QUERY_DTYPE, RTK_INF
from tests.closest_ref import NONE, brute_force, tri_np

pytestmark = pytest.mark.gpu

TAIL = 5                                     # slots behind the batch that nobody may write
FILL = 0x7e7e7e7e


def scene_triangles(api, ds):
    """The scene's current triangle records by primitive id, [T, 3, 3] float32, through the expansion of made-up records"""
    n = ds.info()["num_triangles"]
    rec = np.zeros(n, HIT_RECORD_DTYPE)
    rec["prim"] = np.arange(n, dtype=np.uint32)
    d_hits, _ = ds.expand_device(api.to_device(rec), n)
    return np.ascontiguousarray(d_hits.cpu().numpy().view(HIT_DTYPE)["vertex"]["position"])


def make_queries(points, max2):
    q = np.zeros(len(points), POINT_QUERY_DTYPE)
    q["point"] = points
    q["max_dist2"] = max2
    return q


def run(api, ds, queries, n=None, with_points=True, count=None, ids=None):
    """-> (record words [n + TAIL, 4], point words [n + TAIL, 3] or None) as the device left them"""
    import torch
    n = len(queries) if n is None else n
    d_q = api.to_device(queries) if len(queries) else torch.zeros(16, dtype=torch.uint8, device="cuda")
    d_rec = torch.full(((n + TAIL) * 16,), 0x7e, dtype=torch.uint8, device="cuda")
    d_pts = torch.full(((n + TAIL) * 12,), 0x7e, dtype=torch.uint8, device="cuda") if with_points else None
    d_count = torch.tensor([count], dtype=torch.int64, device="cuda") if count is not None else None
    d_ids = torch.from_numpy(np.ascontiguousarray(ids, np.int64)).cuda() if ids is not None else None
    ds.closest_points_device(d_q, n, d_rec, d_pts, count=d_count, ids=d_ids, want_points=with_points)
    assert api.lib().rtk_dev_trace_status(ds.handle, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0, api.last_error()
    rec = d_rec.cpu().numpy().view(np.uint32).reshape(n + TAIL, 4)
    pts = d_pts.cpu().numpy().view(np.uint32).reshape(n + TAIL, 3) if with_points else None
    assert (rec[n:] == FILL).all() and (pts is None or (pts[n:] == FILL).all()), "written beyond num_queries"
    return rec, pts


def check(api, ds, queries, want=None):
    """the whole batch against brute force over the scene's own records (or the reference given); returns the records"""
    if want is None:
        tris = scene_triangles(api, ds)
        want = brute_force(tris, np.arange(len(tris), dtype=np.uint32), queries["point"], queries["max_dist2"])
    want_rec, want_pts = want
    rec, pts = run(api, ds, queries)
    n = len(queries)
    bad = np.nonzero((rec[:n] != want_rec).any(1) | (pts[:n] != want_pts).any(1))[0]
    assert len(bad) == 0, (len(bad), bad[:5], queries[bad[:5]], rec[bad[:5]], want_rec[bad[:5]], pts[bad[:5]], want_pts[bad[:5]])
    return rec[:n].copy().view(CLOSEST_RECORD_DTYPE).reshape(n)


def query_mix(tris, seed=11):
    """About 1300 queries over a scene of few triangles: uniform in the box, the scene's own vertices and centroids, far away,
    limits around the true distance, limits that are 0, negative and NaN, non-finite coordinates."""
    rng = np.random.RandomState(seed)
    tris = np.asarray(tris, np.float32).reshape(-1, 3, 3)
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    ext = hi - lo
    pick = rng.permutation(len(tris))[:250]
    pts = [rng.uniform(lo - 0.1 * ext, hi + 0.1 * ext, (400, 3)), tris[pick, rng.randint(0, 3, len(pick))], tris[pick].astype(np.float64).mean(1),
           lo + ext * 1e3 * rng.choice([-1.0, 1.0], (50, 3))]
    pts = np.concatenate(pts).astype(np.float32)
    max2 = np.full(len(pts), RTK_INF, np.float32)
    # limits around the true squared distance: its float32 neighbour below, itself (strict <: that triangle no longer counts), above
    some = rng.permutation(len(pts))[:120]
    true2 = tri_np(pts[some, None, :], tris[None, :, 0], tris[None, :, 1], tris[None, :, 2])[0].min(1)
    around = [np.nextafter(true2, np.float32(-1)), true2, np.nextafter(true2, np.float32(np.inf))]
    pts = np.concatenate([pts] + [pts[some]] * 3)
    max2 = np.concatenate([max2] + around).astype(np.float32)
    inside = rng.uniform(lo, hi, (39, 3)).astype(np.float32)
    pts = np.concatenate([pts, inside])
    max2 = np.concatenate([max2, np.repeat(np.array([0.0, -0.0, -1.0, np.nan, -np.inf, 1e-45, 0.01 * float(ext.max()) ** 2], np.float32), 6)[:39]])
    bad = rng.uniform(lo, hi, (9, 3)).astype(np.float32)
    bad[np.arange(9), np.arange(9) % 3] = np.array([np.nan, np.inf, -np.inf], np.float32)[np.arange(9) // 3]
    pts = np.concatenate([pts, bad])
    max2 = np.concatenate([max2, np.full(9, RTK_INF, np.float32)])
    return make_queries(pts, max2)


@pytest.fixture(scope="module")
def base(api):
    class Base:
        pass
    b = Base()
    b.positions = synth.triangle_soup(300, 0.2, seed=5)
    b.tris = b.positions.reshape(300, 3, 3)
    b.ds = api.DeviceScene.build([dict(positions=b.positions)])
    b.queries = query_mix(b.tris)
    # the reference, computed once and shared
    b.want_rec, b.want_pts = brute_force(b.tris, np.arange(300, dtype=np.uint32), b.queries["point"], b.queries["max_dist2"])
    return b


def test_query_mix_equals_brute_force(api, base):
    got = scene_triangles(api, base.ds)
    assert got.tobytes() == base.tris.tobytes()                      # (the records are the input's, in input order)
    rec = check(api, base.ds, base.queries, (base.want_rec, base.want_pts))
    hit = rec["prim"] != NONE
    assert 0.7 < hit.mean() < 1.0 and (rec["dist2"][hit] == 0).sum() >= 80
    assert (rec["u"][~hit] == 0).all() and (rec["v"][~hit] == 0).all()
    # the numpy convenience on top of it: the same records for the unlimited queries
    plain = base.queries["max_dist2"] == RTK_INF
    rec2, pts2 = base.ds.closest_points(base.queries["point"][plain])
    assert rec2.tobytes() == rec[plain].tobytes() and pts2.shape == (int(plain.sum()), 3)
    rec3, _ = base.ds.closest_points(base.queries["point"][plain][:50], max_dist=0.05)
    want3, _ = brute_force(base.tris, np.arange(300), base.queries["point"][plain][:50], np.full(50, np.float32(0.05) * np.float32(0.05), np.float32))
    assert rec3.view(np.uint32).reshape(-1, 4).tobytes() == want3.tobytes()


def test_ties_go_to_the_lowest_id(api, base):
    # a mesh listed twice: the same triangles under two id ranges
    ds = api.DeviceScene.build([dict(positions=base.positions), dict(positions=base.positions)])
    q = base.queries[:700]
    rec = check(api, ds, q)
    hit = rec["prim"] != NONE
    assert hit.any() and (rec["prim"][hit] < 300).all()
    # the centre of a symmetric octahedron: eight faces at one distance
    faces = np.array([[[sx, 0, 0], [0, sy, 0], [0, 0, sz]] for sz in (1, -1) for sy in (1, -1) for sx in (1, -1)], np.float32)
    order = np.random.RandomState(3).permutation(8)
    ds = api.DeviceScene.build([dict(positions=faces[order].reshape(-1, 3))])
    centre = make_queries(np.zeros((1, 3), np.float32), np.array([RTK_INF], np.float32))
    d2 = tri_np(centre["point"][:, None, :], faces[None, :, 0], faces[None, :, 1], faces[None, :, 2])[0]
    assert (d2 == d2[0, 0]).all()
    rec = check(api, ds, centre)
    assert rec["prim"][0] == 0 and rec["dist2"][0] == d2[0, 0]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_sizes(api, base, n):
    which = np.arange(n) % len(base.queries)
    q, want_rec, want_pts = base.queries[which], base.want_rec[which], base.want_pts[which]
    rec, pts = run(api, base.ds, q, n=n)
    assert rec[:n].tobytes() == want_rec.tobytes() and pts[:n].tobytes() == want_pts.tobytes()
    rec, pts = run(api, base.ds, q, n=n, with_points=False)           # d_points == NULL
    assert pts is None and rec[:n].tobytes() == want_rec.tobytes()


def test_the_tree_does_not_matter(api, base):
    """A device build, the CPU task builder's blob uploaded (leaves of 4 to 63, loose boxes), that scene after split_leaves, a
    refit to moved positions, a rebuild: each equals brute force over its own records, and where the triangles are the same
    the answers are the same bytes."""
    L = api.lib()
    q = base.queries
    first = base.want_rec.tobytes()
    before = L.rtk_amd_get_builder()
    L.rtk_amd_set_builder(1)
    try:
        p, keep = api.build_scene([dict(positions=base.positions)])
    finally:
        L.rtk_amd_set_builder(before)
    try:
        up = api.DeviceScene.upload(api.scene_bytes(p))
    finally:
        api.free_scene(p)
    same = scene_triangles(api, up).tobytes() == base.tris.tobytes()         # (the blob keeps the input's vertex order)
    got = check(api, up, q)
    assert not same or got.tobytes() == first
    split = up.split_leaves()
    assert split["leaves_split"] > 0
    got = check(api, up, q)
    assert not same or got.tobytes() == first
    # moved positions: their own brute force
    ds = api.DeviceScene.build([dict(positions=base.positions)])
    rng = np.random.RandomState(8)
    moved = (base.positions + rng.uniform(-0.05, 0.05, base.positions.shape)).astype(np.float32)
    ds.refit([dict(positions=moved)])
    assert scene_triangles(api, ds).tobytes() == moved.tobytes()
    after_refit = check(api, ds, q)
    assert after_refit.tobytes() != first
    ds.rebuild()
    assert scene_triangles(api, ds).tobytes() == moved.tobytes()
    assert check(api, ds, q).tobytes() == after_refit.tobytes()


def test_a_stack_deeper_than_the_on_chip_part(api):
    """The geometric cluster of tests/test_gpu_build.py: a deep, lopsided tree whose walk needs the spill area"""
    from tests.test_gpu_build import _adversarial_scenes
    tris = _adversarial_scenes()["geometric_chain"]
    ds = api.DeviceScene.build([dict(positions=tris.reshape(-1, 3))])
    on_chip = api.lib().rtk_amd_closest_stack_entries()
    assert ds.info()["stack_entries"] > on_chip, (ds.info()["stack_entries"], on_chip)
    rng = np.random.RandomState(4)
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    pts = np.concatenate([rng.uniform(lo, hi, (60, 3)), tris[rng.permutation(len(tris))[:40], 0], lo + (hi - lo) * rng.uniform(0, 1, (28, 3)) ** 8]).astype(np.float32)
    q = make_queries(pts, np.full(len(pts), RTK_INF, np.float32))
    rec = check(api, ds, q)
    assert (rec["prim"] != NONE).all()
    # the counting form says that pushes did go past the on-chip part, and gives the same bytes
    d_rec, d_pts, counts = ds.closest_points_counted(api.to_device(q), len(q))
    print("geometric_chain: stack entries %d, on chip %d, counts %s" % (ds.info()["stack_entries"], on_chip, counts))
    assert counts["stack_spills"] > 0 and counts["rays"] == len(q) and counts["hits"] == len(q)
    assert counts["nodes"] >= len(q) and counts["triangles"] >= counts["leaves"] >= len(q)
    assert d_rec.cpu().numpy().view(CLOSEST_RECORD_DTYPE).tobytes() == rec.tobytes()
    assert api.lib().rtk_dev_trace_status(ds.handle, None) == 0


def test_lists(api, base):
    """A shuffled subset with a repeated id, the count on the device: listed slots as the unlisted call, the rest untouched"""
    n = 1000
    q = base.queries[:n]
    want_rec, want_pts = run(api, base.ds, q)
    rng = np.random.RandomState(6)
    ids = rng.permutation(n)[:333]
    ids = np.concatenate([ids, ids[:7], rng.permutation(n)[:100]])           # 7 repeated ids; 100 entries beyond the count
    count = 340
    listed = np.zeros(n + TAIL, bool)
    listed[ids[:count]] = True
    rec, pts = run(api, base.ds, q, count=count, ids=ids)
    assert (rec[~listed] == FILL).all() and (pts[~listed] == FILL).all()
    assert rec[listed].tobytes() == want_rec[listed].tobytes() and pts[listed].tobytes() == want_pts[listed].tobytes()
    # no ids: the first `count` queries; a count beyond the arrays is clamped to them
    rec, pts = run(api, base.ds, q, count=100)
    assert (rec[100:] == FILL).all() and rec[:100].tobytes() == want_rec[:100].tobytes() and (pts[100:] == FILL).all()
    rec, pts = run(api, base.ds, q, count=n + 1000)
    assert rec.tobytes() == want_rec.tobytes() and pts.tobytes() == want_pts.tobytes()
    # an empty list writes nothing
    rec, pts = run(api, base.ds, q, count=0, ids=ids)
    assert (rec == FILL).all() and (pts == FILL).all()


def test_select_takes_the_records_as_they_are(api, base):
    import torch
    n = len(base.queries)
    d_rec, _ = base.ds.closest_points_device(api.to_device(base.queries), n)
    ids, count = base.ds.select_rays(d_rec, api.SELECT_RECORD_HIT, n)
    miss_ids, miss_count = base.ds.select_rays(d_rec, api.SELECT_RECORD_MISS, n)
    torch.cuda.synchronize()
    prim = d_rec.cpu().numpy().view(CLOSEST_RECORD_DTYPE)["prim"]
    hits = np.nonzero(prim != NONE)[0]
    assert int(count[0]) == len(hits) and (ids.cpu().numpy()[:len(hits)] == hits).all()
    misses = np.nonzero(prim == NONE)[0]
    assert int(miss_count[0]) == len(misses) > 0 and (miss_ids.cpu().numpy()[:len(misses)] == misses).all()
    # ... and a second round over the misses alone, with a wider limit, on the list the select made
    wide = base.queries.copy()
    wide["max_dist2"] = RTK_INF
    d_rec2 = d_rec.clone()
    base.ds.closest_points_device(api.to_device(wide), n, d_rec2, count=miss_count, ids=miss_ids, want_points=False)
    rec2 = d_rec2.cpu().numpy().view(CLOSEST_RECORD_DTYPE)
    finite = np.isfinite(base.queries["point"]).all(1)
    assert (rec2["prim"][finite] != NONE).all() and rec2[hits].tobytes() == d_rec.cpu().numpy().view(CLOSEST_RECORD_DTYPE)[hits].tobytes()


def test_two_launches_give_the_same_bytes(api, base):
    a = run(api, base.ds, base.queries)
    b = run(api, base.ds, base.queries)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
