"""GPU tests of rtk_dev_triangles_within_count / rtk_dev_triangles_within_all. The bar everywhere: counts, records and points are
bit for bit what numpy float32 brute force gives by the rules of rtk_amd/csrc/rtk_closest_rule.h and rtk_within_rule.h
(tests/within_ref.py) over the triangle records the scene holds at that moment, whatever tree is above them and whatever order
the walk takes. Every output is pre-filled with 0x7e and carries a tail; whole buffers are compared, so nothing may be written
beyond a query's kept entries, outside the segments or behind the batch. The base scene is the 300-triangle soup of
tests/test_gpu_closest.py; every brute force stays below half a million (point, triangle) pairs."""
import ctypes as C

import numpy as np
import pytest

from rtk_amd import synth
from rtk_amd.types import CLOSEST_RECORD_DTYPE, RTK_INF
from tests.closest_ref import NONE, tri_np
from tests.test_gpu_closest import FILL, TAIL, make_queries, query_mix, scene_triangles
from tests.within_ref import brute_force_within

pytestmark = pytest.mark.gpu


def status_ok(api, ds):
    import torch
    assert api.lib().rtk_dev_trace_status(ds.handle, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0, api.last_error()


def device_queries(api, queries):
    import torch
    return api.to_device(queries) if len(queries) else torch.zeros(16, dtype=torch.uint8, device="cuda")


def list_tensors(count, ids):
    import torch
    d_count = torch.tensor([count], dtype=torch.int64, device="cuda") if count is not None else None
    d_ids = torch.from_numpy(np.ascontiguousarray(ids, np.int64)).cuda() if ids is not None else None
    return d_count, d_ids


def run_count(api, ds, queries, n=None, count=None, ids=None):
    """-> count words [n + TAIL] as the device left them"""
    import torch
    n = len(queries) if n is None else n
    d_counts = torch.full(((n + TAIL) * 4,), 0x7e, dtype=torch.uint8, device="cuda")
    d_count, d_ids = list_tensors(count, ids)
    ds.count_within_device(device_queries(api, queries), n, d_counts, count=d_count, ids=d_ids)
    status_ok(api, ds)
    got = d_counts.cpu().numpy().view(np.uint32)
    assert (got[n:] == FILL).all(), "written beyond num_queries"
    return got


def run_fill(api, ds, queries, offsets, total, n=None, with_points=True, with_written=True, count=None, ids=None):
    """offsets: numpy int64 [n + 1] or a cuda tensor; total: records the segments span. -> (record words [total + TAIL, 4], point
    words [total + TAIL, 3] or None, written words [n + TAIL] or None) as the device left them"""
    import torch
    n = len(queries) if n is None else n
    d_off = offsets if isinstance(offsets, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(offsets, np.int64)).cuda()
    d_rec = torch.full(((total + TAIL) * 16,), 0x7e, dtype=torch.uint8, device="cuda")
    d_pts = torch.full(((total + TAIL) * 12,), 0x7e, dtype=torch.uint8, device="cuda") if with_points else None
    d_wr = torch.full(((n + TAIL) * 4,), 0x7e, dtype=torch.uint8, device="cuda") if with_written else None
    d_count, d_ids = list_tensors(count, ids)
    ds.within_all_device(device_queries(api, queries), n, d_off, d_rec, d_pts, d_wr, count=d_count, ids=d_ids)
    status_ok(api, ds)
    rec = d_rec.cpu().numpy().view(np.uint32).reshape(total + TAIL, 4)
    pts = d_pts.cpu().numpy().view(np.uint32).reshape(total + TAIL, 3) if with_points else None
    wr = d_wr.cpu().numpy().view(np.uint32) if with_written else None
    return rec, pts, wr


def expected_fill(kept, offsets, total, listed=None):
    """The whole output as it must stand: kept[i] at offsets[i] for every (listed) query, 0x7e everywhere else"""
    n = len(kept)
    rec = np.full((total + TAIL, 4), FILL, np.uint32)
    pts = np.full((total + TAIL, 3), FILL, np.uint32)
    wr = np.full(n + TAIL, FILL, np.uint32)
    for i in range(n):
        if listed is not None and not listed[i]:
            continue
        r, p = kept[i]
        room = max(0, int(offsets[i + 1]) - int(offsets[i]))
        assert len(r) <= room or room == 0
        k = min(len(r), room)
        rec[offsets[i]:offsets[i] + k] = r[:k]
        pts[offsets[i]:offsets[i] + k] = p[:k]
        wr[i] = k
    return rec, pts, wr


def assert_fill(got, want, what=""):
    for g, w, name in zip(got, want, ("records", "points", "written")):
        if g is None:
            continue
        if g.tobytes() != w.tobytes():
            bad = np.nonzero((g != w).reshape(len(g), -1).any(1))[0]
            raise AssertionError("%s %s: %d rows differ, first %s: got %s want %s" % (what, name, len(bad), bad[:5], g[bad[:3]], w[bad[:3]]))


def cut(lists, k):
    return [(r[:k], p[:k]) for r, p in lists]


def within_mix(tris, seed=17):
    """The batch of the issue: the 400 uniform points of query_mix's first block, 100 of the scene's vertices and 50 centroids
    with a radius drawn from {0.05, 0.1, 0.2, 0.4} x the largest extent; 8 unlimited queries; query_mix's limit cases; and for
    60 points limits at the float32 neighbour below, at and above the dist2 of their 1st, 2nd and 5th nearest triangle."""
    rng = np.random.RandomState(seed)
    mix = query_mix(tris)
    ext = float((tris.reshape(-1, 3).max(0) - tris.reshape(-1, 3).min(0)).max())
    pts = np.concatenate([mix["point"][:400], mix["point"][400:500], mix["point"][650:700]])
    radius = (rng.choice([0.05, 0.1, 0.2, 0.4], len(pts)) * ext).astype(np.float32)
    max2 = radius * radius
    pts = np.concatenate([pts, pts[:8]])
    max2 = np.concatenate([max2, np.full(8, RTK_INF, np.float32)])
    limits = mix[-48:]                                               # 0, -0, negative, NaN, -inf, 1e-45, a small radius; NaN / +-inf coordinates
    assert np.isnan(limits["max_dist2"]).any() and not np.isfinite(limits["point"]).all()
    some = rng.permutation(550)[:60]
    d2 = np.sort(tri_np(pts[some, None, :], tris[None, :, 0], tris[None, :, 1], tris[None, :, 2])[0], 1)[:, [0, 1, 4]]
    around = np.stack([np.nextafter(d2, np.float32(-1)), d2, np.nextafter(d2, np.float32(np.inf))], 2).reshape(60, 9)
    pts = np.concatenate([pts, limits["point"], np.repeat(pts[some], 9, 0)])
    max2 = np.concatenate([max2, limits["max_dist2"], around.reshape(-1)]).astype(np.float32)
    return make_queries(pts, max2)


@pytest.fixture(scope="module")
def base(api):
    class Base:
        pass
    b = Base()
    b.positions = synth.triangle_soup(300, 0.2, seed=5)
    b.tris = b.positions.reshape(300, 3, 3)
    b.ds = api.DeviceScene.build([dict(positions=b.positions)])
    b.queries = within_mix(b.tris)
    b.n = len(b.queries)
    # the references, computed once and shared
    b.ref = brute_force_within(b.tris, np.arange(300), b.queries["point"], b.queries["max_dist2"])
    b.unlimited = b.queries.copy()
    b.unlimited["max_dist2"] = RTK_INF
    b.ref_inf = brute_force_within(b.tris, np.arange(300), b.unlimited["point"], b.unlimited["max_dist2"])
    b.offsets = np.concatenate([[0], np.cumsum(b.ref.counts.astype(np.int64))])
    return b


def test_the_reference_has_empty_short_and_long_lists(base):
    c = base.ref.counts
    print("queries %d, pairs %d, mean count %.1f, max %d, empty %.0f %%" % (base.n, int(c.sum()), c.mean(), c.max(), 100 * (c == 0).mean()))
    assert (c == 0).any() and (c == 1).any() and (c > 64).any() and (c[550:558] == 300).all()
    assert (c[558:606] == 0).sum() >= 40                             # the limit cases
    # the strict <: a limit AT the k-th distance leaves that triangle out, the neighbour above takes it in
    around = c[606:].reshape(60, 3, 3)                               # [point, rank 1 / 2 / 5, below / at / above]
    assert (around[:, :, 0] == around[:, :, 1]).all() and (around[:, :, 2] > around[:, :, 1]).all()
    assert (around[:, 0, 1] == 0).all() and (around[:, 0, 2] >= 1).all()


def test_count_equals_brute_force(api, base):
    assert scene_triangles(api, base.ds).tobytes() == base.tris.tobytes()
    got = run_count(api, base.ds, base.queries)
    bad = np.nonzero(got[:base.n] != base.ref.counts)[0]
    assert len(bad) == 0, (len(bad), bad[:5], base.queries[bad[:5]], got[bad[:5]], base.ref.counts[bad[:5]])


def test_fill_with_exact_offsets(api, base):
    """count, torch.cumsum, fill on one stream without a wait in between; then the same with d_points = NULL and d_written = NULL"""
    import torch
    n, total = base.n, int(base.offsets[-1])
    d_q = api.to_device(base.queries)
    d_counts = base.ds.count_within_device(d_q, n)
    d_offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_offsets[1:] = torch.cumsum(d_counts, 0, dtype=torch.int64)
    got = run_fill(api, base.ds, base.queries, d_offsets, total)     # (the buffers are sized from the reference: nothing is read back before)
    assert d_offsets.cpu().numpy().tobytes() == base.offsets.tobytes()
    want = expected_fill(base.ref.lists, base.offsets, total)
    assert_fill(got, want, "exact offsets")
    assert got[2][:n].tobytes() == base.ref.counts.tobytes()
    assert_fill(run_fill(api, base.ds, base.queries, base.offsets, total, with_points=False), want, "no points")
    assert_fill(run_fill(api, base.ds, base.queries, base.offsets, total, with_written=False), want, "no written")
    assert_fill(run_fill(api, base.ds, base.queries, base.offsets, total, with_points=False, with_written=False), want, "records alone")


@pytest.mark.parametrize("k", [0, 1, 3, 8])
def test_k_nearest(api, base, k):
    n = base.n
    offsets = np.arange(n + 1, dtype=np.int64) * k
    for queries, ref, what in ((base.queries, base.ref, "radii"), (base.unlimited, base.ref_inf, "unlimited")):
        got = run_fill(api, base.ds, queries, offsets, n * k)
        assert_fill(got, expected_fill(cut(ref.lists, k), offsets, n * k), "k = %d, %s" % (k, what))
        assert got[2][:n].tobytes() == np.minimum(ref.counts, k).astype(np.uint32).tobytes()
        if k == 0:
            continue
        # the first entry is word for word what closest points writes; its miss goes with an empty segment
        d_rec, d_pts = base.ds.closest_points_device(api.to_device(queries), n)
        c_rec = d_rec.cpu().numpy().view(np.uint32).reshape(n, 4)
        c_pts = d_pts.cpu().numpy().view(np.uint32).reshape(n, 3)
        some = got[2][:n] > 0
        assert ((c_rec[:, 3] == NONE) == ~some).all()
        assert got[0][:n * k].reshape(n, k, 4)[some, 0].tobytes() == c_rec[some].tobytes()
        assert got[1][:n * k].reshape(n, k, 3)[some, 0].tobytes() == c_pts[some].tobytes()


def test_ragged_room(api, base):
    """Room 0 .. 6 per query, and one pair of decreasing offsets: the kept prefix, nothing for the query without room"""
    rng = np.random.RandomState(9)
    n = base.n
    room = rng.randint(0, 7, n)
    assert (room == 0).sum() > 50
    offsets = np.concatenate([[0], np.cumsum(room)]).astype(np.int64)
    # query j's offsets decrease: offsets[j] is raised, which only widens the room of query j - 1, a query without candidates
    j = [i for i in range(100, n - 1) if base.ref.counts[i - 1] == 0 and base.ref.counts[i] > 0][0]
    offsets[j] += 5
    assert offsets[j + 1] < offsets[j]
    total = int(offsets.max())
    rooms = np.maximum(offsets[1:] - offsets[:-1], 0)
    kept = [(r[:rooms[i]], p[:rooms[i]]) for i, (r, p) in enumerate(base.ref.lists)]
    assert len(kept[j][0]) == 0 and any(len(r) == 6 for r, _ in kept) and any(0 < len(r) < rooms[i] for i, (r, _) in enumerate(kept))
    got = run_fill(api, base.ds, base.queries, offsets, total)
    want = expected_fill(kept, offsets, total)
    assert want[2][j] == 0
    assert_fill(got, want, "ragged")


def test_ties_go_to_the_lowest_id_first(api, base):
    # a mesh listed twice: the same triangles under two id ranges
    ds = api.DeviceScene.build([dict(positions=base.positions), dict(positions=base.positions)])
    q = base.queries[:550:2]
    n = len(q)
    tris = scene_triangles(api, ds)
    assert tris[:300].tobytes() == tris[300:].tobytes()
    ref = brute_force_within(tris, np.arange(600), q["point"], q["max_dist2"])
    assert (ref.counts == 2 * base.ref.counts[:550:2]).all()
    assert run_count(api, ds, q)[:n].tobytes() == ref.counts.tobytes()
    offsets = np.concatenate([[0], np.cumsum(ref.counts.astype(np.int64))])
    got = run_fill(api, ds, q, offsets, int(offsets[-1]))
    assert_fill(got, expected_fill(ref.lists, offsets, int(offsets[-1])), "doubled mesh")
    pairs = got[0][:int(offsets[-1])].reshape(-1, 2, 4)              # every distance twice, the lower id first
    assert (pairs[:, 0, 0] == pairs[:, 1, 0]).all() and (pairs[:, 0, 3] + 300 == pairs[:, 1, 3]).all()
    first = run_fill(api, ds, q, np.arange(n + 1, dtype=np.int64), n)
    assert_fill(first, expected_fill(cut(ref.lists, 1), np.arange(n + 1), n), "doubled mesh, k = 1")
    assert (first[0][:n][first[2][:n] == 1, 3] < 300).all() and (first[2][:n] == 1).any()
    # the centre of a symmetric octahedron: eight faces at one distance
    faces = np.array([[[sx, 0, 0], [0, sy, 0], [0, 0, sz]] for sz in (1, -1) for sy in (1, -1) for sx in (1, -1)], np.float32)
    order = np.random.RandomState(3).permutation(8)
    ds = api.DeviceScene.build([dict(positions=faces[order].reshape(-1, 3))])
    centre = make_queries(np.zeros((1, 3), np.float32), np.array([RTK_INF], np.float32))
    ref = brute_force_within(scene_triangles(api, ds), np.arange(8), centre["point"], centre["max_dist2"])
    assert ref.counts[0] == 8 and (ref.lists[0][0][:, 0] == ref.lists[0][0][0, 0]).all()
    got = run_fill(api, ds, centre, np.array([0, 3], np.int64), 3)
    assert_fill(got, expected_fill(cut(ref.lists, 3), np.array([0, 3]), 3), "octahedron")
    assert got[0][:3, 3].tolist() == [0, 1, 2] and run_count(api, ds, centre)[0] == 8


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_sizes(api, base, n):
    which = np.arange(n) % base.n
    q = base.queries[which]
    got = run_count(api, base.ds, q, n=n)
    assert got[:n].tobytes() == base.ref.counts[which].tobytes()
    offsets = np.arange(n + 1, dtype=np.int64) * 3
    kept = cut([base.ref.lists[i] for i in which], 3)
    assert_fill(run_fill(api, base.ds, q, offsets, n * 3, n=n), expected_fill(kept, offsets, n * 3), "n = %d" % n)


def check_scene(api, ds, q, ref=None):
    """count, exact fill and k = 3 fill of one scene against brute force over its own records; returns the bytes of all three"""
    n = len(q)
    if ref is None:
        tris = scene_triangles(api, ds)
        ref = brute_force_within(tris, np.arange(len(tris)), q["point"], q["max_dist2"])
    counts = run_count(api, ds, q)
    assert counts[:n].tobytes() == ref.counts.tobytes()
    offsets = np.concatenate([[0], np.cumsum(ref.counts.astype(np.int64))])
    full = run_fill(api, ds, q, offsets, int(offsets[-1]))
    assert_fill(full, expected_fill(ref.lists, offsets, int(offsets[-1])), "exact offsets")
    k3 = np.arange(n + 1, dtype=np.int64) * 3
    three = run_fill(api, ds, q, k3, n * 3)
    assert_fill(three, expected_fill(cut(ref.lists, 3), k3, n * 3), "k = 3")
    return b"".join(x.tobytes() for x in (counts,) + full + three)


def test_the_tree_does_not_matter(api, base):
    """A device build, the CPU task builder's blob uploaded (leaves of 4 to 63, loose boxes), that scene after split_leaves, a
    refit to moved positions, a rebuild: each equals brute force over its own records, and where the triangles are the same
    the answers are the same bytes."""
    L = api.lib()
    q = base.queries
    first = check_scene(api, base.ds, q, base.ref)
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
    got = check_scene(api, up, q, base.ref if same else None)
    assert not same or got == first
    split = up.split_leaves()
    assert split["leaves_split"] > 0
    got = check_scene(api, up, q, base.ref if same else None)
    assert not same or got == first
    # moved positions: their own brute force
    ds = api.DeviceScene.build([dict(positions=base.positions)])
    rng = np.random.RandomState(8)
    moved = (base.positions + rng.uniform(-0.05, 0.05, base.positions.shape)).astype(np.float32)
    ds.refit([dict(positions=moved)])
    assert scene_triangles(api, ds).tobytes() == moved.tobytes()
    ref = brute_force_within(moved.reshape(300, 3, 3), np.arange(300), q["point"], q["max_dist2"])
    after_refit = check_scene(api, ds, q, ref)
    assert after_refit != first
    ds.rebuild()
    assert scene_triangles(api, ds).tobytes() == moved.tobytes()
    assert check_scene(api, ds, q, ref) == after_refit


def test_a_stack_deeper_than_the_on_chip_part(api):
    """The geometric cluster of tests/test_gpu_build.py: a deep, lopsided tree whose walk needs the spill area"""
    import torch
    from tests.test_gpu_build import _adversarial_scenes
    tris = _adversarial_scenes()["geometric_chain"]
    ds = api.DeviceScene.build([dict(positions=tris.reshape(-1, 3))])
    on_chip = api.lib().rtk_amd_within_stack_entries()
    assert ds.info()["stack_entries"] > on_chip, (ds.info()["stack_entries"], on_chip)
    rng = np.random.RandomState(4)
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    pts = np.concatenate([rng.uniform(lo, hi, (60, 3)), tris[rng.permutation(len(tris))[:40], 0], lo + (hi - lo) * rng.uniform(0, 1, (28, 3)) ** 8]).astype(np.float32)
    assert len(pts) * len(tris) <= 500000
    q = make_queries(pts, np.full(len(pts), RTK_INF, np.float32))
    n = len(q)
    own = scene_triangles(api, ds)
    ref = brute_force_within(own, np.arange(len(own)), q["point"], q["max_dist2"])
    assert (ref.counts == len(own)).all()
    counts = run_count(api, ds, q)
    assert counts[:n].tobytes() == ref.counts.tobytes()
    offsets = np.arange(n + 1, dtype=np.int64) * 4
    want = expected_fill(cut(ref.lists, 4), offsets, n * 4)
    assert_fill(run_fill(api, ds, q, offsets, n * 4), want, "k = 4")
    # the counting forms say that pushes did go past the on-chip part, and give the same bytes
    d_q = api.to_device(q)
    d_counts, visits = ds.triangles_within_counted(d_q, n)
    print("geometric_chain: stack entries %d, on chip %d, count form %s" % (ds.info()["stack_entries"], on_chip, visits))
    assert visits["stack_spills"] > 0 and visits["rays"] == n and visits["hits"] == n and visits["triangles"] == n * len(own)
    assert d_counts.cpu().numpy().view(np.uint32).tobytes() == ref.counts.tobytes()
    d_rec = torch.full(((n * 4 + TAIL) * 16,), 0x7e, dtype=torch.uint8, device="cuda")
    d_pts = torch.full(((n * 4 + TAIL) * 12,), 0x7e, dtype=torch.uint8, device="cuda")
    d_wr = torch.full(((n + TAIL) * 4,), 0x7e, dtype=torch.uint8, device="cuda")
    _, visits = ds.triangles_within_counted(d_q, n, torch.from_numpy(offsets).cuda(), d_rec, d_pts, d_wr)
    print("geometric_chain: fill form k = 4 %s" % (visits,))
    assert visits["stack_spills"] > 0 and visits["rays"] == n and visits["hits"] == n and visits["nodes"] >= n
    assert visits["triangles"] < n * len(own)                        # (the full segment culls)
    got = (d_rec.cpu().numpy().view(np.uint32).reshape(-1, 4), d_pts.cpu().numpy().view(np.uint32).reshape(-1, 3), d_wr.cpu().numpy().view(np.uint32))
    assert_fill(got, want, "counted k = 4")
    assert api.lib().rtk_dev_trace_status(ds.handle, None) == 0


def test_lists(api, base):
    """A shuffled subset with repeated ids, the count on the device: listed slots as the unlisted call, the rest untouched"""
    import torch
    n = 1000
    q = base.queries[:n]
    lists = base.ref.lists[:n]
    rng = np.random.RandomState(6)
    ids = rng.permutation(n)[:333]
    ids = np.concatenate([ids, ids[:7], rng.permutation(n)[:100]])           # 7 repeated ids; 100 entries beyond the count
    count = 340
    listed = np.zeros(n, bool)
    listed[ids[:count]] = True
    got = run_count(api, base.ds, q, count=count, ids=ids)
    assert (got[:n][~listed] == FILL).all() and got[:n][listed].tobytes() == base.ref.counts[:n][listed].tobytes()
    # the fill: segments of 4 per slot, and exact offsets
    k4 = np.arange(n + 1, dtype=np.int64) * 4
    exact = base.offsets[:n + 1]
    for offsets, kept in ((k4, cut(lists, 4)), (exact, lists)):
        total = int(offsets[-1])
        unlisted_run = run_fill(api, base.ds, q, offsets, total)
        assert_fill(unlisted_run, expected_fill(kept, offsets, total), "all")
        got = run_fill(api, base.ds, q, offsets, total, count=count, ids=ids)
        assert_fill(got, expected_fill(kept, offsets, total, listed), "listed")
    # no ids: the first `count` queries; a count beyond the arrays is clamped to them
    first = np.arange(n) < 100
    assert_fill(run_fill(api, base.ds, q, k4, n * 4, count=100), expected_fill(cut(lists, 4), k4, n * 4, first), "count alone")
    assert_fill(run_fill(api, base.ds, q, k4, n * 4, count=n + 1000), expected_fill(cut(lists, 4), k4, n * 4), "count clamped")
    got = run_count(api, base.ds, q, count=100)
    assert (got[100:] == FILL).all() and got[:100].tobytes() == base.ref.counts[:100].tobytes()
    # an empty list writes nothing
    got = run_fill(api, base.ds, q, k4, n * 4, count=0, ids=ids)
    assert all((x == FILL).all() for x in got) and (run_count(api, base.ds, q, count=0, ids=ids) == FILL).all()
    # a list rtk_dev_select_rays made from a closest-points result (the hits) is taken as it stands
    d_q = api.to_device(q)
    d_rec, _ = base.ds.closest_points_device(d_q, n)
    hit_ids, hit_count = base.ds.select_rays(d_rec, api.SELECT_RECORD_HIT, n)
    d_out = torch.full(((n * 4 + TAIL) * 16,), 0x7e, dtype=torch.uint8, device="cuda")
    d_pts = torch.full(((n * 4 + TAIL) * 12,), 0x7e, dtype=torch.uint8, device="cuda")
    d_wr = torch.full(((n + TAIL) * 4,), 0x7e, dtype=torch.uint8, device="cuda")
    base.ds.within_all_device(d_q, n, torch.from_numpy(k4).cuda(), d_out, d_pts, d_wr, count=hit_count, ids=hit_ids)
    status_ok(api, base.ds)
    hits = base.ref.counts[:n] > 0
    assert 0 < hits.sum() < n and int(hit_count[0]) == hits.sum()
    got = (d_out.cpu().numpy().view(np.uint32).reshape(-1, 4), d_pts.cpu().numpy().view(np.uint32).reshape(-1, 3), d_wr.cpu().numpy().view(np.uint32))
    assert_fill(got, expected_fill(cut(lists, 4), k4, n * 4, hits), "a select's list")


def test_two_launches_give_the_same_bytes_and_a_side_stream_sees_its_offsets(api, base):
    import torch
    n, total = base.n, int(base.offsets[-1])
    want = expected_fill(base.ref.lists, base.offsets, total)
    a = run_fill(api, base.ds, base.queries, base.offsets, total)
    b = run_fill(api, base.ds, base.queries, base.offsets, total)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert_fill(a, want, "first launch")
    # count, cumsum and fill enqueued on a side stream, nothing waited for in between
    d_q = api.to_device(base.queries)
    d_rec = torch.full(((total + TAIL) * 16,), 0x7e, dtype=torch.uint8, device="cuda")
    d_pts = torch.full(((total + TAIL) * 12,), 0x7e, dtype=torch.uint8, device="cuda")
    d_wr = torch.full(((n + TAIL) * 4,), 0x7e, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_counts = base.ds.count_within_device(d_q, n)
        d_offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        d_offsets[1:] = torch.cumsum(d_counts, 0, dtype=torch.int64)
        base.ds.within_all_device(d_q, n, d_offsets, d_rec, d_pts, d_wr)
        status_ok(api, base.ds)
    side.synchronize()
    got = (d_rec.cpu().numpy().view(np.uint32).reshape(-1, 4), d_pts.cpu().numpy().view(np.uint32).reshape(-1, 3), d_wr.cpu().numpy().view(np.uint32))
    assert_fill(got, want, "side stream")


def test_python_conveniences(api, base):
    """triangles_within and nearest_triangles return what the device forms computed, for 50 queries"""
    pts = base.queries["point"][:50]
    radius = np.sqrt(base.queries["max_dist2"][:50])
    max2 = (radius * radius).astype(np.float32)                      # (the convenience squares a distance in float32)
    ref = brute_force_within(base.tris, np.arange(300), pts, max2)
    assert ref.counts.sum() > 100
    offsets, rec, points, written = base.ds.triangles_within(pts, radius)
    assert offsets.dtype == np.int64 and offsets.tobytes() == np.concatenate([[0], np.cumsum(ref.counts.astype(np.int64))]).tobytes()
    assert rec.dtype == CLOSEST_RECORD_DTYPE and points.shape == (int(offsets[-1]), 3) and points.dtype == np.float32
    assert written.dtype == np.uint32 and written.tobytes() == ref.counts.tobytes()
    assert rec.tobytes() == np.concatenate([r for r, _ in ref.lists]).tobytes()
    assert points.tobytes() == np.concatenate([p for _, p in ref.lists]).tobytes()
    offsets, rec, points, written = base.ds.triangles_within(pts, radius, max_per_point=3)
    assert offsets.tolist() == list(range(0, 153, 3)) and written.tobytes() == np.minimum(ref.counts, 3).astype(np.uint32).tobytes()
    for i, (r, p) in enumerate(cut(ref.lists, 3)):
        assert rec[3 * i:3 * i + len(r)].tobytes() == r.tobytes() and points[3 * i:3 * i + len(r)].tobytes() == p.tobytes()
        assert not rec[3 * i + len(r):3 * i + 3].view(np.uint32).any()       # (beyond written: zero)
    ref_inf = brute_force_within(base.tris, np.arange(300), pts, np.full(50, RTK_INF, np.float32))
    rec, points, written = base.ds.nearest_triangles(pts, 8)
    assert rec.shape == (50, 8) and points.shape == (50, 8, 3) and (written == 8).all()
    assert rec.tobytes() == np.concatenate([r[:8] for r, _ in ref_inf.lists]).tobytes()
    assert points.tobytes() == np.concatenate([p[:8] for _, p in ref_inf.lists]).tobytes()
    rec, points, written = base.ds.nearest_triangles(pts, 2, max_dist=radius)
    assert written.tobytes() == np.minimum(ref.counts, 2).astype(np.uint32).tobytes()
    o, r0, p0, w0 = base.ds.triangles_within(np.zeros((0, 3), np.float32), 1.0)
    assert o.tolist() == [0] and len(r0) == 0 and p0.shape == (0, 3) and len(w0) == 0
