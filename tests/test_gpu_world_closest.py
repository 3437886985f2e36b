"""Closest points on an instanced world on the GPU (rtk_dev_world_closest_points, rtk_world_closest.hip). Every comparison is an
equality of the bits of dist2, u, v, prim, instance and point: against numpy float32 brute force over (instance, primitive) by
the rule of rtk_amd/csrc/rtk_world_closest_rule.h (tests/world_closest_ref.py), and against the flat placed twin --
DeviceScene.build of the live instances' meshes under their placements, asked by closest_points_device. Scenes and cases are
tests/test_gpu_world.py's. Outputs are pre-filled with 0x7e and carry a tail that must stay untouched."""
import numpy as np
import pytest

from rtk_amd.types import CLOSEST_RECORD_DTYPE, POINT_QUERY_DTYPE
from tests import many_passes as M
from tests import world_closest_ref as R
from tests import world_ref
from tests.test_gpu_world import TRIS, case
from tests.world_ref import F, PRIM_NONE, RTK_INF, placement, rotation

pytestmark = pytest.mark.gpu

TAIL = 5
FILL = 0x7e7e7e7e
N_LIVE, N_MISS, N_DEAD = 4096, 512, 64


@pytest.fixture(scope="module")
def scenes(api):
    return [api.DeviceScene.build([dict(positions=t.reshape(-1, 3))]) for t in TRIS]


def make_queries(points, max2):
    q = np.zeros(len(points), POINT_QUERY_DTYPE)
    q["point"], q["max_dist2"] = points, max2
    return q


_CASES = {}


def reference(name):
    """(which, places, queries, (record words, instances, point words)): the reference, computed once per case and shared"""
    if name not in _CASES:
        which, places = case(name)
        rng = np.random.RandomState(41)
        points, max2 = R.make_queries(TRIS, which, places, rng, N_LIVE // 2, N_LIVE // 2, N_MISS, N_DEAD)
        # the misses: a thousandth of the distance brute force finds without a limit
        rows = slice(N_LIVE, N_LIVE + N_MISS)
        free, _, _ = R.brute_force(TRIS, which, places, points[rows], np.full(N_MISS, RTK_INF, F), prune=True)
        max2[rows] = free[:, 0].view(F) * F(1e-6)
        assert (max2[rows] > 0).all()
        want = R.brute_force(TRIS, which, places, points, max2, prune=len(which) > 4)
        _CASES[name] = (which, places, make_queries(points, max2), want)
    return _CASES[name]


def run(api, world, queries, n=None, with_points=True, count=None, ids=None, **filt):
    """-> (record words [n + TAIL, 4], instances [n + TAIL], point words [n + TAIL, 3] or None) as the device left them"""
    import torch
    n = len(queries) if n is None else n
    d_rec = torch.full(((n + TAIL) * 16,), 0x7e, dtype=torch.uint8, device="cuda")
    d_inst = torch.full(((n + TAIL) * 4,), 0x7e, dtype=torch.uint8, device="cuda")
    d_pts = torch.full(((n + TAIL) * 12,), 0x7e, dtype=torch.uint8, device="cuda") if with_points else None
    d_count = torch.tensor([count], dtype=torch.int64, device="cuda") if count is not None else None
    d_ids = torch.from_numpy(np.ascontiguousarray(ids, np.int64)).cuda() if ids is not None else None
    world.closest_points_device(api.to_device(queries), n, d_rec, d_inst, d_pts, count=d_count, ids=d_ids, want_points=with_points, **filt)
    world.status()
    rec = d_rec.cpu().numpy().view(np.uint32).reshape(n + TAIL, 4)
    inst = d_inst.cpu().numpy().view(np.uint32)
    pts = d_pts.cpu().numpy().view(np.uint32).reshape(n + TAIL, 3) if with_points else None
    assert (rec[n:] == FILL).all() and (inst[n:] == FILL).all() and (pts is None or (pts[n:] == FILL).all()), "written beyond num_queries"
    return rec, inst, pts


def same(got, want, rows=None):
    """bit for bit in dist2, u, v, prim, the instance and the point"""
    n = len(want[0])
    g = [got[0][:n], got[1][:n], got[2][:n]]
    bad = (g[0] != want[0]).any(1) | (g[1] != want[1]) | (g[2] != want[2]).any(1)
    if rows is not None:
        bad = bad & rows
    assert not bad.any(), (int(bad.sum()), np.flatnonzero(bad)[:6], g[0][bad][:3], g[1][bad][:3], want[0][bad][:3], want[1][bad][:3])


def twin_answer(api, which, places, queries):
    """the flat placed twin's answer, its prim mapped back through mesh_base to (instance, prim in the instance's scene)"""
    live = np.flatnonzero(R.live_instances(TRIS, which, places))
    twin = api.DeviceScene.build([dict(positions=TRIS[which[k]].reshape(-1, 3)) for k in live], placements=places[live])
    base = np.asarray(twin.mesh_base(), np.int64)
    n = len(queries)
    d_rec, d_pts = twin.closest_points_device(api.to_device(queries), n)
    rec = d_rec.cpu().numpy().view(np.uint32).reshape(n, 4).copy()
    pts = d_pts.cpu().numpy().view(np.uint32).reshape(n, 3)
    hit = rec[:, 3] != PRIM_NONE
    mesh = np.searchsorted(base[:len(live)], rec[hit, 3].astype(np.int64), side="right") - 1
    inst = np.full(n, PRIM_NONE, np.uint32)
    inst[hit] = live[mesh]
    rec[hit, 3] = (rec[hit, 3].astype(np.int64) - base[mesh]).astype(np.uint32)
    return rec, inst, pts


def scene_triangles(api, ds):
    from tests.test_gpu_closest import scene_triangles as st
    return st(api, ds)


@pytest.mark.parametrize("name", ["one", "two", "65", "257", "special"])
def test_world_equals_brute_force_and_the_flat_twin(api, scenes, name):
    which, places, q, want = reference(name)
    rec, inst, pts = want
    # from the reference alone: the live queries hit, the limited ones and the dead ones miss
    hit = rec[:, 3] != PRIM_NONE
    assert len(q) == N_LIVE + N_MISS + N_DEAD and hit[:N_LIVE].all() and not hit[N_LIVE:].any()
    assert (inst[~hit] == PRIM_NONE).all() and (rec[~hit, 0] == q["max_dist2"][~hit].view(np.uint32)).all() and (rec[~hit, 1:3] == 0).all()
    assert (pts[~hit] == q["point"][~hit].view(np.uint32)).all()
    if name in ("65", "257"):
        # the top level's ordering decides something: the answer is often not in the instance whose proxy box is nearest
        from tests.world_ref import box_np
        boxes = [box_np(TRIS[which[k]].reshape(-1, 3).min(0), TRIS[which[k]].reshape(-1, 3).max(0), places[k]) for k in range(len(which))]
        bound = np.stack([R.closest_ref.box_np(q["point"][:N_LIVE], b[0], b[1]) for b in boxes], 1)
        other = inst[:N_LIVE] != bound.argmin(1)
        print("case %s: %.1f %% of the answers are not in the instance of the nearest proxy box" % (name, 100 * other.mean()))
        assert other.mean() >= 0.05
    world = api.DeviceWorld.create(scenes, which, places)
    got = run(api, world, q)
    same(got, want)
    same(got, twin_answer(api, which, places, q))
    # without points, and the numpy convenience
    rec2, inst2, none = run(api, world, q, with_points=False)
    assert none is None and (rec2[:len(q)] == rec).all() and (inst2[:len(q)] == inst).all()
    r3, i3, p3 = world.closest_points(q["point"][:100])
    assert (r3.view(np.uint32).reshape(-1, 4) == rec[:100]).all() and (i3 == inst[:100]).all() and (p3.view(np.uint32) == pts[:100]).all()
    # rebuild changes no byte
    world.rebuild()
    same(run(api, world, q), want)
    world.free()


def test_the_trees_do_not_matter(api, scenes):
    """The instances' scenes from the CPU task builder's blob (leaves of 4 to 63, loose boxes) with split_leaves applied: the same bytes"""
    which, places, q, want = reference("special")
    L = api.lib()
    ups = []
    for t in TRIS:
        before = L.rtk_amd_get_builder()
        L.rtk_amd_set_builder(1)
        try:
            p, keep = api.build_scene([dict(positions=t.reshape(-1, 3))])
        finally:
            L.rtk_amd_set_builder(before)
        try:
            up = api.DeviceScene.upload(api.scene_bytes(p))
        finally:
            api.free_scene(p)
        up.split_leaves()
        ups.append(up)
    mine = [scene_triangles(api, s) for s in ups]
    if not all(a.tobytes() == b.tobytes() for a, b in zip(mine, TRIS)):      # (a blob that orders its records otherwise: their own brute force)
        want = R.brute_force(mine, which, places, q["point"], q["max_dist2"])
    world = api.DeviceWorld.create(ups, which, places)
    same(run(api, world, q), want)
    world.free()


def test_ties_go_to_the_lowest_instance(api, scenes):
    which, places, q, want = reference("special")
    # an instance duplicated exactly, under a HIGHER number: nothing changes; under a LOWER number the answers move to it
    w2, p2 = np.concatenate([which, which[:1]]), np.concatenate([places, places[:1]])
    world = api.DeviceWorld.create(scenes, w2, p2)
    got = run(api, world, q)
    same(got, want)
    assert (want[1] == 0).sum() > 500 and (got[1] != 4).all()
    world.free()
    w3, p3 = np.concatenate([which[3:4], which]), np.concatenate([places[3:4], places])
    world = api.DeviceWorld.create(scenes, w3, p3)
    got = run(api, world, q)
    moved = np.where(want[1] == PRIM_NONE, PRIM_NONE, np.where(want[1] == 3, 0, want[1] + 1)).astype(np.uint32)
    same(got, (want[0], moved, want[2]))
    assert (want[1] == 3).sum() > 100
    world.free()
    # two cubes that share the face x = 1 / x = -1 (placed at x = -1 and x = +1: the face is the plane x = 0): points of that plane
    # and points equidistant from two faces by construction (on a diagonal plane of the edge) -- the reference's answer
    cubes = np.array([placement(None, (-1, 0, 0)), placement(None, (1, 0, 0))], F)
    wc = np.array([0, 0], np.uint32)
    rng = np.random.RandomState(43)
    on_face = np.concatenate([np.zeros((200, 1)), rng.uniform(-1, 1, (200, 2))], 1)
    t = rng.uniform(0.25, 2.0, (200, 1))
    off_edge = np.concatenate([np.zeros((200, 1)), rng.uniform(-0.5, 0.5, (200, 1)), 1.0 + t], 1)          # above the shared edge z = 1, x = 0
    pts = np.concatenate([on_face, off_edge]).astype(F)
    qq = make_queries(pts, np.full(len(pts), RTK_INF, F))
    ref = R.brute_force(TRIS, wc, cubes, pts, qq["max_dist2"])
    per = [R.brute_force(TRIS, wc[k:k + 1], cubes[k:k + 1], pts, qq["max_dist2"])[0][:, 0] for k in range(2)]
    tie = per[0] == per[1]                                                   # (above the edge every one; in the face those whose q rounds alike in both cubes)
    assert tie[200:].all() and tie[:200].mean() > 0.5 and (ref[1][tie] == 0).all() and (ref[1] == 1).any()      # an exact tie: the lower instance
    world = api.DeviceWorld.create(scenes, wc, cubes)
    same(run(api, world, qq), ref)
    # ... and with the lower one ignored per slot the other answers, at the same dist2
    got = run(api, world, qq, ignore_instance=np.zeros(len(pts), np.uint32))
    assert (got[1][:len(pts)] == 1).all() and (got[0][:len(pts), 0] == per[1]).all()
    world.free()


def test_dead_instances_change_nothing(api, scenes):
    which, places, q, want = reference("special")
    empty = api.DeviceScene.build([dict(positions=np.zeros((0, 3), F))])
    singular = placement(np.array([[1, 2, 3], [1, 2, 3], [0, 0, 1]]), (0, 0, 0))
    nan = placement(None, (np.nan, 0, 0))
    which2 = np.concatenate([which, [1, 3, 0]]).astype(np.uint32)           # a singular sphere, a placed empty scene, a NaN cube
    places2 = np.concatenate([places, [singular, placement(None, (0, 0, 0)), nan]])
    world = api.DeviceWorld.create(scenes + [empty], which2, places2)
    assert world.info()["dead_instances"] == 3
    same(run(api, world, q), want)
    world.free()


def test_filters(api, scenes):
    which, places, q, want = reference("65")
    points, max2 = q["point"], q["max_dist2"]
    world = api.DeviceWorld.create(scenes, which, places)
    # the instance mask: the odd instances and those beyond bit 60 are out
    mask = np.zeros(60, bool)
    mask[::2] = True
    ref = R.brute_force(TRIS, which, places, points, max2, mask=mask, prune=True)
    assert (ref[1] != want[1]).mean() > 0.3
    same(run(api, world, q, instance_mask=mask), ref)
    # per slot the instance of the unfiltered answer is ignored (self-exclusion): brute force over the rest
    ign = want[1].copy()
    ign[::7] = PRIM_NONE
    ref = R.brute_force(TRIS, which, places, points, max2, ignore=ign, prune=True)
    got = run(api, world, q, ignore_instance=ign)
    same(got, ref)
    live = ign[:N_LIVE] != PRIM_NONE
    assert (got[1][:N_LIVE][live] != ign[:N_LIVE][live]).all() and (got[0][:N_LIVE, 3] != PRIM_NONE).all()
    # both at once; and a mask that lets nothing through gives misses
    ref = R.brute_force(TRIS, which, places, points, max2, mask=mask, ignore=ign, prune=True)
    same(run(api, world, q, instance_mask=mask, ignore_instance=ign), ref)
    rec, inst, pts = run(api, world, q, instance_mask=np.zeros(65, bool))
    n = len(q)
    assert (rec[:n, 3] == PRIM_NONE).all() and (inst[:n] == PRIM_NONE).all() and (rec[:n, 0] == max2.view(np.uint32)).all()
    assert (rec[:n, 1:3] == 0).all() and (pts[:n] == points.view(np.uint32)).all()
    world.free()


def test_lists(api, scenes):
    which, places, q, want = reference("65")
    n = 1000
    q, want = q[:n], tuple(w[:n] for w in want)
    world = api.DeviceWorld.create(scenes, which, places)
    rng = np.random.RandomState(6)
    ids = rng.permutation(n)[:333]
    ids = np.concatenate([ids, ids[:7], [n, n + 3, 0xFFFFFFFF], rng.permutation(n)[:100]])       # 7 repeated ids, 3 ids >= n; 100 entries beyond the count
    count = 343
    listed = np.zeros(n + TAIL, bool)
    listed[ids[:340]] = True
    rec, inst, pts = run(api, world, q, count=count, ids=ids)
    assert (rec[~listed] == FILL).all() and (inst[~listed] == FILL).all() and (pts[~listed] == FILL).all()
    same((rec, inst, pts), want, rows=listed[:n])
    # no ids: the first `count` queries; a count beyond the arrays is clamped to them; an empty list writes nothing
    rec, inst, pts = run(api, world, q, count=100)
    assert (rec[100:] == FILL).all() and (inst[100:] == FILL).all() and (pts[100:] == FILL).all()
    same((rec, inst, pts), want, rows=np.arange(n) < 100)
    same(run(api, world, q, count=n + 1000), want)
    rec, inst, pts = run(api, world, q, count=0, ids=ids)
    assert (rec == FILL).all() and (inst == FILL).all() and (pts == FILL).all()
    # the record is a closest record: select takes it, and a second round answers the misses alone
    import torch
    full = reference("65")[2]
    d_rec, d_inst, _ = world.closest_points_device(api.to_device(full), len(full))
    miss_ids, miss_count = scenes[0].select_rays(d_rec, api.SELECT_RECORD_MISS, len(full))
    torch.cuda.synchronize()
    assert int(miss_count[0]) == N_MISS + N_DEAD
    wide = full.copy()
    wide["max_dist2"] = RTK_INF
    world.closest_points_device(api.to_device(wide), len(full), d_rec, d_inst, count=miss_count, ids=miss_ids, want_points=False)
    world.status()
    prim = d_rec.cpu().numpy().view(CLOSEST_RECORD_DTYPE)["prim"]
    assert (prim[:N_LIVE + N_MISS] != PRIM_NONE).all()
    world.free()


def test_update_equals_a_fresh_world(api, scenes):
    which, places, q, _ = reference("65")
    rng = np.random.RandomState(8)
    moved = places.copy()
    moved[::3] = world_ref.random_placements(len(moved[::3]), rng, 12.0)
    moved[which == 2] = places[which == 2]
    world = api.DeviceWorld.create(scenes, which, places)
    before = run(api, world, q)
    world.update(moved)
    fresh = api.DeviceWorld.create(scenes, which, moved)
    a, b = run(api, world, q), run(api, fresh, q)
    assert all((x == y).all() for x, y in zip(a, b)) and (a[0] != before[0]).any()
    same(a, R.brute_force(TRIS, which, moved, q["point"], q["max_dist2"], prune=True))
    # a scene's refit, then update(None): as a fresh world over the refitted scene
    own = api.DeviceScene.build([dict(positions=TRIS[1].reshape(-1, 3))])
    grown = (TRIS[1] * F(1.5)).astype(F)
    w2 = api.DeviceWorld.create([scenes[0], own, scenes[2]], which, moved)
    own.refit([dict(positions=grown.reshape(-1, 3))])
    w2.update(None)
    f2 = api.DeviceWorld.create([scenes[0], own, scenes[2]], which, moved)
    c, d = run(api, w2, q), run(api, f2, q)
    assert all((x == y).all() for x, y in zip(c, d)) and (c[0] != a[0]).any()
    same(c, R.brute_force([TRIS[0], grown, TRIS[2]], which, moved, q["point"], q["max_dist2"], prune=True))
    for w in (world, fresh, w2, f2):
        w.free()


def test_past_one_pass_of_the_grid(api, scenes):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    N, L = M.batch_size(cus), M.mix_length(cus)
    which, places, q, want = reference("65")
    # a prime-length mix: hits of both kinds, misses and dead queries in turn, so that consecutive steps of a lane differ
    pick = np.random.RandomState(9).permutation(len(q))[:L]
    hit = want[0][pick, 3] != PRIM_NONE
    assert 0.05 < (~hit).mean() < 0.5 and all(s % L for s in M.pass_sizes(cus))
    world = api.DeviceWorld.create(scenes, which, places)
    rec, inst, pts = run(api, world, M.tile_rows(q[pick], N), n=N)
    assert (rec[:N] == M.tile_rows(want[0][pick], N)).all() and (inst[:N] == M.tile_rows(want[1][pick], N)).all()
    assert (pts[:N] == M.tile_rows(want[2][pick], N)).all()
    world.free()


def test_the_spill_path(api, scenes):
    """2048 coincident triangles: a query on them has every bound equal to best2 = 0, and because the skip is strict nothing is
    skipped -- every node is entered, every sibling pushed. With the line scene's deep tree beside it."""
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F)
    coincident = np.ascontiguousarray(np.broadcast_to(tri, (2048, 3, 3)))
    pile = api.DeviceScene.build([dict(positions=coincident.reshape(-1, 3))])
    mine = [TRIS[0], coincident, TRIS[2]]
    which = np.array([1, 2, 0], np.uint32)
    places = np.array([placement(rotation([1, 2, 2], 0.8) * 1.5, (3, -1, 2)), placement(rotation([0, 0, 1], 0.3), (1, 2, 3)), placement(None, (-50, 0, 0))], F)
    world = api.DeviceWorld.create([scenes[0], pile, scenes[2]], which, places)
    on_chip = api.lib().rtk_amd_world_closest_stack_entries()
    assert world.info()["stack_entries"] > on_chip > 0
    rng = np.random.RandomState(47)
    w = rng.dirichlet((1, 1, 1), 96)
    on_pile = world_ref.place_np(places[0], (w @ tri.astype(np.float64)).astype(F))
    line = R.placed_tris(TRIS[2], places[1]).astype(np.float64)
    near_line = line[rng.randint(0, 2048, 96)].mean(1) + rng.uniform(-0.01, 0.01, (96, 3))
    pts = np.concatenate([on_pile, near_line, rng.uniform(-60, 110, (64, 3))]).astype(F)
    q = make_queries(pts, np.full(len(pts), RTK_INF, F))
    ref = R.brute_force(mine, which, places, pts, q["max_dist2"])
    assert (ref[1][:96] == 0).all() and (ref[0][:96, 3] == 0).all()          # 2048 ties: primitive 0
    same(run(api, world, q), ref)
    d_rec, d_inst, d_pts, ctr = world.closest_points_counted(api.to_device(q), len(q))
    print("spill: stack entries %d, on chip %d, counts %s" % (world.info()["stack_entries"], on_chip, ctr))
    assert ctr["stack_spills"] > 0 and ctr["rays"] == len(q) and ctr["hits"] == len(q)
    assert ctr["triangles"] >= 48 * 2048                                     # (a point inside the pile's box skips none of its 2048 records; most are)
    got = (d_rec.cpu().numpy().view(np.uint32).reshape(-1, 4), d_inst.cpu().numpy().view(np.uint32), d_pts.cpu().numpy().view(np.uint32).reshape(-1, 3))
    same(got, ref)
    world.status()                                                           # the launch-error word is clear
    world.free()


def test_housekeeping(api, scenes):
    which, places, q, want = reference("special")
    world = api.DeviceWorld.create(scenes, which, places)
    bytes_before = world.info()["total_device_bytes"]
    plain = run(api, world, q)
    d_rec, d_inst, d_pts, ctr = world.closest_points_counted(api.to_device(q), len(q))
    n = len(q)
    assert (d_rec.cpu().numpy().view(np.uint32).reshape(n, 4) == plain[0][:n]).all() and (d_inst.cpu().numpy().view(np.uint32) == plain[1][:n]).all()
    assert (d_pts.cpu().numpy().view(np.uint32).reshape(n, 3) == plain[2][:n]).all()
    same(plain, want)
    assert ctr["rays"] == n and ctr["hits"] == int((want[0][:, 3] != PRIM_NONE).sum()) == N_LIVE
    assert ctr["nodes"] >= N_LIVE and ctr["leaves"] >= 2 * N_LIVE and ctr["triangles"] >= 2 * N_LIVE       # (a top leaf and a scene leaf, a proxy and a record, at least)
    # the counted form with a filter
    ign = want[1].copy()
    _, d_inst, _, ctr2 = world.closest_points_counted(api.to_device(q), n, ignore_instance=ign)
    ref = R.brute_force(TRIS, which, places, q["point"], q["max_dist2"], ignore=ign)
    assert (d_inst.cpu().numpy().view(np.uint32) == ref[1]).all() and ctr2["hits"] == int((ref[0][:, 3] != PRIM_NONE).sum())
    assert api.lib().rtk_amd_world_closest_stack_entries() > 0
    assert world.info()["total_device_bytes"] == bytes_before
    # no queries: nothing to do
    assert api.lib().rtk_dev_world_closest_points(world.handle, None, 0, None, None, None, None, None, None) == 0
    world.free()
