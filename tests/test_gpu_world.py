"""Instanced worlds on the GPU (rtk_dev_world, rtk_world.hip): the world's answer against the per-instance answer -- every
instance's scene traced by DeviceScene.trace_device with the ray transformed in numpy by the rule (tests/world_ref.py), combined
by minimum t -- bit for bit on every ray; dead instances, filters and lists, update and rebuild, the flat placed twin, and the
housekeeping of stack, counters and memory."""
import os

import numpy as np
import pytest

from tests import world_ref
from tests.world_ref import F, PRIM_NONE, brute64, inverse_np, make_rays, placement, random_placements, ray_np, rotation, world_tris64

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRIS = [world_ref.cube(), world_ref.icosphere(2), world_ref.line_scene(2048)]
assert [len(t) for t in TRIS] == [12, 320, 2048]


@pytest.fixture(scope="module")
def scenes(api):
    return [api.DeviceScene.build([dict(positions=t.reshape(-1, 3))]) for t in TRIS]


def rays_rows(rays):
    return np.ascontiguousarray(rays).view(F).reshape(-1, 8)


def per_instance(api, scenes, which, places, rays, skip=()):
    """The reference: (records, instances, blocked) combined over the live instances that are not in `skip`, by minimum t (the
    first instance among bit-equal t), and per ray how many instances attain the minimum."""
    import torch
    rows = rays_rows(rays)
    n = len(rows)
    inv, live = inverse_np(places)
    best = np.zeros(n, api.HIT_RECORD_DTYPE)
    best["t"], best["prim"] = rows[:, 7], PRIM_NONE
    inst = np.full(n, PRIM_NONE, np.uint32)
    ties = np.zeros(n, np.int64)
    blocked = np.zeros(n, bool)
    for k in range(len(which)):
        if not live[k] or k in skip:
            continue
        d = api.to_device(ray_np(inv[k], rows))
        rec = scenes[which[k]].trace_device(d, n).cpu().numpy().view(api.HIT_RECORD_DTYPE)
        occ = scenes[which[k]].trace_any_device(d, n).cpu().numpy().astype(bool)
        torch.cuda.synchronize()
        hit = rec["prim"] != PRIM_NONE
        assert (occ == hit).all()
        blocked |= hit
        closer = hit & (rec["t"] < best["t"])
        ties = np.where(closer, 1, ties + (hit & (rec["t"] == best["t"]) & (best["prim"] != PRIM_NONE)))
        best[closer] = rec[closer]
        inst[closer] = k
    return best, inst, blocked, ties


def same_records(api, got, got_inst, want, want_inst, allow=None):
    """bit for bit in t, u, v, prim and the instance; rows of `allow` may name another instance with the same bits of t"""
    g, w = got.view(np.uint32).reshape(-1, 4), want.view(np.uint32).reshape(-1, 4)
    bad = (g != w).any(1) | (got_inst != want_inst)
    if allow is not None:
        bad &= ~(allow & (g[:, 0] == w[:, 0]) & (got["prim"] != PRIM_NONE))
    assert not bad.any(), (np.flatnonzero(bad)[:8], got[bad][:4], got_inst[bad][:4], want[bad][:4], want_inst[bad][:4])


def placed_of(which, places):
    _, live = inverse_np(places)
    return [world_tris64(TRIS[which[k]], places[k]) for k in range(len(which)) if live[k]]


def case(name):
    """(which, placements): the shapes the issue names"""
    rng = np.random.RandomState({"one": 1, "two": 2, "65": 65, "257": 257, "special": 7}[name])
    if name == "one":
        return np.array([1], np.uint32), random_placements(1, rng, 5.0)
    if name == "two":
        return np.array([1, 1], np.uint32), random_placements(2, rng, 3.0)
    if name in ("65", "257"):
        n = int(name)
        which = (np.arange(n) % 2).astype(np.uint32)
        which[::64] = 2                                                      # a few deep scenes among cubes and spheres
        places = random_placements(n, rng, 12.0 if n == 65 else 20.0)
        for k in np.flatnonzero(which == 2):                                 # the line scene is 100 long: shrink it to the others' spread
            places[k] = placement(rotation(rng.standard_normal(3), rng.uniform(0, 6)) * 0.1, rng.uniform(-10, 10, 3))
        return which, places
    # one mirrored, one non-uniformly scaled (condition number 8), a plain one, and a deep one
    places = np.array([placement(np.diag([-1.0, 1.0, 1.0]) @ rotation([1, 1, 0], 0.5), (-4, 0, 0)),
                       placement(rotation([0, 1, 1], 1.0) @ np.diag([0.5, 1.0, 4.0]), (4, 1, 0)),
                       placement(rotation([1, 0, 0], 0.3), (0, 5, 1)),
                       placement(rotation([0, 0, 1], 0.2) * 0.05, (0, -5, 0))], F)
    return np.array([1, 0, 1, 2], np.uint32), places


_RAYS = {}


def rays_of(name, which, places):
    if name not in _RAYS:
        _RAYS[name] = make_rays(placed_of(which, places), np.random.RandomState(11))
    return _RAYS[name]


@pytest.mark.parametrize("name", ["one", "two", "65", "257", "special"])
def test_world_equals_the_per_instance_answer_bit_for_bit(api, scenes, name):
    which, places = case(name)
    rays = rays_of(name, which, places)
    assert len(rays) == 4096 + 512
    world = api.DeviceWorld.create(scenes, which, places)
    info = world.info()
    assert info["num_instances"] == len(which) and info["num_scenes"] == 3 and info["dead_instances"] == 0
    want, want_inst, blocked, ties = per_instance(api, scenes, which, places, rays)
    # no two candidates of different instances within 1e-6 relative, by float64 brute force: so no ray ties across instances
    bt, bi, _ = brute64(placed_of(which, places), rays)
    near = np.isfinite(bt[:, 1]) & (bi[:, 0] != bi[:, 1]) & (bt[:, 1] - bt[:, 0] <= 1e-6 * bt[:, 1])
    assert near.sum() == 0 and (ties <= 1).all()
    got, got_inst = world.trace(rays)
    same_records(api, got, got_inst, want, want_inst)
    assert (got["prim"][:4096] != PRIM_NONE).all() and (got["prim"][4096:] == PRIM_NONE).all() and (got_inst[4096:] == PRIM_NONE).all()
    assert (got["t"][4096:] == rays["max_t"][4096:]).all()
    assert (world.trace_any(rays) == blocked).all()
    if name in ("65", "257"):
        assert info["top_max_depth"] >= 3 and info["top_nodes"] > (64 if name == "257" else 16) // 3
    # rebuild changes no answer
    world.rebuild()
    again, again_inst = world.trace(rays)
    same_records(api, again, again_inst, want, want_inst)
    world.free()


def test_an_instance_duplicated_exactly_ties_and_either_is_accepted(api, scenes):
    which, places = case("special")
    which, places = np.concatenate([which, which[:1]]), np.concatenate([places, places[:1]])
    rays = rays_of("special", *case("special"))
    world = api.DeviceWorld.create(scenes, which, places)
    want, want_inst, _, ties = per_instance(api, scenes, which, places, rays)
    got, got_inst = world.trace(rays)
    twin = np.isin(want_inst, [0, 4])
    assert (ties[twin] == 2).all() and twin.sum() > 500
    same_records(api, got, got_inst, want, np.where(twin, got_inst, want_inst))
    assert np.isin(got_inst[twin], [0, 4]).all()
    world.free()


def test_dead_instances_are_never_hit_and_change_nothing(api, scenes):
    which, places = case("special")
    rays = rays_of("special", which, places)
    empty = api.DeviceScene.build([dict(positions=np.zeros((0, 3), F))])
    singular = placement(np.array([[1, 2, 3], [1, 2, 3], [0, 0, 1]]), (0, 0, 0))
    nan = placement(None, (np.nan, 0, 0))
    which2 = np.concatenate([which, [1, 3, 0]]).astype(np.uint32)           # a singular sphere, a placed empty scene, a NaN cube
    places2 = np.concatenate([places, [singular, placement(None, (0, 0, 0)), nan]])
    world = api.DeviceWorld.create(scenes + [empty], which2, places2)
    assert world.info()["dead_instances"] == 3 and world.info()["num_scenes"] == 4
    want, want_inst, blocked, _ = per_instance(api, scenes, which, places, rays)
    got, got_inst = world.trace(rays)
    same_records(api, got, got_inst, want, want_inst)
    assert (world.trace_any(rays) == blocked).all()
    world.free()


def test_filters_and_lists(api, scenes):
    import torch
    which, places = case("65")
    rays = rays_of("65", which, places)
    n = len(rays)
    world = api.DeviceWorld.create(scenes, which, places)
    full, full_inst, _, _ = per_instance(api, scenes, which, places, rays)
    # the instance mask: the odd instances and those beyond bit 60 are out
    mask = np.zeros(60, bool)
    mask[::2] = True
    out = [k for k in range(65) if k >= 60 or not mask[k]]
    want, want_inst, blocked, _ = per_instance(api, scenes, which, places, rays, skip=set(out))
    got, got_inst = world.trace(rays, instance_mask=mask)
    same_records(api, got, got_inst, want, want_inst)
    assert (world.trace_any(rays, instance_mask=mask) == blocked).all()
    # per ray the instance it hit first is ignored: the answer is the per-instance one without it (two groups: by the instance's parity)
    ign = full_inst.copy()
    got, got_inst = world.trace(rays, ignore_instance=ign)
    assert (got_inst != ign)[ign != PRIM_NONE].all()
    for k in np.unique(ign[ign != PRIM_NONE])[:6]:
        rows = np.flatnonzero(ign == k)
        w, wi, wb, _ = per_instance(api, scenes, which, places, rays[rows], skip={int(k)})
        same_records(api, got[rows], got_inst[rows], w, wi)
    # a listed call touches only the listed slots
    ids = torch.from_numpy(np.random.RandomState(5).permutation(n)[:1000].astype(np.int64)).cuda()
    count = torch.tensor([700], dtype=torch.int64, device="cuda")
    d_rec = torch.full((n * 16,), 0xAB, dtype=torch.uint8, device="cuda")
    d_inst = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    d_blk = torch.full((n,), 0xCD, dtype=torch.uint8, device="cuda")
    d_rays = api.to_device(rays)
    world.trace_device(d_rays, n, d_rec, d_inst, count=count, ids=ids)
    world.trace_any_device(d_rays, n, d_blk, count=count, ids=ids)
    world.status()
    listed = np.zeros(n, bool)
    listed[ids.cpu().numpy()[:700]] = True
    rec, inst, blk = d_rec.cpu().numpy().view(api.HIT_RECORD_DTYPE), d_inst.cpu().numpy().view(np.uint32), d_blk.cpu().numpy()
    same_records(api, rec[listed], inst[listed], full[listed], full_inst[listed])
    assert (rec[~listed].view(np.uint8) == 0xAB).all() and (inst[~listed] == 0x5A5A5A5A).all() and (blk[~listed] == 0xCD).all()
    assert (blk[listed] == (full["prim"][listed] != PRIM_NONE)).all()
    world.free()


def test_update_equals_a_fresh_world(api, scenes):
    which, places = case("65")
    rng = np.random.RandomState(8)
    moved = places.copy()
    moved[::3] = random_placements(len(moved[::3]), rng, 12.0)
    moved[which == 2] = places[which == 2]
    rays = make_rays(placed_of(which, moved), np.random.RandomState(12), 2048, 256)
    world = api.DeviceWorld.create(scenes, which, places)
    world.update(moved)
    fresh = api.DeviceWorld.create(scenes, which, moved)
    a, ai = world.trace(rays)
    b, bi = fresh.trace(rays)
    same_records(api, a, ai, b, bi)
    assert world.info()["update_ms"] > 0
    # a scene's refit, then update(None): as a fresh world over the refitted scene
    own = api.DeviceScene.build([dict(positions=TRIS[1].reshape(-1, 3))])
    grown = (TRIS[1] * F(1.5)).astype(F)
    w2 = api.DeviceWorld.create([scenes[0], own, scenes[2]], which, moved)
    own.refit([dict(positions=grown.reshape(-1, 3))])
    w2.update(None)
    f2 = api.DeviceWorld.create([scenes[0], own, scenes[2]], which, moved)
    a, ai = w2.trace(rays)
    b, bi = f2.trace(rays)
    same_records(api, a, ai, b, bi)
    assert (a.view(np.uint32) != world.trace(rays)[0].view(np.uint32)).any()          # (the refit did change answers)
    # a placement that turns singular kills its instance; the same placements given on the device
    import torch
    moved[5] = 0
    world.update(torch.from_numpy(moved).cuda())
    assert world.info()["dead_instances"] == 1
    want, want_inst, _, _ = per_instance(api, scenes, which, moved, rays)
    a, ai = world.trace(rays)
    same_records(api, a, ai, want, want_inst)
    for w in (world, fresh, w2, f2):
        w.free()


def test_against_the_flat_placed_twin(api, scenes):
    """Hit / miss and (instance, prim) <-> flat prim on every ray whose two nearest candidates are not within 1e-5 relative in float64
    (at most 1 % are); the world's worst relative error of t against float64 is at most 4 x the twin's on the same rays.
    Measured on MI355X: see profiles/world_accuracy.log."""
    which, places = case("65")
    rays = rays_of("65", which, places)
    placed = placed_of(which, places)
    bt, bi, bp = brute64(placed, rays)
    close = np.isfinite(bt[:, 1]) & (bt[:, 1] - bt[:, 0] <= 1e-5 * bt[:, 1])
    assert close.mean() <= 0.01
    keep = ~close
    twin = api.DeviceScene.build([dict(positions=TRIS[s].reshape(-1, 3)) for s in which], placements=places)
    base = twin.mesh_base()
    world = api.DeviceWorld.create(scenes, which, places)
    got, got_inst = world.trace(rays)
    flat = twin.trace_device(api.to_device(rays), len(rays)).cpu().numpy().view(api.HIT_RECORD_DTYPE)
    hit = bi[:, 0] >= 0
    assert ((got["prim"] != PRIM_NONE) == hit)[keep].all() and ((flat["prim"] != PRIM_NONE) == hit)[keep].all()
    rows = keep & hit
    assert (got_inst[rows] == bi[rows, 0]).all() and (got["prim"][rows] == bp[rows, 0]).all()
    assert (flat["prim"][rows] == base[got_inst[rows]] + got["prim"][rows]).all()
    err_world = (np.abs(got["t"][rows].astype(np.float64) - bt[rows, 0]) / bt[rows, 0]).max()
    err_twin = (np.abs(flat["t"][rows].astype(np.float64) - bt[rows, 0]) / bt[rows, 0]).max()
    text = "t against numpy float64 brute force, 65 instances, %d rays (%d left out as near-ties): world worst %.3e, flat placed twin worst %.3e, ratio %.2f\n" % (
        rows.sum(), close.sum(), err_world, err_twin, err_world / err_twin)
    print(text)
    try:
        with open(os.path.join(ROOT, "profiles", "world_accuracy.log"), "w") as f:
            f.write(text)
    except OSError:
        pass
    assert err_world <= 4 * err_twin, text
    world.free()


def test_housekeeping_stack_counters_and_memory(api, scenes):
    """One deep instance, rays along its line: more than 16 entries are needed, the spill area takes them, the error word stays
    clear; the counted form agrees with the plain one; total_device_bytes is the two ledgers' sum."""
    which = np.array([2, 0], np.uint32)
    places = np.array([placement(rotation([0, 0, 1], 0.3), (1, 2, 3)), placement(None, (-500, 0, 0))], F)
    world = api.DeviceWorld.create(scenes, which, places)
    info = world.info()
    deep = scenes[2].info()
    assert info["stack_entries"] == world.top_scene_info()["stack_entries"] + 1 + deep["stack_entries"] > api.lib().rtk_amd_world_stack_entries()
    # from beyond the thin end of the line towards its inside points and along it
    m = places[0].astype(np.float64).reshape(3, 4)
    rng = np.random.RandomState(21)
    rays = np.zeros(512, world_ref.RAY_DTYPE)
    o_obj = np.array([-5.0, 0, 0]) + rng.uniform(-0.05, 0.05, (512, 3))
    p_obj = np.array([110.0, 0, 0]) + rng.uniform(-0.05, 0.05, (512, 3))
    rays["origin"] = o_obj @ m[:, :3].T + m[:, 3]
    d = (p_obj - o_obj) @ m[:, :3].T
    rays["direction"] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays["max_t"] = world_ref.RTK_INF
    want, want_inst, blocked, _ = per_instance(api, scenes, which, places, rays)
    got, got_inst, ctr = world.trace_counted(rays)
    same_records(api, got, got_inst, want, want_inst)
    assert (got_inst == 0).all() and ctr["rays"] == 512 and ctr["hits"] == 512 and ctr["stack_spills"] > 0
    assert ctr["nodes"] > 512 and ctr["leaves"] >= 1024 and ctr["triangles"] >= 1024
    plain, plain_inst = world.trace(rays)
    same_records(api, plain, plain_inst, want, want_inst)
    world.status()                                                           # the launch-error word is clear
    assert (world.trace_any(rays) == blocked).all()
    n, s = len(which), len(scenes)
    assert info["total_device_bytes"] == world.top_scene_info()["total_device_bytes"] + n * (64 + 48 + 36) + s * 24 + 8
    world.free()
