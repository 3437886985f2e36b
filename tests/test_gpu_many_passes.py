"""Every resident-grid query kernel past one pass of its grid. A batch of N = many_passes.batch_size(CUs) slots -- two passes of
the largest grid a CU count allows, five waves and 37 -- makes every lane take a second and a third step, so the state a step
must start clean with (the stack pointer, best_t, kept, room, worst, the claim bit), the spill slots a lane's steps share and
the per-slot arrays indexed by ids[i] are all exercised. The batch is a mix of L = 997 queries repeated to N rows and the
reference is that mix's brute force repeated (tests/many_passes.py; tests/test_many_passes_cpu.py proves the tiling and that
consecutive steps of a lane differ in their answers). Everything is compared bit for bit; outputs are pre-filled with 0x7e and
carry an untouched tail; rtk_dev_trace_status is 0 after every call (the families' own run helpers assert both).

The grid a launch used cannot be read back: the counted forms report visits, not blocks, and the scene's info has no CU count.
N does not depend on it.

All hits has no counted form: its spilling case asserts the need for the spill area from the scene's info."""
import importlib

import numpy as np
import pytest

from tests import many_passes as M
from tests.many_passes import NONE

pytestmark = pytest.mark.gpu
TAIL = 5
# The largest |default form - exact form| of the winding numbers on the 997 points of many_passes.winding_mix, as measured once
# on an MI355X (profiles/many_passes_timing.log); 2 x it is asserted, as tests/test_gpu_winding.py does with MEASURED_FAST.
MEASURED_DEFAULT = 8.413e-03


@pytest.fixture(scope="module")
def dev(api):
    import torch

    class Dev:
        pass
    d = Dev()
    d.cus = torch.cuda.get_device_properties(0).multi_processor_count
    d.N = M.batch_size(d.cus)
    d.ds = api.DeviceScene.build([dict(positions=M.soup())])
    info = d.ds.info()
    assert "num_cus" not in info or info["num_cus"] == d.cus
    assert d.N > 2 * max(M.pass_sizes(d.cus)) and d.N % 64
    print("%d CUs: N = %d, passes of %s lanes" % (d.cus, d.N, M.pass_sizes(d.cus)))
    return d


def same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.nonzero((got != want).reshape(len(got), -1).any(1))[0]
        raise AssertionError("%s: %d of %d rows differ, first %s: got %s want %s" % (what, len(bad), len(got), bad[:5], got[bad[:3]], want[bad[:3]]))


def module_of(name):
    return importlib.import_module(M.SWEEPS[name][0] if name in M.SWEEPS else "tests.test_gpu_" + name)


def keywords(name, inputs):
    return dict(max2=inputs[1]) if name in ("pair", "near") else {}


def fill_forms(name):
    """(run_count, run_fill, assert_fill) of a family's file (the touch file takes its fill helpers from the box file)"""
    m = module_of(name)
    return m.run_count, m.run_fill, getattr(m, "assert_fill", None) or module_of("box").assert_fill


def run_slots(api, ds, name, inputs, **kw):
    """the per-slot outputs of a closest form as words, in the order of the family's Answer.rows"""
    m = module_of(name)
    if name == "sign":
        sg, rec, pts = m.run(api, ds, inputs[0], **kw)
        return rec, pts, sg
    return tuple(m.run(api, ds, inputs[0], **dict(keywords(name, inputs), **kw)))


def check_slots(api, ds, name, inputs, rows, n, listed=None, **kw):
    got = run_slots(api, ds, name, inputs, **kw)
    for j, (g, w) in enumerate(zip(got, rows)):
        same(g, M.slots(w, n, TAIL, listed), "%s, output %d" % (name, j))
    return len(got) * n


def check_count_then_fill(api, ds, name, inputs, answer, n, **kw):
    """the count form, then the fill form at the exact offsets of that count, against the tiled lists -> rows checked"""
    run_count, run_fill, assert_fill = fill_forms(name)
    t = M.Tiled(answer.counts, n)
    kw = dict(keywords(name, inputs), **kw)
    same(run_count(api, ds, inputs[0], **kw), t.written(TAIL), name + ", counts")
    got = run_fill(api, ds, inputs[0], t.offsets, t.total, **kw)
    assert_fill(got, tuple(t.fill(p, TAIL) for p in answer.fills) + (t.written(TAIL),), name + ", exact offsets")
    return 2 * n + t.total


# ---------------------------------------------------------------- 1. every family, plain forms at N

@pytest.mark.parametrize("name", M.FAMILIES)
def test_plain_forms(api, dev, name):
    f = M.family(name, dev.cus)
    M.conditions(name, f.answer.live, f.answer.key, dev.cus)
    inputs = tuple(M.tile_rows(x, dev.N) for x in f.inputs)
    if name in M.COUNTED:
        rows = check_count_then_fill(api, dev.ds, name, inputs, f.answer, dev.N)
    else:
        rows = check_slots(api, dev.ds, name, inputs, f.answer.rows, dev.N)
        if name in M.SWEEPS:
            flags = module_of(name).run(api, dev.ds, inputs[0], any_hit=True)
            same(flags, M.slots(f.answer.key.astype(np.uint8), dev.N, TAIL), name + ", any hit")
            rows += dev.N
    print("%s: %d slots, %d rows checked" % (name, dev.N, rows))


def check_all_hits(api, ds, rays, counts, kept, period, n, what):
    """rtk_dev_trace_rays_count against counts [L], then rtk_dev_trace_rays_all with room for kept [L] records per slot against
    period (the concatenated first kept[i] records of every list of the mix) -> rows checked"""
    import torch
    from tests.test_gpu_allhits import fill, status_ok
    batch = M.tile_rows(rays, n)
    d_counts = torch.full(((n + TAIL) * 4,), 0x7e, dtype=torch.uint8, device="cuda")
    ds.count_hits_device(api.to_device(batch), n, d_counts)
    assert status_ok(api, ds), api.last_error()
    same(d_counts.cpu().numpy().view(np.uint32), M.Tiled(counts, n).written(TAIL), what + ", counts")
    t = M.Tiled(kept, n)
    rec, wr = fill(api, ds, batch, t.offsets)                        # (0x7e-filled, and the guard band is checked there)
    same(rec.view(np.uint32).reshape(-1, 4), t.fill(period.view(np.uint32).reshape(-1, 4)), what + ", records")
    same(wr, t.counts.astype(np.uint32), what + ", written")
    return 2 * n + t.total


def test_all_hits(api, oracle, dev):
    """rtk_dev_trace_rays_count, then rtk_dev_trace_rays_all at the exact offsets, against the oracle's lists of the mix on the
    blob this scene exports"""
    rays, want = M.allhits_mix(oracle, oracle.Blob(dev.ds.export_blob()), dev.ds.mesh_base(), dev.cus)
    M.conditions("all hits", np.ones(len(rays), bool), want.counts, dev.cus)
    assert want.counts.max() >= 2
    rows = check_all_hits(api, dev.ds, rays, want.counts, want.counts, want.records, dev.N, "all hits")
    print("all hits: %d slots, %d rows checked" % (dev.N, rows))


def test_spill_all_hits(api, oracle, dev):
    """The stack of 4-byte entries without keys. The deep scene of tests/test_gpu_allhits.py (large sheets on the centroids of
    the geometric chain, a ray along x = y = 0.3 enters every box): every seventh ray of a mix of 163 runs along that line and
    has a thousand candidates, the others start at the same places and point away. The count form at N, then the fill form
    with room for the 5 closest per slot (exact offsets would be 150 million records). All hits has no counted form, so
    stack_spills cannot be read: that the walk needs the spill area is asserted from the scene's info, as that file does, and
    the counts say that no push was dropped."""
    from tests import allhits_ref as R
    on_chip = api.lib().rtk_amd_allhits_stack_entries()
    k = np.arange(1200)
    cc = np.stack([0.5 ** (k % 40 + 1) * (1 + (k // 40) * 1e-3), 0.5 ** ((k * 7) % 40 + 1), 0.5 ** ((k * 13) % 40 + 1) * (1 + (k // 40) * 1e-3)], 1).astype(np.float32)
    big = np.float32(2.0)
    tris = np.stack([cc + big * np.float32([-1, -1, 0]), cc + big * np.float32([1, -1, 0]), cc + big * np.float32([0, 2, 0])], 1).astype(np.float32)
    ds = api.DeviceScene.build([dict(positions=tris.reshape(-1, 3))])
    assert ds.info()["stack_entries"] > on_chip, (ds.info(), on_chip)
    L = M.mix_length(dev.cus, 500000 // len(tris) // 2)
    assert all(s % L for s in M.pass_sizes(dev.cus))
    rng = np.random.RandomState(8)
    o = np.concatenate([rng.uniform(0.25, 0.35, (24, 2)), np.full((24, 1), -1.0)], 1).astype(np.float32)
    along = R.make_rays(o, (0, 0, 1))
    along["direction"][12:] = (0.01, -0.02, 1)
    away = along[:16].copy()
    away["direction"] *= -1
    rays = M.deep_mix(along, away, L)
    want = R.oracle_lists(oracle, oracle.Blob(ds.export_blob()), rays, ds.mesh_base())
    assert (want.counts[::7] >= 1000).all() and not np.delete(want.counts, np.arange(0, L, 7)).any()
    kept = np.minimum(want.counts, 5)
    period = np.concatenate([want.records[want.offsets[i]:want.offsets[i] + kept[i]] for i in range(L)])
    rows = check_all_hits(api, ds, rays, want.counts, kept, period, dev.N, "all hits on the deep sheets")
    print("all hits on the deep sheets: stack entries %d, on chip %d, L %d, %d rows checked" % (ds.info()["stack_entries"], on_chip, L, rows))


def world_outputs(api, world, rays, n):
    """trace and trace_any of a world into 0x7e-filled buffers with a tail -> (record words, instance words, blocked bytes)"""
    import torch
    d_rays = api.to_device(rays)
    d_rec = torch.full(((n + TAIL) * 16,), 0x7e, dtype=torch.uint8, device="cuda")
    d_inst = torch.full(((n + TAIL) * 4,), 0x7e, dtype=torch.uint8, device="cuda")
    d_any = torch.full((n + TAIL,), 0x7e, dtype=torch.uint8, device="cuda")
    world.trace_device(d_rays, n, d_rec, d_inst)
    world.trace_any_device(d_rays, n, d_any)
    world.status()
    return d_rec.cpu().numpy().view(np.uint32).reshape(-1, 4), d_inst.cpu().numpy().view(np.uint32), d_any.cpu().numpy()


def check_world(api, world, scenes, which, places, rays, n, what):
    from tests.test_gpu_world import per_instance
    want, want_inst, blocked, ties = per_instance(api, scenes, which, places, rays)
    assert (ties <= 1).all()                                         # (no ray ties across instances: the answer is one record)
    rec, inst, flags = world_outputs(api, world, M.tile_rows(rays, n), n)
    same(rec, M.slots(want.view(np.uint32).reshape(-1, 4), n, TAIL), what + ", records")
    same(inst, M.slots(want_inst, n, TAIL), what + ", instances")
    same(flags, M.slots(blocked.astype(np.uint8), n, TAIL), what + ", any hit")
    return blocked


def test_worlds(api, dev):
    """The four instances of tests/test_gpu_world.py's "special" case (one mirrored, one scaled unevenly, one plain, one deep):
    trace and trace_any against that file's per-instance answer of the mix. Then its world of one deep instance, where every
    seventh ray runs along the line and spills, and the others point away from it."""
    from tests import test_gpu_world as W
    from tests import world_ref
    scenes = [api.DeviceScene.build([dict(positions=t.reshape(-1, 3))]) for t in W.TRIS]
    L = M.mix_length(dev.cus)
    which, places = W.case("special")
    rays = W.rays_of("special", which, places)
    _, _, hit, _ = W.per_instance(api, scenes, which, places, rays)
    rays = rays[M.cut(hit.astype(np.int64), L, dev.cus)]
    world = api.DeviceWorld.create(scenes, which, places)
    blocked = check_world(api, world, scenes, which, places, rays, dev.N, "world of four")
    M.conditions("world", np.ones(L, bool), blocked.astype(np.int64), dev.cus)
    world.free()
    # one deep instance and a cube far away (the housekeeping case of that file)
    which = np.array([2, 0], np.uint32)
    places = np.array([W.placement(W.rotation([0, 0, 1], 0.3), (1, 2, 3)), W.placement(None, (-500, 0, 0))], W.F)
    world = api.DeviceWorld.create(scenes, which, places)
    assert world.info()["stack_entries"] > api.lib().rtk_amd_world_stack_entries() == 16
    m = places[0].astype(np.float64).reshape(3, 4)
    rng = np.random.RandomState(21)
    o_obj = np.array([-5.0, 0, 0]) + rng.uniform(-0.05, 0.05, (64, 3))
    d = (np.array([110.0, 0, 0]) + rng.uniform(-0.05, 0.05, (64, 3)) - o_obj) @ m[:, :3].T
    along = np.zeros(64, world_ref.RAY_DTYPE)
    along["origin"], along["direction"], along["max_t"] = o_obj @ m[:, :3].T + m[:, 3], d / np.linalg.norm(d, axis=1, keepdims=True), world_ref.RTK_INF
    away = along[:16].copy()
    away["direction"] *= -1
    rays = M.deep_mix(along, away, L)
    blocked = check_world(api, world, scenes, which, places, rays, dev.N, "world with a deep instance")
    assert blocked[::7].all() and not np.delete(blocked, np.arange(0, L, 7)).any()
    _, _, ctr = world.trace_counted(M.tile_rows(rays, dev.N))
    print("world with a deep instance: %s" % (ctr,))
    assert ctr["stack_spills"] > 0 and ctr["rays"] == dev.N and ctr["hits"] == int(M.tile_rows(blocked, dev.N).sum())
    world.free()


def test_winding_numbers(api, dev):
    """The exact form and the default form (beta 2), by the rule of tests/test_gpu_winding.py on every row. A winding number is
    a sum in the order of the tree, so the bar is a tolerance. The exact form against float64 of the mix: the file's 4 x the
    error of the sum in float32, which for a scene without a measured figure is max |brute32 - brute64| (as
    tests/test_gpu_queries_hostile_scenes.py takes it), never more than the file's ceiling. The default form against the exact
    form: 2 x the largest difference measured once on an MI355X (MEASURED_DEFAULT, profiles/many_passes_timing.log), in the
    style of that file's MEASURED_FAST; and the side of 0.5 of float64 wherever float64 is further from 0.5 than that bound.
    rtk_amd/csrc/rtk_winding_rule.h promises "the same scene object gives the same bits on every call", so in both forms every
    copy of a query has the bits of its first copy."""
    from tests import test_gpu_winding as m
    pts, w64, rule = M.winding_mix(dev.cus)
    L = len(pts)
    assert rule <= m.CEILING
    batch, first = M.tile_rows(pts, dev.N), np.arange(dev.N) % L
    exact = m.run(api, dev.ds, batch, exact=True)[:dev.N]
    err = float(np.abs(exact.view(np.float32).astype(np.float64) - w64[first]).max())
    print("winding numbers, exact form: worst %.3e on %d rows (brute32 %.3e)" % (err, dev.N, rule))
    assert err <= min(4 * rule, m.CEILING)
    same(exact, exact[first], "winding numbers, exact form: a copy against the first copy")
    fast = m.run(api, dev.ds, batch)[:dev.N]
    diff = np.abs(fast.view(np.float32).astype(np.float64) - exact.view(np.float32).astype(np.float64))
    far = np.abs(fast.view(np.float32).astype(np.float64) - w64[first])
    print("winding numbers, default form: worst |default - exact| %.3e, worst |default - float64| %.3e on %d rows; %d of %d points take a far term"
          % (diff.max(), far.max(), dev.N, (diff[:L] > 0).sum(), L))
    bound = 2 * MEASURED_DEFAULT
    assert diff.max() <= bound, (float(diff.max()), bound)
    assert (diff[:L] > 0).sum() >= L // 4                            # (the far terms are really used: it is not the exact form again)
    decided = np.abs(w64[first] - 0.5) > bound + 4 * rule
    assert decided.mean() > 0.5 and ((fast.view(np.float32)[decided] > 0.5) == (w64[first][decided] > 0.5)).all()
    same(fast, fast[first], "winding numbers, default form: a copy against the first copy")


# ---------------------------------------------------------------- 2. lists at N

def a_list(n, seed):
    """ids: a permutation of the n slots; the count on the device: 0.6 n -- past one pass at every residency, past two at the
    four or five workgroups per CU that 32 KB of LDS stack allow"""
    ids = np.random.RandomState(seed).permutation(n).astype(np.int64)
    count = int(0.6 * n)
    listed = np.zeros(n, bool)
    listed[ids[:count]] = True
    return ids, count, listed


@pytest.mark.parametrize("name", ["closest", "sphere"])
def test_lists(api, dev, name):
    f = M.family(name, dev.cus)
    inputs = tuple(M.tile_rows(x, dev.N) for x in f.inputs)
    ids, count, listed = a_list(dev.N, 3)
    assert count > max(M.pass_sizes(dev.cus)) and count > 2 * M.pass_sizes(dev.cus)[3] and 0 < listed.sum() == count
    check_slots(api, dev.ds, name, inputs, f.answer.rows, dev.N, listed, count=count, ids=ids)
    if name in M.SWEEPS:
        flags = module_of(name).run(api, dev.ds, inputs[0], any_hit=True, count=count, ids=ids)
        same(flags, M.slots(f.answer.key.astype(np.uint8), dev.N, TAIL, listed), name + ", any hit, listed")


def test_lists_fill_form_with_repeated_ids(api, dev):
    """within: the count form and the fill form under a list in which 1000 ids stand twice, the second time spread over all of
    the listed part: every segment holds its brute-force list once, and the claim bitmap is clean in all of its N / 32 words"""
    f = M.family("within", dev.cus)
    q = M.tile_rows(f.inputs[0], dev.N)
    ids, count, _ = a_list(dev.N, 4)
    at = np.linspace(0, count - 1, 1000).astype(np.int64)            # where an id is repeated ...
    ids[at] = ids[(at + count // 2 + 7) % count]                      # ... that also stands half a list away
    listed = np.zeros(dev.N, bool)
    listed[ids[:count]] = True
    assert count - 1000 <= listed.sum() < count and len(np.unique(ids[at] >> 5)) > 900
    t = M.Tiled(f.answer.counts, dev.N)
    assert (t.counts[ids[at]] > 0).sum() > 300                        # (repeated ids with something to write)
    run_count, run_fill, assert_fill = fill_forms("within")
    same(run_count(api, dev.ds, q, count=count, ids=ids), t.written(TAIL, listed), "within, counts, listed")
    got = run_fill(api, dev.ds, q, t.offsets, t.total, count=count, ids=ids)
    assert_fill(got, tuple(t.fill(p, TAIL, listed) for p in f.answer.fills) + (t.written(TAIL, listed),), "within, listed")


# ---------------------------------------------------------------- 3. a per-slot filter at N

def test_ignore_prim_per_slot(api, dev):
    """Sphere sweeps: the odd copies of the mix ignore the triangle they would hit, the even copies are given NONE. The filter
    array is read at the query's slot r, not at the lane."""
    import torch
    from tests.sweep_ref import brute_force
    f = M.family("sphere", dev.cus)
    prims = np.arange(len(f.tris), dtype=np.uint32)
    first = f.answer.rows[0][:, 3].copy()
    ignored = brute_force(f.tris, prims, f.inputs[0], filter=dict(ignore_prim=first))
    hit = first != NONE
    assert (ignored[0][hit, 3] != first[hit]).all() and (ignored[0][hit, 3] != NONE).sum() > 100
    odd = (np.arange(dev.N) // f.L) % 2 == 1
    ignore = np.where(odd, M.tile_rows(first, dev.N), np.uint32(NONE)).astype(np.uint32)
    s = M.tile_rows(f.inputs[0], dev.N)
    got = module_of("sphere").run(api, dev.ds, s, ignore_prim=torch.from_numpy(ignore.view(np.int32)).cuda())
    for j, g in enumerate(got):
        want = np.where(odd[:, None], M.tile_rows(ignored[j], dev.N), M.tile_rows(f.answer.rows[j], dev.N))
        same(g[:dev.N], want, "sphere sweep, ignore_prim per slot, output %d" % j)


# ---------------------------------------------------------------- 4. spill in a later pass, 5. scratch that grows and is reused

@pytest.fixture(scope="module")
def deep(api, dev):
    """The geometric cluster of tests/test_gpu_build.py, the scene the families spill on. Every seventh query of a mix of 163
    goes down the chain, the others are dead or end at the root."""
    from rtk_amd.types import RTK_INF
    from tests.test_gpu_build import _adversarial_scenes
    from tests.test_gpu_closest import make_queries, scene_triangles

    class Deep:
        pass
    d = Deep()
    tris = _adversarial_scenes()["geometric_chain"]
    d.ds = api.DeviceScene.build([dict(positions=tris.reshape(-1, 3))])
    d.tris = scene_triangles(api, d.ds)
    d.entries = d.ds.info()["stack_entries"]
    d.L = M.mix_length(dev.cus, 500000 // len(tris))
    assert d.L * len(tris) <= 500000 and all(s % d.L for s in M.pass_sizes(dev.cus))
    rng = np.random.RandomState(4)
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    # points: the deep ones of tests/test_gpu_closest.py; far away under a small limit (the walk ends at the root); a limit of 0
    pts = np.concatenate([rng.uniform(lo, hi, (12, 3)), tris[rng.permutation(len(tris))[:6], 0], lo + (hi - lo) * rng.uniform(0, 1, (6, 3)) ** 8])
    far = (hi + (hi - lo) * rng.uniform(2, 3, (8, 3))).astype(np.float32)
    shallow = make_queries(np.concatenate([far, far]), np.concatenate([np.full(8, 1e-6), np.zeros(8)]).astype(np.float32))
    d.points = M.deep_mix(make_queries(pts.astype(np.float32), np.full(len(pts), RTK_INF, np.float32)), shallow, d.L)
    # sphere sweeps: the long paths of tests/test_gpu_sweep.py; a path that leads away from the scene; a zero direction
    n = 24
    o = hi + (hi - lo) * rng.uniform(0.1, 0.5, (n, 3))
    s = np.zeros((n, 9), np.float32)
    s[:, 0:3], s[:, 3:6], s[:, 7] = o, lo + (hi - lo) * rng.uniform(0, 1, (n, 3)) ** 8 - o, RTK_INF
    s[:, 8] = rng.uniform(0, 0.05, n) * float((hi - lo).max())
    away = s[:16].copy()
    away[:8, 3:6] *= -1
    away[8:, 3:6] = 0
    d.sweeps = M.deep_mix(s, away, d.L)
    return d


def test_spill_closest_points(api, dev, deep):
    assert deep.entries > api.lib().rtk_amd_closest_stack_entries() == 16
    a = M.brute("closest", deep.tris, (deep.points,))
    assert (a.key[::7] == 1).all() and not np.delete(a.key, np.arange(0, deep.L, 7)).any()
    q = M.tile_rows(deep.points, dev.N)
    check_slots(api, deep.ds, "closest", (q,), a.rows, dev.N)
    _, _, counts = deep.ds.closest_points_counted(api.to_device(q), dev.N)
    print("closest points on the chain: %s" % (counts,))
    assert counts["stack_spills"] > 0 and counts["rays"] == dev.N and counts["hits"] == int(M.tile_rows(a.key, dev.N).sum())


def test_spill_within_count_and_fill(api, dev, deep):
    """the count form (uint32 entries) and the fill form (uint2 entries with keys) with room for 4 per slot"""
    assert deep.entries > api.lib().rtk_amd_within_stack_entries() == 16
    a = M.brute("within", deep.tris, (deep.points,), room=4)
    assert (a.counts[::7] == len(deep.tris)).all() and not np.delete(a.counts, np.arange(0, deep.L, 7)).any()
    q = M.tile_rows(deep.points, dev.N)
    run_count, run_fill, assert_fill = fill_forms("within")
    same(run_count(api, deep.ds, q), M.Tiled(a.counts, dev.N).written(TAIL), "within on the chain, counts")
    t = M.Tiled(a.kept, dev.N)
    assert t.total == 4 * int((np.arange(dev.N) % deep.L % 7 == 0).sum())
    got = run_fill(api, deep.ds, q, t.offsets, t.total)
    assert_fill(got, tuple(t.fill(p, TAIL) for p in a.fills) + (t.written(TAIL),), "within on the chain, room 4")
    _, visits = deep.ds.triangles_within_counted(api.to_device(q), dev.N)
    print("within on the chain, count form: %s" % (visits,))
    assert visits["stack_spills"] > 0 and visits["rays"] == dev.N


def test_spill_sphere_sweeps(api, dev, deep):
    assert deep.entries > api.lib().rtk_amd_sweep_stack_entries() == 16
    a = M.brute("sphere", deep.tris, (deep.sweeps,))
    assert a.key[::7].sum() > deep.L // 14 and not np.delete(a.key, np.arange(0, deep.L, 7)).any()
    s = M.tile_rows(deep.sweeps, dev.N)
    check_slots(api, deep.ds, "sphere", (s,), a.rows, dev.N)
    _, _, _, counts = deep.ds.sweep_spheres_counted(api.to_device(s), dev.N)
    print("sphere sweeps on the chain: %s" % (counts,))
    assert counts["stack_spills"] > 0 and counts["rays"] == dev.N and counts["hits"] == int(M.tile_rows(a.key, dev.N).sum())


def test_scratch_that_grows_and_is_reused(api, dev, deep):
    """One stream, one deep scene: closest points at 257, at N, at 257 again, then the within fill at N. The spill stride of a
    later launch is the capacity an earlier one left."""
    a = M.brute("closest", deep.tris, (deep.points,))
    for n in (257, dev.N, 257):
        check_slots(api, deep.ds, "closest", (M.tile_rows(deep.points, n),), a.rows, n)
    w = M.brute("within", deep.tris, (deep.points,), room=4)
    t = M.Tiled(w.kept, dev.N)
    _, run_fill, assert_fill = fill_forms("within")
    got = run_fill(api, deep.ds, M.tile_rows(deep.points, dev.N), t.offsets, t.total)
    assert_fill(got, tuple(t.fill(p, TAIL) for p in w.fills) + (t.written(TAIL),), "within fill after closest points")
