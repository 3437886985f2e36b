"""The three overlap queries on an instanced world on the GPU (rtk_dev_world_triangles_in_box_* / _in_obb_* / _touching_*,
rtk_world_overlap.hip). Every comparison is an equality of counts and of 64-bit entries (instance << 32 | prim): against numpy
brute force over (instance, record) by the rule of rtk_amd/csrc/rtk_world_overlap_rule.h (tests/world_overlap_ref.py), and against
the flat placed twin -- DeviceScene.build of the live instances' meshes under their placements, asked by the scene call and mapped
back through mesh_base. Scenes and cases are tests/test_gpu_world.py's. Outputs are pre-filled with 0x7e and carry a tail that
must stay untouched. References are computed once per (case, shape) and shared."""
import numpy as np
import pytest

from tests import many_passes as M
from tests import world_overlap_ref as R
from tests import world_ref
from tests.test_gpu_world import TRIS, case
from tests.world_closest_ref import live_instances, placed_tris
from tests.world_ref import F, PRIM_NONE, placement

pytestmark = pytest.mark.gpu

TAIL = 5
FILL = 0x7e7e7e7e
FILL64 = np.uint64(0x7e7e7e7e7e7e7e7e)
N_LIVE, N_OTHER = 2048, 256
WORLD = {"box": "in_box", "obb": "in_obb", "touch": "touching"}          # DeviceWorld.triangles_<..>_count_device, ...
SCENE = {"box": "in_boxes", "obb": "in_obbs", "touch": "touching"}       # DeviceScene.count_<..>_device, <..>_all_device
# the extent of the queries per case: sized until the reference satisfies what test 1 and the room test ask of it (a query
# reaches about this far from the record it is built around; the instances are 1 to 4 across and, in "65" and "257", a few apart)
SIZE = {"one": 0.5, "two": 0.5, "65": 2.5, "257": 2.5, "special": 0.5}


@pytest.fixture(scope="module")
def scenes(api):
    return [api.DeviceScene.build([dict(positions=t.reshape(-1, 3))]) for t in TRIS]


_CASES = {}


def reference(name, shape):
    """(which, places, queries [N_LIVE + N_OTHER, floats], Answer): the reference, computed once per (case, shape) and shared"""
    if (name, shape) not in _CASES:
        which, places = case(name)
        rng = np.random.RandomState(71 + R.SHAPES.index(shape))
        q = R.make_queries(shape, TRIS, which, places, rng, N_LIVE, N_OTHER, SIZE[name])
        _CASES[(name, shape)] = (which, places, q, R.brute_force(shape, TRIS, which, places, q, prune=True))
    return _CASES[(name, shape)]


def lists_of(d_count=None, ids=None):
    import torch
    return (torch.tensor([d_count], dtype=torch.int64, device="cuda") if d_count is not None else None,
            torch.from_numpy(np.ascontiguousarray(ids, np.int64)).cuda() if ids is not None else None)


def run_count(api, world, shape, q, n=None, count=None, ids=None, **kw):
    """-> counts uint32 [n + TAIL] as the device left them"""
    import torch
    n = len(q) if n is None else n
    d_counts = torch.full(((n + TAIL) * 4,), 0x7e, dtype=torch.uint8, device="cuda")
    d_count, d_ids = lists_of(count, ids)
    getattr(world, "triangles_%s_count_device" % WORLD[shape])(api.to_device(q), n, d_counts, count=d_count, ids=d_ids, **kw)
    world.status()
    got = d_counts.cpu().numpy().view(np.uint32)
    assert (got[n:] == FILL).all(), "written beyond num_queries"
    return got


def run_fill(api, world, shape, q, offsets, total, n=None, count=None, ids=None, written=True, **kw):
    """-> (entries uint64 [total + TAIL], written uint32 [n + TAIL] or None) as the device left them"""
    import torch
    n = len(q) if n is None else n
    d_entries = torch.full(((total + TAIL) * 8,), 0x7e, dtype=torch.uint8, device="cuda")
    d_written = torch.full(((n + TAIL) * 4,), 0x7e, dtype=torch.uint8, device="cuda") if written else None
    d_offsets = torch.from_numpy(np.ascontiguousarray(offsets, np.int64)).cuda()
    d_count, d_ids = lists_of(count, ids)
    getattr(world, "triangles_%s_all_device" % WORLD[shape])(api.to_device(q), n, d_offsets, d_entries, d_written, count=d_count, ids=d_ids, **kw)
    world.status()
    entries = d_entries.cpu().numpy().view(np.uint64)
    wr = d_written.cpu().numpy().view(np.uint32) if written else None
    assert (entries[total:] == FILL64).all() and (wr is None or (wr[n:] == FILL).all()), "written beyond the buffers"
    return entries, wr


def expected_fill(kept, offsets, total):
    """entries uint64 [total + TAIL]: kept[i] from offsets[i] on, 0x7e everywhere else"""
    out = np.full(total + TAIL, FILL64, np.uint64)
    for i, l in enumerate(kept):
        out[int(offsets[i]):int(offsets[i]) + len(l)] = l
    return out


def count_then_fill(api, world, shape, q, want, **kw):
    """count -> cumsum -> fill equal the reference exactly"""
    n = len(q)
    counts = run_count(api, world, shape, q, **kw)
    assert (counts[:n] == want.counts).all(), (shape, np.flatnonzero(counts[:n] != want.counts)[:6])
    offsets = np.concatenate([[0], np.cumsum(counts[:n].astype(np.int64))])
    total = int(offsets[-1])
    entries, wr = run_fill(api, world, shape, q, offsets, total, **kw)
    assert (wr[:n] == want.counts).all()
    assert (entries[:total] == want.flat()).all(), shape


def twin_answer(api, shape, which, places, q, live=None, skip_shared=False):
    """the flat placed twin's scene call, its prims mapped back through mesh_base to entries: (counts [n], entries uint64 [total])"""
    import torch
    live = np.flatnonzero(live_instances(TRIS, which, places) if live is None else live)
    twin = api.DeviceScene.build([dict(positions=TRIS[which[k]].reshape(-1, 3)) for k in live], placements=places[live])
    base = np.asarray(twin.mesh_base(), np.int64)
    n = len(q)
    d_q = api.to_device(q)
    kw = dict(skip_shared=skip_shared) if shape == "touch" else {}
    d_counts = getattr(twin, "count_%s_device" % SCENE[shape])(d_q, n, **kw)
    d_offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_offsets[1:] = torch.cumsum(d_counts, 0, dtype=torch.int64)
    total = int(d_offsets[n].item())
    d_prims = torch.zeros(max(total, 1), dtype=torch.int32, device="cuda")
    getattr(twin, "%s_all_device" % SCENE[shape])(d_q, n, d_offsets, d_prims, **kw)
    torch.cuda.synchronize()
    prims = d_prims.cpu().numpy().view(np.uint32)[:total].astype(np.int64)
    mesh = np.searchsorted(base[:len(live)], prims, side="right") - 1
    return d_counts.cpu().numpy().view(np.uint32), R.keys_of(live[mesh], prims - base[mesh])


@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("name", ["one", "two", "65", "257", "special"])
def test_world_equals_brute_force_and_the_flat_twin(api, scenes, name, shape):
    which, places, q, want = reference(name, shape)
    # from the reference alone, before the device is asked
    assert len(q) == N_LIVE + N_OTHER and (want.counts[:N_LIVE] > 0).all() and (want.counts[N_LIVE:] == 0).all()
    if name in ("65", "257"):
        several = (want.instances[:N_LIVE] >= 2).mean()
        print("case %s, %s: %.1f %% of the queries have candidates in two or more instances" % (name, shape, 100 * several))
        assert several >= 0.10
    world = api.DeviceWorld.create(scenes, which, places)
    count_then_fill(api, world, shape, q, want)
    counts, entries = twin_answer(api, shape, which, places, q)
    assert (counts == want.counts).all() and (entries == want.flat()).all()
    # the numpy convenience
    fn = getattr(world, "triangles_" + WORLD[shape])
    args = (q[:100, :3], q[:100, 3:6], q[:100, 6:].reshape(-1, 3, 3)) if shape == "obb" else (q[:100],)
    c, inst, prims = fn(*args)
    assert (c == want.counts[:100]).all() and (R.keys_of(inst, prims) == np.concatenate(want.lists[:100])).all()
    world.free()


@pytest.mark.parametrize("shape", R.SHAPES)
def test_room(api, scenes, shape):
    which, places, q, want = reference("65", shape)
    n = len(q)
    assert (want.counts > 4).mean() >= 0.25                                  # from the reference: room 4 cuts a quarter of the lists
    world = api.DeviceWorld.create(scenes, which, places)
    for k in (1, 4):
        offsets = np.arange(n + 1, dtype=np.int64) * k
        entries, wr = run_fill(api, world, shape, q, offsets, n * k)
        assert (wr[:n] == np.minimum(want.counts, k)).all()
        assert (entries == expected_fill(want.kept(np.full(n, k)), offsets, n * k)).all(), k
    # room 0 for every third query: nothing written for it, written = 0
    room = np.where(np.arange(n) % 3 == 0, 0, 3)
    offsets = np.concatenate([[0], np.cumsum(room)]).astype(np.int64)
    total = int(offsets[-1])
    entries, wr = run_fill(api, world, shape, q, offsets, total)
    assert (wr[:n] == np.minimum(want.counts, room)).all()
    assert (entries == expected_fill(want.kept(room), offsets, total)).all()
    # without d_written
    entries2, none = run_fill(api, world, shape, q, offsets, total, written=False)
    assert none is None and (entries2 == entries).all()
    # offsets that decrease mean no room: nothing is written anywhere, written = 0
    down = (n - np.arange(n + 1, dtype=np.int64)) * 4
    entries, wr = run_fill(api, world, shape, q, down, 4 * n)
    assert (entries == FILL64).all() and (wr[:n] == 0).all()
    world.free()


@pytest.mark.parametrize("shape", R.SHAPES)
def test_lists_and_filters(api, scenes, shape):
    which, places, q, want = reference("65", shape)
    n = 1200
    q = q[:n]
    world = api.DeviceWorld.create(scenes, which, places)
    rng = np.random.RandomState(6)
    ids = rng.permutation(n)[:333]
    ids = np.concatenate([ids, ids[:7], [n, n + 3, 0xFFFFFFFF], rng.permutation(n)[:100]])       # 7 repeated ids, 3 ids >= n; 100 entries beyond the count
    count = 343
    listed = np.zeros(n, bool)
    listed[ids[:340]] = True
    counts = run_count(api, world, shape, q, count=count, ids=ids)
    assert (counts[:n][~listed] == FILL).all() and (counts[:n][listed] == want.counts[:n][listed]).all()
    offsets = np.concatenate([[0], np.cumsum(want.counts[:n].astype(np.int64))])
    total = int(offsets[-1])
    entries, wr = run_fill(api, world, shape, q, offsets, total, count=count, ids=ids)
    assert (wr[:n][~listed] == FILL).all() and (wr[:n][listed] == want.counts[:n][listed]).all()
    kept = [l if listed[i] else l[:0] for i, l in enumerate(want.lists[:n])]
    assert (entries == expected_fill(kept, offsets, total)).all()            # a repeated query is answered once, an unlisted one not at all
    # no ids: the first `count` queries; an empty list writes nothing
    counts = run_count(api, world, shape, q, count=100)
    assert (counts[100:] == FILL).all() and (counts[:100] == want.counts[:100]).all()
    assert (run_count(api, world, shape, q, count=0, ids=ids) == FILL).all()
    # the instance mask (the odd instances and those beyond bit 60 are out) and a per-slot ignored instance, each and both
    q = reference("65", shape)[2]
    mask = np.zeros(60, bool)
    mask[::2] = True
    first = np.array([R.decode(l[:1])[0][0] if len(l) else PRIM_NONE for l in want.lists], np.uint32)
    ign = first.copy()
    ign[::7] = PRIM_NONE
    flags = dict(skip_shared=True) if shape == "touch" else {}
    for kw in (dict(instance_mask=mask), dict(ignore_instance=ign), dict(instance_mask=mask, ignore_instance=ign)):
        ref = R.brute_force(shape, TRIS, which, places, q, mask=kw.get("instance_mask"), ignore=kw.get("ignore_instance"), prune=True,
                            flags=R.SKIP_SHARED_VERTEX if flags else 0)
        assert (ref.counts != want.counts).mean() > 0.2
        count_then_fill(api, world, shape, q, ref, **kw, **flags)
    # ... and a twin built from the instances the mask lets through
    live = live_instances(TRIS, which, places)
    live[1::2] = False
    live[60:] = False
    ref = R.brute_force(shape, TRIS, which, places, q, mask=mask, prune=True)
    counts, entries = twin_answer(api, shape, which, places, q, live=live)
    assert (counts == ref.counts).all() and (entries == ref.flat()).all()
    # a mask that lets nothing through: zeros
    assert (run_count(api, world, shape, q, instance_mask=np.zeros(65, bool))[:len(q)] == 0).all()
    world.free()


@pytest.mark.parametrize("name", ["special", "65"])
def test_shared_vertices_are_left_out_on_the_placed_vertices(api, scenes, name):
    """touch_flags: query triangles with a vertex that has the bits of a placed vertex. With RTK_TOUCH_SKIP_SHARED_VERTEX the
    records around that vertex are left out, without it they are listed: count and fill against brute force and against the flat
    placed twin asked with the same flag, which compares its own placed vertices"""
    import torch
    which, places = case(name)
    q = R.shared_vertex_queries(TRIS, which, places, np.random.RandomState(67), 1024)
    plain = R.brute_force("touch", TRIS, which, places, q, prune=True)
    skipped = R.brute_force("touch", TRIS, which, places, q, flags=R.SKIP_SHARED_VERTEX, prune=True)
    # from the reference alone: the flag removes candidates from every query, adds none, and leaves some
    assert (plain.counts > skipped.counts).all() and all(np.isin(b, a).all() for a, b in zip(plain.lists, skipped.lists))
    assert (skipped.counts > 0).mean() > 0.5
    world = api.DeviceWorld.create(scenes, which, places)
    n = len(q)
    for flag, want in ((False, plain), (True, skipped)):
        count_then_fill(api, world, "touch", q, want, skip_shared=flag)
        counts, entries = twin_answer(api, "touch", which, places, q, skip_shared=flag)
        assert (counts == want.counts).all() and (entries == want.flat()).all(), flag
        # the counted forms and the numpy convenience carry the flag too
        d_counts, ctr = world.triangles_touching_counted(api.to_device(q), n, skip_shared=flag)
        assert (d_counts.cpu().numpy().view(np.uint32) == want.counts).all() and ctr["hits"] == int((want.counts > 0).sum())
        offsets = np.arange(n + 1, dtype=np.int64) * 2
        d_entries = torch.full(((2 * n + TAIL) * 8,), 0x7e, dtype=torch.uint8, device="cuda")
        world.triangles_touching_counted(api.to_device(q), n, torch.from_numpy(offsets).cuda(), d_entries, skip_shared=flag)
        assert (d_entries.cpu().numpy().view(np.uint64) == expected_fill(want.kept(np.full(n, 2)), offsets, 2 * n)).all()
        c, inst, prims = world.triangles_touching(q[:200], skip_shared=flag)
        assert (c == want.counts[:200]).all() and (R.keys_of(inst, prims) == np.concatenate(want.lists[:200])).all()
    world.free()


def scene_triangles(api, ds):
    from tests.test_gpu_closest import scene_triangles as st
    return st(api, ds)


def test_the_trees_do_not_matter(api, scenes):
    """The instances' scenes from the CPU task builder's blob (leaves of 4 to 63, loose boxes) with split_leaves applied, and the
    top tree rebuilt: the same bytes"""
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
    same_records = all(a.tobytes() == b.tobytes() for a, b in zip(mine, TRIS))
    for shape in R.SHAPES:
        which, places, q, want = reference("special", shape)
        if not same_records:                                                 # (a blob that orders its records otherwise: their own brute force)
            want = R.brute_force(shape, mine, which, places, q, prune=True)
        world = api.DeviceWorld.create(ups, which, places)
        count_then_fill(api, world, shape, q, want)
        world.rebuild()
        count_then_fill(api, world, shape, q, want)
        world.free()


def test_the_spill_path(api, scenes):
    """A world whose deepest scene is the line scene, and queries that cover all of it: every node is entered, every sibling pushed"""
    import torch
    which, places = case("special")
    world = api.DeviceWorld.create(scenes, which, places)
    on_chip = api.lib().rtk_amd_world_overlap_stack_entries()
    assert world.info()["stack_entries"] > on_chip > 0
    line = placed_tris(TRIS[2], places[3]).reshape(-1, 3).astype(np.float64)
    lo, hi = line.min(0) - 0.5, line.max(0) + 0.5
    cent = line.reshape(-1, 3, 3).mean(1)                                    # the records' centroids lie on the line's axis
    rng = np.random.RandomState(47)
    for shape in R.SHAPES:
        _, _, q, _ = reference("special", shape)
        q = q[:192].copy()
        for i in range(64):                                                  # the first 64 cover the line instance
            if shape == "box":
                q[i] = np.concatenate([lo - rng.uniform(0, 1, 3), hi + rng.uniform(0, 1, 3)])
            elif shape == "obb":
                q[i] = np.concatenate([(lo + hi) / 2, (hi - lo) * rng.uniform(1.0, 1.5), q[i, 6:]])
            else:
                c, u, v = cent.mean(0), cent[0] - cent[-1], np.array([0.0, 0.0, 1.0])      # a big triangle that holds the line's axis
                r = np.linalg.norm(u)
                u = u / r
                q[i] = np.concatenate([c + 3 * r * u + rng.uniform(-0.01, 0.01, 3), c - 3 * r * u + 3 * r * v, c - 3 * r * u - 3 * r * v])
        q = q.astype(F)
        ref = R.brute_force(shape, TRIS, which, places, q, prune=True)
        assert (R.decode(ref.flat())[0] == 3).sum() > 64 * 1000              # from the reference: most of the 2048 records, 64 times
        count_then_fill(api, world, shape, q, ref)
        n = len(q)
        fn = getattr(world, "triangles_%s_counted" % WORLD[shape])
        d_counts, ctr = fn(api.to_device(q), n)
        print("spill, %s: stack entries %d, on chip %d, counts %s" % (shape, world.info()["stack_entries"], on_chip, ctr))
        assert ctr["stack_spills"] > 0 and ctr["rays"] == n and ctr["hits"] == int((ref.counts > 0).sum())
        assert ctr["triangles"] >= int(ref.counts.sum())
        assert (d_counts.cpu().numpy().view(np.uint32) == ref.counts).all()
        # the counted fill form with room 4: the bytes of the plain call
        offsets = np.arange(n + 1, dtype=np.int64) * 4
        d_entries = torch.full(((4 * n + TAIL) * 8,), 0x7e, dtype=torch.uint8, device="cuda")
        d_wr, ctr = fn(api.to_device(q), n, torch.from_numpy(offsets).cuda(), d_entries)
        assert ctr["stack_spills"] > 0
        plain, wr = run_fill(api, world, shape, q, offsets, 4 * n)
        assert (d_entries.cpu().numpy().view(np.uint64) == plain).all() and (d_wr.cpu().numpy().view(np.uint32) == wr[:n]).all()
        assert (plain == expected_fill(ref.kept(np.full(n, 4)), offsets, 4 * n)).all()
        world.status()                                                       # the launch-error word is clear
    world.free()


@pytest.mark.parametrize("shape", R.SHAPES)
def test_past_one_pass_of_the_grid(api, scenes, shape):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    N, L = M.batch_size(cus), M.mix_length(cus, 600)
    which, places, q, want = reference("65", shape)
    # a prime-length mix of queries with short lists, dead ones and misses in turn, so that consecutive steps of a lane differ
    short = np.flatnonzero(want.counts <= 8)
    pick = short[np.random.RandomState(9).permutation(len(short))[:L]]
    assert len(pick) == L and all(s % L for s in M.pass_sizes(cus))
    counts = want.counts[pick]
    assert 0.05 < (counts == 0).mean() < 0.5 and len(np.unique(counts)) >= 5
    world = api.DeviceWorld.create(scenes, which, places)
    batch = M.tile_rows(q[pick], N)
    t = M.Tiled(counts, N)
    got = run_count(api, world, shape, batch)
    assert (got == t.written(TAIL)).all()
    entries, wr = run_fill(api, world, shape, batch, t.offsets, t.total)
    period = np.concatenate([want.lists[i] for i in pick] + [np.zeros(0, np.uint64)])
    assert (entries.view(np.uint32).reshape(-1, 2) == t.fill(period.view(np.uint32).reshape(-1, 2), TAIL)).all()
    assert (wr == t.written(TAIL)).all()
    world.free()


def test_update_equals_the_reference_of_the_new_state(api, scenes):
    which, places = case("65")
    rng = np.random.RandomState(8)
    moved = places.copy()
    moved[::2] = world_ref.random_placements(len(moved[::2]), rng, 12.0)    # half the instances move
    moved[which == 2] = places[which == 2]
    own = api.DeviceScene.build([dict(positions=TRIS[1].reshape(-1, 3))])
    grown = (TRIS[1] * F(1.5)).astype(F)
    mine = [TRIS[0], grown, TRIS[2]]
    world = api.DeviceWorld.create([scenes[0], own, scenes[2]], which, places)
    for shape in R.SHAPES:
        _, _, q, before = reference("65", shape)
        count_then_fill(api, world, shape, q, before)
    world.update(moved)
    own.refit([dict(positions=grown.reshape(-1, 3))])
    world.update(None)
    for shape in R.SHAPES:
        _, _, q, before = reference("65", shape)
        ref = R.brute_force(shape, mine, which, moved, q, prune=True)
        assert (ref.counts != before.counts).mean() > 0.3
        count_then_fill(api, world, shape, q, ref)
    world.free()


def test_dead_instances_and_empty_scenes_are_never_listed(api, scenes):
    empty = api.DeviceScene.build([dict(positions=np.zeros((0, 3), F))])
    singular = placement(np.array([[1, 2, 3], [1, 2, 3], [0, 0, 1]]), (0, 0, 0))
    nan = placement(None, (np.nan, 0, 0))
    which, places = case("special")
    which2 = np.concatenate([[1], which, [3, 0]]).astype(np.uint32)         # a singular sphere first, a placed empty scene, a NaN cube
    places2 = np.concatenate([[singular], places, [placement(None, (0, 0, 0)), nan]])
    world = api.DeviceWorld.create(scenes + [empty], which2, places2)
    assert world.info()["dead_instances"] == 3
    for shape in R.SHAPES:
        _, _, q, want = reference("special", shape)
        # the live instances are numbered one higher; 0, 5 and 6 never appear
        inst, prim = R.decode(want.flat())
        moved = R.Answer(want.counts, [R.keys_of(R.decode(l)[0] + 1, R.decode(l)[1]) for l in want.lists])
        assert set(np.unique(inst + 1)) <= {1, 2, 3, 4}
        count_then_fill(api, world, shape, q, moved)
    world.free()


def test_refusals_and_no_queries(api, scenes):
    import ctypes as C
    import torch
    which, places = case("two")
    world = api.DeviceWorld.create(scenes, which, places)
    L = api.lib()
    d = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = C.c_void_p(d.data_ptr())
    from tests.test_world_cpu import ERR_BAD_ARG
    f = api.WorldFilter()
    f.struct_size, f.flags = C.sizeof(api.WorldFilter), 1
    l = api.RayList()
    l.struct_size, l.flags, l.d_ids, l.d_count = C.sizeof(api.RayList), 0, None, None
    for stem in ("rtk_dev_world_triangles_in_box", "rtk_dev_world_triangles_in_obb", "rtk_dev_world_triangles_touching"):
        flags = (0,) if stem.endswith("touching") else ()
        fn_count, fn_all = getattr(L, stem + "_count"), getattr(L, stem + "_all")
        for args in ((None, p, 4, None, None, *flags, p, None), (world.handle, None, 4, None, None, *flags, p, None),
                     (world.handle, p, 4, None, None, *flags, None, None), (world.handle, p, 4, C.byref(l), None, *flags, p, None),
                     (world.handle, p, 4, None, C.byref(f), *flags, p, None), (world.handle, p, 1 << 32, None, None, *flags, p, None)):
            assert fn_count(*args) == ERR_BAD_ARG and stem + "_count" in api.last_error(), (stem, api.last_error())
        assert fn_all(world.handle, p, 4, None, None, *flags, p, None, None, None) == ERR_BAD_ARG and stem + "_all" in api.last_error()
        assert fn_all(world.handle, p, 4, None, None, *flags, None, p, None, None) == ERR_BAD_ARG and stem + "_all" in api.last_error()
        # no queries: nothing to do
        assert fn_count(world.handle, None, 0, None, None, *flags, None, None) == 0
        assert fn_all(world.handle, None, 0, None, None, *flags, None, None, None, None) == 0
    assert L.rtk_dev_world_triangles_touching_count(world.handle, p, 4, None, None, 2, p, None) == ERR_BAD_ARG
    assert "rtk_dev_world_triangles_touching_count" in api.last_error() and "touch_flags" in api.last_error()
    world.status()
    world.free()
