"""GPU tests of rtk_dev_triangles_in_obb_count / rtk_dev_triangles_in_obb_all. The bar everywhere: counts and ids are bit for bit
what numpy float32 brute force gives by the rule of rtk_amd/csrc/rtk_obb_rule.h (tests/obb_ref.py) over the triangle records the
scene holds at that moment -- read back through rtk_dev_expand_hits --, whatever tree is above them and whatever order the walk
takes. Every output is pre-filled with 0x7e and carries a tail; whole buffers are compared, so nothing may be written beyond a
query's kept entries, outside the segments or behind the batch; rtk_dev_trace_status is 0 after every call. The base scene is the
300-triangle soup of tests/test_gpu_closest.py; every brute force stays below half a million (box, triangle) pairs."""
import ctypes as C

import numpy as np
import pytest

from rtk_amd import synth
from rtk_amd.types import OBB_QUERY_DTYPE
from tests.box_ref import brute_force_boxes
from tests.obb_ref import brute_force_obbs, live_np, reach_np
from tests.test_gpu_box import assert_fill, cut, expected_fill, list_tensors, make_boxes, status_ok
from tests.test_gpu_closest import FILL, TAIL, scene_triangles
from tests.test_obb_cpu import SIGNED_PERMUTATIONS, quaternion_rows

pytestmark = pytest.mark.gpu
F = np.float32
RANDOM = 500                                  # the mix begins with this many boxes with a random rotation each


def records(q):
    """float32 [n, 15] -> OBB_QUERY_DTYPE [n]"""
    return np.ascontiguousarray(q, F).reshape(-1, 15).view(OBB_QUERY_DTYPE).reshape(-1)


def rows(q):
    return np.ascontiguousarray(q).view(F).reshape(-1, 15)


def device_obbs(api, q):
    import torch
    return api.to_device(q) if len(q) else torch.zeros(60, dtype=torch.uint8, device="cuda")


def run_count(api, ds, q, n=None, count=None, ids=None):
    """-> count words [n + TAIL] as the device left them"""
    import torch
    n = len(q) if n is None else n
    d_counts = torch.full(((n + TAIL) * 4,), 0x7e, dtype=torch.uint8, device="cuda")
    d_count, d_ids = list_tensors(count, ids)
    ds.count_in_obbs_device(device_obbs(api, q), n, d_counts, count=d_count, ids=d_ids)
    status_ok(api, ds)
    got = d_counts.cpu().numpy().view(np.uint32)
    assert (got[n:] == FILL).all(), "written beyond num_queries"
    return got


def run_fill(api, ds, q, offsets, total, n=None, with_written=True, count=None, ids=None):
    """offsets: numpy int64 [n + 1] or a cuda tensor; total: ids the segments span. -> (id words [total + TAIL], written words
    [n + TAIL] or None) as the device left them"""
    import torch
    n = len(q) if n is None else n
    d_off = offsets if isinstance(offsets, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(offsets, np.int64)).cuda()
    d_prims = torch.full(((total + TAIL) * 4,), 0x7e, dtype=torch.uint8, device="cuda")
    d_wr = torch.full(((n + TAIL) * 4,), 0x7e, dtype=torch.uint8, device="cuda") if with_written else None
    d_count, d_ids = list_tensors(count, ids)
    ds.in_obbs_all_device(device_obbs(api, q), n, d_off, d_prims, d_wr, count=d_count, ids=d_ids)
    status_ok(api, ds)
    return d_prims.cpu().numpy().view(np.uint32), d_wr.cpu().numpy().view(np.uint32) if with_written else None


IDENTITY = np.eye(3).reshape(1, 9)


def face_queries(pick, e, axis, side, step):
    """Identity axes, half about 0.05 e: the low (side 0) or high face of [qlo, qhi] along `axis` on the vertex coordinate, or on
    its float32 neighbour below (step -1) or above (+1). Centre and half are chosen so that centre -+ half IS that number in
    float32 wherever the subtraction allows (the reference says how often)."""
    at = pick[:, axis].copy()
    if step:
        at = np.nextafter(at, F(step * np.inf))
    h = np.full(len(pick), 0.05 * e, F)
    c = (at + h) if side == 0 else (at - h)                           # float32 each
    h2 = (c - at) if side == 0 else (at - c)
    centre, half = pick.copy(), np.tile(F(0.05 * e), (len(pick), 3))
    centre[:, axis], half[:, axis] = c, h2
    return np.concatenate([centre, half, np.tile(IDENTITY, (len(pick), 1))], 1).astype(F), at


def obb_mix(tris, seed=29):
    """About 1300 oriented boxes over a scene of few triangles -> (queries OBB_QUERY_DTYPE, the face coordinates the third part
    aims at). RANDOM boxes with a random rotation each; identity and signed-permutation axes; identity axes with a face exactly on
    a vertex coordinate and on its float32 neighbours; point, segment and rectangle boxes at vertices and centroids; the whole
    scene; far away; a negative half; NaN and +-inf members; axes scaled by 1.01, sheared, zero."""
    rng = np.random.RandomState(seed)
    tris = np.asarray(tris, F).reshape(-1, 3, 3)
    T = len(tris)
    lo, hi = tris.reshape(-1, 3).min(0).astype(np.float64), tris.reshape(-1, 3).max(0).astype(np.float64)
    ext = hi - lo
    e = float(ext.max()) or float(np.abs(tris).max()) or 1.0
    ext = np.maximum(ext, 1e-3 * e)
    qs = []
    # the random part
    mid = rng.uniform(lo - 0.05 * ext, hi + 0.05 * ext, (RANDOM, 3))
    half = rng.choice([0.01, 0.025, 0.05, 0.1, 0.2], (RANDOM, 1)) * e * rng.uniform(0.3, 1, (RANDOM, 3))
    qs.append(np.concatenate([mid, half, quaternion_rows(rng, RANDOM)], 1))
    # identity and the 48 signed permutations, twice
    mid = rng.uniform(lo, hi, (96, 3))
    axes = np.array([SIGNED_PERMUTATIONS[k % 48].reshape(9) for k in range(96)], np.float64)
    qs.append(np.concatenate([mid, rng.uniform(0.02, 0.2, (96, 3)) * e, axes], 1))
    # faces on vertex coordinates: 40 vertices x 2 axes x (low face, high face) x 3 neighbours
    pick = tris[rng.randint(0, T, 40), rng.randint(0, 3, 40)]
    aims = []
    for axis in (0, 2):
        for side in (0, 1):
            for step in (-1, 0, 1):
                q, at = face_queries(pick, e, axis, side, step)
                qs.append(q); aims.append(at)
    # boxes without volume at vertices and centroids: points, segments, rectangles; turned and not
    verts = tris[rng.randint(0, T, 100), rng.randint(0, 3, 100)]
    cents = tris[rng.randint(0, T, 50)].astype(np.float64).mean(1)
    at = np.concatenate([verts, cents])
    half = rng.uniform(0.02, 0.1, (150, 3)) * e * (np.arange(3)[None, :] < (np.arange(150) % 3)[:, None])      # 0, 1 or 2 extents
    axes = quaternion_rows(rng, 150)
    axes[::2] = IDENTITY
    qs.append(np.concatenate([at, half, axes], 1))
    # the whole scene, turned
    qs.append(np.concatenate([np.tile((lo + hi) / 2, (4, 1)), np.tile(2 * ext, (4, 1)), quaternion_rows(rng, 4)], 1))
    # far away
    far = lo + ext * 1e3 * rng.choice([-1.0, 1.0], (30, 3))
    qs.append(np.concatenate([far, np.tile(ext, (30, 1)), quaternion_rows(rng, 30)], 1))
    # not live: a negative half; NaN and +-inf members; axes scaled by 1.01, sheared, zero
    dead = np.concatenate([np.tile((lo + hi) / 2, (64, 1)), np.tile(ext, (64, 1)), quaternion_rows(rng, 64)], 1)
    dead[np.arange(10), 3 + np.arange(10) % 3] *= -1
    for k in range(24):
        dead[10 + k, (k * 2) % 15] = [np.nan, np.inf, -np.inf, -np.nan][k % 4]
    dead[34:44, 6:] *= 1.01
    dead[44:54, 6:9] += 0.01 * dead[44:54, 9:12]
    dead[np.arange(54, 64), 6 + 3 * (np.arange(10) % 3)] = 0
    dead[np.arange(54, 64), 7 + 3 * (np.arange(10) % 3)] = 0
    dead[np.arange(54, 64), 8 + 3 * (np.arange(10) % 3)] = 0
    qs.append(dead)
    with np.errstate(over="ignore"):
        return records(np.concatenate(qs).astype(F)), np.concatenate(aims).astype(F)


FACES = slice(RANDOM + 96, RANDOM + 96 + 480)
FLAT = slice(RANDOM + 96 + 480, RANDOM + 96 + 480 + 150)
DEAD = 64


@pytest.fixture(scope="module")
def base(api):
    class Base:
        pass
    b = Base()
    b.positions = synth.triangle_soup(300, 0.2, seed=5)
    b.tris = b.positions.reshape(300, 3, 3)
    b.ds = api.DeviceScene.build([dict(positions=b.positions)])
    b.q, b.aims = obb_mix(b.tris)
    b.n = len(b.q)
    # the reference, computed once and shared
    b.ref = brute_force_obbs(b.tris, np.arange(300), b.q)
    b.offsets = np.concatenate([[0], np.cumsum(b.ref.counts.astype(np.int64))])
    return b


def check_mix_is_not_vacuous(q, aims, ref):
    """From the reference alone: what the issue asks the mix to hold"""
    c = ref.counts
    n = len(q)
    w = rows(q)
    live = live_np(w)
    print("obbs %d, pairs %d, mean count %.1f, max %d, empty %.0f %%" % (n, int(c.sum()), c.mean(), c.max(), 100 * (c == 0).mean()))
    assert 1200 <= n <= 1400 and n * ref.step1.shape[1] <= 500000
    rnd = c[:RANDOM]
    framed = (ref.step1.sum(1) > c)[:RANDOM]                         # a triangle passes step 1 and is separated in the frame
    print("random part: %d with a candidate, %d with four or more, %d where the frame decided" % ((rnd > 0).sum(), (rnd >= 4).sum(), framed.sum()))
    assert live[:RANDOM].all() and (rnd > 0).sum() >= RANDOM // 4 and (rnd >= 4).sum() >= 50 and framed.sum() >= 50
    assert live[:-DEAD].all() and not live[-DEAD:].any() and (c[-DEAD:] == 0).all()
    assert (c[RANDOM:RANDOM + 96] > 0).sum() > 48
    # a face on a vertex coordinate: [qlo, qhi] does have that face, and the closed test keeps what the neighbour outside loses
    _, qlo, qhi = reach_np(w[FACES])
    sel = np.arange(480)
    axis, side = (sel // 240) * 2, (sel // 120) % 2
    face = np.where(side == 0, qlo[sel, axis], qhi[sel, axis])
    print("faces exactly on the coordinate aimed at: %d of 480" % (face == aims).sum())
    assert (face == aims).sum() >= 400
    faces = c[FACES].reshape(2, 2, 3, 40)                            # [axis, side, below / at / above, vertex]
    low, high = faces[:, 0], faces[:, 1]
    assert (low[:, 1] > low[:, 2]).any() and (high[:, 0] < high[:, 1]).any()
    assert (c[FLAT] > 0).any() and (c[FLAT.stop:FLAT.stop + 4] == ref.step1.shape[1]).all()
    assert (c[FLAT.stop + 4:FLAT.stop + 34] == 0).all()                # far away
    assert (c == 0).any() and (c == 1).any() and ((c > 1) & (c < 8)).any() and (c > 64).any()


def test_the_mix_is_not_vacuous(base):
    check_mix_is_not_vacuous(base.q, base.aims, base.ref)


def test_count_equals_brute_force(api, base):
    assert scene_triangles(api, base.ds).tobytes() == base.tris.tobytes()
    got = run_count(api, base.ds, base.q)
    bad = np.nonzero(got[:base.n] != base.ref.counts)[0]
    assert len(bad) == 0, (len(bad), bad[:5], base.q[bad[:5]], got[bad[:5]], base.ref.counts[bad[:5]])


def test_fill_with_exact_offsets(api, base):
    """count, torch.cumsum, fill on one stream without a wait in between; then the same with d_written = NULL"""
    import torch
    n, total = base.n, int(base.offsets[-1])
    d_q = api.to_device(base.q)
    d_counts = base.ds.count_in_obbs_device(d_q, n)
    d_offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_offsets[1:] = torch.cumsum(d_counts, 0, dtype=torch.int64)
    got = run_fill(api, base.ds, base.q, d_offsets, total)           # (the buffers are sized from the reference: nothing is read back before)
    assert d_offsets.cpu().numpy().tobytes() == base.offsets.tobytes()
    want = expected_fill(base.ref.lists, base.offsets, total)
    assert_fill(got, want, "exact offsets")
    assert got[1][:n].tobytes() == base.ref.counts.tobytes()
    assert_fill(run_fill(api, base.ds, base.q, base.offsets, total, with_written=False), want, "no written")
    # a float32 [n, 15] tensor is a batch of queries as it stands
    d_f = torch.from_numpy(rows(base.q).copy()).cuda()
    assert d_f.dtype == torch.float32 and d_f.shape == (n, 15)
    assert base.ds.count_in_obbs_device(d_f, n).cpu().numpy().view(np.uint32).tobytes() == base.ref.counts.tobytes()


@pytest.mark.parametrize("k", [0, 1, 3])
def test_at_most_k(api, base, k):
    n = base.n
    offsets = np.arange(n + 1, dtype=np.int64) * k
    got = run_fill(api, base.ds, base.q, offsets, n * k)
    assert_fill(got, expected_fill(cut(base.ref.lists, k), offsets, n * k), "k = %d" % k)
    assert got[1][:n].tobytes() == np.minimum(base.ref.counts, k).astype(np.uint32).tobytes()
    assert_fill(run_fill(api, base.ds, base.q, offsets, n * k, with_written=False), expected_fill(cut(base.ref.lists, k), offsets, n * k), "k = %d, no written" % k)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_sizes(api, base, n):
    which = (np.arange(n) * 7) % base.n                              # (a stride: every part of the mix at every size)
    q = base.q[which]
    got = run_count(api, base.ds, q, n=n)
    assert got[:n].tobytes() == base.ref.counts[which].tobytes()
    offsets = np.arange(n + 1, dtype=np.int64) * 3
    kept = cut([base.ref.lists[i] for i in which], 3)
    assert_fill(run_fill(api, base.ds, q, offsets, n * 3, n=n), expected_fill(kept, offsets, n * 3), "n = %d" % n)


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
    kept = [l[:rooms[i]] for i, l in enumerate(base.ref.lists)]
    assert len(kept[j]) == 0 and any(len(l) == 6 for l in kept) and any(0 < len(l) < rooms[i] for i, l in enumerate(kept))
    got = run_fill(api, base.ds, base.q, offsets, total)
    want = expected_fill(kept, offsets, total)
    assert want[1][j] == 0
    assert_fill(got, want, "ragged")


def test_lists(api, base):
    """A shuffled subset with repeated ids, the count on the device: listed slots as the unlisted call, the rest untouched"""
    n = 1000
    q = base.q[:n]
    lists = base.ref.lists[:n]
    rng = np.random.RandomState(6)
    ids = rng.permutation(n)[:333]
    ids = np.concatenate([ids, ids[:7], rng.permutation(n)[:100]])           # 7 repeated ids; 100 entries beyond the count
    count = 340
    listed = np.zeros(n, bool)
    listed[ids[:count]] = True
    got = run_count(api, base.ds, q, count=count, ids=ids)
    assert (got[:n][~listed] == FILL).all() and got[:n][listed].tobytes() == base.ref.counts[:n][listed].tobytes()
    assert (base.ref.counts[ids[:7]] > 0).any()                              # (a repeated id with something to write)
    k4 = np.arange(n + 1, dtype=np.int64) * 4
    exact = base.offsets[:n + 1]
    for offsets, kept in ((k4, cut(lists, 4)), (exact, lists)):
        total = int(offsets[-1])
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


def check_scene(api, ds, q, ref=None):
    """count, exact fill and k = 3 fill of one scene against brute force over its own records; returns the bytes of all three"""
    n = len(q)
    if ref is None:
        tris = scene_triangles(api, ds)
        ref = brute_force_obbs(tris, np.arange(len(tris)), q)
    counts = run_count(api, ds, q)
    assert counts[:n].tobytes() == ref.counts.tobytes(), np.nonzero(counts[:n] != ref.counts)[0][:5]
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
    q = base.q
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
    moved = (base.positions + rng.uniform(-0.05, 0.05, base.positions.shape)).astype(F)
    ds.refit([dict(positions=moved)])
    assert scene_triangles(api, ds).tobytes() == moved.tobytes()
    ref = brute_force_obbs(moved.reshape(300, 3, 3), np.arange(300), q)
    after_refit = check_scene(api, ds, q, ref)
    assert after_refit != first
    ds.rebuild()
    assert scene_triangles(api, ds).tobytes() == moved.tobytes()
    assert check_scene(api, ds, q, ref) == after_refit


def test_a_stack_deeper_than_the_on_chip_part(api):
    """The geometric cluster of tests/test_gpu_build.py: a deep, lopsided tree; boxes that hold much of it make the walk push past
    the on-chip part"""
    import torch
    from tests.test_gpu_build import _adversarial_scenes
    tris = _adversarial_scenes()["geometric_chain"]
    ds = api.DeviceScene.build([dict(positions=tris.reshape(-1, 3))])
    on_chip = api.lib().rtk_amd_obb_stack_entries()
    assert ds.info()["stack_entries"] > on_chip, (ds.info()["stack_entries"], on_chip)
    rng = np.random.RandomState(4)
    lo, hi = tris.reshape(-1, 3).min(0).astype(np.float64), tris.reshape(-1, 3).max(0).astype(np.float64)
    ext = hi - lo
    whole = np.concatenate([np.tile((lo + hi) / 2, (40, 1)), np.tile(2 * ext.max(), (40, 3)), quaternion_rows(rng, 40)], 1)
    part = np.concatenate([lo + ext * rng.uniform(0, 1, (88, 3)) ** 4, ext.max() * rng.uniform(0, 0.5, (88, 3)) ** 2, quaternion_rows(rng, 88)], 1)
    q = records(np.concatenate([whole, part]).astype(F))
    n = len(q)
    assert n * len(tris) <= 500000
    own = scene_triangles(api, ds)
    ref = brute_force_obbs(own, np.arange(len(own)), q)
    assert (ref.counts[:40] == len(own)).all() and (ref.counts[40:] < len(own)).any() and (ref.counts[40:] > 0).any()
    counts = run_count(api, ds, q)
    assert counts[:n].tobytes() == ref.counts.tobytes()
    offsets = np.arange(n + 1, dtype=np.int64) * 4
    want = expected_fill(cut(ref.lists, 4), offsets, n * 4)
    assert_fill(run_fill(api, ds, q, offsets, n * 4), want, "k = 4")
    # the counting forms say that pushes did go past the on-chip part, and give the same bytes
    d_q = api.to_device(q)
    d_counts, visits = ds.triangles_in_obbs_counted(d_q, n)
    print("geometric_chain: stack entries %d, on chip %d, count form %s" % (ds.info()["stack_entries"], on_chip, visits))
    assert visits["stack_spills"] > 0 and visits["rays"] == n and visits["hits"] == int((ref.counts > 0).sum())
    assert visits["triangles"] >= int(ref.counts.sum())
    assert d_counts.cpu().numpy().view(np.uint32).tobytes() == ref.counts.tobytes()
    d_prims = torch.full(((n * 4 + TAIL) * 4,), 0x7e, dtype=torch.uint8, device="cuda")
    d_wr = torch.full(((n + TAIL) * 4,), 0x7e, dtype=torch.uint8, device="cuda")
    _, fill_visits = ds.triangles_in_obbs_counted(d_q, n, torch.from_numpy(offsets).cuda(), d_prims, d_wr)
    assert fill_visits == visits                                     # (the fill walks what the count walks: nothing kept can cull it)
    assert_fill((d_prims.cpu().numpy().view(np.uint32), d_wr.cpu().numpy().view(np.uint32)), want, "counted k = 4")
    assert api.lib().rtk_dev_trace_status(ds.handle, None) == 0


def integer_scene_and_queries():
    """Triangles, centres and halves with small integer coordinates, every one of the 48 signed permutations as axes: all the
    rule's arithmetic is exact, in the oriented call and in the axis-aligned one on [centre - g, centre + g]"""
    rng = np.random.RandomState(31)
    tris = (rng.randint(-16, 17, (300, 1, 3)) + rng.randint(-4, 5, (300, 3, 3))).astype(F)
    tris[::10, 1] = tris[::10, 0]                                    # segments
    tris[5::20, 2] = tris[5::20, 1] = tris[5::20, 0]                 # points
    n = 48 * 8
    P = np.array([SIGNED_PERMUTATIONS[i % 48] for i in range(n)])
    c = rng.randint(-16, 17, (n, 3))
    h = rng.randint(0, 7, (n, 3))
    g = np.einsum("nji,nj->ni", np.abs(P), h)
    q = records(np.concatenate([c, h, P.reshape(n, 9)], 1).astype(F))
    return tris, q, make_boxes((c - g).astype(F), (c + g).astype(F))


def test_signed_permutation_axes_equal_the_axis_aligned_call(api):
    from tests import test_gpu_box
    tris, q, boxes = integer_scene_and_queries()
    n = len(q)
    ds = api.DeviceScene.build([dict(positions=np.ascontiguousarray(tris.reshape(-1, 3)))])
    own = scene_triangles(api, ds)
    ref = brute_force_obbs(own, np.arange(len(own)), q)
    _, qlo, qhi = reach_np(rows(q))
    assert qlo.tobytes() == boxes["lo"].tobytes() and qhi.tobytes() == boxes["hi"].tobytes()
    assert (ref.counts > 0).sum() > n // 2 and (ref.counts == 0).any() and (ref.step1.sum(1) > ref.counts).sum() > 20
    a, b = run_count(api, ds, q), test_gpu_box.run_count(api, ds, boxes)
    assert a[:n].tobytes() == ref.counts.tobytes()
    assert a.tobytes() == b.tobytes()
    offsets = np.concatenate([[0], np.cumsum(ref.counts.astype(np.int64))])
    total = int(offsets[-1])
    fa, fb = run_fill(api, ds, q, offsets, total), test_gpu_box.run_fill(api, ds, boxes, offsets, total)
    assert_fill(fa, expected_fill(ref.lists, offsets, total), "oriented")
    assert all(x.tobytes() == y.tobytes() for x, y in zip(fa, fb))


def test_the_walk_is_the_axis_aligned_walk(api, base):
    """The skip is the same function on the same numbers: the random part visits exactly the nodes, leaves and triangles that
    rtk_dev_triangles_in_box_counted visits on the queries' (qlo, qhi)"""
    q = base.q[:RANDOM]
    _, qlo, qhi = reach_np(rows(q))
    d_a, va = base.ds.triangles_in_obbs_counted(api.to_device(q), RANDOM)
    d_b, vb = base.ds.triangles_in_boxes_counted(api.to_device(make_boxes(qlo, qhi)), RANDOM)
    print("oriented %s\naxis-aligned on the bounds %s" % (va, vb))
    for key in ("rays", "nodes", "leaves", "triangles", "stack_spills"):
        assert va[key] == vb[key], key
    assert va["nodes"] > RANDOM and va["hits"] <= vb["hits"]
    assert d_a.cpu().numpy().view(np.uint32).tobytes() == base.ref.counts[:RANDOM].tobytes()
    assert (d_a.cpu().numpy().view(np.uint32) <= d_b.cpu().numpy().view(np.uint32)).all()
    assert api.lib().rtk_dev_trace_status(base.ds.handle, None) == 0


def test_more_queries_than_one_pass_of_the_grid(api, base):
    """tests/many_passes.py's batch size -- two passes of the largest grid the device's CUs can hold, five waves and 37: the
    resident grid steps through the batch at least three times; every copy of the mix counts what the first does"""
    import torch
    from tests.many_passes import batch_size
    n = batch_size(torch.cuda.get_device_properties(0).multi_processor_count)
    assert n > (1 << 19) + 3 and n % 64
    d_mix = api.to_device(base.q).view(torch.uint8).reshape(base.n, 60)
    reps = -(-n // base.n)
    d_q = d_mix.repeat(reps, 1)[:n].contiguous()
    d_counts = torch.full(((n + TAIL) * 4,), 0x7e, dtype=torch.uint8, device="cuda")
    base.ds.count_in_obbs_device(d_q, n, d_counts)
    status_ok(api, base.ds)
    got = d_counts.cpu().numpy().view(np.uint32)
    assert (got[n:] == FILL).all()
    assert got[:n].tobytes() == np.tile(base.ref.counts, reps)[:n].tobytes()


def hostile_queries(tris):
    """A scene's own mix cut to 200, and the three groups of tests/hostile_scenes.py as boxes with identity axes: point boxes on
    vertices of copied records, far away, of zero thickness in the plane"""
    from tests import hostile_scenes as H
    lo, hi = H.box_groups(tris)
    with np.errstate(over="ignore", invalid="ignore"):
        c, h = (lo + hi) * F(0.5), (hi - lo) * F(0.5)
    groups = np.concatenate([c, h, np.tile(IDENTITY, (len(c), 1))], 1).astype(F)
    return np.concatenate([H.cut(obb_mix(tris)[0]), records(groups)])


@pytest.mark.parametrize("name", ["mix15", "mix16", "mix10", "mix6", "tiny_cluster_plus_far_triangle", "all_identical", "line_along_x", "huge_coordinates",
                                  "two_distant_clusters", "coplanar", "flat_floor_grid", "zero_area_row", "geometric_chain"])
def test_hostile_scenes(api, name):
    from tests import test_gpu_queries_hostile_scenes as G
    import sys
    m = sys.modules[__name__]
    ds, tris = G.build(api, name)
    q = hostile_queries(tris)
    ref = brute_force_obbs(tris, np.arange(len(tris)), q)
    G.not_vacuous(name, "obb", live_np(rows(q)), ref.counts > 0, G.copies_in(tris, ref.lists))
    G.three_trees(api, ds, tris, lambda ds: G.count_then_fill(m, api, ds, q, ref.counts, ref.lists, len(q)))


def test_python_conveniences(api, base):
    """triangles_in_obbs with matrices and with quaternions, with and without max_per_box; occupancy_oriented on a 6 x 5 x 4 grid
    against brute force over the cells that oriented_grid makes on the host"""
    import torch
    rng = np.random.RandomState(14)
    n = 60
    centres = rng.uniform(0.1, 0.9, (n, 3)).astype(F)
    half = rng.uniform(0.02, 0.2, (n, 3)).astype(F)
    quats = rng.normal(size=(n, 4))
    q = api.obb_query_array(centres, half, quats)
    ref = brute_force_obbs(base.tris, np.arange(300), q)
    assert ref.counts.sum() > 100 and (ref.counts == 0).any()
    for rotation in (quats, api.obb_axes(quats, n)):
        offsets, prims, written = base.ds.triangles_in_obbs(centres, half, rotation)
        assert offsets.dtype == np.int64 and offsets.tobytes() == np.concatenate([[0], np.cumsum(ref.counts.astype(np.int64))]).tobytes()
        assert prims.dtype == np.uint32 and written.dtype == np.uint32 and written.tobytes() == ref.counts.tobytes()
        assert prims.tobytes() == np.concatenate(ref.lists).astype(np.uint32).tobytes()
        offsets, prims, written = base.ds.triangles_in_obbs(centres, half, rotation, max_per_box=3)
        assert offsets.tolist() == list(range(0, 3 * n + 1, 3)) and written.tobytes() == np.minimum(ref.counts, 3).astype(np.uint32).tobytes()
        for i, l in enumerate(cut(ref.lists, 3)):
            assert prims[3 * i:3 * i + len(l)].tobytes() == l.tobytes() and not prims[3 * i + len(l):3 * i + 3].any()   # (beyond written: zero)
    # one rotation and a scalar half for all
    one = base.ds.triangles_in_obbs(centres, 0.1, quats[0])
    ref1 = brute_force_obbs(base.tris, np.arange(300), api.obb_query_array(centres, 0.1, quats[0]))
    assert one[2].tobytes() == ref1.counts.tobytes() and one[1].tobytes() == np.concatenate(ref1.lists).astype(np.uint32).tobytes()
    o, p0, w0 = base.ds.triangles_in_obbs(np.zeros((0, 3), F), 0.1, np.eye(3))
    assert o.tolist() == [0] and len(p0) == 0 and len(w0) == 0
    # the occupancy grid in a turned box about the scene's middle
    centre, ghalf, quat = [0.5, 0.45, 0.55], [0.5, 0.4, 0.3], [0.2, -0.4, 0.1, 0.8]
    occ = base.ds.occupancy_oriented(centre, ghalf, quat, (6, 5, 4))
    status_ok(api, base.ds)
    assert occ.dtype == torch.bool and tuple(occ.shape) == (6, 5, 4) and occ.is_cuda
    cells = api.oriented_grid(centre, ghalf, quat, (6, 5, 4))
    refg = brute_force_obbs(base.tris, np.arange(300), cells)
    assert (refg.counts != 0).any() and (refg.counts == 0).any()
    assert (occ.cpu().numpy().reshape(-1) == (refg.counts != 0)).all()
