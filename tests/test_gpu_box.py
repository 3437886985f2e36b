"""GPU tests of rtk_dev_triangles_in_box_count / rtk_dev_triangles_in_box_all. The bar everywhere: counts and ids are bit for bit
what numpy float32 brute force gives by the rule of rtk_amd/csrc/rtk_box_rule.h (tests/box_ref.py) over the triangle records the
scene holds at that moment -- read back through rtk_dev_expand_hits --, whatever tree is above them and whatever order the walk
takes. Every output is pre-filled with 0x7e and carries a tail; whole buffers are compared, so nothing may be written beyond a
query's kept entries, outside the segments or behind the batch; rtk_dev_trace_status is 0 after every call. The base scene is the
300-triangle soup of tests/test_gpu_closest.py; every brute force stays below half a million (box, triangle) pairs."""
import ctypes as C

import numpy as np
import pytest

from rtk_amd import synth
from rtk_amd.types import BOX_QUERY_DTYPE
from tests.box_ref import brute_force_boxes
from tests.test_gpu_closest import FILL, TAIL, scene_triangles

pytestmark = pytest.mark.gpu


def status_ok(api, ds):
    import torch
    assert api.lib().rtk_dev_trace_status(ds.handle, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0, api.last_error()


def make_boxes(lo, hi):
    q = np.zeros(len(lo), BOX_QUERY_DTYPE)
    q["lo"], q["hi"] = lo, hi
    return q


def device_boxes(api, boxes):
    import torch
    return api.to_device(boxes) if len(boxes) else torch.zeros(24, dtype=torch.uint8, device="cuda")


def list_tensors(count, ids):
    import torch
    d_count = torch.tensor([count], dtype=torch.int64, device="cuda") if count is not None else None
    d_ids = torch.from_numpy(np.ascontiguousarray(ids, np.int64)).cuda() if ids is not None else None
    return d_count, d_ids


def run_count(api, ds, boxes, n=None, count=None, ids=None):
    """-> count words [n + TAIL] as the device left them"""
    import torch
    n = len(boxes) if n is None else n
    d_counts = torch.full(((n + TAIL) * 4,), 0x7e, dtype=torch.uint8, device="cuda")
    d_count, d_ids = list_tensors(count, ids)
    ds.count_in_boxes_device(device_boxes(api, boxes), n, d_counts, count=d_count, ids=d_ids)
    status_ok(api, ds)
    got = d_counts.cpu().numpy().view(np.uint32)
    assert (got[n:] == FILL).all(), "written beyond num_queries"
    return got


def run_fill(api, ds, boxes, offsets, total, n=None, with_written=True, count=None, ids=None):
    """offsets: numpy int64 [n + 1] or a cuda tensor; total: ids the segments span. -> (id words [total + TAIL], written words
    [n + TAIL] or None) as the device left them"""
    import torch
    n = len(boxes) if n is None else n
    d_off = offsets if isinstance(offsets, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(offsets, np.int64)).cuda()
    d_prims = torch.full(((total + TAIL) * 4,), 0x7e, dtype=torch.uint8, device="cuda")
    d_wr = torch.full(((n + TAIL) * 4,), 0x7e, dtype=torch.uint8, device="cuda") if with_written else None
    d_count, d_ids = list_tensors(count, ids)
    ds.in_boxes_all_device(device_boxes(api, boxes), n, d_off, d_prims, d_wr, count=d_count, ids=d_ids)
    status_ok(api, ds)
    return d_prims.cpu().numpy().view(np.uint32), d_wr.cpu().numpy().view(np.uint32) if with_written else None


def expected_fill(kept, offsets, total, listed=None):
    """The whole output as it must stand: kept[i] at offsets[i] for every (listed) query, 0x7e everywhere else"""
    n = len(kept)
    prims = np.full(total + TAIL, FILL, np.uint32)
    wr = np.full(n + TAIL, FILL, np.uint32)
    for i in range(n):
        if listed is not None and not listed[i]:
            continue
        room = max(0, int(offsets[i + 1]) - int(offsets[i]))
        k = min(len(kept[i]), room)
        prims[offsets[i]:offsets[i] + k] = kept[i][:k]
        wr[i] = k
    return prims, wr


def assert_fill(got, want, what=""):
    for g, w, name in zip(got, want, ("ids", "written")):
        if g is None:
            continue
        if g.tobytes() != w.tobytes():
            bad = np.nonzero(g != w)[0]
            raise AssertionError("%s %s: %d words differ, first %s: got %s want %s" % (what, name, len(bad), bad[:5], g[bad[:5]], w[bad[:5]]))


def cut(lists, k):
    return [l[:k] for l in lists]


def box_mix(tris, seed=23):
    """About 1300 boxes over a scene of few triangles: uniform small cubes; boxes with a face exactly on a vertex coordinate and
    on its float32 neighbours either side; point boxes at vertices and centroids; thin slabs; the whole scene; far away; lo > hi;
    NaN and +-inf members."""
    rng = np.random.RandomState(seed)
    tris = np.asarray(tris, np.float32).reshape(-1, 3, 3)
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    ext = hi - lo
    e = float(ext.max())
    los, his = [], []
    # 500 uniform cubes
    mid = rng.uniform(lo - 0.05 * ext, hi + 0.05 * ext, (500, 3))
    half = rng.choice([0.01, 0.025, 0.05, 0.1, 0.2], (500, 1)) * e
    los.append(mid - half); his.append(mid + half)
    # a face exactly on a vertex coordinate, and on its float32 neighbours: 40 vertices x (low face, high face) x 3 neighbours x 2 axes
    pick = tris[rng.permutation(len(tris))[:40], rng.randint(0, 3, 40)]
    for axis in (0, 2):
        for side in (0, 1):
            for step in (-1, 0, 1):
                at = pick[:, axis].copy()
                if step:
                    at = np.nextafter(at, np.float32(step * np.inf))
                blo, bhi = pick - np.float32(0.05 * e), pick + np.float32(0.05 * e)
                if side == 0:
                    blo[:, axis] = at                                  # the vertex on, just inside, just outside the low face
                else:
                    bhi[:, axis] = at
                los.append(blo); his.append(bhi)
    # point boxes at vertices and at centroids
    verts = tris[rng.permutation(len(tris))[:100], rng.randint(0, 3, 100)]
    cents = tris[rng.permutation(len(tris))[:50]].astype(np.float64).mean(1)
    los += [verts, cents]; his += [verts, cents]
    # thin slabs: the whole scene on two axes, thin or flat on the third
    for k in range(60):
        a = k % 3
        blo, bhi = lo - 0.1 * ext, hi + 0.1 * ext
        at = rng.uniform(lo[a], hi[a])
        blo[a], bhi[a] = at, at + rng.choice([0.0, 1e-6, 1e-3, 1e-2]) * e
        los.append(blo[None]); his.append(bhi[None])
    # the whole scene, exactly and with room
    los += [lo[None], (lo - ext)[None], (lo - 1e30)[None], lo[None]]
    his += [hi[None], (hi + ext)[None], (hi + 1e30)[None], (hi + 3e38)[None]]
    # far away
    far = lo + ext * 1e3 * rng.choice([-1.0, 1.0], (50, 3))
    los.append(far); his.append(far + ext)
    # lo > hi on one axis; NaN and +-inf members
    inside = rng.uniform(lo, hi, (20, 3))
    blo, bhi = inside - 0.3 * ext, inside + 0.3 * ext
    blo[np.arange(20), np.arange(20) % 3] = bhi[np.arange(20), np.arange(20) % 3] + 1e-3
    los.append(blo); his.append(bhi)
    blo, bhi = np.tile(lo - ext, (24, 1)), np.tile(hi + ext, (24, 1))
    for k in range(24):
        (blo if k % 2 == 0 else bhi)[k, (k // 2) % 3] = [np.nan, np.inf, -np.inf, -np.nan][(k // 6) % 4]
    los.append(blo); his.append(bhi)
    with np.errstate(over="ignore"):
        return make_boxes(np.concatenate(los).astype(np.float32), np.concatenate(his).astype(np.float32))


@pytest.fixture(scope="module")
def base(api):
    class Base:
        pass
    b = Base()
    b.positions = synth.triangle_soup(300, 0.2, seed=5)
    b.tris = b.positions.reshape(300, 3, 3)
    b.ds = api.DeviceScene.build([dict(positions=b.positions)])
    b.boxes = box_mix(b.tris)
    b.n = len(b.boxes)
    # the reference, computed once and shared
    b.ref = brute_force_boxes(b.tris, np.arange(300), b.boxes["lo"], b.boxes["hi"])
    b.offsets = np.concatenate([[0], np.cumsum(b.ref.counts.astype(np.int64))])
    return b


def test_the_reference_has_empty_short_and_long_lists(base):
    c = base.ref.counts
    print("boxes %d, pairs %d, mean count %.1f, max %d, empty %.0f %%" % (base.n, int(c.sum()), c.mean(), c.max(), 100 * (c == 0).mean()))
    assert 1200 <= base.n <= 1400 and base.n * 300 <= 500000
    assert (c == 0).any() and (c == 1).any() and ((c > 1) & (c < 8)).any() and (c > 64).any() and (c == 300).sum() >= 4
    assert (c[:500] > 0).any() and (c[:500] == 0).any()
    # a face on a vertex coordinate: the closed test keeps what the neighbour outside loses
    faces = c[500:980].reshape(2, 2, 3, 40)                          # [axis, side, below / at / above, vertex]
    low, high = faces[:, 0], faces[:, 1]
    assert (low[:, 1] > low[:, 2]).any() and (high[:, 0] < high[:, 1]).any()
    assert (c[980:1130] > 0).any()                                   # point boxes
    assert (c[1130:1190] > 0).all()                                  # slabs
    assert (c[-94:] == 0).all()                                      # far away, lo > hi, NaN and infinities


def test_count_equals_brute_force(api, base):
    assert scene_triangles(api, base.ds).tobytes() == base.tris.tobytes()
    got = run_count(api, base.ds, base.boxes)
    bad = np.nonzero(got[:base.n] != base.ref.counts)[0]
    assert len(bad) == 0, (len(bad), bad[:5], base.boxes[bad[:5]], got[bad[:5]], base.ref.counts[bad[:5]])


def test_fill_with_exact_offsets(api, base):
    """count, torch.cumsum, fill on one stream without a wait in between; then the same with d_written = NULL"""
    import torch
    n, total = base.n, int(base.offsets[-1])
    d_q = api.to_device(base.boxes)
    d_counts = base.ds.count_in_boxes_device(d_q, n)
    d_offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_offsets[1:] = torch.cumsum(d_counts, 0, dtype=torch.int64)
    got = run_fill(api, base.ds, base.boxes, d_offsets, total)       # (the buffers are sized from the reference: nothing is read back before)
    assert d_offsets.cpu().numpy().tobytes() == base.offsets.tobytes()
    want = expected_fill(base.ref.lists, base.offsets, total)
    assert_fill(got, want, "exact offsets")
    assert got[1][:n].tobytes() == base.ref.counts.tobytes()
    assert_fill(run_fill(api, base.ds, base.boxes, base.offsets, total, with_written=False), want, "no written")
    # a float32 [n, 6] tensor is a batch of queries as it stands
    d_f = torch.from_numpy(np.concatenate([base.boxes["lo"], base.boxes["hi"]], 1)).cuda()
    assert d_f.dtype == torch.float32 and d_f.shape == (n, 6)
    assert base.ds.count_in_boxes_device(d_f, n).cpu().numpy().view(np.uint32).tobytes() == base.ref.counts.tobytes()


@pytest.mark.parametrize("k", [0, 1, 3, 8])
def test_at_most_k(api, base, k):
    n = base.n
    offsets = np.arange(n + 1, dtype=np.int64) * k
    got = run_fill(api, base.ds, base.boxes, offsets, n * k)
    assert_fill(got, expected_fill(cut(base.ref.lists, k), offsets, n * k), "k = %d" % k)
    assert got[1][:n].tobytes() == np.minimum(base.ref.counts, k).astype(np.uint32).tobytes()


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
    got = run_fill(api, base.ds, base.boxes, offsets, total)
    want = expected_fill(kept, offsets, total)
    assert want[1][j] == 0
    assert_fill(got, want, "ragged")


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_sizes(api, base, n):
    which = np.arange(n) % base.n
    q = base.boxes[which]
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
        ref = brute_force_boxes(tris, np.arange(len(tris)), q["lo"], q["hi"])
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
    q = base.boxes
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
    ref = brute_force_boxes(moved.reshape(300, 3, 3), np.arange(300), q["lo"], q["hi"])
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
    on_chip = api.lib().rtk_amd_box_stack_entries()
    assert ds.info()["stack_entries"] > on_chip, (ds.info()["stack_entries"], on_chip)
    rng = np.random.RandomState(4)
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    ext = hi - lo
    a = lo + ext * rng.uniform(0, 1, (88, 3)) ** 8
    b = lo + ext * rng.uniform(0, 1, (88, 3)) ** 2
    blo = np.concatenate([np.tile(lo, (40, 1)), np.minimum(a, b)]).astype(np.float32)
    bhi = np.concatenate([np.tile(hi, (40, 1)), np.maximum(a, b)]).astype(np.float32)
    q = make_boxes(blo, bhi)
    n = len(q)
    assert n * len(tris) <= 500000
    own = scene_triangles(api, ds)
    ref = brute_force_boxes(own, np.arange(len(own)), q["lo"], q["hi"])
    assert (ref.counts[:40] == len(own)).all() and (ref.counts[40:] < len(own)).any()
    counts = run_count(api, ds, q)
    assert counts[:n].tobytes() == ref.counts.tobytes()
    offsets = np.arange(n + 1, dtype=np.int64) * 4
    want = expected_fill(cut(ref.lists, 4), offsets, n * 4)
    assert_fill(run_fill(api, ds, q, offsets, n * 4), want, "k = 4")
    # the counting forms say that pushes did go past the on-chip part, and give the same bytes
    d_q = api.to_device(q)
    d_counts, visits = ds.triangles_in_boxes_counted(d_q, n)
    print("geometric_chain: stack entries %d, on chip %d, count form %s" % (ds.info()["stack_entries"], on_chip, visits))
    assert visits["stack_spills"] > 0 and visits["rays"] == n and visits["hits"] == int((ref.counts > 0).sum())
    assert visits["triangles"] >= int(ref.counts.sum())
    assert d_counts.cpu().numpy().view(np.uint32).tobytes() == ref.counts.tobytes()
    d_prims = torch.full(((n * 4 + TAIL) * 4,), 0x7e, dtype=torch.uint8, device="cuda")
    d_wr = torch.full(((n + TAIL) * 4,), 0x7e, dtype=torch.uint8, device="cuda")
    _, fill_visits = ds.triangles_in_boxes_counted(d_q, n, torch.from_numpy(offsets).cuda(), d_prims, d_wr)
    print("geometric_chain: fill form k = 4 %s" % (fill_visits,))
    assert fill_visits == visits                                     # (the fill walks what the count walks: nothing kept can cull it)
    assert_fill((d_prims.cpu().numpy().view(np.uint32), d_wr.cpu().numpy().view(np.uint32)), want, "counted k = 4")
    assert api.lib().rtk_dev_trace_status(ds.handle, None) == 0


def test_lists(api, base):
    """A shuffled subset with repeated ids, the count on the device: listed slots as the unlisted call, the rest untouched"""
    n = 1000
    q = base.boxes[:n]
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
    # the fill: segments of 4 per slot, and exact offsets
    k4 = np.arange(n + 1, dtype=np.int64) * 4
    exact = base.offsets[:n + 1]
    for offsets, kept in ((k4, cut(lists, 4)), (exact, lists)):
        total = int(offsets[-1])
        assert_fill(run_fill(api, base.ds, q, offsets, total), expected_fill(kept, offsets, total), "all")
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


def test_two_launches_give_the_same_bytes_and_a_side_stream_sees_its_offsets(api, base):
    import torch
    n, total = base.n, int(base.offsets[-1])
    want = expected_fill(base.ref.lists, base.offsets, total)
    a = run_fill(api, base.ds, base.boxes, base.offsets, total)
    b = run_fill(api, base.ds, base.boxes, base.offsets, total)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert_fill(a, want, "first launch")
    # count, cumsum and fill enqueued on a side stream, nothing waited for in between
    d_q = api.to_device(base.boxes)
    d_prims = torch.full(((total + TAIL) * 4,), 0x7e, dtype=torch.uint8, device="cuda")
    d_wr = torch.full(((n + TAIL) * 4,), 0x7e, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_counts = base.ds.count_in_boxes_device(d_q, n)
        d_offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        d_offsets[1:] = torch.cumsum(d_counts, 0, dtype=torch.int64)
        base.ds.in_boxes_all_device(d_q, n, d_offsets, d_prims, d_wr)
        status_ok(api, base.ds)
    side.synchronize()
    assert_fill((d_prims.cpu().numpy().view(np.uint32), d_wr.cpu().numpy().view(np.uint32)), want, "side stream")


def test_python_conveniences(api, base):
    """triangles_in_boxes returns what the device forms computed, for 60 boxes; occupancy on a 4 x 4 x 4 grid equals brute-force
    counts over the same float32 linspace faces"""
    import torch
    pick = np.concatenate([np.arange(40), np.arange(500, 510), np.arange(1130, 1140)])
    lo, hi = base.boxes["lo"][pick], base.boxes["hi"][pick]
    counts = base.ref.counts[pick]
    lists = [base.ref.lists[i] for i in pick]
    assert counts.sum() > 100
    offsets, prims, written = base.ds.triangles_in_boxes(np.concatenate([lo, hi], 1))
    assert offsets.dtype == np.int64 and offsets.tobytes() == np.concatenate([[0], np.cumsum(counts.astype(np.int64))]).tobytes()
    assert prims.dtype == np.uint32 and written.dtype == np.uint32 and written.tobytes() == counts.tobytes()
    assert prims.tobytes() == np.concatenate(lists).astype(np.uint32).tobytes()
    offsets, prims, written = base.ds.triangles_in_boxes(base.boxes[pick], max_per_box=3)
    assert offsets.tolist() == list(range(0, 183, 3)) and written.tobytes() == np.minimum(counts, 3).astype(np.uint32).tobytes()
    for i, l in enumerate(cut(lists, 3)):
        assert prims[3 * i:3 * i + len(l)].tobytes() == l.tobytes() and not prims[3 * i + len(l):3 * i + 3].any()   # (beyond written: zero)
    o, p0, w0 = base.ds.triangles_in_boxes(np.zeros((0, 6), np.float32))
    assert o.tolist() == [0] and len(p0) == 0 and len(w0) == 0
    # the occupancy grid
    glo, ghi = base.tris.reshape(-1, 3).min(0), base.tris.reshape(-1, 3).max(0)
    occ = base.ds.occupancy(glo, ghi, (4, 4, 4))
    status_ok(api, base.ds)
    assert occ.dtype == torch.bool and tuple(occ.shape) == (4, 4, 4) and occ.is_cuda
    faces = [torch.linspace(float(glo[a]), float(ghi[a]), 5, dtype=torch.float32).numpy() for a in range(3)]
    blo = np.stack(np.meshgrid(faces[0][:-1], faces[1][:-1], faces[2][:-1], indexing="ij"), -1).reshape(-1, 3)
    bhi = np.stack(np.meshgrid(faces[0][1:], faces[1][1:], faces[2][1:], indexing="ij"), -1).reshape(-1, 3)
    ref = brute_force_boxes(base.tris, np.arange(300), blo, bhi)
    assert (occ.cpu().numpy().reshape(-1) == (ref.counts != 0)).all()
    # an uneven grid, fine enough for empty voxels
    occ = base.ds.occupancy(glo, ghi, (7, 3, 5))
    faces = [torch.linspace(float(glo[a]), float(ghi[a]), s + 1, dtype=torch.float32).numpy() for a, s in enumerate((7, 3, 5))]
    blo = np.stack(np.meshgrid(faces[0][:-1], faces[1][:-1], faces[2][:-1], indexing="ij"), -1).reshape(-1, 3)
    bhi = np.stack(np.meshgrid(faces[0][1:], faces[1][1:], faces[2][1:], indexing="ij"), -1).reshape(-1, 3)
    ref = brute_force_boxes(base.tris, np.arange(300), blo, bhi)
    assert tuple(occ.shape) == (7, 3, 5) and (occ.cpu().numpy().reshape(-1) == (ref.counts != 0)).all()
