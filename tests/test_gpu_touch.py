"""GPU tests of rtk_dev_triangles_touching_count / rtk_dev_triangles_touching_all. The bar everywhere: counts and ids are bit for
bit what numpy float32 brute force gives by the rule of rtk_amd/csrc/rtk_touch_rule.h (tests/touch_ref.py) over the triangle
records the scene holds at that moment -- read back through rtk_dev_expand_hits --, whatever tree is above them and whatever order
the walk takes. Every output is pre-filled with 0x7e and carries a tail; whole buffers are compared, so nothing may be written
beyond a query's kept entries, outside the segments or behind the batch; rtk_dev_trace_status is 0 after every call. The base
scene is the 300-triangle soup of tests/test_gpu_box.py; every brute force stays below half a million (query, triangle) pairs;
tests/test_touch_cpu.py checks what the query mix holds."""
import numpy as np
import pytest

from rtk_amd import synth
from tests.test_gpu_box import assert_fill, cut, expected_fill, list_tensors, status_ok
from tests.test_gpu_closest import FILL, TAIL, scene_triangles
from tests.touch_ref import brute_force_touching, mix_slices, query_mix

pytestmark = pytest.mark.gpu


def device_queries(api, q):
    import torch
    return api.to_device(np.ascontiguousarray(q, np.float32)) if len(q) else torch.zeros(36, dtype=torch.uint8, device="cuda")


def device_first(first):
    import torch
    return torch.from_numpy(np.ascontiguousarray(first, np.uint32).view(np.int32)).cuda() if first is not None else None


def run_count(api, ds, q, n=None, count=None, ids=None, first=None, skip_shared=False):
    """-> count words [n + TAIL] as the device left them"""
    import torch
    n = len(q) if n is None else n
    d_counts = torch.full(((n + TAIL) * 4,), 0x7e, dtype=torch.uint8, device="cuda")
    d_count, d_ids = list_tensors(count, ids)
    ds.count_touching_device(device_queries(api, q), n, d_counts, count=d_count, ids=d_ids, first_prim=device_first(first), skip_shared=skip_shared)
    status_ok(api, ds)
    got = d_counts.cpu().numpy().view(np.uint32)
    assert (got[n:] == FILL).all(), "written beyond num_queries"
    return got


def run_fill(api, ds, q, offsets, total, n=None, with_written=True, count=None, ids=None, first=None, skip_shared=False):
    """offsets: numpy int64 [n + 1] or a cuda tensor; total: ids the segments span. -> (id words [total + TAIL], written words
    [n + TAIL] or None) as the device left them"""
    import torch
    n = len(q) if n is None else n
    d_off = offsets if isinstance(offsets, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(offsets, np.int64)).cuda()
    d_prims = torch.full(((total + TAIL) * 4,), 0x7e, dtype=torch.uint8, device="cuda")
    d_wr = torch.full(((n + TAIL) * 4,), 0x7e, dtype=torch.uint8, device="cuda") if with_written else None
    d_count, d_ids = list_tensors(count, ids)
    ds.touching_all_device(device_queries(api, q), n, d_off, d_prims, d_wr, count=d_count, ids=d_ids, first_prim=device_first(first), skip_shared=skip_shared)
    status_ok(api, ds)
    return d_prims.cpu().numpy().view(np.uint32), d_wr.cpu().numpy().view(np.uint32) if with_written else None


@pytest.fixture(scope="module")
def base(api):
    class Base:
        pass
    b = Base()
    b.positions = synth.triangle_soup(300, 0.2, seed=5)
    b.tris = b.positions.reshape(300, 3, 3)
    b.ds = api.DeviceScene.build([dict(positions=b.positions)])
    b.q = query_mix(b.tris)
    b.n = len(b.q)
    # the reference, computed once and shared
    b.ref = brute_force_touching(b.tris, np.arange(300), b.q)
    b.offsets = np.concatenate([[0], np.cumsum(b.ref.counts.astype(np.int64))])
    return b


def test_count_equals_brute_force(api, base):
    assert scene_triangles(api, base.ds).tobytes() == base.tris.tobytes()
    assert base.ds.triangles().cpu().numpy().tobytes() == base.tris.tobytes()
    got = run_count(api, base.ds, base.q)
    bad = np.nonzero(got[:base.n] != base.ref.counts)[0]
    assert len(bad) == 0, (len(bad), bad[:5], base.q[bad[:5]], got[bad[:5]], base.ref.counts[bad[:5]])
    part = mix_slices()
    assert (got[part["huge and degenerate on purpose"]] == 300).any() and (got[part["not live"]] == 0).all()


@pytest.mark.parametrize("with_written", [True, False])
def test_fill_with_exact_offsets(api, base, with_written):
    """count, torch.cumsum, fill on one stream without a wait in between, with d_written and with NULL"""
    import torch
    n, total = base.n, int(base.offsets[-1])
    d_q = device_queries(api, base.q)
    d_counts = base.ds.count_touching_device(d_q, n)
    d_offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_offsets[1:] = torch.cumsum(d_counts, 0, dtype=torch.int64)
    got = run_fill(api, base.ds, base.q, d_offsets, total, with_written=with_written)   # (sized from the reference: nothing is read back before)
    assert d_offsets.cpu().numpy().tobytes() == base.offsets.tobytes()
    assert_fill(got, expected_fill(base.ref.lists, base.offsets, total), "exact offsets")
    if with_written:
        assert got[1][:n].tobytes() == base.ref.counts.tobytes()
    # a float32 [n, 3, 3] tensor is a batch of queries as it stands
    d_f = torch.from_numpy(base.q).cuda()
    assert d_f.dtype == torch.float32 and d_f.shape == (n, 3, 3)
    assert base.ds.count_touching_device(d_f, n).cpu().numpy().view(np.uint32).tobytes() == base.ref.counts.tobytes()


@pytest.mark.parametrize("k", [0, 1, 3, 8])
def test_at_most_k(api, base, k):
    n = base.n
    offsets = np.arange(n + 1, dtype=np.int64) * k
    got = run_fill(api, base.ds, base.q, offsets, n * k)
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
    got = run_fill(api, base.ds, base.q, offsets, total)
    want = expected_fill(kept, offsets, total)
    assert want[1][j] == 0
    assert_fill(got, want, "ragged")


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_sizes(api, base, n):
    which = (np.arange(n) * 7) % base.n                              # (a stride: every part of the mix at every size)
    q = base.q[which]
    got = run_count(api, base.ds, q, n=n)
    assert got[:n].tobytes() == base.ref.counts[which].tobytes()
    offsets = np.arange(n + 1, dtype=np.int64) * 3
    kept = cut([base.ref.lists[i] for i in which], 3)
    assert_fill(run_fill(api, base.ds, q, offsets, n * 3, n=n), expected_fill(kept, offsets, n * 3), "n = %d" % n)


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
    # the fill: segments of 4 per slot, and exact offsets
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


def test_two_launches_give_the_same_bytes_and_a_side_stream_sees_its_offsets(api, base):
    import torch
    n, total = base.n, int(base.offsets[-1])
    want = expected_fill(base.ref.lists, base.offsets, total)
    a = run_fill(api, base.ds, base.q, base.offsets, total)
    b = run_fill(api, base.ds, base.q, base.offsets, total)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert_fill(a, want, "first launch")
    # count, cumsum and fill enqueued on a side stream, nothing waited for in between
    d_q = device_queries(api, base.q)
    d_prims = torch.full(((total + TAIL) * 4,), 0x7e, dtype=torch.uint8, device="cuda")
    d_wr = torch.full(((n + TAIL) * 4,), 0x7e, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_counts = base.ds.count_touching_device(d_q, n)
        d_offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        d_offsets[1:] = torch.cumsum(d_counts, 0, dtype=torch.int64)
        base.ds.touching_all_device(d_q, n, d_offsets, d_prims, d_wr)
        status_ok(api, base.ds)
    side.synchronize()
    assert_fill((d_prims.cpu().numpy().view(np.uint32), d_wr.cpu().numpy().view(np.uint32)), want, "side stream")


def check_scene(api, ds, q, ref=None):
    """count, exact fill and k = 3 fill of one scene against brute force over its own records; returns the bytes of all three"""
    n = len(q)
    if ref is None:
        tris = scene_triangles(api, ds)
        ref = brute_force_touching(tris, np.arange(len(tris)), q)
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
    moved = (base.positions + rng.uniform(-0.05, 0.05, base.positions.shape)).astype(np.float32)
    ds.refit([dict(positions=moved)])
    assert scene_triangles(api, ds).tobytes() == moved.tobytes()
    ref = brute_force_touching(moved.reshape(300, 3, 3), np.arange(300), q)
    after_refit = check_scene(api, ds, q, ref)
    assert after_refit != first
    ds.rebuild()
    assert scene_triangles(api, ds).tobytes() == moved.tobytes()
    assert check_scene(api, ds, q, ref) == after_refit


def test_a_stack_deeper_than_the_on_chip_part(api):
    """The geometric cluster of tests/test_gpu_build.py: a deep, lopsided tree; query triangles that span much of it make the walk
    push past the on-chip part"""
    import torch
    from tests.test_gpu_build import _adversarial_scenes
    tris = _adversarial_scenes()["geometric_chain"]
    ds = api.DeviceScene.build([dict(positions=tris.reshape(-1, 3))])
    on_chip = api.lib().rtk_amd_touch_stack_entries()
    assert ds.info()["stack_entries"] > on_chip, (ds.info()["stack_entries"], on_chip)
    rng = np.random.RandomState(4)
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    ext = hi - lo
    # 40 segments along the scene's diagonal and beyond it (their box is the scene's or more), 88 triangles with vertices
    # anywhere in the scene, crowded towards the corner the chain converges on
    t = rng.uniform(1, 4, (40, 1))
    spans = np.stack([lo - t * ext, hi + t * ext, hi + t * ext], 1)
    anywhere = lo + ext * rng.uniform(0, 1, (88, 3, 3)) ** rng.choice([1, 2, 8], (88, 3, 1))
    q = np.concatenate([spans, anywhere]).astype(np.float32)
    n = len(q)
    assert n * len(tris) <= 500000
    own = scene_triangles(api, ds)
    ref = brute_force_touching(own, np.arange(len(own)), q)
    assert (ref.counts > 0).any() and (ref.counts == 0).any()
    counts = run_count(api, ds, q)
    assert counts[:n].tobytes() == ref.counts.tobytes()
    offsets = np.arange(n + 1, dtype=np.int64) * 4
    want = expected_fill(cut(ref.lists, 4), offsets, n * 4)
    assert_fill(run_fill(api, ds, q, offsets, n * 4), want, "k = 4")
    # the counting forms say that pushes did go past the on-chip part, and give the same bytes
    d_q = device_queries(api, q)
    d_counts, visits = ds.triangles_touching_counted(d_q, n)
    print("geometric_chain: stack entries %d, on chip %d, count form %s" % (ds.info()["stack_entries"], on_chip, visits))
    assert visits["stack_spills"] > 0 and visits["rays"] == n and visits["hits"] == int((ref.counts > 0).sum())
    assert visits["triangles"] >= int(ref.counts.sum())
    assert d_counts.cpu().numpy().view(np.uint32).tobytes() == ref.counts.tobytes()
    d_prims = torch.full(((n * 4 + TAIL) * 4,), 0x7e, dtype=torch.uint8, device="cuda")
    d_wr = torch.full(((n + TAIL) * 4,), 0x7e, dtype=torch.uint8, device="cuda")
    _, fill_visits = ds.triangles_touching_counted(d_q, n, torch.from_numpy(offsets).cuda(), d_prims, d_wr)
    assert fill_visits == visits                                     # (the fill walks what the count walks: nothing kept can cull it)
    assert_fill((d_prims.cpu().numpy().view(np.uint32), d_wr.cpu().numpy().view(np.uint32)), want, "counted k = 4")
    assert api.lib().rtk_dev_trace_status(ds.handle, None) == 0


def torus(nu=10, nv=10, R=1.0, r=0.4):
    """A closed mesh of 2 nu nv triangles whose neighbours share vertex positions bit for bit: [2 nu nv, 3, 3] float32"""
    u, v = np.meshgrid(np.arange(nu) * (2 * np.pi / nu), np.arange(nv) * (2 * np.pi / nv), indexing="ij")
    p = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], -1).astype(np.float32)
    tris = []
    for i in range(nu):
        for j in range(nv):
            a, b, c, d = p[i, j], p[(i + 1) % nu, j], p[(i + 1) % nu, (j + 1) % nv], p[i, (j + 1) % nv]
            tris += [[a, b, c], [a, c, d]]
    return np.array(tris, np.float32)


@pytest.fixture(scope="module")
def pierced(api):
    """One closed mesh of 200 triangles with shared vertices plus 20 triangles that pierce it"""
    class Scene:
        pass
    s = Scene()
    rng = np.random.RandomState(12)
    mesh = torus()
    ang = rng.uniform(0, 2 * np.pi, 20)
    centre = np.stack([np.cos(ang), np.sin(ang), np.zeros(20)], 1)           # on the tube's centre line
    blades = centre[:, None, :] + rng.uniform(-0.7, 0.7, (20, 3, 3))
    s.tris = np.concatenate([mesh, blades]).astype(np.float32)
    s.T = len(s.tris)
    s.ds = api.DeviceScene.build([dict(positions=s.tris.reshape(-1, 3))])
    return s


def test_the_filter_gives_each_self_intersecting_pair_once(api, pierced):
    s = pierced
    own = scene_triangles(api, s.ds)
    assert own.tobytes() == s.tris.tobytes() and s.T == 220
    ids = np.arange(s.T)
    # without the filter every triangle lists itself and its neighbours
    plain = brute_force_touching(own, ids, own)
    shares = (own[:, None, :, None, :] == own[None, :, None, :, :]).all(-1).any((-1, -2))     # [T, T]: a common vertex position
    for i in range(s.T):
        assert i in plain.lists[i] and set(np.nonzero(shares[i])[0]) <= set(plain.lists[i].tolist())
    assert (shares[:200].sum(1) >= 12).all()                                  # (a torus vertex is shared by six triangles)
    assert run_count(api, s.ds, own)[:s.T].tobytes() == plain.counts.tobytes()
    off = np.concatenate([[0], np.cumsum(plain.counts.astype(np.int64))])
    assert_fill(run_fill(api, s.ds, own, off, int(off[-1])), expected_fill(plain.lists, off, int(off[-1])), "no filter")
    # the unordered non-adjacent meeting pairs, from the unfiltered brute force
    pairs = sorted((i, int(j)) for i in range(s.T) for j in plain.lists[i] if j > i and not shares[i, j])
    assert len(pairs) >= 20
    assert any(i < 200 <= j for i, j in pairs)                                # a blade through the mesh
    first = ids + 1
    ref = brute_force_touching(own, ids, own, first, 1)
    assert sorted((i, int(j)) for i in range(s.T) for j in ref.lists[i]) == pairs
    assert run_count(api, s.ds, own, first=first, skip_shared=True)[:s.T].tobytes() == ref.counts.tobytes()
    off = np.concatenate([[0], np.cumsum(ref.counts.astype(np.int64))])
    got = run_fill(api, s.ds, own, off, int(off[-1]), first=first, skip_shared=True)
    assert_fill(got, expected_fill(ref.lists, off, int(off[-1])), "skip_shared, first_prim = id + 1")
    # either part of the filter alone, and a first_prim at, below and above a candidate's id
    for fl, fp in ((0, first), (1, None)):
        ref = brute_force_touching(own, ids, own, fp, fl)
        assert run_count(api, s.ds, own, first=fp, skip_shared=bool(fl))[:s.T].tobytes() == ref.counts.tobytes()
    for shift in (-1, 0, 1):
        fp = np.array([max(int(l[len(l) // 2]) + shift, 0) for l in plain.lists], np.uint32)
        ref = brute_force_touching(own, ids, own, fp, 0)
        k2 = np.arange(s.T + 1, dtype=np.int64) * 2
        assert_fill(run_fill(api, s.ds, own, k2, s.T * 2, first=fp), expected_fill(cut(ref.lists, 2), k2, s.T * 2), "first_prim %+d" % shift)
    # the counted form takes the filter too
    d_counts, visits = s.ds.triangles_touching_counted(device_queries(api, own), s.T, first_prim=device_first(first), skip_shared=True)
    assert visits["rays"] == s.T and visits["hits"] == len(set(i for i, _ in pairs))
    # the convenience
    got = s.ds.self_intersections()
    status_ok(api, s.ds)
    assert got.dtype.is_floating_point is False and tuple(got.shape) == (len(pairs), 2) and got.is_cuda
    assert [tuple(x) for x in got.cpu().numpy().tolist()] == pairs


def test_python_conveniences(api, base, pierced):
    """triangles_touching returns what the device forms computed; intersections between two small scenes equals brute force"""
    import torch
    part = mix_slices()
    pick = np.concatenate([np.arange(40), np.arange(part["the scene's own"].start, part["the scene's own"].start + 10),
                           np.arange(part["huge and degenerate on purpose"].start, part["huge and degenerate on purpose"].stop)])
    q = base.q[pick]
    counts = base.ref.counts[pick]
    lists = [base.ref.lists[i] for i in pick]
    assert counts.sum() > 300
    offsets, prims, written = base.ds.triangles_touching(q)
    assert offsets.dtype == np.int64 and offsets.tobytes() == np.concatenate([[0], np.cumsum(counts.astype(np.int64))]).tobytes()
    assert prims.dtype == np.uint32 and written.dtype == np.uint32 and written.tobytes() == counts.tobytes()
    assert prims.tobytes() == np.concatenate(lists).astype(np.uint32).tobytes()
    offsets, prims, written = base.ds.triangles_touching(q.reshape(-1, 9), max_per_tri=3)
    assert offsets.tolist() == list(range(0, 3 * len(pick) + 1, 3)) and written.tobytes() == np.minimum(counts, 3).astype(np.uint32).tobytes()
    for i, l in enumerate(cut(lists, 3)):
        assert prims[3 * i:3 * i + len(l)].tobytes() == l.tobytes() and not prims[3 * i + len(l):3 * i + 3].any()   # (beyond written: zero)
    first = np.full(len(pick), 150, np.uint32)
    ref = brute_force_touching(base.tris, np.arange(300), q, first, 1)
    offsets, prims, written = base.ds.triangles_touching(q, first_prim=first, skip_shared=True)
    assert written.tobytes() == ref.counts.tobytes() and prims.tobytes() == np.concatenate(ref.lists).astype(np.uint32).tobytes()
    o, p0, w0 = base.ds.triangles_touching(np.zeros((0, 9), np.float32))
    assert o.tolist() == [0] and len(p0) == 0 and len(w0) == 0
    # one body's triangles against another body's scene: (prim of other, prim of self), ascending
    ref = brute_force_touching(base.tris, np.arange(300), pierced.tris)
    want = [(i, int(j)) for i in range(pierced.T) for j in ref.lists[i]]
    got = base.ds.intersections(pierced.ds)
    status_ok(api, base.ds)
    assert got.dtype == torch.int64 and got.is_cuda and tuple(got.shape) == (len(want), 2) and len(want) > 20
    assert [tuple(x) for x in got.cpu().numpy().tolist()] == want
    back = pierced.ds.intersections(base.ds)
    ref = brute_force_touching(pierced.tris, np.arange(pierced.T), base.tris)
    assert [tuple(x) for x in back.cpu().numpy().tolist()] == [(i, int(j)) for i in range(300) for j in ref.lists[i]]
    # a scene far from the other: no pairs
    far = api.DeviceScene.build([dict(positions=(base.positions + np.float32(1e4)))])
    assert tuple(base.ds.intersections(far).shape) == (0, 2)
