"""GPU tests of rtk_dev_triangles_near_count / rtk_dev_triangles_near_all. The bar everywhere: counts, records and both point
arrays are bit for bit what numpy float32 brute force gives by the rules of rtk_amd/csrc/rtk_pair_rule.h and rtk_near_rule.h
(tests/near_ref.py) over the triangle records the scene holds at that moment, whatever tree is above them and whatever order
the walk takes. Every output is pre-filled with 0x7e and carries a tail; whole buffers are compared, so nothing may be written
beyond a query's kept entries, outside the segments or behind the batch; rtk_dev_trace_status is 0 after every call. The base
scene is the 300-triangle soup of tests/test_gpu_pair.py and its query mix without the huge members; every brute force stays
below half a million (query, triangle) pairs. No tolerance anywhere."""
import numpy as np
import pytest

from rtk_amd import synth
from rtk_amd.types import RTK_INF
from tests.near_ref import brute_force_near
from tests.pair_ref import FEATURE_PIERCE, pair_np
from tests.test_gpu_box import list_tensors, status_ok
from tests.test_gpu_closest import FILL, TAIL, scene_triangles
from tests.test_gpu_touch import device_first, device_queries, torus
from tests.touch_ref import mix_slices, query_mix

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF


def filled(words, width):
    import torch
    return torch.full((words * width * 4,), 0x7e, dtype=torch.uint8, device="cuda")


def device_limits(max2):
    import torch
    return torch.from_numpy(np.ascontiguousarray(max2, np.float32)).cuda() if max2 is not None else None


def run_count(api, ds, q, n=None, max2=None, count=None, ids=None, first=None, skip_shared=False):
    """-> count words [n + TAIL] as the device left them"""
    n = len(q) if n is None else n
    d_counts = filled(n + TAIL, 1)
    d_count, d_ids = list_tensors(count, ids)
    ds.count_near_device(device_queries(api, q), n, d_counts, max_dist2=device_limits(max2), count=d_count, ids=d_ids, first_prim=device_first(first),
                         skip_shared=skip_shared)
    status_ok(api, ds)
    return d_counts.cpu().numpy().view(np.uint32)


def run_fill(api, ds, q, offsets, total, n=None, max2=None, points=(True, True), with_written=True, count=None, ids=None, first=None, skip_shared=False):
    """offsets: numpy int64 [n + 1] or a cuda tensor; total: records the segments span. -> (record words [total + TAIL, 4], words
    of the points on the query [total + TAIL, 3] or None, on the scene or None, written words [n + TAIL] or None)"""
    import torch
    n = len(q) if n is None else n
    d_off = offsets if isinstance(offsets, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(offsets, np.int64)).cuda()
    d_rec = filled(total + TAIL, 4)
    d_pts = [filled(total + TAIL, 3) if want else None for want in points]
    d_wr = filled(n + TAIL, 1) if with_written else None
    d_count, d_ids = list_tensors(count, ids)
    ds.near_all_device(device_queries(api, q), n, d_off, d_rec, d_pts[0], d_pts[1], d_wr, max_dist2=device_limits(max2), count=d_count, ids=d_ids,
                       first_prim=device_first(first), skip_shared=skip_shared)
    status_ok(api, ds)
    return (d_rec.cpu().numpy().view(np.uint32).reshape(-1, 4),) + tuple(d.cpu().numpy().view(np.uint32).reshape(-1, 3) if d is not None else None for d in d_pts) + \
        (d_wr.cpu().numpy().view(np.uint32) if with_written else None,)


def expected_fill(kept, offsets, total, listed=None):
    """The whole output as it must stand: the first `room` entries of kept[i] at offsets[i] for every (listed) query, 0x7e
    everywhere else"""
    n = len(kept)
    rec = np.full((total + TAIL, 4), FILL, np.uint32)
    pa = np.full((total + TAIL, 3), FILL, np.uint32)
    pb = np.full((total + TAIL, 3), FILL, np.uint32)
    wr = np.full(n + TAIL, FILL, np.uint32)
    for i in range(n):
        if listed is not None and not listed[i]:
            continue
        room = max(0, int(offsets[i + 1]) - int(offsets[i]))
        k = min(len(kept[i][0]), room)
        for dst, src in zip((rec, pa, pb), kept[i]):
            dst[offsets[i]:offsets[i] + k] = src[:k]
        wr[i] = k
    return rec, pa, pb, wr


def expected_counts(counts, listed=None):
    want = np.full(len(counts) + TAIL, FILL, np.uint32)
    rows = np.ones(len(counts), bool) if listed is None else listed
    want[:len(counts)][rows] = counts[rows]
    return want


def assert_fill(got, want, what=""):
    for g, w, name in zip(got, want, ("records", "points on the query", "points on the scene", "written")):
        if g is None:
            continue
        if g.tobytes() != w.tobytes():
            bad = np.nonzero((g != w).reshape(len(g), -1).any(1))[0]
            raise AssertionError("%s %s: %d rows differ, first %s: got %s want %s" % (what, name, len(bad), bad[:5], g[bad[:3]], w[bad[:3]]))


def limits(rng, n, scale):
    """one squared limit per query, as tests/test_gpu_pair.py draws them: some none, some tight, and the entries that make an
    empty list"""
    max2 = (rng.choice([0.02, 0.1, 0.5, 2.0], n) * scale).astype(np.float32) ** 2
    max2[::4] = RTK_INF
    max2[1::16] = np.tile(np.array([0.0, -0.0, -1.0, np.nan, -np.inf, 1e-45], np.float32), n // 16 + 1)[:len(max2[1::16])]
    return max2


@pytest.fixture(scope="module")
def base(api):
    class Base:
        pass
    b = Base()
    b.positions = synth.triangle_soup(300, 0.2, seed=5)
    b.tris = b.positions.reshape(300, 3, 3)
    b.ds = api.DeviceScene.build([dict(positions=b.positions)])
    part = mix_slices()
    huge = part["huge and degenerate on purpose"]
    mix = query_mix(b.tris)
    b.q = np.concatenate([mix[:huge.start], mix[huge.stop:]])
    b.n = len(b.q)
    assert b.n * 300 <= 500000
    b.max2 = limits(np.random.RandomState(3), b.n, 0.2)
    # the references, computed once and shared: with the limits, all queries; without, a subset (a NULL limit counts the whole
    # filtered scene)
    b.ref = brute_force_near(b.tris, np.arange(300), b.q, b.max2)
    b.offsets = np.concatenate([[0], np.cumsum(b.ref.counts.astype(np.int64))])
    b.some = np.arange(0, b.n, 11)
    b.ref_inf = brute_force_near(b.tris, np.arange(300), b.q[b.some])
    return b


def test_the_reference_has_empty_single_long_and_pierced_lists(base):
    """Asserted on the CPU result before any GPU comparison"""
    c = base.ref.counts
    pierced2 = sum(1 for r, _, _ in base.ref.kept if len(r) >= 2 and r[0, 0] == 0 and r[1, 0] == 0)
    print("queries %d, pairs %d, mean count %.1f, max %d, empty %d, single %d, more than 16: %d, two pierced in front: %d"
          % (base.n, int(c.sum()), c.mean(), c.max(), (c == 0).sum(), (c == 1).sum(), (c > 16).sum(), pierced2))
    assert (c == 0).any() and (c == 1).any() and (c > 16).any() and pierced2 > 0
    # those leading entries are pierced pairs by the rule, in ascending ids
    i = next(i for i, (r, _, _) in enumerate(base.ref.kept) if len(r) >= 2 and r[0, 0] == 0 and r[1, 0] == 0 and
             (pair_np(base.q[i].reshape(1, 3, 3), base.tris[r[:2, 3]]).feature >= FEATURE_PIERCE).all())
    assert base.ref.kept[i][0][0, 3] < base.ref.kept[i][0][1, 3]
    # a live query without a limit has the whole scene as its list; a limit that is not > 0 has none
    live = np.isfinite(base.q.reshape(base.n, 9)).all(1)
    assert (base.ref_inf.counts[live[base.some]] == 300).all() and (base.ref_inf.counts[~live[base.some]] == 0).all() and (~live[base.some]).any()
    with np.errstate(invalid="ignore"):
        assert (c[~(base.max2 > 0)] == 0).all() and (~(base.max2 > 0)).sum() > 50


def test_count_equals_brute_force(api, base):
    assert scene_triangles(api, base.ds).tobytes() == base.tris.tobytes()
    got = run_count(api, base.ds, base.q, max2=base.max2)
    assert got.tobytes() == expected_counts(base.ref.counts).tobytes(), np.nonzero(got[:base.n] != base.ref.counts)[0][:10]
    got = run_count(api, base.ds, base.q[base.some])
    assert got.tobytes() == expected_counts(base.ref_inf.counts).tobytes()
    # RTK_INF in every entry is the call without the array
    got = run_count(api, base.ds, base.q[base.some], max2=np.full(len(base.some), RTK_INF, np.float32))
    assert got.tobytes() == expected_counts(base.ref_inf.counts).tobytes()


def test_fill_with_exact_offsets(api, base):
    """count, torch.cumsum, fill on one stream without a wait in between; then with either point array alone and with none"""
    import torch
    n, total = base.n, int(base.offsets[-1])
    d_q, d_max = device_queries(api, base.q), device_limits(base.max2)
    d_counts = base.ds.count_near_device(d_q, n, max_dist2=d_max)
    d_offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    d_offsets[1:] = torch.cumsum(d_counts, 0, dtype=torch.int64)
    got = run_fill(api, base.ds, base.q, d_offsets, total, max2=base.max2)     # (the buffers are sized from the reference: nothing is read back before)
    assert d_offsets.cpu().numpy().tobytes() == base.offsets.tobytes()
    want = expected_fill(base.ref.kept, base.offsets, total)
    assert_fill(got, want, "exact offsets")
    assert got[3][:n].tobytes() == base.ref.counts.tobytes()
    for points in ((True, False), (False, True), (False, False)):
        assert_fill(run_fill(api, base.ds, base.q, base.offsets, total, max2=base.max2, points=points), want, "points %s" % (points,))
    assert_fill(run_fill(api, base.ds, base.q, base.offsets, total, max2=base.max2, with_written=False), want, "no written")


def closest(api, ds, q, max2):
    """rtk_dev_closest_triangles' three outputs as words"""
    n = len(q)
    d_rec, d_pq, d_ps = ds.closest_triangles_device(device_queries(api, q), n, max_dist2=device_limits(max2))
    status_ok(api, ds)
    return d_rec.cpu().numpy().view(np.uint32).reshape(n, 4), d_pq.cpu().numpy().view(np.uint32).reshape(n, 3), d_ps.cpu().numpy().view(np.uint32).reshape(n, 3)


@pytest.mark.parametrize("k", [0, 1, 3, 8])
def test_k_nearest(api, base, k):
    for q, max2, ref, what in ((base.q, base.max2, base.ref, "limits"), (base.q[base.some], None, base.ref_inf, "no limit")):
        n = len(q)
        offsets = np.arange(n + 1, dtype=np.int64) * k
        got = run_fill(api, base.ds, q, offsets, n * k, max2=max2)
        assert_fill(got, expected_fill(ref.kept, offsets, n * k), "k = %d, %s" % (k, what))
        assert got[3][:n].tobytes() == np.minimum(ref.counts, k).astype(np.uint32).tobytes()
        if k == 0:
            continue
        # the first entry is word for word what closest triangles writes; its miss goes with an empty segment
        c_rec, c_pq, c_ps = closest(api, base.ds, q, max2)
        some = got[3][:n] > 0
        assert ((c_rec[:, 3] == NONE) == ~some).all() and some.any() and (~some).any()
        assert got[0][:n * k].reshape(n, k, 4)[some, 0].tobytes() == c_rec[some].tobytes()
        assert got[1][:n * k].reshape(n, k, 3)[some, 0].tobytes() == c_pq[some].tobytes()
        assert got[2][:n * k].reshape(n, k, 3)[some, 0].tobytes() == c_ps[some].tobytes()


def test_ragged_room(api, base):
    """Room 0, short, exact and over-long per query, and pairs of decreasing offsets: the kept prefix, nothing for a query
    without room"""
    rng = np.random.RandomState(9)
    n = base.n
    c = base.ref.counts.astype(np.int64)
    kind = rng.randint(0, 4, n)
    room = np.where(kind == 0, 0, np.where(kind == 1, c // 2, np.where(kind == 2, c, c + rng.randint(1, 5, n))))
    starts = np.concatenate([[0], np.cumsum(room)])
    total = int(starts[-1])
    assert ((room < c) & (room > 0)).any() and ((room == c) & (c > 0)).any() and (room > c).any() and ((room == 0) & (c > 0)).any()
    got = run_fill(api, base.ds, base.q, starts, total, max2=base.max2)
    assert_fill(got, expected_fill(base.ref.kept, starts, total), "ragged")
    # decreasing offsets: no room, d_written = 0, nothing written
    off = starts.copy()
    # (offsets are shared between neighbours: the query behind such a pair is one with an empty list, which writes nothing
    # whatever room the lowered offset seems to give it)
    down = np.nonzero((c[:-1] > 0) & (room[:-1] > 0) & (c[1:] == 0) & (starts[:-2] >= 1))[0][:5]
    off[down + 1] = off[down] - 1
    assert len(down) == 5 and (off[down + 1] < off[down]).all() and (off >= 0).all()
    got = run_fill(api, base.ds, base.q, off, total, max2=base.max2)
    want = expected_fill(base.ref.kept, off, total)
    assert (want[3][down] == 0).all()
    assert_fill(got, want, "decreasing offsets")


def test_ties(api, base):
    """The whole scene once more under the ids 300 .. 599: every dist2 stands under two ids, the lower comes first, and a full
    segment whose worst entry ties a later candidate of lower id takes it (whichever the walk meets first)"""
    twice = np.concatenate([base.tris, base.tris])
    ds = api.DeviceScene.build([dict(positions=twice.reshape(-1, 3))])
    own = scene_triangles(api, ds)
    assert own.tobytes() == twice.tobytes()
    pick = np.arange(0, base.n, 2)[:800]
    q, max2 = base.q[pick], base.max2[pick]
    assert len(q) * 600 <= 500000
    ref = brute_force_near(own, np.arange(600), q, max2)
    n = len(q)
    full = [r for r, _, _ in ref.kept if len(r)]
    for r in full:
        at = {int(p): j for j, p in enumerate(r[:, 3])}
        assert len(r) % 2 == 0 and all(p + 300 in at and at[p] < at[p + 300] and r[at[p], 0] == r[at[p + 300], 0] for p in at if p < 300)
    for k in (1, 3):
        # (an odd k cuts every list of k + 1 or more entries between two equal dist2: the entry kept is the lower id)
        offsets = np.arange(n + 1, dtype=np.int64) * k
        assert sum(1 for r in full if len(r) > k and r[k - 1, 0] == r[k, 0]) > 100
        got = run_fill(api, ds, q, offsets, n * k, max2=max2)
        assert_fill(got, expected_fill(ref.kept, offsets, n * k), "ties, k = %d" % k)
    got = run_count(api, ds, q, max2=max2)
    assert got.tobytes() == expected_counts(ref.counts).tobytes()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_sizes(api, base, n):
    which = (np.arange(n) * 7) % base.n                              # (a stride: every part of the mix at every size)
    q = base.q[which]
    max2 = base.max2[which] if n else np.zeros(1, np.float32)
    counts = base.ref.counts[which]
    kept = [base.ref.kept[i] for i in which]
    got = run_count(api, base.ds, q, n=n, max2=max2)
    assert got.tobytes() == expected_counts(counts).tobytes()
    offsets = np.arange(n + 1, dtype=np.int64) * 3
    assert_fill(run_fill(api, base.ds, q, offsets, n * 3, n=n, max2=max2), expected_fill(kept, offsets, n * 3), "n = %d" % n)


def both_forms(api, ds, q, max2, ref, k=8):
    """count and the k nearest of every query against ref -> all bytes"""
    n = len(q)
    counts = run_count(api, ds, q, max2=max2)
    assert counts.tobytes() == expected_counts(ref.counts).tobytes()
    offsets = np.arange(n + 1, dtype=np.int64) * k
    got = run_fill(api, ds, q, offsets, n * k, max2=max2)
    assert_fill(got, expected_fill(ref.kept, offsets, n * k), "scene")
    return counts.tobytes() + b"".join(x.tobytes() for x in got)


def test_the_tree_does_not_matter(api, base):
    """A device build, that scene after split_leaves and after a rebuild, and the CPU task builder's blob uploaded (leaves of 4
    to 63, loose boxes): the same bytes"""
    L = api.lib()
    q, max2 = base.q, base.max2
    first = both_forms(api, base.ds, q, max2, base.ref)
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
    assert scene_triangles(api, up).tobytes() == base.tris.tobytes()         # (the blob keeps the input's vertex order)
    assert both_forms(api, up, q, max2, base.ref) == first
    split = up.split_leaves()
    assert split["leaves_split"] > 0
    assert both_forms(api, up, q, max2, base.ref) == first
    up.rebuild()
    assert scene_triangles(api, up).tobytes() == base.tris.tobytes()
    assert both_forms(api, up, q, max2, base.ref) == first


def test_a_stack_deeper_than_the_on_chip_part(api):
    """The geometric cluster of tests/test_gpu_build.py: a deep, lopsided tree. A count without a limit visits all of it and
    keeps every level's sibling on the stack"""
    import torch
    from tests.test_gpu_build import _adversarial_scenes
    tris = _adversarial_scenes()["geometric_chain"]
    ds = api.DeviceScene.build([dict(positions=tris.reshape(-1, 3))])
    on_chip = api.lib().rtk_amd_near_stack_entries()
    assert ds.info()["stack_entries"] > on_chip, (ds.info()["stack_entries"], on_chip)
    rng = np.random.RandomState(4)
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    ext = hi - lo
    t = rng.uniform(1, 4, (40, 1))
    spans = np.stack([lo - t * ext, hi + t * ext, hi + t * ext], 1)
    anywhere = lo + ext * rng.uniform(0, 1, (88, 3, 3)) ** rng.choice([1, 2, 8], (88, 3, 1))
    q = np.concatenate([spans, anywhere]).astype(np.float32)
    n, k = len(q), 4
    assert n * len(tris) <= 500000
    own = scene_triangles(api, ds)
    ref = brute_force_near(own, np.arange(len(own)), q)
    assert (ref.counts == len(own)).all()
    assert run_count(api, ds, q).tobytes() == expected_counts(ref.counts).tobytes()
    offsets = np.arange(n + 1, dtype=np.int64) * k
    want = expected_fill(ref.kept, offsets, n * k)
    assert_fill(run_fill(api, ds, q, offsets, n * k), want, "deep tree")
    # the counted forms: the same bytes, and the stack did go past the on-chip part
    d_q = device_queries(api, q)
    d_counts = filled(n + TAIL, 1)
    _, visits = ds.near_counted(d_q, n, d_counts=d_counts)
    print("geometric_chain: stack entries %d, on chip %d, count form %s" % (ds.info()["stack_entries"], on_chip, visits))
    assert visits["stack_spills"] > 0 and visits["rays"] == n and visits["hits"] == n and visits["triangles"] == n * len(own)
    assert d_counts.cpu().numpy().view(np.uint32).tobytes() == expected_counts(ref.counts).tobytes()
    d_rec, d_pq, d_ps, d_wr = filled(n * k + TAIL, 4), filled(n * k + TAIL, 3), filled(n * k + TAIL, 3), filled(n + TAIL, 1)
    _, visits = ds.near_counted(d_q, n, torch.from_numpy(offsets).cuda(), d_rec, d_pq, d_ps, d_wr)
    print("fill form, k = %d: %s" % (k, visits))
    assert visits["rays"] == n and visits["hits"] == n and visits["triangles"] <= n * len(own)
    got = (d_rec.cpu().numpy().view(np.uint32).reshape(-1, 4), d_pq.cpu().numpy().view(np.uint32).reshape(-1, 3), d_ps.cpu().numpy().view(np.uint32).reshape(-1, 3),
           d_wr.cpu().numpy().view(np.uint32))
    assert_fill(got, want, "deep tree, counted")
    # everything filtered: the walk still visits all of it, and every list is empty
    none = np.full(n, len(own), np.uint32)
    d_counts = filled(n + TAIL, 1)
    _, visits = ds.near_counted(d_q, n, d_counts=d_counts, first_prim=device_first(none))
    assert visits["stack_spills"] > 0 and visits["hits"] == 0 and visits["triangles"] == n * len(own)
    assert d_counts.cpu().numpy().view(np.uint32).tobytes() == expected_counts(np.zeros(n, np.uint32)).tobytes()
    assert api.lib().rtk_dev_trace_status(ds.handle, None) == 0


def test_lists(api, base):
    """A shuffled subset with repeated ids, the count on the device: listed slots as the unlisted call, the rest untouched"""
    n = 1000
    q, max2 = base.q[:n], base.max2[:n]
    counts, kept = base.ref.counts[:n], base.ref.kept[:n]
    rng = np.random.RandomState(6)
    ids = rng.permutation(n)[:333]
    ids = np.concatenate([ids, ids[:7], rng.permutation(n)[:100]])           # 7 repeated ids; 100 entries beyond the count
    count = 340
    listed = np.zeros(n, bool)
    listed[ids[:count]] = True
    offsets = base.offsets[:n + 1]
    total = int(offsets[-1])
    assert counts[ids[:7]].max() > 1                                         # (a repeated id with a list that has to be sorted)
    for kw, rows, what in ((dict(count=count, ids=ids), listed, "listed"), (dict(count=100), np.arange(n) < 100, "count alone"),
                           (dict(count=n + 1000), np.ones(n, bool), "count clamped"), (dict(count=0, ids=ids), np.zeros(n, bool), "zero count")):
        assert run_count(api, base.ds, q, max2=max2, **kw).tobytes() == expected_counts(counts, rows).tobytes(), what
        assert_fill(run_fill(api, base.ds, q, offsets, total, max2=max2, **kw), expected_fill(kept, offsets, total, rows), what)
    # the k nearest through a list whose every id stands three times
    k = 3
    off = np.arange(n + 1, dtype=np.int64) * k
    thrice = np.tile(rng.permutation(n)[:300], 3)
    rows = np.zeros(n, bool)
    rows[thrice] = True
    assert_fill(run_fill(api, base.ds, q, off, n * k, max2=max2, count=len(thrice), ids=thrice), expected_fill(kept, off, n * k, rows), "every id three times")


def test_two_launches_give_the_same_bytes_and_a_side_stream_sees_its_inputs(api, base):
    import torch
    n, k = base.n, 5
    offsets = np.arange(n + 1, dtype=np.int64) * k
    a = run_fill(api, base.ds, base.q, offsets, n * k, max2=base.max2)
    b = run_fill(api, base.ds, base.q, offsets, n * k, max2=base.max2)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert run_count(api, base.ds, base.q, max2=base.max2).tobytes() == run_count(api, base.ds, base.q, max2=base.max2).tobytes()
    # queries, limits and offsets made on a side stream, the calls enqueued behind them, nothing waited for in between
    h_q, h_max, h_off = torch.from_numpy(base.q).pin_memory(), torch.from_numpy(base.max2).pin_memory(), torch.from_numpy(offsets).pin_memory()
    d_rec, d_pq, d_ps, d_wr, d_counts = filled(n * k + TAIL, 4), filled(n * k + TAIL, 3), filled(n * k + TAIL, 3), filled(n + TAIL, 1), filled(n + TAIL, 1)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_q = h_q.cuda(non_blocking=True).clone()                    # (device work of the stream ahead of the call)
        d_max = h_max.cuda(non_blocking=True).clone()
        d_off = h_off.cuda(non_blocking=True).clone()
        base.ds.count_near_device(d_q, n, d_counts, max_dist2=d_max)
        base.ds.near_all_device(d_q, n, d_off, d_rec, d_pq, d_ps, d_wr, max_dist2=d_max)
        status_ok(api, base.ds)
    side.synchronize()
    got = (d_rec.cpu().numpy().view(np.uint32).reshape(-1, 4), d_pq.cpu().numpy().view(np.uint32).reshape(-1, 3), d_ps.cpu().numpy().view(np.uint32).reshape(-1, 3),
           d_wr.cpu().numpy().view(np.uint32))
    assert_fill(got, expected_fill(base.ref.kept, offsets, n * k), "side stream")
    assert d_counts.cpu().numpy().view(np.uint32).tobytes() == expected_counts(base.ref.counts).tobytes()


@pytest.fixture(scope="module")
def closed(api):
    """test_gpu_touch.py's closed 10 x 10 torus of 200 triangles with shared vertices plus 20 triangles that pierce it"""
    class Scene:
        pass
    s = Scene()
    rng = np.random.RandomState(12)
    mesh = torus()
    ang = rng.uniform(0, 2 * np.pi, 20)
    centre = np.stack([np.cos(ang), np.sin(ang), np.zeros(20)], 1)
    blades = centre[:, None, :] + rng.uniform(-0.7, 0.7, (20, 3, 3))
    s.tris = np.concatenate([mesh, blades]).astype(np.float32)
    s.T = len(s.tris)
    s.ds = api.DeviceScene.build([dict(positions=s.tris.reshape(-1, 3))])
    return s


def test_the_filter_and_self_contacts(api, closed):
    s = closed
    own = scene_triangles(api, s.ds)
    assert own.tobytes() == s.tris.tobytes() and s.T == 220
    ids = np.arange(s.T)
    first = (ids + 1).astype(np.uint32)
    margin = np.float32(0.15)
    max2 = np.full(s.T, margin * margin, np.float32)
    for fp, fl in ((None, False), (first, False), (None, True), (first, True)):
        ref = brute_force_near(own, ids, own, max2, fp, int(fl))
        what = "first_prim %s, skip_shared %s" % (fp is not None, fl)
        assert run_count(api, s.ds, own, max2=max2, first=fp, skip_shared=fl).tobytes() == expected_counts(ref.counts).tobytes(), what
        offsets = np.concatenate([[0], np.cumsum(ref.counts.astype(np.int64))])
        total = int(offsets[-1])
        assert_fill(run_fill(api, s.ds, own, offsets, total, max2=max2, first=fp, skip_shared=fl), expected_fill(ref.kept, offsets, total), what)
        if fp is None and not fl:
            assert all(len(r) and r[0, 0] == 0 for r, _, _ in ref.kept)      # every triangle finds itself, or a lower id, at distance 0
    # (both): each pair once, i < j, no neighbours; a blade through the mesh has dist2 = 0
    assert total > 100 and all((r[:, 3] > i).all() for i, (r, _, _) in enumerate(ref.kept)) and any(len(r) and r[0, 0] == 0 for r, _, _ in ref.kept)
    pairs, dist, pa, pb = s.ds.self_contacts(float(margin))
    status_ok(api, s.ds)
    who = np.repeat(ids, ref.counts)
    rec = np.concatenate([r for r, _, _ in ref.kept])
    assert pairs.cpu().numpy().tobytes() == np.stack([who, rec[:, 3].astype(np.int64)], 1).astype(np.int64).tobytes()
    assert (pairs[:, 0] < pairs[:, 1]).all() and len(np.unique(pairs.cpu().numpy(), axis=0)) == total
    assert dist.cpu().numpy().view(np.uint32).tobytes() == np.sqrt(rec[:, 0].copy().view(np.float32)).view(np.uint32).tobytes()
    assert pa.cpu().numpy().view(np.uint32).tobytes() == np.concatenate([x for _, x, _ in ref.kept]).tobytes()
    assert pb.cpu().numpy().view(np.uint32).tobytes() == np.concatenate([x for _, _, x in ref.kept]).tobytes()


def test_python_conveniences(api, base, closed):
    # triangles_near returns what the device forms computed
    pick = np.arange(0, base.n, 9)
    dist = np.sqrt(np.maximum(base.max2[pick], 0))
    max2 = dist.astype(np.float32) ** 2
    ref = brute_force_near(base.tris, np.arange(300), base.q[pick], max2)
    offsets, rec, pq, ps, written = base.ds.triangles_near(base.q[pick], dist)
    assert offsets.tobytes() == np.concatenate([[0], np.cumsum(ref.counts.astype(np.int64))]).tobytes() and written.tobytes() == ref.counts.tobytes()
    assert rec.tobytes() == np.concatenate([r for r, _, _ in ref.kept]).tobytes()
    assert pq.view(np.uint32).tobytes() == np.concatenate([x for _, x, _ in ref.kept]).tobytes()
    assert ps.view(np.uint32).tobytes() == np.concatenate([x for _, _, x in ref.kept]).tobytes()
    # the k nearest: rows of k, zero beyond written
    k = 4
    rec, pq, ps, written = base.ds.nearest_triangles_to(base.q[pick], k, dist)
    assert rec.shape == (len(pick), k) and pq.shape == (len(pick), k, 3) and written.tobytes() == np.minimum(ref.counts, k).astype(np.uint32).tobytes()
    for i in range(len(pick)):
        w = int(written[i])
        assert rec[i, :w].tobytes() == ref.kept[i][0][:w].tobytes() and ps[i, :w].view(np.uint32).tobytes() == ref.kept[i][2][:w].tobytes()
        assert not rec[i, w:].view(np.uint32).any() and not pq[i, w:].view(np.uint32).any()
    # empty input gives empty outputs
    out = base.ds.triangles_near(np.zeros((0, 9), np.float32), 1.0)
    assert out[0].tolist() == [0] and all(len(x) == 0 for x in out[1:])
    out = base.ds.nearest_triangles_to(np.zeros((0, 3, 3), np.float32), 3)
    assert out[0].shape == (0, 3) and len(out[3]) == 0
    # contacts between two scenes: the blades against the mesh
    mesh = api.DeviceScene.build([dict(positions=closed.tris[:200].reshape(-1, 3))])
    blades = api.DeviceScene.build([dict(positions=closed.tris[200:].reshape(-1, 3))])
    margin = np.float32(0.05)
    ref = brute_force_near(closed.tris[:200], np.arange(200), closed.tris[200:], np.full(20, margin * margin, np.float32))
    pairs, d, pa, pb = mesh.contacts(blades, float(margin))
    status_ok(api, mesh)
    rec = np.concatenate([r for r, _, _ in ref.kept])
    assert len(rec) > 20 and (rec[:, 0] == 0).any()
    assert pairs.cpu().numpy().tobytes() == np.stack([np.repeat(np.arange(20), ref.counts), rec[:, 3].astype(np.int64)], 1).astype(np.int64).tobytes()
    assert d.cpu().numpy().view(np.uint32).tobytes() == np.sqrt(rec[:, 0].copy().view(np.float32)).view(np.uint32).tobytes()
    assert pa.cpu().numpy().view(np.uint32).tobytes() == np.concatenate([x for _, x, _ in ref.kept]).tobytes()
    assert pb.cpu().numpy().view(np.uint32).tobytes() == np.concatenate([x for _, _, x in ref.kept]).tobytes()
