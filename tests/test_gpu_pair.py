"""GPU tests of rtk_dev_closest_triangles. The bar everywhere: records and both point arrays are bit for bit what numpy float32
brute force gives by the rule of rtk_amd/csrc/rtk_pair_rule.h (tests/pair_ref.py) over the triangle records the scene holds at
that moment -- read back through rtk_dev_expand_hits --, whatever tree is above them and whatever order the walk takes. Every
output is pre-filled with 0x7e and carries a tail; whole buffers are compared, so nothing may be written outside the answered
slots or behind the batch; rtk_dev_trace_status is 0 after every call. The base scene is the 300-triangle soup of
tests/test_gpu_touch.py and its query mix without the eight huge members (their overflowing intermediates make NaN weights,
whose bits a host and a device need not share); every brute force stays below half a million (query, triangle) pairs."""
import ctypes as C

import numpy as np
import pytest

from rtk_amd import synth
from rtk_amd.types import RTK_INF
from tests.pair_ref import FEATURE_PIERCE, brute_force_pairs, pair_np
from tests.test_gpu_box import list_tensors, status_ok
from tests.test_gpu_closest import FILL, TAIL, scene_triangles
from tests.test_gpu_touch import device_first, device_queries, torus
from tests.touch_ref import mix_slices, query_mix

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF


def run(api, ds, q, n=None, max2=None, count=None, ids=None, first=None, skip_shared=False, points=(True, True)):
    """-> (record words [n + TAIL, 4], query-point words [n + TAIL, 3] or None, scene-point words or None) as the device left them"""
    import torch
    n = len(q) if n is None else n
    d_rec = torch.full(((n + TAIL) * 16,), 0x7e, dtype=torch.uint8, device="cuda")
    d_pts = [torch.full(((n + TAIL) * 12,), 0x7e, dtype=torch.uint8, device="cuda") if want else None for want in points]
    d_max = torch.from_numpy(np.ascontiguousarray(max2, np.float32)).cuda() if max2 is not None else None
    d_count, d_ids = list_tensors(count, ids)
    # (the C call itself: the Python form allocates point arrays that are not given, and NULL must be tried)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    d_q, d_first = device_queries(api, q), device_first(first)
    l = api.make_ray_list(d_count, d_ids) if d_count is not None else None
    f = api.make_touch_filter(d_first, skip_shared)
    rc = api.lib().rtk_dev_closest_triangles(ds.handle, ptr(d_q), n, C.byref(l) if l is not None else None, C.byref(f) if f is not None else None,
                                             ptr(d_max), ptr(d_rec), ptr(d_pts[0]), ptr(d_pts[1]), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, api.last_error()
    status_ok(api, ds)
    return (d_rec.cpu().numpy().view(np.uint32).reshape(-1, 4),) + tuple(d.cpu().numpy().view(np.uint32).reshape(-1, 3) if d is not None else None for d in d_pts)


def assert_same(got, want, what, answered=None):
    """got as run() left it; want = brute_force_pairs' three arrays; answered: bool [n] or None (all)"""
    n = len(want[0])
    for g, w, name in zip(got, want, ("records", "points on the query", "points on the scene")):
        if g is None:
            continue
        assert (g[n:] == FILL).all(), (what, name, "written beyond num_queries")
        rows = np.ones(n, bool) if answered is None else answered
        bad = np.nonzero((g[:n][rows] != w[rows]).any(1))[0]
        assert len(bad) == 0, (what, name, len(bad), np.nonzero(rows)[0][bad[:5]], g[:n][rows][bad[:3]], w[rows][bad[:3]])
        assert (g[:n][~rows] == FILL).all(), (what, name, "a slot that is not listed was written")


def limits(rng, n, scale):
    """one squared limit per query: some none, some tight, and the entries that make a miss"""
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
    b.segments, b.points = part["segments"], part["points"]             # (both stand before the part taken out)
    b.not_live = slice(b.n - 36, b.n)
    b.max2 = limits(np.random.RandomState(3), b.n, 0.2)
    # the references, computed once and shared
    b.ref = brute_force_pairs(b.tris, np.arange(300), b.q)
    b.ref_max = brute_force_pairs(b.tris, np.arange(300), b.q, b.max2)
    return b


def test_equals_brute_force_without_a_limit(api, base):
    assert scene_triangles(api, base.ds).tobytes() == base.tris.tobytes()
    got = run(api, base.ds, base.q)
    assert_same(got, base.ref, "no limit")
    rec = base.ref[0]
    hit = rec[:, 3] != NONE
    assert hit[:base.not_live.start].all() and not hit[base.not_live].any()
    assert (rec[base.not_live, 0] == np.float32(RTK_INF).view(np.uint32)).all()
    assert (base.ref[1][base.not_live] == base.q[base.not_live, 0].view(np.uint32)).all()          # vertex 0 as given, NaN bits included
    d = rec[:, 0].view(np.float32)
    assert (d[hit] == 0).sum() > 100 and (d[hit] > 0).sum() > 300
    # segments and points as queries: answered by the pair rule alone, and found
    assert hit[base.segments].all() and hit[base.points].all() and (d[base.segments] > 0).any() and (d[base.points] > 0).any()
    # a float32 [n, 3, 3] tensor is a batch of queries as it stands; NULL point arrays: the records alone, the same
    assert_same(run(api, base.ds, base.q, points=(False, False)), base.ref, "no points")
    assert_same(run(api, base.ds, base.q, points=(True, False)), base.ref, "query points only")
    assert_same(run(api, base.ds, base.q, points=(False, True)), base.ref, "scene points only")


def test_equals_brute_force_with_limits(api, base):
    got = run(api, base.ds, base.q, max2=base.max2)
    assert_same(got, base.ref_max, "limits")
    rec = base.ref_max[0]
    miss = rec[:, 3] == NONE
    bad_limit = ~(base.max2 > 0)
    assert bad_limit.sum() > 50 and miss[bad_limit].all() and (rec[miss, 0] == base.max2.view(np.uint32)[miss]).all()
    assert (miss & ~bad_limit)[:base.not_live.start].any() and (~miss).sum() > 300                  # a limit that cuts, and one that does not
    assert (rec[~miss, 0].view(np.float32) < base.max2[~miss]).all()
    # RTK_INF in every entry is the call without the array
    assert_same(run(api, base.ds, base.q, max2=np.full(base.n, RTK_INF, np.float32)), base.ref, "RTK_INF entries")


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_sizes(api, base, n):
    which = (np.arange(n) * 7) % base.n                              # (a stride: every part of the mix at every size)
    want = tuple(x[which] for x in base.ref_max)
    assert_same(run(api, base.ds, base.q[which], n=n, max2=base.max2[which] if n else np.zeros(1, np.float32)), want, "n = %d" % n)


def test_lists(api, base):
    """A shuffled subset with repeated ids, the count on the device: listed slots as the unlisted call, the rest untouched"""
    n = 1000
    q, max2 = base.q[:n], base.max2[:n]
    want = tuple(x[:n] for x in base.ref_max)
    rng = np.random.RandomState(6)
    ids = rng.permutation(n)[:333]
    ids = np.concatenate([ids, ids[:7], rng.permutation(n)[:100]])           # 7 repeated ids; 100 entries beyond the count
    count = 340
    listed = np.zeros(n, bool)
    listed[ids[:count]] = True
    assert_same(run(api, base.ds, q, max2=max2, count=count, ids=ids), want, "listed", listed)
    # no ids: the first `count` queries; a count beyond the arrays is clamped to them; an empty list writes nothing
    assert_same(run(api, base.ds, q, max2=max2, count=100), want, "count alone", np.arange(n) < 100)
    assert_same(run(api, base.ds, q, max2=max2, count=n + 1000), want, "count clamped")
    assert_same(run(api, base.ds, q, max2=max2, count=0, ids=ids), want, "zero count", np.zeros(n, bool))


def test_two_launches_give_the_same_bytes_and_a_side_stream_sees_its_inputs(api, base):
    import torch
    a = run(api, base.ds, base.q, max2=base.max2)
    b = run(api, base.ds, base.q, max2=base.max2)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    # queries and limits made on a side stream, the call enqueued behind them, nothing waited for in between
    n = base.n
    h_q, h_max = torch.from_numpy(base.q).pin_memory(), torch.from_numpy(base.max2).pin_memory()
    d_rec = torch.full(((n + TAIL) * 16,), 0x7e, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_q = h_q.cuda(non_blocking=True).clone()                    # (device work of the stream ahead of the call)
        d_max = h_max.cuda(non_blocking=True).clone()
        _, d_pq, d_ps = base.ds.closest_triangles_device(d_q, n, d_rec, max_dist2=d_max)
        status_ok(api, base.ds)
    side.synchronize()
    got = (d_rec.cpu().numpy().view(np.uint32).reshape(-1, 4), d_pq.cpu().numpy().view(np.uint32).reshape(-1, 3), d_ps.cpu().numpy().view(np.uint32).reshape(-1, 3))
    for g, w in zip(got, base.ref_max):
        assert g[:n].tobytes() == w.tobytes()


def check_scene(api, ds, q, max2, ref=None):
    if ref is None:
        tris = scene_triangles(api, ds)
        ref = brute_force_pairs(tris, np.arange(len(tris)), q, max2)
    got = run(api, ds, q, max2=max2)
    assert_same(got, ref, "scene")
    return b"".join(x.tobytes() for x in got)


def test_the_tree_does_not_matter(api, base):
    """A device build, the CPU task builder's blob uploaded (leaves of 4 to 63, loose boxes), that scene after split_leaves, a
    refit to moved positions, a rebuild: each equals brute force over its own records, and where the triangles are the same
    the answers are the same bytes."""
    L = api.lib()
    q, max2 = base.q, base.max2
    first = check_scene(api, base.ds, q, max2, base.ref_max)
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
    got = check_scene(api, up, q, max2, base.ref_max if same else None)
    assert not same or got == first
    split = up.split_leaves()
    assert split["leaves_split"] > 0
    got = check_scene(api, up, q, max2, base.ref_max if same else None)
    assert not same or got == first
    # moved positions: their own brute force
    ds = api.DeviceScene.build([dict(positions=base.positions)])
    rng = np.random.RandomState(8)
    moved = (base.positions + rng.uniform(-0.05, 0.05, base.positions.shape)).astype(np.float32)
    ds.refit([dict(positions=moved)])
    assert scene_triangles(api, ds).tobytes() == moved.tobytes()
    ref = brute_force_pairs(moved.reshape(300, 3, 3), np.arange(300), q, max2)
    after_refit = check_scene(api, ds, q, max2, ref)
    assert after_refit != first
    ds.rebuild()
    assert scene_triangles(api, ds).tobytes() == moved.tobytes()
    assert check_scene(api, ds, q, max2, ref) == after_refit


def test_a_stack_deeper_than_the_on_chip_part(api):
    """The geometric cluster of tests/test_gpu_build.py: a deep, lopsided tree; query triangles far from the corner the chain
    converges on keep every level's sibling on the stack"""
    from tests.test_gpu_build import _adversarial_scenes
    tris = _adversarial_scenes()["geometric_chain"]
    ds = api.DeviceScene.build([dict(positions=tris.reshape(-1, 3))])
    on_chip = api.lib().rtk_amd_pair_stack_entries()
    assert ds.info()["stack_entries"] > on_chip, (ds.info()["stack_entries"], on_chip)
    rng = np.random.RandomState(4)
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    ext = hi - lo
    t = rng.uniform(1, 4, (40, 1))
    spans = np.stack([lo - t * ext, hi + t * ext, hi + t * ext], 1)
    anywhere = lo + ext * rng.uniform(0, 1, (88, 3, 3)) ** rng.choice([1, 2, 8], (88, 3, 1))
    q = np.concatenate([spans, anywhere]).astype(np.float32)
    n = len(q)
    assert n * len(tris) <= 500000
    own = scene_triangles(api, ds)
    # an equal distance everywhere keeps every subtree alive: a first_prim beyond every id makes the walk visit all of it
    ref = brute_force_pairs(own, np.arange(len(own)), q)
    assert_same(run(api, ds, q), ref, "deep tree")
    none = np.full(n, len(own), np.uint32)
    ref_none = brute_force_pairs(own, np.arange(len(own)), q, None, none)
    assert (ref_none[0][:, 3] == NONE).all()
    assert_same(run(api, ds, q, first=none), ref_none, "deep tree, everything filtered")
    d_rec, d_pq, d_ps, visits = ds.closest_triangles_counted(device_queries(api, q), n, first_prim=device_first(none))
    print("geometric_chain: stack entries %d, on chip %d, counted %s" % (ds.info()["stack_entries"], on_chip, visits))
    assert visits["stack_spills"] > 0 and visits["rays"] == n and visits["hits"] == 0 and visits["triangles"] == n * len(own)
    assert d_rec.cpu().numpy().view(np.uint32).reshape(n, 4).tobytes() == ref_none[0].tobytes()
    d_rec, d_pq, d_ps, visits = ds.closest_triangles_counted(device_queries(api, q), n)
    assert visits["rays"] == n and visits["hits"] == n and visits["triangles"] < n * len(own)
    for g, w in zip((d_rec, d_pq, d_ps), ref):
        assert g.cpu().numpy().view(np.uint32).tobytes() == w.tobytes()
    assert api.lib().rtk_dev_trace_status(ds.handle, None) == 0


@pytest.fixture(scope="module")
def pierced(api):
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


def test_the_filter_and_pierced_pairs(api, pierced):
    s = pierced
    own = scene_triangles(api, s.ds)
    assert own.tobytes() == s.tris.tobytes() and s.T == 220
    ids = np.arange(s.T)
    # without the filter every triangle finds itself, or a lower id at distance 0
    plain = brute_force_pairs(own, ids, own)
    assert (plain[0][:, 0] == 0).all() and (plain[0][:, 3] <= ids).all()
    assert_same(run(api, s.ds, own), plain, "no filter")
    # first_prim alone, skip_shared alone, and both: self-clearance per triangle
    first = (ids + 1).astype(np.uint32)
    for fp, fl in ((first, False), (None, True), (first, True)):
        ref = brute_force_pairs(own, ids, own, None, fp, int(fl))
        assert_same(run(api, s.ds, own, first=fp, skip_shared=fl), ref, "first_prim %s, skip_shared %s" % (fp is not None, fl))
    rec = ref[0]                                                    # (both)
    hit = rec[:, 3] != NONE
    assert hit.sum() > 150 and (~hit).any() and (rec[hit, 3] > ids[hit]).all()
    d = rec[:, 0].view(np.float32)
    assert (d[hit] == 0).sum() >= 10 and (d[hit] > 0).sum() > 100            # a blade through the mesh; a clean neighbourhood
    which = np.nonzero(hit & (d == 0))[0]
    feat = pair_np(own[which], own[rec[which, 3]]).feature
    assert (feat >= FEATURE_PIERCE).any()
    # the counted form takes the filter and the limits too
    max2 = np.full(s.T, 0.01, np.float32)
    ref = brute_force_pairs(own, ids, own, max2, first, 1)
    import torch
    d_rec, d_pq, d_ps, visits = s.ds.closest_triangles_counted(device_queries(api, own), s.T, max_dist2=torch.from_numpy(max2).cuda(),
                                                               first_prim=device_first(first), skip_shared=True)
    assert visits["rays"] == s.T and visits["hits"] == int((ref[0][:, 3] != NONE).sum())
    for g, w in zip((d_rec, d_pq, d_ps), ref):
        assert g.cpu().numpy().view(np.uint32).tobytes() == w.tobytes()


def test_python_conveniences(api, base, pierced):
    # closest_triangles returns what the device form computed
    pick = np.arange(0, base.n, 9)
    dist, prim, u, v, pq, ps = base.ds.closest_triangles(base.q[pick], max_dist=np.sqrt(np.maximum(base.max2[pick], 0)))
    max2 = np.sqrt(np.maximum(base.max2[pick], 0)).astype(np.float32) ** 2
    ref = brute_force_pairs(base.tris, np.arange(300), base.q[pick], max2)
    assert prim.tobytes() == ref[0][:, 3].tobytes() and u.view(np.uint32).tobytes() == ref[0][:, 1].tobytes() and v.view(np.uint32).tobytes() == ref[0][:, 2].tobytes()
    assert (dist.view(np.uint32) == np.sqrt(ref[0][:, 0].view(np.float32)).view(np.uint32)).all()
    assert pq.view(np.uint32).tobytes() == ref[1].tobytes() and ps.view(np.uint32).tobytes() == ref[2].tobytes()
    assert all(len(x) == 0 for x in base.ds.closest_triangles(np.zeros((0, 9), np.float32)))
    # two separated tori: the distance is the brute-force minimum, the lowest query among equal ones
    ta = torus()
    tb = (torus() + np.array([3.5, 0.3, 0.2], np.float32)).astype(np.float32)
    da, db = (api.DeviceScene.build([dict(positions=t.reshape(-1, 3))]) for t in (ta, tb))
    ref = brute_force_pairs(ta, np.arange(len(ta)), tb)
    d2 = ref[0][:, 0].view(np.float32)
    i = int(np.argmin(d2))                                           # (the first among equal ones)
    got = da.distance(db)
    status_ok(api, da)
    assert got[0] == float(np.sqrt(d2[i])) and got[0] > 0.5 and got[1] == i and got[2] == int(ref[0][i, 3])
    assert got[3].view(np.uint32).tobytes() == ref[1][i].tobytes() and got[4].view(np.uint32).tobytes() == ref[2][i].tobytes()
    # the pierced pair: the blades go through the mesh
    mesh = api.DeviceScene.build([dict(positions=pierced.tris[:200].reshape(-1, 3))])
    blades = api.DeviceScene.build([dict(positions=pierced.tris[200:].reshape(-1, 3))])
    got = mesh.distance(blades)
    assert got[0] == 0.0 and (got[3] == got[4]).all()
    # a clean torus: its self-clearance is positive and equals brute force
    ids = np.arange(len(ta))
    ref = brute_force_pairs(ta, ids, ta, None, (ids + 1).astype(np.uint32), 1)
    d2 = np.where(ref[0][:, 3] != NONE, ref[0][:, 0].view(np.float32), np.float32(np.inf))
    i = int(np.argmin(d2))
    got = da.self_clearance()
    assert got[0] == float(np.sqrt(d2[i])) and got[0] > 0 and got[1] == i and got[2] == int(ref[0][i, 3]) and got[2] > got[1]
    assert got[3].view(np.uint32).tobytes() == ref[1][i].tobytes() and got[4].view(np.uint32).tobytes() == ref[2][i].tobytes()
