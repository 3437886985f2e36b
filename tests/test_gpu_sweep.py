"""GPU tests of rtk_dev_sweep_spheres / _any / _counted. The bar everywhere: records, contact points and centres are bit for bit
what numpy float32 brute force gives by the rule of rtk_amd/csrc/rtk_sweep_rule.h (tests/sweep_ref.py) over the triangle records
the scene holds at that moment -- read back through rtk_dev_expand_hits, so they are the scene's own --, whatever tree is above
them. Outputs are pre-filled with 0x7e and carry a tail that must stay untouched. The base scene is the 300-triangle soup of the
closest-points tests with about 1500 sweeps; every brute force stays below a million (query, triangle) pairs."""
import ctypes as C

import numpy as np
import pytest

from rtk_amd import synth
from rtk_amd.types import HIT_DTYPE, HIT_RECORD_DTYPE, RTK_INF
from tests.sweep_ref import NONE, brute_force

pytestmark = pytest.mark.gpu

TAIL = 5                                     # slots behind the batch that nobody may write
FILL = 0x7e7e7e7e


def scene_triangles(api, ds):
    """The scene's current triangle records by primitive id, [T, 3, 3] float32, through the expansion of made-up records"""
    n = ds.info()["num_triangles"]
    rec = np.zeros(n, HIT_RECORD_DTYPE)
    rec["prim"] = np.arange(n, dtype=np.uint32)
    d_hits, _ = ds.expand_device(api.to_device(rec), n)
    return np.ascontiguousarray(d_hits.cpu().numpy().view(HIT_DTYPE)["vertex"]["position"])


def run(api, ds, sweeps, n=None, count=None, ids=None, any_hit=False, **filt):
    """sweeps: float32 [n, 9]. -> (record words [n + TAIL, 4], point words [n + TAIL, 3], centre words [n + TAIL, 3]) as the device
    left them, or the bytes [n + TAIL] of the any-hit form"""
    import torch
    n = len(sweeps) if n is None else n
    d_s = api.to_device(np.ascontiguousarray(sweeps, np.float32)) if len(sweeps) else torch.zeros(36, dtype=torch.uint8, device="cuda")
    d_count = torch.tensor([count], dtype=torch.int64, device="cuda") if count is not None else None
    d_ids = torch.from_numpy(np.ascontiguousarray(ids, np.int64)).cuda() if ids is not None else None
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if any_hit:
        d_b = torch.full((n + TAIL,), 0x7e, dtype=torch.uint8, device="cuda")
        ds.sweep_spheres_any_device(d_s, n, d_b, count=d_count, ids=d_ids, **filt)
        assert api.lib().rtk_dev_trace_status(ds.handle, stream) == 0, api.last_error()
        b = d_b.cpu().numpy()
        assert (b[n:] == 0x7e).all(), "written beyond num_sweeps"
        return b
    d_rec = torch.full(((n + TAIL) * 16,), 0x7e, dtype=torch.uint8, device="cuda")
    d_pts = torch.full(((n + TAIL) * 12,), 0x7e, dtype=torch.uint8, device="cuda")
    d_ctr = torch.full(((n + TAIL) * 12,), 0x7e, dtype=torch.uint8, device="cuda")
    ds.sweep_spheres_device(d_s, n, d_rec, d_pts, d_ctr, count=d_count, ids=d_ids, **filt)
    assert api.lib().rtk_dev_trace_status(ds.handle, stream) == 0, api.last_error()
    rec = d_rec.cpu().numpy().view(np.uint32).reshape(n + TAIL, 4)
    pts = d_pts.cpu().numpy().view(np.uint32).reshape(n + TAIL, 3)
    ctr = d_ctr.cpu().numpy().view(np.uint32).reshape(n + TAIL, 3)
    assert (rec[n:] == FILL).all() and (pts[n:] == FILL).all() and (ctr[n:] == FILL).all(), "written beyond num_sweeps"
    return rec, pts, ctr


def check(api, ds, sweeps, want=None, **filt):
    """the whole batch against brute force over the scene's own records (or the reference given); returns the records"""
    if want is None:
        tris = scene_triangles(api, ds)
        want = brute_force(tris, np.arange(len(tris), dtype=np.uint32), sweeps)
    want_rec, want_pts, want_ctr = want
    rec, pts, ctr = run(api, ds, sweeps, **filt)
    n = len(sweeps)
    bad = np.nonzero((rec[:n] != want_rec).any(1) | (pts[:n] != want_pts).any(1) | (ctr[:n] != want_ctr).any(1))[0]
    assert len(bad) == 0, (len(bad), bad[:5], sweeps[bad[:5]], rec[bad[:5]], want_rec[bad[:5]], pts[bad[:5]], want_pts[bad[:5]], ctr[bad[:5]], want_ctr[bad[:5]])
    return rec[:n].copy().view(HIT_RECORD_DTYPE).reshape(n)


def sweep_mix(tris, seed=11):
    """About 1500 sweeps over a scene of few triangles, float32 [n, 9]: paths through the box and beside it, starts on and inside
    the surface, radii from 0 to a fifth of the extent, max_t around the true time, RTK_INF, queries that are not live."""
    rng = np.random.RandomState(seed)
    tris = np.asarray(tris, np.float32).reshape(-1, 3, 3)
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    ext = hi - lo
    size = float(ext.max())

    def rows(o, d, r, max_t=RTK_INF, min_t=0.0):
        n = len(o)
        s = np.zeros((n, 9), np.float32)
        s[:, 0:3], s[:, 3:6] = o, d
        s[:, 6], s[:, 7], s[:, 8] = min_t, max_t, r
        return s
    radii = lambda n: (rng.uniform(0, 1, n) ** 2 * 0.2 * size) * (rng.uniform(0, 1, n) > 0.15)      # (a seventh: radius 0)
    parts = []
    # through the box: from outside towards a point inside
    o = lo - ext + rng.uniform(0, 3, (500, 3)) * ext
    parts.append(rows(o, rng.uniform(lo, hi, (500, 3)) - o, radii(500)))
    # beside it: parallel to an axis, outside or just inside a face of the box
    o = rng.uniform(lo - 0.3 * ext, hi + 0.3 * ext, (200, 3))
    d = np.zeros((200, 3)); d[np.arange(200), np.arange(200) % 3] = rng.choice([-1.0, 1.0], 200) * size
    o[np.arange(200), np.arange(200) % 3] = (lo - ext)[np.arange(200) % 3]
    d[np.arange(200), np.arange(200) % 3] = np.abs(d[np.arange(200), np.arange(200) % 3]) * 3
    parts.append(rows(o, d, radii(200)))
    # starts on the surface (vertices, centroids) and inside the scene's box, short and long paths
    pick = rng.permutation(len(tris))[:150]
    o = np.concatenate([tris[pick, rng.randint(0, 3, 150)], tris[pick].astype(np.float64).mean(1), rng.uniform(lo, hi, (150, 3))])
    parts.append(rows(o, rng.standard_normal((450, 3)) * size, radii(450), max_t=rng.choice([RTK_INF, 0.05, 1.0], 450), min_t=rng.choice([0.0, -0.1, 0.02], 450)))
    # min_t = max_t
    parts.append(rows(rng.uniform(lo, hi, (60, 3)), rng.standard_normal((60, 3)), radii(60) * 0.5, max_t=0.25, min_t=0.25))
    mix = np.concatenate(parts)
    # max_t at the float32 neighbour below the true time, at it (the interval is closed: still a hit) and above it
    through = brute_force(tris, np.arange(len(tris), dtype=np.uint32), mix[:500])[0]
    some = np.nonzero(through[:, 3] != NONE)[0][:80]
    assert len(some) == 80
    true_t = through[some, 0].view(np.float32)
    for t in (np.nextafter(true_t, np.float32(-np.inf)), true_t, np.nextafter(true_t, np.float32(np.inf))):
        s = mix[some].copy(); s[:, 7] = t
        parts.append(s)
    # the same three with min_t < 0 and a start inside the grown box of the triangle that is hit (a ball a little more than its
    # radius above a face, moving towards it): the entry time te is negative and larger than the time, so max_t - te rounds
    # coarsely, and a time an ulp beyond max_t must become a miss (2. (iv) of the rule)
    pick = rng.permutation(len(tris))[:240]
    a, b, c = (tris[pick, k].astype(np.float64) for k in range(3))
    nrm = np.cross(b - a, c - a); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    r = rng.uniform(0.005, 0.05, 240) * size
    o = (a + b + c) / 3 + nrm * (r * rng.uniform(1.05, 1.5, 240))[:, None]
    d = -nrm * size * rng.uniform(0.5, 2.0, (240, 1)) + rng.standard_normal((240, 3)) * 0.1 * size
    near = rows(o, d, r, min_t=-rng.uniform(0.05, 0.5, 240))
    rec = brute_force(tris, np.arange(len(tris), dtype=np.uint32), near)[0]
    some = np.nonzero((rec[:, 3] != NONE) & (rec[:, 0].view(np.float32) > 0))[0][:30]
    assert len(some) == 30
    true_t = rec[some, 0].view(np.float32)
    for t in (np.nextafter(true_t, np.float32(-np.inf)), true_t, np.nextafter(true_t, np.float32(np.inf))):
        s = near[some].copy(); s[:, 7] = t
        parts.append(s)
    # not live: NaN and infinities in every field, a negative radius, a zero direction, min_t > max_t
    bad = mix[rng.permutation(500)[:45]].copy()
    bad[np.arange(27), np.arange(27) % 9] = np.array([np.nan, np.inf, -np.inf], np.float32)[np.arange(27) // 9]
    bad[27:33, 8] = -0.01 * size
    bad[33:39, 3:6] = 0.0
    bad[39:45, 6], bad[39:45, 7] = 2.0, 1.0
    parts.append(bad)
    return np.concatenate(parts).astype(np.float32)


@pytest.fixture(scope="module")
def base(api):
    class Base:
        pass
    b = Base()
    b.positions = synth.triangle_soup(300, 0.2, seed=5)
    b.tris = b.positions.reshape(300, 3, 3)
    b.ds = api.DeviceScene.build([dict(positions=b.positions)])
    b.sweeps = sweep_mix(b.tris)
    # the reference, computed once and shared
    b.want = brute_force(b.tris, np.arange(300, dtype=np.uint32), b.sweeps)
    return b


def test_sweep_mix_equals_brute_force(api, base):
    assert scene_triangles(api, base.ds).tobytes() == base.tris.tobytes()     # (the records are the input's, in input order)
    n = len(base.sweeps)
    assert 1400 <= n <= 1600 and n * 300 < 1000000
    # what the numpy reference shows for these inputs: the hit share, starts that touch, every kind of miss
    want_hit = base.want[0][:, 3] != NONE
    print("sweeps %d, hits by the reference %.3f" % (n, want_hit.mean()))
    assert 0.5 < want_hit.mean() < 0.9
    assert (base.want[0][want_hit, 0].view(np.float32) == base.sweeps[want_hit, 6]).sum() >= 100     # a hit at min_t: the start touches
    rec = check(api, base.ds, base.sweeps, base.want)
    hit = rec["prim"] != NONE
    assert 0.5 < hit.mean() < 0.9
    assert (rec["u"][~hit] == 0).all() and (rec["v"][~hit] == 0).all() and (rec["t"][~hit].view(np.uint32) == base.sweeps[~hit, 7].view(np.uint32)).all()
    # max_t below, at and above the true time (the words are the reference's, checked above): below it a miss; at it the closed
    # interval keeps the hit unless the rounding of max_t - te in the rule loses it; above it the unlimited query's record
    k = n - 45 - 90 - 240
    below, at, above = rec[k:k + 80], rec[k + 80:k + 160], rec[k + 160:k + 240]
    assert (below["prim"] == NONE).all() and (above["prim"] != NONE).sum() >= 70 and 20 <= (at["prim"] != NONE).sum() <= 80
    assert (at["t"][at["prim"] != NONE] == base.sweeps[k + 80:k + 160, 7][at["prim"] != NONE]).all()
    # the same with min_t < 0 and a negative entry time: a touch of the same triangle or of a later one is beyond max_t
    k = n - 45 - 90
    assert (base.sweeps[k:k + 90, 6] < 0).all()
    below, at, above = rec[k:k + 30], rec[k + 30:k + 60], rec[k + 60:k + 90]
    assert (below["prim"] == NONE).all() and (above["prim"] != NONE).sum() >= 25 and 8 <= (at["prim"] != NONE).sum() <= 30
    assert (at["t"][at["prim"] != NONE] == base.sweeps[k + 30:k + 60, 7][at["prim"] != NONE]).all()
    # no record, hit or miss, has a time outside [min_t, max_t]
    live = (np.arange(n) < n - 45) & (base.sweeps[:, 6] <= base.sweeps[:, 7])    # (max_t below a time of 0 is not live)
    assert live.sum() >= n - 50 and (rec["t"][live] >= base.sweeps[live, 6]).all() and (rec["t"][live] <= base.sweeps[live, 7]).all()
    assert (rec["prim"][n - 45:] == NONE).all()                               # not live
    # the numpy conveniences on top of it: the same records
    plain = np.nonzero((base.sweeps[:, 6] == 0) & (base.sweeps[:, 7] == RTK_INF))[0][:400]
    s = base.sweeps[plain]
    rec2, pts2, ctr2 = base.ds.sweep_spheres(s[:, 0:3], s[:, 3:6], s[:, 8])
    assert rec2.tobytes() == rec[plain].tobytes() and pts2.shape == (len(plain), 3) and ctr2.shape == (len(plain), 3)
    assert pts2.view(np.uint32).tobytes() == base.want[1][plain].tobytes() and ctr2.view(np.uint32).tobytes() == base.want[2][plain].tobytes()
    blocked = base.ds.path_blocked(s[:, 0:3], s[:, 3:6], s[:, 8])
    assert blocked.dtype == bool and (blocked == (rec2["prim"] != NONE)).all()
    rec3, _, _ = base.ds.sweep_spheres(s[:50, 0:3], s[:50, 3:6], 0.01, max_t=0.5, min_t=-0.25)
    s3 = s[:50].copy(); s3[:, 6], s3[:, 7], s3[:, 8] = -0.25, 0.5, 0.01
    assert rec3.view(np.uint32).reshape(-1, 4).tobytes() == brute_force(base.tris, np.arange(300), s3)[0].tobytes()


def test_the_tree_does_not_matter(api, base):
    """A device build, the CPU task builder's blob uploaded (leaves of 4 to 63, loose boxes), that scene after split_leaves, a
    refit to moved positions, a rebuild: each equals brute force over its own records, and where the triangles are the same
    the answers are the same bytes."""
    L = api.lib()
    s = base.sweeps[:1000]
    first = base.want[0][:1000].tobytes()
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
    got = check(api, up, s)
    assert not same or got.tobytes() == first
    split = up.split_leaves()
    assert split["leaves_split"] > 0
    got = check(api, up, s)
    assert not same or got.tobytes() == first
    # moved positions: their own brute force
    ds = api.DeviceScene.build([dict(positions=base.positions)])
    rng = np.random.RandomState(8)
    moved = (base.positions + rng.uniform(-0.05, 0.05, base.positions.shape)).astype(np.float32)
    ds.refit([dict(positions=moved)])
    assert scene_triangles(api, ds).tobytes() == moved.tobytes()
    after_refit = check(api, ds, s)
    assert after_refit.tobytes() != first
    ds.rebuild()
    assert scene_triangles(api, ds).tobytes() == moved.tobytes()
    assert check(api, ds, s).tobytes() == after_refit.tobytes()


def test_any_hit_form_equals_the_closest_form(api, base):
    n = len(base.sweeps)
    b = run(api, base.ds, base.sweeps, any_hit=True)
    want = (base.want[0][:, 3] != NONE).astype(np.uint8)
    assert (b[:n] == want).all(), np.nonzero(b[:n] != want)[0][:10]
    assert 0 < want.sum() < n


def test_filters(api, base):
    """A mesh mask on a three-mesh scene and a per-slot ignore_prim, each against the filtered brute force; among duplicated
    triangles the lowest id wins"""
    # three meshes: the soup in two halves, and the first half once more (so that every triangle of it has a twin with a higher id)
    a, b = base.positions[:450], base.positions[450:]
    ds = api.DeviceScene.build([dict(positions=a), dict(positions=b), dict(positions=a)])
    tris = scene_triangles(api, ds)
    assert len(tris) == 450 and tris[:300].tobytes() == base.tris.tobytes() and tris[300:].tobytes() == base.tris[:150].tobytes()
    prims = np.arange(450, dtype=np.uint32)
    mesh_of = np.repeat([0, 1, 2], 150)
    s = base.sweeps[:900]
    rec = check(api, ds, s)
    hit = rec["prim"] != NONE
    assert (rec["prim"][hit] < 300).all() and rec.tobytes() == base.want[0][:900].tobytes()          # the twin never wins
    for mask in ([False, True, True], [True, False], [False, False, False], [True, True, True, True]):
        want = brute_force(tris, prims, s, mesh_of=mesh_of, filter=dict(mesh_mask=mask))
        got = check(api, ds, s, want, mesh_mask=mask)
        h = got["prim"] != NONE
        assert all(mask[m] for m in np.unique(mesh_of[got["prim"][h]])) and (h.any() or not any(mask))
        assert (run(api, ds, s, any_hit=True, mesh_mask=mask)[:900] == h).all()
    got = check(api, ds, s, brute_force(tris, prims, s, mesh_of=mesh_of, filter=dict(mesh_mask=[False, True, True])), mesh_mask=[False, True, True])
    assert (got["prim"][got["prim"] != NONE] >= 150).all() and (got["prim"] >= 300).sum() > 50 and (got["prim"] != rec["prim"]).any()
    # ignore_prim per query slot: every query ignores the triangle it would hit; then its twin or the next one is found
    ignore = rec["prim"].copy()
    want = brute_force(tris, prims, s, filter=dict(ignore_prim=ignore))
    got = check(api, ds, s, want, ignore_prim=ignore)
    assert (got["prim"][hit] != rec["prim"][hit]).all() and (got["prim"][hit & (rec["prim"] < 150)] != NONE).all()    # (at least its twin is left)
    assert (got["prim"][hit & (rec["prim"] < 150)] == rec["prim"][hit & (rec["prim"] < 150)] + 300).sum() > 100
    assert got[~hit].tobytes() == rec[~hit].tobytes()
    # both at once, with a list: the filter array is read at the query's own slot
    import torch
    ids = np.random.RandomState(2).permutation(900)[:300]
    want = brute_force(tris, prims, s, mesh_of=mesh_of, filter=dict(mesh_mask=[True, True, False], ignore_prim=ignore))
    r, p, c = run(api, ds, s, count=300, ids=ids, mesh_mask=[True, True, False], ignore_prim=torch.from_numpy(ignore.view(np.int32)).cuda())
    assert r[ids].tobytes() == want[0][ids].tobytes() and p[ids].tobytes() == want[1][ids].tobytes() and c[ids].tobytes() == want[2][ids].tobytes()


def test_lists(api, base):
    """A shuffled subset with repeated ids, the count on the device: listed slots as the unlisted call, the rest untouched"""
    n = 1000
    s = base.sweeps[:n]
    want = [w[:n] for w in base.want]
    rng = np.random.RandomState(6)
    ids = rng.permutation(n)[:333]
    ids = np.concatenate([ids, ids[:7], rng.permutation(n)[:100]])           # 7 repeated ids; 100 entries beyond the count
    count = 340
    listed = np.zeros(n + TAIL, bool)
    listed[ids[:count]] = True
    out = run(api, base.ds, s, count=count, ids=ids)
    for got, w in zip(out, want):
        assert (got[~listed] == FILL).all() and got[listed].tobytes() == w[listed[:n]].tobytes()
    b = run(api, base.ds, s, count=count, ids=ids, any_hit=True)
    assert (b[~listed] == 0x7e).all() and (b[listed] == (want[0][listed[:n], 3] != NONE)).all()
    # no ids: the first `count` queries; a count beyond the arrays is clamped to them
    out = run(api, base.ds, s, count=100)
    for got, w in zip(out, want):
        assert (got[100:] == FILL).all() and got[:100].tobytes() == w[:100].tobytes()
    out = run(api, base.ds, s, count=n + 1000)
    for got, w in zip(out, want):
        assert got[:n].tobytes() == w.tobytes()
    # an empty list writes nothing
    out = run(api, base.ds, s, count=0, ids=ids)
    assert all((got == FILL).all() for got in out)
    assert (run(api, base.ds, s, count=0, any_hit=True) == 0x7e).all()


def test_a_stack_deeper_than_the_on_chip_part(api):
    """The geometric cluster of tests/test_gpu_build.py: a deep, lopsided tree whose walk needs the spill area"""
    from tests.test_gpu_build import _adversarial_scenes
    tris = _adversarial_scenes()["geometric_chain"]
    ds = api.DeviceScene.build([dict(positions=tris.reshape(-1, 3))])
    on_chip = api.lib().rtk_amd_sweep_stack_entries()
    assert ds.info()["stack_entries"] > on_chip, (ds.info()["stack_entries"], on_chip)
    rng = np.random.RandomState(4)
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    n = 128
    assert n * len(tris) < 1000000
    # long paths with a radius that keeps every box of the chain alive: from the far corner towards the cluster's dense end
    o = hi + (hi - lo) * rng.uniform(0.1, 0.5, (n, 3))
    target = lo + (hi - lo) * rng.uniform(0, 1, (n, 3)) ** 8
    s = np.zeros((n, 9), np.float32)
    s[:, 0:3], s[:, 3:6], s[:, 7] = o, target - o, RTK_INF
    s[:, 8] = rng.uniform(0, 0.05, n) * float((hi - lo).max())
    rec = check(api, ds, s)
    assert (rec["prim"] != NONE).sum() > n // 2
    # the counting form says that pushes did go past the on-chip part, and gives the same bytes
    d_rec, d_pts, d_ctr, counts = ds.sweep_spheres_counted(api.to_device(s), n)
    print("geometric_chain: stack entries %d, on chip %d, counts %s" % (ds.info()["stack_entries"], on_chip, counts))
    assert counts["stack_spills"] > 0 and counts["rays"] == n and counts["hits"] == int((rec["prim"] != NONE).sum())
    assert counts["nodes"] >= n and counts["triangles"] >= counts["leaves"] > 0
    assert d_rec.cpu().numpy().view(HIT_RECORD_DTYPE).tobytes() == rec.tobytes()
    assert api.lib().rtk_dev_trace_status(ds.handle, None) == 0


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_sizes(api, base, n):
    which = np.arange(n) % len(base.sweeps)
    out = run(api, base.ds, base.sweeps[which], n=n)
    for got, w in zip(out, base.want):
        assert got[:n].tobytes() == w[which].tobytes()
    assert (run(api, base.ds, base.sweeps[which], n=n, any_hit=True)[:n] == (base.want[0][which, 3] != NONE)).all()


def test_an_empty_scene_and_an_mgpu_scene(api, base):
    import torch
    s = base.sweeps[:200]
    empty = api.DeviceScene.build([dict(positions=np.zeros((0, 3), np.float32))])
    rec = check(api, empty, s, brute_force(np.zeros((0, 3, 3), np.float32), np.zeros(0, np.uint32), s))
    assert (rec["prim"] == NONE).all() and not run(api, empty, s, any_hit=True)[:200].any()
    L = api.lib()
    m = L.rtk_mgpu_create((C.c_int * 1)(0), 1)
    assert m, api.last_error()
    try:
        ms = api.MeshSet([dict(positions=base.positions)])
        assert L.rtk_mgpu_build(m, C.byref(ms.desc)) == 0, api.last_error()
        handle = L.rtk_mgpu_scene(m, 0)
        assert handle
        d_s = api.to_device(s)
        d_rec = torch.full((200 * 16,), 0x7e, dtype=torch.uint8, device="cuda")
        d_b = torch.full((200,), 0x7e, dtype=torch.uint8, device="cuda")
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert L.rtk_dev_sweep_spheres(handle, C.c_void_p(d_s.data_ptr()), 200, None, C.c_void_p(d_rec.data_ptr()), None, None, None, stream) == 0, api.last_error()
        assert L.rtk_dev_sweep_spheres_any(handle, C.c_void_p(d_s.data_ptr()), 200, None, C.c_void_p(d_b.data_ptr()), None, stream) == 0, api.last_error()
        assert d_rec.cpu().numpy().view(np.uint32).reshape(200, 4).tobytes() == base.want[0][:200].tobytes()   # (d_points, d_centres NULL)
        assert (d_b.cpu().numpy() == (base.want[0][:200, 3] != NONE)).all()
    finally:
        L.rtk_mgpu_destroy(m)


def test_counted_form(api, base):
    n = len(base.sweeps)
    d_rec, d_pts, d_ctr, counts = base.ds.sweep_spheres_counted(api.to_device(base.sweeps), n)
    assert counts["rays"] == n and counts["hits"] == int((base.want[0][:, 3] != NONE).sum())
    assert counts["nodes"] > 0 and counts["triangles"] >= counts["leaves"] > 0 and counts["triangles"] < n * 300
    assert d_rec.cpu().numpy().view(np.uint32).reshape(n, 4).tobytes() == base.want[0].tobytes()
    assert d_pts.cpu().numpy().view(np.uint32).reshape(n, 3).tobytes() == base.want[1].tobytes()
    assert d_ctr.cpu().numpy().view(np.uint32).reshape(n, 3).tobytes() == base.want[2].tobytes()
