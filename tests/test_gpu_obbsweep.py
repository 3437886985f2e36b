"""GPU tests of rtk_dev_sweep_obbs / _any / _counted. The bar everywhere: records, centres and normals are bit for bit what numpy
float32 brute force gives by the rule of rtk_amd/csrc/rtk_obbsweep_rule.h (tests/obbsweep_ref.py) over the triangle records the
scene holds at that moment -- read back through rtk_dev_expand_hits, so they are the scene's own --, whatever tree is above
them. Outputs are pre-filled with 0x7e and carry a tail that must stay untouched. The base scene is the 300-triangle soup of the
closest-points tests with about 1500 sweeps; every brute force stays below a million (query, triangle) pairs."""
import ctypes as C

import numpy as np
import pytest

from rtk_amd import synth
from rtk_amd.types import HIT_DTYPE, HIT_RECORD_DTYPE, RTK_INF
from tests.obbsweep_ref import NONE, brute_force, prepare

pytestmark = pytest.mark.gpu

TAIL = 5                                     # slots behind the batch that nobody may write
FILL = 0x7e7e7e7e
NOT_LIVE = 45                                # the mix ends with this many queries that are not live for the axis-aligned reasons


def scene_triangles(api, ds):
    """The scene's current triangle records by primitive id, [T, 3, 3] float32, through the expansion of made-up records"""
    n = ds.info()["num_triangles"]
    rec = np.zeros(n, HIT_RECORD_DTYPE)
    rec["prim"] = np.arange(n, dtype=np.uint32)
    d_hits, _ = ds.expand_device(api.to_device(rec), n)
    return np.ascontiguousarray(d_hits.cpu().numpy().view(HIT_DTYPE)["vertex"]["position"])


def run(api, ds, sweeps, n=None, count=None, ids=None, any_hit=False, **filt):
    """sweeps: float32 [n, 20]. -> (record words [n + TAIL, 4], centre words [n + TAIL, 3], normal words [n + TAIL, 3]) as the device
    left them, or the bytes [n + TAIL] of the any-hit form"""
    import torch
    n = len(sweeps) if n is None else n
    d_s = api.to_device(np.ascontiguousarray(sweeps, np.float32)) if len(sweeps) else torch.zeros(80, dtype=torch.uint8, device="cuda")
    d_count = torch.tensor([count], dtype=torch.int64, device="cuda") if count is not None else None
    d_ids = torch.from_numpy(np.ascontiguousarray(ids, np.int64)).cuda() if ids is not None else None
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if any_hit:
        d_b = torch.full((n + TAIL,), 0x7e, dtype=torch.uint8, device="cuda")
        ds.sweep_obbs_any_device(d_s, n, d_b, count=d_count, ids=d_ids, **filt)
        assert api.lib().rtk_dev_trace_status(ds.handle, stream) == 0, api.last_error()
        b = d_b.cpu().numpy()
        assert (b[n:] == 0x7e).all(), "written beyond num_sweeps"
        return b
    d_rec = torch.full(((n + TAIL) * 16,), 0x7e, dtype=torch.uint8, device="cuda")
    d_ctr = torch.full(((n + TAIL) * 12,), 0x7e, dtype=torch.uint8, device="cuda")
    d_nrm = torch.full(((n + TAIL) * 12,), 0x7e, dtype=torch.uint8, device="cuda")
    ds.sweep_obbs_device(d_s, n, d_rec, d_ctr, d_nrm, count=d_count, ids=d_ids, **filt)
    assert api.lib().rtk_dev_trace_status(ds.handle, stream) == 0, api.last_error()
    rec = d_rec.cpu().numpy().view(np.uint32).reshape(n + TAIL, 4)
    ctr = d_ctr.cpu().numpy().view(np.uint32).reshape(n + TAIL, 3)
    nrm = d_nrm.cpu().numpy().view(np.uint32).reshape(n + TAIL, 3)
    assert (rec[n:] == FILL).all() and (ctr[n:] == FILL).all() and (nrm[n:] == FILL).all(), "written beyond num_sweeps"
    return rec, ctr, nrm


def check(api, ds, sweeps, want=None, **filt):
    """the whole batch against brute force over the scene's own records (or the reference given); returns the records"""
    if want is None:
        tris = scene_triangles(api, ds)
        want = brute_force(tris, np.arange(len(tris), dtype=np.uint32), sweeps)
    want_rec, want_ctr, want_nrm = want
    rec, ctr, nrm = run(api, ds, sweeps, **filt)
    n = len(sweeps)
    bad = np.nonzero((rec[:n] != want_rec).any(1) | (ctr[:n] != want_ctr).any(1) | (nrm[:n] != want_nrm).any(1))[0]
    assert len(bad) == 0, (len(bad), bad[:5], sweeps[bad[:5]], rec[bad[:5]], want_rec[bad[:5]], ctr[bad[:5]], want_ctr[bad[:5]], nrm[bad[:5]], want_nrm[bad[:5]])
    return rec[:n].copy().view(HIT_RECORD_DTYPE).reshape(n)


def quat_rows(q):
    """quaternions (x, y, z, w) [n, 4] -> [n, 3, 3] float64 whose ROWS are the images of the unit vectors: the box's axes"""
    q = np.asarray(q, np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    x, y, z, w = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                  2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)
    return R.transpose(0, 2, 1)


def rotations(rng, n):
    """One rotation per query as quaternions [n, 4]: random (rows 0 mod 4), identity (1 mod 4), 45 degrees about one axis (2 mod
    4), random again (3 mod 4)"""
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    k = np.arange(n)
    q[k % 4 == 1] = [0.0, 0.0, 0.0, 1.0]
    turn = np.nonzero(k % 4 == 2)[0]
    q[turn] = 0.0
    q[turn, (turn // 4) % 3] = np.sin(np.pi / 8)
    q[turn, 3] = np.cos(np.pi / 8)
    return q


def sweep_mix(tris, seed=11):
    """tests/test_gpu_boxsweep.py's mix with a rotation per query, float32 [n, 20], and the quaternions the axes were made from:
    paths through the scene's box and beside it, starts on and inside the surface, half extents from 0 to a fifth of the extent (a
    seventh of the boxes are points, a fifth are flat on one axis, a fifth are needles along one), max_t around the true time,
    RTK_INF, queries that are not live; a twentieth of the first 1210 have axes that are not orthonormal."""
    rng = np.random.RandomState(seed)
    tris = np.asarray(tris, np.float32).reshape(-1, 3, 3)
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    ext = hi - lo
    size = float(ext.max())
    prims = np.arange(len(tris), dtype=np.uint32)

    def rows(o, d, h, max_t=RTK_INF, min_t=0.0):
        n = len(o)
        s = np.zeros((n, 20), np.float32)
        s[:, 0:3], s[:, 3:6], s[:, 8:11] = o, d, h
        s[:, 6], s[:, 7] = min_t, max_t
        return s

    def radii(n):
        h = (rng.uniform(0, 1, (n, 3)) ** 2 * 0.2 * size) * (rng.uniform(0, 1, (n, 1)) > 0.15)      # (a seventh: a point)
        kind, axis = rng.randint(0, 5, n), rng.randint(0, 3, n)
        flat, needle = np.nonzero(kind == 0)[0], np.nonzero(kind == 1)[0]
        h[flat, axis[flat]] = 0.0                                            # a rectangle
        h[needle, (axis[needle] + 1) % 3] = 0.0                              # a segment
        h[needle, (axis[needle] + 2) % 3] = 0.0
        return h
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
    quat = rotations(rng, len(mix))
    axes = quat_rows(quat)
    # a twentieth not orthonormal: scaled, sheared, a zero row, two equal rows
    off = np.arange(7, len(mix), 20)
    axes[off[0::4], 0] *= 1.1
    axes[off[1::4], 1] += 0.2 * axes[off[1::4], 2]
    axes[off[2::4], 2] = 0.0
    axes[off[3::4], 1] = axes[off[3::4], 0]
    mix[:, 11:20] = axes.reshape(-1, 9)
    # max_t at the float32 neighbour below the true time, at it (the interval is closed: still a hit) and above it
    through = brute_force(tris, prims, mix[:500])[0]
    some = np.nonzero(through[:, 3] != NONE)[0][:80]
    assert len(some) == 80
    true_t = through[some, 0].view(np.float32)
    parts, quats = [mix], [quat]
    for t in (np.nextafter(true_t, np.float32(-np.inf)), true_t, np.nextafter(true_t, np.float32(np.inf))):
        s = mix[some].copy(); s[:, 7] = t
        parts.append(s); quats.append(quat[some])
    # the same three with min_t < 0 and a start inside the grown box of the triangle that is hit (a cube a little more than its
    # reach above a face, moving towards it): the entry time te is negative and larger than the time, so max_t - te rounds
    # coarsely, and a time an ulp beyond max_t must become a miss (2. (iii) of the rule)
    pick = rng.permutation(len(tris))[:240]
    a, b, c = (tris[pick, k].astype(np.float64) for k in range(3))
    nrm = np.cross(b - a, c - a); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    r = rng.uniform(0.005, 0.05, 240) * size
    nq = rotations(rng, 240)
    U = quat_rows(nq)
    reach = (np.abs(np.einsum("njk,nk->nj", U, nrm)) * r[:, None]).sum(1)      # of the cube along the triangle's normal
    o = (a + b + c) / 3 + nrm * (reach * rng.uniform(1.05, 1.5, 240))[:, None]
    d = -nrm * size * rng.uniform(0.5, 2.0, (240, 1)) + rng.standard_normal((240, 3)) * 0.1 * size
    near = rows(o, d, r[:, None], min_t=-rng.uniform(0.05, 0.5, 240))
    near[:, 11:20] = U.reshape(-1, 9)
    rec = brute_force(tris, prims, near)[0]
    some = np.nonzero((rec[:, 3] != NONE) & (rec[:, 0].view(np.float32) > 0))[0][:30]
    assert len(some) == 30
    true_t = rec[some, 0].view(np.float32)
    for t in (np.nextafter(true_t, np.float32(-np.inf)), true_t, np.nextafter(true_t, np.float32(np.inf))):
        s = near[some].copy(); s[:, 7] = t
        parts.append(s); quats.append(nq[some])
    # not live: NaN and infinities in every field, a negative half extent, a zero direction, min_t > max_t
    which = rng.permutation(500)[:NOT_LIVE]
    bad = mix[which].copy()
    bad[np.arange(27), (np.arange(27) * 3) % 20] = np.array([np.nan, np.inf, -np.inf], np.float32)[np.arange(27) // 9]
    bad[np.arange(27, 33), 8 + np.arange(6) % 3] = -0.01 * size
    bad[33:39, 3:6] = 0.0
    bad[39:45, 6], bad[39:45, 7] = 2.0, 1.0
    parts.append(bad); quats.append(quat[which])
    return np.concatenate(parts).astype(np.float32), np.concatenate(quats)


@pytest.fixture(scope="module")
def base(api):
    class Base:
        pass
    b = Base()
    b.positions = synth.triangle_soup(300, 0.2, seed=5)
    b.tris = b.positions.reshape(300, 3, 3)
    b.ds = api.DeviceScene.build([dict(positions=b.positions)])
    b.sweeps, b.quat = sweep_mix(b.tris)
    # the reference, computed once and shared
    b.want = brute_force(b.tris, np.arange(300, dtype=np.uint32), b.sweeps)
    return b


def test_sweep_mix_equals_brute_force(api, base):
    assert scene_triangles(api, base.ds).tobytes() == base.tris.tobytes()     # (the records are the input's, in input order)
    n = len(base.sweeps)
    assert 1400 <= n <= 1600 and n * 300 < 1000000
    # what the numpy reference alone shows for these inputs, before the GPU is asked: the hit share, starts that touch, the
    # rotations, the queries that are not live, the closed interval
    want_rec = base.want[0].copy().view(HIT_RECORD_DTYPE).reshape(n)
    want_hit = want_rec["prim"] != NONE
    live = prepare(base.sweeps).live
    print("sweeps %d, hits by the reference %.3f, live %d" % (n, want_hit.mean(), live.sum()))
    assert 0.5 < want_hit.mean() < 0.9
    assert (want_rec["t"][want_hit] == base.sweeps[want_hit, 6]).sum() >= 100     # a hit at min_t: the start touches
    gate = np.arange(7, 1210, 20)
    assert len(gate) >= 1210 // 20 and not live[gate].any() and not want_hit[gate].any() and live[:1210].sum() == 1210 - len(gate)
    assert not live[n - NOT_LIVE:].any() and live[1210:n - NOT_LIVE].all()
    ident = (base.sweeps[:, 11:20] == np.eye(3, dtype=np.float32).reshape(9)).all(1)
    assert ident.sum() > 250 and (want_hit & ident).sum() > 100 and (want_hit & ~ident).sum() > 500
    k = n - NOT_LIVE - 90 - 240
    wb, wa, wo = want_rec[k:k + 80], want_rec[k + 80:k + 160], want_rec[k + 160:k + 240]
    assert (wb["prim"] == NONE).all() and (wo["prim"] != NONE).sum() >= 70 and 20 <= (wa["prim"] != NONE).sum() <= 80
    assert (wa["t"][wa["prim"] != NONE] == base.sweeps[k + 80:k + 160, 7][wa["prim"] != NONE]).all()
    k = n - NOT_LIVE - 90
    assert (base.sweeps[k:k + 90, 6] < 0).all()
    wb, wa, wo = want_rec[k:k + 30], want_rec[k + 30:k + 60], want_rec[k + 60:k + 90]
    assert (wb["prim"] == NONE).all() and (wo["prim"] != NONE).sum() >= 25 and 8 <= (wa["prim"] != NONE).sum() <= 30
    assert (wa["t"][wa["prim"] != NONE] == base.sweeps[k + 30:k + 60, 7][wa["prim"] != NONE]).all()
    # the normals of the reference: unit length against the motion, or zero; never a NaN; zero for every miss and every hit at
    # min_t (an overlap at the start), and for nothing else but an axis without a length
    want_nrm = base.want[2].view(np.float32)
    length = np.linalg.norm(want_nrm.astype(np.float64), axis=1)
    assert not np.isnan(want_nrm).any() and ((np.abs(length - 1) < 1e-6) | (length == 0)).all()
    assert (length[~want_hit] == 0).all() and (length[want_hit & (want_rec["t"] == base.sweeps[:, 6])] == 0).all()
    later = want_hit & (want_rec["t"] > base.sweeps[:, 6])
    assert later.sum() > 300 and (length[later] > 0).mean() > 0.99
    assert ((want_nrm[length > 0].astype(np.float64) * base.sweeps[length > 0, 3:6]).sum(1) < 0).all()
    # the GPU: the same words
    rec = check(api, base.ds, base.sweeps, base.want)
    hit = rec["prim"] != NONE
    assert (rec["u"][~hit] == 0).all() and (rec["v"][~hit] == 0).all() and (rec["t"][~hit].view(np.uint32) == base.sweeps[~hit, 7].view(np.uint32)).all()
    # no record, hit or miss, has a time outside [min_t, max_t]
    ok = live & (base.sweeps[:, 6] <= base.sweeps[:, 7])
    assert (rec["t"][ok] >= base.sweeps[ok, 6]).all() and (rec["t"][ok] <= base.sweeps[ok, 7]).all()
    # the numpy conveniences on top of it: the same bytes, from matrices and from the quaternions they were made from
    plain = np.nonzero((base.sweeps[:, 6] == 0) & (base.sweeps[:, 7] == RTK_INF) & live)[0][:400]
    s, quat = base.sweeps[plain], base.quat[plain]
    for rotation in (s[:, 11:20].reshape(-1, 3, 3), quat, quat * 2.5):
        rec2, ctr2, nrm2 = base.ds.sweep_obbs(s[:, 0:3], s[:, 3:6], s[:, 8:11], rotation)
        assert rec2.tobytes() == rec[plain].tobytes() and ctr2.shape == (len(plain), 3) and nrm2.shape == (len(plain), 3)
        assert ctr2.view(np.uint32).tobytes() == base.want[1][plain].tobytes() and nrm2.view(np.uint32).tobytes() == base.want[2][plain].tobytes()
        blocked = base.ds.obb_path_blocked(s[:, 0:3], s[:, 3:6], s[:, 8:11], rotation)
        assert blocked.dtype == bool and (blocked == (rec2["prim"] != NONE)).all()
    one = quat_rows(quat[:1])[0]
    rec3, _, _ = base.ds.sweep_obbs(s[:50, 0:3], s[:50, 3:6], 0.01, one, max_t=0.5, min_t=-0.25)
    s3 = s[:50].copy(); s3[:, 6], s3[:, 7], s3[:, 8:11], s3[:, 11:20] = -0.25, 0.5, 0.01, one.reshape(9)
    assert rec3.view(np.uint32).reshape(-1, 4).tobytes() == brute_force(base.tris, np.arange(300), s3)[0].tobytes()
    rec4, _, _ = base.ds.sweep_obbs(s[:50, 0:3], s[:50, 3:6], 0.01, quat[0], max_t=0.5, min_t=-0.25)
    assert rec4.tobytes() == rec3.tobytes()


def test_a_scene_of_one_triangle(api, base):
    tri = base.positions[:3]
    ds = api.DeviceScene.build([dict(positions=tri)])
    want = brute_force(tri.reshape(1, 3, 3), np.zeros(1, np.uint32), base.sweeps)
    rec = check(api, ds, base.sweeps, want)
    assert 0 < (rec["prim"] == 0).sum() < len(rec) and np.isin(rec["prim"], [0, NONE]).all()


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
    split = up.split_leaves(1)
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
        want = brute_force(tris, prims, s, mesh_of=mesh_of, mesh_mask=mask)
        got = check(api, ds, s, want, mesh_mask=mask)
        h = got["prim"] != NONE
        assert all(mask[m] for m in np.unique(mesh_of[got["prim"][h]])) and (h.any() or not any(mask))
        assert (run(api, ds, s, any_hit=True, mesh_mask=mask)[:900] == h).all()
    got = check(api, ds, s, brute_force(tris, prims, s, mesh_of=mesh_of, mesh_mask=[False, True, True]), mesh_mask=[False, True, True])
    assert (got["prim"][got["prim"] != NONE] >= 150).all() and (got["prim"] >= 300).sum() > 50 and (got["prim"] != rec["prim"]).any()
    # ignore_prim per query slot: every query ignores the triangle it would hit; then its twin or the next one is found
    ignore = rec["prim"].copy()
    want = brute_force(tris, prims, s, ignore_prim=ignore)
    got = check(api, ds, s, want, ignore_prim=ignore)
    assert (got["prim"][hit] != rec["prim"][hit]).all() and (got["prim"][hit & (rec["prim"] < 150)] != NONE).all()    # (at least its twin is left)
    assert (got["prim"][hit & (rec["prim"] < 150)] == rec["prim"][hit & (rec["prim"] < 150)] + 300).sum() > 100
    assert got[~hit].tobytes() == rec[~hit].tobytes()
    # both at once, with a list: the filter array is read at the query's own slot
    import torch
    ids = np.random.RandomState(2).permutation(900)[:300]
    want = brute_force(tris, prims, s, mesh_of=mesh_of, mesh_mask=[True, True, False], ignore_prim=ignore)
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
    # a count equal to the arrays' length, without ids and with every id once in a shuffled order: the unlisted call's words
    # (run() itself checks that the tail behind slot n keeps its fill)
    for ids_n in (None, rng.permutation(n)):
        out = run(api, base.ds, s, count=n, ids=ids_n)
        for got, w in zip(out, want):
            assert got[:n].tobytes() == w.tobytes()
        b = run(api, base.ds, s, count=n, ids=ids_n, any_hit=True)
        assert (b[:n] == (want[0][:, 3] != NONE)).all()
    # an empty list writes nothing
    out = run(api, base.ds, s, count=0, ids=ids)
    assert all((got == FILL).all() for got in out)
    assert (run(api, base.ds, s, count=0, any_hit=True) == 0x7e).all()


def test_a_stack_deeper_than_the_on_chip_part(api):
    """The geometric cluster of tests/test_gpu_build.py: a deep, lopsided tree whose walk needs the spill area"""
    from tests.test_gpu_build import _adversarial_scenes
    tris = _adversarial_scenes()["geometric_chain"]
    ds = api.DeviceScene.build([dict(positions=tris.reshape(-1, 3))])
    on_chip = api.lib().rtk_amd_obbsweep_stack_entries()
    assert ds.info()["stack_entries"] > on_chip, (ds.info()["stack_entries"], on_chip)
    rng = np.random.RandomState(4)
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    n = 128
    assert n * len(tris) < 1000000
    # long paths with half extents that keep every box of the chain alive: from the far corner towards the cluster's dense end
    o = hi + (hi - lo) * rng.uniform(0.1, 0.5, (n, 3))
    target = lo + (hi - lo) * rng.uniform(0, 1, (n, 3)) ** 8
    s = np.zeros((n, 20), np.float32)
    s[:, 0:3], s[:, 3:6], s[:, 7] = o, target - o, RTK_INF
    s[:, 8:11] = rng.uniform(0, 0.05, (n, 3)) * float((hi - lo).max())
    s[:, 11:20] = quat_rows(rotations(rng, n)).reshape(-1, 9)
    rec = check(api, ds, s)
    assert (rec["prim"] != NONE).sum() > n // 2
    # the counting form says that pushes did go past the on-chip part, and gives the same bytes
    d_rec, d_ctr, d_nrm, counts = ds.sweep_obbs_counted(api.to_device(s), n)
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
        assert L.rtk_dev_sweep_obbs(handle, C.c_void_p(d_s.data_ptr()), 200, None, C.c_void_p(d_rec.data_ptr()), None, None, None, stream) == 0, api.last_error()
        assert L.rtk_dev_sweep_obbs_any(handle, C.c_void_p(d_s.data_ptr()), 200, None, C.c_void_p(d_b.data_ptr()), None, stream) == 0, api.last_error()
        assert d_rec.cpu().numpy().view(np.uint32).reshape(200, 4).tobytes() == base.want[0][:200].tobytes()   # (d_centres, d_normals NULL)
        assert (d_b.cpu().numpy() == (base.want[0][:200, 3] != NONE)).all()
    finally:
        L.rtk_mgpu_destroy(m)


def test_counted_form(api, base):
    n = len(base.sweeps)
    d_rec, d_ctr, d_nrm, counts = base.ds.sweep_obbs_counted(api.to_device(base.sweeps), n)
    assert counts["rays"] == n and counts["hits"] == int((base.want[0][:, 3] != NONE).sum())
    assert counts["nodes"] > 0 and counts["triangles"] >= counts["leaves"] > 0 and counts["triangles"] < n * 300
    assert d_rec.cpu().numpy().view(np.uint32).reshape(n, 4).tobytes() == base.want[0].tobytes()
    assert d_ctr.cpu().numpy().view(np.uint32).reshape(n, 3).tobytes() == base.want[1].tobytes()
    assert d_nrm.cpu().numpy().view(np.uint32).reshape(n, 3).tobytes() == base.want[2].tobytes()
