"""GPU tests of rtk_dev_trace_rays_count / rtk_dev_trace_rays_all. The bar everywhere is equality over ALL rays of a case: counts,
records (bytes) and `written` equal what the oracle's reject-all callback is offered on the same blob, sorted by (t, prim)
(tests/allhits_ref.py; the fixtures themselves are pinned on the CPU in tests/test_allhits_cpu.py). Record buffers are pre-filled
with 0x7e and carry a guard band behind the last segment that nobody may write."""
import ctypes as C
import os

import numpy as np
import pytest

from rtk_amd import synth
from rtk_amd.types import HIT_RECORD_DTYPE, RTK_INF
from tests import allhits_ref as R
from tests.util import group_redo_cases

pytestmark = pytest.mark.gpu

GUARD = 7
FILL = 0x7e7e7e7e
REDO_CASES = [c.name for c in group_redo_cases(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))]


def status_ok(api, ds):
    import torch
    return api.lib().rtk_dev_trace_status(ds.handle, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0


def check_all(api, ds, rays, want, **filters):
    """count, then count + prefix sum + fill: everything equals the reference"""
    counts = ds.count_hits(rays, **filters)
    bad = np.nonzero(counts != want.counts)[0]
    assert bad.size == 0, "counts differ on %d rays, first %s: %s vs %s" % (bad.size, bad[:8], counts[bad[:8]], want.counts[bad[:8]])
    offsets, records, written = ds.trace_all(rays, **filters)
    assert (offsets == want.offsets).all() and (written == want.counts).all()
    assert records.tobytes() == want.records.tobytes()
    return records


def fill(api, ds, rays, offsets, flt=None, opts=None):
    """rtk_dev_trace_rays_all into a 0x7e-filled buffer with a guard band -> (records [offsets[-1]], written [n]) as the device left them"""
    import torch
    n, total = len(rays), int(offsets[-1])
    d_rec = torch.full(((total + GUARD) * 16,), 0x7e, dtype=torch.uint8, device="cuda")
    d_wr = torch.full((n + GUARD,), FILL, dtype=torch.int32, device="cuda")
    d_off = torch.from_numpy(np.ascontiguousarray(offsets, np.int64)).cuda()
    ds.trace_all_device(api.to_device(rays), n, d_off, d_rec, d_wr, filter=flt, opts=opts)
    assert status_ok(api, ds), api.last_error()
    rec = d_rec.cpu().numpy().view(HIT_RECORD_DTYPE)
    wr = d_wr.cpu().numpy().view(np.uint32)
    assert (rec[total:].view(np.uint32) == FILL).all() and (wr[n:] == FILL).all(), "written behind the last segment"
    return rec[:total], wr[:n]


def check_room(api, ds, rays, want, room):
    """segments of `room[i]` records: the first min(count, room) of the full list, `written` says how many, the rest of a segment is untouched"""
    off, recs, written = want.first(room)
    exp = np.full(int(off[-1]) * 16, 0x7e, np.uint8).view(HIT_RECORD_DTYPE)
    for i, r in enumerate(recs):
        exp[off[i]:off[i] + len(r)] = r
    rec, wr = fill(api, ds, rays, off)
    assert (wr == written).all()
    bad = np.nonzero((rec.view(np.uint32).reshape(-1, 4) != exp.view(np.uint32).reshape(-1, 4)).any(1))[0]
    assert bad.size == 0, "%d records differ, first %s" % (bad.size, bad[:8])


class Scene:
    def __init__(self, api, oracle, ds, blob=None):
        self.ds = ds
        self.blob = blob if blob is not None else oracle.Blob(ds.export_blob())
        self.base = ds.mesh_base()


# ---------------------------------------------------------------- 1. sheets

@pytest.mark.parametrize("how", ["device_built", "uploaded"])
def test_sheets(api, oracle, how):
    """24 parallel squares, 3 meshes: 24 crossings in t order on generic rays; exact zeros on the diagonal and corner rays, in
    partial groups (device build: leaves of at most 3) and in full groups (the oracle's builder: leaves of 4 to 63)"""
    meshes = R.sheets_meshes()
    rays, generic = R.sheets_rays()
    if how == "device_built":
        s = Scene(api, oracle, api.DeviceScene.build(meshes))
        assert s.ds.info()["num_nodes"] >= 4
    else:
        blob = oracle.build_scene(meshes)
        s = Scene(api, oracle, api.DeviceScene.upload(blob), blob)
        assert 3 * oracle.validate_blob(blob)[1]["leaves"] < 48
    want = R.oracle_lists(oracle, s.blob, rays, s.base)
    assert (want.counts[generic] == R.SHEETS).all() and (want.counts[~generic] > R.SHEETS).any()
    rec = check_all(api, s.ds, rays, want)
    first = rec[want.offsets[0]:want.offsets[1]]
    assert (np.diff(first["t"]) > 0).all()


# ---------------------------------------------------------------- 2 - 6. soup

@pytest.fixture(scope="module")
def soup(api, oracle):
    s = Scene(api, oracle, api.DeviceScene.build(R.soup_meshes()))
    s.rays = R.soup_rays()
    assert len(s.rays) == 4097 and list(s.base) == [0, 1000, 2000, 3000]
    s.want = R.oracle_lists(oracle, s.blob, s.rays, s.base)
    print("soup: mean %.2f, max %d candidates per ray, %d rays without" % (s.want.counts.mean(), s.want.counts.max(), (s.want.counts == 0).sum()))
    assert s.want.counts.max() >= 8 and (s.want.counts == 0).any() and s.want.counts.mean() >= 2
    return s


def test_soup_counts_and_lists(api, soup):
    rec = check_all(api, soup.ds, soup.rays, soup.want)
    exact = api.make_opts(exact_nodes=True)
    assert ((soup.want.counts > 0) == soup.ds.trace_any(soup.rays, opts=exact)).all()
    closest = soup.ds.trace(soup.rays, opts=exact, full=False)
    hit = soup.want.counts > 0
    assert ((closest["prim"] != R.NONE) == hit).all()
    assert closest[hit].tobytes() == rec[soup.want.offsets[:-1][hit]].tobytes()
    assert check_all(api, soup.ds, soup.rays, soup.want).tobytes() == rec.tobytes()       # two runs, the same bytes


@pytest.mark.parametrize("k", [1, 4, 5])
def test_k_closest(api, soup, k):
    check_room(api, soup.ds, soup.rays, soup.want, k)


def test_ragged_room(api, soup):
    room = np.random.RandomState(41).randint(0, 7, len(soup.rays))
    assert (room == 0).any() and (room < soup.want.counts).any() and (room > soup.want.counts).any()
    check_room(api, soup.ds, soup.rays, soup.want, room)


def test_filters(api, oracle, soup):
    rays, want, n = soup.rays, soup.want, len(soup.rays)
    vis = [True, False, True]
    masked = R.oracle_lists(oracle, soup.blob, rays, soup.base, mesh_mask=vis)
    assert 0 < masked.counts.sum() < want.counts.sum()
    check_all(api, soup.ds, rays, masked, mesh_mask=vis)
    ignore = np.full(n, R.NONE, np.uint32)
    after = np.zeros(n, HIT_RECORD_DTYPE)
    after["prim"] = R.NONE
    for i in range(n):
        l = want.of(i)
        if len(l) >= 1:
            ignore[i] = l[len(l) // 2]["prim"]
        if len(l) >= 3:
            after[i] = l[2]
    check_all(api, soup.ds, rays, R.oracle_lists(oracle, soup.blob, rays, soup.base, ignore_prim=ignore), ignore_prim=ignore)
    paged = R.oracle_lists(oracle, soup.blob, rays, soup.base, after=after)
    rec = check_all(api, soup.ds, rays, paged, after=after)
    tail = np.concatenate([want.of(i)[3:] if want.counts[i] >= 3 else want.of(i) for i in range(n)])
    assert rec.tobytes() == tail.tobytes()                                 # the list from the fourth record on
    # all three at once
    every = R.oracle_lists(oracle, soup.blob, rays, soup.base, mesh_mask=vis, ignore_prim=ignore, after=after)
    check_all(api, soup.ds, rays, every, mesh_mask=vis, ignore_prim=ignore, after=after)


def test_after_chain_enumerates_the_same_list(api, soup):
    """the route there was before: one filtered closest-hit walk per candidate, fed back through d_after, on 256 rays"""
    rays, want = soup.rays[:256], soup.want
    prev = np.zeros(256, HIT_RECORD_DTYPE)
    prev["prim"] = R.NONE
    got = [[] for _ in range(256)]
    for _ in range(int(want.counts[:256].max()) + 1):
        rec = soup.ds.trace_filtered(rays, after=prev, opts=api.make_opts(exact_nodes=True))
        live = rec["prim"] != R.NONE
        if not live.any():
            break
        for i in np.nonzero(live)[0]:
            got[i].append(rec[i])
        # a finished ray keeps paging behind its last record and keeps missing
        prev = prev.copy()
        prev[live] = rec[live]
    else:
        raise AssertionError("the chain did not end")
    for i in range(256):
        assert np.array(got[i], HIT_RECORD_DTYPE).tobytes() == want.of(i).tobytes(), i


@pytest.mark.parametrize("n", [0, 1, 63, 65])
def test_sizes(api, soup, n):
    import torch
    rays = soup.rays[:n]
    if n == 0:
        assert len(soup.ds.count_hits(rays)) == 0 and len(soup.ds.trace_all(rays)[1]) == 0
        d = torch.zeros(64, dtype=torch.uint8, device="cuda")
        assert api.lib().rtk_dev_trace_rays_count(soup.ds.handle, None, 0, None, None, None, None) == 0
        assert api.lib().rtk_dev_trace_rays_all(soup.ds.handle, C.c_void_p(d.data_ptr()), 0, None, None, None, None, None, None) == 0
        return
    sub = R.Lists([[(r["t"], int(r["prim"]), r["u"], r["v"]) for r in soup.want.of(i)] for i in range(n)])
    check_all(api, soup.ds, rays, sub)
    check_room(api, soup.ds, rays, sub, 2)


# ---------------------------------------------------------------- 7. special rays

@pytest.mark.parametrize("how", ["uploaded", "device_built"])
def test_exotic_rays(api, oracle, how):
    """synth.rays_exotic on the 10k-triangle scene of tests/golden/exotic_rays.npz (zeros, negative zeros, denormals, huge and tied
    direction components, NaN-min and empty intervals): the SSE-operand-order form of the slab test, beside ordinary rays in a wave"""
    tris = synth.scene_for_config(1)
    rays = synth.rays_exotic(2048, tris=tris)
    if how == "uploaded":
        blob = oracle.build_scene([dict(positions=tris)])
        s = Scene(api, oracle, api.DeviceScene.upload(blob), blob)
    else:
        s = Scene(api, oracle, api.DeviceScene.build([dict(positions=tris)]))
    want = R.oracle_lists(oracle, s.blob, rays, s.base)
    assert (want.counts > 0).sum() > 300
    check_all(api, s.ds, rays, want)
    assert status_ok(api, s.ds)


@pytest.mark.parametrize("name", REDO_CASES)
def test_group_redo_leaves(api, oracle, golden_dir, name):
    """tests/golden/group_redo.npz: single leaves of 4 .. 63 triangles, rays that start bit-exactly on a vertex of one triangle, so
    one FULL group has an exact zero and is evaluated in double, the others in float: 756 rays, more than one workgroup"""
    c = [k for k in group_redo_cases(golden_dir) if k.name == name][0]
    blob = c.blob(oracle)
    s = Scene(api, oracle, api.DeviceScene.upload(blob), blob)
    rays = np.ascontiguousarray(np.tile(c.rays, 3))
    want = R.oracle_lists(oracle, blob, rays, s.base)
    assert want.counts.sum() > len(rays) // 2
    check_all(api, s.ds, rays, want)
    check_room(api, s.ds, rays, want, 1)


# ---------------------------------------------------------------- 8. deep stack

def test_a_stack_deeper_than_the_on_chip_part(api, oracle):
    """Centroids on the geometric sequences of test_gpu_build's geometric_chain (a deep, lopsided Morton tree), but every
    triangle is a large sheet around the line x = y = 0.3: a ray along that line enters every box of every level, so every
    sibling waits on the stack, up to 3 entries per level (measured: depth 18, 55 stack entries against 30 on chip). The precondition is
    that the scene needs more entries than are held on chip; the entries come back in the lists, and no push was dropped."""
    on_chip = api.lib().rtk_amd_allhits_stack_entries()
    k = np.arange(1200)
    cc = np.stack([0.5 ** (k % 40 + 1) * (1 + (k // 40) * 1e-3), 0.5 ** ((k * 7) % 40 + 1), 0.5 ** ((k * 13) % 40 + 1) * (1 + (k // 40) * 1e-3)], 1).astype(np.float32)
    big = np.float32(2.0)
    tris = np.stack([cc + big * np.float32([-1, -1, 0]), cc + big * np.float32([1, -1, 0]), cc + big * np.float32([0, 2, 0])], 1).astype(np.float32)
    s = Scene(api, oracle, api.DeviceScene.build([dict(positions=tris.reshape(-1, 3))]))
    info = s.ds.info()
    print("deep scene: depth %d, stack entries %d, on chip %d" % (info["max_depth"], info["stack_entries"], on_chip))
    assert info["stack_entries"] > on_chip, (info, on_chip)
    rng = np.random.RandomState(8)
    o = np.concatenate([rng.uniform(0.25, 0.35, (70, 2)), np.full((70, 1), -1.0)], 1).astype(np.float32)
    rays = R.make_rays(o, (0, 0, 1))
    rays["direction"][35:] = (0.01, -0.02, 1)
    want = R.oracle_lists(oracle, s.blob, rays, s.base)
    assert (want.counts >= 1000).all()
    check_all(api, s.ds, rays, want)
    check_room(api, s.ds, rays, want, 5)
    assert status_ok(api, s.ds)


# ---------------------------------------------------------------- 9. after a change

def test_after_split_and_refit(api, oracle, soup):
    meshes = R.soup_meshes()
    blob = oracle.build_scene(meshes)
    ds = api.DeviceScene.upload(blob)
    rays = soup.rays[:1500]
    base = ds.mesh_base()
    check_all(api, ds, rays, R.oracle_lists(oracle, blob, rays, base))
    assert ds.split_leaves()["leaves_split"] > 0
    check_all(api, ds, rays, R.oracle_lists(oracle, oracle.Blob(ds.export_blob()), rays, base))
    # build, move every vertex, refit
    ds2 = api.DeviceScene.build(meshes)
    rng = np.random.RandomState(9)
    moved = [dict(positions=(m["positions"] + rng.uniform(-0.03, 0.03, m["positions"].shape)).astype(np.float32)) for m in meshes]
    ds2.refit(moved)
    want = R.oracle_lists(oracle, oracle.Blob(ds2.export_blob()), rays, base)
    assert want.records.tobytes() != soup.want.records[:len(want.records)].tobytes()
    check_all(api, ds2, rays, want)


# ---------------------------------------------------------------- 10. contains

def test_contains(api, oracle):
    s = Scene(api, oracle, api.DeviceScene.build(R.box_mesh()))
    pts, inside = R.box_points()
    want = R.oracle_lists(oracle, s.blob, R.make_rays(pts, R.CONTAINS_DIRECTION), s.base)
    got = s.ds.contains(pts)
    assert (got == (want.counts & 1).astype(bool)).all()
    assert (got == inside).all()
