"""GPU tests of rtk_dev_winding_numbers and the table of moments behind it. A winding number is a sum whose order follows the
tree, so the bar is a tolerance, not bits (rtk_amd/csrc/rtk_winding_rule.h "WHAT IS PROMISED"): the exact form against the float64
sum of tests/winding_ref.py within 4 x the error measured once (profiles/winding_accuracy.log; never more than 1e-3), the fast
form against the exact one within 2 x the measured difference, and the side of 0.5 of every test point. Query points keep 5 % of
the shape's size away from every triangle. Outputs are pre-filled with 0x7e and carry a tail that must stay untouched.
With RTK_AMD_WINDING_LOG=<file> the measured figures are appended to that file: that is how the log in profiles/ was made."""
import ctypes as C
import os

import numpy as np
import pytest

from rtk_amd.types import POINT_QUERY_DTYPE
from tests import winding_ref
from tests.sign_ref import F, RTK_INF, TILT, distance64, l_prism, plus_shape, torus, torus_inside
from tests.winding_ref import NAN_BITS, brute64, fixtures, icosphere, open_cube, query_points

pytestmark = pytest.mark.gpu

TAIL, FILL = 5, 0x7e7e7e7e
ERR_BAD_ARG, ERR_UNSUPPORTED = -2, -6
CEILING = 1e-3                              # no asserted bound of the exact form may exceed it: 500 x below the 0.5 that decides inside

# The largest |exact form - float64| per case, as measured once on an MI355X (profiles/winding_accuracy.log); 4 x it is asserted.
MEASURED_EXACT = {"torus": 2.396e-05, "L": 4.742e-06, "plus": 8.464e-06, "icosphere": 2.372e-05, "open cube": 2.208e-06,
                  "torus uploaded": 2.396e-05, "two placed tori": 1.800e-05, "one triangle": 2.728e-07, "two triangles": 5.664e-07,
                  "nested icospheres": 4.554e-05, "flipped icosphere": 2.360e-05, "deep chain": 1.133e-07}
# The largest |fast form - exact form| per (beta, case), from the same log; 2 x it is asserted. (0: no far term is ever taken
# for these points -- every cluster is within beta * R of them -- and the fast form is the exact one, bit for bit.)
MEASURED_FAST = {(2.0, "torus"): 2.815e-02, (4.0, "torus"): 6.910e-03, (2.0, "L"): 3.601e-03, (4.0, "L"): 1.172e-04,
                 (2.0, "plus"): 5.724e-03, (4.0, "plus"): 1.329e-04, (2.0, "icosphere"): 2.046e-02, (4.0, "icosphere"): 3.948e-03,
                 (2.0, "open cube"): 3.139e-03, (4.0, "open cube"): 0.0, (2.0, "torus uploaded"): 5.402e-02, (4.0, "torus uploaded"): 6.505e-03,
                 (2.0, "two placed tori"): 2.706e-02, (4.0, "two placed tori"): 6.293e-03, (2.0, "one triangle"): 0.0, (4.0, "one triangle"): 0.0,
                 (2.0, "two triangles"): 0.0, (4.0, "two triangles"): 0.0, (2.0, "nested icospheres"): 2.217e-02, (4.0, "nested icospheres"): 5.082e-03,
                 (2.0, "flipped icosphere"): 2.315e-02, (4.0, "flipped icosphere"): 5.592e-03, (2.0, "deep chain"): 1.133e-07, (4.0, "deep chain"): 1.133e-07}


def log(line):
    print(line)
    path = os.environ.get("RTK_AMD_WINDING_LOG")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def mesh_of(tris):
    return dict(positions=np.ascontiguousarray(tris.reshape(-1, 3), F))


def make_queries(points):
    q = np.zeros(len(points), POINT_QUERY_DTYPE)
    q["point"] = points
    q["max_dist2"] = RTK_INF
    return q


def run(api, ds, points, n=None, beta=2.0, exact=False, count=None, ids=None):
    """-> the words of d_winding [n + TAIL]; the tail is checked here"""
    import torch
    q = make_queries(points)
    n = len(q) if n is None else n
    d_q = api.to_device(q) if len(q) else torch.zeros(16, dtype=torch.uint8, device="cuda")
    d_w = torch.full((n + TAIL,), 0, dtype=torch.int32, device="cuda").fill_(FILL).view(torch.float32)
    d_count = torch.tensor([count], dtype=torch.int64, device="cuda") if count is not None else None
    d_ids = torch.from_numpy(np.ascontiguousarray(ids, np.int64)).cuda() if ids is not None else None
    ds.winding_numbers_device(d_q, n, d_w, count=d_count, ids=d_ids, beta=beta, exact=exact)
    assert api.lib().rtk_dev_trace_status(ds.handle, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0, api.last_error()
    w = d_w.view(torch.int32).cpu().numpy().view(np.uint32)
    assert (w[n:] == FILL).all(), "written beyond num_queries"
    return w


def values(api, ds, points, **kw):
    return run(api, ds, points, **kw)[:len(points)].view(F).astype(np.float64)


class Case:
    def __init__(self, ds, tris, pts):
        self.ds, self.tris, self.pts = ds, tris, pts
        self.w64 = brute64(tris, pts)


@pytest.fixture(scope="module")
def cases(api, oracle):
    """name -> Case: every scene under test with its triangles as the scene holds them, 256 points (fewer triangles: 128) kept
    5 % of the size away, and their float64 winding numbers, computed once"""
    from oracle import pyoracle
    from tests.test_place_cpu import place_np
    from tests.test_gpu_build import _adversarial_scenes
    out = {}
    for k, (name, (tris, size)) in enumerate(fixtures().items()):
        pts = query_points(tris, size, 256, 70 + k)
        if name == "torus":
            # (the tube is a small part of the box and 5 % of the size is a third of its radius: 64 of the points are drawn inside it)
            rng = np.random.RandomState(69)
            u, phi, rho = rng.uniform(0, 2 * np.pi, 64), rng.uniform(0, 2 * np.pi, 64), 0.4 * np.sqrt(rng.uniform(0, 1, 64))
            tube = np.stack([(2.0 + rho * np.cos(phi)) * np.cos(u), (2.0 + rho * np.cos(phi)) * np.sin(u), rho * np.sin(phi)], 1).astype(F)
            pts = np.ascontiguousarray(np.concatenate([pts[:192], tube]))
            assert (distance64(tris, pts) >= 0.05 * size).all() and torus_inside(pts).sum() >= 64
        out[name] = Case(api.DeviceScene.build([mesh_of(tris)]), tris, pts)
    t = out["torus"]
    out["torus uploaded"] = Case(api.DeviceScene.upload(pyoracle.build_scene([mesh_of(t.tris)])), t.tris, t.pts)
    small = torus(32, 16)
    pl = np.array([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], [0.6, 0, 0.8, 7.0, 0, 1, 0, 0.5, -0.8, 0, 0.6, 1.0]], F)
    world = np.concatenate([place_np(pl[m], small.reshape(-1, 3)).reshape(-1, 3, 3) for m in range(2)]).astype(F)
    out["two placed tori"] = Case(api.DeviceScene.build([mesh_of(small), mesh_of(small)], placements=pl), world, query_points(world, 5.5, 256, 80))
    one = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], F)
    two = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[1, 0, 0], [1, 1, 0.5], [0, 1, 0]]], F)
    out["one triangle"] = Case(api.DeviceScene.build([mesh_of(one)]), one, query_points(one, 1.0, 128, 81))
    out["two triangles"] = Case(api.DeviceScene.build([mesh_of(two)]), two, query_points(two, 1.0, 128, 82))
    nested = np.concatenate([icosphere(3), icosphere(3, 2.0)])
    out["nested icospheres"] = Case(api.DeviceScene.build([mesh_of(nested)]), nested, query_points(nested, 4.0, 256, 83))
    flipped = np.ascontiguousarray(icosphere(3)[:, [0, 2, 1]])
    out["flipped icosphere"] = Case(api.DeviceScene.build([mesh_of(flipped)]), flipped, query_points(flipped, 2.0, 256, 84))
    chain = _adversarial_scenes()["geometric_chain"]
    out["deep chain"] = Case(api.DeviceScene.build([mesh_of(chain)]), chain, query_points(chain, 0.5, 128, 85))
    assert set(out) == set(MEASURED_EXACT)
    return out


def test_exact_form_against_float64(api, cases):
    """RTK_WINDING_EXACT on every scene: built, uploaded from a CPU-built blob, placed, one and two triangles. 4 x the measured
    error is asserted, and that bound may not exceed 1e-3."""
    failed = []
    for name, c in cases.items():
        err = np.abs(values(api, c.ds, c.pts, exact=True) - c.w64).max()
        log("exact form against float64: %-18s %5d triangles %4d points: worst %.3e" % (name, len(c.tris), len(c.pts), err))
        bound = 4 * MEASURED_EXACT[name]
        assert bound <= CEILING, name
        if not err <= bound:
            failed.append((name, err, bound))
    assert not failed, failed


def test_values_known_without_a_reference(api, cases):
    """1 inside and 0 outside the torus, the L and the plus (analytic inside tests), 2 inside two nested icospheres, -1 inside the
    icosphere wound inwards, 5/6 at the centre of the cube without a face: each within its case's bound of the first test."""
    L, plus = l_prism(TILT), plus_shape(TILT)
    for name, inside in (("torus", torus_inside), ("L", L.inside), ("plus", plus.inside)):
        c = cases[name]
        w = values(api, c.ds, c.pts, exact=True)
        ins = inside(c.pts)
        assert ins.sum() >= 5 and (~ins).sum() >= 5, (name, int(ins.sum()))
        assert np.abs(w - ins).max() <= 4 * MEASURED_EXACT[name], name
    c = cases["nested icospheres"]
    r = np.linalg.norm(c.pts.astype(np.float64), axis=1)
    w = values(api, c.ds, c.pts, exact=True)
    want = np.where(r < 0.99, 2.0, np.where(r < 1.98, 1.0, 0.0))
    assert (r < 0.99).sum() >= 3 and np.abs(w - want)[(r < 0.99) | ((r > 1.0) & (r < 1.98)) | (r > 2.0)].max() <= 4 * MEASURED_EXACT["nested icospheres"]
    c = cases["flipped icosphere"]
    r = np.linalg.norm(c.pts.astype(np.float64), axis=1)
    w = values(api, c.ds, c.pts, exact=True)
    assert (r < 0.99).sum() >= 3 and np.abs(w[r < 0.99] + 1.0).max() <= 4 * MEASURED_EXACT["flipped icosphere"]
    c = cases["open cube"]
    w = values(api, c.ds, np.zeros((1, 3), F), exact=True)[0]
    assert abs(w - 5.0 / 6.0) <= 4 * MEASURED_EXACT["open cube"], w


def test_fast_form_against_exact_form(api, cases):
    """beta 2 and beta 4 against RTK_WINDING_EXACT on the same scene and points: 2 x the measured difference. contains_winding
    agrees with the float64 classification on EVERY point, and the error at beta 4 is not above the asserted bound at beta 2."""
    failed = []
    for name, c in cases.items():
        exact = values(api, c.ds, c.pts, exact=True)
        diff = {}
        for beta in (2.0, 4.0):
            diff[beta] = np.abs(values(api, c.ds, c.pts, beta=beta) - exact).max()
            log("beta %g against the exact form: %-18s worst %.3e" % (beta, name, diff[beta]))
            if not diff[beta] <= 2 * MEASURED_FAST[(beta, name)]:
                failed.append((name, beta, diff[beta]))
        if not diff[4.0] <= 2 * MEASURED_FAST[(2.0, name)]:
            failed.append((name, "beta 4 above the bound of beta 2", diff[4.0]))
        got = c.ds.contains_winding(c.pts)
        wrong = np.nonzero(got != (c.w64 > 0.5))[0]
        if len(wrong):
            failed.append((name, "side", c.pts[wrong[:3]], c.w64[wrong[:3]]))
        margin = np.abs(c.w64 - 0.5).min()
        log("side of 0.5 at beta 2:          %-18s %d of %d points differ from float64 (closest float64 value to 0.5: %.3e away)" % (name, len(wrong), len(c.pts), margin))
    assert not failed, failed


def test_the_far_terms_are_really_used(api, cases):
    c = cases["torus"]
    n, prims = 64, len(c.tris)
    rng = np.random.RandomState(11)
    d = rng.standard_normal((n, 3))
    far = (d / np.linalg.norm(d, axis=1, keepdims=True) * 100 * 5.5).astype(F)       # 100 x the diameter away
    d_w, counts = c.ds.winding_numbers_counted(api.to_device(make_queries(far)), n)
    assert counts["triangles"] == 0 and counts["nodes"] == n and counts["rays"] == n and counts["hits"] >= n, counts
    assert np.abs(d_w.cpu().numpy()).max() < 1e-4
    d_w, counts = c.ds.winding_numbers_counted(api.to_device(make_queries(far)), n, exact=True)
    assert counts["triangles"] == n * prims and counts["hits"] == 0, counts
    # inside the tube: on the CPU first, a float64 walk over the table read back, every leaf taken for the builder's limit of 3
    inside = c.pts[torus_inside(c.pts)][:32]
    assert len(inside) >= 8 and prims >= 2048
    tests = winding_ref.walk64(c.ds.winding_moments().cpu().numpy(), inside, 2.0, lambda first: 3)
    log("triangle tests per query inside the torus at beta 2, float64 walk with 3 per leaf: mean %.0f, worst %d of %d" % (tests.mean(), tests.max(), prims))
    assert tests.sum() < len(inside) * prims / 8                             # (with room: half of what is asserted below)
    d_w, counts = c.ds.winding_numbers_counted(api.to_device(make_queries(inside)), len(inside))
    log("the same on the device: %d triangle tests, %d table records, %d far terms for %d queries" % (counts["triangles"], counts["nodes"], counts["hits"], len(inside)))
    assert counts["triangles"] < len(inside) * prims / 4 and counts["hits"] > 0 and counts["nodes"] >= len(inside)


def test_table(api, cases):
    """The sums at the root against float64, the records' shape, and the ledger. (The child words are compared with the
    structure a tree must have -- every node named once, every record under exactly one leaf -- not with the scene's nodes:
    there is no read-back of DevNode records.)"""
    for name in ("torus", "L", "plus", "icosphere", "open cube", "torus uploaded"):
        c = cases[name]
        ds = api.DeviceScene.build([mesh_of(c.tris)]) if name != "torus uploaded" else c.ds
        before = ds.info()["total_device_bytes"]
        info = ds.prepare_winding()
        n64, a64 = winding_ref.area_vector64(c.tris)
        # every addition rounds within 2^-24 of a partial sum no larger than the total area; a value goes through fewer than 64 of them
        tol = 64 * 2.0 ** -24 * a64
        assert np.abs(np.array(info["total_area_vector"]) - n64).max() <= tol and abs(info["total_area"] - a64) <= tol, (name, info)
        if name == "open cube":
            assert np.abs(np.array(info["total_area_vector"]) - [0, 0, -4]).max() <= tol
        else:
            assert np.abs(info["total_area_vector"]).max() <= tol
        nodes = ds.info()["num_nodes"]
        assert info["nodes"] == nodes and info["table_bytes"] == 128 * nodes and (info["table_ms"] > 0 or name == "torus uploaded")
        if name != "torus uploaded":
            assert ds.info()["total_device_bytes"] == before + info["table_bytes"]
        m = ds.winding_moments().cpu().numpy()
        assert m.shape == (nodes, 8, 4)
        child = m[:, 7].view(np.uint32)
        used = child != winding_ref.NONE
        R = m[:, 6]
        assert np.isfinite(R[used]).all() and (R[used] >= 0).all()
        assert (m[:, :7][np.broadcast_to(~used[:, None, :], (nodes, 7, 4))] == 0).all()      # an empty slot's record is all zero
        inner = child[used & ((child & winding_ref.LEAF) == 0)]
        assert sorted(inner.tolist()) == list(range(1, nodes))               # a tree: every node but the root named exactly once
        leaves = child[used & ((child & winding_ref.LEAF) != 0)] & 0x7FFFFFFF
        assert len(set(leaves.tolist())) == len(leaves) and leaves.max() < len(c.tris)
        root = m[0].astype(np.float64)
        assert np.abs(root[0:3].sum(1) - info["total_area_vector"]).max() <= 1e-12 + tol
        if name != "torus uploaded":
            assert ds.prepare_winding()["table_ms"] == 0
    # the ledger, exactly: a scene whose refit schedule and side arrays exist already
    c = cases["L"]
    ds = api.DeviceScene.build([mesh_of(c.tris)])
    ds.validate()
    ds.refit([mesh_of(c.tris)])
    base = ds.info()["total_device_bytes"]
    info = ds.prepare_winding()
    assert ds.info()["total_device_bytes"] == base + info["table_bytes"]
    ds.refit([mesh_of(c.tris)])
    assert ds.info()["total_device_bytes"] == base                          # dropped: shrinks by exactly table_bytes
    values(api, ds, c.pts[:8])
    assert ds.info()["total_device_bytes"] == base + info["table_bytes"]     # made again by the first query


def test_lifetime(api, oracle, cases):
    """A refit to the torus scaled by 2 drops the table and the results follow the new positions; split_leaves(2) and rebuild()
    drop it too, and the results stay within the bound of the first test; a second prepare_winding finds it made."""
    from oracle import pyoracle
    c = cases["torus"]
    bound = 4 * MEASURED_EXACT["torus"]
    ds = api.DeviceScene.build([mesh_of(c.tris)])
    first = values(api, ds, c.pts, exact=True)
    assert ds.prepare_winding()["table_ms"] == 0
    big = (c.tris * F(2)).astype(F)
    ds.refit([mesh_of(big)])
    moved = ds.prepare_winding()
    assert moved["table_ms"] > 0 and abs(moved["total_area"] - 4 * winding_ref.area_vector64(c.tris)[1]) < 1e-3
    assert ds.prepare_winding()["table_ms"] == 0
    assert np.abs(values(api, ds, c.pts * F(2), exact=True) - c.w64).max() <= bound            # (scaling by 2 is exact: the same float64 numbers)
    assert np.abs(values(api, ds, c.pts, exact=True) - brute64(big, c.pts)).max() <= CEILING and not np.allclose(values(api, ds, c.pts, exact=True), first, atol=1e-2)
    up = api.DeviceScene.upload(pyoracle.build_scene([mesh_of(c.tris)]))
    for ds, step in ((up, lambda d: d.split_leaves(2)), (up, lambda d: d.rebuild()), (api.DeviceScene.build([mesh_of(c.tris)]), lambda d: d.rebuild())):
        before = values(api, ds, c.pts, exact=True)
        fast_before = values(api, ds, c.pts)
        nodes = ds.prepare_winding()["nodes"]
        step(ds)
        info = ds.prepare_winding()
        assert info["table_ms"] > 0 and info["nodes"] == ds.info()["num_nodes"], (nodes, info)
        after = values(api, ds, c.pts, exact=True)
        assert np.abs(after - before).max() <= bound and np.abs(after - c.w64).max() <= bound
        # (each fast result within its bound of its exact one, the exact ones within theirs of each other)
        assert np.abs(values(api, ds, c.pts) - fast_before).max() <= 2 * 2 * MEASURED_FAST[(2.0, "torus")] + bound


@pytest.fixture(scope="module")
def cfg1_blob(oracle):
    from rtk_amd import synth
    return oracle.build_scene([dict(positions=synth.scene_for_config(1))])


def test_calling_conventions(api, oracle, cases, cfg1_blob):
    import torch
    c = cases["plus"]
    ds = api.DeviceScene.build([mesh_of(c.tris)])
    # no queries: OK, and no table is made
    before = ds.info()["total_device_bytes"]
    run(api, ds, c.pts[:0])
    assert ds.info()["total_device_bytes"] == before
    full = run(api, ds, c.pts)
    assert (full == run(api, ds, c.pts)).all()                               # the same scene object: the same bits
    n = len(c.pts)
    # lists: a slot that is not listed is not written; an id may repeat; the count is clamped
    ids = np.array([7, 3, 3, n - 1, 0, 100, 7], np.int64)
    for count, use in ((len(ids), ids), (4, ids[:4]), (0, ids[:0])):
        w = run(api, ds, c.pts, count=count, ids=ids)
        listed = np.zeros(n + TAIL, bool)
        listed[use] = True
        assert (w[listed] == full[listed]).all() and (w[~listed] == FILL).all()
    w = run(api, ds, c.pts, count=100)
    assert (w[:100] == full[:100]).all() and (w[100:] == FILL).all()
    for size in (1, 63, 64, 65, 1025):                                      # one lane, a wave and one more, more than one workgroup
        which = np.arange(size) % n
        assert (run(api, ds, c.pts[which])[:size] == full[which]).all()
    # a non-finite coordinate: the quiet NaN, its neighbours answered; max_dist2 is not read
    pts = c.pts[:8].copy()
    pts[2, 0] = np.nan; pts[4, 1] = np.inf; pts[5, 2] = -np.inf
    w = run(api, ds, pts)
    ok = np.array([0, 1, 3, 6, 7])
    assert (w[[2, 4, 5]] == NAN_BITS).all() and (w[ok] == full[ok]).all()
    q = make_queries(c.pts[:8])
    q["max_dist2"] = [0.0, -1.0, np.nan, 1e-9, np.inf, 1.0, RTK_INF, 5.0]
    d_w = ds.winding_numbers_device(api.to_device(q), 8)
    assert (d_w.view(torch.int32).cpu().numpy().view(np.uint32) == full[:8]).all()
    # refusals on a live scene: the code, and nothing written
    L = api.lib()
    d_q = api.to_device(make_queries(c.pts[:8]))
    d_out = torch.full((8,), 0, dtype=torch.int32, device="cuda").fill_(FILL)
    for kw in (dict(struct_size=8), dict(beta=-1.0), dict(beta=float("nan")), dict(flags=4)):
        o = api.make_winding_opts()
        for k, v in kw.items():
            setattr(o, k, v)
        assert L.rtk_dev_winding_numbers(ds.handle, C.c_void_p(d_q.data_ptr()), 8, None, C.byref(o), C.c_void_p(d_out.data_ptr()), None) == ERR_BAD_ARG, kw
    assert L.rtk_dev_winding_numbers(ds.handle, C.c_void_p(d_q.data_ptr()), 8, None, None, None, None) == ERR_BAD_ARG
    assert L.rtk_dev_winding_numbers(ds.handle, None, 8, None, None, C.c_void_p(d_out.data_ptr()), None) == ERR_BAD_ARG
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy().view(np.uint32) == FILL).all()
    o = api.make_winding_opts(beta=0.0)                                      # beta 0: the default
    assert L.rtk_dev_winding_numbers(ds.handle, C.c_void_p(d_q.data_ptr()), 8, None, C.byref(o), C.c_void_p(d_out.data_ptr()), None) == 0
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy().view(np.uint32) == full[:8]).all()
    # a blob that names a primitive twice (the fixture of tests/test_gpu_sign.py): -6, nothing allocated
    from tests.test_gpu_rebuild import _as_blob, _leaves
    data = np.array(cfg1_blob.data, copy=True)
    off, cnt = next((o, k) for o, k in _leaves(data) if k >= 2 and k % 4 != 1)
    prim_ids = data[off + 8:off + 8 + 8 * cnt].view("<u4")[1::2]
    twice = data.copy()
    twice[off + 8:off + 8 + 8 * cnt].view("<u4")[2 * cnt - 1] = prim_ids[cnt - 2]
    bad = api.DeviceScene.upload(_as_blob(oracle, twice))
    info_before = bad.info()
    buf = torch.zeros(64, dtype=torch.uint8, device="cuda")
    assert L.rtk_dev_scene_prepare_winding(bad.handle, C.byref(api.WindingInfo()), None) == ERR_UNSUPPORTED and "one triangle record per primitive" in api.last_error()
    assert L.rtk_dev_winding_numbers(bad.handle, C.c_void_p(buf.data_ptr()), 1, None, None, C.c_void_p(buf.data_ptr()), None) == ERR_UNSUPPORTED
    assert L.rtk_dev_scene_winding_moments(bad.handle, C.c_void_p(buf.data_ptr()), None) == ERR_UNSUPPORTED
    assert bad.info() == info_before
    good = api.DeviceScene.upload(_as_blob(oracle, data))
    assert good.prepare_winding()["table_bytes"] == 128 * good.info()["num_nodes"]


def test_a_stack_deeper_than_the_on_chip_part(api, cases):
    """the geometric cluster of tests/test_gpu_closest.py's spill test: with every child pushed (the exact form) the walk goes
    past the on-chip entries, and the result is still the float64 one"""
    c = cases["deep chain"]
    on_chip = api.lib().rtk_amd_winding_stack_entries()
    assert c.ds.info()["stack_entries"] > on_chip, (c.ds.info()["stack_entries"], on_chip)
    d_w, counts = c.ds.winding_numbers_counted(api.to_device(make_queries(c.pts)), len(c.pts), exact=True)
    log("deep chain: stack entries %d, on chip %d, counts %s" % (c.ds.info()["stack_entries"], on_chip, counts))
    assert counts["stack_spills"] > 0 and counts["rays"] == len(c.pts) and counts["triangles"] == len(c.pts) * len(c.tris)
    assert np.abs(d_w.cpu().numpy().astype(np.float64) - c.w64).max() <= 4 * MEASURED_EXACT["deep chain"]
    assert (d_w.view(__import__("torch").int32).cpu().numpy().view(np.uint32) == run(api, c.ds, c.pts, exact=True)[:len(c.pts)]).all()
    assert api.lib().rtk_dev_trace_status(c.ds.handle, None) == 0


def test_an_mgpu_scene(api, cases):
    """rtk_mgpu_scene(m, 0) of a one-device context gives the words of a plain scene built from the same meshes"""
    import torch
    c = cases["icosphere"]
    want = run(api, c.ds, c.pts)[:len(c.pts)]
    L = api.lib()
    m = L.rtk_mgpu_create((C.c_int * 1)(0), 1)
    assert m, api.last_error()
    try:
        ms = api.MeshSet([mesh_of(c.tris)])
        assert L.rtk_mgpu_build(m, C.byref(ms.desc)) == 0, api.last_error()
        handle = L.rtk_mgpu_scene(m, 0)
        assert handle
        n = len(c.pts)
        d_q = api.to_device(make_queries(c.pts))
        d_w = torch.full((n,), 0, dtype=torch.int32, device="cuda").fill_(FILL)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert L.rtk_dev_winding_numbers(handle, C.c_void_p(d_q.data_ptr()), n, None, None, C.c_void_p(d_w.data_ptr()), stream) == 0, api.last_error()
        assert (d_w.cpu().numpy().view(np.uint32) == want).all()
    finally:
        L.rtk_mgpu_destroy(m)
