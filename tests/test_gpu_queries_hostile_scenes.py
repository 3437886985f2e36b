"""Every query family on the scenes that break a tree (tests/hostile_scenes.py: four degenerate mixes of tests/test_gpu_sizes.py
and a strided subset of every adversarial scene of tests/test_gpu_build.py), bit for bit against the family's own brute force
over the records the scene holds (read back through rtk_dev_expand_hits), on three trees per scene: the device build, that
scene after split_leaves(2), and after rebuild(). Queries: the family's own mix cut to 200 rows and three groups of 32 -- on
copied records, 1e3 extents away, inside the zero thickness of the scene's flat direction. Outputs are pre-filled with 0x7e and
carry an untouched tail; rtk_dev_trace_status is 0 after every call (the families' own run helpers assert both). Every case
asserts from the reference alone that it is not vacuous: 20 % of its live queries hit, and on the scenes with more than 100
copied records 16 queries have two or more triangles at the winning dist2 or t (lists: two copies in the list).

(scene, family) pairs left out, 4 of 130:

    scene   family                     reason
    mix15   box, touch, pair, near     the family's own mix draws 40 distinct triangles of the scene; this one has 37

Winding numbers leave out all_identical: 600 copies of one record add the same rounding 600 times, and max |brute32 - brute64|
on its 128 points is 1.734e-03, beyond the 1e-3 ceiling of tests/test_gpu_winding.py.

Then scenes with NaN and infinite vertex coordinates: one call per family, and only what include/rtk_amd.h promises for them."""
import ctypes as C
import types

import numpy as np
import pytest

from rtk_amd.types import RTK_INF
from tests import hostile_scenes as H
from tests.test_gpu_closest import FILL, TAIL, scene_triangles

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
SCENES = ["mix15", "mix16", "mix10", "mix6", "tiny_cluster_plus_far_triangle", "all_identical", "line_along_x", "huge_coordinates", "two_distant_clusters",
          "coplanar", "flat_floor_grid", "zero_area_row", "geometric_chain"]
COPIED = ("mix10", "mix6", "all_identical")                     # condition (a): more than 100 copied records
DROPPED = {("mix15", f): "the family's own mix draws 40 distinct triangles; the scene has 37" for f in ("box", "touch", "pair", "near")}
FAMILIES = 10
assert 4 * len(DROPPED) <= len(SCENES) * FAMILIES
SWEEPS = {"sphere": ("tests.test_gpu_sweep", "tests.sweep_ref"), "box": ("tests.test_gpu_boxsweep", "tests.boxsweep_ref"),
          "capsule": ("tests.test_gpu_capsule", "tests.capsule_ref"), "obb": ("tests.test_gpu_obbsweep", "tests.obbsweep_ref")}
GROUPS = slice(-3 * H.GROUP, None)                              # the three groups stand at the end of every batch


def scenes_for(family):
    return [s for s in SCENES if (s, family) not in DROPPED]


def test_the_scene_set_and_the_dropped_pairs():
    sc = H.scenes()
    assert list(sc) == SCENES
    held = H.check_conditions(sc)
    assert set(held["a"]) == set(COPIED), held
    print("conditions held by: %s" % held)


def build(api, name):
    """-> (scene, its records): the records are the input's, in input order"""
    tris = H.scenes()[name]
    ds = api.DeviceScene.build([dict(positions=np.ascontiguousarray(tris.reshape(-1, 3)))])
    got = scene_triangles(api, ds)
    assert got.tobytes() == tris.tobytes()
    return ds, got


def three_trees(api, ds, tris, check):
    """check(ds) -> bytes, on the device build, after split_leaves(2) and after rebuild(): the same bytes each time"""
    first = check(ds)
    ds.split_leaves(2)
    assert scene_triangles(api, ds).tobytes() == tris.tobytes()
    assert check(ds) == first, "after split_leaves(2)"
    ds.rebuild()
    assert scene_triangles(api, ds).tobytes() == tris.tobytes()
    assert check(ds) == first, "after rebuild()"


def not_vacuous(name, family, live, hit, tied):
    """live, hit: bool per query; tied: queries with two or more triangles at the winning value (or two copies in the list)"""
    share = float(hit[live].mean())
    print("%s %s: %d queries, %d live, %d hit (%.0f %%), %d tied" % (name, family, len(live), live.sum(), (hit & live).sum(), 100 * share, tied))
    assert live.sum() >= 100 and share >= 0.2, (name, family, share)
    if name in COPIED:
        assert tied >= 16, (name, family, tied)


def copies_in(tris, lists):
    cp = H.copies(tris)
    return sum(1 for l in lists if cp[np.asarray(l, np.int64)].sum() >= 2)


def count_then_fill(m, api, ds, q, ref_counts, want_lists, n, **kw):
    """a family's count form, then its fill form at the exact offsets of that count pass -> all bytes"""
    counts = m.run_count(api, ds, q, **kw)
    assert counts[:n].tobytes() == ref_counts.tobytes(), np.nonzero(counts[:n] != ref_counts)[0][:5]
    assert (counts[n:] == FILL).all()
    offsets = np.concatenate([[0], np.cumsum(counts[:n].astype(np.int64))])
    total = int(offsets[-1])
    got = m.run_fill(api, ds, q, offsets, total, **kw)
    m.assert_fill(got, m.expected_fill(want_lists, offsets, total), "exact offsets")
    return counts.tobytes() + b"".join(x.tobytes() for x in got)


# ---------------------------------------------------------------- the tree-independent families

@pytest.mark.parametrize("name", scenes_for("closest"))
def test_closest_points(api, name):
    from tests import test_gpu_closest as m
    from tests.closest_ref import brute_force
    ds, tris = build(api, name)
    q = H.point_queries(tris, "closest")
    want = brute_force(tris, np.arange(len(tris), dtype=np.uint32), q["point"], q["max_dist2"])
    live = np.isfinite(q["point"]).all(1) & (q["max_dist2"] > 0)
    tied = H.tied_winners(brute_force, tris, q["point"][GROUPS], q["max_dist2"][GROUPS]).sum() if name in COPIED else 0
    not_vacuous(name, "closest", live, want[0][:, 3] != NONE, tied)
    three_trees(api, ds, tris, lambda ds: m.check(api, ds, q, want).tobytes())


@pytest.mark.parametrize("name", scenes_for("within"))
def test_triangles_within(api, name):
    from tests import test_gpu_within as m
    from tests.within_ref import brute_force_within
    ds, tris = build(api, name)
    q = H.point_queries(tris, "within")
    ref = brute_force_within(tris, np.arange(len(tris)), q["point"], q["max_dist2"])
    live = np.isfinite(q["point"]).all(1) & (q["max_dist2"] > 0)
    tied = sum(1 for r, _ in ref.lists if len(r) >= 2 and r[0, 0] == r[1, 0])
    not_vacuous(name, "within", live, ref.counts > 0, tied)
    three_trees(api, ds, tris, lambda ds: count_then_fill(m, api, ds, q, ref.counts, ref.lists, len(q)))


@pytest.mark.parametrize("name", scenes_for("box"))
def test_triangles_in_box(api, name):
    from tests import test_gpu_box as m
    from tests.box_ref import brute_force_boxes
    ds, tris = build(api, name)
    q = H.box_queries(tris)
    ref = brute_force_boxes(tris, np.arange(len(tris)), q["lo"], q["hi"])
    live = ~(np.isnan(q["lo"]).any(1) | np.isnan(q["hi"]).any(1)) & (q["lo"] <= q["hi"]).all(1)
    not_vacuous(name, "box", live, ref.counts > 0, copies_in(tris, ref.lists))
    three_trees(api, ds, tris, lambda ds: count_then_fill(m, api, ds, q, ref.counts, ref.lists, len(q)))


@pytest.mark.parametrize("name", scenes_for("touch"))
def test_triangles_touching(api, name):
    from tests import test_gpu_touch as m
    from tests.test_gpu_box import assert_fill, expected_fill
    from tests.touch_ref import brute_force_touching
    ds, tris = build(api, name)
    q, _ = H.triangle_queries(tris, "touch")
    ref = brute_force_touching(tris, np.arange(len(tris)), q)
    not_vacuous(name, "touch", np.isfinite(q).all((1, 2)), ref.counts > 0, copies_in(tris, ref.lists))

    # (the touch file takes its fill helpers from the box file)
    forms = types.SimpleNamespace(run_count=m.run_count, run_fill=m.run_fill, assert_fill=assert_fill, expected_fill=expected_fill)
    three_trees(api, ds, tris, lambda ds: count_then_fill(forms, api, ds, q, ref.counts, ref.lists, len(q)))


@pytest.mark.parametrize("name", scenes_for("pair"))
def test_closest_triangles(api, name):
    from tests import test_gpu_pair as m
    from tests.pair_ref import brute_force_pairs
    ds, tris = build(api, name)
    q, max2 = H.triangle_queries(tris, "pair")
    ref = brute_force_pairs(tris, np.arange(len(tris)), q, max2)
    live = np.isfinite(q).all((1, 2)) & (max2 > 0)
    tied = H.tied_winners(brute_force_pairs, tris, q[GROUPS], max2[GROUPS]).sum() if name in COPIED else 0
    not_vacuous(name, "pair", live, ref[0][:, 3] != NONE, tied)
    three_trees(api, ds, tris, lambda ds: m.check_scene(api, ds, q, max2, ref))


@pytest.mark.parametrize("name", scenes_for("near"))
def test_triangles_near(api, name):
    from tests import test_gpu_near as m
    from tests.near_ref import brute_force_near
    ds, tris = build(api, name)
    q, max2 = H.triangle_queries(tris, "near")
    ref = brute_force_near(tris, np.arange(len(tris)), q, max2)
    live = np.isfinite(q).all((1, 2)) & (max2 > 0)
    tied = sum(1 for k in ref.kept if len(k[0]) >= 2 and k[0][0, 0] == k[0][1, 0])
    not_vacuous(name, "near", live, ref.counts > 0, tied)
    three_trees(api, ds, tris, lambda ds: count_then_fill(m, api, ds, q, ref.counts, ref.kept, len(q), max2=max2))


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("kind", list(SWEEPS))
def test_sweeps(api, kind, name):
    """The closest form (records and both point outputs) and the any-hit form of the four sweeps"""
    import importlib
    m, r = (importlib.import_module(x) for x in SWEEPS[kind])
    ds, tris = build(api, name)
    s, own = H.sweep_queries(kind, tris)
    want = r.brute_force(tris, np.arange(len(tris), dtype=np.uint32), s)
    hit = want[0][:, 3] != NONE
    tied = H.tied_winners(r.brute_force, tris, s[GROUPS]).sum() if name in COPIED else 0
    not_vacuous(name, kind + " sweep" + ("" if own else " (paths of tests/hostile_scenes.py: the family's mix cannot be made of this scene)"),
                H.sweep_live(kind, s), hit, tied)

    def check(ds):
        rec = m.check(api, ds, s, want)
        flags = m.run(api, ds, s, any_hit=True)
        assert (flags[:len(s)] == hit.astype(np.uint8)).all(), np.nonzero(flags[:len(s)] != hit)[0][:10]
        return rec.tobytes() + flags.tobytes()
    three_trees(api, ds, tris, check)


# ---------------------------------------------------------------- signed distance, winding numbers, all hits

@pytest.mark.parametrize("name", ["mix15", "mix16", "mix10", "mix6", "all_identical"])
def test_signed_distance(api, name):
    from tests import test_gpu_sign as m
    from tests.sign_ref import table_np
    ds, tris = build(api, name)
    table, info = table_np(tris)
    got = ds.prepare_signs()
    assert {k: got[k] for k in m.COUNTS} == info, (got, info)
    assert got["table_bytes"] == 72 * len(tris)
    m.same_table(m.table_words(ds), table)
    q = H.point_queries(tris, "closest")
    sg = m.check(api, ds, tris, q["point"], q["max_dist2"], table)
    print("%s signed distance: %d degenerate triangles, %d places, %d answered of %d" % (name, info["degenerate_triangles"], info["places"],
                                                                                       (sg != RTK_INF).sum(), len(q)))
    assert (sg != RTK_INF).sum() >= 0.2 * len(q)


@pytest.mark.parametrize("name", [s for s in SCENES if s != "all_identical"])
def test_winding_numbers_exact_form(api, name):
    """|device - float64| <= 4 x max |brute32 - brute64| on the same points, the bound capped by the winding file's ceiling"""
    from tests import test_gpu_winding as m
    from tests.winding_ref import brute32, brute64, query_points
    ds, tris = build(api, name)
    size = float((tris.reshape(-1, 3).max(0) - tris.reshape(-1, 3).min(0)).max())
    pts = query_points(tris, size, 128, 90 + SCENES.index(name))
    w64 = brute64(tris, pts)
    rule = float(np.abs(brute32(tris, pts).astype(np.float64) - w64).max())
    assert rule <= m.CEILING, "left out: the rule's own float error %.3e is beyond the ceiling" % rule
    err = float(np.abs(m.values(api, ds, pts, exact=True) - w64).max())
    m.log("exact form against float64, hostile scene: %-30s %5d triangles %4d points: worst %.3e (brute32 %.3e)" % (name, len(tris), len(pts), err, rule))
    assert err <= min(4 * rule, m.CEILING), (name, err, rule)


@pytest.mark.parametrize("name", ["mix15", "mix16", "mix6", "coplanar"])      # (mix10 is a line of zero-area records: 15 % of these rays meet it)
def test_all_hits(api, oracle, name):
    from tests import allhits_ref as R
    from tests.test_gpu_allhits import check_all, fill
    ds, tris = build(api, name)
    rays = H.adversarial_rays(tris)
    want = R.oracle_lists(oracle, oracle.Blob(ds.export_blob()), rays, ds.mesh_base())
    print("%s all hits: %d rays, %d with candidates, %d candidates, longest list %d" % (name, len(rays), (want.counts > 0).sum(), want.counts.sum(), want.counts.max()))
    assert (want.counts > 0).mean() >= 0.2 and want.counts.max() >= 2
    check_all(api, ds, rays, want)
    rec, wr = fill(api, ds, rays, want.offsets)                  # the fill form into a 0x7e-filled buffer with a guard band
    assert rec.tobytes() == want.records.tobytes() and (wr == want.counts).all()


# ---------------------------------------------------------------- scenes with NaN and infinite vertex coordinates

def filled(words):
    import torch
    return torch.full((words * 4,), 0x7e, dtype=torch.uint8, device="cuda")


def words(t):
    return t.cpu().numpy().view(np.uint32)


def status_ok(api, ds):
    import torch
    assert api.lib().rtk_dev_trace_status(ds.handle, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0, api.last_error()


def prims_ok(prim, T):
    return ((prim < T) | (prim == NONE)).all()


def lists_ok(m_count, m_fill, T, n, width, room=4):
    """a count form and a fill form with `room` slots per query: counts <= T, written <= room, ids below T in the slots that
    are written, 0x7e in every other slot and in both tails"""
    counts = m_count()
    assert (counts[:n] <= T).all() and (counts[n:] == FILL).all()
    offsets = np.arange(n + 1, dtype=np.int64) * room
    got = m_fill(offsets, n * room)
    rec, wr = got[0].reshape(n * room + TAIL, width), got[-1]
    assert (wr[:n] <= room).all() and (wr[:n] == np.minimum(counts[:n], room)).all() and (wr[n:] == FILL).all()
    used = (np.arange(room)[None, :] < wr[:n, None]).reshape(-1)
    assert (rec[:n * room][~used] == FILL).all() and (rec[n * room:] == FILL).all()
    assert prims_ok(rec[:n * room][used][:, -1], T)
    for pts in got[1:-1]:                                        # point outputs move with the records
        p = pts.reshape(n * room + TAIL, 3)
        assert (p[:n * room][~used] == FILL).all() and (p[n * room:] == FILL).all()


@pytest.mark.parametrize("name", ["soup1000", "mix16"])
def test_non_finite_vertices(api, oracle, name):
    """NaN in one coordinate, whole NaN triangles, +inf and -inf (the recipe of tests/test_gpu_sizes.py): every call returns
    RTK_AMD_OK with a status word of 0, writes only inside its outputs, names only primitives of the scene, counts at most T
    and writes at most its room; the two derived tables are made and the ledger counts them; and a finite sibling scene built
    in the same process still equals its brute force afterwards."""
    import importlib
    import torch
    from tests import test_gpu_box, test_gpu_closest, test_gpu_near, test_gpu_pair, test_gpu_sign, test_gpu_touch, test_gpu_winding, test_gpu_within
    from tests.closest_ref import brute_force
    bad, good = H.non_finite_scenes()[name]
    T = len(bad)
    ds = api.DeviceScene.build([dict(positions=np.ascontiguousarray(bad.reshape(-1, 3)))])
    sibling = api.DeviceScene.build([dict(positions=np.ascontiguousarray(good.reshape(-1, 3)))])
    assert ds.info()["num_triangles"] == T
    # the queries are made of the finite sibling: they are finite themselves, apart from what a family's own mix holds
    pq = H.point_queries(good, "closest")
    n = len(pq)
    rec, pts = test_gpu_closest.run(api, ds, pq)                 # (run asserts rc, status and the tail)
    assert prims_ok(rec[:n, 3], T)
    wq = H.point_queries(good, "within")
    lists_ok(lambda: test_gpu_within.run_count(api, ds, wq), lambda off, total: test_gpu_within.run_fill(api, ds, wq, off, total), T, len(wq), 4)
    bq = H.box_queries(good)
    lists_ok(lambda: test_gpu_box.run_count(api, ds, bq), lambda off, total: test_gpu_box.run_fill(api, ds, bq, off, total), T, len(bq), 1)
    tq, _ = H.triangle_queries(good, "touch")
    lists_ok(lambda: test_gpu_touch.run_count(api, ds, tq), lambda off, total: test_gpu_touch.run_fill(api, ds, tq, off, total), T, len(tq), 1)
    nq, max2 = H.triangle_queries(good, "near")
    got = test_gpu_pair.run(api, ds, nq, max2=max2)
    assert all((g[len(nq):] == FILL).all() for g in got) and prims_ok(got[0][:len(nq), 3], T)
    lists_ok(lambda: test_gpu_near.run_count(api, ds, nq, max2=max2), lambda off, total: test_gpu_near.run_fill(api, ds, nq, off, total, max2=max2), T, len(nq), 4)
    for kind, (mod, _) in SWEEPS.items():
        m = importlib.import_module(mod)
        s, _ = H.sweep_queries(kind, good)
        out = m.run(api, ds, s)                                  # (run asserts rc, status and the three tails)
        assert prims_ok(out[0][:len(s), 3], T)
        flags = m.run(api, ds, s, any_hit=True)
        assert (flags[:len(s)] <= 1).all()
    # every hit along a ray: counts, then lists of at most 4
    rays = H.adversarial_rays(good, 512)
    counts = ds.count_hits(rays)
    assert (counts <= T).all()
    from tests.test_gpu_allhits import fill
    r, wr = fill(api, ds, rays, np.arange(len(rays) + 1, dtype=np.int64) * 4)
    assert (wr <= 4).all() and (wr == np.minimum(counts, 4)).all()
    used = (np.arange(4)[None, :] < wr[:, None]).reshape(-1)
    assert (r.view(np.uint32).reshape(-1, 4)[~used] == FILL).all() and prims_ok(r["prim"][used], T)
    # the derived tables: made, and counted by the ledger
    before = ds.info()["total_device_bytes"]
    signs = ds.prepare_signs()
    assert signs["table_bytes"] == 72 * T and ds.info()["total_device_bytes"] == before + signs["table_bytes"]
    sg, srec, spts = test_gpu_sign.run(api, ds, pq)
    assert prims_ok(srec[:n, 3], T) and srec[:n].tobytes() == rec[:n].tobytes() and spts[:n].tobytes() == pts[:n].tobytes()
    before = ds.info()["total_device_bytes"]
    winding = ds.prepare_winding()
    assert winding["table_bytes"] > 0 and ds.info()["total_device_bytes"] == before + winding["table_bytes"]
    for exact in (True, False):
        w = test_gpu_winding.run(api, ds, pq["point"], exact=exact)   # (run asserts rc, status and the tail)
        assert (w[:n] != FILL).all()
    status_ok(api, ds)
    torch.cuda.synchronize()
    # nothing is left behind in the shared scratch set: the finite sibling still equals its brute force
    assert scene_triangles(api, sibling).tobytes() == good.tobytes()
    test_gpu_closest.check(api, sibling, pq, brute_force(good, np.arange(len(good), dtype=np.uint32), pq["point"], pq["max_dist2"]))
