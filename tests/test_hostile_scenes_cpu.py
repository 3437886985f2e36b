"""CPU side of tests/test_gpu_queries_hostile_scenes.py: the conditions on the scene set, the query groups, and that the scenes
tell a wrong tie order and a wrong cull from the right ones (two hand-made mutants of closest_ref's brute force)."""
import numpy as np

from tests import hostile_scenes as H
from tests.closest_ref import better_np, brute_force, tri_box, box_np, tri_np

NONE = 0xFFFFFFFF


def test_the_scene_set_holds_the_conditions():
    sc = H.scenes()
    held = H.check_conditions(sc)
    assert set(held["a"]) == {"mix10", "mix6", "all_identical"} and "zero_area_row" in held["c"] and "mix10" in held["c"]
    assert "tiny_cluster_plus_far_triangle" in held["d"] and held["e"] == ["huge_coordinates"] and len(held["b"]) >= 4
    assert all(len(t) <= 2500 for t in sc.values()) and len(sc["all_identical"]) == 600


def test_the_three_groups_are_what_they_say():
    for name in ("mix10", "mix6", "coplanar", "huge_coordinates"):
        tris = H.scenes()[name]
        f = H.Frame(tris)
        g = H.point_groups(tris)
        assert g.shape == (96, 3)
        verts = {v.tobytes() for v in tris[H.copies(tris)].reshape(-1, 3)} if f.has_copies else {v.tobytes() for v in tris.reshape(-1, 3)}
        assert all(p.tobytes() in verts for p in g[:32])
        assert g[32].tobytes() == (f.lo - np.float32(1e3) * f.ext).astype(np.float32).tobytes()
        assert g[33].tobytes() == (f.hi + np.float32(1e3) * f.ext).astype(np.float32).tobytes()
        assert (g[64:, f.axis] == f.plane).all()
        t = H.triangle_groups(tris)
        assert (t[64:, :, f.axis] == f.plane).all()
        lo, hi = H.box_groups(tris)
        assert (lo[64:, f.axis] == f.plane).all() and (hi[64:, f.axis] == f.plane).all() and (lo[:32] == hi[:32]).all()
    assert H.Frame(H.scenes()["coplanar"]).in_plane == len(H.scenes()["coplanar"]) and H.Frame(H.scenes()["coplanar"]).axis == 2
    assert H.Frame(H.scenes()["mix10"]).in_plane == 300


def mutant(tris, points, max2, ties_to_highest=False, cull_at_equal=False):
    """closest_ref.brute_force's primitives by a walk over one box per triangle, from the highest id down (so that the lowest id
    at the winning dist2 is always met last, behind a bound that may equal the best dist2 so far), optionally with one of two
    faults: a tie stays with the highest id; a box whose bound EQUALS the best dist2 is culled (>= where rtk_closest_skip has >)"""
    a, b, c = tris[:, 0], tris[:, 1], tris[:, 2]
    lo, hi = tri_box(a, b, c)
    prim = np.full(len(points), NONE, np.uint32)
    best = max2.astype(np.float32).copy()
    for t in range(len(tris) - 1, -1, -1):
        bound = box_np(points, lo[t], hi[t])
        d2 = tri_np(points, a[t], b[t], c[t])[0]
        skip = bound >= best if cull_at_equal else bound > best
        take = (d2 < max2) & ((d2 < best) if ties_to_highest else better_np(d2, np.uint32(t), best, prim)) & ~skip
        best = np.where(take, d2, best)
        prim = np.where(take, np.uint32(t), prim)
    return prim


def test_the_scenes_tell_the_mutants_apart():
    """For closest points on the copied scenes: the faithful walk gives the reference's primitives; ties to the highest id and
    a cull at equality each change the answer of at least 16 queries of the tied group"""
    for name in ("mix10", "all_identical"):
        tris = H.scenes()[name]
        q = H.point_queries(tris, "closest")
        live = np.isfinite(q["point"]).all(1)
        want = brute_force(tris, np.arange(len(tris), dtype=np.uint32), q["point"], q["max_dist2"])[0][:, 3]
        with np.errstate(all="ignore"):
            assert (mutant(tris, q["point"], q["max_dist2"])[live] == want[live]).all()
            high = mutant(tris, q["point"], q["max_dist2"], ties_to_highest=True)
            cull = mutant(tris, q["point"], q["max_dist2"], cull_at_equal=True)
        print("%s: ties to the highest id change %d answers, a cull at equality %d, of %d" % (name, (high != want)[live].sum(), (cull != want)[live].sum(), live.sum()))
        assert (high != want)[live].sum() >= 16
        assert (cull != want)[live].sum() >= 16
