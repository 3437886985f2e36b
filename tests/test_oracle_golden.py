"""CPU tests: the oracle (CPU restatement) against the golden fixtures that were produced by
the REAL reference (oracle/gen_golden.py, leaf-chain through rtk.c's own rtk_trace_ray).

No GPU needed. These pin the checker itself: generators (input checksums), triangle
arithmetic (bit-exact on identical blobs), and the oracle's builder + traversal (ids exact,
t/u/v within tolerance on its own BVH).
"""
import numpy as np
import pytest

from rtk_amd import synth
from rtk_amd.types import RAY_DTYPE
from tests.util import compare_hits_struct, load_golden, sha


@pytest.fixture(scope="module")
def scene1():
    return synth.scene_for_config(1)


@pytest.fixture(scope="module")
def scene2():
    return synth.scene_for_config(2)


def test_generators_are_pinned(golden_dir, scene1):
    g = load_golden(golden_dir, "cfg1_full.npz")
    assert sha(scene1) == str(g["scene_sha256"])
    assert sha(synth.rays_config1(65536)) == str(g["rays_sha256"])
    g3 = load_golden(golden_dir, "cfg3_sample.npz")
    assert sha(synth.rays_incoherent(4096)) == str(g3["rays_sha256"])


def test_edge_cases_bit_exact_on_same_blob(oracle, golden_dir):
    """Same single-leaf blob as the reference saw -> every byte of (t,u,v,ids) must match."""
    g = load_golden(golden_dir, "edge_cases.npz")
    rays = np.ascontiguousarray(g["rays"]).view(RAY_DTYPE).reshape(-1)
    blobs = oracle.leaf_chain_blobs(g["tris"], g["mesh"], g["tri_index"])
    hits, mask = oracle.trace_chain(blobs, rays, threads=1)
    st = compare_hits_struct(hits, mask, g, "edge/chain")
    assert st["bit_exact"] == 1.0
    # the constructed cases really exercise what they claim
    assert mask[0] and hits["t"][0] == 1.0 and hits["triangle_index"][0] == 0 and hits["mesh_index"][0] == 0
    assert mask[1] and hits["triangle_index"][1] == 0          # diagonal tie resolved to the lower id
    assert mask[10] and hits["t"][10] == 2.0                   # t == min_t rejected, next surface found
    assert not mask[11]                                        # t == max_t rejected
    assert mask[19] and hits["triangle_index"][19] == 4        # in the plane of 0/1 (det == 0 there), lands on 4


@pytest.mark.parametrize("ties", ["canonical", "reference"])
def test_edge_cases_on_oracle_bvh(oracle, golden_dir, ties):
    """Oracle-built BVH over the edge scene: ids exact (canonical ties), values within tolerance."""
    g = load_golden(golden_dir, "edge_cases.npz")
    rays = np.ascontiguousarray(g["rays"]).view(RAY_DTYPE).reshape(-1)
    tris = g["tris"]
    meshes = []
    for m in np.unique(g["mesh"]):
        meshes.append(dict(positions=tris[g["mesh"] == m].reshape(-1, 3)))
    blob = oracle.build_scene(meshes)
    rc, counts = oracle.validate_blob(blob)
    assert rc == 0 and counts["tris"] == len(tris)
    mode = oracle.TIES_CANONICAL if ties == "canonical" else oracle.TIES_REFERENCE
    hits, mask = oracle.trace(blob, rays, ties=mode, threads=1)
    if ties == "canonical":
        compare_hits_struct(hits, mask, g, "edge/bvh")
    else:
        # first-encountered semantics may pick another of the exact duplicates, never another t
        assert (mask == g["hit_mask"].astype(bool)).all()
        assert np.allclose(hits["t"][mask], g["hit_t"][mask], rtol=1e-5, atol=0)


def test_config1_full_on_oracle_bvh(oracle, golden_dir, scene1):
    g = load_golden(golden_dir, "cfg1_full.npz")
    rays = synth.rays_config1(65536)
    blob = oracle.build_scene([dict(positions=scene1)])
    rc, counts = oracle.validate_blob(blob)
    assert rc == 0 and counts["tris"] == 10000
    hits, mask, ctr = oracle.trace(blob, rays, counters=True)
    st = compare_hits_struct(hits, mask, g, "cfg1/bvh")
    assert st["hits"] == int(g["hit_mask"].sum()) == ctr["hits"]
    assert st["max_rel_t"] < 2e-6


def test_config1_chain_bit_exact_subset(oracle, golden_dir, scene1):
    g = load_golden(golden_dir, "cfg1_full.npz")
    sel = np.arange(0, 65536, 16)
    rays = synth.rays_config1(65536)[sel]
    blobs = oracle.leaf_chain_blobs(scene1.reshape(-1, 3, 3))
    hits, mask = oracle.trace_chain(blobs, rays)
    gs = {k: g[k][sel] for k in ("hit_mask", "hit_mesh", "hit_tri", "hit_t", "hit_u", "hit_v")}
    st = compare_hits_struct(hits, mask, gs, "cfg1/chain")
    assert st["bit_exact"] == 1.0


@pytest.mark.slow
def test_config2_and_3_samples_on_oracle_bvh(oracle, golden_dir, scene2):
    g2 = load_golden(golden_dir, "cfg2_sample.npz")
    g3 = load_golden(golden_dir, "cfg3_sample.npz")
    assert sha(scene2) == str(g2["scene_sha256"])
    blob = oracle.build_scene([dict(positions=scene2)])
    rc, counts = oracle.validate_blob(blob)
    assert rc == 0 and counts["tris"] == 1_000_000
    r2 = np.concatenate([synth.rays_pinhole(first=int(i), count=1) for i in g2["ray_index"]])
    assert sha(r2) == str(g2["rays_sha256"])
    hits, mask = oracle.trace(blob, r2)
    compare_hits_struct(hits, mask, g2, "cfg2/bvh")
    hits, mask = oracle.trace(blob, synth.rays_incoherent(4096))
    compare_hits_struct(hits, mask, g3, "cfg3/bvh")


def test_ray_setup_vectors(oracle):
    """kz = first axis with |d| == max (x, y, z order); sign mask from sign bits (rtk.c:550-556)."""
    def ray(d):
        r = np.zeros(1, RAY_DTYPE)
        r["direction"] = d
        return r
    k, sh, sm = oracle.ray_setup(ray((1, 1, 1)))
    assert list(k) == [1, 2, 0] and sm == 0 and list(sh) == [-1.0, -1.0, 1.0]
    k, sh, sm = oracle.ray_setup(ray((0, -1, 1)))
    assert list(k) == [2, 0, 1] and sm == 2
    k, sh, sm = oracle.ray_setup(ray((-0.0, 0.25, -2)))
    assert list(k) == [0, 1, 2] and sm == 5 and sh[2] == -0.5 and sh[1] == 0.125


def test_exotic_rays_chain_bit_exact(oracle, golden_dir, scene1):
    """2048 rays made of zeros, negative zeros, denormals, huge and tied direction components, far / on-vertex origins,
    empty, reversed and NaN-min intervals (synth.rays_exotic): same leaf chain as the REAL rtk.c saw -> identical hit/miss,
    ids and t/u/v bits. Pins the oracle's ray set-up (rtk.c:550-566) and leaf arithmetic where it is most fragile."""
    g = load_golden(golden_dir, "exotic_rays.npz")
    rays = synth.rays_exotic(2048, tris=scene1)
    assert sha(scene1) == str(g["scene_sha256"]) and sha(rays) == str(g["rays_sha256"])
    blobs = oracle.leaf_chain_blobs(scene1.reshape(-1, 3, 3))
    hits, mask = oracle.trace_chain(blobs, rays)
    gm = g["hit_mask"].astype(bool)
    assert (mask == gm).all()
    assert gm.sum() > 300
    assert (hits["triangle_index"][mask] == g["hit_tri"][gm]).all()
    for f, k in (("t", "hit_t"), ("u", "hit_u"), ("v", "hit_v")):
        assert (hits[f][mask].view(np.uint32) == g[k][gm].view(np.uint32)).all(), f


def _group_redo_ids():
    import os
    from tests.util import group_redo_cases
    return [c.name for c in group_redo_cases(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))]


@pytest.mark.parametrize("name", _group_redo_ids())
def test_group_redo_oracle_equals_the_reference_on_both_orders(oracle, golden_dir, name):
    """tests/golden/group_redo.npz: a ray that starts bit-exactly on a vertex of triangle X has exactly-zero edge functions for X,
    which switches X's whole group of four -- and no other full group -- to the double-precision edge functions (rtk.c:302-336).
    The oracle must return the REAL rtk.c's hit / miss, ids and t, u, v bits on the leaf in order P and on the same triangles in
    order Q (X in another group): that pins its switch for the other three members of a group, which near_ties.npz (four copies
    of one triangle) does not. The precondition every later user of the fixture relies on is asserted here as a condition: with X
    in a full group, at least a quarter of the rays that hit one triangle on P and on Q differ in the bits of t, u or v, so an
    answer equal to P's cannot come from a traversal that grouped differently; with X in the padded group (double anyway) P
    equals Q although Q's float groups are in another order."""
    from tests.util import GROUP_REDO_MIN_SHARE, group_redo_cases
    c = [k for k in group_redo_cases(golden_dir) if k.name == name][0]
    for order, want in (("p", c.p), ("q", c.q)):
        hits, mask = oracle.trace_chain([c.blob(oracle, order)], c.rays, threads=1)
        gm = want["hit_mask"].astype(bool)
        assert (mask == gm).all(), order
        assert (hits["triangle_index"][mask] == want["hit_tri"][gm]).all() and (hits["mesh_index"][mask] == want["hit_mesh"][gm]).all(), order
        for f, k in (("t", "hit_t"), ("u", "hit_u"), ("v", "hit_v")):
            assert (hits[f][mask].view(np.uint32) == want[k][gm].view(np.uint32)).all(), (order, f)
    # rays start on a vertex of X: all three in turn, or the vertex two Xs share
    xs = c.p["tris"][np.isin(c.p["tri"], c.x)]
    on_vertex = (c.rays["origin"][:, None, None, :].view(np.uint32) == xs[None].view(np.uint32)).all(axis=3)
    assert on_vertex.any(axis=(1, 2)).all() and (on_vertex.any(axis=(0, 1)).sum() == 3 or len(c.x) == 2)
    same, differ = c.same_triangle(), c.bits_differ()
    assert same.sum() > len(c.rays) // 2
    if c.control:
        slot = int(np.nonzero(c.p["tri"] == c.x[0])[0][0])
        assert slot // 4 == c.n // 4 and c.n % 4                    # X really is in the padded group
        assert (c.p["tri"] != c.q["tri"]).any()
        assert same.all() or (same == c.p["hit_mask"].astype(bool)).all()
        assert not differ.any() and (c.p["hit_mask"] == c.q["hit_mask"]).all()
    else:
        for x in c.x:
            slot = int(np.nonzero(c.p["tri"] == x)[0][0])
            assert slot // 4 < c.n // 4                              # X is in a full group of P ...
            qslot = int(np.nonzero(c.q["tri"] == x)[0][0])
            mates = set(c.p["tri"][4 * (slot // 4):4 * (slot // 4) + 4]) - {x}
            assert not mates & set(c.q["tri"][4 * (qslot // 4):4 * (qslot // 4) + 4])      # ... and has other company in Q
        assert differ.sum() >= GROUP_REDO_MIN_SHARE * same.sum(), (int(differ.sum()), int(same.sum()))


def test_group_redo_fixture_covers_what_it_says(golden_dir):
    """Leaf sizes 4, 5, 8, 11, 12, 63; X in slot 0 and slot 3 of the first full group, in a middle group, in the last full group and
    in the padded group; two Xs in two full groups of one leaf; X in a mesh of its own."""
    from tests.util import group_redo_cases
    cases = group_redo_cases(golden_dir)
    where = {}
    for c in cases:
        if len(c.x) == 1 and not c.p["mesh"].any():
            slot = int(np.nonzero(c.p["tri"] == c.x[0])[0][0])
            full = c.n // 4
            kind = "padded" if slot // 4 == full else ("slot%d" % slot if slot in (0, 3) else ("last" if slot // 4 == full - 1 else "middle"))
            where.setdefault(c.n, set()).add(kind)
    assert where == {4: {"slot0", "slot3"}, 5: {"slot0", "slot3", "padded"}, 8: {"slot0", "slot3", "last"},
                     11: {"slot0", "slot3", "last", "padded"}, 12: {"slot0", "slot3", "middle", "last"},
                     63: {"slot0", "slot3", "middle", "last", "padded"}}
    two = [c for c in cases if len(c.x) == 2]
    assert len(two) == 1
    g = [int(np.nonzero(two[0].p["tri"] == x)[0][0]) // 4 for x in two[0].x]
    assert g[0] != g[1] and max(g) < two[0].n // 4
    own = [c for c in cases if c.p["mesh"].any()]
    assert len(own) == 1 and (own[0].p["mesh"] == (own[0].p["tri"] == own[0].x[0])).all()
