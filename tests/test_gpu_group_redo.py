"""GPU tests of the group-of-four rule where it is rare: an exactly-zero edge function inside a FULL group (rtk.c:302-336).

A leaf's triangles are tested in groups of four; one exact zero switches its whole group to the double-precision edge functions,
the other full groups stay float. Every traversal carries a copy of that rule: rtk_trace_kernel (closest hit, any hit, the
collecting form behind host filters, the filtered forms), the C++ packet kernel, one_leaf of rtk_trace_one_kernel, and the assembly
kernels by handing such rays back. tests/golden/group_redo.npz holds single leaves of 4 .. 63 triangles in a known order P, rays
that start bit-exactly on a vertex of one triangle X of the leaf, and the REAL rtk.c's answers on P and on the same triangles in
order Q, where X sits in another group. Everything here is compared with P bit for bit -- t, u, v; ids and flags exact; no
tolerance anywhere -- and each test asserts its precondition first: on at least a quarter of the rays that hit one triangle on both
orders, P's and Q's t, u, v differ in their bits, so a traversal that skipped the redo, restored the wrong snapshot, redid the wrong
four slots or left a group early would not return P's. The control cases (X in the padded group, double anyway) have P equal to Q.

The leaves are uploaded as the single-node blobs the reference traced (num_nodes == 1). Batches are the fixture's 252 rays three
times over: 756 rays are more than one workgroup (so that the assembly per-lane kernel, which takes queue-fed batches only, runs
first and must hand the rays back), no multiple of 64, and the copies land in other lanes and waves."""
import ctypes as C
import os

import numpy as np
import pytest

from rtk_amd import synth
from rtk_amd.types import HIT_RECORD_DTYPE, RAY_DTYPE
from tests.util import GROUP_REDO_MIN_SHARE, group_redo_cases

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
REPEAT = 3
CASES = [c.name for c in group_redo_cases(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))]
PER_RAY_CASES = [n for n in CASES if n[:3] in ("n08", "n12", "n63")]
# cases in which many rays have a second candidate behind their first hit (the small leaves mostly have none): the filters' subjects
SECOND_CANDIDATES = ["n08_first3", "n08_last", "n11_first0", "n11_first3", "n12_first0", "n12_first3", "n12_middle", "n12_last",
                     "n63_first0", "n63_first3", "n63_middle", "n63_last"]


class Leaf:
    """one case on the device: the uploaded leaf, P's answers as the records the kernels write, and the rays in three sizes"""

    def __init__(self, api, oracle, c):
        self.c = c
        self.blob = c.blob(oracle)
        self.ds = api.DeviceScene.upload(self.blob)
        info = self.ds.info()
        assert info["num_nodes"] == 1 and info["num_triangles"] == c.n
        self.base = self.ds.mesh_base()
        self.rays = c.rays
        self.many = np.ascontiguousarray(np.tile(c.rays, REPEAT))
        self.want = self.records(c.p)
        self.want_q = self.records(c.q)

    def prims(self, mesh, tri, mask):
        m = np.asarray(mask).astype(bool)
        return np.where(m, self.base[np.where(m, mesh, 0).astype(np.int64)] + np.where(m, tri, 0), NONE).astype(np.uint32)

    def records(self, g):
        r = np.zeros(len(g["hit_mask"]), HIT_RECORD_DTYPE)
        r["t"], r["u"], r["v"] = g["hit_t"], g["hit_u"], g["hit_v"]
        r["prim"] = self.prims(g["hit_mesh"], g["hit_tri"], g["hit_mask"])
        return r

    def precondition(self):
        """P and Q differ on enough rays for equality with P to be evidence; returns how many"""
        same, differ = self.c.same_triangle(), self.c.bits_differ()
        if self.c.control:
            assert not differ.any() and same.sum() > len(self.rays) // 2
        else:
            assert differ.sum() >= GROUP_REDO_MIN_SHARE * same.sum() and same.sum() > len(self.rays) // 2, (int(differ.sum()), int(same.sum()))
            assert self.want.tobytes() != self.want_q.tobytes()
        return int(differ.sum())


def same_records(rec, want, what):
    """prim exact on every ray; t, u, v bit for bit on every hit (`want` may be shorter: the batch is copies of it)"""
    want = want[np.arange(len(rec)) % len(want)]
    assert (rec["prim"] == want["prim"]).all(), "%s: ids differ on rays %s" % (what, np.nonzero(rec["prim"] != want["prim"])[0][:8])
    hit = want["prim"] != NONE
    for f in ("t", "u", "v"):
        bad = np.nonzero(hit & (rec[f].view(np.uint32) != want[f].view(np.uint32)))[0]
        assert bad.size == 0, "%s: %s differs in its bits on %d rays, first %s" % (what, f, bad.size, bad[:8])


@pytest.fixture(scope="module")
def leaves(api, oracle, golden_dir):
    cases = {c.name: c for c in group_redo_cases(golden_dir)}
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Leaf(api, oracle, cases[name])
        return cache[name]
    return get


def image_of(rays, w, h):
    """the batch repeated until it fills a w x h image"""
    return np.ascontiguousarray(rays[np.arange(w * h) % len(rays)])


# ---------------------------------------------------------------- closest hit

@pytest.mark.parametrize("form", ["default", "one_workgroup", "no_asm", "exact_nodes", "static", "sort_rays"])
@pytest.mark.parametrize("name", CASES)
def test_closest_hit_forms(api, leaves, name, form):
    """rtk_trace_kernel MODE 0 behind every launch form; in the default form rtk_lane_hot_closest runs first and hands the rays back.
    The expanded rtk_hit's ids are the fixture's too."""
    L = leaves(name)
    L.precondition()
    opts = {"default": None, "one_workgroup": None, "no_asm": api.make_opts(no_asm=True), "exact_nodes": api.make_opts(exact_nodes=True),
            "static": api.make_opts(static=True), "sort_rays": api.make_opts(sort_rays=True)}[form]
    rays = L.rays if form == "one_workgroup" else L.many
    hits, mask, rec = L.ds.trace(rays, opts=opts)
    same_records(rec, L.want, "%s/%s" % (name, form))
    k = np.arange(len(rays)) % len(L.rays)
    gm = L.c.p["hit_mask"].astype(bool)[k]
    assert (mask == gm).all()
    assert (hits["mesh_index"][mask] == L.c.p["hit_mesh"][k][gm]).all() and (hits["triangle_index"][mask] == L.c.p["hit_tri"][k][gm]).all()
    for f, g in (("t", "hit_t"), ("u", "hit_u"), ("v", "hit_v")):
        assert (hits[f][mask].view(np.uint32) == L.c.p[g][k][gm].view(np.uint32)).all(), f


@pytest.mark.parametrize("name", CASES)
def test_closest_hit_counted_form(api, leaves, name):
    """rtk_dev_trace_rays_counted (the COUNT instantiation): the same records, and every ray meets the one leaf"""
    L = leaves(name)
    L.precondition()
    rec, ctr = L.ds.trace_counted(L.many)
    same_records(rec, L.want, name + "/counted")
    assert rec.tobytes() == L.ds.trace(L.many, full=False).tobytes()
    assert ctr["rays"] == len(L.many) and ctr["leaves"] == len(L.many) and ctr["triangles"] >= L.c.n * len(L.many)


@pytest.mark.parametrize("name", CASES)
def test_closest_hit_as_an_image(api, leaves, name):
    """With an image hint the packet kernels take the batch. 64 x 64: rtk_trace_packet_kernel (pk_leaf's own redo) takes every tile,
    as an image of one block per row is below what the assembly takes. 128 x 64: rtk_packet_beam2 computes full groups in float and
    must hand a pair that meets an exact zero back; the counting form shows that it did, so the hand-back, not the float path,
    produced the answer."""
    L = leaves(name)
    L.precondition()
    small = image_of(L.rays, 64, 64)
    same_records(L.ds.trace(small, opts=api.make_opts(image=(64, 64)), full=False), L.want, name + "/image 64x64")
    frame = image_of(L.rays, 128, 64)
    opts = api.make_opts(image=(128, 64))
    rec = L.ds.trace(frame, opts=opts, full=False)
    same_records(rec, L.want, name + "/image 128x64")
    rec2, pk = L.ds.trace_packet_counted(frame, opts)
    assert rec2.tobytes() == rec.tobytes()
    assert pk["tiles"] == 128 and pk["tiles_handed_back"] > 0, pk


# ---------------------------------------------------------------- any hit

def bounded(L, rays):
    """Intervals from the fixture itself: every even ray ends exactly at P's t (t < max_t fails: a miss), every odd ray one ulp
    behind it (a hit); a ray that misses on P keeps its interval and misses."""
    k = np.arange(len(rays)) % len(L.rays)
    hit = (L.want["prim"] != NONE)[k]
    t = L.want["t"][k]
    odd = (np.arange(len(rays)) & 1) == 1
    out = rays.copy()
    out["max_t"] = np.where(hit, np.where(odd, np.nextafter(t, np.float32(np.inf)), t), rays["max_t"]).astype(np.float32)
    return out, hit & odd


@pytest.mark.parametrize("name", CASES)
def test_any_hit_on_intervals_one_ulp_apart(api, leaves, name):
    """rtk_trace_kernel MODE 1 (the any-hit form leaves a leaf at a group boundary once a group accepted something, which must not
    cut a redo short), with and without the assembly, and as an image (rtk_packet_any2 hands back, the C++ packet kernel answers).
    Precondition: had a kernel computed Q's t for a ray, some of these flags would flip."""
    L = leaves(name)
    L.precondition()
    # (the fixture's ray count is even, so a ray keeps its parity in every copy)
    assert len(L.rays) % 2 == 0
    same = L.c.same_triangle()
    tp, tq = L.want["t"], L.want_q["t"]
    odd = (np.arange(len(L.rays)) & 1) == 1
    flips = same & np.where(odd, ~(tq < np.nextafter(tp, np.float32(np.inf))), tq < tp)
    assert flips.any() or L.c.control, name
    rays, want = bounded(L, L.many)
    assert want.any() and not want.all()
    for what, opts in (("default", None), ("no_asm", api.make_opts(no_asm=True)), ("exact_nodes", api.make_opts(exact_nodes=True))):
        assert (L.ds.trace_any(rays, opts=opts) == want).all(), (name, what)
    occ, ctr = L.ds.trace_any_counted(rays)
    assert (occ == want).all() and ctr["rays"] == len(rays)
    for w, h in ((64, 64), (128, 64)):
        frame, fwant = bounded(L, image_of(L.rays, w, h))
        assert (L.ds.trace_any(frame, opts=api.make_opts(image=(w, h))) == fwant).all(), (name, w, h)
    # and the closest-hit kernels on the same intervals: the hit survives an interval that ends one ulp behind it
    rec = L.ds.trace(rays, opts=api.make_opts(no_asm=True), full=False)
    assert ((rec["prim"] != NONE) == want).all()
    same_records(rec[want], L.want[(np.arange(len(rays)) % len(L.rays))[want]], name + "/bounded closest")


# ---------------------------------------------------------------- device filters

def oracle_records(L, oh, om):
    r = np.zeros(len(om), HIT_RECORD_DTYPE)
    r["t"], r["u"], r["v"] = oh["t"], oh["u"], oh["v"]
    r["prim"] = L.prims(oh["mesh_index"], oh["triangle_index"], om)
    return r


@pytest.mark.parametrize("name", CASES)
def test_device_filters(api, oracle, leaves, name):
    """The FILT forms apply the ignored primitive, `after` and the mesh mask to candidates of a redone group: against
    oracle.trace_filtered on the same blob, closest hit and any hit. With X in a mesh of its own and that mesh hidden, X is
    invisible but its zero still switches its group: the result keeps P's bits, not Q's."""
    L = leaves(name)
    L.precondition()
    rays = L.many
    k = np.arange(len(rays)) % len(L.rays)
    p = L.c.p
    hit = p["hit_mask"].astype(bool)[k]
    pm = np.where(hit, p["hit_mesh"][k], NONE).astype(np.uint32)
    pt = np.where(hit, p["hit_tri"][k], 0).astype(np.uint32)
    plain = np.ascontiguousarray(L.want[k])

    # the primitive each ray hits first is ignored: the next candidate, often of the same (redone) group
    rec = L.ds.trace_filtered(rays, ignore_prim=plain["prim"].copy())
    oh, om = oracle.trace_filtered(L.blob, rays, ignore=(pm, pt))
    same_records(rec, oracle_records(L, oh, om), name + "/ignore_prim")
    assert ((rec["prim"] != plain["prim"]) | ~hit).all()
    if name in SECOND_CANDIDATES:
        # precondition of its own: the second candidates' bits depend on the grouping too (the oracle on Q, which the CPU tests pin)
        qh, qm = oracle.trace_filtered(L.c.blob(oracle, "q"), rays, ignore=(pm, pt))
        both = om & qm & (oh["triangle_index"] == qh["triangle_index"])
        assert (both & ((oh["t"].view(np.uint32) != qh["t"].view(np.uint32)) | (oh["u"].view(np.uint32) != qh["u"].view(np.uint32)) |
                        (oh["v"].view(np.uint32) != qh["v"].view(np.uint32)))).sum() >= 10 * REPEAT
    assert (L.ds.trace_filtered(rays, ignore_prim=plain["prim"].copy(), any_hit=True) == om).all()
    for opts in (api.make_opts(exact_nodes=True), api.make_opts(static=True)):
        assert L.ds.trace_filtered(rays, ignore_prim=plain["prim"].copy(), opts=opts).tobytes() == rec.tobytes()

    # continuation behind P's own records
    rec3 = L.ds.trace_filtered(rays, after=plain)
    oh3, om3 = oracle.trace_filtered(L.blob, rays, after=(plain["t"], pm, pt))
    same_records(rec3, oracle_records(L, oh3, om3), name + "/after")
    assert (L.ds.trace_filtered(rays, after=plain, any_hit=True) == om3).all()
    # ... and behind a record just in front of them: P's hit itself comes back, in P's bits
    before = plain.copy()
    before["t"] = np.where(hit, np.nextafter(plain["t"], np.float32(-np.inf)), plain["t"])
    same_records(L.ds.trace_filtered(rays, after=before), L.want, name + "/after, one ulp in front")

    # mesh mask
    nm = int(p["mesh"].max()) + 1
    vis = [True] + [False] * (nm - 1)
    rec4 = L.ds.trace_filtered(rays, mesh_mask=vis)
    oh4, om4 = oracle.trace_filtered(L.blob, rays, mesh_mask=vis)
    same_records(rec4, oracle_records(L, oh4, om4), name + "/mesh_mask")
    assert (L.ds.trace_filtered(rays, mesh_mask=vis, any_hit=True) == om4).all()
    visible = hit & (pm == 0)
    assert visible.sum() > len(rays) // 2
    same_records(rec4[visible], plain[visible], name + "/mesh_mask keeps P's bits")
    if nm > 1:
        # X is hidden: no ray reports it, and on the rays where P and Q differ the answer is P's, so it is not Q's
        x_prim = L.prims(np.array([1]), np.array([int(L.c.x[0])]), np.array([True]))[0]
        assert (rec4["prim"] != x_prim).all()
        d = L.c.bits_differ()[k] & visible
        assert d.sum() > 100 and (rec4[d] != L.want_q[k][d]).all()


# ---------------------------------------------------------------- host filter batch

@pytest.mark.parametrize("name", ["n08_first3", "n08_last", "n11_first3", "n12_first3", "n12_two", "n63_middle", "n63_padded"])
def test_host_filter_batch(api, oracle, leaves, name):
    """rtk_trace_rays_filter collects candidate lists on the device (MODE 2 cannot undo an insertion: it scans a full group for zeros,
    then evaluates it). The predicate rejects each ray's first candidate; the answer is oracle.trace_filtered's with the same
    predicate, which is also the device's ignore_prim answer."""
    L = leaves(name)
    L.precondition()
    rays = L.many
    k = np.arange(len(rays)) % len(L.rays)
    p = L.c.p
    first = set((int(i), int(p["hit_mesh"][j]), int(p["hit_tri"][j])) for i, j in enumerate(k) if p["hit_mask"][j])
    offered = []

    def pred(i, hit):
        offered.append(int(i))
        return (int(i), int(hit["mesh_index"]), int(hit["triangle_index"])) not in first
    try:
        hits, mask = api.trace_rays_filter(L.blob.ptr, rays, pred)
        plain_hits, plain_mask = api.trace_rays(L.blob.ptr, rays)
    finally:
        api.lib().rtk_amd_forget_scene(C.c_void_p(L.blob.ptr))
    assert len(set(offered)) == int(p["hit_mask"][k].sum())
    oh, om = oracle.trace_filtered(L.blob, rays, callback=pred)
    assert (mask == om).all() and mask.sum() >= 10 * REPEAT
    same_records(oracle_records(L, hits, mask), oracle_records(L, oh, om), name + "/host filter")
    # the unfiltered host batch is P
    same_records(oracle_records(L, plain_hits, plain_mask), L.want, name + "/rtk_trace_rays")
    # the first candidate that was offered and rejected was P's hit in P's bits, or the filtered answer would differ from ignore_prim's
    rec = L.ds.trace_filtered(rays, ignore_prim=np.ascontiguousarray(L.want[k])["prim"].copy())
    same_records(oracle_records(L, hits, mask), rec, name + "/host filter vs ignore_prim")


# ---------------------------------------------------------------- per-ray calls

@pytest.fixture
def per_ray_on_gpu(api):
    api.lib().rtk_amd_set_per_ray(1)
    yield
    api.lib().rtk_amd_set_per_ray(0)


@pytest.mark.parametrize("name", PER_RAY_CASES)
def test_single_ray_kernel(api, oracle, leaves, per_ray_on_gpu, name):
    """rtk_amd_set_per_ray(RTK_AMD_PER_RAY_GPU): rtk_trace_ray runs rtk_trace_one_kernel, whose one_leaf is a copy of the redo of its
    own. Every field of rtk_hit equals the batch call's and, for ids and t, u, v, the fixture's."""
    L = leaves(name)
    L.precondition()
    p = L.c.p
    try:
        hits, mask = api.trace_rays(L.blob.ptr, L.rays)
        assert (mask == p["hit_mask"].astype(bool)).all()
        for i in range(len(L.rays)):
            one = api.trace_ray(L.blob.ptr, L.rays[i])
            assert (one is not None) == bool(p["hit_mask"][i]), (name, i)
            if one is None:
                continue
            assert one.tobytes() == hits[i].tobytes(), (name, i, one, hits[i])
            assert int(one["mesh_index"]) == p["hit_mesh"][i] and int(one["triangle_index"]) == p["hit_tri"][i], (name, i)
            for f, g in (("t", "hit_t"), ("u", "hit_u"), ("v", "hit_v")):
                assert np.float32(one[f]).view(np.uint32) == p[g][i].view(np.uint32), (name, i, f)
    finally:
        api.lib().rtk_amd_forget_scene(C.c_void_p(L.blob.ptr))
    oh, om = oracle.trace(L.blob, L.rays)
    assert hits[mask].tobytes() == oh[om].tobytes()


# ---------------------------------------------------------------- listed tracing

@pytest.mark.parametrize("name", ["n12_two"])
def test_listed_every_third(api, leaves, name):
    """rtk_dev_trace_rays_listed with every third ray: the assembly's listed kernel hands every ray back, so the caller's list and
    the kernels' own left-over list are both live. Listed slots are P, the others untouched; any-hit alike."""
    import torch
    L = leaves(name)
    L.precondition()
    n = len(L.many)
    ids = np.arange(0, n, 3, dtype=np.int64)
    d_rays = api.to_device(L.many)
    d_ids = torch.from_numpy(ids).cuda()
    d_count = torch.tensor([len(ids)], dtype=torch.int64, device="cuda")
    for opts in (None, api.make_opts(no_asm=True)):
        out = torch.full((n * 16,), 0x7e, dtype=torch.uint8, device="cuda")
        L.ds.trace_listed_device(d_rays, n, d_count, d_ids, out, opts=opts)
        got = out.cpu().numpy().view(HIT_RECORD_DTYPE)
        same_records(got[ids], L.want[ids % len(L.rays)], name + "/listed")
        rest = np.ones(n, bool)
        rest[ids] = False
        assert (got[rest].view(np.uint8) == 0x7e).all()
    rays, want = bounded(L, L.many)
    out = torch.full((n,), 0x7e, dtype=torch.uint8, device="cuda")
    L.ds.trace_any_listed_device(api.to_device(rays), n, d_count, d_ids, out)
    got = out.cpu().numpy()
    assert (got[ids].astype(bool) == want[ids]).all() and (got[rest] == 0x7e).all()


# ---------------------------------------------------------------- one tree

def test_one_tree_of_the_references_leaf_sizes(api, oracle):
    """The same overlapping soup as one scene: oracle.build_scene makes leaves of 4 to 63 triangles, rays start on vertices of every
    7th triangle (exact zeros wherever that triangle's leaf puts it) and aim at triangle centroids. The GPU on the uploaded blob --
    default, without the assembly, as an image, any hit -- against oracle.trace on the same blob, bit for bit."""
    n = 2000
    tv = synth.triangle_soup(n, 0.6, seed=78).reshape(n, 3, 3)
    blob = oracle.build_scene([dict(positions=tv.reshape(-1, 3))])
    rc, counts = oracle.validate_blob(blob)
    assert rc == 0 and counts["tris"] == n and 3 * counts["leaves"] < n         # so there are leaves of four and more: full groups
    w, h = 128, 64
    r = np.arange(w * h)
    xs = np.arange(0, n, 7)
    rays = np.zeros(w * h, RAY_DTYPE)
    rays["origin"] = tv[xs[r % len(xs)], (r // len(xs)) % 3]
    centroid = (tv[:, 0] + tv[:, 1] + tv[:, 2]) * np.float32(1.0 / 3.0)
    rays["direction"] = centroid[(r * 37 + 11) % n] - rays["origin"]
    rays["max_t"] = np.float32(3e38)
    oh, om = oracle.trace(blob, rays)
    assert om.sum() > len(rays) // 2
    ds = api.DeviceScene.upload(blob)
    assert ds.info()["num_meshes"] == 1
    want = np.zeros(len(rays), HIT_RECORD_DTYPE)
    want["t"], want["u"], want["v"] = oh["t"], oh["u"], oh["v"]
    want["prim"] = np.where(om, oh["triangle_index"], NONE)
    for what, opts in (("default", None), ("no_asm", api.make_opts(no_asm=True)), ("no_detect", api.make_opts(no_detect=True)),
                       ("image", api.make_opts(image=(w, h))), ("exact_nodes", api.make_opts(exact_nodes=True))):
        same_records(ds.trace(rays, opts=opts, full=False), want, "tree/" + what)
    odd = rays[:len(rays) - 3]                                              # no image: the per-lane kernels, whatever the look says
    same_records(ds.trace(odd, full=False), want[:len(odd)], "tree/per lane")
    for opts in (None, api.make_opts(no_asm=True), api.make_opts(image=(w, h))):
        assert (ds.trace_any(rays, opts=opts) == om).all()
    assert (ds.trace_any(odd) == om[:len(odd)]).all()
