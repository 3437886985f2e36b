"""GPU tests of the entry-list pre-pass of image frames (rtk_packet_entries_kernel, read back through
rtk_dev_debug_packet_entries): the lists are what the specification gives, run on the scene's own exported nodes; blocks that
must not get a list get none while their neighbours keep theirs; the records of a frame do not depend on the lists; and the
launch's counters start from zero.

The specification is beam_entries, the Python port in tests/test_packet_asm_emulated.py -- with the one step the kernel has
gained since the port was written: the reciprocal box is widened by two ulps (rlo -= 2^-22 |rlo|, rhi += 2^-22 |rhi|) before
the margins are formed, so that rtk_packet_beam2's v_rcp_f32 reciprocals fit the box of the correctly rounded ones. The
emulated assembly tests feed the port's lists to the kernels, which take either box, so the port itself has stayed as it
was. spec_entries below is the port with that step (and the depth cap as a parameter); test_specification_is_the_port_plus_the_widening
holds it to beam_entries, byte for byte, with the step switched off.

Frames of 256 x 192 pixels: 12 blocks of 64 x 64, four per row in three rows."""
import numpy as np
import pytest

from rtk_amd import synth
from rtk_amd.types import SceneHeader

from .test_packet_asm_emulated import ENTRIES, beam_entries

pytestmark = pytest.mark.gpu

W, H = 256, 192
NBLK = (W // 64) * (H // 64)
NONE, LEAF = 0xFFFFFFFF, 0x80000000
SPEC_LEVELS = 14              # the depth cap beam_entries is written with
NODE = np.dtype([("bx", "<f4", (2, 4)), ("by", "<f4", (2, 4)), ("bz", "<f4", (2, 4)), ("child", "<u4", (4,)), ("order", "<u4", (4,))])


def spec_entries(nodes, rays, w, h, bound, target, levels=SPEC_LEVELS, widen=True):
    """beam_entries (tests/test_packet_asm_emulated.py), statement for statement, plus the widening of the reciprocal box; the
    four children of a node are tested as one float32 array (the same float32 operations in the same order)."""
    f = np.float32
    bpr, rows = w // 64, h // 64
    out = np.zeros(bpr * rows, dtype=ENTRIES)
    img = rays.reshape(h, w)
    with np.errstate(all="ignore"):
        for blk in range(bpr * rows):
            bx, by = blk % bpr, blk // bpr
            sub = img[by * 64:by * 64 + 64, bx * 64:bx * 64 + 64]
            at = np.array([0, 31, 63])
            edge = sub[np.ix_(at, at)].reshape(-1)
            o, d = edge["origin"], edge["direction"]
            rd = (f(1.0) / d).astype(f)
            e = out[blk]
            rlo, rhi = rd.min(axis=0), rd.max(axis=0)
            if widen:
                rlo, rhi = (rlo - f(2.0 ** -22) * np.abs(rlo)).astype(f), (rhi + f(2.0 ** -22) * np.abs(rhi)).astype(f)
            e["olo"], e["ohi"], e["rlo"], e["rhi"] = o.min(axis=0), o.max(axis=0), rlo, rhi
            e["tmin"] = edge["min_t"].min()
            neg = np.signbit(d)
            ok = (neg.all(axis=0) | (~neg).all(axis=0)).all() and (np.abs(o) < 2.0 ** 19).all() and (np.abs(rd) > 2.0 ** -100).all() and \
                (np.abs(rd) < 2.0 ** 100).all() and bound < 2.0 ** 19 and not np.isnan(edge["min_t"]).any() and not np.isnan(edge["max_t"]).any()
            if not ok:
                continue
            neg = neg[0]
            m = (f(2.0 ** -21) * (np.maximum(np.abs(e["rlo"]), np.abs(e["rhi"])) * (np.maximum(np.abs(e["olo"]), np.abs(e["ohi"])) + f(bound)))).astype(f)
            olo, ohi, rlo, rhi = e["olo"].copy(), e["ohi"].copy(), e["rlo"].copy(), e["rhi"].copy()

            def children(nd):
                n, far = np.full(4, e["tmin"], f), np.full(4, np.inf, f)
                for a, ax in enumerate(("bx", "by", "bz")):
                    lo, hi = nd[ax][0], nd[ax][1]
                    pn, pf = (hi, lo) if neg[a] else (lo, hi)
                    ns = [(pn - oo) * rr for oo in (olo[a], ohi[a]) for rr in (rlo[a], rhi[a])]
                    fs = [(pf - oo) * rr for oo in (olo[a], ohi[a]) for rr in (rlo[a], rhi[a])]
                    assert ns[0].dtype == f
                    n = np.maximum(n, np.minimum(np.minimum(ns[0], ns[1]), np.minimum(ns[2], ns[3])) - m[a])
                    far = np.minimum(far, np.maximum(np.maximum(fs[0], fs[1]), np.maximum(fs[2], fs[3])) + m[a])
                return n <= far, n
            cur, listed, over = [(0, f(e["tmin"]))], [], False
            for level in range(levels):
                if not cur or (level > 0 and len(listed) + len(cur) >= target):
                    break
                nxt = []
                for ref, t_self in cur:
                    nd = nodes[ref]
                    ok_k, tlo = children(nd)
                    reached = [(int(nd["child"][k]), tlo[k]) for k in range(4) if int(nd["child"][k]) != NONE and ok_k[k]]
                    if any(c & LEAF for c, _ in reached):
                        listed.append((ref, t_self))
                    else:
                        nxt += reached
                over = over or len(listed) > 56 or len(nxt) > 128
                if over:
                    break
                cur = nxt
            listed += cur
            if over or len(listed) > 56:
                continue
            order = sorted(range(len(listed)), key=lambda i: (listed[i][1], i))
            e["count"] = len(listed)
            for q, i in enumerate(order):
                e["e"][q] = (listed[i][0], listed[i][1])
    return out


def exported_nodes(ds):
    """The device's nodes from the exported blob: node i of the blob is node i of the device, its 24 planes are the device's
    bytes; child pointers back to references (inner: the index; a leaf: tagged, the slot does not matter here; none)."""
    blob = ds.export_blob()
    hdr = SceneHeader.from_buffer_copy(blob[:56].tobytes())
    n = (int(hdr.leaf_offset) - int(hdr.node_offset)) // 128
    raw = blob[int(hdr.node_offset):int(hdr.node_offset) + n * 128]
    ptr = raw.view(np.uint64).reshape(n, 16)[:, 12:16]
    leaf = (ptr & np.uint64(1)) != 0
    inner = ((ptr - np.uint64(hdr.node_offset)) // np.uint64(128)).astype(np.uint32)
    # (padding nodes past the last one a pointer reaches do not matter: nothing refers to them)
    nodes = np.zeros(n, dtype=NODE)
    planes = raw.view(np.float32).reshape(n, 32)[:, :24]
    nodes["bx"], nodes["by"], nodes["bz"] = planes[:, 0:8].reshape(n, 2, 4), planes[:, 8:16].reshape(n, 2, 4), planes[:, 16:24].reshape(n, 2, 4)
    nodes["child"] = np.where(leaf, np.where(ptr == (np.uint64(hdr.leaf_offset) | np.uint64(1)), np.uint32(NONE), np.uint32(LEAF)), inner)
    return nodes


def scene_bound(nodes):
    """max(largest |plane| of the root's children, 1): what the library passes to the pre-pass for a scene it built."""
    root, b = nodes[0], 1.0
    for k in range(4):
        if root["child"][k] != NONE:
            b = max([b] + [abs(float(root[ax][s][k])) for ax in ("bx", "by", "bz") for s in (0, 1)])
    return np.float32(b)


def octant_frame(o):
    """The off-axis cameras of test_packet_beam_kernel_on_every_octant..., at this size: every ray has octant o's signs."""
    r = synth.rays_pinhole(W, H).copy()
    sx, sy, sz = (-1.0 if o & 1 else 1.0), (-1.0 if o & 2 else 1.0), (-1.0 if o & 4 else 1.0)
    r["direction"][:, 0] = (np.abs(r["direction"][:, 0]) * np.float32(0.5) + np.float32(0.05)) * np.float32(sx)
    r["direction"][:, 1] = (np.abs(r["direction"][:, 1]) * np.float32(0.5) + np.float32(0.05)) * np.float32(sy)
    r["direction"][:, 2] = np.float32(sz)
    r["origin"] = (0.5 - 0.35 * sx, 0.5 - 0.35 * sy, 0.5 - 2.0 * sz)
    return r


def inside_frame():
    """One-signed rays from a point inside the scene: every block's beam reaches many nodes at once."""
    r = octant_frame(0)
    r["origin"] = (0.3, 0.3, 0.2)
    return r


def edge_frame():
    """The pinhole camera moved so that its top-left block looks past the scene's corner: few nodes per level there."""
    r = synth.rays_pinhole(W, H).copy()
    r["origin"] = (0.3, 0.3, -1.5)
    return r


def frames():
    return [("pinhole", synth.rays_pinhole(W, H))] + [("octant %d" % o, octant_frame(o)) for o in range(8)] + [("inside", inside_frame()), ("edge", edge_frame())]


@pytest.fixture(scope="module")
def scene(api):
    tris = synth.triangle_soup(20_000, 0.05, 7)
    ds = api.DeviceScene.build([dict(positions=tris)])
    nodes = exported_nodes(ds)
    return ds, nodes, scene_bound(nodes)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_block(got, want, nodes, what):
    assert int(got["count"]) == int(want["count"]), what
    for f in ("olo", "ohi", "rlo", "rhi", "tmin"):
        assert (bits(got[f]) == bits(want[f])).all(), (what, f)
    n = int(got["count"])
    assert n <= 56
    g, s = got["e"][:n], want["e"][:n]
    assert sorted(zip(g["ref"].tolist(), bits(g["tlo"]).tolist())) == sorted(zip(s["ref"].tolist(), bits(s["tlo"]).tolist())), what
    assert (g["tlo"][1:] >= g["tlo"][:-1]).all(), what
    assert ((g["ref"] & LEAF) == 0).all() and (g["ref"] < len(nodes)).all(), what


def test_specification_is_the_port_plus_the_widening(api, scene):
    ds, nodes, bound = scene
    for rays in (synth.rays_pinhole(W, H), octant_frame(5)):
        port, spec = beam_entries(nodes, rays, W, H, bound, target=26), spec_entries(nodes, rays, W, H, bound, 26, widen=False)
        assert (port["count"] > 0).sum() >= 8
        for blk in range(NBLK):
            assert port[blk].tobytes() == spec[blk].tobytes(), blk
        # ... and the kernel's beam is the port's, the reciprocal box two ulps wider
        got = ds.debug_packet_entries(rays, W, H, target=26, max_levels=SPEC_LEVELS)
        f = np.float32
        for fld in ("olo", "ohi", "tmin"):
            assert (bits(got[fld]) == bits(port[fld])).all(), fld
        assert (bits(got["rlo"]) == bits((port["rlo"] - f(2.0 ** -22) * np.abs(port["rlo"])).astype(f))).all()
        assert (bits(got["rhi"]) == bits((port["rhi"] + f(2.0 ** -22) * np.abs(port["rhi"])).astype(f))).all()
        assert ((got["count"] == 0) == (port["count"] == 0)).all()


def test_lists_equal_the_specification(api, scene):
    ds, nodes, bound = scene
    assert api.PACKET_ENTRIES_DTYPE == ENTRIES
    listed = 0
    for name, rays in frames():
        # every frame at the standing target; the three frames that differ in kind also at the smallest and the largest one
        for target in ((6, 26, 56) if name in ("pinhole", "inside", "edge") else (26,)):
            got = ds.debug_packet_entries(rays, W, H, target=target, max_levels=SPEC_LEVELS)
            want = spec_entries(nodes, rays, W, H, bound, target)
            print(name, "target", target, "counts", got["count"].tolist(), "spec", want["count"].tolist())
            for blk in range(NBLK):
                check_block(got[blk], want[blk], nodes, (name, target, blk))
            listed += int((got["count"] > 0).sum())
    assert listed > 100
    # the level cap (the library's own knobs are 26 entries and 8 levels): the edge frame's top-left block looks past the scene's
    # corner, finds few nodes per level and is cut short by it; no level at all lists the root alone
    edge = dict(frames())["edge"]
    for levels in (0, 1, 3, 8):
        got, want = ds.debug_packet_entries(edge, W, H, target=26, max_levels=levels), spec_entries(nodes, edge, W, H, bound, 26, levels=levels)
        print("edge, levels", levels, "counts", got["count"].tolist(), "spec", want["count"].tolist())
        for blk in range(NBLK):
            check_block(got[blk], want[blk], nodes, ("edge", levels, blk))
    assert (ds.debug_packet_entries(edge, W, H)["count"] == got["count"]).all()
    capped, full = spec_entries(nodes, edge, W, H, bound, 26, levels=3), spec_entries(nodes, edge, W, H, bound, 26)
    assert (capped["count"] != full["count"]).any()


def test_blocks_that_must_not_get_a_list(api, scene):
    ds, nodes, bound = scene
    # mixed direction signs: the pinhole camera's axis runs along the middle row of blocks (y = 96), between the columns (x = 128)
    got = ds.debug_packet_entries(synth.rays_pinhole(W, H), W, H, target=26, max_levels=SPEC_LEVELS)
    assert (got["count"][4:8] == 0).all() and (got["count"][:4] > 0).all() and (got["count"][8:] > 0).all()
    # rays that are not tame, and a NaN min_t, each on one of the nine pixels its block samples
    clean = octant_frame(0)
    base = ds.debug_packet_entries(clean, W, H, target=26, max_levels=SPEC_LEVELS)
    assert (base["count"] > 0).all()
    broken = clean.copy().reshape(H, W)
    broken["origin"][64 + 31, 64 + 31, 1] = np.float32(2.0 ** 19)          # block 5, its centre
    broken["direction"][128 + 63, 128 + 0, 0] = np.float32(0.0)           # block 10, its bottom-left corner
    broken["min_t"][0 + 31, 128 + 63] = np.float32(np.nan)                # block 2, the middle of its right edge
    broken["origin"][0 + 0, 192 + 31, 0] = np.float32(-2.0 ** 19)         # block 3, the middle of its top edge
    got = ds.debug_packet_entries(broken.reshape(-1), W, H, target=26, max_levels=SPEC_LEVELS)
    bad = [5, 10, 2, 3]
    assert (got["count"][bad] == 0).all()
    for blk in range(NBLK):
        if blk not in bad:
            assert got[blk].tobytes()[:64 + 8 * int(base[blk]["count"])] == base[blk].tobytes()[:64 + 8 * int(base[blk]["count"])], blk
    # ... and a pixel the pre-pass does not sample changes nothing
    unseen = clean.copy().reshape(H, W)
    unseen["min_t"][5, 7] = np.float32(np.nan)
    got = ds.debug_packet_entries(unseen.reshape(-1), W, H, target=26, max_levels=SPEC_LEVELS)
    assert int(got[0]["count"]) == int(base[0]["count"]) > 0
    # a list that would exceed 56 entries: the largest target, from inside the scene and from the pinhole camera. The
    # specification says which blocks: those it lists at target 6 and not at 56; their neighbours keep their lists.
    overs = 0
    for name, rays in (("inside", inside_frame()), ("pinhole", synth.rays_pinhole(W, H))):
        small, want = spec_entries(nodes, rays, W, H, bound, 6), spec_entries(nodes, rays, W, H, bound, 56)
        got = ds.debug_packet_entries(rays, W, H, target=56, max_levels=SPEC_LEVELS)
        print(name, "target 56: counts", got["count"].tolist(), "spec", want["count"].tolist(), "at target 6", small["count"].tolist())
        overs += int(((want["count"] == 0) & (small["count"] > 0)).sum())
        for blk in range(NBLK):
            check_block(got[blk], want[blk], nodes, (name, 56, blk))
    assert overs > 0


def negative_min_t_frame():
    r = synth.rays_pinhole(W, H).copy()
    r["min_t"] = -1.0
    return r


def test_records_do_not_depend_on_the_lists(api, scene):
    ds, nodes, bound = scene
    hit = 0.0
    for name, rays in frames() + [("negative min_t", negative_min_t_frame())]:
        for no_asm in (False, True):
            with_lists = ds.trace(rays, opts=api.make_opts(image=(W, H), no_asm=no_asm), full=False)
            from_root = ds.trace(rays, opts=api.make_opts(image=(W, H), no_asm=no_asm, no_entries=True), full=False)
            assert with_lists.tobytes() == from_root.tobytes(), (name, no_asm)
        hit = max(hit, float((from_root["prim"] != NONE).mean()))
    assert hit > 0.5


def test_counters_start_from_zero(api, scene):
    """The pre-pass clears the launch's queue heads and counters. A frame whose tiles are all handed back leaves the hand-over
    words set; the counting launch after it must not see them."""
    ds, nodes, bound = scene
    clean = octant_frame(0)
    opts = api.make_opts(image=(W, H))
    rec0, fresh = ds.trace_packet_counted(clean, opts)
    ds.trace(negative_min_t_frame(), opts=opts, full=False)
    ds.trace(clean, opts=opts, full=False)
    _, handed = ds.trace_packet_counted(negative_min_t_frame(), opts)
    rec1, again = ds.trace_packet_counted(clean, opts)
    print(fresh, handed, again)
    assert handed["tiles_handed_back"] > 0 and fresh["tiles_handed_back"] < handed["tiles_handed_back"]
    assert again["tiles"] * 64 == W * H and again == fresh
    assert rec1.tobytes() == rec0.tobytes()
