"""rtk_dev_scene_validate against tests/blob_reference.py, a check of the same blob in numpy and Python that shares no code with it;
and the producers of finished nodes against each other.

Valid scenes: device builds at 2 .. 10 000 triangles (1023 .. 1025 straddle the 1024-triangle refit tile), the tile collapse forced at
1025 and 10 000, and the 10 000-triangle scene after a refit, after split_leaves() of the uploaded oracle blob, after rebuild(): the
validator says ok, the reference on export_blob() says no violation, no loose box, every primitive once, and both count the same
nodes, leaves and triangles.

Mutants: one edit each of a base blob -- the oracle's SAH blob of triangle_soup(300, 0.2, seed=4), and the exported blob of the device
build of 1025 triangles -- uploaded, validated, and given to the reference as the same bytes. No mutant may upload and validate ok
except an outward step; a mutant that uploads and is reported is traced once and leaves no error word.

  edit                                                              reference               upload / validator
  one plane of one child box one float32 step INWARD: every         box_violations 1 at     not ok: box_violations, loose_boxes and
    non-empty slot, axis, min and max, at the root (with an inner     the node (+1 loose      first_bad_index are the reference's
    child) and at a deepest inner node (leaf children: every plane    above it if the node's
    of an exact box is touched by a vertex)                           union shrank)
  the same planes one step OUTWARD                                  loose_boxes 1; if the   ok, loose_boxes 1, box_violations 0; where
                                                                      node's union grew, 1    the union grew not ok, counts and
                                                                      violation at its parent first_bad_index (the parent) the reference's
  a NaN in a plane                                                  bad_empty_slots         refused
  an empty slot weakened to +2 / -2 on all axes                     bad_empty_slots         refused
  an empty slot weakened to +1 / -1, +1 / -1, 0 / 0                 bad_empty_slots         refused
  one triangle given its leaf neighbour's primitive id              an id twice, one never  primitive_id_errors
  a leaf count lowered by one                                       an id never             primitive_id_errors
  a leaf count raised by one (the all-zero padding record behind    an id twice             primitive_id_errors
    the leaf's last becomes a triangle: the next record there is;     (full leaf: not clean)  (full leaf: that, or refused)
    where every leaf is full to a multiple of four, the head of its
    mesh table does, and the table is read further on)
  a leaf count of 0                                                 leaf_count_errors       primitive_id_errors (the loader takes the
                                                                                              slot for an empty one; its ids are missed)
  a child word pointing at another child's leaf                     shared                  refused
  a child word pointing at an ancestor (the root)                   shared                  refused
  a child word pointing past the last node (past the blob)          out_of_range            refused

Rules these rest on: a slot inverted or NaN on some axis is an empty slot to a blob's readers, and must then be exactly
+1 / -1 on every axis -- the loader refuses anything else, where it used to rewrite the box and drop the subtree; every primitive
id of an uploaded blob occurs once, as in a built scene -- the validator used to let ids go unused whenever the counts differed.
A blob has no end-of-leaf flag (the loader derives it from the count), so "the last-triangle flag cleared" has no blob form; and
the loader's tree check leaves bad_references, leaf_format_errors, triangles_missing / _duplicated and nodes_unreachable / _shared
nothing to count in an uploaded scene: they guard the device's own producers.
(A plane of a box that is flat on that axis is left alone: a step inward inverts it, which is the NaN mutant's case.)
The reference alone says which mutants are defects; that it flags every one with the field named above and neither base blob is
checked without a GPU (the first base blob, and an oracle blob of 1025 triangles standing in for the second, which needs a device).

Producers: the tile collapse (eight lanes per node, rows transposed through lane exchanges, the compressed node stored as four
uint4 pieces) and k_top_finish finish the nodes of a build with RTK_AMD_TILE_COLLAPSE_MIN=0; a full refit with the very same
vertices rewrites every order word and every compressed node through k_quantize (rtk_refit.hip calls rtk_quantize_nodes with
only_first = 0xffffffff). Hash, records and every step counter of the packet and the per-lane kernels are the same before and
after: one differing order word or compressed byte moves a counter."""
import numpy as np
import pytest

from rtk_amd import synth
from rtk_amd.api import RtkError
from tests import blob_reference
from tests.test_gpu_refit import _as_blob, deform


def _nodes(buf):
    """The blob's nodes breadth-first: dicts of off, number, depth, parent (number), box [3, 2, 4], words, live (non-empty slots)"""
    out, todo, qi = [], [(128, 1, None)], 0
    while qi < len(todo):
        off, depth, parent = todo[qi]
        box = np.frombuffer(buf, "<f4", 24, off).reshape(3, 2, 4)
        words = [int(w) for w in np.frombuffer(buf, "<u8", 4, off + 96)]
        live = [k for k in range(4) if (box[:, 0, k] <= box[:, 1, k]).all()]
        todo.extend((words[k], depth + 1, qi) for k in live if not words[k] & 1)
        out.append(dict(off=off, number=qi, depth=depth, parent=parent, box=box, words=words, live=live))
        qi += 1
    return out


def _root_and_deepest(nodes):
    """The root, which must have an inner child, and a deepest node all of whose children are leaves (two of them at least)"""
    root = nodes[0]
    assert any(not root["words"][k] & 1 for k in root["live"])
    deepest = max((n for n in nodes if n["number"] and len(n["live"]) >= 2 and all(n["words"][k] & 1 for k in n["live"])),
                  key=lambda n: (n["depth"], n["number"]))
    return root, deepest


def _union(box, live):
    return box[:, 0, live].min(axis=1), box[:, 1, live].max(axis=1)


def plane_mutants(data):
    """[dict(what, number, parent, kind of child, inward, outward, union_moves)]: every plane of every non-empty slot of the root and
    of a deepest inner node, one float32 step each way; union_moves: the step changes the union of the node's child boxes"""
    out = []
    for node in _root_and_deepest(_nodes(data)):
        off, live = node["off"], node["live"]
        for k in live:
            for axis in range(3):
                at = [off + 4 * (8 * axis + 4 * side + k) for side in (0, 1)]
                lo, hi = node["box"][axis, 0, k], node["box"][axis, 1, k]
                if lo == hi:
                    continue
                for side in (0, 1):
                    m = dict(what="node %d slot %d axis %d %s" % (node["number"], k, axis, ("min", "max")[side]), number=node["number"],
                             parent=node["parent"], kind="leaf" if node["words"][k] & 1 else "inner")
                    for name, inward in (("inward", True), ("outward", False)):
                        b = np.array(data, copy=True)
                        towards = np.float32(np.inf) if (side == 0) == inward else np.float32(-np.inf)
                        b[at[side]:at[side] + 4].view("<f4")[0] = np.nextafter((lo, hi)[side], towards)
                        m[name] = b
                        before = _union(node["box"], live)
                        after = _union(np.frombuffer(b, "<f4", 24, off).reshape(3, 2, 4), live)
                        m[name + "_union_moves"] = not all((x == y).all() for x, y in zip(before, after))
                    out.append(m)
    kinds = {(m["number"] == 0, m["kind"]) for m in out}
    assert (True, "inner") in kinds and (False, "leaf") in kinds
    return out


def _plane_expectation(m, direction):
    """(box_violations, loose_boxes, first_bad_index) the geometry gives: exact, the base blobs' boxes being exact"""
    moves = m[direction + "_union_moves"] and m["number"] != 0
    if direction == "inward":
        return 1, 1 if moves else 0, m["number"]
    return (1, 1, m["parent"]) if moves else (0, 1, None)


def other_mutants(data):
    """[(what, the reference's field, the validator's field or "refused", bytes)]"""
    nodes = _nodes(data)
    root, deepest = _root_and_deepest(nodes)
    out = []

    def edited(what, ref_field, dev_field, edit):
        b = np.array(data, copy=True)
        edit(b)
        out.append((what, ref_field, dev_field, b))

    def plane(node, axis, side, k):
        return node["off"] + 4 * (8 * axis + 4 * side + k)

    def set_planes(b, node, k, values):
        for axis, (lo, hi) in enumerate(values):
            b[plane(node, axis, 0, k):plane(node, axis, 0, k) + 4].view("<f4")[0] = lo
            b[plane(node, axis, 1, k):plane(node, axis, 1, k) + 4].view("<f4")[0] = hi

    k_inner = next(k for k in root["live"] if not root["words"][k] & 1)
    edited("NaN plane", "bad_empty_slots", "refused",
           lambda b: b[plane(root, 1, 0, k_inner):plane(root, 1, 0, k_inner) + 4].view("<f4").__setitem__(0, np.nan))
    holey = next(n for n in nodes if len(n["live"]) < 4)
    k_empty = next(k for k in range(4) if k not in holey["live"])
    assert (holey["box"][:, 0, k_empty] == 1).all() and (holey["box"][:, 1, k_empty] == -1).all()
    edited("empty slot +2 / -2", "bad_empty_slots", "refused", lambda b: set_planes(b, holey, k_empty, [(2, -2)] * 3))
    edited("empty slot 0 / 0 on z", "bad_empty_slots", "refused", lambda b: set_planes(b, holey, k_empty, [(1, -1), (1, -1), (0, 0)]))
    # leaves: (offset, count, triangle indices); one mesh, so a record's index is its primitive id
    leaves = []
    for n in nodes:
        for k in n["live"]:
            if n["words"][k] & 1:
                off = n["words"][k] ^ 1
                cnt = int(np.frombuffer(data, "<u8", 1, off)[0]) & 63
                leaves.append((off, cnt, np.frombuffer(data, "<u4", 2 * cnt, off + 8)[1::2]))
    largest = max(int(ids.max()) for _, _, ids in leaves)
    # a leaf of two or more whose count is not 1 mod 4 (the mesh table stays where it is) and that does not hold the largest id (the
    # number of primitives stays); a device build of a sparse soup may hold leaves of one triangle only: then the neighbour is the
    # next leaf, the count of 0 is tried on a leaf of one, and "lowered by one" is that same edit and is not made twice
    pick = next((l for l in leaves if l[1] >= 2 and l[1] % 4 != 1 and largest not in l[2]), None)
    if pick is not None:
        off, cnt, ids = pick
        edited("neighbour's primitive id", "id_twice", "primitive_id_errors",
               lambda b: b[off + 8:off + 8 + 8 * cnt].view("<u4").__setitem__(2 * cnt - 1, ids[cnt - 2]))
        edited("leaf count - 1", "id_never", "primitive_id_errors", lambda b: b[off:off + 8].view("<u8").__setitem__(0, b[off:off + 8].view("<u8")[0] - 1))
    else:
        singles = [l for l in leaves if largest not in l[2]]
        (off, cnt, ids), other = singles[0], singles[1]
        edited("neighbour's primitive id", "id_twice", "primitive_id_errors",
               lambda b: b[off + 8:off + 8 + 8 * cnt].view("<u4").__setitem__(2 * cnt - 1, other[2][0]))
    edited("leaf count 0", "leaf_count_errors", "primitive_id_errors", lambda b: b[off:off + 8].view("<u8").__setitem__(0, b[off:off + 8].view("<u8")[0] & ~np.uint64(63)))
    off2, cnt2, _ = next((l for l in leaves if l[1] % 4 != 0), leaves[0])
    if cnt2 % 4:
        assert not data[off2 + 8 + 8 * cnt2:off2 + 16 + 8 * cnt2].any()                                # the padding record is all zero: vertex 0 thrice, id 0
        fields = ("id_twice", "primitive_id_errors")
    else:
        # every leaf is full to a multiple of four: the next record is the head of the leaf's mesh table, and the table is then read
        # four records further on -- whatever lies there. A defect either way; which one depends on the bytes.
        fields = ("not_clean", "refused|primitive_id_errors")
    edited("leaf count + 1", fields[0], fields[1], lambda b: b[off2:off2 + 8].view("<u8").__setitem__(0, b[off2:off2 + 8].view("<u8")[0] + 1))
    k0, k1 = deepest["live"][:2]
    word = lambda node, k: slice(node["off"] + 96 + 8 * k, node["off"] + 104 + 8 * k)
    edited("another child's leaf", "shared", "refused", lambda b: b[word(deepest, k1)].view("<u8").__setitem__(0, deepest["words"][k0]))
    edited("an ancestor", "shared", "refused", lambda b: b[word(deepest, k1)].view("<u8").__setitem__(0, 128))
    edited("past the last node", "out_of_range", "refused", lambda b: b[word(deepest, k1)].view("<u8").__setitem__(0, (len(data) + 127) & ~127))
    return out


def _reference_field(r, field):
    if field == "id_twice":
        return int((r["prim_counts"] > 1).sum())
    if field == "not_clean":
        return 0 if r["clean"] else 1
    if field == "id_never":
        return int((r["prim_counts"] == 0).sum())
    return r[field]


@pytest.fixture(scope="module")
def soup300_blob(oracle):
    return oracle.build_scene([dict(positions=synth.triangle_soup(300, 0.2, seed=4))])


def test_reference_flags_every_mutant_and_neither_base_blob(oracle, soup300_blob):
    for blob in (soup300_blob, oracle.build_scene([dict(positions=synth.triangle_soup(1025, 0.05, seed=70))])):
        data = np.array(blob.data, copy=True)
        base = blob_reference.check(data)
        assert base["clean"] and base["loose_boxes"] == 0 and base["triangles"] == len(base["prim_counts"]), base
        mutants = plane_mutants(data)
        assert len(mutants) >= 24
        for m in mutants:
            for direction in ("inward", "outward"):
                r = blob_reference.check(m[direction])
                assert (r["box_violations"], r["loose_boxes"], r["first_bad_index"]) == _plane_expectation(m, direction), (m["what"], direction, r)
                assert r["clean"] == (r["box_violations"] == 0)
        others = other_mutants(data)
        assert len(others) == 10
        assert [w for w, _, _, _ in others][3:7] == ["neighbour's primitive id", "leaf count - 1", "leaf count 0", "leaf count + 1"]
        for what, ref_field, _, b in others:
            r = blob_reference.check(b)
            assert not r["clean"] and _reference_field(r, ref_field) >= 1, (what, ref_field, r)


def _both_say_valid(ds):
    ok, c = ds.validate()
    assert ok, c
    r = blob_reference.check(ds.export_blob())
    assert r["clean"] and r["box_violations"] == 0 and r["loose_boxes"] == 0 and (r["prim_counts"] == 1).all(), r
    assert (r["nodes"], r["leaves"], r["triangles"]) == (c["nodes_checked"], c["leaves_checked"], c["triangles_checked"]), (r, c)
    assert c["box_violations"] == 0 and c["loose_boxes"] == 0
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("n,collapse", [(2, False), (3, False), (1023, False), (1024, False), (1025, False), (10_000, False), (1025, True), (10_000, True)])
def test_valid_builds_are_valid_to_both(api, n, collapse, monkeypatch):
    if collapse:
        monkeypatch.setenv("RTK_AMD_TILE_COLLAPSE_MIN", "0")
    ds = api.DeviceScene.build([dict(positions=synth.triangle_soup(n, 0.05 if n > 100 else 0.5, seed=70))])
    assert _both_say_valid(ds)["triangles_checked"] == n


@pytest.mark.gpu
def test_valid_passes_are_valid_to_both(api, oracle):
    v = synth.triangle_soup(10_000, 0.05, seed=70)
    ds = api.DeviceScene.build([dict(positions=v)])
    ds.refit([dict(positions=deform(v, 2))])
    _both_say_valid(ds)
    up = api.DeviceScene.upload(oracle.build_scene([dict(positions=v)]))
    assert up.split_leaves()["leaves_split"] > 0
    _both_say_valid(up)
    up.rebuild()
    _both_say_valid(up)


def _traced_without_error(api, ds, rays):
    ds.trace(rays, full=False)
    assert api.lib().rtk_dev_trace_status(ds.handle, None) == 0, api.last_error()


@pytest.mark.gpu
@pytest.mark.parametrize("base", ["oracle 300", "device 1025"])
def test_mutants(api, oracle, soup300_blob, base):
    if base == "oracle 300":
        data = np.array(soup300_blob.data, copy=True)
    else:
        data = np.array(api.DeviceScene.build([dict(positions=synth.triangle_soup(1025, 0.05, seed=70))]).export_blob(), copy=True)
    assert blob_reference.check(data)["clean"]
    ok, c0 = api.DeviceScene.upload(_as_blob(oracle, data)).validate()
    assert ok and c0["box_violations"] == 0 and c0["loose_boxes"] == 0, c0
    rays = synth.rays_config1(4096)
    mutants = plane_mutants(data)
    assert len(mutants) >= 24
    for m in mutants:
        for direction in ("inward", "outward"):
            want = blob_reference.check(m[direction])
            ds = api.DeviceScene.upload(_as_blob(oracle, m[direction]))
            ok, c = ds.validate()
            assert direction == "outward" or want["box_violations"] >= 1
            assert ok == (want["box_violations"] == 0), (m["what"], direction, c, want)
            assert c["box_violations"] == want["box_violations"] and c["loose_boxes"] == want["loose_boxes"], (m["what"], direction, c, want)
            if not ok:
                assert c["first_bad_index"] == want["first_bad_index"], (m["what"], direction, c, want)
                _traced_without_error(api, ds, rays)
    outcomes = []
    for what, ref_field, dev_field, b in other_mutants(data):
        assert not blob_reference.check(b)["clean"], what
        try:
            ds = api.DeviceScene.upload(_as_blob(oracle, b))
        except RtkError as e:
            assert "refused" in dev_field.split("|") and "scene blob" in str(e), (what, dev_field, str(e))
            outcomes.append((what, "refused"))
            continue
        ok, c = ds.validate()
        named = [f for f in dev_field.split("|") if f != "refused"]
        assert named and not ok and c[named[0]] >= 1, (what, dev_field, ok, c)
        outcomes.append((what, named[0]))
        _traced_without_error(api, ds, rays)
    # (the device build's leaves of this sparse soup hold one triangle each: "count - 1" is "count 0" there and is made once)
    assert [o for o in outcomes if o[0] == "leaf count - 1"] == ([("leaf count - 1", "primitive_id_errors")] if base == "oracle 300" else [])
    assert len(outcomes) == (10 if base == "oracle 300" else 9), outcomes


# ---------------------------------------------------------------------------------------------- the producers of finished nodes

def _moved_rays(rays, scale, centre):
    r = rays.copy()
    r["origin"] = (r["origin"] - np.float32(0.5)) * np.float32(scale) + np.float32(centre)
    r["direction"] = r["direction"] * np.float32(scale)
    return r


def _figures(api, ds, frame, incoherent):
    """The packet leg is required in all three scenes: the assembly packet kernel takes bounds below 2^19 (rtk_trace_plan.h), the
    moved scene's is 1e4 + 50. Any refusal or error of the call fails the test."""
    out = {}
    rec, pk = ds.trace_packet_counted(frame, api.make_opts(image=(256, 256)))
    out["packet"] = (rec.tobytes(), pk["node_steps"], pk["triangles_fetched"], pk["triangle_group_tests"])
    rec, c = ds.trace_counted(incoherent)
    out["lane"] = (rec.tobytes(), c["nodes"], c["leaves"], c["triangles"])
    out["hash"] = ds.validate()[1]["content_hash"]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n,moved", [(1025, False), (10_000, False), (10_000, True)])
def test_tile_collapse_and_quantize_finish_nodes_alike(api, n, moved, monkeypatch):
    monkeypatch.setenv("RTK_AMD_TILE_COLLAPSE_MIN", "0")
    v = synth.triangle_soup(n, 0.05, seed=70)
    frame, incoherent = synth.rays_pinhole(256, 256), synth.rays_incoherent(65536)
    if moved:                                                        # centre 1e4, extent 100; the camera and the rays go with it
        v = ((v - np.float32(0.5)) * np.float32(100) + np.float32(1e4)).astype(np.float32)
        frame, incoherent = _moved_rays(frame, 100, 1e4), _moved_rays(incoherent, 100, 1e4)
    ds = api.DeviceScene.build([dict(positions=v)])
    ok, c = ds.validate()
    assert ok and c["compressed_node_errors"] == 0, c
    before = _figures(api, ds, frame, incoherent)
    assert before["lane"][1] > 65536 and before["packet"][1] > 0 and before["packet"][2] > 0           # the rays do walk the tree
    assert (np.frombuffer(before["packet"][0], np.uint32)[3::4] != 0xFFFFFFFF).sum() > 1000              # ... and the frame sees the scene
    ds.refit([dict(positions=v)])
    after = _figures(api, ds, frame, incoherent)
    assert before == after, {k: (before[k][1:], after[k][1:]) if k != "hash" else (before[k], after[k]) for k in before if before[k] != after[k]}
