"""Triangles near a triangle without a GPU: the rule of rtk_amd/csrc/rtk_near_rule.h, run by tests/near_rule_driver.cpp under the
address and undefined-behaviour sanitizers, against numpy (tests/near_ref.py): the bounded sorted insertion alone, with guard
words around the segment and both point arrays; rtk_near_skip's truth table; a host walk of a small 4-wide tree in four child
orders and three rooms against brute force, bit for bit; the bound against the distance of everything below a box; and the
parts of the interface that need no device -- header text, symbols, argtypes, the refusals decided before any HIP call. No
tolerance anywhere: every comparison is an equality."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from rtk_amd.types import RTK_INF
from tests.near_ref import brute_force_near
from tests.pair_ref import box_bound_np, brute_force_pairs, pair_np
from tests.test_pair_cpu import walk_queries, walk_scene
from tests.test_within_cpu import hexes, run_driver, small_tree
from tests.touch_ref import box_np, live_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_BAD_ARG = -2
GUARD = 4                                     # entries on either side of the driver's segment
FILL = 0x7e7e7e7e
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """The driver built against the rule headers alone (no HIP include path, -Wall -Werror, no FMA contraction as in the
    library) with both sanitizers. -O2 and -mfma: a compiler that were allowed to contract would do it here."""
    exe = str(tmp_path_factory.mktemp("near_rule") / "near_rule_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-mfma", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "rtk_amd", "csrc"), os.path.join(ROOT, "tests", "near_rule_driver.cpp"), "-o", exe])
    return exe


def split_segment(words, room):
    """the driver's dump -> (record words [room, 4], words of the points on the query [room, 3], on the scene [room, 3]); the
    guards must be untouched"""
    total = GUARD + room + GUARD
    w = np.array([int(x, 16) for x in words], np.uint32)
    assert len(w) == total * 10
    rec, pa, pb = w[:total * 4].reshape(total, 4), w[total * 4:total * 7].reshape(total, 3), w[total * 7:].reshape(total, 3)
    for x, name in ((rec, "record"), (pa, "query point"), (pb, "scene point")):
        assert (x[:GUARD] == FILL).all() and (x[GUARD + room:] == FILL).all(), "a %s guard was written" % name
    return rec[GUARD:GUARD + room], pa[GUARD:GUARD + room], pb[GUARD:GUARD + room]


def sorted_prefix(cand, room):
    """cand uint32 [n, 10] (dist2 u v prim qa[3] qb[3]) -> its rows without a NaN dist2, ascending in (dist2, prim) by a Python
    list sort, order of arrival among equal pairs, the first `room` of them"""
    d = cand[:, 0].copy().view(np.float32)
    rows = [i for i in range(len(cand)) if not np.isnan(d[i])]
    rows.sort(key=lambda i: (float(d[i]), int(cand[i, 3])))           # (stable: equal pairs stay in arrival order)
    return cand[rows[:room]]


def candidate_streams():
    rng = np.random.RandomState(20250312)
    streams = []
    for n, kind in ((0, "plain"), (1, "plain"), (5, "plain"), (40, "plain"), (200, "plain"), (200, "ties"), (300, "ties+nan"), (64, "descending"),
                    (64, "ascending"), (90, "all equal"), (30, "nan only"), (120, "pierced")):
        c = np.zeros((n, 10), np.uint32)
        d = rng.uniform(0, 10, n).astype(np.float32)
        if kind.startswith("ties"):
            d = rng.choice(np.array([0.0, 0.25, 1.0, 1.0000001, 3.5, np.inf], np.float32), n)
        if kind == "all equal":
            d = np.full(n, 2.0, np.float32)
        if kind == "pierced":
            d[rng.permutation(n)[:n // 2]] = 0.0                      # (many entries at dist2 = 0: they come first, by id)
        if kind == "descending":
            d = np.sort(d)[::-1].copy()
        if kind == "ascending":
            d = np.sort(d)
        if kind == "ties+nan":
            d[rng.permutation(n)[:n // 5]] = np.nan
        if kind == "nan only":
            d[:] = np.nan
        c[:, 0] = d.view(np.uint32)
        c[:, 1:3] = rng.randint(0, 2 ** 32, (n, 2), dtype=np.uint64)    # (u, v and the points are carried, any bits)
        c[:, 3] = rng.permutation(n).astype(np.uint32) if kind != "plain" else rng.randint(0, 2 ** 32 - 1, n, dtype=np.uint64)
        c[:, 4:] = rng.randint(0, 2 ** 32, (n, 6), dtype=np.uint64)
        # (a float that is copied as a float keeps its bits unless it is a signalling NaN: carried words are kept away from NaNs)
        carried = [1, 2, 4, 5, 6, 7, 8, 9]
        nan = (c[:, carried] & 0x7f800000) == 0x7f800000
        c[:, carried] = np.where(nan, c[:, carried] & 0xff7fffff, c[:, carried])
        streams.append((kind, c))
    return streams


@pytest.mark.parametrize("room", [0, 1, 2, 3, 7, 64])
def test_insertion_alone(driver, tmp_path, room):
    """Every stream into a segment of `room` entries: the first `room` of the sorted stream with both points, the rest of the
    segment and the guards untouched. The driver itself checks that the variants with one point array or none keep the same
    records and that `worst` is the last entry after every insertion into a full segment."""
    streams = candidate_streams()
    text = "".join("i %d %d %s\n" % (room, len(c), hexes(c)) for _, c in streams)
    out = run_driver(driver, text, len(streams), tmp_path, "insert_%d" % room)
    full = not_full = 0
    for (kind, c), line in zip(streams, out):
        want = sorted_prefix(c, room)
        kept = int(line[0])
        rec, pa, pb = split_segment(line[1:], room)
        assert kept == len(want), kind
        assert rec[:kept].tobytes() == want[:, :4].tobytes() and pa[:kept].tobytes() == want[:, 4:7].tobytes() and pb[:kept].tobytes() == want[:, 7:].tobytes(), kind
        assert (rec[kept:] == FILL).all() and (pa[kept:] == FILL).all() and (pb[kept:] == FILL).all(), kind
        full += kept == room
        not_full += kept < room
        if kind in ("ties", "pierced") and room >= 2:
            d, prim = rec[:kept, 0].copy().view(np.float32), rec[:kept, 3]
            assert ((np.diff(d) > 0) | ((np.diff(d) == 0) & (np.diff(prim.astype(np.int64)) > 0))).all()
            assert (np.diff(d) == 0).any()                            # (equal dist2 values did meet)
            if kind == "pierced":
                assert d[0] == 0 and d[1] == 0
    assert full >= 6 or room == 64
    assert not_full >= 2 or room == 0


def test_skip_truth_table(driver, tmp_path):
    """skip iff bound >= max_dist2, or full and bound > worst2 (strictly); a NaN bound is never skipped"""
    values = np.array([0.0, 1.0, np.nextafter(np.float32(1), np.float32(2)), 2.0, np.inf, np.nan], np.float32)
    cases = [(b, m, f, w) for b in values for m in values for f in (0, 1) for w in values]
    text = "".join("s %s %x %s\n" % (hexes(np.array([b, m], np.float32).view(np.uint32)), f, hexes(np.array([w], np.float32).view(np.uint32))) for b, m, f, w in cases)
    out = run_driver(driver, text, len(cases), tmp_path, "skip")
    seen = set()
    for (b, m, f, w), line in zip(cases, out):
        with np.errstate(invalid="ignore"):
            want = bool(b >= m) or (bool(f) and bool(b > w))
        assert int(line[0]) == int(want), (b, m, f, w)
        if np.isnan(b):
            assert line[0] == "0"
        seen.add((int(want), bool(f), bool(b == w), bool(b == m)))
    # an equal bound: skipped against the limit, NOT skipped against the worst entry
    assert (1, False, False, True) in seen and (0, True, True, False) in seen and (1, True, False, False) in seen


# ---------------------------------------------------------------------------------------------- the walk

def below(nodes, recs):
    """every child box of the driver's tree -> (lo [3], hi [3], ids of the records below it)"""
    out = []

    def leaf_ids(slot):
        ids = []
        while True:
            ids.append(int(recs[slot, 9]))
            if recs[slot, 10]:
                return ids
            slot += 1

    def under(ref):
        if ref & 0x80000000:
            return leaf_ids(int(ref & 0x7fffffff))
        ids = []
        box = nodes[ref, :24].copy().view(np.float32).reshape(6, 4)
        for k in range(4):
            child = int(nodes[ref, 24 + k])
            if child == NONE:
                continue
            got = under(child)
            out.append((box[0::2, k].copy(), box[1::2, k].copy(), got))
            ids += got
        return ids
    assert sorted(under(0)) == sorted(int(x) for x in recs[:, 9])
    return out


@pytest.fixture(scope="module")
def walk():
    class W:
        pass
    w = W()
    rng = np.random.RandomState(5)
    w.tris, w.n_soup, w.n_mesh, w.n_plates = walk_scene(rng)
    w.nodes, w.recs = small_tree(rng, w.tris, 5)
    w.q, w.max2, w.first, w.flags = walk_queries(rng, w.tris, w.n_soup, w.n_mesh, w.n_plates)
    w.prims = np.arange(len(w.tris))
    return w


def by_flag(w, room):
    """brute force per query with that query's own flag"""
    ref = [brute_force_near(w.tris, w.prims, w.q, w.max2, w.first, fl, room) for fl in (0, 1)]
    counts = np.where(w.flags == 1, ref[1].counts, ref[0].counts)
    kept = [ref[int(w.flags[i])].kept[i] for i in range(len(w.q))]
    return counts, kept


def test_host_walk_equals_brute_force_in_every_order_and_room(driver, tmp_path, walk):
    """The scene of tests/test_pair_cpu.py's walk (a soup, a closed mesh twice in place, plates pierced all at once) under a random
    4-wide tree: count and kept prefix equal brute force bit for bit in four child orders and three rooms"""
    w = walk
    T, n = len(w.tris), len(w.q)
    assert len(w.nodes) > 8
    text = "n %d %s\nt %d %s\n" % (len(w.nodes), hexes(w.nodes), len(w.recs), hexes(w.recs))
    closest = [brute_force_pairs(w.tris, w.prims, w.q, w.max2, w.first, fl) for fl in (0, 1)]
    closest = tuple(np.where((w.flags == 1)[:, None], closest[1][k], closest[0][k]) for k in range(3))
    for room_all in (1, 4, T):
        room = np.full(n, room_all, np.uint32)
        counts, kept = by_flag(w, room)
        assert (counts == 0).any() and (counts == 1).any() and (counts > 16).any()
        # the first list entry is closest triangles' answer, and an empty list is its miss
        hit = closest[0][:, 3] != NONE
        assert ((counts > 0) == hit).all()
        for i in np.nonzero(hit)[0]:
            assert all(kept[i][k][0].tobytes() == closest[k][i].tobytes() for k in range(3)), i
        qwords = np.concatenate([w.q.reshape(-1, 9).view(np.uint32), w.max2.view(np.uint32)[:, None], w.first[:, None], w.flags[:, None], room[:, None]], 1)
        evaluated = []
        for order in (0, 1, 2, 3):
            out = run_driver(driver, text + "".join("q %d %s\n" % (order, hexes(x)) for x in qwords), n, tmp_path, "walk_%d_%d" % (room_all, order))
            for i, line in enumerate(out):
                rec, pa, pb = split_segment(line[3:], room_all)
                k = len(kept[i][0])
                assert int(line[0]) == counts[i] and int(line[1]) == k == min(int(counts[i]), room_all), (room_all, order, i)
                for got, want in zip((rec, pa, pb), kept[i]):
                    assert got[:k].tobytes() == want.tobytes(), (room_all, order, i)
                    assert (got[k:] == FILL).all(), (room_all, order, i)
            evaluated.append(sum(int(line[2]) for line in out))
        print("room %d: records evaluated in slot order %d, reversed %d, drawn %d, nearest first %d of %d" % ((room_all,) + tuple(evaluated) + (n * T,)))
        if room_all == 1:
            assert evaluated[3] < min(evaluated[:3]) and evaluated[3] < 0.25 * n * T            # (the worst entry does cull)
    # the through-everything queries pierce all eight plates: eight entries at dist2 = 0 come first, by id
    first_plate = w.n_soup + w.n_mesh
    for i in (n - 4, n - 3):
        rec = kept[i][0]                                             # (room T: the whole list)
        assert (rec[:w.n_plates, 0] == 0).all() and (rec[:w.n_plates, 3] == first_plate + np.arange(w.n_plates)).all()
    # the mesh stands twice in place: equal dist2 under two ids, the lower id first
    both = [r for r, _, _ in kept if len(r) > 1 and (np.diff(r[:, 0].copy().view(np.float32)) == 0).any()]
    assert both and all((np.diff(r[:, 3].astype(np.int64))[np.diff(r[:, 0].copy().view(np.float32)) == 0] > 0).all() for r in both)
    # a scene without triangles: no candidates
    out = run_driver(driver, "n 0\nt 0\nq 0 %s\n" % hexes(qwords[0]), 1, tmp_path, "empty")
    assert out[0][:2] == ["0", "0"]


def test_the_bound_never_exceeds_the_distance_of_anything_below(walk):
    """For every child box of the tree and for every record's own box: bound <= dist2 of every record below it, for every live
    query -- pierced pairs (dist2 = 0, bound 0) included -- without a margin"""
    w = walk
    live = live_np(w.q)
    q = w.q[live]
    d = pair_np(q[:, None], w.tris[None]).dist2                       # [Q, T]
    assert not np.isnan(d).any() and (d == 0).sum() > 20
    alo, ahi = box_np(q)
    boxes = below(w.nodes, w.recs)
    assert len(boxes) > 20
    positive = 0
    for lo, hi, ids in boxes:
        bound = box_bound_np(lo[None], hi[None], alo, ahi)
        assert (bound[:, None] <= d[:, ids]).all()
        positive += int((bound > 0).sum())
    blo, bhi = box_np(w.tris)
    own = box_bound_np(blo[None], bhi[None], alo[:, None], ahi[:, None])
    assert (own <= d).all() and (own == d).any() and positive > 100 and (own[d == 0] == 0).all()


# ---------------------------------------------------------------------------------------------- the interface

def test_rule_header_includes_no_hip_and_says_what_it_must():
    text = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_near_rule.h")).read()
    assert [l.split()[1] for l in text.splitlines() if l.startswith("#include")] == ['"rtk_pair_rule.h"']
    assert "hip_runtime" not in text and "__global__" not in text and "fmaf" not in text
    code = text.split("#pragma once")[1]
    for used in ("rtk_near_candidate(", "rtk_near_skip(", "rtk_near_insert(", "rtk_closest_better("):
        assert used in code, used
    flat = " ".join(text.replace("\n//", "\n").split())
    for word in ("dist2 < max_dist2", "LOWEST PRIMITIVE ID", "b >= max_dist2", "b > worst.dist2", "bound <= dist2", "WITHOUT A MARGIN", "STRICT", "EXACT",
                 "only ever gets better", "A NaN bound", "never a candidate", "rtk_pair_box_bound", "rtk_pair_evaluate", "rtk_touch_filter_passes",
                 "rtk_touch_live", "ITS OWN box", "TWO optional point arrays", "rule 6 of rtk_pair_rule.h", "rtk_dev_closest_triangles"):
        assert word in flat, word
    for name in ("rtk_within_rule.h", "rtk_pair_rule.h", "rtk_touch_rule.h", "rtk_closest_rule.h"):
        assert "rtk_near" not in open(os.path.join(ROOT, "rtk_amd", "csrc", name)).read()        # (used as they are, not changed)
    header = open(os.path.join(ROOT, "include", "rtk_amd.h")).read()
    section = header[header.index("/* ---- Triangles near a triangle"):header.index("/* ---- Every hit along a ray")]
    section = " ".join(section.replace("\n *", "\n").split())
    for word in ("rtk_near_rule.h", "rtk_pair_rule.h", "ARE NOT WRITTEN", "A SLOT THAT IS NOT LISTED IS NOT WRITTEN", "d_offsets[i] = i * k", "DETERMINISTIC",
                 "NOTHING ELSE IS PROMISED", "rtk_dev_trace_status", "rtk_mgpu_scene(m, i)", "LOWEST PRIMITIVE ID FIRST AMONG EQUAL dist2", "PIERCING",
                 "RTK_TOUCH_SKIP_SHARED_VERTEX", "unknown bit", "dist2 < max_dist2", "b >= max_dist2", "b > worst.dist2", "without a margin",
                 "NULL means RTK_INF", "word for word what rtk_dev_closest_triangles writes", "NOT CHECKED", "d_written[i] = 0"):
        assert word in section, word
    mk = open(os.path.join(ROOT, "rtk_amd", "csrc", "Makefile")).read()
    assert "rtk_near_rule.h" in mk and "rtk_near.hip" in mk and "-fhip-fp32-correctly-rounded-divide-sqrt" in mk and "-ffp-contract=off" in mk
    kernel = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_near.hip")).read()
    for used in ("rtk_pair_hoist_query(", "rtk_pair_evaluate(", "rtk_pair_box_bound(", "rtk_near_skip(", "rtk_near_candidate(", "rtk_near_insert(", "rtk_touch_live(",
                 "rtk_touch_filter_passes(", "LaunchScratch", "sc->select", "kernel-resource-usage", "NR_RESOURCES", "scratch 0"):
        assert used in kernel, used
    for doc, word in (("README.md", "rtk_dev_triangles_near_count"), ("INTEGRATION.md", "## Triangles near a triangle"), ("DESIGN.md", "Triangles near a triangle"),
                      (os.path.join("docs", "HISTORY.md"), "rtk_dev_triangles_near"), (os.path.join("scripts", "README.md"), "near_timing.py")):
        assert word in open(os.path.join(ROOT, doc)).read(), doc
    assert os.path.exists(os.path.join(ROOT, "scripts", "near_timing.py"))


def test_header_symbols_and_argtypes(api):
    text = open(os.path.join(ROOT, "include", "rtk_amd.h")).read()
    for word in ("int rtk_dev_triangles_near_count(const rtk_dev_scene *ds, const rtk_tri_query *d_tris, size_t num_queries,",
                 "int rtk_dev_triangles_near_all(const rtk_dev_scene *ds, const rtk_tri_query *d_tris, size_t num_queries,",
                 "int rtk_dev_triangles_near_counted(const rtk_dev_scene *ds, const rtk_tri_query *d_tris, size_t num_queries,",
                 "uint32_t rtk_amd_near_stack_entries(void);"):
        assert word in text, word
    assert text.index("/* ---- Closest triangles") < text.index("/* ---- Triangles near a triangle") < text.index("/* ---- Every hit along a ray")
    L = api.lib()
    for name in ("rtk_dev_triangles_near_count", "rtk_dev_triangles_near_all", "rtk_dev_triangles_near_counted", "rtk_amd_near_stack_entries"):
        assert name in api.RTK_AMD_H_SYMBOLS and hasattr(L, name), name
    P, F = C.POINTER(api.RayList), C.POINTER(api.TouchFilter)
    v = C.c_void_p
    assert L.rtk_dev_triangles_near_count.argtypes == [v, v, C.c_size_t, P, F, v, v, v]
    assert L.rtk_dev_triangles_near_all.argtypes == [v, v, C.c_size_t, P, F, v, v, v, v, v, v, v]
    assert L.rtk_dev_triangles_near_counted.argtypes == [v, v, C.c_size_t, F, v, v, v, v, v, v, C.POINTER(api.TraceCounters)]
    assert L.rtk_dev_triangles_near_count.restype == C.c_int and L.rtk_dev_triangles_near_all.restype == C.c_int
    assert L.rtk_dev_triangles_near_counted.restype == C.c_int
    assert L.rtk_amd_near_stack_entries.restype == C.c_uint32 and 1 <= L.rtk_amd_near_stack_entries() <= 64
    for name in ("count_near_device", "near_all_device", "near_counted", "triangles_near", "nearest_triangles_to", "contacts", "self_contacts"):
        assert callable(getattr(api.DeviceScene, name)), name


def test_refusals_need_no_device(api):
    L = api.lib()
    buf = C.create_string_buffer(64)
    dummy = C.cast(buf, C.c_void_p)                                          # (what is refused is refused before the scene is looked at)
    count = C.cast(C.create_string_buffer(8), C.c_void_p)

    def ray_list(**kw):
        l = api.RayList()
        l.struct_size, l.flags, l.d_ids, l.d_count = C.sizeof(api.RayList), 0, None, count.value
        for k, v in kw.items():
            setattr(l, k, v)
        return l

    def touch_filter(**kw):
        f = api.TouchFilter()
        f.struct_size, f.flags, f.d_first_prim = C.sizeof(api.TouchFilter), 0, None
        for k, v in kw.items():
            setattr(f, k, v)
        return f
    bad_lists = (ray_list(struct_size=8), ray_list(flags=1), ray_list(d_count=None))
    bad_filters = (touch_filter(struct_size=8), touch_filter(struct_size=0), touch_filter(flags=2), touch_filter(flags=0x80000001))
    good = C.byref(touch_filter(flags=1))
    # count: scene, triangles, n, list, filter, max_dist2, counts, stream
    for args in [(None, dummy, 4, None, None, None, dummy, None), (dummy, None, 4, None, None, None, dummy, None), (dummy, dummy, 4, None, good, dummy, None, None),
                 (dummy, dummy, 1 << 32, None, None, None, dummy, None), (dummy, dummy, 1 << 32, C.byref(ray_list()), good, None, dummy, None)] + \
                [(dummy, dummy, 4, C.byref(l), None, None, dummy, None) for l in bad_lists] + \
                [(dummy, dummy, 4, None, C.byref(f), None, dummy, None) for f in bad_filters]:
        assert L.rtk_dev_triangles_near_count(*args) == ERR_BAD_ARG, args
        assert "rtk_dev_triangles_near_count:" in api.last_error()
    # fill: scene, triangles, n, list, filter, max_dist2, offsets, records, points on the query, points on the scene, written, stream
    for args in [(None, dummy, 4, None, None, None, dummy, dummy, None, None, None, None), (dummy, None, 4, None, None, None, dummy, dummy, None, None, None, None),
                 (dummy, dummy, 4, None, None, None, None, dummy, None, None, None, None), (dummy, dummy, 4, None, good, dummy, dummy, None, dummy, dummy, dummy, None),
                 (dummy, dummy, 1 << 32, None, None, None, dummy, dummy, None, None, None, None)] + \
                [(dummy, dummy, 4, C.byref(l), None, None, dummy, dummy, None, None, None, None) for l in bad_lists] + \
                [(dummy, dummy, 4, None, C.byref(f), None, dummy, dummy, None, None, None, None) for f in bad_filters]:
        assert L.rtk_dev_triangles_near_all(*args) == ERR_BAD_ARG, args
        assert "rtk_dev_triangles_near_all:" in api.last_error()
    # counted: scene, triangles, n, filter, max_dist2, offsets, records, points, points, counts or written, counters
    ctr = api.TraceCounters()
    for args in [(dummy, dummy, 4, None, None, None, None, None, None, dummy, None), (None, dummy, 4, None, None, None, None, None, None, dummy, C.byref(ctr)),
                 (dummy, None, 4, None, None, None, None, None, None, dummy, C.byref(ctr)), (dummy, dummy, 4, good, None, None, None, None, None, None, C.byref(ctr)),
                 (dummy, dummy, 4, None, None, dummy, None, None, None, None, C.byref(ctr)), (dummy, dummy, 1 << 32, None, None, None, None, None, None, dummy, C.byref(ctr))] + \
                [(dummy, dummy, 4, C.byref(f), None, None, None, None, None, dummy, C.byref(ctr)) for f in bad_filters]:
        assert L.rtk_dev_triangles_near_counted(*args) == ERR_BAD_ARG, args
        assert "rtk_dev_triangles_near_counted:" in api.last_error()
    # no queries: nothing to do, nothing launched
    assert L.rtk_dev_triangles_near_count(dummy, None, 0, None, None, None, None, None) == 0
    assert L.rtk_dev_triangles_near_count(dummy, dummy, 0, C.byref(ray_list()), good, dummy, dummy, None) == 0
    assert L.rtk_dev_triangles_near_all(dummy, None, 0, None, None, None, None, None, None, None, None, None) == 0
    assert L.rtk_dev_triangles_near_all(dummy, dummy, 0, C.byref(ray_list()), good, dummy, dummy, dummy, dummy, dummy, dummy, None) == 0
    ctr.rays = 7
    assert L.rtk_dev_triangles_near_counted(dummy, None, 0, None, None, None, None, None, None, None, C.byref(ctr)) == 0 and ctr.rays == 0
