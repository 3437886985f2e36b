"""Triangles within a distance without a GPU: the rule of rtk_amd/csrc/rtk_within_rule.h, run by tests/within_rule_driver.cpp
under the address and undefined-behaviour sanitizers, against numpy (tests/within_ref.py): the bounded sorted insertion alone,
with guard words around the segment; a host walk of a small 4-wide tree in three child orders against brute force, bit for
bit; and the parts of the interface that need no device -- header text, symbols, argtypes, the refusals decided before any HIP
call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from rtk_amd.types import RTK_INF
from tests.closest_ref import tri_box
from tests.within_ref import brute_force_within

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_BAD_ARG = -2
GUARD = 4                                     # entries on either side of the driver's segment
FILL = 0x7e7e7e7e
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """The driver built against the two rule headers alone (no HIP include path, -Wall -Werror, no FMA contraction as in the
    library) with both sanitizers. -O2 and -mfma: a compiler that were allowed to contract would do it here."""
    exe = str(tmp_path_factory.mktemp("within_rule") / "within_rule_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-mfma", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "rtk_amd", "csrc"), os.path.join(ROOT, "tests", "within_rule_driver.cpp"), "-o", exe])
    return exe


def run_driver(exe, text, outputs, tmp_path, name):
    """-> one list of integers per output line (the leading counts decimal, the rest hexadecimal words)"""
    path = str(tmp_path / (name + ".txt"))
    with open(path, "w") as f:
        f.write(text)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    assert lines[outputs] == "ok"
    return [line.split() for line in lines[:outputs]]


def hexes(words):
    return " ".join("%x" % w for w in np.asarray(words, np.uint32).reshape(-1).tolist())


def split_segment(words, room):
    """the driver's dump -> (record words [room, 4], point words [room, 3]); the guards must be untouched"""
    total = GUARD + room + GUARD
    w = np.array([int(x, 16) for x in words], np.uint32)
    assert len(w) == total * 7
    rec, pts = w[:total * 4].reshape(total, 4), w[total * 4:].reshape(total, 3)
    assert (rec[:GUARD] == FILL).all() and (rec[GUARD + room:] == FILL).all(), "a record guard was written"
    assert (pts[:GUARD] == FILL).all() and (pts[GUARD + room:] == FILL).all(), "a point guard was written"
    return rec[GUARD:GUARD + room], pts[GUARD:GUARD + room]


def sorted_prefix(cand, room):
    """cand uint32 [n, 7] (dist2 u v prim q0 q1 q2) -> its rows without a NaN dist2, ascending in (dist2, prim), order of
    arrival among equal pairs, the first `room` of them"""
    d = cand[:, 0].copy().view(np.float32)
    rows = [i for i in range(len(cand)) if not np.isnan(d[i])]
    rows.sort(key=lambda i: (float(d[i]), int(cand[i, 3])))           # (stable: equal pairs stay in arrival order)
    return cand[rows[:room]]


def candidate_streams():
    rng = np.random.RandomState(20250211)
    streams = []
    for n, kind in ((0, "plain"), (1, "plain"), (5, "plain"), (40, "plain"), (200, "plain"), (200, "ties"), (300, "ties+nan"), (64, "descending"),
                    (64, "ascending"), (90, "all equal"), (30, "nan only")):
        c = np.zeros((n, 7), np.uint32)
        d = rng.uniform(0, 10, n).astype(np.float32)
        if kind.startswith("ties") or kind == "all equal":
            d = rng.choice(np.array([0.0, 0.25, 1.0, 1.0000001, 3.5, np.inf], np.float32), n) if kind != "all equal" else np.full(n, 2.0, np.float32)
        if kind == "descending":
            d = np.sort(d)[::-1].copy()
        if kind == "ascending":
            d = np.sort(d)
        if kind == "ties+nan":
            d[rng.permutation(n)[:n // 5]] = np.nan
        if kind == "nan only":
            d[:] = np.nan
        c[:, 0] = d.view(np.uint32)
        c[:, 1:3] = rng.randint(0, 2 ** 32, (n, 2), dtype=np.uint64)    # (u, v and q are carried, any bits)
        c[:, 3] = rng.permutation(n).astype(np.uint32) if kind != "plain" else rng.randint(0, 2 ** 32 - 1, n, dtype=np.uint64)
        c[:, 4:] = rng.randint(0, 2 ** 32, (n, 3), dtype=np.uint64)
        # (a float that is copied as a float keeps its bits unless it is a signalling NaN: carried words are kept away from NaNs)
        nan = (c[:, [1, 2, 4, 5, 6]] & 0x7f800000) == 0x7f800000
        c[:, [1, 2, 4, 5, 6]] = np.where(nan, c[:, [1, 2, 4, 5, 6]] & 0xff7fffff, c[:, [1, 2, 4, 5, 6]])
        streams.append((kind, c))
    return streams


def test_rule_header_includes_no_hip_and_says_what_it_must():
    text = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_within_rule.h")).read()
    assert [l.split()[1] for l in text.splitlines() if l.startswith("#include")] == ['"rtk_closest_rule.h"']
    assert "hip_runtime" not in text and "__global__" not in text
    readme = open(os.path.join(ROOT, "README.md")).read()
    header = open(os.path.join(ROOT, "include", "rtk_amd.h")).read()
    section = header[header.index("/* ---- Triangles within a distance"):header.index("/* ---- Every hit along a ray")]
    section = " ".join(section.replace("\n *", "\n").split())         # (the comment's line breaks and stars taken out)
    for name, where in (("rtk_within_rule.h", " ".join(text.replace("\n//", "\n").split())), ("README.md", " ".join(readme.split())), ("rtk_amd.h", section)):
        for word in ("dist2 < max_dist2", "LOWEST PRIMITIVE ID", "b >= max_dist2", "b > worst.dist2"):
            assert word in where, (name, word)
    for word in ("bound <= dist2", "WITHOUT A MARGIN", "STRICT", "NaN", "rtk_closest_better", "rtk_closest_box_bound", "rtk_closest_triangle"):
        assert word in text, word
    for word in ("rtk_within_rule.h", "ARE NOT WRITTEN", "A SLOT THAT IS NOT LISTED IS NOT WRITTEN", "d_offsets[i] = i * k", "DETERMINISTIC", "NOTHING ELSE IS PROMISED",
                 "rtk_dev_trace_status", "rtk_mgpu_scene(m, i)"):
        assert word in section, word
    # rtk_closest_rule.h is used, not changed: the functions this rule stands on are there under their names
    closest = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_closest_rule.h")).read()
    for word in ("rtk_closest_triangle(", "rtk_closest_box_bound(", "rtk_closest_better(", "rtk_within"):
        assert (word in closest) == (word != "rtk_within"), word
    mk = open(os.path.join(ROOT, "rtk_amd", "csrc", "Makefile")).read()
    assert "rtk_within_rule.h" in mk and "rtk_within.hip" in mk and "-fhip-fp32-correctly-rounded-divide-sqrt" in mk
    kernel = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_within.hip")).read()
    assert "rtk_within_insert(" in kernel and "rtk_within_skip(" in kernel and "rtk_within_candidate(" in kernel and "rtk_within_live(" in kernel
    assert "kernel-resource-usage" in kernel and "scratch 0" in kernel


@pytest.mark.parametrize("room", [0, 1, 2, 3, 7, 64])
def test_insertion_alone(driver, tmp_path, room):
    """Every stream into a segment of `room` entries: the first `room` of the sorted stream, the rest of the segment and the
    guards untouched"""
    streams = candidate_streams()
    text = "".join("i %d %d %s\n" % (room, len(c), hexes(c)) for _, c in streams)
    out = run_driver(driver, text, len(streams), tmp_path, "insert_%d" % room)
    full = 0
    for (kind, c), line in zip(streams, out):
        want = sorted_prefix(c, room)
        kept = int(line[0])
        rec, pts = split_segment(line[1:], room)
        assert kept == len(want), kind
        assert rec[:kept].tobytes() == want[:, :4].tobytes() and pts[:kept].tobytes() == want[:, 4:].tobytes(), kind
        assert (rec[kept:] == FILL).all() and (pts[kept:] == FILL).all(), kind
        full += kept == room
        if kind == "ties" and room >= 2:
            d, prim = rec[:kept, 0].copy().view(np.float32), rec[:kept, 3]
            assert ((np.diff(d) > 0) | ((np.diff(d) == 0) & (np.diff(prim.astype(np.int64)) > 0))).all()
            assert (np.diff(d) == 0).any()                            # (equal dist2 values did meet)
    assert full >= 6 or room == 64


def small_tree(rng, tris, max_leaf):
    """A 4-wide tree over tris [T, 3, 3] in the driver's words: nodes uint32 [N, 28], triangle records uint32 [T, 11] in leaf
    order. Boxes are the exact min / max of what lies below; leaves hold 1 to max_leaf records; empty slots occur."""
    lo, hi = tri_box(tris[:, 0], tris[:, 1], tris[:, 2])
    nodes, recs = [], []

    def leaf(idx):
        first = len(recs)
        for k, t in enumerate(idx):
            recs.append(np.concatenate([tris[t].reshape(9).view(np.uint32), np.array([t, k == len(idx) - 1], np.uint32)]))
        return 0x80000000 | first

    def build(idx):
        at = len(nodes)
        nodes.append(None)
        axis = int(np.argmax(hi[idx].max(0) - lo[idx].min(0)))
        idx = idx[np.argsort((lo[idx, axis] + hi[idx, axis]), kind="stable")]
        parts = [p for p in np.array_split(idx, rng.randint(2, 5)) if len(p)]
        box = np.zeros((6, 4), np.float32)
        child = np.full(4, NONE, np.uint32)
        slots = rng.permutation(4)[:len(parts)]
        for s, part in zip(slots, parts):
            box[0::2, s], box[1::2, s] = lo[part].min(0), hi[part].max(0)
            child[s] = leaf(part) if len(part) <= rng.randint(1, max_leaf + 1) else build(part)
        nodes[at] = np.concatenate([box.view(np.uint32).reshape(-1), child])
        return at

    build(np.arange(len(tris)))
    return np.array(nodes, np.uint32), np.array(recs, np.uint32)


def walk_queries(rng, tris):
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    ext = float((hi - lo).max())
    pts = np.concatenate([rng.uniform(lo - 0.1 * ext, hi + 0.1 * ext, (60, 3)), tris[rng.permutation(len(tris))[:20], 1], tris[:10].mean(1)]).astype(np.float32)
    max2 = (rng.choice([0.05, 0.1, 0.2, 0.4], len(pts)) * ext).astype(np.float32) ** 2
    max2[::9] = RTK_INF
    room = rng.randint(0, 7, len(pts))
    room[::7] = len(tris)                                            # room for the whole list
    # the limit cases: no candidates, no walk
    bad_pts = rng.uniform(lo, hi, (9, 3)).astype(np.float32)
    bad_max = np.array([0.0, -0.0, -1.0, np.nan, -np.inf, RTK_INF, RTK_INF, RTK_INF, 1e-45], np.float32)
    bad_pts[5, 0], bad_pts[6, 1], bad_pts[7, 2] = np.nan, np.inf, -np.inf
    return np.concatenate([pts, bad_pts]), np.concatenate([max2, bad_max]), np.concatenate([room, np.full(9, 5)])


def test_host_walk_equals_brute_force_in_every_order(driver, tmp_path):
    """A soup with exact duplicates (equal dist2 under two ids) under a random 4-wide tree, leaves of 1 to 5: count and kept
    prefix equal brute force bit for bit whichever way the children are visited"""
    rng = np.random.RandomState(5)
    base = (rng.uniform(0, 1, (70, 1, 3)) + rng.uniform(-0.08, 0.08, (70, 3, 3))).astype(np.float32)
    tris = np.concatenate([base, base[:20]])                         # ids 70 .. 89 repeat ids 0 .. 19
    nodes, recs = small_tree(rng, tris, 5)
    assert len(nodes) > 8 and set(np.diff(np.nonzero(np.concatenate([[1], recs[:, 10]]))[0]).tolist()) >= {1, 2, 3}
    pts, max2, room = walk_queries(rng, tris)
    ref = brute_force_within(tris, np.arange(len(tris)), pts, max2, room)
    assert (ref.counts == 0).any() and (ref.counts > 6).any() and (ref.counts[-9:] == 0).all()
    text = "n %d %s\nt %d %s\n" % (len(nodes), hexes(nodes), len(recs), hexes(recs))
    qwords = np.concatenate([pts.view(np.uint32), max2.view(np.uint32)[:, None], room.astype(np.uint32)[:, None]], 1)
    for order in (0, 1, 2):
        out = run_driver(driver, text + "".join("q %d %s\n" % (order, hexes(w)) for w in qwords), len(qwords), tmp_path, "walk_%d" % order)
        for i, line in enumerate(out):
            want_rec, want_pts = ref.kept[i]
            rec, seg_pts = split_segment(line[2:], int(room[i]))
            assert int(line[0]) == ref.counts[i], (order, i)
            assert int(line[1]) == len(want_rec), (order, i)
            assert rec[:len(want_rec)].tobytes() == want_rec.tobytes() and seg_pts[:len(want_rec)].tobytes() == want_pts.tobytes(), (order, i)
            assert (rec[len(want_rec):] == FILL).all() and (seg_pts[len(want_rec):] == FILL).all(), (order, i)
    # the duplicates did meet, and the lower id stands first
    both = [r for r, _ in ref.lists if len(r) > 1 and (np.diff(r[:, 0].copy().view(np.float32)) == 0).any()]
    assert both and all((np.diff(r[:, 3].astype(np.int64))[np.diff(r[:, 0].copy().view(np.float32)) == 0] > 0).all() for r in both)
    # a scene without triangles: no candidates
    out = run_driver(driver, "n 0\nt 0\nq 0 %s\n" % hexes(qwords[0]), 1, tmp_path, "empty")
    assert out[0][:2] == ["0", "0"]


def test_header_symbols_and_argtypes(api):
    text = open(os.path.join(ROOT, "include", "rtk_amd.h")).read()
    for word in ("int rtk_dev_triangles_within_count(const rtk_dev_scene *ds, const rtk_point_query *d_queries, size_t num_queries,",
                 "int rtk_dev_triangles_within_all(const rtk_dev_scene *ds, const rtk_point_query *d_queries, size_t num_queries,",
                 "int rtk_dev_triangles_within_counted(const rtk_dev_scene *ds, const rtk_point_query *d_queries, size_t num_queries,",
                 "uint32_t rtk_amd_within_stack_entries(void);"):
        assert word in text, word
    assert text.index("/* ---- Closest points") < text.index("/* ---- Triangles within a distance") < text.index("/* ---- Every hit along a ray")
    L = api.lib()
    for name in ("rtk_dev_triangles_within_count", "rtk_dev_triangles_within_all", "rtk_dev_triangles_within_counted", "rtk_amd_within_stack_entries"):
        assert name in api.RTK_AMD_H_SYMBOLS and hasattr(L, name), name
    assert L.rtk_dev_triangles_within_count.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(api.RayList), C.c_void_p, C.c_void_p]
    assert L.rtk_dev_triangles_within_all.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(api.RayList), C.c_void_p, C.c_void_p, C.c_void_p,
                                                       C.c_void_p, C.c_void_p]
    assert L.rtk_dev_triangles_within_counted.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                           C.POINTER(api.TraceCounters)]
    assert L.rtk_dev_triangles_within_count.restype == C.c_int and L.rtk_dev_triangles_within_all.restype == C.c_int
    assert L.rtk_dev_triangles_within_counted.restype == C.c_int
    assert L.rtk_amd_within_stack_entries.restype == C.c_uint32 and 1 <= L.rtk_amd_within_stack_entries() <= 64
    for name in ("count_within_device", "within_all_device", "triangles_within_counted", "triangles_within", "nearest_triangles"):
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
    bad_lists = (ray_list(struct_size=8), ray_list(flags=1), ray_list(d_count=None))
    # count: scene, queries, n, list, counts, stream
    for args in [(None, dummy, 4, None, dummy, None), (dummy, None, 4, None, dummy, None), (dummy, dummy, 4, None, None, None),
                 (dummy, dummy, 1 << 32, None, dummy, None), (dummy, dummy, 1 << 32, C.byref(ray_list()), dummy, None)] + \
                [(dummy, dummy, 4, C.byref(l), dummy, None) for l in bad_lists]:
        assert L.rtk_dev_triangles_within_count(*args) == ERR_BAD_ARG, args
        assert "rtk_dev_triangles_within_count:" in api.last_error()
    # fill: scene, queries, n, list, offsets, records, points, written, stream
    for args in [(None, dummy, 4, None, dummy, dummy, None, None, None), (dummy, None, 4, None, dummy, dummy, None, None, None),
                 (dummy, dummy, 4, None, None, dummy, None, None, None), (dummy, dummy, 4, None, dummy, None, dummy, dummy, None),
                 (dummy, dummy, 1 << 32, None, dummy, dummy, None, None, None)] + \
                [(dummy, dummy, 4, C.byref(l), dummy, dummy, None, None, None) for l in bad_lists]:
        assert L.rtk_dev_triangles_within_all(*args) == ERR_BAD_ARG, args
        assert "rtk_dev_triangles_within_all:" in api.last_error()
    # counted: scene, queries, n, offsets, records, points, counts or written, counters
    ctr = api.TraceCounters()
    for args in ((dummy, dummy, 4, None, None, None, dummy, None), (None, dummy, 4, None, None, None, dummy, C.byref(ctr)),
                 (dummy, None, 4, None, None, None, dummy, C.byref(ctr)), (dummy, dummy, 4, None, None, None, None, C.byref(ctr)),
                 (dummy, dummy, 4, dummy, None, None, None, C.byref(ctr)), (dummy, dummy, 1 << 32, None, None, None, dummy, C.byref(ctr))):
        assert L.rtk_dev_triangles_within_counted(*args) == ERR_BAD_ARG, args
        assert "rtk_dev_triangles_within_counted:" in api.last_error()
    # no queries: nothing to do, nothing launched
    assert L.rtk_dev_triangles_within_count(dummy, None, 0, None, None, None) == 0
    assert L.rtk_dev_triangles_within_count(dummy, dummy, 0, C.byref(ray_list()), dummy, None) == 0
    assert L.rtk_dev_triangles_within_all(dummy, None, 0, None, None, None, None, None, None) == 0
    assert L.rtk_dev_triangles_within_all(dummy, dummy, 0, C.byref(ray_list()), dummy, dummy, dummy, dummy, None) == 0
    ctr.rays = 7
    assert L.rtk_dev_triangles_within_counted(dummy, None, 0, None, None, None, None, C.byref(ctr)) == 0 and ctr.rays == 0
