"""Triangles that touch a box without a GPU: the rule of rtk_amd/csrc/rtk_box_rule.h, run by tests/box_rule_driver.cpp under the
address and undefined-behaviour sanitizers, against numpy (tests/box_ref.py): on integer inputs, where every float32 operation of
the rule is exact, against the same 13-axis test in Python integers and against an independent exact answer (the triangle
clipped against the box's six half-spaces in fractions); on non-integer inputs bit for bit against numpy; the skip against the
candidates; the bounded sorted insertion alone, with guard words around the segment; a host walk of a small 4-wide tree in three
child orders against brute force; and the parts of the interface that need no device -- header text, symbols, argtypes, the
refusals decided before any HIP call."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests.box_ref import brute_force_boxes, candidate_np, boxes_touch_np, centre_np, live_np, separated_np, skip_np
from tests.test_within_cpu import hexes, run_driver, small_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_BAD_ARG = -2
GUARD = 4                                     # entries on either side of the driver's segment
FILL = 0x7e7e7e7e


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """The driver built against the rule headers alone (no HIP include path, -Wall -Werror, no FMA contraction as in the
    library) with both sanitizers. -O2 and -mfma: a compiler that were allowed to contract would do it here."""
    exe = str(tmp_path_factory.mktemp("box_rule") / "box_rule_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-mfma", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "rtk_amd", "csrc"), os.path.join(ROOT, "tests", "box_rule_driver.cpp"), "-o", exe])
    return exe


def run_bulk(exe, v, lo, hi, clo, chi, tmp_path, name):
    """v [N, 3, 3], the others [N, 3], float32 -> the driver's bits per case, uint8 [N]: 1 live, 2 boxes touch, 4 separated, 8 skip"""
    words = np.concatenate([v.reshape(-1, 9), lo, hi, clo, chi], 1).astype(np.float32)
    assert words.shape[1] == 21
    path = str(tmp_path / (name + ".bin"))
    words.tofile(path)
    r = subprocess.run([exe, "-b", path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-200:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    assert lines[1] == "ok" and len(lines[0]) == len(words)
    return np.array([int(ch, 16) for ch in lines[0]], np.uint8)


def numpy_bits(v, lo, hi, clo, chi):
    c, h = centre_np(lo, hi)
    bits = live_np(lo, hi) * 1 + boxes_touch_np(v[:, 0], v[:, 1], v[:, 2], lo, hi) * 2 + separated_np(v[:, 0], v[:, 1], v[:, 2], c, h) * 4 + skip_np(clo, chi, lo, hi) * 8
    assert ((bits & 7 == 3) == candidate_np(v[:, 0], v[:, 1], v[:, 2], lo, hi)).all()
    return bits.astype(np.uint8)


def enlarged(rng, v):
    """a box above each triangle: its own box, grown by nothing on some sides and by something on others"""
    grow = np.abs(v).max((1, 2))[:, None] * rng.choice([0.0, 0.0, 1e-6, 0.3], (len(v), 6)).astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        return (v.min(1) - grow[:, :3]).astype(np.float32), (v.max(1) + grow[:, 3:]).astype(np.float32)


# ---------------------------------------------------------------------------------------------- integer inputs

def integer_cases(seed=7, n=20000):
    """Triangles and boxes with integer coordinates in [-32, 32]: small ranges so that the two meet often, degenerate triangles
    (points, segments), degenerate boxes (lo == hi on one, two or three axes), and contacts by construction: a box face on a
    vertex coordinate, a box corner on a point of an edge."""
    rng = np.random.RandomState(seed)
    centre = rng.randint(-20, 21, (n, 1, 3))
    v = centre + rng.randint(-12, 13, (n, 3, 3))
    kind = rng.randint(0, 10, n)
    v[kind == 0, 1] = v[kind == 0, 0]; v[kind == 0, 2] = v[kind == 0, 0]                     # a point
    v[kind == 1, 1] = v[kind == 1, 0]                                                       # a segment, two equal vertices
    seg = kind == 2                                                                         # a segment, three collinear vertices
    d = rng.randint(-4, 5, (n, 3))
    v[seg, 1] = v[seg, 0] + d[seg]; v[seg, 2] = v[seg, 0] - 2 * d[seg]
    lo = centre[:, 0] + rng.randint(-14, 10, (n, 3))
    size = rng.randint(0, 9, (n, 3)) * (rng.randint(0, 4, (n, 3)) != 0)                     # a quarter of the extents are 0
    hi = lo + size
    touch = rng.randint(0, 4, n)
    a = rng.randint(0, 3, n)
    rows = np.arange(n)
    # a face on a vertex coordinate
    t1 = touch == 1
    lo[t1, a[t1]] = v[t1, rng.randint(0, 3, n)[t1], a[t1]]; hi[t1, a[t1]] = lo[t1, a[t1]] + size[t1, a[t1]]
    t2 = touch == 2
    hi[t2, a[t2]] = v[t2, rng.randint(0, 3, n)[t2], a[t2]]; lo[t2, a[t2]] = hi[t2, a[t2]] - size[t2, a[t2]]
    # a corner on the midpoint of an edge with even differences (the contact is edge against corner)
    t3 = touch == 3
    v[t3, 1] = v[t3, 0] + 2 * rng.randint(-5, 6, (n, 3))[t3]
    mid = (v[:, 0] + v[:, 1]) // 2
    lo[t3] = mid[t3]; hi[t3] = lo[t3] + size[t3]
    v, lo, hi = np.clip(v, -32, 32), np.clip(lo, -32, 32), np.clip(hi, -32, 32)
    assert (lo <= hi).all() and rows.size == n
    return v, lo, hi


def sat13_integers(v, lo, hi):
    """The 13-axis test in Python integers, in half units: c2 = lo + hi, h2 = hi - lo, w2 = 2 v - c2"""
    v = [[int(x) for x in p] for p in v]
    lo, hi = [int(x) for x in lo], [int(x) for x in hi]
    for a in range(3):
        if not (min(p[a] for p in v) <= hi[a] and max(p[a] for p in v) >= lo[a]):
            return False
    c2 = [lo[a] + hi[a] for a in range(3)]
    h2 = [hi[a] - lo[a] for a in range(3)]
    w = [[2 * p[a] - c2[a] for a in range(3)] for p in v]
    e = [[v[(k + 1) % 3][a] - v[k][a] for a in range(3)] for k in range(3)]
    for ej in e:
        for i in range(3):
            ia, ib = (i + 1) % 3, (i + 2) % 3                    # unit_i X e: p = e[ia] * w[ib] - e[ib] * w[ia]
            p = [ej[ia] * wk[ib] - ej[ib] * wk[ia] for wk in w]
            r = h2[ia] * abs(ej[ib]) + h2[ib] * abs(ej[ia])
            if min(p) > r or max(p) < -r:
                return False
    n = [e[0][1] * e[1][2] - e[0][2] * e[1][1], e[0][2] * e[1][0] - e[0][0] * e[1][2], e[0][0] * e[1][1] - e[0][1] * e[1][0]]
    d = sum(n[a] * w[0][a] for a in range(3))
    r = sum(h2[a] * abs(n[a]) for a in range(3))
    return not (d > r or d < -r)


def clipped_is_not_empty(v, lo, hi):
    """Sutherland-Hodgman against the six closed half-spaces in fractions: the triangle and the box touch iff something is left"""
    poly = [[Fraction(int(x)) for x in p] for p in v]
    for a in range(3):
        for bound, sign in ((int(lo[a]), 1), (int(hi[a]), -1)):
            out = []
            for k in range(len(poly)):
                p, q = poly[k], poly[(k + 1) % len(poly)]
                dp, dq = sign * (p[a] - bound), sign * (q[a] - bound)      # >= 0: inside
                if dp >= 0:
                    out.append(p)
                if (dp > 0 and dq < 0) or (dp < 0 and dq > 0):
                    t = dp / (dp - dq)
                    out.append([p[i] + t * (q[i] - p[i]) for i in range(3)])
            poly = out
            if not poly:
                return False
    return True


def test_integer_inputs_equal_the_exact_answers(driver, tmp_path):
    v, lo, hi = integer_cases()
    n = len(v)
    vf, lof, hif = v.astype(np.float32), lo.astype(np.float32), hi.astype(np.float32)
    rng = np.random.RandomState(1)
    clo, chi = enlarged(rng, vf)
    got = run_bulk(driver, vf, lof, hif, clo, chi, tmp_path, "integers")
    ref = numpy_bits(vf, lof, hif, clo, chi)
    assert (got == ref).all(), np.nonzero(got != ref)[0][:10]
    assert (got & 1).all()
    cand = (got & 7) == 3
    want = np.array([sat13_integers(v[i], lo[i], hi[i]) for i in range(n)])
    bad = np.nonzero(cand != want)[0]
    assert len(bad) == 0, (len(bad), v[bad[:3]], lo[bad[:3]], hi[bad[:3]])
    e0, e1 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 1]
    proper = np.cross(e0, e1).any(1)
    exact = np.array([clipped_is_not_empty(v[i], lo[i], hi[i]) for i in np.nonzero(proper)[0]])
    bad = np.nonzero(proper)[0][cand[proper] != exact]
    assert len(bad) == 0, (len(bad), v[bad[:3]], lo[bad[:3]], hi[bad[:3]])
    # what the cases hold: both answers in number, degenerate triangles and boxes, contacts that only a closed test keeps
    print("integer cases %d: candidates %d, proper %d, degenerate candidates %d" % (n, cand.sum(), proper.sum(), (cand & ~proper).sum()))
    assert 0.15 * n < cand.sum() < 0.85 * n and (~proper).sum() > 0.2 * n and (cand & ~proper).sum() > 500
    assert ((lo == hi).sum(1) == 3).sum() > 50 and ((lo == hi).sum(1) == 1).sum() > 1000
    touching = cand & ((v.min(1) == hi) | (v.max(1) == lo)).any(1)
    assert touching.sum() > 500
    # a segment whose box touches the query is NOT always a candidate: its own nine axes still separate
    segs = ~proper & (e0.any(1) | e1.any(1))
    assert ((got[segs] & 7) == 7).any()
    # rule 5 never skips a box above a candidate
    assert not ((got & 8 != 0) & cand).any() and (got & 8 != 0).sum() > 0.1 * n


# ---------------------------------------------------------------------------------------------- non-integer inputs

PER = 45000                                   # cases per kind of the non-integer inputs


def float_cases(seed=3, per=PER):
    rng = np.random.RandomState(seed)
    vs, los, his = [], [], []
    # five pairs of (triangle size, box size); the box lies about a point of the triangle, so that the two meet often but not always
    for tri, box in ((1.0, 1.0), (1.0, 0.05), (0.05, 1.0), (1e3, 1e-3), (1e-3, 1e3)):
        centre = rng.uniform(-1, 1, (per, 1, 3)) * max(tri, box)
        v = centre + rng.uniform(-tri, tri, (per, 3, 3))
        vs.append(v)
        bary = rng.dirichlet([1, 1, 1], per)
        mid = (v * bary[:, :, None]).sum(1) + rng.uniform(-1.5, 1.5, (per, 3)) * box
        half = rng.uniform(0, box, (per, 3))
        los.append(mid - half); his.append(mid + half)
    # slivers: the third vertex on the first edge but for a few ulps; and exactly degenerate ones
    a, b = rng.uniform(-1, 1, (per, 3)), rng.uniform(-1, 1, (per, 3))
    t = rng.uniform(-0.5, 1.5, (per, 1))
    c = a + t * (b - a) + rng.choice([0.0, 1e-7, 1e-5], (per, 1)) * rng.uniform(-1, 1, (per, 3))
    vs.append(np.stack([a, b, c], 1))
    mid = a + rng.uniform(0, 1, (per, 1)) * (b - a) + rng.uniform(-0.1, 0.1, (per, 3))
    half = rng.uniform(0, 0.1, (per, 3))
    los.append(mid - half); his.append(mid + half)
    # denormals: everything within a few thousand ulps of zero
    tiny = np.float32(1e-45).astype(np.float64)
    vs.append(rng.randint(-3000, 3000, (per // 2, 3, 3)) * tiny)
    lo = rng.randint(-3000, 3000, (per // 2, 3)) * tiny
    los.append(lo); his.append(lo + rng.randint(0, 2000, (per // 2, 3)) * tiny)
    # boxes whose hi - lo or lo + hi overflows, around ordinary and huge triangles; queries that are not live
    m = per // 2
    vs.append(rng.uniform(-1, 1, (m, 3, 3)) * rng.choice([1.0, 1e30, 3e38], (m, 1, 1)))
    lo = -rng.choice([1.0, 2e38, 3.4e38], (m, 3)) * rng.uniform(0.5, 1, (m, 3))
    hi = rng.choice([1.0, 2e38, 3.4e38], (m, 3)) * rng.uniform(0.5, 1, (m, 3))
    flip = rng.randint(0, 8, m) == 0
    lo[flip], hi[flip] = hi[flip] * 0.9, hi[flip]                          # (both large and of one sign: lo + hi overflows)
    bad = rng.randint(0, 10, m) == 0
    lo[bad, 0] = rng.choice([np.nan, np.inf, -np.inf, 5e38], bad.sum())
    worse = rng.randint(0, 10, m) == 0
    hi[worse, 2] = rng.choice([np.nan, np.inf, -np.inf, -5e38], worse.sum())
    los.append(lo); his.append(hi)
    with np.errstate(over="ignore"):
        return tuple(np.concatenate(x).astype(np.float32) for x in (vs, los, his))


def test_non_integer_inputs_equal_numpy_bit_for_bit(driver, tmp_path):
    v, lo, hi = float_cases()
    n = len(v)
    assert n >= 300000
    clo, chi = enlarged(np.random.RandomState(2), v)
    got = run_bulk(driver, v, lo, hi, clo, chi, tmp_path, "floats")
    ref = numpy_bits(v, lo, hi, clo, chi)
    bad = np.nonzero(got != ref)[0]
    assert len(bad) == 0, (len(bad), bad[:5], got[bad[:5]], ref[bad[:5]], v[bad[:2]], lo[bad[:2]], hi[bad[:2]])
    cand = (got & 7) == 3
    for k, name in enumerate(("1 / 1", "1 / 0.05", "0.05 / 1", "1e3 / 1e-3", "1e-3 / 1e3", "slivers")):
        part = cand[k * PER:(k + 1) * PER]
        print("%-12s candidates %5.1f %%, separated behind touching boxes %5.1f %%" % (name, 100 * part.mean(), 100 * ((got[k * PER:(k + 1) * PER] & 7) == 7).mean()))
        assert 0.02 < part.mean() < 0.98, name
    # the other ten axes did decide, queries that are not live occurred, and so did the NaNs of an overflowing box
    assert ((got & 7) == 7).sum() > 5000 and ((got & 1) == 0).sum() > 1000
    with np.errstate(over="ignore", invalid="ignore"):
        assert np.isinf(hi - lo).any() and np.isinf(lo + hi).any()
    # rule 5 never skips a box above a candidate
    assert not ((got & 8 != 0) & cand).any() and (got & 8 != 0).sum() > 0.1 * n


# ---------------------------------------------------------------------------------------------- insertion, tree

def split_segment(words, room):
    """the driver's dump -> the segment's words [room]; the guards must be untouched"""
    w = np.array([int(x, 16) for x in words], np.uint32)
    assert len(w) == GUARD + room + GUARD
    assert (w[:GUARD] == FILL).all() and (w[GUARD + room:] == FILL).all(), "a guard was written"
    return w[GUARD:GUARD + room]


def id_streams():
    rng = np.random.RandomState(20250611)
    streams = []
    for n, kind in ((0, "plain"), (1, "plain"), (5, "plain"), (40, "plain"), (200, "plain"), (64, "descending"), (64, "ascending"), (50, "repeats")):
        ids = rng.randint(0, 2 ** 32 - 1, n, dtype=np.uint64).astype(np.uint32) if kind == "plain" else rng.permutation(n).astype(np.uint32)
        if kind == "descending":
            ids = np.sort(ids)[::-1].copy()
        if kind == "ascending":
            ids = np.sort(ids)
        if kind == "repeats":
            ids = ids // 3
        streams.append((kind, ids))
    return streams


@pytest.mark.parametrize("room", [0, 1, 3, 8])
def test_insertion_alone(driver, tmp_path, room):
    """Every stream into a segment of `room` entries: the first `room` of the sorted stream, the rest of the segment and the
    guards untouched"""
    streams = id_streams()
    text = "".join("i %d %d %s\n" % (room, len(ids), hexes(ids)) for _, ids in streams)
    out = run_driver(driver, text, len(streams), tmp_path, "insert_%d" % room)
    for (kind, ids), line in zip(streams, out):
        want = np.sort(ids, kind="stable")[:room]
        kept = int(line[0])
        seg = split_segment(line[1:], room)
        assert kept == len(want), kind
        assert seg[:kept].tobytes() == want.tobytes(), kind
        assert (seg[kept:] == FILL).all(), kind


def walk_boxes(rng, tris):
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    ext = hi - lo
    mid = rng.uniform(lo, hi, (60, 3))
    half = rng.choice([0.02, 0.1, 0.3], (60, 1)) * ext * rng.uniform(0.2, 1, (60, 3))
    blo, bhi = [mid - half], [mid + half]
    verts = tris[rng.permutation(len(tris))[:15], 1]
    blo.append(verts); bhi.append(verts)                             # point boxes at vertices
    blo.append(verts - np.float32(0.1) * ext); bhi.append(verts)     # a corner exactly on a vertex
    blo.append([lo, lo - ext]); bhi.append([hi, hi + ext])           # the whole scene
    blo.append([hi + ext, lo, lo, lo]); bhi.append([hi + 2 * ext, lo - 1, hi * np.float32(np.nan), hi * np.float32(np.inf)])   # far, lo > hi, NaN, inf
    blo, bhi = np.concatenate(blo).astype(np.float32), np.concatenate(bhi).astype(np.float32)
    room = rng.randint(0, 7, len(blo))
    room[::7] = len(tris)                                            # room for the whole list
    return blo, bhi, room


def test_host_walk_equals_brute_force_in_every_order(driver, tmp_path):
    """A soup under a random 4-wide tree, leaves of 1 to 5: count and kept prefix equal brute force bit for bit whichever way the
    children are visited"""
    rng = np.random.RandomState(5)
    tris = (rng.uniform(0, 1, (90, 1, 3)) + rng.uniform(-0.08, 0.08, (90, 3, 3))).astype(np.float32)
    nodes, recs = small_tree(rng, tris, 5)
    assert len(nodes) > 8
    lo, hi, room = walk_boxes(rng, tris)
    ref = brute_force_boxes(tris, np.arange(len(tris)), lo, hi, room)
    assert (ref.counts == 0).any() and (ref.counts > 6).any() and (ref.counts == 90).any() and (ref.counts[-4:] == 0).all()
    text = "n %d %s\nt %d %s\n" % (len(nodes), hexes(nodes), len(recs), hexes(recs))
    qwords = np.concatenate([lo.view(np.uint32), hi.view(np.uint32), room.astype(np.uint32)[:, None]], 1)
    for order in (0, 1, 2):
        out = run_driver(driver, text + "".join("q %d %s\n" % (order, hexes(w)) for w in qwords), len(qwords), tmp_path, "walk_%d" % order)
        for i, line in enumerate(out):
            want = ref.kept[i]
            seg = split_segment(line[2:], int(room[i]))
            assert int(line[0]) == ref.counts[i], (order, i)
            assert int(line[1]) == len(want), (order, i)
            assert seg[:len(want)].tobytes() == want.tobytes(), (order, i)
            assert (seg[len(want):] == FILL).all(), (order, i)
    # a scene without triangles: no candidates
    out = run_driver(driver, "n 0\nt 0\nq 0 %s\n" % hexes(qwords[0]), 1, tmp_path, "empty")
    assert out[0][:2] == ["0", "0"]


# ---------------------------------------------------------------------------------------------- the interface

def test_rule_header_includes_no_hip_and_states_its_rules():
    text = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_box_rule.h")).read()
    assert [l.split()[1] for l in text.splitlines() if l.startswith("#include")] == ['"rtk_closest_rule.h"']
    assert "hip_runtime" not in text and "__global__" not in text and "fmaf" not in text
    text = " ".join(text.replace("\n//", "\n").split())              # (the comment's line breaks and slashes taken out)
    for word in ("1. LIVE", "2. BOXES", "3. THE OTHER TEN AXES", "4. CANDIDATE", "5. SKIP", "6. INSERT", "CLOSED", "FLOAT RULE", "DEFINED BY IT",
                 "ZERO-AREA", "NON-FINITE", "NOTHING ELSE IS PROMISED", "NEVER SEPARATES", "WITHOUT A MARGIN", "ASCENDING PRIMITIVE ID"):
        assert word in text, word
    closest = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_closest_rule.h")).read()
    assert "rtk_box" not in closest                                   # (used for its macros, not changed)
    header = open(os.path.join(ROOT, "include", "rtk_amd.h")).read()
    section = header[header.index("/* ---- Triangles that touch a box"):header.index("/* ---- Every hit along a ray")]
    section = " ".join(section.replace("\n *", "\n").split())
    for word in ("rtk_box_rule.h", "ARE NOT WRITTEN", "A SLOT THAT IS NOT LISTED IS NOT WRITTEN", "d_offsets[i] = i * k", "DETERMINISTIC", "NOTHING ELSE IS PROMISED",
                 "rtk_dev_trace_status", "rtk_mgpu_scene(m, i)", "CANNOT BE CULLED BY WHAT IT HAS KEPT", "ASCENDING PRIMITIVE ID", "touching counts"):
        assert word in section, word
    mk = open(os.path.join(ROOT, "rtk_amd", "csrc", "Makefile")).read()
    assert "rtk_box_rule.h" in mk and "rtk_box.hip" in mk and "rtk_overlap_walk.h" in mk
    # the shape's own calls in its file, what the three overlap shapes share in the walk
    kernel = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_box.hip")).read()
    walk = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_overlap_walk.h")).read()
    assert "rtk_box_insert(" in walk and "rtk_box_skip(" in kernel and "rtk_box_candidate(" in kernel and "rtk_box_live(" in kernel
    assert "rtk_box_boxes_touch(" in kernel and "rtk_box_separated(" in kernel         # (rtk_box_candidate's one line, spelled out there)
    assert "kernel-resource-usage" in kernel and "scratch 0" in kernel


def test_header_symbols_and_argtypes(api):
    from rtk_amd import types
    text = open(os.path.join(ROOT, "include", "rtk_amd.h")).read()
    for word in ("typedef struct rtk_box_query { float lo[3], hi[3]; } rtk_box_query;",
                 "int rtk_dev_triangles_in_box_count(const rtk_dev_scene *ds, const rtk_box_query *d_boxes, size_t num_queries,",
                 "int rtk_dev_triangles_in_box_all(const rtk_dev_scene *ds, const rtk_box_query *d_boxes, size_t num_queries,",
                 "int rtk_dev_triangles_in_box_counted(const rtk_dev_scene *ds, const rtk_box_query *d_boxes, size_t num_queries,",
                 "uint32_t rtk_amd_box_stack_entries(void);"):
        assert word in text, word
    assert text.index("/* ---- Triangles within a distance") < text.index("/* ---- Triangles that touch a box") < text.index("/* ---- Every hit along a ray")
    assert types.BOX_QUERY_DTYPE.itemsize == 24 and types.BOX_QUERY_DTYPE.names == ("lo", "hi") and types.BOX_QUERY_DTYPE.fields["hi"][1] == 12
    L = api.lib()
    for name in ("rtk_dev_triangles_in_box_count", "rtk_dev_triangles_in_box_all", "rtk_dev_triangles_in_box_counted", "rtk_amd_box_stack_entries"):
        assert name in api.RTK_AMD_H_SYMBOLS and hasattr(L, name), name
    assert L.rtk_dev_triangles_in_box_count.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(api.RayList), C.c_void_p, C.c_void_p]
    assert L.rtk_dev_triangles_in_box_all.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(api.RayList), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert L.rtk_dev_triangles_in_box_counted.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(api.TraceCounters)]
    assert L.rtk_dev_triangles_in_box_count.restype == C.c_int and L.rtk_dev_triangles_in_box_all.restype == C.c_int
    assert L.rtk_dev_triangles_in_box_counted.restype == C.c_int
    assert L.rtk_amd_box_stack_entries.restype == C.c_uint32 and 1 <= L.rtk_amd_box_stack_entries() <= 64
    for name in ("count_in_boxes_device", "in_boxes_all_device", "triangles_in_boxes_counted", "triangles_in_boxes", "occupancy"):
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
    # count: scene, boxes, n, list, counts, stream
    for args in [(None, dummy, 4, None, dummy, None), (dummy, None, 4, None, dummy, None), (dummy, dummy, 4, None, None, None),
                 (dummy, dummy, 1 << 32, None, dummy, None), (dummy, dummy, 1 << 32, C.byref(ray_list()), dummy, None)] + \
                [(dummy, dummy, 4, C.byref(l), dummy, None) for l in bad_lists]:
        assert L.rtk_dev_triangles_in_box_count(*args) == ERR_BAD_ARG, args
        assert "rtk_dev_triangles_in_box_count:" in api.last_error()
    # fill: scene, boxes, n, list, offsets, prims, written, stream
    for args in [(None, dummy, 4, None, dummy, dummy, None, None), (dummy, None, 4, None, dummy, dummy, None, None),
                 (dummy, dummy, 4, None, None, dummy, None, None), (dummy, dummy, 4, None, dummy, None, dummy, None),
                 (dummy, dummy, 1 << 32, None, dummy, dummy, None, None)] + \
                [(dummy, dummy, 4, C.byref(l), dummy, dummy, None, None) for l in bad_lists]:
        assert L.rtk_dev_triangles_in_box_all(*args) == ERR_BAD_ARG, args
        assert "rtk_dev_triangles_in_box_all:" in api.last_error()
    # counted: scene, boxes, n, offsets, prims, counts or written, counters
    ctr = api.TraceCounters()
    for args in ((dummy, dummy, 4, None, None, dummy, None), (None, dummy, 4, None, None, dummy, C.byref(ctr)),
                 (dummy, None, 4, None, None, dummy, C.byref(ctr)), (dummy, dummy, 4, None, None, None, C.byref(ctr)),
                 (dummy, dummy, 4, dummy, None, None, C.byref(ctr)), (dummy, dummy, 1 << 32, None, None, dummy, C.byref(ctr))):
        assert L.rtk_dev_triangles_in_box_counted(*args) == ERR_BAD_ARG, args
        assert "rtk_dev_triangles_in_box_counted:" in api.last_error()
    # no queries: nothing to do, nothing launched
    assert L.rtk_dev_triangles_in_box_count(dummy, None, 0, None, None, None) == 0
    assert L.rtk_dev_triangles_in_box_count(dummy, dummy, 0, C.byref(ray_list()), dummy, None) == 0
    assert L.rtk_dev_triangles_in_box_all(dummy, None, 0, None, None, None, None, None) == 0
    assert L.rtk_dev_triangles_in_box_all(dummy, dummy, 0, C.byref(ray_list()), dummy, dummy, dummy, None) == 0
    ctr.rays = 7
    assert L.rtk_dev_triangles_in_box_counted(dummy, None, 0, None, None, None, C.byref(ctr)) == 0 and ctr.rays == 0
