"""rtk_amd/csrc/rtk_node_finish.h without a GPU: the header that turns the boxes and child words of a 4-wide node into its order
words (DevNode::order), its compressed copy (DevNodeQ) and the scene bound, run by tests/node_finish_driver.cpp under the address
and undefined-behaviour sanitizers and compared, bit for bit, with a reference written from the format's contract in rtk_node.h /
rtk_dev.h -- not from the header's text. Whatever the contract states exactly is computed in fractions.Fraction. (One exception:
the contract says nothing of a NaN plane, and the rule taken for it below is the one fminf and fmaxf give the header; those cases
pin that the rule stays, not that it is right.)

The contract, per axis of a compressed node:
  org    the smallest low plane of the non-empty children;
  scale  a power of two: the smallest s (a float, so s >= 2^-149) with 254 * s >= fl(max - min), max the largest high plane and
         fl() one float32 subtraction; doubled at most three times, and only while some high plane needs more than 255;
  bytes  low byte = the LARGEST q in 0..255 with org + q * scale <= lo, high byte = the SMALLEST q in 0..255 with
         org + q * scale >= hi (containment and tightness in one: a q one step looser fails); an empty slot has 255 / 0;
         a flat axis (max == min) has every byte 0 and the smallest normal float as scale; a node without children is flat at 0;
  child  words copied;
  misfit reported exactly when no such scale exists: fl(max - min) not finite (a low plane at
         -inf, a high plane at +inf, an extent that overflows float). A low plane at +inf or a high plane at -inf beside finite
         ones is an inverted box that fits: the last q that holds, 255 and 0. What the other twelve words of a misfit node hold is not part of the contract (the scene keeps to its exact nodes, nothing reads
         them), so only the flag and the child words are compared there.
Order words, per octant: the stable sort of the slots by the float32 key +-(lo+hi)x +-(lo+hi)y +-(lo+hi)z, summed in that
order; empty slots and NaN keys count as +inf (last, ties to the lower slot); the six pair bits agree with the permutation.
root_bound: the largest |plane| of the non-empty children, inf if one is not finite or beyond 3e38.

Limit: this run proves the header's text under the host's frexpf, ldexpf, floorf and ceilf, and the host's float division by a
denormal step (extents below 2^-126, the only place the header divides). It does not prove the device's versions of those; the
four functions are exact operations (no rounding to get wrong), the division is correctly rounded on both sides
(-fhip-fp32-correctly-rounded-divide-sqrt) with denormals kept, and the validator's containment check of every compressed node
runs on the device after every build."""
import math
import os
import subprocess
from fractions import Fraction as F

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE, LEAF = 0xFFFFFFFF, 0x80000000
MIN_NORMAL = np.float32(2.0 ** -126)
f32 = np.float32


# ---------------------------------------------------------------------------------------------- the reference

def ref_axis(lo, hi, live):
    """One axis: lo, hi float32 [4], live = the non-empty slots -> (org bits, scale bits, low word, high word, and which bits of the
    two words the contract defines), or None: misfit."""
    if not live:
        return 0, int(MIN_NORMAL.view(np.uint32)), 0xFFFFFFFF, 0, 0xFFFFFFFF, 0xFFFFFFFF
    # A NaN plane: the documents are silent. The rule chosen here is the one the builder's unions follow: a NaN
    # takes part in no minimum and no maximum, the node is no misfit for it (a scene with one NaN triangle keeps its compressed
    # nodes), and the byte of that plane is not defined -- the validator reports the child, nothing can contain a NaN box.
    lows, tops = [lo[k] for k in live if not np.isnan(lo[k])], [hi[k] for k in live if not np.isnan(hi[k])]
    if not lows or not tops:
        return 0, int(MIN_NORMAL.view(np.uint32)), 0, 0, 0, 0     # nothing to span: flat at 0, no byte defined
    org, top = min(lows), max(tops)
    with np.errstate(all="ignore"):
        ext = f32(top) - f32(org)
    if not np.isfinite(ext):
        return None                                               # no power of two has 254 * s >= inf
    ml = sum(255 << (8 * k) for k in range(4) if k not in live or not np.isnan(lo[k]))
    mh = sum(255 << (8 * k) for k in range(4) if k not in live or not np.isnan(hi[k]))
    wl = wh = 0
    for k in range(4):
        if k not in live:
            wl |= 255 << (8 * k)
    if not ext > 0:
        assert ext == 0, "the inputs hold no inverted box among the non-empty slots"
        return int(org.view(np.uint32)), int(MIN_NORMAL.view(np.uint32)), wl, wh, ml, mh
    ext_q = F(float(ext))
    e = math.frexp(float(ext) / 254.0)[1]
    while 254 * F(2) ** e < ext_q:
        e += 1
    while 254 * F(2) ** (e - 1) >= ext_q:
        e -= 1
    e = max(e, -149)
    org_q = F(float(org))
    for doubled in range(4):
        if e + doubled > 127:
            return None
        s = F(2) ** (e + doubled)
        qlows, qhighs = [], []
        for k in live:
            # (a low plane at +inf, a high plane at -inf -- an inverted box -- take the last q that holds: 255, 0)
            qlows.append(0 if np.isnan(lo[k]) else 255 if np.isposinf(lo[k]) else min(255, math.floor((F(float(lo[k])) - org_q) / s)))
            qhighs.append(0 if np.isnan(hi[k]) or np.isneginf(hi[k]) else max(0, math.ceil((F(float(hi[k])) - org_q) / s)))
        if max(qhighs) <= 255:
            break
    else:
        return None
    for k, ql, qh in zip(live, qlows, qhighs):
        assert 0 <= ql <= 255
        # the two rules, stated: q fits and the next looser one does not
        if np.isfinite(lo[k]):
            assert org_q + ql * s <= F(float(lo[k])) and (ql == 255 or org_q + (ql + 1) * s > F(float(lo[k])))
        if np.isfinite(hi[k]):
            assert org_q + qh * s >= F(float(hi[k])) and (qh == 0 or org_q + (qh - 1) * s < F(float(hi[k])))
        wl |= ql << (8 * k)
        wh |= qh << (8 * k)
    scale = f32(float(s))
    assert F(float(scale)) == s
    return int(org.view(np.uint32)), int(scale.view(np.uint32)), wl, wh, ml, mh


def ref_order(box, child):
    """The four order words. box float32 [3, 2, 4]."""
    with np.errstate(all="ignore"):
        c = box[:, 0, :] + box[:, 1, :]                          # float32 [3, 4]
        words = [0, 0, 0, 0]
        for o in range(8):
            sx, sy, sz = (c[a] if not (o >> a) & 1 else -c[a] for a in range(3))
            key = (sx + sy) + sz
            assert key.dtype == np.float32
            key = [math.inf if (child[k] == NONE or np.isnan(key[k])) else float(key[k]) for k in range(4)]
            perm = sorted(range(4), key=lambda k: (key[k], k))
            word = 0
            for pos, k in enumerate(perm):
                word |= k << (2 * pos)
            rank = {k: pos for pos, k in enumerate(perm)}
            for bit, (i, j) in enumerate(((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))):
                if rank[j] < rank[i]:
                    word |= 1 << (8 + bit)
            words[o >> 1] |= word << (16 * (o & 1))
    return words


def ref_bound(box, child):
    b = f32(0)
    for k in range(4):
        if child[k] == NONE:
            continue
        for v in box[:, :, k].reshape(-1):
            if not abs(v) <= f32(3.0e38):
                return f32(np.inf)
            b = max(b, abs(v))
    return f32(b)


def ref_node(box, child):
    live = [k for k in range(4) if child[k] != NONE]
    axes = [ref_axis(box[a, 0], box[a, 1], live) for a in range(3)]
    return dict(axes=axes, misfit=any(x is None for x in axes), order=ref_order(box, child), bound=ref_bound(box, child))


# ---------------------------------------------------------------------------------------------- running the header

@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """Built against rtk_node_finish.h and rtk_node.h alone (no HIP include path), flags as for the other rule drivers."""
    exe = str(tmp_path_factory.mktemp("node_finish") / "node_finish_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-mfma", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "rtk_amd", "csrc"), os.path.join(ROOT, "tests", "node_finish_driver.cpp"), "-o", exe])
    return exe


def run_driver(exe, nodes):
    """nodes: [(box float32 [3, 2, 4], child [4])] -> uint32 [n, 22]: 16 words of DevNodeQ, 4 order words, misfit, bound bits."""
    text = "".join(" ".join("%x" % w for w in np.ascontiguousarray(box, np.float32).view(np.uint32).reshape(-1)) + " " +
                   " ".join("%x" % c for c in child) + "\n" for box, child in nodes)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    assert lines[len(nodes)] == "ok"
    return np.array([[int(w, 16) for w in line.split()] for line in lines[:len(nodes)]], np.uint64).astype(np.uint32)


def check(exe, nodes, what):
    """Every node through the header and the reference; returns the references (for the tests' own claims about their inputs)."""
    got = run_driver(exe, nodes)
    refs = []
    for i, (box, child) in enumerate(nodes):
        box = np.ascontiguousarray(box, np.float32)
        ref = ref_node(box, child)
        refs.append(ref)
        g = got[i]
        where = "%s: node %d %s %s" % (what, i, box.tolist(), ["%x" % c for c in child])
        assert [int(x) for x in g[16:20]] == ref["order"], where + " order %s" % [hex(int(x)) for x in g[16:20]]
        gb, wb = g[21:22].view(np.float32)[0], ref["bound"]
        assert (np.isnan(gb) and np.isnan(wb)) or int(g[21]) == int(wb.view(np.uint32)), where + " bound"
        assert [int(x) for x in g[12:16]] == list(child), where + " child words"
        assert int(g[20]) == (1 if ref["misfit"] else 0), where + " misfit flag %d" % int(g[20])
        if ref["misfit"]:
            continue
        for a in range(3):
            org, scale, wl, wh, ml, mh = ref["axes"][a]
            have = (int(g[a]), int(g[3 + a]), int(g[6 + 2 * a]) & ml, int(g[7 + 2 * a]) & mh)
            assert have == (org, scale, wl, wh), where + " axis %d: got org %08x scale %08x low %08x high %08x, want %08x %08x %08x %08x" % ((a,) + have + (org, scale, wl, wh))
    return refs


# ---------------------------------------------------------------------------------------------- inputs

def node_of(lo, hi, empty=()):
    """lo, hi [4][3] (slot, axis) -> (box float32 [3, 2, 4], child words): leaves at slots 0, 7, 14, 21; `empty` slots carry +1 / -1."""
    lo, hi = np.array(lo, np.float32).reshape(4, 3).copy(), np.array(hi, np.float32).reshape(4, 3).copy()
    child = [LEAF | (7 * k) for k in range(4)]
    for k in empty:
        lo[k], hi[k], child[k] = 1.0, -1.0, NONE
    box = np.stack([lo.T, hi.T], axis=1)                             # [axis, min|max, slot]
    return np.ascontiguousarray(box, np.float32), child


def step(x, n):
    """x moved by n float32 steps (n may be negative)."""
    x = f32(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, f32(np.inf if n > 0 else -np.inf))
    return x


def one_axis(org, planes):
    """A node whose four children have the given (lo, hi) on x, offsets from nothing: absolute values; y and z are plain."""
    lo = [[p[0], 0.0, -1.0] for p in planes]
    hi = [[p[1], 1.0 + k, 2.0] for k, p in enumerate(planes)]
    return node_of(lo, hi)


def random_nodes(rng, n, kmin, kmax):
    out = []
    for _ in range(n):
        k = rng.randint(kmin, kmax + 1)
        S = 2.0 ** k
        centre = S * rng.uniform(-4, 4, 3) * rng.choice([0.0, 1.0, 64.0])
        lo = centre + S * rng.uniform(0, 1, (4, 3))
        hi = lo + S * rng.uniform(0, 1, (4, 3)) * rng.choice([1.0, 1e-3], (4, 1))
        with np.errstate(all="ignore"):
            lo32, hi32 = lo.astype(np.float32), hi.astype(np.float32)
        hi32 = np.maximum(hi32, lo32)
        empty = list(rng.choice(4, rng.choice([0, 0, 1, 2, 3]), replace=False))
        out.append(node_of(lo32, hi32, empty))
    return out


def test_header_includes_no_hip():
    text = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_node_finish.h")).read()
    assert [l.split()[1] for l in text.splitlines() if l.startswith("#include")] == ['"rtk_node.h"', "<math.h>"]
    node = open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_node.h")).read()
    assert [l.split()[1] for l in node.splitlines() if l.startswith("#include")] == ["<stdint.h>"]
    assert '#include "rtk_node.h"' in open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_dev.h")).read()
    assert "rtk_node.h" in open(os.path.join(ROOT, "rtk_amd", "csrc", "Makefile")).read()


def test_reference_refuses_a_looser_or_coarser_node():
    """The reference can fail: it is exact about tightness and about the scale (what the validator's containment check cannot see)."""
    box, child = node_of([[0, 0, 0], [1, 1, 1], [2, 2, 2], [3, 3, 3]], [[1, 1, 1], [2, 2, 2], [3, 3, 3], [4, 4, 4]])
    org, scale, wl, wh, ml, mh = ref_node(box, child)["axes"][0]
    assert ml == mh == 0xFFFFFFFF
    assert f32(0).view(np.uint32) == org and f32(2.0 ** -5).view(np.uint32) == scale         # 254 / 64 < 4 <= 254 / 32
    assert wl == (0 | 32 << 8 | 64 << 16 | 96 << 24) and wh == (32 | 64 << 8 | 96 << 16 | 128 << 24)


def test_random_nodes(driver):
    rng = np.random.RandomState(20250117)
    nodes = random_nodes(rng, 1200, -20, 20) + random_nodes(rng, 600, -120, 120)
    refs = check(driver, nodes, "random")
    assert sum(r["misfit"] for r in refs) == 0
    assert len({tuple(r["order"]) for r in refs}) > 300


def test_extents_around_the_grid_step_thresholds(driver):
    """Extents at 2^k, 254 * 2^k, 256 * 2^k and one float step either side (the correction branch of grid_step), with org 0, an
    org of the extent's size and a far org; high planes at q = 254, 255, 256 of the scale an extent of 254 * 2^k gets, and a step
    either side of each (the retry loop)."""
    nodes = []
    for k in list(range(-140, 121, 9)) + [-149, -148, -141, -127, -126, -125, 0, 119, 120]:
        for mult in (1.0, 254.0, 256.0):
            for d in (-1, 0, 1):
                with np.errstate(all="ignore"):
                    ext = step(f32(mult) * f32(2.0 ** k), d)
                if not np.isfinite(ext) or not ext > 0:
                    continue
                with np.errstate(all="ignore"):
                    orgs = (f32(0), ext, -ext * f32(3), f32(-1.5) * ext * f32(1024))
                for org in orgs:
                    with np.errstate(all="ignore"):
                        top = org + ext
                    if not np.isfinite(top) or not np.isfinite(org) or not np.isfinite(top - org):
                        continue
                    mid = org + ext * f32(0.37)
                    nodes.append(one_axis(org, [(org, mid), (mid, top), (org, org), (top, top)]))
        s = f32(2.0 ** k)
        with np.errstate(all="ignore"):
            orgs = (f32(0), s * f32(1024), -s * f32(77.5))
        for org in orgs:
            for q in (254, 255, 256):
                for d in (-1, 0, 1):
                    with np.errstate(all="ignore"):
                        top = step(org + f32(q) * s, d)
                        lowish = step(org + f32(q - 1) * s, d)
                        wide = top - org
                    if not (np.isfinite(top) and np.isfinite(org) and top > org and np.isfinite(wide)):
                        continue
                    nodes.append(one_axis(org, [(org, top), (lowish, top), (org, lowish), (lowish, lowish)]))
        # fl(max - min) rounds DOWN to 254 * s: the true extent needs q = 255 at the scale the rounded one gets
        if -120 <= k <= 100:
            org = -s * f32(2.0 ** -30)
            nodes.append(one_axis(org, [(org, f32(254) * s), (f32(0), f32(253) * s), (org, org), (s, step(s, 1))]))
    refs = check(driver, nodes, "thresholds")
    assert len(nodes) > 1000 and [i for i, r in enumerate(refs) if r["misfit"]] == []
    highs = [(r["axes"][0][3] >> (8 * k)) & 255 for r in refs for k in range(4)]
    assert 255 in highs and 254 in highs and 128 in highs


def test_far_away_and_tiny_scenes(driver):
    """Boxes at 1e4 with detail 0.5 -- one float step of org is larger than the scale, so every plane is a whole number of steps of
    org's own spacing and the bytes must still be tight -- and a scene 1e-6 wide."""
    rng = np.random.RandomState(5)
    nodes = []
    ulp = f32(2.0 ** -10)                                            # of a float near 1e4
    for _ in range(300):
        org = f32(1e4) + ulp * f32(rng.randint(-2000, 2000))
        lo = org + ulp * rng.randint(0, 30, (4, 3)).astype(np.float32)
        hi = lo + ulp * rng.randint(0, 30, (4, 3)).astype(np.float32)
        lo[0] = org
        nodes.append(node_of(lo, hi, list(rng.choice(4, rng.choice([0, 1]), replace=False) + 0) if rng.rand() < 0.3 else ()))
    for _ in range(150):
        lo = f32(1e4) + (rng.uniform(-50, 50, (4, 3))).astype(np.float32)
        hi = lo + rng.uniform(0, 0.5, (4, 3)).astype(np.float32)
        nodes.append(node_of(lo, hi))
    for _ in range(300):
        lo = (rng.uniform(0, 1e-6, (4, 3))).astype(np.float32)
        hi = np.minimum(lo + rng.uniform(0, 3e-7, (4, 3)).astype(np.float32), f32(1e-6))
        nodes.append(node_of(lo, np.maximum(lo, hi)))
    refs = check(driver, nodes, "far and tiny")
    far = [r for r in refs[:300] if r["axes"][0][1] < int(ulp.view(np.uint32))]
    assert len(far) > 100 and sum(r["misfit"] for r in refs) == 0


def test_denormal_extents(driver):
    """Extents below 2^-126: the scale has no finite reciprocal and the header divides; down to the smallest float, whose scale is
    itself (no smaller power of two exists)."""
    rng = np.random.RandomState(6)
    tiny = f32(2.0 ** -149)
    nodes = []
    for base in (f32(0), f32(2.0 ** -126), -f32(2.0 ** -126), f32(2.0 ** -125)):
        for top in [1, 2, 3, 7, 8, 254, 255, 256, 257, 1000, 65535, 1 << 20, (1 << 22) + 5, (1 << 23) - 1]:
            for _ in range(4):
                a = np.sort(rng.randint(0, top + 1, (4, 3, 2)), axis=2)
                a[0, :, 0], a[1, :, 1] = 0, top
                a[1, :, 0] = np.minimum(a[1, :, 0], top)
                lo, hi = base + tiny * a[:, :, 0].astype(np.float32), base + tiny * a[:, :, 1].astype(np.float32)
                nodes.append(node_of(lo, hi))
    refs = check(driver, nodes, "denormal extents")
    assert sum(r["misfit"] for r in refs) == 0
    assert min(r["axes"][0][1] for r in refs) == int(tiny.view(np.uint32))


def test_points_flats_zeros_and_empties(driver):
    inf, nan, big = f32(np.inf), f32(np.nan), f32(3.0e38)
    p = [[1.5, -2.0, 3.0]] * 4
    nodes = [
        node_of(p, p), node_of(p, p, (1, 2, 3)), node_of(p, p, (0, 1, 2, 3)),                                # point boxes; no child at all
        node_of([[0, 0, 0]] * 4, [[1, 0, 2], [2, 0, 3], [3, 0, 0], [4, 0, 1]]),                          # a flat axis
        node_of([[-0.0, -0.0, -0.0]] * 4, [[-0.0, 1.0, 0.0]] * 4),                                       # -0 as org, as a high plane
        node_of([[-0.0, -1.0, 0.0]] * 4, [[1.0, -0.0, -0.0]] * 4, (3,)),
        node_of([[-1.0, -1.0, -1.0], [-0.0, -0.0, -0.0], [0.5, 0.5, 0.5], [0.0, 0.0, 0.0]], [[-0.0, -0.0, -0.0], [1.0, 1.0, 1.0], [0.5, 0.5, 0.5], [0.0, 0.0, 0.0]]),
    ]
    for empty in ((0,), (3,), (1, 2), (0, 3), (0, 1, 2), (1, 2, 3), (0, 1, 2, 3)):
        nodes.append(node_of([[0, 0, 0], [1, 2, 3], [-4, 5, 6], [7, -8, 9]], [[1, 1, 1], [3, 3, 4], [-3, 7, 6.5], [7.25, -7, 10]], empty))
    refs = check(driver, nodes, "points, flats, zeros, empties")
    assert sum(r["misfit"] for r in refs) == 0
    assert refs[2]["axes"][0][:4] == (0, int(MIN_NORMAL.view(np.uint32)), 0xFFFFFFFF, 0)
    assert refs[4]["axes"][0][0] == 0x80000000 and refs[3]["axes"][1][1] == int(MIN_NORMAL.view(np.uint32))
    # planes that are not finite, extents that are not: a misfit, and no bound
    base_lo, base_hi = [[0, 0, 0], [1, 2, 3], [-4, 5, 6], [7, -8, 9]], [[1, 1, 1], [3, 3, 4], [-3, 7, 6.5], [7.25, -7, 10]]
    bad = []
    for value in (inf, -inf, nan):
        for slot in (0, 2, 3):
            for axis in range(3):
                for which in (0, 1):
                    lo, hi = np.array(base_lo, np.float32), np.array(base_hi, np.float32)
                    (lo, hi)[which][slot, axis] = value
                    bad.append(node_of(lo, hi))
    lo, hi = np.array(base_lo, np.float32), np.array(base_hi, np.float32)
    lo[:, 1], hi[:, 1] = nan, nan
    bad.append(node_of(lo, hi))
    lo, hi = np.array(base_lo, np.float32), np.array(base_hi, np.float32)
    lo[1, 0], hi[2, 0] = -big, big                                                                        # an extent of 6e38
    bad.append(node_of(lo, hi))
    lo, hi = np.array(base_lo, np.float32), np.array(base_hi, np.float32)
    lo[1, 2], hi[1, 2] = f32(-3.3e38), f32(-3.2e38)                                                       # finite, beyond 3e38: fits, no bound
    beyond = node_of(lo, hi)
    want = [(value == inf and which == 1) or (value == -inf and which == 0)
            for value in (inf, -inf, nan) for slot in (0, 2, 3) for axis in range(3) for which in (0, 1)] + [False, True, False]
    refs = check(driver, bad + [beyond], "not finite")
    assert [r["misfit"] for r in refs] == want
    assert all(np.isinf(r["bound"]) for r in refs[:-2] + refs[-1:]) and refs[-2]["bound"] == big
    # a non-finite plane in an EMPTY slot is nobody's: the node fits and has a bound
    lo, hi = np.array(base_lo, np.float32), np.array(base_hi, np.float32)
    box, child = node_of(lo, hi, (2,))
    box[0, 0, 2], box[1, 1, 2] = nan, inf
    refs = check(driver, [(box, child)], "junk in an empty slot")
    assert not refs[0]["misfit"] and refs[0]["bound"] == f32(10)


def test_equal_centres_and_order_ties(driver):
    """Equal centres in some or all octants: ties go to the lower slot, empty slots last whatever they hold, keys that overflow
    to inf or cancel to NaN last as well."""
    big = f32(3.0e38)
    nodes = [
        node_of([[0, 0, 0]] * 4, [[1, 1, 1]] * 4),                                                       # all equal
        node_of([[0, 0, 0]] * 4, [[1, 1, 1]] * 4, (1,)),
        node_of([[0, 0, 0], [1, -1, 0], [-1, 1, 0], [0, 0, 1]], [[1, 1, 1], [2, 0, 1], [0, 2, 1], [1, 1, 2]]),   # equal along x+y, not along x-y
        node_of([[0, 0, 0], [2, 0, 0], [0, 2, 0], [0, 0, 2]], [[1, 1, 1], [3, 1, 1], [1, 3, 1], [1, 1, 3]]),     # three equal in octant 0
        node_of([[3, 0, 0], [2, 0, 0], [1, 0, 0], [0, 0, 0]], [[4, 1, 1], [3, 1, 1], [2, 1, 1], [1, 1, 1]]),     # reversed
        node_of([[3, 0, 0], [2, 0, 0], [1, 0, 0], [0, 0, 0]], [[4, 1, 1], [3, 1, 1], [2, 1, 1], [1, 1, 1]], (0, 2)),
        node_of([[big, 0, 0], [0, 0, 0], [-big, 0, 0], [1, 0, 0]], [[big, 1, 1], [1, 1, 1], [-big, 1, 1], [2, 1, 1]]),   # lo + hi = +-inf
        node_of([[big, -big, 0], [0, 0, 0], [big, big, 0], [1, 0, 0]], [[big, -big, 1], [1, 1, 1], [big, big, 1], [2, 1, 1]]),  # inf - inf = NaN in half the octants
    ]
    rng = np.random.RandomState(9)
    for _ in range(300):                                                                                 # centres on a coarse grid: many ties
        c = rng.randint(-2, 3, (4, 3)).astype(np.float32)
        h = rng.randint(0, 2, (4, 3)).astype(np.float32)
        nodes.append(node_of(c - h, c + h, list(rng.choice(4, rng.choice([0, 0, 1, 2]), replace=False))))
    refs = check(driver, nodes, "ties")
    assert refs[0]["order"] == [0x00E400E4] * 4                                                          # identity, no pair bit
    assert refs[4]["order"][0] & 0xFFFF == 0x3F1B and refs[4]["order"][0] >> 16 == 0x00E4               # +x: 3 2 1 0, every pair swapped; -x: identity
