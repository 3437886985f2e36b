"""Batches longer than one pass of a resident grid (numpy only). The query kernels launch num_cus x blocks_per_cu workgroups of
BLOCK lanes and every lane steps through the batch; a pass can never exceed the lanes a CU holds at once -- 8 waves per SIMD x
4 SIMDs x 64 lanes = 2048 ("Up to 32 waves/CU -- i.e. up to 8 waves/SIMD", the CU section of the MI355X microarchitecture notes)
-- times the CUs. batch_size(cus) is two such passes, five waves and 37: whatever the residency, every kernel makes two whole
passes and a ragged third, and the batch ends inside a wave.

The reference of such a batch is brute force on a mix of L queries, L a prime that divides no pass size, repeated to N rows:
records, points and flags tile by row (tile_rows), fill buffers are periodic with the period sum(counts) and end in a partial
tail (Tiled). family(name) gives a family's own mix on the 300-triangle soup of its GPU test file, cut to L rows by choose() and
answered by that file's brute force; conditions() asserts from the reference alone that stale state would change an answer."""
import importlib

import numpy as np

from rtk_amd import synth

F = np.float32
NONE = 0xFFFFFFFF
FILL = 0x7e7e7e7e
LANES_PER_CU = 8 * 4 * 64                    # waves per SIMD x SIMDs x lanes
BLOCK = 256                                  # lanes of a workgroup of every resident-grid kernel (CL_THREADS, WI_THREADS, ...)
RESIDENCIES = range(1, LANES_PER_CU // BLOCK + 1)       # workgroups per CU: 1 .. 8
SWEEPS = {"sphere": ("tests.test_gpu_sweep", "tests.sweep_ref"), "boxsweep": ("tests.test_gpu_boxsweep", "tests.boxsweep_ref"),
          "capsule": ("tests.test_gpu_capsule", "tests.capsule_ref"), "obbsweep": ("tests.test_gpu_obbsweep", "tests.obbsweep_ref")}
COUNTED = ("within", "box", "obb", "touch", "near")     # a count form and a fill form
CLOSEST = ("closest", "pair", "sign") + tuple(SWEEPS)   # one answer per slot
FAMILIES = CLOSEST[:1] + COUNTED + CLOSEST[1:]


def batch_size(cus):
    return 2 * LANES_PER_CU * cus + 64 * 5 + 37


def pass_sizes(cus):
    """the lanes of one pass at every residency a workgroup of BLOCK lanes can have"""
    return [cus * r * BLOCK for r in RESIDENCIES]


def mix_length(cus, about=1000):
    """the largest prime <= about that does not divide the CU count: coprime to 64 and, being larger than 8, to every pass size"""
    for n in range(about, 8, -1):
        if all(n % k for k in range(2, int(n ** 0.5) + 1)) and cus % n:
            return n
    raise ValueError(about)


def tile_rows(a, n):
    """row i of the result is row i mod len(a)"""
    return np.ascontiguousarray(a[np.arange(n) % len(a)])


class Tiled:
    """The fill form's buffers for the mix repeated to n slots, each slot with exactly the room of its count: offsets [n + 1],
    total, and fill(period) for a buffer whose period is the mix's concatenated lists."""

    def __init__(self, counts, n):
        counts = np.asarray(counts, np.int64)
        L, self.n = len(counts), n
        off = np.concatenate([[0], np.cumsum(counts)])
        self.period = int(off[-1])
        i = np.arange(n + 1)
        self.offsets = (i // L) * self.period + off[i % L]
        self.total = int(self.offsets[-1])
        self.counts = counts[np.arange(n) % L]

    def fill(self, period, tail=0, listed=None):
        """period: [sum(counts), ...]. -> [total + tail, ...]: the lists in slot order, 0x7e in the tail and in the segments of
        slots that are not listed"""
        period = np.asarray(period)
        assert len(period) == self.period
        out = np.full((self.total + tail,) + period.shape[1:], FILL, np.uint32)
        if self.period:
            out[:self.total] = period.view(np.uint32)[np.arange(self.total) % self.period]
        if listed is not None:
            out[:self.total][~np.repeat(np.asarray(listed, bool), self.counts)] = FILL
        return out

    def written(self, tail=0, listed=None):
        out = np.full(self.n + tail, FILL, np.uint32)
        out[:self.n] = self.counts
        if listed is not None:
            out[:self.n][~np.asarray(listed, bool)] = FILL
        return out


def slots(want, n, tail=0, listed=None):
    """a per-slot output [L, ...] tiled to n rows with 0x7e in the tail and in the slots that are not listed"""
    fill = FILL if want.dtype.itemsize == 4 else 0x7e               # (words, or the bytes of an any-hit form)
    out = np.full((n + tail,) + want.shape[1:], fill, want.dtype)
    out[:n] = tile_rows(want, n)
    if listed is not None:
        out[:n][~np.asarray(listed, bool)] = fill
    return out


def conditions(name, live, key, cus):
    """From the reference alone. key: the count, or 1 for a hit. 20 % of the live queries hit; 10 % of all are dead or miss; and
    at every pass size s a quarter of the positions j differ from (j + s) mod L in hit versus miss or in count -- consecutive
    steps of a lane differ, so state kept from one step to the next changes an answer."""
    key = np.asarray(key, np.int64)
    L = len(key)
    hit = key > 0
    assert not hit[~live].any(), name
    share, empty = float(hit[live].mean()), float((~hit).mean())
    differ = steps_differ(key, cus)
    print("%-9s L %d, live %d, hit %.0f %% of live, dead or miss %.0f %%, steps that differ %.0f .. %.0f %%, mean key %.2f"
          % (name, L, live.sum(), 100 * share, 100 * empty, 100 * min(differ), 100 * max(differ), key.mean()))
    assert all(L % 2 and s % L for s in pass_sizes(cus)), (name, L)
    assert share >= 0.2 and empty >= 0.1 and min(differ) >= 0.25, (name, share, empty, differ)


def choose(key, L, seed, cap=8, long_lists=24):
    """L rows of a mix, shuffled: `long_lists` of the rows whose key is above the cap (a fill of a million slots stays a few
    million entries), the rest hits and misses as near half and half as the mix allows"""
    rng = np.random.RandomState(seed)
    key = np.asarray(key, np.int64)
    assert len(key) >= L
    cap = max(cap, int(np.sort(key)[L - long_lists - 1]))
    order = rng.permutation(len(key))
    large, small = order[key[order] > cap][:long_lists], order[key[order] <= cap]
    need = L - len(large)
    hits, miss = small[key[small] > 0], small[key[small] == 0]
    m = min(len(miss), max(need - len(hits), need // 2))
    assert need - m <= len(hits)
    if key[hits[:need - m]].sum() > 8 * L:
        hits = hits[np.argsort(key[hits], kind="stable")]           # too many entries: the shortest lists first
    return rng.permutation(np.concatenate([large, hits[:need - m], miss[:m]]))


def soup():
    """the base scene of every family's GPU test file"""
    return synth.triangle_soup(300, 0.2, seed=5)


def _cat(parts, width):
    parts = [np.asarray(p, np.uint32).reshape((-1,) + width) for p in parts]
    return np.concatenate(parts) if parts else np.zeros((0,) + width, np.uint32)


class Answer:
    """rows: the per-slot outputs [n, ...] as words; counts and fills (the concatenated lists) where the family has lists;
    key and live for conditions()"""

    def __init__(self, live, rows=(), counts=None, fills=()):
        self.live, self.rows, self.counts, self.fills = np.asarray(live, bool), tuple(rows), counts, tuple(fills)
        self.key = np.asarray(counts, np.int64) if counts is not None else (self.rows[0][:, 3] != NONE).astype(np.int64)


def brute(name, tris, inputs, room=None):
    """the family's own brute force over tris [T, 3, 3] -> Answer (within: the fills cut to `room` entries per query)"""
    T = len(tris)
    prims = np.arange(T, dtype=np.uint32)
    assert len(inputs[0]) * T <= 500000, (name, len(inputs[0]), T)
    with np.errstate(all="ignore"):
        if name in ("closest", "sign"):
            q, = inputs
            live = np.isfinite(q["point"]).all(1) & (q["max_dist2"] > 0)
            if name == "closest":
                from tests.closest_ref import brute_force
                return Answer(live, brute_force(tris, prims, q["point"], q["max_dist2"]))
            from tests.sign_ref import signed_np, table_np
            sg, rec, pts, _, _ = signed_np(tris, table_np(tris)[0], q["point"], q["max_dist2"])
            return Answer(live, (rec, pts, np.ascontiguousarray(sg, F).view(np.uint32)))
        if name == "within":
            from tests.within_ref import brute_force_within
            q, = inputs
            ref = brute_force_within(tris, prims, q["point"], q["max_dist2"])
            live = np.isfinite(q["point"]).all(1) & (q["max_dist2"] > 0)
            a = Answer(live, (), ref.counts, (_cat([r[:room] for r, _ in ref.lists], (4,)), _cat([p[:room] for _, p in ref.lists], (3,))))
            a.kept = np.minimum(ref.counts, room if room is not None else ref.counts)      # entries a segment of `room` keeps
            return a
        if name == "box":
            from tests.box_ref import brute_force_boxes, live_np
            q, = inputs
            ref = brute_force_boxes(tris, prims, q["lo"], q["hi"])
            return Answer(live_np(q["lo"], q["hi"]), (), ref.counts, (_cat(ref.lists, ()),))
        if name == "obb":
            from tests.obb_ref import brute_force_obbs, live_np
            q, = inputs
            ref = brute_force_obbs(tris, prims, q)
            return Answer(live_np(np.ascontiguousarray(q).view(F).reshape(-1, 15)), (), ref.counts, (_cat(ref.lists, ()),))
        if name == "touch":
            from tests.touch_ref import brute_force_touching
            q, = inputs
            ref = brute_force_touching(tris, prims, q)
            return Answer(np.isfinite(q).all((1, 2)), (), ref.counts, (_cat(ref.lists, ()),))
        if name in ("pair", "near"):
            q, max2 = inputs
            live = np.isfinite(q).all((1, 2)) & (max2 > 0)
            if name == "pair":
                from tests.pair_ref import brute_force_pairs
                return Answer(live, brute_force_pairs(tris, prims, q, max2))
            from tests.near_ref import brute_force_near
            ref = brute_force_near(tris, prims, q, max2)
            return Answer(live, (), ref.counts, tuple(_cat([k[j] for k in ref.kept], (w,)) for j, w in enumerate((4, 3, 3))))
        s, = inputs
        from tests import hostile_scenes as H
        kind = {"boxsweep": "box", "obbsweep": "obb"}.get(name, name)
        return Answer(H.sweep_live(kind, s), importlib.import_module(SWEEPS[name][1]).brute_force(tris, prims, s))


def own_mix(name, tris):
    """the whole mix of the family's GPU test file, as the tuple of arrays its calls take"""
    with np.errstate(all="ignore"):
        if name in ("closest", "sign"):
            from tests.test_gpu_closest import query_mix
            return (query_mix(tris),)
        if name == "within":
            from tests.test_gpu_within import within_mix
            return (within_mix(tris),)
        if name == "box":
            from tests.test_gpu_box import box_mix
            return (box_mix(tris),)
        if name == "obb":
            from tests.test_gpu_obb import obb_mix
            return (obb_mix(tris)[0],)
        from tests.touch_ref import mix_slices, query_mix
        if name == "touch":
            return (query_mix(tris),)
        if name in ("pair", "near"):
            from tests.test_gpu_pair import limits
            mix, huge = query_mix(tris), mix_slices()["huge and degenerate on purpose"]
            q = np.concatenate([mix[:huge.start], mix[huge.stop:]])
            max2 = limits(np.random.RandomState(3), len(q), 0.2)
            if name == "near":
                # (a query without a limit lists the whole scene and the file draws every fourth so: here 12 of them stay, the
                # others get the file's second limit, and a fill of a million slots stays a few million entries)
                from rtk_amd.types import RTK_INF
                max2[np.nonzero(max2 == RTK_INF)[0][12:]] = F(0.1 * 0.2) ** 2
            return q, max2
        mix = importlib.import_module(SWEEPS[name][0]).sweep_mix(tris)
        return (np.ascontiguousarray(mix[0] if isinstance(mix, tuple) else mix, F),)


class Family:
    pass


_FAMILIES = {}


def family(name, cus=256):
    """The family's mix on the soup cut to mix_length(cus) rows, with its brute-force Answer (computed once and shared). The cut
    is decided by the brute force of the whole mix where that stays under the pair limit, else of its first 1600 rows."""
    if (name, cus) not in _FAMILIES:
        f = Family()
        f.name, f.tris = name, soup().reshape(-1, 3, 3)
        f.L = mix_length(cus)
        mix = tuple(x[:500000 // len(f.tris)] for x in own_mix(name, f.tris))
        whole = brute(name, f.tris, mix)
        pick = cut(whole.key, f.L, cus)
        f.inputs = tuple(np.ascontiguousarray(x[pick]) for x in mix)
        f.answer = brute(name, f.tris, f.inputs)
        assert (f.answer.key == whole.key[pick]).all()
        _FAMILIES[(name, cus)] = f
    return _FAMILIES[(name, cus)]


def steps_differ(key, cus):
    """per pass size s: the share of positions j whose key differs from that of (j + s) mod L"""
    key = np.asarray(key)
    return [float((key != key[(np.arange(len(key)) + s) % len(key)]).mean()) for s in pass_sizes(cus)]


def cut(key, L, cus):
    """the rows of a mix that choose() picks, under the first seed at which a quarter of the consecutive steps of a lane differ
    at every pass size; no such seed is an error"""
    for seed in range(16):
        pick = choose(key, L, seed)
        if min(steps_differ(np.asarray(key, np.int64)[pick], cus)) >= 0.25:
            return pick
    raise AssertionError("no cut of the mix makes consecutive steps differ")


def allhits_mix(oracle, blob, mesh_base, cus=256):
    """All hits has no numpy brute force: its reference is the oracle's reject-all lists (tests/allhits_ref.py) on a blob of the
    soup. -> (rays [L], their lists): the rays tests/test_gpu_queries_hostile_scenes.py sends through a scene, cut by cut()"""
    from tests import allhits_ref as R, hostile_scenes as H
    rays = H.adversarial_rays(soup().reshape(-1, 3, 3), 1600)
    rays = rays[cut(R.oracle_lists(oracle, blob, rays, mesh_base).counts, mix_length(cus), cus)]
    return rays, R.oracle_lists(oracle, blob, rays, mesh_base)


def winding_mix(cus=256):
    """-> (points [L, 3] kept 5 % of the soup's size away from every triangle, their float64 winding numbers, the largest
    |brute32 - brute64| on them)"""
    from tests.winding_ref import brute32, brute64, query_points
    tris = soup().reshape(-1, 3, 3)
    pts = query_points(tris, float((tris.reshape(-1, 3).max(0) - tris.reshape(-1, 3).min(0)).max()), mix_length(cus), 90)
    w64 = brute64(tris, pts)
    return pts, w64, float(np.abs(brute32(tris, pts).astype(np.float64) - w64).max())


def deep_mix(deep, shallow, L):
    """[L] rows: every seventh a row of `deep` (in turn), the others rows of `shallow` (in turn): a lane alternates deep and
    shallow walks, and the batch stays cheap"""
    i = np.arange(L)
    return np.ascontiguousarray(np.concatenate([deep, shallow])[np.where(i % 7 == 0, (i // 7) % len(deep), len(deep) + i % len(shallow))])
