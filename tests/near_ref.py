"""The rule of rtk_amd/csrc/rtk_near_rule.h restated in numpy float32 on top of tests/pair_ref.py and tests/touch_ref.py (imported,
not copied), for tests/test_near_cpu.py (against the header's driver) and tests/test_gpu_near.py (against the kernel): per query
the count of its candidates and the first `room` entries of its list in ascending (dist2, prim) order -- record words plus the
words of both points."""
import numpy as np

from tests.pair_ref import SKIP_SHARED_VERTEX, pair_np
from tests.touch_ref import live_np, shares_vertex_np

F = np.float32


class Near:
    """counts uint32 [Q]; kept[i] = (record words uint32 [k_i, 4] -- dist2, u, v, prim --, words of the points on the query
    uint32 [k_i, 3], words of the points on the scene uint32 [k_i, 3]), ascending in (dist2, prim), k_i = min(count_i, room_i)
    (the whole list without room)"""

    def __init__(self, counts, kept):
        self.counts, self.kept = counts, kept

    def written(self):
        return np.array([len(k[0]) for k in self.kept], np.uint32)

    def cut(self, k):
        return Near(self.counts, [tuple(x[:k] for x in e) for e in self.kept])


def brute_force_near(tris, prims, queries, max2=None, first_prim=None, flags=0, room=None, chunk=200000):
    """tris [T, 3, 3] float32 with ids prims [T], queries [Q, 3, 3] (or [Q, 9]), max2 None (RTK_INF) or [Q], first_prim None or
    [Q], room None or [Q] -> Near. A candidate: a live query, max2 > 0, prim >= first_prim, no shared vertex position under the
    flag, dist2 < max2 (a NaN dist2 is none)."""
    from rtk_amd.types import RTK_INF
    tris = np.ascontiguousarray(tris, F).reshape(-1, 3, 3)
    prims = np.asarray(prims, np.uint32)
    queries = np.ascontiguousarray(queries, F).reshape(-1, 3, 3)
    Q, T = len(queries), len(tris)
    max2 = np.full(Q, RTK_INF, F) if max2 is None else np.ascontiguousarray(max2, F)
    first = np.zeros(Q, np.uint32) if first_prim is None else np.asarray(first_prim, np.uint32)
    empty = (np.zeros((0, 4), np.uint32), np.zeros((0, 3), np.uint32), np.zeros((0, 3), np.uint32))
    counts = np.zeros(Q, np.uint32)
    kept = [empty] * Q
    if T == 0 or Q == 0:
        return Near(counts, kept)
    rows = max(1, chunk // T)
    for at in range(0, Q, rows):
        sl = slice(at, min(at + rows, Q))
        a = queries[sl]
        r = pair_np(a[:, None], tris[None])
        with np.errstate(invalid="ignore"):
            ok = (live_np(a) & (max2[sl] > 0))[:, None] & (prims[None, :] >= first[sl, None]) & (r.dist2 < max2[sl, None])
        if flags & SKIP_SHARED_VERTEX:
            ok = ok & ~shares_vertex_np(a[:, None], tris[None])
        counts[sl] = ok.sum(1)
        for i in range(len(a)):
            col = np.nonzero(ok[i])[0]
            col = col[np.lexsort((prims[col], r.dist2[i, col]))]     # (dist2 first, the id among equals; no NaN among candidates)
            if room is not None:
                col = col[:max(0, int(room[at + i]))]
            rec = np.stack([r.dist2[i, col].view(np.uint32), r.u[i, col].view(np.uint32), r.v[i, col].view(np.uint32), prims[col]], 1).reshape(-1, 4)
            kept[at + i] = (rec, np.ascontiguousarray(r.qa[i, col]).view(np.uint32).reshape(-1, 3),
                            np.ascontiguousarray(r.qb[i, col]).view(np.uint32).reshape(-1, 3))
    return Near(counts, kept)
