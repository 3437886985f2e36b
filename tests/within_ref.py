"""The rule of rtk_amd/csrc/rtk_within_rule.h restated in numpy float32 on top of tests/closest_ref.py (imported, not copied), for
tests/test_within_cpu.py (against the header's driver) and tests/test_gpu_within.py (against the kernel): per query the count
of its candidates, its full list in ascending (dist2, prim) order, and the prefix a segment of a given room keeps."""
import numpy as np

from tests.closest_ref import tri_np


class Within:
    """counts uint32 [Q]; lists[i] = (record words uint32 [count_i, 4] -- dist2, u, v, prim --, point words uint32 [count_i, 3]),
    sorted by (dist2, prim); kept[i] = the same, cut to room[i] entries (the lists themselves without room)"""

    def __init__(self, counts, lists, kept):
        self.counts, self.lists, self.kept = counts, lists, kept

    def written(self):
        return np.array([len(r) for r, _ in self.kept], np.uint32)


def brute_force_within(tris, prims, points, max2, room=None):
    """tris [T, 3, 3] float32 with ids prims [T], points [Q, 3], max2 [Q], room None or [Q] -> Within. A candidate: dist2 <
    max2 (a NaN dist2 is none) of a live query (max2 > 0, finite coordinates)."""
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 3, 3)
    prims = np.asarray(prims, np.uint32)
    points = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    max2 = np.ascontiguousarray(max2, np.float32)
    Q, T = len(points), len(tris)
    empty = (np.zeros((0, 4), np.uint32), np.zeros((0, 3), np.uint32))
    if T == 0 or Q == 0:
        return Within(np.zeros(Q, np.uint32), [empty] * Q, [empty] * Q)
    dist2, u, v, q, _ = tri_np(points[:, None, :], tris[None, :, 0], tris[None, :, 1], tris[None, :, 2])
    with np.errstate(invalid="ignore"):
        live = (max2 > 0) & np.isfinite(points).all(1)
        cand = (dist2 < max2[:, None]) & live[:, None]
    counts = cand.sum(1).astype(np.uint32)
    lists, kept = [], []
    for i in range(Q):
        col = np.nonzero(cand[i])[0]
        col = col[np.lexsort((prims[col], dist2[i, col]))]           # (dist2 first, the id among equals; no NaN among candidates)
        rec = np.stack([dist2[i, col].view(np.uint32), u[i, col].view(np.uint32), v[i, col].view(np.uint32), prims[col]], 1).reshape(-1, 4)
        pts = np.ascontiguousarray(q[i, col]).view(np.uint32).reshape(-1, 3)
        lists.append((rec, pts))
        r = len(col) if room is None else min(len(col), int(room[i]))
        kept.append((rec[:r], pts[:r]))
    return Within(counts, lists, kept)
