"""The rule of rtk_amd/csrc/rtk_obb_rule.h restated in numpy float32, for tests/test_obb_cpu.py (against the header's driver) and
tests/test_gpu_obb.py (against the kernel): every product, sum and difference is one float32 operation in the header's order.
The ten axes, the boxes' test and the skip are tests/box_ref.py's own. A query is [..., 15]: centre, half, the nine axis floats.
With dtype=np.float64 the same routines are the float64 reference of the accuracy test."""
import numpy as np

from tests.box_ref import InBoxes, boxes_touch_np, separated_np
from tests.box_ref import skip_np as box_skip_np

F = np.float32
TOL = 2.0 ** -10


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def split(q):
    """[..., 15] -> centre [..., 3], half [..., 3], u0, u1, u2 [..., 3] each"""
    return q[..., 0:3], q[..., 3:6], q[..., 6:9], q[..., 9:12], q[..., 12:15]


def live_np(q):
    """rule 0: [..., 15] -> bool [...]"""
    c, h, u0, u1, u2 = split(q)
    one, tol = q.dtype.type(1), q.dtype.type(TOL)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        finite = (q - q == 0).all(-1)
        ortho = (np.abs(_dot(u0, u0) - one) <= tol) & (np.abs(_dot(u1, u1) - one) <= tol) & (np.abs(_dot(u2, u2) - one) <= tol) & \
            (np.abs(_dot(u0, u1)) <= tol) & (np.abs(_dot(u0, u2)) <= tol) & (np.abs(_dot(u1, u2)) <= tol)
        return finite & (h >= 0).all(-1) & ortho


def reach_np(q):
    """rule 0: -> g, qlo, qhi, [..., 3] each"""
    c, h, u0, u1, u2 = split(q)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        g = (np.abs(u0) * h[..., 0:1] + np.abs(u1) * h[..., 1:2]) + np.abs(u2) * h[..., 2:3]
        return g, c - g, c + g


def to_frame_np(q, v):
    c, h, u0, u1, u2 = split(q)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        w = v - c
        return np.stack([_dot(u0, w), _dot(u1, w), _dot(u2, w)], -1)


def separated13_np(q, v0, v1, v2):
    """rule 2: does one of the thirteen axes separate?"""
    h = q[..., 3:6]
    p0, p1, p2 = to_frame_np(q, v0), to_frame_np(q, v1), to_frame_np(q, v2)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        own = (((p0 > h) & (p1 > h) & (p2 > h)) | ((p0 < -h) & (p1 < -h) & (p2 < -h))).any(-1)
        hb = np.broadcast_to(h, p0.shape)
        return own | separated_np(p0, p1, p2, np.zeros_like(hb), hb)


def candidate_np(q, v0, v1, v2):
    """rule 3, arrays that broadcast against each other: q [..., 15], v [..., 3] -> bool [...]"""
    _, qlo, qhi = reach_np(q)
    return live_np(q) & boxes_touch_np(v0, v1, v2, qlo, qhi) & ~separated13_np(q, v0, v1, v2)


def skip_np(q, clo, chi):
    """rule 4"""
    _, qlo, qhi = reach_np(q)
    return box_skip_np(clo, chi, qlo, qhi)


def brute_force_obbs(tris, prims, q, room=None):
    """tris [T, 3, 3] float32 with ids prims [T], q [Q, 15] float32 (or OBB_QUERY_DTYPE records), room None or [Q] -> InBoxes.
    Also sets .step1 [Q, T]: the triangle's box touches [qlo, qhi] and the query is live (what the frame then decides about)."""
    tris = np.ascontiguousarray(tris, F).reshape(-1, 3, 3)
    prims = np.asarray(prims, np.uint32)
    q = np.ascontiguousarray(q)
    q = q.view(F).reshape(-1, 15) if q.dtype.names else np.ascontiguousarray(q, F).reshape(-1, 15)
    Q, T = len(q), len(tris)
    empty = np.zeros(0, np.uint32)
    if T == 0 or Q == 0:
        out = InBoxes(np.zeros(Q, np.uint32), [empty] * Q, [empty] * Q)
        out.step1 = np.zeros((Q, T), bool)
        return out
    qq = q[:, None, :]
    _, qlo, qhi = reach_np(qq)
    step1 = live_np(qq) & boxes_touch_np(tris[None, :, 0], tris[None, :, 1], tris[None, :, 2], qlo, qhi)
    cand = np.zeros((Q, T), bool)
    qi, ti = np.nonzero(step1)                                   # (the frame only where step 1 holds: the rule's own shortcut)
    cand[qi, ti] = ~separated13_np(q[qi], tris[ti, 0], tris[ti, 1], tris[ti, 2])
    counts = cand.sum(1).astype(np.uint32)
    lists, kept = [], []
    for i in range(Q):
        ids = np.sort(prims[np.nonzero(cand[i])[0]])
        lists.append(ids)
        kept.append(ids if room is None else ids[:int(room[i])])
    out = InBoxes(counts, lists, kept)
    out.step1 = step1
    return out
