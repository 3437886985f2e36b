"""The accuracy statement of rtk_amd/csrc/rtk_pair_rule.h, measured on the CPU: the rule in numpy float32 (tests/pair_ref.py,
bit for bit the header) against the same walk -- features and piercing -- in float64, over random pairs at the five combinations
of triangle size and distance that rtk_closest_rule.h uses. Slivers (smallest height below a twentieth of the longest edge) and
degenerate triangles are left out. Prints, per combination and overall, the worst |sqrt(dist2) - exact| in units of 2^-23 of
the largest coordinate magnitude of the pair.

    python scripts/pair_accuracy.py [--pairs 8000000] [--seed 20250117]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.pair_ref import pair_np  # noqa: E402

SCALE_PAIRS = [(1.0, 1.0), (1e-3, 1.0), (1.0, 1e-3), (100.0, 1.0), (1e-3, 1e-3)]      # (triangle scale, offset scale)


def not_sliver(t):
    """t [n, 3, 3] float64: the smallest height is at least a twentieth of the longest edge"""
    e = np.stack([t[:, 1] - t[:, 0], t[:, 2] - t[:, 1], t[:, 0] - t[:, 2]], 1)
    longest = np.sqrt((e * e).sum(2)).max(1)
    area2 = np.sqrt((np.cross(e[:, 0], e[:, 1]) ** 2).sum(1))                        # twice the area
    return area2 / np.maximum(longest, 1e-300) >= longest / 20


def random_pairs(rng, n, tri_scale, off_scale):
    """Two triangles of the given size; B's centre at the given distance from a point of A's plane that lies inside A or a little
    outside (tests/test_closest_cpu.py's random_family with a triangle in the place of the point)"""
    a = (rng.standard_normal((n, 3, 3)) * tri_scale).astype(np.float32)
    w = rng.uniform(-0.6, 1.6, (n, 2))
    on = a[:, 0] + (a[:, 1] - a[:, 0]) * w[:, :1] + (a[:, 2] - a[:, 0]) * w[:, 1:]
    b = rng.standard_normal((n, 3, 3)) * tri_scale
    b = (b - b.mean(1, keepdims=True) + (on + rng.standard_normal((n, 3)) * off_scale)[:, None, :]).astype(np.float32)
    keep = not_sliver(a.astype(np.float64)) & not_sliver(b.astype(np.float64))
    return a[keep], b[keep]


def worst_error(a, b):
    """-> (worst error in 2^-23 of the largest coordinate, the share of pierced pairs)"""
    got = pair_np(a, b)
    exact = pair_np(a.astype(np.float64), b.astype(np.float64), np.float64)
    mag = np.maximum(np.abs(a).reshape(-1, 9).max(1), np.abs(b).reshape(-1, 9).max(1)).astype(np.float64)
    err = np.abs(np.sqrt(got.dist2.astype(np.float64)) - np.sqrt(exact.dist2)) / mag
    return float(err.max() * 2.0 ** 23), float((got.feature >= 16).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8000000)
    ap.add_argument("--seed", type=int, default=20250117)
    ap.add_argument("--chunk", type=int, default=200000)
    args = ap.parse_args()
    rng = np.random.RandomState(args.seed)
    overall, total = 0.0, 0
    for sp in SCALE_PAIRS:
        worst, pierced, kept = 0.0, 0.0, 0
        for _ in range(max(1, args.pairs // len(SCALE_PAIRS) // args.chunk)):
            a, b = random_pairs(rng, args.chunk, *sp)
            w, p = worst_error(a, b)
            worst, pierced, kept = max(worst, w), pierced + p * len(a), kept + len(a)
        print("scale pair %s: %d pairs, %.1f %% pierced, worst error %.2f * 2^-23 of the largest coordinate" % (sp, kept, 100 * pierced / kept, worst), flush=True)
        overall, total = max(overall, worst), total + kept
    print("overall: %d pairs, worst error %.2f * 2^-23" % (total, overall))


if __name__ == "__main__":
    main()
