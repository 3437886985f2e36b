// rtk_world_closest_rule.h -- the rule by which a closest-point query on an instanced world is answered
// (rtk_dev_world_closest_points, rtk_amd.h), for the host and the device: the kernel (rtk_world_closest.hip) and
// tests/world_closest_rule_driver.cpp include this file, and nothing but it, rtk_closest_rule.h and rtk_place_rule.h decides a bit
// of a result. No HIP, no libm. The answer is a pure function of the instances' triangle records, their placements, the filter
// and the query; neither tree decides more than how few records are looked at. DESIGN.md 3.23.1.
//
// 1. THE PLACED TRIANGLE. A record's v0 / v1 / v2, as the instance's scene holds them, are moved by rtk_place_vertex under the
//    instance's FORWARD placement (the rtk_placement the world was given, not the inverse the rays use); rtk_closest_triangle on
//    the placed vertices gives dist2, u, v and q in world coordinates. The ingest of rtk_dev_scene_build_placed places the same
//    floats by the same rule, so these are the bits rtk_dev_closest_points gives on the flat placed twin.
// 2. THE PLACED BOX (rtk_world_placed_box). For world axis j, with the row r = (m[4j], m[4j+1], m[4j+2], m[4j+3]):
//        whi[j] = rtk_place_row(r, cx, cy, cz)    cx = m[4j] < 0 ? lo.x : hi.x,  cy by m[4j+1],  cz by m[4j+2]
//        wlo[j] = rtk_place_row(r, the opposite corner)
//    six rows per box. WHY IT IS EXACT: rtk_place_row is a chain of separately rounded products and sums. A rounded product
//    a * x is monotone in x (rising for a >= 0, falling for a < 0; constant for a = 0), a rounded sum is monotone in each
//    operand, so the row is monotone in each of x, y and z, in the direction the sign of its coefficient gives. Over a box its
//    largest value is therefore attained at the corner chosen above and its smallest at the opposite one: [wlo, whi] is the
//    min / max over the eight corners placed by rtk_place_vertex, as values bit for bit (where a bound is a zero and the
//    translation is -0 the SIGN of that zero may be another corner's; rtk_closest_box_bound does not see the sign of a zero).
//    Every vertex inside [lo, hi] is placed inside [wlo, whi] EXACTLY, by the same monotonicity, and so is every box inside
//    [lo, hi]. rtk_closest_box_bound(p, wlo, whi) is therefore a lower bound of every dist2 of 1. below that node, without a
//    margin: the argument of rtk_closest_rule.h point 2 on the placed vertices.
//    THE TOP TREE needs nothing new: a proxy's box is this box of the scene's root (rtk_world_box takes the same eight corners)
//    grown by a pad, the top tree's node boxes contain the proxies, so rtk_closest_box_bound on them as they are -- no margin,
//    no rtk_world_margin -- is a lower bound too.
//    (All this for finite values. A placed vertex that is not finite promises nothing about results.)
// 3. BETTER THAN (rtk_world_closest_better). (dist2, inst, prim) beats (best2, best_inst, best_prim) iff dist2 < best2, or
//    dist2 == best2 and inst < best_inst, or both are equal and prim < best_prim. A NaN dist2 never wins. Unlike the world's
//    rays, a tie ACROSS INSTANCES IS DECIDED: the lowest instance number. A subtree is skipped iff bound > best2, strictly
//    (rtk_closest_skip), at a top node, a proxy, a scene node and again at the pop.
// The answer to (p, max_dist2) is the best by 3. over every triangle of every live instance the filter lets through with
// dist2 < max_dist2, or a miss. Liveness of a query and the miss record are rtk_dev_closest_points's.
#pragma once

#include "rtk_world_rule.h"
#include "rtk_closest_rule.h"

// 2. the world bounds of the local box [lo, hi] under placement m[12]: exactly the min / max over its eight placed corners
RTK_CLOSEST_FN void rtk_world_placed_box(const float *m, const float *lo, const float *hi, float *wlo, float *whi)
{
	for (int j = 0; j < 3; j++) {
		const float a = m[4 * j], b = m[4 * j + 1], c = m[4 * j + 2], d = m[4 * j + 3];
		const bool nx = a < 0.0f, ny = b < 0.0f, nz = c < 0.0f;
		whi[j] = rtk_place_row(a, b, c, d, nx ? lo[0] : hi[0], ny ? lo[1] : hi[1], nz ? lo[2] : hi[2]);
		wlo[j] = rtk_place_row(a, b, c, d, nx ? hi[0] : lo[0], ny ? hi[1] : lo[1], nz ? hi[2] : lo[2]);
	}
}

// 1. p against the record (a, b, c) of an instance placed by m[12]: rtk_closest_triangle on the placed vertices
RTK_CLOSEST_FN float rtk_world_closest_triangle(const float *p, const float *m, const float *a, const float *b, const float *c, float *q, float &u, float &v)
{
	float pa[3] = { a[0], a[1], a[2] }, pb[3] = { b[0], b[1], b[2] }, pc[3] = { c[0], c[1], c[2] };
	rtk_place_vertex(m, pa[0], pa[1], pa[2]);
	rtk_place_vertex(m, pb[0], pb[1], pb[2]);
	rtk_place_vertex(m, pc[0], pc[1], pc[2]);
	int region;
	return rtk_closest_triangle(p, pa, pb, pc, q, u, v, region);
}

// 3. does (dist2, inst, prim) beat (best2, best_inst, best_prim)?
RTK_CLOSEST_FN bool rtk_world_closest_better(float dist2, uint32_t inst, uint32_t prim, float best2, uint32_t best_inst, uint32_t best_prim)
{
	return dist2 < best2 || (dist2 == best2 && (inst < best_inst || (inst == best_inst && prim < best_prim)));
}
