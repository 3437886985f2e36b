// rtk_obb_rule.h -- the one rule by which "the triangles that touch an oriented box" are counted and listed
// (rtk_dev_triangles_in_obb_count / rtk_dev_triangles_in_obb_all, rtk_amd.h), for the host and the device: the kernel
// (rtk_obb.hip) and tests/obb_rule_driver.cpp include this file, and nothing else decides a bit of a result. tests/obb_ref.py
// restates it in numpy. The result is a pure function of the scene's triangle records and the query; the tree only decides how
// few of the records are looked at, and the order of the walk decides nothing.
//
// All arithmetic is float32. Every product, sum and difference below is ONE float operation, rounded on its own, in the order
// written: no fused multiply-add anywhere (rtk_closest_rule.h says how that is kept on the device and on the host; its macros
// are used here). |x| clears the sign bit, min and max are selects, dot(x, y) = (x0 * y0 + x1 * y1) + x2 * y2. Denormal inputs
// and results are kept.
//
// THE QUERY is a rtk_obb_query: centre, half = the half extents along the box's own axes, u0, u1, u2 = the rows of `axes`: the
// box's axes in scene coordinates. The box is { centre + a0 * u0 + a1 * u1 + a2 * u2 : |aj| <= half[j] }.
// 0. LIVE (rtk_obb_prepare). The query is live iff all fifteen floats are finite (x - x == 0), every half[j] >= 0 and the axes
//    are orthonormal to within RTK_OBB_ORTHO_TOL = 2^-10, by the six comparisons rtk_obbsweep_prepare makes (restated here; the
//    sweep's header is not touched): |dot(uj, uj) - 1| <= tol for j = 0, 1, 2 and |dot(u0, u1)|, |dot(u0, u2)|, |dot(u1, u2)|
//    <= tol. The tolerance is a gate against garbage, not an accuracy claim: within it the axes are used as given and treated
//    as orthonormal. A left-handed triple is a box as well. half == 0 on one, two or three axes is legal: a rectangle, a
//    segment, a point. A query that is not live has no candidates, and neither has any query of a scene without triangles.
//    Once per query:
//        g[k]   = (|u0[k]| * half[0] + |u1[k]| * half[1]) + |u2[k]| * half[2]      the box's reach along scene axis k (the sweep's)
//        qlo[k] = centre[k] - g[k]        qhi[k] = centre[k] + g[k]                 the box's bounds in the scene's axes
// 1. BOXES: rtk_box_boxes_touch(v0, v1, v2, qlo, qhi) of rtk_box_rule.h as it stands: closed, comparisons only.
// 2. THE FRAME (rtk_obb_separated). w_k = v_k - centre in the scene's axes, then w_k' = (dot(u0, w_k), dot(u1, w_k), dot(u2, w_k)).
//    The box's own axis j separates iff w_0'[j], w_1'[j], w_2'[j] are all > half[j] or all < -half[j]. The other ten axes are
//    rtk_box_separated(w_0', w_1', w_2', zero, half) of rtk_box_rule.h AS IT STANDS: with c = 0 its w = v - c is exact and its
//    edges are differences of the primed vertices. A COMPARISON WITH A NaN NEVER SEPARATES.
// 3. CANDIDATE (rtk_obb_candidate). A triangle record is a candidate iff the query is live, 1. holds and none of the thirteen
//    axes of 2. separates. The COUNT of a query is the number of its candidates, the LIST its candidates in ASCENDING PRIMITIVE
//    ID; a segment with room for r entries keeps the first min(count, r), through rtk_box_insert unchanged.
// 4. SKIP: rtk_box_skip(clo, chi, qlo, qhi). EXACT WITHOUT A MARGIN for the reason the box rule gives: every box above a triangle
//    contains the triangle's own box, 1. is part of the candidate rule, so a node box disjoint from [qlo, qhi] proves that 1.
//    fails for everything below it. Only the exact 128-byte nodes are used. A tighter test of a node box by the box's own axes
//    would need a margin and would make the set depend on rounding the triangle rule does not share: it is not made.
//
// WHAT THE RULE IS AND IS NOT.
//  * It is a FLOAT RULE, and the candidate set is DEFINED BY IT: where the rounded w', p, r and d put a triangle that passes
//    within a few ulps of the box's face, edge or corner on the other side of a comparison than real arithmetic would, the
//    rule wins. On inputs whose every intermediate is exact (small integers with signed-permutation axes) it is the exact
//    separating-axis answer, and touching counts. 1. uses the reach g, which is rounded as well: a triangle that the thirteen
//    axes would keep but whose box misses [qlo, qhi] by a rounding of g is not a candidate.
//  * IDENTITY AXES give the answer of rtk_dev_triangles_in_box_* on [centre - half, centre + half] UP TO ROUNDING, NOT bit
//    for bit: g = half and w' = w exactly (a product with 1, sums with +-0), but that call measures from (lo + hi) * 0.5f with
//    (hi - lo) * 0.5f, which need not be centre and half again, and its edges are differences of the stored vertices, not of
//    the shifted ones. Where centre, half and the vertices are small integers the two agree byte for byte
//    (tests/test_gpu_obb.py, all 48 signed-permutation axes).
//  * A ZERO-AREA TRIANGLE behaves as in rtk_box_rule.h, in the box's frame: its plane separates nothing; three coinciding
//    vertices are a candidate whenever 1. holds and no own axis of the box separates the point; a segment is decided by the
//    nine edge axes, and a sliver whose n, p and r all round towards 0 is kept whenever 1. and the three own axes keep it.
//  * A box WITHOUT VOLUME has r = 0 on the axes its zero extents take part in, and there the comparison is with the rounding
//    error of w', p or d alone: a point box at a vertex is a candidate of that vertex's triangles only where the rounded frame
//    coordinates and projections come out as exact zeros, which a turned frame rarely grants. Give such a query the extent the
//    data's accuracy calls for.
//  * A scene with NON-FINITE vertex coordinates: the calls terminate and write only inside their outputs.
//    NOTHING ELSE IS PROMISED about their results.
//
// ACCURACY of 1. to 3., measured against the same rule in float64 (tests/test_obb_cpu.py) over 1.2 million (triangle, box,
// rotation) cases at four combinations of triangle size, box size and distance from the origin, rotations from random unit
// quaternions rounded to float32; three quarters of the cases are contacts by construction (a vertex on a face, a corner on
// the triangle's plane, an edge on an edge), moved off the contact by 0 to 64 ulps of the largest coordinate, because random
// cases are hardly ever within a rounding of a threshold. float32 and float64 disagreed about candidate or not on
// RTK_OBB_DISAGREE of them, and in every one of these each comparison that came out differently had a float64 margin -- by how
// much the axis separates or keeps, as a length -- within RTK_OBB_K * 2^-23 of the largest coordinate magnitude involved
// (vertices, centre -+ reach); the test asserts 3.23 * 2^-23, 2.5 times that.
//   RTK_OBB_DISAGREE = 37118      RTK_OBB_K = 1.29
#pragma once

#include <stdint.h>
#include "rtk_closest_rule.h"      // RTK_CLOSEST_FN, RTK_CL_MUL / _ADD / _SUB / _DOT, RTK_CL_MIN / _MAX: the macros only
#include "rtk_box_rule.h"          // rtk_box_boxes_touch, rtk_box_separated, rtk_box_skip, rtk_box_insert: as they stand

#ifndef RTK_OBB_ORTHO_TOL
#define RTK_OBB_ORTHO_TOL 0.0009765625f       // 2^-10 (rtk_obbsweep_rule.h states the same number)
#endif

// what the walk keeps of a query: the fifteen floats as given, and the box's bounds in the scene's axes
struct rtk_obb_prepared {
	float c[3], h[3], U[9];
	float qlo[3], qhi[3];
};

// 0. w: the fifteen floats of a rtk_obb_query. Returns whether the query is live; Q is filled either way
RTK_CLOSEST_FN bool rtk_obb_prepare(const float *w, rtk_obb_prepared &Q)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	bool finite = true;
	for (int k = 0; k < 15; k++) finite = finite && RTK_CL_SUB(w[k], w[k]) == 0.0f;
	for (int k = 0; k < 3; k++) { Q.c[k] = w[k]; Q.h[k] = w[3 + k]; }
	for (int k = 0; k < 9; k++) Q.U[k] = w[6 + k];
	const float *u0 = Q.U, *u1 = Q.U + 3, *u2 = Q.U + 6;
	for (int k = 0; k < 3; k++) {
		const float g = RTK_CL_ADD(RTK_CL_ADD(RTK_CL_MUL(RTK_BOX_ABS(u0[k]), Q.h[0]), RTK_CL_MUL(RTK_BOX_ABS(u1[k]), Q.h[1])), RTK_CL_MUL(RTK_BOX_ABS(u2[k]), Q.h[2]));
		Q.qlo[k] = RTK_CL_SUB(Q.c[k], g);
		Q.qhi[k] = RTK_CL_ADD(Q.c[k], g);
	}
	const float tol = RTK_OBB_ORTHO_TOL;
	const float d00 = RTK_CL_SUB(RTK_CL_DOT(u0[0], u0[1], u0[2], u0[0], u0[1], u0[2]), 1.0f);
	const float d11 = RTK_CL_SUB(RTK_CL_DOT(u1[0], u1[1], u1[2], u1[0], u1[1], u1[2]), 1.0f);
	const float d22 = RTK_CL_SUB(RTK_CL_DOT(u2[0], u2[1], u2[2], u2[0], u2[1], u2[2]), 1.0f);
	const float d01 = RTK_CL_DOT(u0[0], u0[1], u0[2], u1[0], u1[1], u1[2]);
	const float d02 = RTK_CL_DOT(u0[0], u0[1], u0[2], u2[0], u2[1], u2[2]);
	const float d12 = RTK_CL_DOT(u1[0], u1[1], u1[2], u2[0], u2[1], u2[2]);
	const bool ortho = RTK_BOX_ABS(d00) <= tol && RTK_BOX_ABS(d11) <= tol && RTK_BOX_ABS(d22) <= tol &&
		RTK_BOX_ABS(d01) <= tol && RTK_BOX_ABS(d02) <= tol && RTK_BOX_ABS(d12) <= tol;
	return finite && Q.h[0] >= 0.0f && Q.h[1] >= 0.0f && Q.h[2] >= 0.0f && ortho;
}

// 2. a vertex in the box's frame: w = v - centre, then the three dots
RTK_CLOSEST_FN void rtk_obb_to_frame(const rtk_obb_prepared &Q, const float *v, float *p)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	const float w0 = RTK_CL_SUB(v[0], Q.c[0]), w1 = RTK_CL_SUB(v[1], Q.c[1]), w2 = RTK_CL_SUB(v[2], Q.c[2]);
	p[0] = RTK_CL_DOT(Q.U[0], Q.U[1], Q.U[2], w0, w1, w2);
	p[1] = RTK_CL_DOT(Q.U[3], Q.U[4], Q.U[5], w0, w1, w2);
	p[2] = RTK_CL_DOT(Q.U[6], Q.U[7], Q.U[8], w0, w1, w2);
}

// 2. does one of the thirteen axes separate the triangle from the box?
RTK_CLOSEST_FN bool rtk_obb_separated(const rtk_obb_prepared &Q, const float *v0, const float *v1, const float *v2)
{
	float p0[3], p1[3], p2[3];
	rtk_obb_to_frame(Q, v0, p0);
	rtk_obb_to_frame(Q, v1, p1);
	rtk_obb_to_frame(Q, v2, p2);
	bool sep = false;
	for (int j = 0; j < 3; j++) {
		const float h = Q.h[j], nh = -h;
		sep = sep || (p0[j] > h && p1[j] > h && p2[j] > h) || (p0[j] < nh && p1[j] < nh && p2[j] < nh);
	}
	const float zero[3] = { 0.0f, 0.0f, 0.0f };
	return sep || rtk_box_separated(p0, p1, p2, zero, Q.h);
}

// 3. `live` from rtk_obb_prepare
RTK_CLOSEST_FN bool rtk_obb_candidate(const rtk_obb_prepared &Q, bool live, const float *v0, const float *v1, const float *v2)
{
	return live && rtk_box_boxes_touch(v0, v1, v2, Q.qlo, Q.qhi) && !rtk_obb_separated(Q, v0, v1, v2);
}

// 4. may what lies below the child box [clo, chi] be left out?
RTK_CLOSEST_FN bool rtk_obb_skip(const rtk_obb_prepared &Q, const float *clo, const float *chi)
{
	return rtk_box_skip(clo, chi, Q.qlo, Q.qhi);
}
