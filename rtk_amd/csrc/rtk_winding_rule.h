// rtk_winding_rule.h -- the one rule by which a generalized winding number is evaluated (rtk_dev_winding_numbers, rtk_amd.h), for
// the host and the device: the kernels (rtk_winding.hip) and tests/winding_rule_driver.cpp include this file and nothing else
// decides a value. No HIP, no libm.
//
// The winding number of a point p about a set of oriented triangles is the sum of the signed solid angles they subtend at p,
// divided by 4 pi (Jacobson, Kavan and Sorkine-Hornung 2013): 1 inside and 0 outside a closed surface wound outwards, k inside k
// nested shells, -1 inside a shell wound inwards, a smooth fraction near a hole. It is evaluated over the scene's tree (Barill et
// al. 2018, "Fast winding numbers for soups and clouds", the first-order form): a subtree that is far from p is answered by ONE
// term from its moments, a near one is descended, a leaf's triangles are summed one by one.
//
// Every product, sum, difference and quotient below is ONE float operation, rounded on its own, in the order written: no fused
// multiply-add anywhere (RTK_CL_* of rtk_closest_rule.h: __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn on the device,
// -ffp-contract=off and the pragma "fp contract(off)" on the host). sqrt is RTK_SIGN_SQRT, the correctly rounded root of
// rtk_sign_rule.h; the angle is rtk_sign_angle, that header's polynomial atan2 (1.82e-6 rad against float64). Denormals are kept.
// dot(x, y) = (x0 * y0 + x1 * y1) + x2 * y2, cross(x, y) = (x1 * y2 - x2 * y1, x2 * y0 - x0 * y2, x0 * y1 - x1 * y0).
//
// 1. TRIANGLE TERM (rtk_winding_triangle), p the query, (a, b, c) a record (van Oosterom and Strackee's solid angle):
//        A = a - p    B = b - p    C = c - p                        (componentwise, first)
//        la = sqrt(dot(A, A))    lb = sqrt(dot(B, B))    lc = sqrt(dot(C, C))
//        num = dot(A, cross(B, C))
//        den = (((la * lb) * lc + dot(A, B) * lc) + dot(A, C) * lb) + dot(B, C) * la
//        omega = 2 * rtk_sign_angle(num, den)
//        term = omega * RTK_WINDING_INV_4PI
//    A DEGENERATE triangle with two equal corners (b = c, say) has cross(B, C) = 0 exactly, so num = 0, and den > 0 for a query
//    off its segment: the term is 0 by the atan2's zero cases (0 over a positive x is +0). A query ON A CORNER (A = 0, say) has
//    la = 0, num = 0 and den = 0: the term is +0 (case Z of the angle). A query in the triangle's plane has num = 0 up to
//    rounding: outside the triangle den > 0 and the term is 0, inside it den < 0 and the term is +-1/2, the jump of the surface.
// 2. FAR TERM (rtk_winding_far) of a cluster with area vector N, centre P: the solid angle of a small oriented area N seen from p.
//        d = P - p    r2 = dot(d, d)    r = sqrt(r2)
//        term = (dot(N, d) / (r2 * r)) * RTK_WINDING_INV_4PI
// 3. ACCEPT TEST (rtk_winding_accept). A child with centre P and radius R is answered by its far term iff
//        r2 > (beta * R) * (beta * R)
//    with r2 of 2. The comparison is false for a NaN on either side and for a product that overflows to infinity: a cluster
//    without a finite R is always descended. Otherwise the child is descended, and a leaf's triangles are summed by 1.
//    beta = 2 is the default; a larger beta descends more and is more exact. RTK_WINDING_EXACT accepts nothing.
// 4. MOMENTS OF A CHILD SLOT (rtk_winding_tri_moments, rtk_winding_add, rtk_winding_slot), from the triangles under it:
//        per triangle   e1 = b - a   e2 = c - a   k = cross(e1, e2)
//                       n = 0.5 * k                         (the area vector)
//                       area = 0.5 * sqrt(dot(k, k))
//                       g = ((a + b) + c) / 3               (the centroid)
//                       s = area * g
//        of a LEAF slot    (N, area, S) = the sums of (n, area, s) over the leaf's records IN SLOT ORDER, starting from +0
//        of an INNER slot  the sums of (N, area, S) of the FOUR slots of the node it names, slot 0 to slot 3, starting from
//                          slot 0's values (an empty slot holds +0 everywhere)
//        P = S / area  (componentwise) if area > 0 and area < infinity, else the centre of the child's box, lo * 0.5 + hi * 0.5
//        R, FROM THE BOX:  c = lo * 0.5 + hi * 0.5    h = hi * 0.5 - lo * 0.5    e = P - c
//                          R = (sqrt(dot(e, e)) + sqrt(dot(h, h))) * RTK_WINDING_R_UP
//    Every corner of every triangle under the child lies in the child's box, so within |P - c| + |h| of P; the factor 1 + 2^-18
//    is far above the rounding of the dozen operations before it (each within 2^-24), so R is an upper bound of the distances.
//    It is the bound from the box, not the exact maximum: no second pass over the triangles, a little more descent. An empty
//    slot's record is all +0 and is never read: its child word says it is empty.
//    So THE ORDER OF THE SUMS FOLLOWS THE TREE: which records share a leaf and which slots share a node decide it.
// 5. THE WALK. w starts at +0. The root is node 0. At a node the four slots are looked at in slot order: an empty one is passed
//    over; one that 3. accepts adds its far term to w then and there; of the others the first is entered next and the rest are
//    pushed, to be taken last in first out. At a leaf the triangle terms of its records are added to w in slot order.
//    A query with a non-finite coordinate is answered RTK_WINDING_NAN without a walk.
//
// WHAT IS PROMISED. A winding number is a sum whose order follows the tree, so -- unlike the sign of rtk_sign_rule.h -- THE
// RESULT IS NOT PROMISED BIT FOR BIT ACROSS TREES: a split, a rebuild or another builder may change last bits. The same scene
// object gives the same bits on every call. What is promised instead is a tolerance (tests/test_gpu_winding.py; the measured
// figures are in profiles/winding_accuracy.log): the exact form stays within 1e-3 of the float64 sum over all triangles for
// points that are not within 5 % of the shape's size of the surface -- the per-triangle budget is 2 * 3.64e-6 / (4 pi), about
// 5.8e-7 --, and the fast form classifies such points by w > 0.5 as the float64 sum does.
#pragma once

#include <stdint.h>

#include "rtk_sign_rule.h"

#define RTK_WINDING_INV_4PI 0.0795774683f      // 0x3da2f983: 1 / (4 pi)
#define RTK_WINDING_R_UP 1.00000381f           // 0x3f800020: 1 + 2^-18
#define RTK_WINDING_NAN_BITS 0x7fc00000u       // what a query with a non-finite coordinate is answered

// 1. the term of one record
RTK_CLOSEST_FN float rtk_winding_triangle(const float *p, const float *a, const float *b, const float *c)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	const float A[3] = { RTK_CL_SUB(a[0], p[0]), RTK_CL_SUB(a[1], p[1]), RTK_CL_SUB(a[2], p[2]) };
	const float B[3] = { RTK_CL_SUB(b[0], p[0]), RTK_CL_SUB(b[1], p[1]), RTK_CL_SUB(b[2], p[2]) };
	const float C[3] = { RTK_CL_SUB(c[0], p[0]), RTK_CL_SUB(c[1], p[1]), RTK_CL_SUB(c[2], p[2]) };
	const float la = RTK_SIGN_SQRT(RTK_CL_DOT(A[0], A[1], A[2], A[0], A[1], A[2]));
	const float lb = RTK_SIGN_SQRT(RTK_CL_DOT(B[0], B[1], B[2], B[0], B[1], B[2]));
	const float lc = RTK_SIGN_SQRT(RTK_CL_DOT(C[0], C[1], C[2], C[0], C[1], C[2]));
	float k[3];
	rtk_sign_cross(B, C, k);
	const float num = RTK_CL_DOT(A[0], A[1], A[2], k[0], k[1], k[2]);
	const float ab = RTK_CL_DOT(A[0], A[1], A[2], B[0], B[1], B[2]);
	const float ac = RTK_CL_DOT(A[0], A[1], A[2], C[0], C[1], C[2]);
	const float bc = RTK_CL_DOT(B[0], B[1], B[2], C[0], C[1], C[2]);
	float den = RTK_CL_MUL(RTK_CL_MUL(la, lb), lc);
	den = RTK_CL_ADD(den, RTK_CL_MUL(ab, lc));
	den = RTK_CL_ADD(den, RTK_CL_MUL(ac, lb));
	den = RTK_CL_ADD(den, RTK_CL_MUL(bc, la));
	const float omega = RTK_CL_MUL(2.0f, rtk_sign_angle(num, den));
	return RTK_CL_MUL(omega, RTK_WINDING_INV_4PI);
}

// 2. r2 of the cluster centre P from p, and the far term given r2
RTK_CLOSEST_FN float rtk_winding_r2(const float *p, const float *P, float *d)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	d[0] = RTK_CL_SUB(P[0], p[0]); d[1] = RTK_CL_SUB(P[1], p[1]); d[2] = RTK_CL_SUB(P[2], p[2]);
	return RTK_CL_DOT(d[0], d[1], d[2], d[0], d[1], d[2]);
}
RTK_CLOSEST_FN float rtk_winding_far_of(const float *N, const float *d, float r2)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	const float r = RTK_SIGN_SQRT(r2);
	const float q = RTK_CL_DIV(RTK_CL_DOT(N[0], N[1], N[2], d[0], d[1], d[2]), RTK_CL_MUL(r2, r));
	return RTK_CL_MUL(q, RTK_WINDING_INV_4PI);
}
RTK_CLOSEST_FN float rtk_winding_far(const float *p, const float *N, const float *P)
{
	float d[3];
	const float r2 = rtk_winding_r2(p, P, d);
	return rtk_winding_far_of(N, d, r2);
}

// 3. is the cluster far enough for its far term?
RTK_CLOSEST_FN bool rtk_winding_accept(float r2, float beta, float R)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	const float br = RTK_CL_MUL(beta, R);
	return r2 > RTK_CL_MUL(br, br);
}

// 4. what is summed per child slot: m[0 .. 2] the area vector, m[3] the area, m[4 .. 6] area * centroid
RTK_CLOSEST_FN void rtk_winding_tri_moments(const float *a, const float *b, const float *c, float *m)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	const float e1[3] = { RTK_CL_SUB(b[0], a[0]), RTK_CL_SUB(b[1], a[1]), RTK_CL_SUB(b[2], a[2]) };
	const float e2[3] = { RTK_CL_SUB(c[0], a[0]), RTK_CL_SUB(c[1], a[1]), RTK_CL_SUB(c[2], a[2]) };
	float k[3];
	rtk_sign_cross(e1, e2, k);
	m[0] = RTK_CL_MUL(0.5f, k[0]); m[1] = RTK_CL_MUL(0.5f, k[1]); m[2] = RTK_CL_MUL(0.5f, k[2]);
	m[3] = RTK_CL_MUL(0.5f, RTK_SIGN_SQRT(RTK_CL_DOT(k[0], k[1], k[2], k[0], k[1], k[2])));
	for (int i = 0; i < 3; i++) m[4 + i] = RTK_CL_MUL(m[3], RTK_CL_DIV(RTK_CL_ADD(RTK_CL_ADD(a[i], b[i]), c[i]), 3.0f));
}
RTK_CLOSEST_FN void rtk_winding_add(float *sum, const float *m)
{
	for (int i = 0; i < 7; i++) sum[i] = RTK_CL_ADD(sum[i], m[i]);
}
// the record of a slot from its sums and the child's box: out[0 .. 2] = N, out[3 .. 5] = P, out[6] = R
RTK_CLOSEST_FN void rtk_winding_slot(const float *sum, const float *lo, const float *hi, float *out)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	const bool weighted = sum[3] > 0.0f && sum[3] < __builtin_inff();           // (a NaN fails both)
	float e[3], h[3];
	for (int i = 0; i < 3; i++) {
		const float c = RTK_CL_ADD(RTK_CL_MUL(lo[i], 0.5f), RTK_CL_MUL(hi[i], 0.5f));
		h[i] = RTK_CL_SUB(RTK_CL_MUL(hi[i], 0.5f), RTK_CL_MUL(lo[i], 0.5f));
		out[i] = sum[i];
		out[3 + i] = weighted ? RTK_CL_DIV(sum[4 + i], sum[3]) : c;
		e[i] = RTK_CL_SUB(out[3 + i], c);
	}
	const float r = RTK_CL_ADD(RTK_SIGN_SQRT(RTK_CL_DOT(e[0], e[1], e[2], e[0], e[1], e[2])), RTK_SIGN_SQRT(RTK_CL_DOT(h[0], h[1], h[2], h[0], h[1], h[2])));
	out[6] = RTK_CL_MUL(r, RTK_WINDING_R_UP);
}
