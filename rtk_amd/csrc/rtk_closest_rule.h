// rtk_closest_rule.h -- the one rule by which a closest-point query is answered (rtk_dev_closest_points, rtk_amd.h), for the host
// and the device: the kernel (rtk_closest.hip) and tests/closest_rule_driver.cpp include this file and nothing else decides a bit
// of a result. The result of a query is a pure function of the scene's triangle records and the query; the tree only decides how
// few of the records are looked at.
//
// Every product, sum, difference and quotient below is ONE float operation, rounded on its own, in the order written: no fused
// multiply-add anywhere. On the device that is __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn (the library is built with
// -fhip-fp32-correctly-rounded-divide-sqrt: the quotient is IEEE's); on the host the file must be compiled with
// -ffp-contract=off (the library's flags; clang is told once more by the pragma below). It is what numpy float32 arithmetic
// gives, so a test states the expected bits without a GPU. Denormal inputs and results are kept, as in rtk_place_rule.h.
// min(x, y) is "y < x ? y : x" and max(x, y) is "y > x ? y : x": selects, so that a NaN and the sign of a zero go one stated way.
//
// 1. POINT AND TRIANGLE (rtk_closest_triangle). p is the query, a, b, c are DevTri.v0 / v1 / v2 as the scene holds them,
//    dot(x, y) = (x0 * y0 + x1 * y1) + x2 * y2. Ericson's walk over the regions of the triangle's plane; the first case that
//    matches wins:
//        ab = b - a   ac = c - a   ap = p - a     d1 = dot(ab, ap)  d2 = dot(ac, ap)
//        bp = p - b                               d3 = dot(ab, bp)  d4 = dot(ac, bp)
//        cp = p - c                               d5 = dot(ab, cp)  d6 = dot(ac, cp)
//        vc = d1 * d4 - d3 * d2    vb = d5 * d2 - d1 * d6    va = d3 * d6 - d5 * d4
//         1  d1 <= 0 && d2 <= 0                             wb = 0              wc = 0          (vertex a)
//         2  d3 >= 0 && d4 <= d3                            wb = 1              wc = 0          (vertex b)
//         3  vc <= 0 && d1 >= 0 && d3 <= 0                  wb = d1 / (d1 - d3) wc = 0          (edge ab)
//         4  d6 >= 0 && d5 <= d6                            wb = 0              wc = 1          (vertex c)
//         5  vb <= 0 && d2 >= 0 && d6 <= 0                  wb = 0              wc = d2 / (d2 - d6)   (edge ac)
//         6  e = d4 - d3, g = d5 - d6; va <= 0 && e >= 0 && g >= 0     w = e / (e + g)  wb = 1 - w  wc = w   (edge bc)
//         7  otherwise      den = 1 / ((va + vb) + vc)      wb = vb * den       wc = vc * den   (the face)
//        q = (a + ab * wb) + ac * wc                               (componentwise)
//        lo = min(min(a, b), c)  hi = max(max(a, b), c);  q = q < lo ? lo : (q > hi ? hi : q)      (a NaN stays a NaN)
//        e = p - q;  dist2 = (e0 * e0 + e1 * e1) + e2 * e2
//        u = (1 - wb) - wc  (the weight of vertex 0, rtk's convention)      v = wb  (the weight of vertex 1)
//    The clamp of q to the triangle's own box is part of the rule: it is what makes the skip of 2. exact.
//    A NaN in p fails every comparison, ends in case 7 and gives a NaN dist2; a degenerate triangle (a = b = c) ends in case 1.
//    A triangle with exactly two equal vertices (a = b, say) can end in an edge case whose quotient is 0 / 0: its dist2 is then
//    a NaN, and by 3. such a triangle is never the answer to that query.
// 2. POINT AND BOX (rtk_closest_box_bound). q' = p < lo ? lo : (p > hi ? hi : p), e = p - q', bound = (e0 * e0 + e1 * e1) + e2 * e2:
//    the operations of dist2 in the same order. A box above a triangle contains the triangle's box, so on every axis
//    |p - q| >= |p - q'| holds EXACTLY (p < lo' <= lo <= q, or the mirror image, or q' = p); a rounded difference, a rounded
//    square and a rounded sum are monotone, so bound <= dist2 for every triangle below the box, without a margin.
// 3. BETTER THAN (rtk_closest_better). (dist2, prim) beats (best2, best_prim) iff dist2 < best2 || (dist2 == best2 && prim <
//    best_prim). A NaN dist2 never beats anything. A subtree may be skipped iff bound > best2 -- strictly: an equal bound can
//    hide a lower id -- (rtk_closest_skip; a NaN bound is not skipped).
// The answer to (p, max_dist2) is the best (dist2, prim) by 3. over ALL triangle records with dist2 < max_dist2, or a miss.
//
// Accuracy of 1., measured against the same walk in float64 over 8 million random pairs at five combinations of triangle
// size and point distance (slivers and degenerate triangles left out, and not measured): |sqrt(dist2) - exact| stayed within
// 6.3 * 2^-23 of the largest coordinate magnitude involved. tests/test_closest_cpu.py asserts 16 * 2^-23.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define RTK_CLOSEST_FN __host__ __device__ __forceinline__      // (the arrays of a call are registers once it is inlined)
#else
#define RTK_CLOSEST_FN static inline
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define RTK_CL_MUL(a, b) __fmul_rn((a), (b))
#define RTK_CL_ADD(a, b) __fadd_rn((a), (b))
#define RTK_CL_SUB(a, b) __fsub_rn((a), (b))
#define RTK_CL_DIV(a, b) __fdiv_rn((a), (b))
#else
#define RTK_CL_MUL(a, b) ((a) * (b))
#define RTK_CL_ADD(a, b) ((a) + (b))
#define RTK_CL_SUB(a, b) ((a) - (b))
#define RTK_CL_DIV(a, b) ((a) / (b))
#endif
#define RTK_CL_DOT(x0, x1, x2, y0, y1, y2) RTK_CL_ADD(RTK_CL_ADD(RTK_CL_MUL(x0, y0), RTK_CL_MUL(x1, y1)), RTK_CL_MUL(x2, y2))
#define RTK_CL_MIN(x, y) ((y) < (x) ? (y) : (x))
#define RTK_CL_MAX(x, y) ((y) > (x) ? (y) : (x))
#define RTK_CL_CLAMP(x, lo, hi) ((x) < (lo) ? (lo) : ((x) > (hi) ? (hi) : (x)))

// 1. p against the triangle (a, b, c), each three floats: returns dist2; q[3] the clamped closest point, u and v the weights of
// vertex 0 and vertex 1, region the case taken (1 .. 7)
RTK_CLOSEST_FN float rtk_closest_triangle(const float *p, const float *a, const float *b, const float *c, float *q, float &u, float &v, int &region)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	const float ab0 = RTK_CL_SUB(b[0], a[0]), ab1 = RTK_CL_SUB(b[1], a[1]), ab2 = RTK_CL_SUB(b[2], a[2]);
	const float ac0 = RTK_CL_SUB(c[0], a[0]), ac1 = RTK_CL_SUB(c[1], a[1]), ac2 = RTK_CL_SUB(c[2], a[2]);
	const float ap0 = RTK_CL_SUB(p[0], a[0]), ap1 = RTK_CL_SUB(p[1], a[1]), ap2 = RTK_CL_SUB(p[2], a[2]);
	const float bp0 = RTK_CL_SUB(p[0], b[0]), bp1 = RTK_CL_SUB(p[1], b[1]), bp2 = RTK_CL_SUB(p[2], b[2]);
	const float cp0 = RTK_CL_SUB(p[0], c[0]), cp1 = RTK_CL_SUB(p[1], c[1]), cp2 = RTK_CL_SUB(p[2], c[2]);
	const float d1 = RTK_CL_DOT(ab0, ab1, ab2, ap0, ap1, ap2), d2 = RTK_CL_DOT(ac0, ac1, ac2, ap0, ap1, ap2);
	const float d3 = RTK_CL_DOT(ab0, ab1, ab2, bp0, bp1, bp2), d4 = RTK_CL_DOT(ac0, ac1, ac2, bp0, bp1, bp2);
	const float d5 = RTK_CL_DOT(ab0, ab1, ab2, cp0, cp1, cp2), d6 = RTK_CL_DOT(ac0, ac1, ac2, cp0, cp1, cp2);
	const float vc = RTK_CL_SUB(RTK_CL_MUL(d1, d4), RTK_CL_MUL(d3, d2));
	const float vb = RTK_CL_SUB(RTK_CL_MUL(d5, d2), RTK_CL_MUL(d1, d6));
	const float va = RTK_CL_SUB(RTK_CL_MUL(d3, d6), RTK_CL_MUL(d5, d4));
	const float e = RTK_CL_SUB(d4, d3), g = RTK_CL_SUB(d5, d6);
	// the case, and the ONE quotient it needs (cases 1, 2 and 4 need none: theirs is 0 / 1 and is not used)
	float num = 0.0f, den = 1.0f;
	if (d1 <= 0.0f && d2 <= 0.0f) region = 1;
	else if (d3 >= 0.0f && d4 <= d3) region = 2;
	else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) { region = 3; num = d1; den = RTK_CL_SUB(d1, d3); }
	else if (d6 >= 0.0f && d5 <= d6) region = 4;
	else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) { region = 5; num = d2; den = RTK_CL_SUB(d2, d6); }
	else if (va <= 0.0f && e >= 0.0f && g >= 0.0f) { region = 6; num = e; den = RTK_CL_ADD(e, g); }
	else { region = 7; num = 1.0f; den = RTK_CL_ADD(RTK_CL_ADD(va, vb), vc); }
	const float t = RTK_CL_DIV(num, den);
	float wb = 0.0f, wc = 0.0f;
	if (region == 2) wb = 1.0f;
	else if (region == 3) wb = t;
	else if (region == 4) wc = 1.0f;
	else if (region == 5) wc = t;
	else if (region == 6) { wb = RTK_CL_SUB(1.0f, t); wc = t; }
	else if (region == 7) { wb = RTK_CL_MUL(vb, t); wc = RTK_CL_MUL(vc, t); }
	const float ab[3] = { ab0, ab1, ab2 }, ac[3] = { ac0, ac1, ac2 };
	float s = 0.0f;
	for (int k = 0; k < 3; k++) {
		const float r = RTK_CL_ADD(RTK_CL_ADD(a[k], RTK_CL_MUL(ab[k], wb)), RTK_CL_MUL(ac[k], wc));
		const float m = RTK_CL_MIN(a[k], b[k]), lo = RTK_CL_MIN(m, c[k]);
		const float M = RTK_CL_MAX(a[k], b[k]), hi = RTK_CL_MAX(M, c[k]);
		q[k] = RTK_CL_CLAMP(r, lo, hi);
		const float ek = RTK_CL_SUB(p[k], q[k]), ek2 = RTK_CL_MUL(ek, ek);
		s = k == 0 ? ek2 : RTK_CL_ADD(s, ek2);
	}
	u = RTK_CL_SUB(RTK_CL_SUB(1.0f, wb), wc);
	v = wb;
	return s;
}

// 2. p against the box [lo, hi], each three floats: the bound no triangle inside the box comes below
RTK_CLOSEST_FN float rtk_closest_box_bound(const float *p, const float *lo, const float *hi)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	const float q0 = RTK_CL_CLAMP(p[0], lo[0], hi[0]), q1 = RTK_CL_CLAMP(p[1], lo[1], hi[1]), q2 = RTK_CL_CLAMP(p[2], lo[2], hi[2]);
	const float e0 = RTK_CL_SUB(p[0], q0), e1 = RTK_CL_SUB(p[1], q1), e2 = RTK_CL_SUB(p[2], q2);
	return RTK_CL_ADD(RTK_CL_ADD(RTK_CL_MUL(e0, e0), RTK_CL_MUL(e1, e1)), RTK_CL_MUL(e2, e2));
}

// 3. does (dist2, prim) beat (best2, best_prim)? ... and may what lies behind `bound` be left out?
RTK_CLOSEST_FN bool rtk_closest_better(float dist2, uint32_t prim, float best2, uint32_t best_prim)
{
	return dist2 < best2 || (dist2 == best2 && prim < best_prim);
}
RTK_CLOSEST_FN bool rtk_closest_skip(float bound, float best2) { return bound > best2; }
