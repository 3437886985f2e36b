// rtk_sweep_rule.h -- the one rule by which a sphere sweep is answered (rtk_dev_sweep_spheres, rtk_amd.h), for the host and the
// device: the kernel (rtk_sweep.hip) and tests/sweep_rule_driver.cpp include this file and nothing else decides a bit of a
// result. The result of a query is a pure function of the scene's triangle records and the query; the tree only decides how few
// of the records are looked at.
//
// Every product, sum, difference, quotient and square root below is ONE float operation, rounded on its own, in the order
// written: no fused multiply-add anywhere. On the device that is __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn and sqrtf (the
// library is built with -fhip-fp32-correctly-rounded-divide-sqrt: quotient and root are IEEE's; __fsqrt_rn is NOT used, HIP
// maps it to the native approximation, which is an ulp off on one root in a hundred); on the host the file must be
// compiled with -ffp-contract=off (the library's flags; clang is told once more by the pragma below). It is what numpy float32
// arithmetic gives, so a test states the expected bits without a GPU. Denormal inputs and results are kept. min and max are the
// selects of rtk_closest_rule.h; -x is the exact negation; dot(x, y) = (x0 * y0 + x1 * y1) + x2 * y2;
// cross(x, y) = (x1 * y2 - x2 * y1, x2 * y0 - x0 * y2, x0 * y1 - x1 * y0).
//
// 0. THE QUERY (rtk_sweep_prepare). O = origin, D = direction, r = radius; the ball's centre is c(t) = O + D * t (componentwise,
//    one product and one sum), t over the CLOSED interval [min_t, max_t] -- not a ray's open one. A query is LIVE iff O, D, min_t,
//    max_t and r are finite (RTK_INF is a finite float: "no limit"), D is not all zeros, r >= 0 and min_t <= max_t; a query that
//    is not live is a miss. Once per query: dd = dot(D, D), r2 = r * r, s = c(min_t).
// 1. THE PATH AND A BOX (rtk_sweep_slab): the box [lo, hi] grown by r against the path, clipped to [min_t, max_t].
//        t0 = min_t, t1 = max_t; for k = 0, 1, 2:   l = lo[k] - r,  h = hi[k] + r
//            D[k] == 0:   empty unless l <= O[k] && O[k] <= h                      (a closed containment test, no quotient)
//            otherwise    tl = (l - O[k]) / D[k], th = (h - O[k]) / D[k];  D[k] > 0: t0 = max(t0, tl), t1 = min(t1, th)
//                                                                          D[k] < 0: t0 = max(t0, th), t1 = min(t1, tl)
//        empty unless t0 <= t1; the ENTRY TIME is te = t0.
//    A quotient, not a reciprocal: for a live query and finite boxes no operand is a NaN (O is finite, so l - O[k] is never
//    inf - inf; D[k] != 0, so no 0 / 0, also for a denormal D[k]), hence neither is te.
//    THE BOUND: a box above a triangle contains the triangle's own box (lo' <= lo, hi' >= hi). A rounded difference, a rounded sum
//    and a rounded quotient by a fixed divisor are monotone, and so are the selects: on every axis l' <= l and h' >= h, the
//    containment test of the larger box holds where the smaller one's does, the near plane's time of the larger box is <= and
//    its far plane's time >= the smaller one's (for D[k] < 0 the planes swap and the quotient reverses the order twice). So
//    t0' <= t0 and t1' >= t1 EXACTLY: the larger box's interval is empty only if the triangle's is, and its entry time never
//    exceeds the triangle's te, without a margin. By 2. (iv) the triangle's time is >= its te: entry time <= time for every
//    triangle below the box.
// 2. THE BALL AND ONE TRIANGLE (rtk_sweep_triangle). a, b, c are DevTri.v0 / v1 / v2 as the scene holds them. A time or "none":
//    (i)   the triangle's own box lo = min(min(a, b), c), hi = max(max(a, b), c) by 1.: empty means none; its entry time is te.
//    (ii)  START OVERLAP: rtk_closest_triangle(s) gives dist2 <= r2 (touching counts; a NaN dist2 does not): the time is
//          max(min_t, te) -- min_t, or an ulp above it where the start sits on the border of the grown box.
//    (iii) otherwise the smallest valid time of seven features, in this order, the first among equal times. They are measured
//          FROM THE CENTRE AT te: O' = c(te), lo_t = min_t - te, hi_t = max_t - te, c'(t) = O' + D * t. (Measured from the origin,
//          the quadratics below cancel catastrophically once the origin is far from the triangle compared with the radius:
//          the error then reached a third of the largest coordinate. From c(te) every m is of the size of the grown box.)
//          FACE      ab = b - a, ac = c - a, n = cross(ab, ac), nn = dot(n, n), len = sqrt(nn), ma = O' - a,
//                    h0 = dot(n, ma), hd = dot(n, D), hs = h0 + lo_t * hd, sr = hs < 0 ? -r : r,
//                    t = (sr * len - h0) / hd;  valid iff nn > 0 && hd != 0 && rtk_closest_triangle(c'(t)) ends in case 7
//          ENTRY     of a path m + D * t into the ball of radius r about 0, with A = dot(D, D) and B = dot(m, D), by its closest
//                    approach: t0 = -B / A, m0 = m + D * t0, disc = r2 - dot(m0, m0), t = t0 - sqrt(disc / A); real iff disc >= 0.
//                    (The textbook root (-B - sqrt(B * B - A * C)) / A subtracts squares of the size of the TRIANGLE: with a
//                    radius of a thousandth of that size its discriminant kept no digit, triangles were missed and the error
//                    reached 1.8e-3 of the largest coordinate. Here disc subtracts squares of the size of the radius.)
//          EDGES     ab, bc, ca (p to q): e = q - p, m = O' - p, ee = dot(e, e), nd = dot(e, D), md = dot(e, m); the parts across
//                    the edge D' = D - e * (nd / ee), m' = m - e * (md / ee); t = ENTRY of m' + D' * t with A = dot(D', D'),
//                    B = dot(m', D');  w = md + t * nd;  valid iff ee > 0 && A > 0 && real && 0 <= w && w <= ee
//          VERTICES  a, b, c (p): m = O' - p;  t = ENTRY of m + D * t with A = dd, B = dot(m, D);  valid iff real
//          and every feature needs lo_t <= t && t <= hi_t (a NaN t fails it). No valid feature: none.
//    (iv)  THE TIME of a feature is max(te + t, te). In exact arithmetic the contact lies inside the grown box and the max
//          changes nothing; stated in floats it is what makes the skip of 3. exact, as the clamp of q is for closest points.
//          A time > max_t is NONE: for te < 0 the rounding of max_t - te can admit a t whose te + t rounds to the neighbour
//          above max_t, and no time outside [min_t, max_t] is ever reported (te >= min_t, and te <= max_t where the interval
//          is not empty, so the time of (ii) is inside as well).
//    ENTRY is the smaller root of the feature's quadratic: the time the ball enters the feature's cylinder or sphere; a ball that starts clear
//    of the triangle first touches it at the smallest of them whose contact lies on the feature.
//    r == 0 is legal and is this rule on a point: it is NOT rtk's watertight ray test and not bit-equal to a trace.
// 3. BETTER THAN (rtk_sweep_better). (t, prim) beats (best_t, best_prim) iff t < best_t || (t == best_t && prim < best_prim). A
//    NaN never beats anything. A subtree may be skipped iff its interval by 1. is empty or te > best_t -- strictly: an equal
//    entry time can hide a lower id -- (rtk_sweep_skip; a NaN entry time is not skipped).
// The answer is the best (t, prim) by 3. over ALL triangle records that pass the filter and have a time, starting from
// (max_t, RTK_PRIM_NONE), or a miss. ONE rtk_closest_triangle(c(t)) on the answer's triangle gives the record: u, v and the
// contact point q; the centre c(t) is reported as computed there.
//
// Accuracy of 2., measured against the same features in float64 over 3 million random (triangle, path, radius) cases at five
// combinations of triangle size, start distance and radius, on the 0.49 million that have a time from a feature in both
// (52 of them from another feature in float64: a contact on the border between two; slivers, degenerate triangles, grazing contacts and starts that overlap left out, and not measured): |t - exact| * |D| stayed
// within 56.71 * 2^-23 of the largest coordinate magnitude involved; tests/test_sweep_cpu.py asserts 142 * 2^-23. float32 and
// float64 disagreed about hit or none on 13 of the 3 million pairs, every one of them within rounding of a threshold.
#pragma once

#include <stdint.h>
#include "rtk_closest_rule.h"

// (the same on the device: under the library's flag the builtin is IEEE's root, while HIP's __fsqrt_rn is the native approximation)
#define RTK_SW_SQRT(a) __builtin_sqrtf((a))
#define RTK_SW_MAX_FLOAT 3.402823466e38f
#define RTK_SW_FINITE(x) ((x) >= -RTK_SW_MAX_FLOAT && (x) <= RTK_SW_MAX_FLOAT)

// what 2. found: none, the start overlap, or the feature that gave the time
enum { RTK_SW_NONE = 0, RTK_SW_START = 1, RTK_SW_FACE = 2, RTK_SW_EDGE_AB = 3, RTK_SW_EDGE_BC = 4, RTK_SW_EDGE_CA = 5,
	RTK_SW_VERTEX_A = 6, RTK_SW_VERTEX_B = 7, RTK_SW_VERTEX_C = 8 };

// 0. the query and what is computed once from it
struct rtk_sweep_query {
	float O[3], D[3], tmin, tmax, r;
	float r2, dd, S[3];
};

// the centre at t
RTK_CLOSEST_FN void rtk_sweep_centre(const rtk_sweep_query &Q, float t, float *c)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	c[0] = RTK_CL_ADD(Q.O[0], RTK_CL_MUL(Q.D[0], t));
	c[1] = RTK_CL_ADD(Q.O[1], RTK_CL_MUL(Q.D[1], t));
	c[2] = RTK_CL_ADD(Q.O[2], RTK_CL_MUL(Q.D[2], t));
}

// 0. w: the nine floats of a rtk_sphere_sweep. Returns whether the query is live; Q is filled either way
RTK_CLOSEST_FN bool rtk_sweep_prepare(const float *w, rtk_sweep_query &Q)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	Q.O[0] = w[0]; Q.O[1] = w[1]; Q.O[2] = w[2];
	Q.D[0] = w[3]; Q.D[1] = w[4]; Q.D[2] = w[5];
	Q.tmin = w[6]; Q.tmax = w[7]; Q.r = w[8];
	Q.r2 = RTK_CL_MUL(Q.r, Q.r);
	Q.dd = RTK_CL_DOT(Q.D[0], Q.D[1], Q.D[2], Q.D[0], Q.D[1], Q.D[2]);
	rtk_sweep_centre(Q, Q.tmin, Q.S);
	bool finite = true;
	for (int k = 0; k < 9; k++) finite = finite && RTK_SW_FINITE(w[k]);
	const bool moves = Q.D[0] != 0.0f || Q.D[1] != 0.0f || Q.D[2] != 0.0f;
	return finite && moves && Q.r >= 0.0f && Q.tmin <= Q.tmax;
}

// 1. the path against the box [lo, hi] grown by r: false = empty; te the entry time
RTK_CLOSEST_FN bool rtk_sweep_slab(const rtk_sweep_query &Q, const float *lo, const float *hi, float &te)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	float t0 = Q.tmin, t1 = Q.tmax;
	bool inside = true;
	for (int k = 0; k < 3; k++) {
		const float l = RTK_CL_SUB(lo[k], Q.r), h = RTK_CL_ADD(hi[k], Q.r);
		const float d = Q.D[k];
		if (d == 0.0f) inside = inside && l <= Q.O[k] && Q.O[k] <= h;
		else {
			const float tl = RTK_CL_DIV(RTK_CL_SUB(l, Q.O[k]), d), th = RTK_CL_DIV(RTK_CL_SUB(h, Q.O[k]), d);
			const float tn = d > 0.0f ? tl : th, tf = d > 0.0f ? th : tl;
			t0 = RTK_CL_MAX(t0, tn);
			t1 = RTK_CL_MIN(t1, tf);
		}
	}
	te = t0;
	return inside && t0 <= t1;
}

// the entry of 2. (iii): the path m + D * t (A = dot(D, D), B = dot(m, D)) against the ball of radius r about 0, by its closest
// approach. false if disc < 0 or a NaN (t is then a NaN)
RTK_CLOSEST_FN bool rtk_sweep_entry(const rtk_sweep_query &Q, const float *m, const float *D, float A, float B, float &t)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	const float t0 = RTK_CL_DIV(-B, A);
	const float m0 = RTK_CL_ADD(m[0], RTK_CL_MUL(D[0], t0)), m1 = RTK_CL_ADD(m[1], RTK_CL_MUL(D[1], t0)), m2 = RTK_CL_ADD(m[2], RTK_CL_MUL(D[2], t0));
	const float disc = RTK_CL_SUB(Q.r2, RTK_CL_DOT(m0, m1, m2, m0, m1, m2));
	t = RTK_CL_SUB(t0, RTK_SW_SQRT(RTK_CL_DIV(disc, A)));
	return disc >= 0.0f;
}

// an edge of 2. (iii): e = q - p, m = O' - p. Returns whether t is a valid time of the edge
RTK_CLOSEST_FN bool rtk_sweep_edge(const rtk_sweep_query &Q, const float *e, const float *m, float &t)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	const float ee = RTK_CL_DOT(e[0], e[1], e[2], e[0], e[1], e[2]);
	const float nd = RTK_CL_DOT(e[0], e[1], e[2], Q.D[0], Q.D[1], Q.D[2]);
	const float md = RTK_CL_DOT(e[0], e[1], e[2], m[0], m[1], m[2]);
	const float fd = RTK_CL_DIV(nd, ee), fm = RTK_CL_DIV(md, ee);
	const float Dp[3] = { RTK_CL_SUB(Q.D[0], RTK_CL_MUL(e[0], fd)), RTK_CL_SUB(Q.D[1], RTK_CL_MUL(e[1], fd)), RTK_CL_SUB(Q.D[2], RTK_CL_MUL(e[2], fd)) };
	const float mp[3] = { RTK_CL_SUB(m[0], RTK_CL_MUL(e[0], fm)), RTK_CL_SUB(m[1], RTK_CL_MUL(e[1], fm)), RTK_CL_SUB(m[2], RTK_CL_MUL(e[2], fm)) };
	const float A = RTK_CL_DOT(Dp[0], Dp[1], Dp[2], Dp[0], Dp[1], Dp[2]), B = RTK_CL_DOT(mp[0], mp[1], mp[2], Dp[0], Dp[1], Dp[2]);
	const bool real = rtk_sweep_entry(Q, mp, Dp, A, B, t);
	const float w = RTK_CL_ADD(md, RTK_CL_MUL(t, nd));
	return ee > 0.0f && A > 0.0f && real && 0.0f <= w && w <= ee && Q.tmin <= t && t <= Q.tmax;
}

// a vertex of 2. (iii): m = O' - p
RTK_CLOSEST_FN bool rtk_sweep_vertex(const rtk_sweep_query &Q, const float *m, float &t)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	const bool real = rtk_sweep_entry(Q, m, Q.D, Q.dd, RTK_CL_DOT(m[0], m[1], m[2], Q.D[0], Q.D[1], Q.D[2]), t);
	return real && Q.tmin <= t && t <= Q.tmax;
}

// 2. the ball against the triangle (a, b, c): the feature (RTK_SW_NONE: no time) and the time by (iv)
RTK_CLOSEST_FN int rtk_sweep_triangle(const rtk_sweep_query &Q, const float *a, const float *b, const float *c, float &t_out)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	t_out = Q.tmax;
	// (i)
	const float lo[3] = { RTK_CL_MIN(RTK_CL_MIN(a[0], b[0]), c[0]), RTK_CL_MIN(RTK_CL_MIN(a[1], b[1]), c[1]), RTK_CL_MIN(RTK_CL_MIN(a[2], b[2]), c[2]) };
	const float hi[3] = { RTK_CL_MAX(RTK_CL_MAX(a[0], b[0]), c[0]), RTK_CL_MAX(RTK_CL_MAX(a[1], b[1]), c[1]), RTK_CL_MAX(RTK_CL_MAX(a[2], b[2]), c[2]) };
	float te;
	if (!rtk_sweep_slab(Q, lo, hi, te)) return RTK_SW_NONE;
	// (ii)
	float q[3], u, v;
	int region;
	const float dist2 = rtk_closest_triangle(Q.S, a, b, c, q, u, v, region);
	if (dist2 <= Q.r2) { t_out = RTK_CL_MAX(Q.tmin, te); return RTK_SW_START; }
	// (iii), from the centre at te: R is the query moved there
	rtk_sweep_query R = Q;
	rtk_sweep_centre(Q, te, R.O);
	R.tmin = RTK_CL_SUB(Q.tmin, te);
	R.tmax = RTK_CL_SUB(Q.tmax, te);
	int feature = RTK_SW_NONE;
	float best = 0.0f, t;
	const float ab[3] = { RTK_CL_SUB(b[0], a[0]), RTK_CL_SUB(b[1], a[1]), RTK_CL_SUB(b[2], a[2]) };
	const float ma[3] = { RTK_CL_SUB(R.O[0], a[0]), RTK_CL_SUB(R.O[1], a[1]), RTK_CL_SUB(R.O[2], a[2]) };
	{
		const float ac[3] = { RTK_CL_SUB(c[0], a[0]), RTK_CL_SUB(c[1], a[1]), RTK_CL_SUB(c[2], a[2]) };
		const float n0 = RTK_CL_SUB(RTK_CL_MUL(ab[1], ac[2]), RTK_CL_MUL(ab[2], ac[1]));
		const float n1 = RTK_CL_SUB(RTK_CL_MUL(ab[2], ac[0]), RTK_CL_MUL(ab[0], ac[2]));
		const float n2 = RTK_CL_SUB(RTK_CL_MUL(ab[0], ac[1]), RTK_CL_MUL(ab[1], ac[0]));
		const float nn = RTK_CL_DOT(n0, n1, n2, n0, n1, n2);
		const float len = RTK_SW_SQRT(nn);
		const float h0 = RTK_CL_DOT(n0, n1, n2, ma[0], ma[1], ma[2]), hd = RTK_CL_DOT(n0, n1, n2, R.D[0], R.D[1], R.D[2]);
		const float hs = RTK_CL_ADD(h0, RTK_CL_MUL(R.tmin, hd));
		const float sr = hs < 0.0f ? -R.r : R.r;
		t = RTK_CL_DIV(RTK_CL_SUB(RTK_CL_MUL(sr, len), h0), hd);
		if (nn > 0.0f && hd != 0.0f && R.tmin <= t && t <= R.tmax) {
			float ct[3];
			rtk_sweep_centre(R, t, ct);
			(void)rtk_closest_triangle(ct, a, b, c, q, u, v, region);
			if (region == 7) { feature = RTK_SW_FACE; best = t; }
		}
	}
	const float mb[3] = { RTK_CL_SUB(R.O[0], b[0]), RTK_CL_SUB(R.O[1], b[1]), RTK_CL_SUB(R.O[2], b[2]) };
	const float mc[3] = { RTK_CL_SUB(R.O[0], c[0]), RTK_CL_SUB(R.O[1], c[1]), RTK_CL_SUB(R.O[2], c[2]) };
	const float bc[3] = { RTK_CL_SUB(c[0], b[0]), RTK_CL_SUB(c[1], b[1]), RTK_CL_SUB(c[2], b[2]) };
	const float ca[3] = { RTK_CL_SUB(a[0], c[0]), RTK_CL_SUB(a[1], c[1]), RTK_CL_SUB(a[2], c[2]) };
	if (rtk_sweep_edge(R, ab, ma, t) && (feature == RTK_SW_NONE || t < best)) { feature = RTK_SW_EDGE_AB; best = t; }
	if (rtk_sweep_edge(R, bc, mb, t) && (feature == RTK_SW_NONE || t < best)) { feature = RTK_SW_EDGE_BC; best = t; }
	if (rtk_sweep_edge(R, ca, mc, t) && (feature == RTK_SW_NONE || t < best)) { feature = RTK_SW_EDGE_CA; best = t; }
	if (rtk_sweep_vertex(R, ma, t) && (feature == RTK_SW_NONE || t < best)) { feature = RTK_SW_VERTEX_A; best = t; }
	if (rtk_sweep_vertex(R, mb, t) && (feature == RTK_SW_NONE || t < best)) { feature = RTK_SW_VERTEX_B; best = t; }
	if (rtk_sweep_vertex(R, mc, t) && (feature == RTK_SW_NONE || t < best)) { feature = RTK_SW_VERTEX_C; best = t; }
	// (iv)
	if (feature != RTK_SW_NONE) {
		const float time = RTK_CL_ADD(te, best), late = RTK_CL_MAX(time, te);
		if (late > Q.tmax) feature = RTK_SW_NONE;
		else t_out = late;
	}
	return feature;
}

// 3. does (t, prim) beat (best_t, best_prim)? ... and may what lies behind the entry time te be left out?
RTK_CLOSEST_FN bool rtk_sweep_better(float t, uint32_t prim, float best_t, uint32_t best_prim)
{
	return t < best_t || (t == best_t && prim < best_prim);
}
RTK_CLOSEST_FN bool rtk_sweep_skip(float te, float best_t) { return te > best_t; }
