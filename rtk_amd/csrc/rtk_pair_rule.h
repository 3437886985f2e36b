// rtk_pair_rule.h -- the one rule by which "the closest triangle to a triangle" is answered (rtk_dev_closest_triangles,
// rtk_amd.h), for the host and the device: the kernel (rtk_pair.hip) and tests/pair_rule_driver.cpp include this file, and
// nothing else decides a bit of a result. tests/pair_ref.py restates it in numpy. The result is a pure function of the scene's
// triangle records and the query; the tree only decides how few of the records are looked at, and the order of the walk decides
// nothing.
//
// All arithmetic is float32. Every product, sum, difference and quotient below is ONE float operation, rounded on its own, in
// the order written: no fused multiply-add anywhere (rtk_closest_rule.h says how that is kept on the device and on the host; its
// macros are used here). Denormal inputs and results are kept. min(x, y) is "y < x ? y : x", max(x, y) is "y > x ? y : x",
// clamp(x, lo, hi) is "x < lo ? lo : (x > hi ? hi : x)", clamp01(x) is clamp(x, 0, 1): selects, so a NaN stays a NaN.
// dot(x, y) = (x0 * y0 + x1 * y1) + x2 * y2; the cross product is rtk_touch_rule.h's (two products and one difference per
// component). The query triangle is A = (a0, a1, a2); a scene record is B = (b0, b1, b2), its vertices as the scene holds them.
// Edge i of a triangle runs from vertex i to vertex (i + 1) % 3: ea_i = a_(i+1) - a_i, eb_j = b_(j+1) - b_j (rtk_touch_edges).
// alo / ahi are the componentwise min / max of A's vertices (min(min(a0, a1), a2)), blo / bhi the same of B's.
//
// 1. LIVE (rtk_touch_live). The query is live iff its nine numbers are finite. A query without area (a segment, a point) is
//    live and is a supported use. A query that is not live is a miss; so is a query whose max_dist2 is NaN, zero or negative
//    (!(max_dist2 > 0)), and so is any query of a scene without triangles.
// 2. FIFTEEN FEATURE PAIRS (rtk_pair_evaluate), numbered 0 .. 14 in this order. Each gives a point qa on A, a point qb on B,
//    dist2, and u, v, the weights of b0 and b1 at qb:
//      0, 1, 2   a_k against B: rtk_closest_triangle(a_k, b0, b1, b2) as it is. qa = a_k (inside A's box as it stands), qb = its
//                clamped point q, dist2, u and v are what it returns.
//      3, 4, 5   b_k against A: rtk_closest_triangle(b_k, a0, a1, a2) as it is. qa = its clamped point q, qb = b_k, dist2 is
//                what it returns (its e is qb - qa; the squares are those of qa - qb). (u, v) = (1, 0), (0, 1), (0, 0).
//      6 + 3 i + j   edge i of A against edge j of B, i outer and j inner (rtk_pair_segments). With p1 = a_i, d1 = ea_i,
//                p2 = b_j, d2 = eb_j:
//                    r = p1 - p2    a = dot(d1, d1)   e = dot(d2, d2)   f = dot(d2, r)   c = dot(d1, r)   b = dot(d1, d2)
//                    denom = a * e - b * b
//                    s0 = denom > 0 ? clamp01((b * f - c * e) / denom) : 0            (parallel, or an edge without length: 0)
//                    t0 = e > 0 ? (b * s0 + f) / e : 0
//                    low = !(e > 0) || t0 < 0        high = e > 0 && t0 > 1
//                    s1 = a > 0 ? clamp01((low ? -c : b - c) / a) : 0
//                    s = low || high ? s1 : s0       t = low ? 0 : (high ? 1 : t0)
//                A quotient whose divisor the select rules out is formed with the divisor 1: NOTHING IS EVER DECIDED BY 0 / 0, and
//                there is no epsilon: a zero (or negative, or NaN) denom, a and e take the stated branch.
//                    qa = clamp(a_i + ea_i * s, alo, ahi)    qb = clamp(b_j + eb_j * t, blo, bhi)     (componentwise)
//                    g = qa - qb      dist2 = (g0 * g0 + g1 * g1) + g2 * g2
//                (u, v) = (1 - t, t) for j = 0, (0, 1 - t) for j = 1, (t, 0) for j = 2.
//    The clamp of qa to A's own box and of qb to B's own box is part of the rule: it is what makes the skip of 6. exact.
//    THE PAIR'S RESULT is the feature with the smallest dist2, THE FIRST IN THIS ORDER AMONG EQUAL ONES: it starts as
//    (dist2 = +infinity, u = v = 0, qa = a0, qb = b0, feature 15) and feature k replaces it iff dist2_k < dist2, strictly. A NaN
//    dist2 never wins. (rtk_closest_triangle can answer NaN for a triangle with two equal vertices: the edge features, which
//    divide by nothing they have not looked at, then carry the pair.)
// 3. PIERCING (rtk_pair_edge_pierces), before 2. The fifteen features miss two triangles that cross through each other's
//    interiors, whose true distance is 0. Six tests in this order: edges 0, 1, 2 of A against B, then edges 0, 1, 2 of B against
//    A (features 16 .. 21). For the edge from p to q with d = q - p (the triangle's stored edge vector) and the triangle
//    (v0, v1, v2) with n = e0 X e1:
//        dp = dot(n, p - v0)    dq = dot(n, q - v0)      opposite = (dp > 0 && dq < 0) || (dp < 0 && dq > 0)
//        w_k = v_k - p          s_0 = dot(d, w_0 X w_1)  s_1 = dot(d, w_1 X w_2)  s_2 = dot(d, w_2 X w_0)
//        inside = ((s_0 >= 0 && s_1 >= 0 && s_2 >= 0) || (s_0 <= 0 && s_1 <= 0 && s_2 <= 0)) && (s_0 != 0 || s_1 != 0 || s_2 != 0)
//    The edge pierces iff opposite && inside: STRICTLY OPPOSITE SIGNS of dp and dq; of the three triple products zero counts as
//    either sign, but not all three may be zero. A triangle without area has n = 0 and is never pierced; a zero-length edge has
//    dp == dq and never pierces; a NaN fails every comparison it stands in. A CROSSING COUNTS ONLY IF THE TWO TRIANGLES' OWN
//    BOXES TOUCH by the closed comparisons of rtk_box_boxes_touch (blo <= ahi && bhi >= alo on all three axes): that keeps the
//    bound of every box above B at 0. The seventeen axes of rtk_touch_rule.h are NOT used: they may keep a segment that passes
//    beside a triangle in its plane, and a segment must get its true distance here.
//    A PIERCED PAIR has dist2 = 0.0f and qa = qb = x, THE FIRST PIERCING EDGE IN THIS ORDER deciding:
//        t = dp / (dp - dq)     x = clamp(p + d * t, max(alo, blo), min(ahi, bhi))      (componentwise; the boxes' intersection)
//    (u, v): an edge j of B at t as in 2.; an edge of A through B: sum = (s_0 + s_1) + s_2, u = s_1 / sum, v = s_2 / sum.
// 4. FILTER, part of the rule: rtk_touch_filter_passes of rtk_touch_rule.h as it is (first_prim, and
//    RTK_TOUCH_SKIP_SHARED_VERTEX), applied to the record's global primitive id and stored positions. The flag together with
//    first_prim = own id + 1 gives each triangle of a mesh its nearest non-adjacent triangle of a higher id: self-clearance.
// 5. ANSWER. Over ALL records that pass 4. and whose dist2 < max_dist2 -- strictly --, the best by rtk_closest_better: the
//    smallest dist2, THE LOWEST PRIMITIVE ID among equal dist2. Otherwise the query is a miss. The record is
//    rtk_closest_record's {dist2, u, v, prim}; the two points are qa and qb.
// 6. BOX BOUND (rtk_pair_box_bound) of a node box [lo, hi] against A's box, per axis
//        g = max(max(lo - ahi, alo - hi), 0)       bound = (g0 * g0 + g1 * g1) + g2 * g2
//    subtractions and selects, then the operations of dist2 in the same order. A subtree (or a record, by its own box) is
//    SKIPPED iff bound > best2 -- strictly: an equal bound can hide a lower id -- or bound >= max_dist2 (rtk_pair_skip). A NaN
//    bound is not skipped. bound <= dist2 HOLDS FOR EVERY RECORD BELOW THE BOX, WITHOUT A MARGIN: qa lies in A's box (a vertex
//    of A, or clamped to it), qb lies in B's box (likewise), and B's box lies inside every box above B because both are selects
//    of the stored coordinates. On an axis with lo - ahi > 0 we have qa <= ahi < lo <= qb, so qb - qa >= lo - ahi in real
//    numbers; a rounded difference is monotone and |fl(qa - qb)| = fl(qb - qa), so |g_dist| >= g_bound; the mirror image for
//    alo - hi > 0; otherwise g_bound is 0. A rounded square and a rounded sum of non-negative numbers are monotone, hence
//    bound <= dist2. A pierced pair has dist2 = 0 and touching own boxes: lo <= blo <= ahi and alo <= bhi <= hi, so both
//    differences are <= 0 on every axis and the bound of every box above it is 0 as well.
//
// WHAT THE RULE IS AND IS NOT. It is a FLOAT RULE and the result is DEFINED BY IT. In exact arithmetic two triangles in one
// plane that overlap, or that touch without an edge of one going strictly through the other, are not pierced: their dist2 is
// the features' (0 or a rounding error). In floats the dp, dq and s_k of two triangles that lie in one plane up to rounding are
// rounding errors of either sign, and 3. can then call such a pair pierced: IF ITS OWN BOXES TOUCH, A PAIR IN ONE PLANE CAN GET
// dist2 = 0 ALTHOUGH THE TWO ARE APART (by less than their boxes' extent; on exact inputs, integers say, never). The accuracy
// figure below does not cover such pairs. A scene with NON-FINITE vertex coordinates: the call terminates and writes only inside its outputs; NOTHING
// ELSE IS PROMISED about its results.
//
// Accuracy, measured against the same walk (features and piercing) in float64 over 8 million random pairs (7.8 million once slivers are left out; scripts/pair_accuracy.py) at the five
// combinations of triangle size and distance that rtk_closest_rule.h uses (both triangles of the stated size, their distance
// of the stated offset; slivers -- smallest height below a twentieth of the longest edge -- and degenerate triangles left out,
// and not measured): |sqrt(dist2) - exact| stayed within 1.47 * 2^-23 of the largest coordinate magnitude
// involved. tests/test_pair_cpu.py asserts 3.7 * 2^-23.
#pragma once

#include "rtk_touch_rule.h"        // rtk_touch_live, rtk_touch_edges, rtk_touch_cross, rtk_touch_filter_passes; through it
                                   // rtk_box_boxes_touch and rtk_closest_triangle, rtk_closest_better and the macros

#define RTK_PAIR_CLAMP01(x) ((x) < 0.0f ? 0.0f : ((x) > 1.0f ? 1.0f : (x)))
#define RTK_PAIR_FEATURE_NONE 15
#define RTK_PAIR_FEATURE_PIERCE 16     // + 0, 1, 2: that edge of A through B; + 3, 4, 5: edge 0, 1, 2 of B through A

// what is formed once per query: A's vertices, box, edges, their squared lengths and nA
struct rtk_pair_hoist {
	float a[3][3];
	float lo[3], hi[3];
	float e[3][3];                 // ea0, ea1, ea2
	float ee[3];                   // dot(ea_i, ea_i)
	float n[3];                    // nA = ea0 X ea1
};

// the result of one pair
struct rtk_pair_result {
	float dist2, u, v;
	float qa[3], qb[3];
	int feature;                   // 0 .. 14, RTK_PAIR_FEATURE_NONE, or RTK_PAIR_FEATURE_PIERCE + 0 .. 5
};

RTK_CLOSEST_FN void rtk_pair_box(const float *v0, const float *v1, const float *v2, float *lo, float *hi)
{
	for (int x = 0; x < 3; x++) {
		const float m0 = RTK_CL_MIN(v0[x], v1[x]), m1 = RTK_CL_MAX(v0[x], v1[x]);
		lo[x] = RTK_CL_MIN(m0, v2[x]);
		hi[x] = RTK_CL_MAX(m1, v2[x]);
	}
}

RTK_CLOSEST_FN void rtk_pair_hoist_query(const float *a0, const float *a1, const float *a2, rtk_pair_hoist &h)
{
	for (int x = 0; x < 3; x++) { h.a[0][x] = a0[x]; h.a[1][x] = a1[x]; h.a[2][x] = a2[x]; }
	rtk_pair_box(a0, a1, a2, h.lo, h.hi);
	rtk_touch_edges(a0, a1, a2, h.e);
	for (int i = 0; i < 3; i++) h.ee[i] = RTK_CL_DOT(h.e[i][0], h.e[i][1], h.e[i][2], h.e[i][0], h.e[i][1], h.e[i][2]);
	rtk_touch_cross(h.e[0], h.e[1], h.n);
}

// 2. the segment from p1 along d1 (a = dot(d1, d1)) against the segment from p2 along d2 (e = dot(d2, d2)): s and t
RTK_CLOSEST_FN void rtk_pair_segments(const float *p1, const float *d1, float a, const float *p2, const float *d2, float e, float &s, float &t)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	const float r0 = RTK_CL_SUB(p1[0], p2[0]), r1 = RTK_CL_SUB(p1[1], p2[1]), r2 = RTK_CL_SUB(p1[2], p2[2]);
	const float f = RTK_CL_DOT(d2[0], d2[1], d2[2], r0, r1, r2);
	const float c = RTK_CL_DOT(d1[0], d1[1], d1[2], r0, r1, r2);
	const float b = RTK_CL_DOT(d1[0], d1[1], d1[2], d2[0], d2[1], d2[2]);
	const float denom = RTK_CL_SUB(RTK_CL_MUL(a, e), RTK_CL_MUL(b, b));
	const bool cross = denom > 0.0f, epos = e > 0.0f, apos = a > 0.0f;
	const float x0 = RTK_CL_DIV(RTK_CL_SUB(RTK_CL_MUL(b, f), RTK_CL_MUL(c, e)), cross ? denom : 1.0f);
	const float s0 = cross ? RTK_PAIR_CLAMP01(x0) : 0.0f;
	const float y0 = RTK_CL_DIV(RTK_CL_ADD(RTK_CL_MUL(b, s0), f), epos ? e : 1.0f);
	const float t0 = epos ? y0 : 0.0f;
	const bool low = !epos || t0 < 0.0f, high = epos && t0 > 1.0f;
	const float x1 = RTK_CL_DIV(low ? -c : RTK_CL_SUB(b, c), apos ? a : 1.0f);
	const float s1 = apos ? RTK_PAIR_CLAMP01(x1) : 0.0f;
	s = (low || high) ? s1 : s0;
	t = low ? 0.0f : (high ? 1.0f : t0);
}

// 3. does the edge from p along d to q pierce the triangle (v0, v1, v2) of normal n? t = dp / (dp - dq), s[3] the triple products
RTK_CLOSEST_FN bool rtk_pair_edge_pierces(const float *p, const float *q, const float *d, const float *v0, const float *v1, const float *v2,
	const float *n, float &t, float *s)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	const float dp = RTK_CL_DOT(n[0], n[1], n[2], RTK_CL_SUB(p[0], v0[0]), RTK_CL_SUB(p[1], v0[1]), RTK_CL_SUB(p[2], v0[2]));
	const float dq = RTK_CL_DOT(n[0], n[1], n[2], RTK_CL_SUB(q[0], v0[0]), RTK_CL_SUB(q[1], v0[1]), RTK_CL_SUB(q[2], v0[2]));
	const bool opposite = (dp > 0.0f && dq < 0.0f) || (dp < 0.0f && dq > 0.0f);
	t = 0.0f; s[0] = s[1] = s[2] = 0.0f;
	if (!opposite) return false;
	float w0[3], w1[3], w2[3], m[3];
	for (int x = 0; x < 3; x++) { w0[x] = RTK_CL_SUB(v0[x], p[x]); w1[x] = RTK_CL_SUB(v1[x], p[x]); w2[x] = RTK_CL_SUB(v2[x], p[x]); }
	rtk_touch_cross(w0, w1, m); s[0] = RTK_CL_DOT(d[0], d[1], d[2], m[0], m[1], m[2]);
	rtk_touch_cross(w1, w2, m); s[1] = RTK_CL_DOT(d[0], d[1], d[2], m[0], m[1], m[2]);
	rtk_touch_cross(w2, w0, m); s[2] = RTK_CL_DOT(d[0], d[1], d[2], m[0], m[1], m[2]);
	const bool inside = ((s[0] >= 0.0f && s[1] >= 0.0f && s[2] >= 0.0f) || (s[0] <= 0.0f && s[1] <= 0.0f && s[2] <= 0.0f))
		&& (s[0] != 0.0f || s[1] != 0.0f || s[2] != 0.0f);
	t = RTK_CL_DIV(dp, RTK_CL_SUB(dp, dq));
	return inside;
}

// 2. (u, v) of the point at t on edge j of B
RTK_CLOSEST_FN void rtk_pair_edge_weights(int j, float t, float &u, float &v)
{
	const float w = RTK_CL_SUB(1.0f, t);
	u = j == 0 ? w : (j == 1 ? 0.0f : t);
	v = j == 0 ? t : (j == 1 ? w : 0.0f);
}

// 3. test k of the six: if the edge from p along d to q pierces (v0, v1, v2), r becomes the pierced pair's result
RTK_CLOSEST_FN bool rtk_pair_pierced(int k, const float *p, const float *q, const float *d, const float *v0, const float *v1, const float *v2,
	const float *n, const float *ilo, const float *ihi, rtk_pair_result &r)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	float t, s[3];
	if (!rtk_pair_edge_pierces(p, q, d, v0, v1, v2, n, t, s)) return false;
	for (int x = 0; x < 3; x++) {
		const float at = RTK_CL_ADD(p[x], RTK_CL_MUL(d[x], t));
		r.qa[x] = r.qb[x] = RTK_CL_CLAMP(at, ilo[x], ihi[x]);
	}
	if (k < 3) {
		const float sum = RTK_CL_ADD(RTK_CL_ADD(s[0], s[1]), s[2]);
		r.u = RTK_CL_DIV(s[1], sum); r.v = RTK_CL_DIV(s[2], sum);
	} else rtk_pair_edge_weights(k - 3, t, r.u, r.v);
	r.dist2 = 0.0f; r.feature = RTK_PAIR_FEATURE_PIERCE + k;
	return true;
}

// 2. and 3.: one pair, h from rtk_pair_hoist_query of a LIVE query
RTK_CLOSEST_FN void rtk_pair_evaluate(const rtk_pair_hoist &h, const float *b0, const float *b1, const float *b2, rtk_pair_result &r)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	const float *const bv[3] = { b0, b1, b2 };
	float blo[3], bhi[3], eb[3][3];
	rtk_pair_box(b0, b1, b2, blo, bhi);
	rtk_touch_edges(b0, b1, b2, eb);
	r.dist2 = __builtin_huge_valf(); r.u = 0.0f; r.v = 0.0f; r.feature = RTK_PAIR_FEATURE_NONE;
	for (int x = 0; x < 3; x++) { r.qa[x] = h.a[0][x]; r.qb[x] = b0[x]; }

	// 3. piercing, if the two boxes touch: six calls with constant indices, so that nothing is addressed through a selected pointer
	if (rtk_box_boxes_touch(b0, b1, b2, h.lo, h.hi)) {
		float nb[3], ilo[3], ihi[3];
		rtk_touch_cross(eb[0], eb[1], nb);
		for (int x = 0; x < 3; x++) { ilo[x] = RTK_CL_MAX(h.lo[x], blo[x]); ihi[x] = RTK_CL_MIN(h.hi[x], bhi[x]); }
		if (rtk_pair_pierced(0, h.a[0], h.a[1], h.e[0], b0, b1, b2, nb, ilo, ihi, r)) return;
		if (rtk_pair_pierced(1, h.a[1], h.a[2], h.e[1], b0, b1, b2, nb, ilo, ihi, r)) return;
		if (rtk_pair_pierced(2, h.a[2], h.a[0], h.e[2], b0, b1, b2, nb, ilo, ihi, r)) return;
		if (rtk_pair_pierced(3, b0, b1, eb[0], h.a[0], h.a[1], h.a[2], h.n, ilo, ihi, r)) return;
		if (rtk_pair_pierced(4, b1, b2, eb[1], h.a[0], h.a[1], h.a[2], h.n, ilo, ihi, r)) return;
		if (rtk_pair_pierced(5, b2, b0, eb[2], h.a[0], h.a[1], h.a[2], h.n, ilo, ihi, r)) return;
	}

	// 2. the fifteen features
	for (int k = 0; k < 3; k++) {
		float q[3], u, v;
		int region;
		const float d2 = rtk_closest_triangle(h.a[k], b0, b1, b2, q, u, v, region);
		if (d2 < r.dist2) {
			r.dist2 = d2; r.u = u; r.v = v; r.feature = k;
			for (int x = 0; x < 3; x++) { r.qa[x] = h.a[k][x]; r.qb[x] = q[x]; }
		}
	}
	for (int k = 0; k < 3; k++) {
		float q[3], u, v;
		int region;
		const float d2 = rtk_closest_triangle(bv[k], h.a[0], h.a[1], h.a[2], q, u, v, region);
		if (d2 < r.dist2) {
			r.dist2 = d2; r.u = k == 0 ? 1.0f : 0.0f; r.v = k == 1 ? 1.0f : 0.0f; r.feature = 3 + k;
			for (int x = 0; x < 3; x++) { r.qa[x] = q[x]; r.qb[x] = bv[k][x]; }
		}
	}
	float ebb[3];
	for (int j = 0; j < 3; j++) ebb[j] = RTK_CL_DOT(eb[j][0], eb[j][1], eb[j][2], eb[j][0], eb[j][1], eb[j][2]);
	for (int i = 0; i < 3; i++) {
		for (int j = 0; j < 3; j++) {
			float s, t, qa[3], qb[3], g[3];
			rtk_pair_segments(h.a[i], h.e[i], h.ee[i], bv[j], eb[j], ebb[j], s, t);
			for (int x = 0; x < 3; x++) {
				const float pa = RTK_CL_ADD(h.a[i][x], RTK_CL_MUL(h.e[i][x], s)), pb = RTK_CL_ADD(bv[j][x], RTK_CL_MUL(eb[j][x], t));
				qa[x] = RTK_CL_CLAMP(pa, h.lo[x], h.hi[x]);
				qb[x] = RTK_CL_CLAMP(pb, blo[x], bhi[x]);
				g[x] = RTK_CL_SUB(qa[x], qb[x]);
			}
			const float d2 = RTK_CL_ADD(RTK_CL_ADD(RTK_CL_MUL(g[0], g[0]), RTK_CL_MUL(g[1], g[1])), RTK_CL_MUL(g[2], g[2]));
			if (d2 < r.dist2) {
				r.dist2 = d2; r.feature = 6 + 3 * i + j;
				rtk_pair_edge_weights(j, t, r.u, r.v);
				for (int x = 0; x < 3; x++) { r.qa[x] = qa[x]; r.qb[x] = qb[x]; }
			}
		}
	}
}

// 6. the box [lo, hi] against A's box [alo, ahi]: the bound no record inside the box comes below
RTK_CLOSEST_FN float rtk_pair_box_bound(const float *lo, const float *hi, const float *alo, const float *ahi)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	float g[3];
	for (int x = 0; x < 3; x++) {
		const float x1 = RTK_CL_SUB(lo[x], ahi[x]), x2 = RTK_CL_SUB(alo[x], hi[x]);
		const float m = RTK_CL_MAX(x1, x2);
		g[x] = RTK_CL_MAX(m, 0.0f);
	}
	return RTK_CL_ADD(RTK_CL_ADD(RTK_CL_MUL(g[0], g[0]), RTK_CL_MUL(g[1], g[1])), RTK_CL_MUL(g[2], g[2]));
}

// 6. may what lies behind `bound` be left out? (a NaN bound: no)
RTK_CLOSEST_FN bool rtk_pair_skip(float bound, float best2, float max_dist2) { return bound > best2 || bound >= max_dist2; }

// 4. and 5.: is the record (its pair result in r) a candidate that beats (best2, best_prim)?
RTK_CLOSEST_FN bool rtk_pair_wins(float dist2, uint32_t prim, float max_dist2, float best2, uint32_t best_prim)
{
	return dist2 < max_dist2 && rtk_closest_better(dist2, prim, best2, best_prim);
}
