// rtk_capsule_rule.h -- the one rule by which a capsule sweep is answered (rtk_dev_sweep_capsules, rtk_amd.h), for the host and
// the device: the kernel (rtk_capsule.hip) and tests/capsule_rule_driver.cpp include this file and nothing else decides a bit of
// a result. tests/capsule_ref.py restates it in numpy. THE RESULT DOES NOT DEPEND ON THE TREE: it is a pure function of the
// scene's triangle records, the filter and the query; the tree only decides how few of the records are looked at.
//
// Every product, sum, difference, quotient and square root below is ONE float operation, rounded on its own, in the order
// written: no fused multiply-add anywhere (rtk_sweep_rule.h and rtk_closest_rule.h say how that is kept on the device and on the
// host; their macros are used here). Denormal inputs and results are kept. min, max, clamp and clamp01 are the selects of
// rtk_pair_rule.h; |x| is "x < 0 ? -x : x" (a NaN stays a NaN); dot and cross are those of rtk_sweep_rule.h. This file calls, AS
// THEY ARE, rtk_sweep_centre, rtk_sweep_entry, rtk_sweep_edge and rtk_sweep_vertex (rtk_sweep_rule.h), rtk_closest_triangle
// (rtk_closest_rule.h), rtk_pair_segments, rtk_pair_edge_pierces and rtk_pair_edge_weights (rtk_pair_rule.h); the sphere
// sweep's face step is inline in rtk_sweep_triangle and is restated here as rtk_capsule_face.
//
// 0. THE QUERY (rtk_capsule_prepare). O = origin, D = direction, r = radius, h = half_axis. The capsule at time t is every point
//    within r of the segment from c(t) - h to c(t) + h, c(t) = O + D * t (rtk_sweep_centre); it does not rotate; t runs over the
//    CLOSED interval [min_t, max_t]. A query is LIVE iff all twelve floats are finite (RTK_INF is a finite float: "no limit"),
//    D is not all zeros, r >= 0 and min_t <= max_t; a query that is not live is a miss. h == 0 is legal and is a ball, r == 0
//    is legal and is a moving segment, both at once is a point (NOT rtk's watertight ray test, not bit-equal to a trace).
//    Once per query: r2 = r * r, dd = dot(D, D), s = c(min_t) as the sphere sweep forms them; g[k] = r + |h[k]|, one sum per
//    axis; the start's end points p0 = s - h, p1 = s + h (one rounded difference and sum per component).
// 1. THE PATH AND A BOX (rtk_capsule_slab): rtk_sweep_rule.h 1. with g[k] in the place of the radius on axis k:
//        t0 = min_t, t1 = max_t; for k = 0, 1, 2:   l = lo[k] - g[k],  h = hi[k] + g[k]
//            D[k] == 0:   empty unless l <= O[k] && O[k] <= h
//            otherwise    tl = (l - O[k]) / D[k], th = (h - O[k]) / D[k];  D[k] > 0: t0 = max(t0, tl), t1 = min(t1, th)
//                                                                          D[k] < 0: t0 = max(t0, th), t1 = min(t1, tl)
//        empty unless t0 <= t1; the ENTRY TIME is te = t0. For a live query and finite boxes no operand is a NaN, hence neither is te.
//    THE BOUND carries over word for word, g[k] being a fixed number per axis: a box above a triangle contains the triangle's
//    own box (lo' <= lo, hi' >= hi). A rounded difference, a rounded sum and a rounded quotient by a fixed divisor are monotone,
//    and so are the selects: on every axis l' <= l and h' >= h, the containment test of the larger box holds where the smaller
//    one's does, the near plane's time of the larger box is <= and its far plane's time >= the smaller one's (for D[k] < 0 the
//    planes swap and the quotient reverses the order twice). So t0' <= t0 and t1' >= t1 EXACTLY: the larger box's interval is
//    empty only if the triangle's is, and its entry time never exceeds the triangle's te, WITHOUT A MARGIN. By 2. (ii) and (iv)
//    the triangle's time is >= its te: entry time <= time for every triangle below the box.
// 2. THE CAPSULE AND ONE TRIANGLE (rtk_capsule_triangle). a, b, c are DevTri.v0 / v1 / v2 as the scene holds them. A time or none:
//    (i)   OWN BOX: lo = min(min(a, b), c), hi = max(max(a, b), c) by 1.: empty means none; its entry time is te.
//    (ii)  START OVERLAP (rtk_capsule_distance at p0, p1). The squared distance of the segment [p0, p1] and the triangle, with
//          x = p1 - p0 (one rounded difference; the AXIS), xx = dot(x, x), slo = min(p0, p1), shi = max(p0, p1), and the
//          triangle's edges e0 = b - a, e1 = c - b, e2 = a - c (rtk_touch_edges), n = cross(e0, e1):
//            PIERCE  if the two boxes touch (lo <= shi && hi >= slo on all three axes, closed) and
//                    rtk_pair_edge_pierces(p0, p1, x, a, b, c, n) holds: dist2 = 0, both points are
//                    clamp(p0 + x * t, max(slo, lo), min(shi, hi)), sum = (s_0 + s_1) + s_2, u = s_1 / sum, v = s_2 / sum
//            otherwise the smallest of five values, THE FIRST AMONG EQUALS IN THIS ORDER (a later one replaces an earlier one
//            iff it is strictly smaller; the walk starts from dist2 = +infinity, u = v = 0, the triangle's point a, the axis
//            point p0; a NaN never wins):
//            END 0   rtk_closest_triangle(p0, a, b, c): its dist2, u, v and clamped point; the axis point is p0
//            END 1   rtk_closest_triangle(p1, a, b, c): likewise; the axis point is p1
//            EDGE j  for j = 0, 1, 2 (ab, bc, ca): rtk_pair_segments(p0, x, xx, v_j, e_j, dot(e_j, e_j)) gives s and t;
//                    qa = clamp(p0 + x * s, slo, shi), qb = clamp(v_j + e_j * t, lo, hi), f = qa - qb,
//                    dist2 = (f0 * f0 + f1 * f1) + f2 * f2, (u, v) by rtk_pair_edge_weights(j, t)
//          dist2 <= r2 (touching counts; a NaN does not): the time is max(min_t, te).
//          An axis PARALLEL to the triangle's plane, or IN it, has dp and dq of one sign or zero and is never a pierce (strictly
//          opposite signs are asked): such a start is decided by the five values, whose edge evaluations reach 0 where the axis
//          crosses the triangle's border and whose end evaluations reach 0 where an end lies on the triangle. h == 0 gives
//          x = 0: no pierce, the two ends are one point, the edges take the branch a == 0 of rtk_pair_segments. This is a different
//          float expression from the sphere sweep's start test: h == 0 IS NOT PROMISED BIT-EQUAL to rtk_dev_sweep_spheres.
//    (iii) FEATURES. Otherwise the smallest valid time of the 26 features of the prism T + [-h, +h], measured FROM THE CENTRE
//          AT te exactly as the sphere rule does: O' = c(te), lo_t = min_t - te, hi_t = max_t - te, c'(t) = O' + D * t. The
//          capsule touches T iff its centre is within r of that prism, and every feature below is a subset of the prism, so
//          none can report a time before the true contact. The six vertices, each ONE rounded difference or sum per component:
//              a- = a - h, b- = b - h, c- = c - h, a+ = a + h, b+ = b + h, c+ = c + h
//          The prism's surface is eight triangles: L = (a-, b-, c-), U = (a+, b+, c+), and for each edge pq in ab, bc, ca the
//          two halves of its parallelogram, the triangles p- q- q+ and p- q+ p+. The features IN THIS ORDER, THE FIRST AMONG
//          EQUAL TIMES (a later one replaces an earlier one iff its t is strictly smaller):
//          FACES     2 .. 9: L, U, ab's two halves, bc's two, ca's two. A HALF IS NAMED FROM THE CORNER AT WHICH ITS SIDE ALONG
//                    h STARTS, in the same sense of rotation: p- q- q+ is handed to the face step as (A, B, C) = (q-, q+, p-) and
//                    p- q+ p+ as (p+, p-, q+). Then AB = +-(p+ - p-) is the difference of two floats that differ by 2 h: it is
//                    exact or nearly so however short h is, AC is an edge, and the normal cross(AB, AC) has the relative
//                    error of its products unless h runs along the edge. Named (p-, q-, q+), AB and AC are two long vectors that
//                    differ by 2 h, each rounded at the size of the EDGE: the normal's direction is then known to 2^-23 *
//                    |edge| / |h| only, and for |h| below 1e-5 of the edge it is noise, the face step reported contacts that
//                    were not there (17 clear cases in the 3 million of the accuracy test) and the error reached a tenth
//                    of the largest coordinate. For the triangle (A, B, C), rtk_capsule_face:
//                    AB = B - A, AC = C - A, n = cross(AB, AC), nn = dot(n, n), len = sqrt(nn), m = O' - A, h0 = dot(n, m),
//                    hd = dot(n, D), hs = h0 + lo_t * hd, sr = hs < 0 ? -r : r, t = (sr * len - h0) / hd;
//                    valid iff nn > 0 && hd != 0 && lo_t <= t && t <= hi_t && rtk_closest_triangle(c'(t), A, B, C) ends in case 7
//          EDGES     10 .. 21 through rtk_sweep_edge(e = q - p, m = O' - p), p to q: L's three a- b-, b- c-, c- a-; U's three
//                    a+ b+, b+ c+, c+ a+; the three lateral ones a- a+, b- b+, c- c+; the three diagonals a- b+, b- c+, c- a+,
//                    which close the seam between a parallelogram's halves
//          VERTICES  22 .. 27 through rtk_sweep_vertex(m = O' - p): a-, b-, c-, a+, b+, c+
//          No valid feature: none. Degenerate pieces take the branches the called functions state and NOTHING IS DECIDED BY
//          0 / 0: a face without area has nn == 0 and is not valid; an edge without length has ee == 0 and is not valid (its
//          quotients are NaN or infinite and fail the comparisons); h == 0 makes L and U both T, the lateral faces and edges
//          empty and the diagonals T's edges: the first of the equal times wins and the time is the sphere rule's. h ALONG
//          AN EDGE pq makes that edge's parallelogram a segment (nn == 0 up to rounding; what area rounding leaves is a
//          sliver whose normal has few digits); its L and U edges, the lateral edges and the diagonal lie on one line and
//          carry it. h IN THE TRIANGLE'S PLANE makes the prism a flat polygon: L, U and the
//          parallelograms that are not empty cover it from both sides, with equal times of which the first wins. D parallel
//          to a face has hd == 0 (or a rounding error: then t is huge and fails the interval): that face is not valid and
//          the edges and vertices carry the contact. A NaN t fails lo_t <= t && t <= hi_t in every feature.
//    (iv)  THE TIME of a feature is max(te + t, te), as in rtk_sweep_rule.h 2. (iv). A time > max_t is NONE. No time outside
//          [min_t, max_t] is ever reported (te >= min_t, and te <= max_t where the interval is not empty).
// 3. BETTER THAN: rtk_sweep_better and rtk_sweep_skip of rtk_sweep_rule.h unchanged. (t, prim) beats (best_t, best_prim) iff
//    t < best_t || (t == best_t && prim < best_prim): THE LOWEST PRIMITIVE ID WINS AMONG EQUAL TIMES; a NaN never beats anything;
//    a subtree may be skipped iff its interval by 1. is empty or te > best_t, strictly.
// The answer is the best (t, prim) by 3. over ALL triangle records that pass the filter and have a time, starting from
// (max_t, RTK_PRIM_NONE), or a miss. THE RECORD (rtk_capsule_record): ONE evaluation of the distance walk of (ii) at
// c(best_t) -- end points c(best_t) - h and c(best_t) + h -- on the answer's triangle gives u, v, the point on the triangle and
// the point on the axis: those of the winning item, or the pierce point for both. If every one of the five values is a NaN
// (a triangle with two equal vertices can do that to the end evaluations, never to all three edges of a finite triangle) the
// walk's starting values are reported.
// A scene with NON-FINITE vertex coordinates: every loop here has a fixed count, so the call terminates; NOTHING ELSE IS PROMISED.
//
// Accuracy of 2., measured against the same features in float64 (tests/test_capsule_cpu.py) over 3 million random (triangle,
// path, radius, half axis) cases at the five combinations of triangle size, start distance and radius of rtk_sweep_rule.h,
// the half axis in a random direction and from nothing up to four times the largest radius long, on the 0.72 million that
// have a time from a feature in both (slivers -- T's smallest altitude below a hundredth of its longest edge; the prism's
// lateral faces are not looked at, however thin --, degenerate triangles, contacts grazing within 3 degrees and starts that
// overlap left out, and not measured): |t - exact| * |D| stayed within 25.50 * 2^-23 of the largest coordinate magnitude
// involved; the test asserts 64 * 2^-23. float32 and float64 disagreed about hit or none on none of the 3 million cases.
// What is not covered: a half axis within a fraction of a degree of an edge's direction, whose parallelogram is a sliver in
// the plain sense; its faces' normals lose digits in proportion to 1 / sin of that angle.
#pragma once

#include "rtk_sweep_rule.h"
#include "rtk_pair_rule.h"

// (fixed-count loops whose bodies index V by constants once unrolled; the host compiler needs no telling)
#if defined(__HIPCC__)
#define RTK_CP_UNROLL _Pragma("unroll")
#else
#define RTK_CP_UNROLL
#endif

// what 2. found: none, the start overlap, or the feature that gave the time
enum { RTK_CP_NONE = 0, RTK_CP_START = 1, RTK_CP_FACE = 2 /* .. 9 */, RTK_CP_EDGE = 10 /* .. 21 */, RTK_CP_VERTEX = 22 /* .. 27 */,
	RTK_CP_FEATURES = 28 };
// the deciding item of the distance walk of 2. (ii)
enum { RTK_CP_ITEM_NONE = 0, RTK_CP_ITEM_PIERCE = 1, RTK_CP_ITEM_END0 = 2, RTK_CP_ITEM_END1 = 3, RTK_CP_ITEM_EDGE = 4 /* .. 6 */ };

// 0. the query and what is computed once from it: S is the sphere sweep's query (O, D, tmin, tmax, r, r2, dd, S = c(min_t))
struct rtk_capsule_query {
	rtk_sweep_query S;
	float h[3], g[3];
	float p0[3], p1[3];            // the start's end points
};

struct rtk_capsule_contact {
	float dist2, u, v;
	float qt[3], qa[3];            // the point on the triangle, the point on the axis
	int item;
};

// 0. w: the twelve floats of a rtk_capsule_sweep. Returns whether the query is live; Q is filled either way
RTK_CLOSEST_FN bool rtk_capsule_prepare(const float *w, rtk_capsule_query &Q)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	Q.S.O[0] = w[0]; Q.S.O[1] = w[1]; Q.S.O[2] = w[2];
	Q.S.D[0] = w[3]; Q.S.D[1] = w[4]; Q.S.D[2] = w[5];
	Q.S.tmin = w[6]; Q.S.tmax = w[7]; Q.S.r = w[8];
	Q.S.r2 = RTK_CL_MUL(Q.S.r, Q.S.r);
	Q.S.dd = RTK_CL_DOT(Q.S.D[0], Q.S.D[1], Q.S.D[2], Q.S.D[0], Q.S.D[1], Q.S.D[2]);
	rtk_sweep_centre(Q.S, Q.S.tmin, Q.S.S);
	bool finite = true;
	for (int k = 0; k < 12; k++) finite = finite && RTK_SW_FINITE(w[k]);
	for (int k = 0; k < 3; k++) {
		const float hk = w[9 + k];
		Q.h[k] = hk;
		Q.g[k] = RTK_CL_ADD(Q.S.r, hk < 0.0f ? -hk : hk);
		Q.p0[k] = RTK_CL_SUB(Q.S.S[k], hk);
		Q.p1[k] = RTK_CL_ADD(Q.S.S[k], hk);
	}
	const bool moves = Q.S.D[0] != 0.0f || Q.S.D[1] != 0.0f || Q.S.D[2] != 0.0f;
	return finite && moves && Q.S.r >= 0.0f && Q.S.tmin <= Q.S.tmax;
}

// 1. the path against the box [lo, hi] grown by g: false = empty; te the entry time
RTK_CLOSEST_FN bool rtk_capsule_slab(const rtk_capsule_query &Q, const float *lo, const float *hi, float &te)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	float t0 = Q.S.tmin, t1 = Q.S.tmax;
	bool inside = true;
	for (int k = 0; k < 3; k++) {
		const float l = RTK_CL_SUB(lo[k], Q.g[k]), h = RTK_CL_ADD(hi[k], Q.g[k]);
		const float d = Q.S.D[k];
		if (d == 0.0f) inside = inside && l <= Q.S.O[k] && Q.S.O[k] <= h;
		else {
			const float tl = RTK_CL_DIV(RTK_CL_SUB(l, Q.S.O[k]), d), th = RTK_CL_DIV(RTK_CL_SUB(h, Q.S.O[k]), d);
			const float tn = d > 0.0f ? tl : th, tf = d > 0.0f ? th : tl;
			t0 = RTK_CL_MAX(t0, tn);
			t1 = RTK_CL_MIN(t1, tf);
		}
	}
	te = t0;
	return inside && t0 <= t1;
}

// 2. (ii): the distance walk of the segment [p0, p1] and the triangle (a, b, c)
RTK_CLOSEST_FN void rtk_capsule_distance(const float *p0, const float *p1, const float *a, const float *b, const float *c, rtk_capsule_contact &r)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	float x[3], slo[3], shi[3], lo[3], hi[3], e[3][3];
	bool touch = true;
	for (int k = 0; k < 3; k++) {
		x[k] = RTK_CL_SUB(p1[k], p0[k]);
		slo[k] = RTK_CL_MIN(p0[k], p1[k]); shi[k] = RTK_CL_MAX(p0[k], p1[k]);
		lo[k] = RTK_CL_MIN(RTK_CL_MIN(a[k], b[k]), c[k]); hi[k] = RTK_CL_MAX(RTK_CL_MAX(a[k], b[k]), c[k]);
		touch = touch && lo[k] <= shi[k] && hi[k] >= slo[k];
	}
	rtk_touch_edges(a, b, c, e);
	r.dist2 = __builtin_huge_valf(); r.u = 0.0f; r.v = 0.0f; r.item = RTK_CP_ITEM_NONE;
	for (int k = 0; k < 3; k++) { r.qt[k] = a[k]; r.qa[k] = p0[k]; }
	if (touch) {
		float n[3], t, s[3];
		rtk_touch_cross(e[0], e[1], n);
		if (rtk_pair_edge_pierces(p0, p1, x, a, b, c, n, t, s)) {
			for (int k = 0; k < 3; k++) {
				const float at = RTK_CL_ADD(p0[k], RTK_CL_MUL(x[k], t));
				const float ilo = RTK_CL_MAX(slo[k], lo[k]), ihi = RTK_CL_MIN(shi[k], hi[k]);
				r.qt[k] = r.qa[k] = RTK_CL_CLAMP(at, ilo, ihi);
			}
			const float sum = RTK_CL_ADD(RTK_CL_ADD(s[0], s[1]), s[2]);
			r.u = RTK_CL_DIV(s[1], sum); r.v = RTK_CL_DIV(s[2], sum);
			r.dist2 = 0.0f; r.item = RTK_CP_ITEM_PIERCE;
			return;
		}
	}
	{
		float q[3], u, v;
		int region;
		const float d0 = rtk_closest_triangle(p0, a, b, c, q, u, v, region);
		if (d0 < r.dist2) {
			r.dist2 = d0; r.u = u; r.v = v; r.item = RTK_CP_ITEM_END0;
			for (int k = 0; k < 3; k++) { r.qt[k] = q[k]; r.qa[k] = p0[k]; }
		}
		const float d1 = rtk_closest_triangle(p1, a, b, c, q, u, v, region);
		if (d1 < r.dist2) {
			r.dist2 = d1; r.u = u; r.v = v; r.item = RTK_CP_ITEM_END1;
			for (int k = 0; k < 3; k++) { r.qt[k] = q[k]; r.qa[k] = p1[k]; }
		}
	}
	const float xx = RTK_CL_DOT(x[0], x[1], x[2], x[0], x[1], x[2]);
RTK_CP_UNROLL
	for (int j = 0; j < 3; j++) {
		const float *vj = j == 0 ? a : (j == 1 ? b : c);
		const float ee = RTK_CL_DOT(e[j][0], e[j][1], e[j][2], e[j][0], e[j][1], e[j][2]);
		float s, t, qa[3], qb[3], f[3];
		rtk_pair_segments(p0, x, xx, vj, e[j], ee, s, t);
		for (int k = 0; k < 3; k++) {
			const float pa = RTK_CL_ADD(p0[k], RTK_CL_MUL(x[k], s)), pb = RTK_CL_ADD(vj[k], RTK_CL_MUL(e[j][k], t));
			qa[k] = RTK_CL_CLAMP(pa, slo[k], shi[k]);
			qb[k] = RTK_CL_CLAMP(pb, lo[k], hi[k]);
			f[k] = RTK_CL_SUB(qa[k], qb[k]);
		}
		const float d2 = RTK_CL_ADD(RTK_CL_ADD(RTK_CL_MUL(f[0], f[0]), RTK_CL_MUL(f[1], f[1])), RTK_CL_MUL(f[2], f[2]));
		if (d2 < r.dist2) {
			r.dist2 = d2; r.item = RTK_CP_ITEM_EDGE + j;
			rtk_pair_edge_weights(j, t, r.u, r.v);
			for (int k = 0; k < 3; k++) { r.qt[k] = qb[k]; r.qa[k] = qa[k]; }
		}
	}
}

// a face of 2. (iii): the sphere rule's face step on the triangle (A, B, C); R is the query moved to the centre at te
RTK_CLOSEST_FN bool rtk_capsule_face(const rtk_sweep_query &R, const float *A, const float *B, const float *C, float &t)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	const float ab[3] = { RTK_CL_SUB(B[0], A[0]), RTK_CL_SUB(B[1], A[1]), RTK_CL_SUB(B[2], A[2]) };
	const float ac[3] = { RTK_CL_SUB(C[0], A[0]), RTK_CL_SUB(C[1], A[1]), RTK_CL_SUB(C[2], A[2]) };
	const float ma[3] = { RTK_CL_SUB(R.O[0], A[0]), RTK_CL_SUB(R.O[1], A[1]), RTK_CL_SUB(R.O[2], A[2]) };
	const float n0 = RTK_CL_SUB(RTK_CL_MUL(ab[1], ac[2]), RTK_CL_MUL(ab[2], ac[1]));
	const float n1 = RTK_CL_SUB(RTK_CL_MUL(ab[2], ac[0]), RTK_CL_MUL(ab[0], ac[2]));
	const float n2 = RTK_CL_SUB(RTK_CL_MUL(ab[0], ac[1]), RTK_CL_MUL(ab[1], ac[0]));
	const float nn = RTK_CL_DOT(n0, n1, n2, n0, n1, n2);
	const float len = RTK_SW_SQRT(nn);
	const float h0 = RTK_CL_DOT(n0, n1, n2, ma[0], ma[1], ma[2]), hd = RTK_CL_DOT(n0, n1, n2, R.D[0], R.D[1], R.D[2]);
	const float hs = RTK_CL_ADD(h0, RTK_CL_MUL(R.tmin, hd));
	const float sr = hs < 0.0f ? -R.r : R.r;
	t = RTK_CL_DIV(RTK_CL_SUB(RTK_CL_MUL(sr, len), h0), hd);
	if (!(nn > 0.0f && hd != 0.0f && R.tmin <= t && t <= R.tmax)) return false;
	float ct[3], q[3], u, v;
	int region;
	rtk_sweep_centre(R, t, ct);
	(void)rtk_closest_triangle(ct, A, B, C, q, u, v, region);
	return region == 7;
}

// an edge of 2. (iii) from p to q
RTK_CLOSEST_FN bool rtk_capsule_edge(const rtk_sweep_query &R, const float *p, const float *q, float &t)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	const float e[3] = { RTK_CL_SUB(q[0], p[0]), RTK_CL_SUB(q[1], p[1]), RTK_CL_SUB(q[2], p[2]) };
	const float m[3] = { RTK_CL_SUB(R.O[0], p[0]), RTK_CL_SUB(R.O[1], p[1]), RTK_CL_SUB(R.O[2], p[2]) };
	return rtk_sweep_edge(R, e, m, t);
}

// a vertex of 2. (iii)
RTK_CLOSEST_FN bool rtk_capsule_vertex(const rtk_sweep_query &R, const float *p, float &t)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	const float m[3] = { RTK_CL_SUB(R.O[0], p[0]), RTK_CL_SUB(R.O[1], p[1]), RTK_CL_SUB(R.O[2], p[2]) };
	return rtk_sweep_vertex(R, m, t);
}

// the vertex picks of 2. (iii): indices into V = { a-, b-, c-, a+, b+, c+ }
#define RTK_CP_FACE_PICKS { { 0, 1, 2 }, { 3, 4, 5 }, { 1, 4, 0 }, { 3, 0, 4 }, { 2, 5, 1 }, { 4, 1, 5 }, { 0, 3, 2 }, { 5, 2, 3 } }
#define RTK_CP_EDGE_PICKS { { 0, 1 }, { 1, 2 }, { 2, 0 }, { 3, 4 }, { 4, 5 }, { 5, 3 }, { 0, 3 }, { 1, 4 }, { 2, 5 }, { 0, 4 }, { 1, 5 }, { 2, 3 } }

// 2. the capsule against the triangle (a, b, c): the feature (RTK_CP_NONE: no time) and the time by (iv)
RTK_CLOSEST_FN int rtk_capsule_triangle(const rtk_capsule_query &Q, const float *a, const float *b, const float *c, float &t_out)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	t_out = Q.S.tmax;
	// (i)
	const float lo[3] = { RTK_CL_MIN(RTK_CL_MIN(a[0], b[0]), c[0]), RTK_CL_MIN(RTK_CL_MIN(a[1], b[1]), c[1]), RTK_CL_MIN(RTK_CL_MIN(a[2], b[2]), c[2]) };
	const float hi[3] = { RTK_CL_MAX(RTK_CL_MAX(a[0], b[0]), c[0]), RTK_CL_MAX(RTK_CL_MAX(a[1], b[1]), c[1]), RTK_CL_MAX(RTK_CL_MAX(a[2], b[2]), c[2]) };
	float te;
	if (!rtk_capsule_slab(Q, lo, hi, te)) return RTK_CP_NONE;
	// (ii)
	{
		rtk_capsule_contact at;
		rtk_capsule_distance(Q.p0, Q.p1, a, b, c, at);
		if (at.dist2 <= Q.S.r2) { t_out = RTK_CL_MAX(Q.S.tmin, te); return RTK_CP_START; }
	}
	// (iii), from the centre at te: R is the sphere part of the query moved there
	rtk_sweep_query R = Q.S;
	rtk_sweep_centre(Q.S, te, R.O);
	R.tmin = RTK_CL_SUB(Q.S.tmin, te);
	R.tmax = RTK_CL_SUB(Q.S.tmax, te);
	float V[6][3];
	for (int k = 0; k < 3; k++) {
		V[0][k] = RTK_CL_SUB(a[k], Q.h[k]); V[1][k] = RTK_CL_SUB(b[k], Q.h[k]); V[2][k] = RTK_CL_SUB(c[k], Q.h[k]);
		V[3][k] = RTK_CL_ADD(a[k], Q.h[k]); V[4][k] = RTK_CL_ADD(b[k], Q.h[k]); V[5][k] = RTK_CL_ADD(c[k], Q.h[k]);
	}
	int feature = RTK_CP_NONE;
	float best = 0.0f, t;
	{
		const int F[8][3] = RTK_CP_FACE_PICKS;
RTK_CP_UNROLL
		for (int i = 0; i < 8; i++)
			if (rtk_capsule_face(R, V[F[i][0]], V[F[i][1]], V[F[i][2]], t) && (feature == RTK_CP_NONE || t < best)) { feature = RTK_CP_FACE + i; best = t; }
		const int E[12][2] = RTK_CP_EDGE_PICKS;
RTK_CP_UNROLL
		for (int i = 0; i < 12; i++)
			if (rtk_capsule_edge(R, V[E[i][0]], V[E[i][1]], t) && (feature == RTK_CP_NONE || t < best)) { feature = RTK_CP_EDGE + i; best = t; }
RTK_CP_UNROLL
		for (int i = 0; i < 6; i++)
			if (rtk_capsule_vertex(R, V[i], t) && (feature == RTK_CP_NONE || t < best)) { feature = RTK_CP_VERTEX + i; best = t; }
	}
	// (iv)
	if (feature != RTK_CP_NONE) {
		const float time = RTK_CL_ADD(te, best), late = RTK_CL_MAX(time, te);
		if (late > Q.S.tmax) feature = RTK_CP_NONE;
		else t_out = late;
	}
	return feature;
}

// the record: the distance walk at c(t) on the answer's triangle
RTK_CLOSEST_FN void rtk_capsule_record(const rtk_capsule_query &Q, float t, const float *a, const float *b, const float *c, rtk_capsule_contact &r)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	float ct[3], p0[3], p1[3];
	rtk_sweep_centre(Q.S, t, ct);
	for (int k = 0; k < 3; k++) { p0[k] = RTK_CL_SUB(ct[k], Q.h[k]); p1[k] = RTK_CL_ADD(ct[k], Q.h[k]); }
	rtk_capsule_distance(p0, p1, a, b, c, r);
}
