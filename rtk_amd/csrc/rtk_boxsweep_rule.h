// rtk_boxsweep_rule.h -- the one rule by which a box sweep is answered (rtk_dev_sweep_boxes, rtk_amd.h), for the host and the
// device: the kernel (rtk_boxsweep.hip) and tests/boxsweep_rule_driver.cpp include this file and nothing else decides a bit of a
// result. The result of a query is a pure function of the scene's triangle records, the filter and the query; the tree only
// decides how few of the records are looked at.
//
// The arithmetic is rtk_sweep_rule.h's: every product, sum, difference, quotient and square root below is ONE float operation,
// rounded on its own, in the order written: no fused multiply-add anywhere. On the device that is __fmul_rn / __fadd_rn /
// __fsub_rn / __fdiv_rn and sqrtf (the library is built with -fhip-fp32-correctly-rounded-divide-sqrt: quotient and root are
// IEEE's; __fsqrt_rn is NOT used, HIP maps it to the native approximation); on the host the file must be compiled with
// -ffp-contract=off (the library's flags; clang is told once more by the pragma below). It is what numpy float32 arithmetic
// gives, so a test states the expected bits without a GPU. Denormal inputs and results are kept. min and max are the selects of
// rtk_closest_rule.h; -x and |x| are exact; dot(x, y) = (x0 * y0 + x1 * y1) + x2 * y2;
// cross(x, y) = (x1 * y2 - x2 * y1, x2 * y0 - x0 * y2, x0 * y1 - x1 * y0).
//
// 0. THE QUERY (rtk_boxsweep_prepare). O = origin, D = direction, H = half; the box at time t is [c(t) - H, c(t) + H] with the
//    centre c(t) = O + D * t (componentwise, one product and one sum), t over the CLOSED interval [min_t, max_t] -- not a ray's
//    open one. A query is LIVE iff all eleven floats are finite (RTK_INF is a finite float: "no limit"), D is not all zeros,
//    every H[k] >= 0 and min_t <= max_t; a query that is not live is a miss. H == 0 on one, two or three axes is legal: a
//    rectangle, a segment and a point are boxes.
// 1. THE PATH AND A BOX (rtk_boxsweep_slab): rtk_sweep_slab with H[k] in the place of r on axis k. The box [lo, hi] grown by H
//    against the path of the centre, clipped to [min_t, max_t].
//        t0 = min_t, t1 = max_t, axis = START; for k = 0, 1, 2:   l = lo[k] - H[k],  h = hi[k] + H[k]
//            D[k] == 0:   empty unless l <= O[k] && O[k] <= h                      (a closed containment test, no quotient)
//            otherwise    tl = (l - O[k]) / D[k], th = (h - O[k]) / D[k];  D[k] > 0: tn = tl, tf = th;  D[k] < 0: tn = th, tf = tl
//                         tn > t0: t0 = tn, axis = BOX_X + k;    tf < t1: t1 = tf
//        empty unless t0 <= t1; the ENTRY TIME is te = t0, the EXIT TIME is tx = t1, and `axis` names the face of the grown box
//        that gave te (START: none did, the centre is inside the slabs at min_t; the first axis wins among equal times).
//    For a live query and finite boxes no operand is a NaN (O is finite, so l - O[k] is never inf - inf; D[k] != 0, so no 0 / 0,
//    also for a denormal D[k]), hence neither is te.
//    THE BOUND: a box above a triangle contains the triangle's own box (lo' <= lo, hi' >= hi). A rounded difference, a rounded sum
//    and a rounded quotient by a fixed divisor are monotone, and so are the selects: on every axis l' <= l and h' >= h, the
//    containment test of the larger box holds where the smaller one's does, the near plane's time of the larger box is <= and
//    its far plane's time >= the smaller one's (for D[k] < 0 the planes swap and the quotient reverses the order twice). So
//    t0' <= t0 and t1' >= t1 EXACTLY: the larger box's interval is empty only if the triangle's is, and its entry time never
//    exceeds the triangle's te, without a margin. By 2. (iii) the triangle's time is >= its te: entry time <= time for every
//    triangle below the box.
// 2. THE BOX AND ONE TRIANGLE (rtk_boxsweep_triangle). a, b, c are DevTri.v0 / v1 / v2 as the scene holds them. A time or "none",
//    and the axis that gave it: swept separating axes, thirteen of them.
//    (i)   The three axes of the box are the triangle's own box lo = min(min(a, b), c), hi = max(max(a, b), c) by 1.: empty
//          means none; otherwise te, tx and the face that gave te.
//    (ii)  The other ten are measured FROM THE CENTRE AT te: O' = c(te), wa = a - O', wb = b - O', wc = c - O'. (Measured from the
//          origin, the projections below cancel once the start is far away compared with the box and the triangle, as the
//          quadratics of the sphere rule do; from c(te) every projection is of the size of the grown box.) The running
//          interval starts at enter = 0, leave = tx - te. The edges are ab = b - a, bc = c - b, ca = a - c, and ac = c - a. The axes
//          L, in this order:
//              NORMAL       L = cross(ab, ac);    p(w) = dot(L, w);   rb = (|L0| * H0 + |L1| * H1) + |L2| * H2;   s = dot(L, D)
//              EDGE e, j    for e = ab, bc, ca and j = 0, 1, 2, with i1 = (j + 1) % 3, i2 = (j + 2) % 3:  L = cross(e, unit_j), whose
//                           component j is zero, L[i1] = e[i2], L[i2] = -e[i1]; stated over its two other components:
//                           p(w) = e[i2] * w[i1] - e[i1] * w[i2];   rb = |e[i2]| * H[i1] + |e[i1]| * H[i2];
//                           s = e[i2] * D[i1] - e[i1] * D[i2]
//          Per axis: pmin = min(min(p(wa), p(wb)), p(wc)), pmax = max(max(p(wa), p(wb)), p(wc)): the triangle's extent; the box's
//          is [s * t - rb, s * t + rb].
//              s == 0:    the pair is separated for good, NONE, iff pmin > rb || pmax < -rb; otherwise the axis says nothing
//              otherwise  q0 = (pmin - rb) / s, q1 = (pmax + rb) / s;   s > 0: en = q0, ex = q1;   s < 0: en = q1, ex = q0
//                         en > enter: enter = en, axis = this one;    ex < leave: leave = ex
//          A zero axis (a = b, a triangle in an axis plane, ...) has p = rb = s = 0 and says nothing; a NaN fails every
//          comparison and so never separates and never moves the interval: the touching rule's convention. The first axis in
//          the order BOX_X, BOX_Y, BOX_Z, NORMAL, AB_X .. CA_Z wins among equal enter times. None unless enter <= leave.
//    (iii) THE TIME is max(te + enter, te): enter >= 0 and the max changes nothing but for a NaN; stated in floats it is what
//          makes the skip of 3. exact. A time > max_t is NONE: for te < 0 the rounding of tx - te can admit an enter whose
//          te + enter rounds to the neighbour above max_t, and no time outside [min_t, max_t] is ever reported (te >= min_t, and
//          te <= max_t where the interval of (i) is not empty). A box that overlaps the triangle at min_t has te = min_t and
//          enter = 0: a hit at the start, axis START.
//    THE NORMAL (rtk_boxsweep_normal) is the axis that gave the time, of unit length and turned against the motion: all zeros
//    for START; for BOX_X + k the unit vector of axis k times -1 if D[k] > 0, else +1, the other components +0; for the others
//    L as above (all three components, the one that is zero by construction as +0), len = sqrt(dot(L, L)), s = dot(L, D) (which
//    equals the s above: the product with the zero component adds a zero), n[k] = (s > 0 ? -L[k] : L[k]) / len -- and all zeros
//    unless 0 < len <= FLT_MAX (a cross product whose square underflows or overflows has no length in float). Never a NaN for a
//    live query and a finite scene.
//    H == 0 is this rule on a point: it is NOT rtk's watertight ray test and not bit-equal to a trace.
// 3. BETTER THAN and SKIP are rtk_sweep_rule.h's own rtk_sweep_better and rtk_sweep_skip: (t, prim) beats (best_t, best_prim) iff
//    t < best_t || (t == best_t && prim < best_prim); a NaN never beats anything. A subtree may be skipped iff its interval by 1.
//    is empty or te > best_t -- strictly: an equal entry time can hide a lower id.
// The answer is the best (t, prim) by 3. over ALL triangle records that pass the filter and have a time, starting from
// (max_t, RTK_PRIM_NONE), or a miss. ONE rtk_closest_triangle(c(t)) on the answer's triangle gives u and v: those of the
// triangle's point nearest to the centre, a witness on the triangle, not necessarily a point of contact. The centre c(t) is
// reported as computed there, the normal by rtk_boxsweep_normal.
//
// ACCURACY of 2., measured against the same thirteen axes in float64 over 3 million random (triangle, path, box) cases at five
// combinations of triangle size, start distance and half extents, on ALL of the 0.57 million that have a time in both (8.7 % to
// 29.5 % of a family), slivers, starts that overlap and grazing contacts included: |t - exact| * |D| stayed within
// 1730.41 * 2^-23 of the largest coordinate magnitude involved (origin, triangle, the box's faces at the contact);
// tests/test_boxsweep_cpu.py asserts 4327 * 2^-23. That figure is a grazing contact's: a time is (pmin - rb) / s, and where the
// motion runs 0.01 degrees off the contact plane, s has lost four digits and the time's own condition number is 5000; the error
// times the cosine between motion and normal stayed below 7 * 2^-23. Without grazing contacts (cosine below 0.05) and starts that
// overlap, as the sphere sweep's statement is measured: 31.96 * 2^-23 over 0.54 million, asserted at 80 * 2^-23. float32 and
// float64 disagreed about hit or none on 419 of the 3 million cases, every one of them within the asserted rounding of a threshold.
#pragma once

#include <stdint.h>
#include "rtk_closest_rule.h"
#include "rtk_sweep_rule.h"

// (the same on the device: under the library's flag the builtin is IEEE's root, while HIP's __fsqrt_rn is the native approximation)
#define RTK_BS_SQRT(a) __builtin_sqrtf((a))
#define RTK_BS_ABS(a) __builtin_fabsf((a))
#define RTK_BS_MAX_FLOAT 3.402823466e38f
#define RTK_BS_FINITE(x) ((x) >= -RTK_BS_MAX_FLOAT && (x) <= RTK_BS_MAX_FLOAT)

// what 2. found: none, an overlap at the start, or the axis that gave the time (the edge axes: RTK_BS_EDGE + 3 * edge + j)
enum { RTK_BS_NONE = 0, RTK_BS_START = 1, RTK_BS_BOX_X = 2, RTK_BS_BOX_Y = 3, RTK_BS_BOX_Z = 4, RTK_BS_NORMAL = 5, RTK_BS_EDGE = 6,
	RTK_BS_AXES = 15 };

// 0. the query
struct rtk_boxsweep_query {
	float O[3], D[3], tmin, tmax, H[3];
};

// the centre at t
RTK_CLOSEST_FN void rtk_boxsweep_centre(const rtk_boxsweep_query &Q, float t, float *c)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	c[0] = RTK_CL_ADD(Q.O[0], RTK_CL_MUL(Q.D[0], t));
	c[1] = RTK_CL_ADD(Q.O[1], RTK_CL_MUL(Q.D[1], t));
	c[2] = RTK_CL_ADD(Q.O[2], RTK_CL_MUL(Q.D[2], t));
}

// 0. w: the eleven floats of a rtk_box_sweep. Returns whether the query is live; Q is filled either way
RTK_CLOSEST_FN bool rtk_boxsweep_prepare(const float *w, rtk_boxsweep_query &Q)
{
	Q.O[0] = w[0]; Q.O[1] = w[1]; Q.O[2] = w[2];
	Q.D[0] = w[3]; Q.D[1] = w[4]; Q.D[2] = w[5];
	Q.tmin = w[6]; Q.tmax = w[7];
	Q.H[0] = w[8]; Q.H[1] = w[9]; Q.H[2] = w[10];
	bool finite = true;
	for (int k = 0; k < 11; k++) finite = finite && RTK_BS_FINITE(w[k]);
	const bool moves = Q.D[0] != 0.0f || Q.D[1] != 0.0f || Q.D[2] != 0.0f;
	return finite && moves && Q.H[0] >= 0.0f && Q.H[1] >= 0.0f && Q.H[2] >= 0.0f && Q.tmin <= Q.tmax;
}

// 1. the path against the box [lo, hi] grown by H: false = empty; te the entry time, tx the leave time, axis what gave te
RTK_CLOSEST_FN bool rtk_boxsweep_slab(const rtk_boxsweep_query &Q, const float *lo, const float *hi, float &te, float &tx, int &axis)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	float t0 = Q.tmin, t1 = Q.tmax;
	bool inside = true;
	axis = RTK_BS_START;
	for (int k = 0; k < 3; k++) {
		const float l = RTK_CL_SUB(lo[k], Q.H[k]), h = RTK_CL_ADD(hi[k], Q.H[k]);
		const float d = Q.D[k];
		if (d == 0.0f) inside = inside && l <= Q.O[k] && Q.O[k] <= h;
		else {
			const float tl = RTK_CL_DIV(RTK_CL_SUB(l, Q.O[k]), d), th = RTK_CL_DIV(RTK_CL_SUB(h, Q.O[k]), d);
			const float tn = d > 0.0f ? tl : th, tf = d > 0.0f ? th : tl;
			if (tn > t0) { t0 = tn; axis = RTK_BS_BOX_X + k; }
			t1 = RTK_CL_MIN(t1, tf);
		}
	}
	te = t0;
	tx = t1;
	return inside && t0 <= t1;
}

// one axis of 2. (ii): the projections of the three vertices, the box's reach and the speed. false = separated for good
RTK_CLOSEST_FN bool rtk_boxsweep_axis(float pa, float pb, float pc, float rb, float s, int code, float &enter, float &leave, int &axis)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	const float pmin = RTK_CL_MIN(RTK_CL_MIN(pa, pb), pc), pmax = RTK_CL_MAX(RTK_CL_MAX(pa, pb), pc);
	if (s == 0.0f) return !(pmin > rb || pmax < -rb);
	const float q0 = RTK_CL_DIV(RTK_CL_SUB(pmin, rb), s), q1 = RTK_CL_DIV(RTK_CL_ADD(pmax, rb), s);
	const float en = s > 0.0f ? q0 : q1, ex = s > 0.0f ? q1 : q0;
	if (en > enter) { enter = en; axis = code; }
	leave = RTK_CL_MIN(leave, ex);
	return true;
}

// the axis cross(e, unit_j) of 2. (ii) over its two components i1, i2
#define RTK_BS_EDGE_P(e, w, i1, i2) RTK_CL_SUB(RTK_CL_MUL((e)[i2], (w)[i1]), RTK_CL_MUL((e)[i1], (w)[i2]))
#define RTK_BS_EDGE_AXIS(e, i1, i2, code) \
	rtk_boxsweep_axis(RTK_BS_EDGE_P(e, wa, i1, i2), RTK_BS_EDGE_P(e, wb, i1, i2), RTK_BS_EDGE_P(e, wc, i1, i2), \
		RTK_CL_ADD(RTK_CL_MUL(RTK_BS_ABS((e)[i2]), Q.H[i1]), RTK_CL_MUL(RTK_BS_ABS((e)[i1]), Q.H[i2])), RTK_BS_EDGE_P(e, Q.D, i1, i2), (code), enter, leave, axis)

// the three axes of one edge; false = separated for good
RTK_CLOSEST_FN bool rtk_boxsweep_edge(const rtk_boxsweep_query &Q, const float *e, const float *wa, const float *wb, const float *wc, int code,
	float &enter, float &leave, int &axis)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	bool some = RTK_BS_EDGE_AXIS(e, 1, 2, code);
	some = RTK_BS_EDGE_AXIS(e, 2, 0, code + 1) && some;
	some = RTK_BS_EDGE_AXIS(e, 0, 1, code + 2) && some;
	return some;
}

// 2. the box against the triangle (a, b, c): the axis (RTK_BS_NONE: no time) and the time by (iii)
RTK_CLOSEST_FN int rtk_boxsweep_triangle(const rtk_boxsweep_query &Q, const float *a, const float *b, const float *c, float &t_out)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	t_out = Q.tmax;
	// (i)
	const float lo[3] = { RTK_CL_MIN(RTK_CL_MIN(a[0], b[0]), c[0]), RTK_CL_MIN(RTK_CL_MIN(a[1], b[1]), c[1]), RTK_CL_MIN(RTK_CL_MIN(a[2], b[2]), c[2]) };
	const float hi[3] = { RTK_CL_MAX(RTK_CL_MAX(a[0], b[0]), c[0]), RTK_CL_MAX(RTK_CL_MAX(a[1], b[1]), c[1]), RTK_CL_MAX(RTK_CL_MAX(a[2], b[2]), c[2]) };
	float te, tx;
	int axis;
	if (!rtk_boxsweep_slab(Q, lo, hi, te, tx, axis)) return RTK_BS_NONE;
	// (ii), from the centre at te
	float Op[3];
	rtk_boxsweep_centre(Q, te, Op);
	const float wa[3] = { RTK_CL_SUB(a[0], Op[0]), RTK_CL_SUB(a[1], Op[1]), RTK_CL_SUB(a[2], Op[2]) };
	const float wb[3] = { RTK_CL_SUB(b[0], Op[0]), RTK_CL_SUB(b[1], Op[1]), RTK_CL_SUB(b[2], Op[2]) };
	const float wc[3] = { RTK_CL_SUB(c[0], Op[0]), RTK_CL_SUB(c[1], Op[1]), RTK_CL_SUB(c[2], Op[2]) };
	const float ab[3] = { RTK_CL_SUB(b[0], a[0]), RTK_CL_SUB(b[1], a[1]), RTK_CL_SUB(b[2], a[2]) };
	const float bc[3] = { RTK_CL_SUB(c[0], b[0]), RTK_CL_SUB(c[1], b[1]), RTK_CL_SUB(c[2], b[2]) };
	const float ca[3] = { RTK_CL_SUB(a[0], c[0]), RTK_CL_SUB(a[1], c[1]), RTK_CL_SUB(a[2], c[2]) };
	const float ac[3] = { RTK_CL_SUB(c[0], a[0]), RTK_CL_SUB(c[1], a[1]), RTK_CL_SUB(c[2], a[2]) };
	float enter = 0.0f, leave = RTK_CL_SUB(tx, te);
	const float n0 = RTK_CL_SUB(RTK_CL_MUL(ab[1], ac[2]), RTK_CL_MUL(ab[2], ac[1]));
	const float n1 = RTK_CL_SUB(RTK_CL_MUL(ab[2], ac[0]), RTK_CL_MUL(ab[0], ac[2]));
	const float n2 = RTK_CL_SUB(RTK_CL_MUL(ab[0], ac[1]), RTK_CL_MUL(ab[1], ac[0]));
	const float rb = RTK_CL_ADD(RTK_CL_ADD(RTK_CL_MUL(RTK_BS_ABS(n0), Q.H[0]), RTK_CL_MUL(RTK_BS_ABS(n1), Q.H[1])), RTK_CL_MUL(RTK_BS_ABS(n2), Q.H[2]));
	bool some = rtk_boxsweep_axis(RTK_CL_DOT(n0, n1, n2, wa[0], wa[1], wa[2]), RTK_CL_DOT(n0, n1, n2, wb[0], wb[1], wb[2]),
		RTK_CL_DOT(n0, n1, n2, wc[0], wc[1], wc[2]), rb, RTK_CL_DOT(n0, n1, n2, Q.D[0], Q.D[1], Q.D[2]), RTK_BS_NORMAL, enter, leave, axis);
	some = rtk_boxsweep_edge(Q, ab, wa, wb, wc, RTK_BS_EDGE, enter, leave, axis) && some;
	some = rtk_boxsweep_edge(Q, bc, wa, wb, wc, RTK_BS_EDGE + 3, enter, leave, axis) && some;
	some = rtk_boxsweep_edge(Q, ca, wa, wb, wc, RTK_BS_EDGE + 6, enter, leave, axis) && some;
	if (!some || !(enter <= leave)) return RTK_BS_NONE;
	// (iii)
	const float time = RTK_CL_ADD(te, enter), late = RTK_CL_MAX(time, te);
	if (late > Q.tmax) return RTK_BS_NONE;
	t_out = late;
	return axis;
}

// the normal of 2.: the axis that gave the time, unit length, against the motion; zeros for RTK_BS_START and RTK_BS_NONE
RTK_CLOSEST_FN void rtk_boxsweep_normal(const rtk_boxsweep_query &Q, const float *a, const float *b, const float *c, int axis, float *n)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	n[0] = 0.0f; n[1] = 0.0f; n[2] = 0.0f;
	if (axis < RTK_BS_BOX_X || axis >= RTK_BS_AXES) return;
	// (selects, no indexing by a variable: the arrays stay registers on the device)
	if (axis <= RTK_BS_BOX_Z) {
		n[0] = axis == RTK_BS_BOX_X ? (Q.D[0] > 0.0f ? -1.0f : 1.0f) : 0.0f;
		n[1] = axis == RTK_BS_BOX_Y ? (Q.D[1] > 0.0f ? -1.0f : 1.0f) : 0.0f;
		n[2] = axis == RTK_BS_BOX_Z ? (Q.D[2] > 0.0f ? -1.0f : 1.0f) : 0.0f;
		return;
	}
	float L[3];
	if (axis == RTK_BS_NORMAL) {
		const float ab[3] = { RTK_CL_SUB(b[0], a[0]), RTK_CL_SUB(b[1], a[1]), RTK_CL_SUB(b[2], a[2]) };
		const float ac[3] = { RTK_CL_SUB(c[0], a[0]), RTK_CL_SUB(c[1], a[1]), RTK_CL_SUB(c[2], a[2]) };
		L[0] = RTK_CL_SUB(RTK_CL_MUL(ab[1], ac[2]), RTK_CL_MUL(ab[2], ac[1]));
		L[1] = RTK_CL_SUB(RTK_CL_MUL(ab[2], ac[0]), RTK_CL_MUL(ab[0], ac[2]));
		L[2] = RTK_CL_SUB(RTK_CL_MUL(ab[0], ac[1]), RTK_CL_MUL(ab[1], ac[0]));
	} else {
		const int k = (axis - RTK_BS_EDGE) / 3, j = (axis - RTK_BS_EDGE) % 3;
		const float e0 = k == 0 ? RTK_CL_SUB(b[0], a[0]) : k == 1 ? RTK_CL_SUB(c[0], b[0]) : RTK_CL_SUB(a[0], c[0]);
		const float e1 = k == 0 ? RTK_CL_SUB(b[1], a[1]) : k == 1 ? RTK_CL_SUB(c[1], b[1]) : RTK_CL_SUB(a[1], c[1]);
		const float e2 = k == 0 ? RTK_CL_SUB(b[2], a[2]) : k == 1 ? RTK_CL_SUB(c[2], b[2]) : RTK_CL_SUB(a[2], c[2]);
		L[0] = j == 0 ? 0.0f : j == 1 ? -e2 : e1;
		L[1] = j == 0 ? e2 : j == 1 ? 0.0f : -e0;
		L[2] = j == 0 ? -e1 : j == 1 ? e0 : 0.0f;
	}
	const float len = RTK_BS_SQRT(RTK_CL_DOT(L[0], L[1], L[2], L[0], L[1], L[2]));
	const float s = RTK_CL_DOT(L[0], L[1], L[2], Q.D[0], Q.D[1], Q.D[2]);
	if (!(len > 0.0f && len <= RTK_BS_MAX_FLOAT)) return;
	n[0] = RTK_CL_DIV(s > 0.0f ? -L[0] : L[0], len);
	n[1] = RTK_CL_DIV(s > 0.0f ? -L[1] : L[1], len);
	n[2] = RTK_CL_DIV(s > 0.0f ? -L[2] : L[2], len);
}
