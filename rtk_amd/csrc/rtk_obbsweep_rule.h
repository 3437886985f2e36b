// rtk_obbsweep_rule.h -- the one rule by which an oriented box sweep is answered (rtk_dev_sweep_obbs, rtk_amd.h), for the host and
// the device: the kernel (rtk_obbsweep.hip) and tests/obbsweep_rule_driver.cpp include this file and nothing else decides a bit of
// a result. The result of a query is a pure function of the scene's triangle records, the filter and the query; the tree only
// decides how few of the records are looked at.
//
// The arithmetic is rtk_boxsweep_rule.h's: every product, sum, difference, quotient and square root below is ONE float operation,
// rounded on its own, in the order written: no fused multiply-add anywhere. On the device that is __fmul_rn / __fadd_rn /
// __fsub_rn / __fdiv_rn and the IEEE root (the library is built with -fhip-fp32-correctly-rounded-divide-sqrt; __fsqrt_rn is NOT
// used); on the host the file must be compiled with -ffp-contract=off (clang is told once more by the pragma below). It is what
// numpy float32 arithmetic gives, so a test states the expected bits without a GPU. Denormal inputs and results are kept. min and
// max are the selects of rtk_closest_rule.h; -x and |x| are exact; dot(x, y) = (x0 * y0 + x1 * y1) + x2 * y2.
//
// 0. THE QUERY (rtk_obbsweep_prepare). O = origin, D = direction, half = the box's half extents along its own axes, u0, u1, u2 =
//    the rows of `axes`: the box's axes in scene coordinates. The box at time t is { c(t) + a0 * u0 + a1 * u1 + a2 * u2 :
//    |aj| <= half[j] } with the centre c(t) = O + D * t (componentwise, one product and one sum), t over the CLOSED interval
//    [min_t, max_t]; it does not turn while it moves. A query is LIVE iff all twenty floats are finite (RTK_INF is a finite
//    float: "no limit"), D is not all zeros, every half[j] >= 0, min_t <= max_t and the axes are orthonormal to within
//    RTK_OBB_ORTHO_TOL = 2^-10: |dot(uj, uj) - 1| <= tol for j = 0, 1, 2 and |dot(u0, u1)|, |dot(u0, u2)|, |dot(u1, u2)| <= tol
//    (a dot that overflows fails). A query that is not live is a miss. The tolerance is a gate against garbage, not an accuracy
//    claim: rows rounded from a float64 rotation or made from a float32 quaternion pass with room to spare. Within the gate the
//    axes are used as given and treated as orthonormal (a left-handed triple is a box as well). Once per query:
//        D'[j] = dot(uj, D)                                                    the motion in the box's frame
//        g[k]  = (|u0[k]| * half[0] + |u1[k]| * half[1]) + |u2[k]| * half[2]     the box's reach along scene axis k
//    half == 0 on one, two or three axes is legal: a rectangle, a segment and a point are boxes.
// 1. THE PATH AND A BOX (rtk_obbsweep_slab): rtk_boxsweep_slab AS IT STANDS with g in the place of H, in the scene's axes: the
//    box [lo, hi] grown by g against the path of the centre, clipped to [min_t, max_t]: empty, or the ENTRY TIME te and the EXIT
//    TIME tx. The face that routine names means nothing here (the grown box's faces are not the box's) and is not used.
//    THE BOUND: g is a fixed number per axis and query, so the argument of rtk_boxsweep_rule.h carries over word for word: a box
//    above a triangle contains the triangle's own box, every operation of the slab is monotone, so the larger box's interval
//    contains the smaller one's EXACTLY: it is empty only if the triangle's is, and its entry time never exceeds the triangle's
//    te, without a margin. By 2. (iii) the triangle's time is >= its te: entry time <= time for every triangle below the box.
// 2. THE BOX AND ONE TRIANGLE (rtk_obbsweep_triangle). a, b, c are DevTri.v0 / v1 / v2 as the scene holds them.
//    (i)   The slab of 1. on the triangle's own box lo = min(min(a, b), c), hi = max(max(a, b), c): empty means none; otherwise
//          te and tx.
//    (ii)  Everything else is measured FROM THE CENTRE AT te, in the box's frame: O' = c(te), wa = a - O', wb = b - O', wc = c - O'
//          in the scene's axes, then wa' = (dot(u0, wa), dot(u1, wa), dot(u2, wa)) and likewise wb', wc'. The edges are
//          ab' = wb' - wa', bc' = wc' - wb', ca' = wa' - wc', and ac' = wc' - wa'. In that frame the box is axis-aligned with half
//          extents `half` and moves by D': the thirteen axes, in the order U0, U1, U2, NORMAL, AB_0 .. CA_2, are the routines of
//          rtk_boxsweep_rule.h on the primed vectors:
//              Uj           rtk_boxsweep_axis(wa'[j], wb'[j], wc'[j], half[j], D'[j])
//              NORMAL       L' = cross(ab', ac');   p(w') = dot(L', w');   rb = (|L'0| * half0 + |L'1| * half1) + |L'2| * half2;
//                           s = dot(L', D')
//              EDGE e, j    rtk_boxsweep_edge(e', wa', wb', wc') with D' and half: L' = cross(e', unit_j) as 2. (ii) there states it
//          with that rule's conventions: s == 0 separates for good (NONE) iff pmin > rb || pmax < -rb and otherwise says
//          nothing; a zero axis says nothing; a NaN fails every comparison and so never separates and never moves the interval.
//    (iii) This is where the rule departs from the axis-aligned one. There the slab's faces are the box's own, so an entry of 0
//          after te belongs to them; here they are not. The running entry starts below every float (-infinity), with no axis
//          named, and leave = tx - te. The latest en over the thirteen axes names the axis (en > enter: the first in the written
//          order wins among equal ones). None unless max(enter, 0) <= leave. THE TIME is max(te + max(enter, 0), te); a time
//          > max_t is NONE (for te < 0 the rounding of tx - te can admit a time an ulp beyond max_t; no time outside
//          [min_t, max_t] is ever reported). The reported axis is START -- the box overlaps the triangle at the start -- iff
//          enter <= 0 and te == min_t; otherwise it is the named axis. (Where no axis was named -- every s is zero or a NaN, which
//          takes a D' that underflowed -- and it is not a START, the code is RTK_OS_UNNAMED: a time without a normal.) The time is
//          >= te, which closes the chain entry time <= time.
//    THE NORMAL (rtk_obbsweep_normal) is the axis that gave the time, taken back to scene coordinates, of unit length and turned
//    against the motion: all zeros for START, for none and for an axis without a float length. Otherwise, with L' as above (for
//    Uj the unit vector of axis j, the components that are zero by construction as +0): n[k] = (L'[0] * u0[k] + L'[1] * u1[k])
//    + L'[2] * u2[k]; s = D'[j] for Uj, dot(L', D') for the others (which equals the s of (ii): the product with the zero
//    component adds a zero); len = sqrt(dot(n, n)); n[k] = (s > 0 ? -n[k] : n[k]) / len -- and all zeros unless 0 < len <= FLT_MAX
//    (a vector whose square underflows or overflows, or holds a NaN, has no length in float). Never a NaN for a live query and a
//    finite scene.
//    IDENTITY AXES (u0, u1, u2 the unit vectors) give the axis-aligned rule's answers UP TO ROUNDING, NOT bit for bit: D' = D,
//    g = half and w' = w exactly, but the edges are differences of shifted vertices here (wb' - wa', not b - a), and a contact
//    at te is named by its own axis instead of the slab's face. That is not promised.
//    half == 0 is this rule on a point: it is NOT rtk's watertight ray test and not bit-equal to a trace.
// 3. BETTER THAN and SKIP are rtk_sweep_rule.h's own rtk_sweep_better and rtk_sweep_skip: (t, prim) beats (best_t, best_prim) iff
//    t < best_t || (t == best_t && prim < best_prim); a NaN never beats anything. A subtree may be skipped iff its interval by 1.
//    is empty or te > best_t -- strictly: an equal entry time can hide a lower id.
// The answer is the best (t, prim) by 3. over ALL triangle records that pass the filter and have a time, starting from
// (max_t, RTK_PRIM_NONE), or a miss. ONE rtk_closest_triangle(c(t)) on the answer's triangle gives u and v: those of the
// triangle's point nearest to the centre, a witness on the triangle, not necessarily a point of contact. The centre c(t) is
// reported as computed there, the normal by rtk_obbsweep_normal.
//
// ACCURACY of 2., measured against the same rule in float64 over 3 million random (triangle, path, box, rotation) cases at five
// combinations of triangle size, start distance and half extents, rotations from random unit quaternions rounded to float32, on
// ALL of the 0.57 million that have a time in both, slivers, starts that overlap and grazing contacts included:
// |t - exact| * |D| stayed within 726.86 * 2^-23 of the largest coordinate magnitude involved (origin, triangle, the centre
// at the contact plus the box's reach g); tests/test_obbsweep_cpu.py asserts 1818 * 2^-23. As for the axis-aligned box that
// figure is a grazing contact's, where the time's own condition number is in the thousands. Without grazing contacts (cosine
// between motion and normal below 0.05) and starts that overlap: 41.09 * 2^-23, asserted at 103 * 2^-23.
// float32 and float64 disagreed about hit or none on 405 of the 3 million cases, every one of them within the asserted
// rounding of a threshold.
#pragma once

#include <stdint.h>
#include "rtk_closest_rule.h"
#include "rtk_sweep_rule.h"
#include "rtk_boxsweep_rule.h"

#define RTK_OBB_ORTHO_TOL 0.0009765625f       // 2^-10

// what 2. found: the box sweep's codes with the box's own axes in the place of the scene's, and one more: a time that no axis named
enum { RTK_OS_NONE = RTK_BS_NONE, RTK_OS_START = RTK_BS_START, RTK_OS_U0 = RTK_BS_BOX_X, RTK_OS_U1 = RTK_BS_BOX_Y, RTK_OS_U2 = RTK_BS_BOX_Z,
	RTK_OS_NORMAL = RTK_BS_NORMAL, RTK_OS_EDGE = RTK_BS_EDGE, RTK_OS_UNNAMED = RTK_BS_AXES, RTK_OS_CODES = RTK_BS_AXES + 1 };

// 0. the query: S is the path in the scene's axes with H = g (what the slab reads), F the box's frame: D = D', H = half (what the
// axis routines read; its O, tmin and tmax are the path's and are not read); U the three rows
struct rtk_obbsweep_query {
	rtk_boxsweep_query S, F;
	float U[9];
};

RTK_CLOSEST_FN void rtk_obbsweep_centre(const rtk_obbsweep_query &Q, float t, float *c) { rtk_boxsweep_centre(Q.S, t, c); }

// 0. w: the twenty floats of a rtk_obb_sweep. Returns whether the query is live; Q is filled either way
RTK_CLOSEST_FN bool rtk_obbsweep_prepare(const float *w, rtk_obbsweep_query &Q)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	Q.S.O[0] = w[0]; Q.S.O[1] = w[1]; Q.S.O[2] = w[2];
	Q.S.D[0] = w[3]; Q.S.D[1] = w[4]; Q.S.D[2] = w[5];
	Q.S.tmin = w[6]; Q.S.tmax = w[7];
	Q.F.O[0] = w[0]; Q.F.O[1] = w[1]; Q.F.O[2] = w[2];
	Q.F.tmin = w[6]; Q.F.tmax = w[7];
	Q.F.H[0] = w[8]; Q.F.H[1] = w[9]; Q.F.H[2] = w[10];
	bool finite = true;
	for (int k = 0; k < 20; k++) finite = finite && RTK_BS_FINITE(w[k]);
	for (int k = 0; k < 9; k++) Q.U[k] = w[11 + k];
	const float *u0 = Q.U, *u1 = Q.U + 3, *u2 = Q.U + 6;
	Q.F.D[0] = RTK_CL_DOT(u0[0], u0[1], u0[2], w[3], w[4], w[5]);
	Q.F.D[1] = RTK_CL_DOT(u1[0], u1[1], u1[2], w[3], w[4], w[5]);
	Q.F.D[2] = RTK_CL_DOT(u2[0], u2[1], u2[2], w[3], w[4], w[5]);
	for (int k = 0; k < 3; k++)
		Q.S.H[k] = RTK_CL_ADD(RTK_CL_ADD(RTK_CL_MUL(RTK_BS_ABS(u0[k]), w[8]), RTK_CL_MUL(RTK_BS_ABS(u1[k]), w[9])), RTK_CL_MUL(RTK_BS_ABS(u2[k]), w[10]));
	const float tol = RTK_OBB_ORTHO_TOL;
	const float d00 = RTK_CL_SUB(RTK_CL_DOT(u0[0], u0[1], u0[2], u0[0], u0[1], u0[2]), 1.0f);
	const float d11 = RTK_CL_SUB(RTK_CL_DOT(u1[0], u1[1], u1[2], u1[0], u1[1], u1[2]), 1.0f);
	const float d22 = RTK_CL_SUB(RTK_CL_DOT(u2[0], u2[1], u2[2], u2[0], u2[1], u2[2]), 1.0f);
	const float d01 = RTK_CL_DOT(u0[0], u0[1], u0[2], u1[0], u1[1], u1[2]);
	const float d02 = RTK_CL_DOT(u0[0], u0[1], u0[2], u2[0], u2[1], u2[2]);
	const float d12 = RTK_CL_DOT(u1[0], u1[1], u1[2], u2[0], u2[1], u2[2]);
	const bool ortho = RTK_BS_ABS(d00) <= tol && RTK_BS_ABS(d11) <= tol && RTK_BS_ABS(d22) <= tol &&
		RTK_BS_ABS(d01) <= tol && RTK_BS_ABS(d02) <= tol && RTK_BS_ABS(d12) <= tol;
	const bool moves = w[3] != 0.0f || w[4] != 0.0f || w[5] != 0.0f;
	return finite && moves && w[8] >= 0.0f && w[9] >= 0.0f && w[10] >= 0.0f && w[6] <= w[7] && ortho;
}

// 1. the path against the box [lo, hi] grown by g: false = empty; te the entry time, tx the leave time
RTK_CLOSEST_FN bool rtk_obbsweep_slab(const rtk_obbsweep_query &Q, const float *lo, const float *hi, float &te, float &tx)
{
	int face;
	return rtk_boxsweep_slab(Q.S, lo, hi, te, tx, face);
}

// a vector of the scene in the box's frame
RTK_CLOSEST_FN void rtk_obbsweep_to_frame(const rtk_obbsweep_query &Q, const float *w, float *p)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	p[0] = RTK_CL_DOT(Q.U[0], Q.U[1], Q.U[2], w[0], w[1], w[2]);
	p[1] = RTK_CL_DOT(Q.U[3], Q.U[4], Q.U[5], w[0], w[1], w[2]);
	p[2] = RTK_CL_DOT(Q.U[6], Q.U[7], Q.U[8], w[0], w[1], w[2]);
}

// 2. the box against the triangle (a, b, c): the axis (RTK_OS_NONE: no time) and the time by (iii)
RTK_CLOSEST_FN int rtk_obbsweep_triangle(const rtk_obbsweep_query &Q, const float *a, const float *b, const float *c, float &t_out)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	t_out = Q.S.tmax;
	// (i)
	const float lo[3] = { RTK_CL_MIN(RTK_CL_MIN(a[0], b[0]), c[0]), RTK_CL_MIN(RTK_CL_MIN(a[1], b[1]), c[1]), RTK_CL_MIN(RTK_CL_MIN(a[2], b[2]), c[2]) };
	const float hi[3] = { RTK_CL_MAX(RTK_CL_MAX(a[0], b[0]), c[0]), RTK_CL_MAX(RTK_CL_MAX(a[1], b[1]), c[1]), RTK_CL_MAX(RTK_CL_MAX(a[2], b[2]), c[2]) };
	float te, tx;
	if (!rtk_obbsweep_slab(Q, lo, hi, te, tx)) return RTK_OS_NONE;
	// (ii), from the centre at te, in the box's frame
	float Op[3];
	rtk_obbsweep_centre(Q, te, Op);
	const float sa[3] = { RTK_CL_SUB(a[0], Op[0]), RTK_CL_SUB(a[1], Op[1]), RTK_CL_SUB(a[2], Op[2]) };
	const float sb[3] = { RTK_CL_SUB(b[0], Op[0]), RTK_CL_SUB(b[1], Op[1]), RTK_CL_SUB(b[2], Op[2]) };
	const float sc[3] = { RTK_CL_SUB(c[0], Op[0]), RTK_CL_SUB(c[1], Op[1]), RTK_CL_SUB(c[2], Op[2]) };
	float wa[3], wb[3], wc[3];
	rtk_obbsweep_to_frame(Q, sa, wa);
	rtk_obbsweep_to_frame(Q, sb, wb);
	rtk_obbsweep_to_frame(Q, sc, wc);
	const float ab[3] = { RTK_CL_SUB(wb[0], wa[0]), RTK_CL_SUB(wb[1], wa[1]), RTK_CL_SUB(wb[2], wa[2]) };
	const float bc[3] = { RTK_CL_SUB(wc[0], wb[0]), RTK_CL_SUB(wc[1], wb[1]), RTK_CL_SUB(wc[2], wb[2]) };
	const float ca[3] = { RTK_CL_SUB(wa[0], wc[0]), RTK_CL_SUB(wa[1], wc[1]), RTK_CL_SUB(wa[2], wc[2]) };
	const float ac[3] = { RTK_CL_SUB(wc[0], wa[0]), RTK_CL_SUB(wc[1], wa[1]), RTK_CL_SUB(wc[2], wa[2]) };
	const float *H = Q.F.H, *D = Q.F.D;
	float enter = -__builtin_inff(), leave = RTK_CL_SUB(tx, te);
	int axis = RTK_OS_UNNAMED;
	bool some = rtk_boxsweep_axis(wa[0], wb[0], wc[0], H[0], D[0], RTK_OS_U0, enter, leave, axis);
	some = rtk_boxsweep_axis(wa[1], wb[1], wc[1], H[1], D[1], RTK_OS_U1, enter, leave, axis) && some;
	some = rtk_boxsweep_axis(wa[2], wb[2], wc[2], H[2], D[2], RTK_OS_U2, enter, leave, axis) && some;
	const float n0 = RTK_CL_SUB(RTK_CL_MUL(ab[1], ac[2]), RTK_CL_MUL(ab[2], ac[1]));
	const float n1 = RTK_CL_SUB(RTK_CL_MUL(ab[2], ac[0]), RTK_CL_MUL(ab[0], ac[2]));
	const float n2 = RTK_CL_SUB(RTK_CL_MUL(ab[0], ac[1]), RTK_CL_MUL(ab[1], ac[0]));
	const float rb = RTK_CL_ADD(RTK_CL_ADD(RTK_CL_MUL(RTK_BS_ABS(n0), H[0]), RTK_CL_MUL(RTK_BS_ABS(n1), H[1])), RTK_CL_MUL(RTK_BS_ABS(n2), H[2]));
	some = rtk_boxsweep_axis(RTK_CL_DOT(n0, n1, n2, wa[0], wa[1], wa[2]), RTK_CL_DOT(n0, n1, n2, wb[0], wb[1], wb[2]),
		RTK_CL_DOT(n0, n1, n2, wc[0], wc[1], wc[2]), rb, RTK_CL_DOT(n0, n1, n2, D[0], D[1], D[2]), RTK_OS_NORMAL, enter, leave, axis) && some;
	some = rtk_boxsweep_edge(Q.F, ab, wa, wb, wc, RTK_OS_EDGE, enter, leave, axis) && some;
	some = rtk_boxsweep_edge(Q.F, bc, wa, wb, wc, RTK_OS_EDGE + 3, enter, leave, axis) && some;
	some = rtk_boxsweep_edge(Q.F, ca, wa, wb, wc, RTK_OS_EDGE + 6, enter, leave, axis) && some;
	// (iii)
	const float after = RTK_CL_MAX(enter, 0.0f);
	if (!some || !(after <= leave)) return RTK_OS_NONE;
	const float time = RTK_CL_ADD(te, after), late = RTK_CL_MAX(time, te);
	if (late > Q.S.tmax) return RTK_OS_NONE;
	t_out = late;
	return (enter <= 0.0f && te == Q.S.tmin) ? RTK_OS_START : axis;
}

// the normal of 2.: the axis that gave the time in scene coordinates, unit length, against the motion; zeros for RTK_OS_START,
// RTK_OS_NONE and RTK_OS_UNNAMED
RTK_CLOSEST_FN void rtk_obbsweep_normal(const rtk_obbsweep_query &Q, const float *a, const float *b, const float *c, int axis, float *n)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	n[0] = 0.0f; n[1] = 0.0f; n[2] = 0.0f;
	if (axis < RTK_OS_U0 || axis >= RTK_OS_UNNAMED) return;
	// (selects, no indexing by a variable: the arrays stay registers on the device)
	float L0, L1, L2;
	bool flip;
	if (axis <= RTK_OS_U2) {
		L0 = axis == RTK_OS_U0 ? 1.0f : 0.0f;
		L1 = axis == RTK_OS_U1 ? 1.0f : 0.0f;
		L2 = axis == RTK_OS_U2 ? 1.0f : 0.0f;
		// (three comparisons, not a select between D'[0], D'[1], D'[2]: that becomes an indexed load from a private array)
		flip = (axis == RTK_OS_U0 && Q.F.D[0] > 0.0f) || (axis == RTK_OS_U1 && Q.F.D[1] > 0.0f) || (axis == RTK_OS_U2 && Q.F.D[2] > 0.0f);
	} else {
		// the primed vertices of 2. (ii) differ from one another as they do there whatever point they are measured from, but
		// only bit for bit if it is the same point: the centre at the triangle's te
		const float lo[3] = { RTK_CL_MIN(RTK_CL_MIN(a[0], b[0]), c[0]), RTK_CL_MIN(RTK_CL_MIN(a[1], b[1]), c[1]), RTK_CL_MIN(RTK_CL_MIN(a[2], b[2]), c[2]) };
		const float hi[3] = { RTK_CL_MAX(RTK_CL_MAX(a[0], b[0]), c[0]), RTK_CL_MAX(RTK_CL_MAX(a[1], b[1]), c[1]), RTK_CL_MAX(RTK_CL_MAX(a[2], b[2]), c[2]) };
		float te, tx, Op[3];
		if (!rtk_obbsweep_slab(Q, lo, hi, te, tx)) return;
		rtk_obbsweep_centre(Q, te, Op);
		const float sa[3] = { RTK_CL_SUB(a[0], Op[0]), RTK_CL_SUB(a[1], Op[1]), RTK_CL_SUB(a[2], Op[2]) };
		const float sb[3] = { RTK_CL_SUB(b[0], Op[0]), RTK_CL_SUB(b[1], Op[1]), RTK_CL_SUB(b[2], Op[2]) };
		const float sc[3] = { RTK_CL_SUB(c[0], Op[0]), RTK_CL_SUB(c[1], Op[1]), RTK_CL_SUB(c[2], Op[2]) };
		float wa[3], wb[3], wc[3];
		rtk_obbsweep_to_frame(Q, sa, wa);
		rtk_obbsweep_to_frame(Q, sb, wb);
		rtk_obbsweep_to_frame(Q, sc, wc);
		if (axis == RTK_OS_NORMAL) {
			const float ab[3] = { RTK_CL_SUB(wb[0], wa[0]), RTK_CL_SUB(wb[1], wa[1]), RTK_CL_SUB(wb[2], wa[2]) };
			const float ac[3] = { RTK_CL_SUB(wc[0], wa[0]), RTK_CL_SUB(wc[1], wa[1]), RTK_CL_SUB(wc[2], wa[2]) };
			L0 = RTK_CL_SUB(RTK_CL_MUL(ab[1], ac[2]), RTK_CL_MUL(ab[2], ac[1]));
			L1 = RTK_CL_SUB(RTK_CL_MUL(ab[2], ac[0]), RTK_CL_MUL(ab[0], ac[2]));
			L2 = RTK_CL_SUB(RTK_CL_MUL(ab[0], ac[1]), RTK_CL_MUL(ab[1], ac[0]));
		} else {
			const int k = (axis - RTK_OS_EDGE) / 3, j = (axis - RTK_OS_EDGE) % 3;
			const float e0 = k == 0 ? RTK_CL_SUB(wb[0], wa[0]) : k == 1 ? RTK_CL_SUB(wc[0], wb[0]) : RTK_CL_SUB(wa[0], wc[0]);
			const float e1 = k == 0 ? RTK_CL_SUB(wb[1], wa[1]) : k == 1 ? RTK_CL_SUB(wc[1], wb[1]) : RTK_CL_SUB(wa[1], wc[1]);
			const float e2 = k == 0 ? RTK_CL_SUB(wb[2], wa[2]) : k == 1 ? RTK_CL_SUB(wc[2], wb[2]) : RTK_CL_SUB(wa[2], wc[2]);
			L0 = j == 0 ? 0.0f : j == 1 ? -e2 : e1;
			L1 = j == 0 ? e2 : j == 1 ? 0.0f : -e0;
			L2 = j == 0 ? -e1 : j == 1 ? e0 : 0.0f;
		}
		flip = RTK_CL_DOT(L0, L1, L2, Q.F.D[0], Q.F.D[1], Q.F.D[2]) > 0.0f;
	}
	const float m0 = RTK_CL_ADD(RTK_CL_ADD(RTK_CL_MUL(L0, Q.U[0]), RTK_CL_MUL(L1, Q.U[3])), RTK_CL_MUL(L2, Q.U[6]));
	const float m1 = RTK_CL_ADD(RTK_CL_ADD(RTK_CL_MUL(L0, Q.U[1]), RTK_CL_MUL(L1, Q.U[4])), RTK_CL_MUL(L2, Q.U[7]));
	const float m2 = RTK_CL_ADD(RTK_CL_ADD(RTK_CL_MUL(L0, Q.U[2]), RTK_CL_MUL(L1, Q.U[5])), RTK_CL_MUL(L2, Q.U[8]));
	const float len = RTK_BS_SQRT(RTK_CL_DOT(m0, m1, m2, m0, m1, m2));
	if (!(len > 0.0f && len <= RTK_BS_MAX_FLOAT)) return;
	n[0] = RTK_CL_DIV(flip ? -m0 : m0, len);
	n[1] = RTK_CL_DIV(flip ? -m1 : m1, len);
	n[2] = RTK_CL_DIV(flip ? -m2 : m2, len);
}
