// rtk_sign_rule.h -- the one rule by which a closest-point answer gets its sign (rtk_dev_signed_distances, rtk_amd.h), for the
// host and the device: the kernels (rtk_sign.hip) and tests/sign_rule_driver.cpp include this file and nothing else decides a bit
// of the table of pseudonormals or of a signed distance. Both are pure functions of the scene's SET of triangle records (and the
// query): slots, leaves, the tree and the way the scene was made play no part.
//
// The method is Baerentzen and Aanaes's angle-weighted pseudonormal ("Signed distance computation using the angle weighted
// pseudonormal", 2005): the sign of dot(p - q, N), N the normal of the FEATURE of the triangle the closest point q lies on.
//
// Every product, sum, difference and quotient below is ONE float operation, rounded on its own, in the order written: no fused
// multiply-add anywhere (RTK_CL_* of rtk_closest_rule.h: __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn on the device,
// -ffp-contract=off and the pragma "fp contract(off)" on the host). sqrt is the correctly rounded one (__builtin_sqrtf on both sides:
// the library is built with -fhip-fp32-correctly-rounded-divide-sqrt; HIP's __fsqrt_rn is the native approximation and is NOT used). No libm function is called: device and host libm differ,
// and the table must be bit-equal across both. It is what numpy float32 arithmetic gives, operation by operation (tests/sign_ref.py).
// Denormal inputs and results are kept. dot(x, y) = (x0 * y0 + x1 * y1) + x2 * y2 and
// cross(x, y) = (x1 * y2 - x2 * y1, x2 * y0 - x0 * y2, x0 * y1 - x1 * y0), |x| = sqrt(dot(x, x)).
//
// 1. SAME PLACE (rtk_sign_same_place). A corner is one vertex of one triangle record: (prim, k), k = 0, 1, 2 for a, b, c =
//    DevTri.v0 / v1 / v2. Two corners are at the same place iff their three floats compare equal AS NUMBERS: -0 equals +0 (a sort
//    key of a coordinate maps both zeros to one word: rtk_sign_key), a NaN coordinate is equal to nothing, itself included (such
//    a corner is a place of its own). Vertex indices and mesh numbers play no part: a seam whose vertices are duplicated under
//    other indices is welded, and so are two meshes that meet. A placed mesh's records are world positions already.
// 2. UNIT FACE NORMAL of a record (a, b, c) (rtk_sign_unit_normal): n = cross(b - a, c - a), len = |n|, unit = n / len. If len is
//    0, not finite or a NaN the triangle HAS NO NORMAL: it contributes nothing to any sum, and it is counted as a degenerate
//    triangle. It still gets the sums of its neighbours in its own rows of the table, and it is still a triangle record to 5.'s counts.
// 3. CORNER ANGLE (rtk_sign_angle). The angle at corner X between the two edges e1, e2 that leave it (at a: b - a, c - a; at b:
//    c - b, a - b; at c: a - c, b - c) is rtk_sign_angle(|cross(e1, e2)|, dot(e1, e2)): an atan2(y, x) written here from +, -, *, /
//    and selects only.
//        ay = y < 0 ? 0 - y : y     ax = x < 0 ? 0 - x : x     mx = ay > ax ? ay : ax     mn = ay > ax ? ax : ay
//        mx == 0 (or both NaN-free zeros of either sign):   the angle is +0                        (case Z)
//        t = mn / mx      s = t * t
//        r = (((((C5 * s + C4) * s + C3) * s + C2) * s + C1) * s + C0) * t          (Horner, each * and + rounded on its own)
//        ay > ax:   r = PIO2 - r        (the quotient was x / y: case S)
//        x < 0:     r = PI - r          (the left half plane: case L)
//        y < 0:     r = 0 - r           (the lower half plane: case N)
//    The cases S, L, N are applied in that order, each to the result of the one before. Exactly: (0, x > 0) = +0; (y > 0, 0) =
//    RTK_SIGN_PIO2; (0, 0) = +0; (0, x < 0) = RTK_SIGN_PI. Inputs that are not finite give a NaN or a value of no meaning; a
//    triangle with such a cross product has no normal by 2. and its angle is never used.
//    The polynomial is an odd one of degree 11, fitted to atan on [0, 1]. Its absolute error against float64 math.atan2, measured
//    by tests/test_sign_cpu.py over the grid |y| / |x| = 2^(k / 8), k = -160 .. 160 (2^-20 .. 2^20), times x in {1, 3, 2^-10,
//    1.7 * 2^10}, all four sign combinations, plus the exact zeros: 1.82e-06 rad. The test asserts twice that, 3.64e-06; the
//    condition for the sign is 1e-5 rad, and the weights of 4. need no more.
// 4. VERTEX PSEUDONORMAL of a place P: the sum over every corner (prim, k) at P whose triangle has a normal of angle * unit normal
//    (three products), componentwise, added in ASCENDING (prim, k) order STARTING FROM THE FIRST TERM (not from 0.0: the sign of a
//    zero sum is the first term's way). A place none of whose triangles has a normal has the pseudonormal (+0, +0, +0).
// 5. EDGE PSEUDONORMAL of the unordered pair of places {P, Q}, P != Q: the sum of the unit normals of every triangle record that
//    has a corner at P and another at Q and has a normal, in ascending prim order, starting from the first term; (+0, +0, +0) if
//    there is none. A record counts once however many of its corners lie at P or Q. For an edge of a triangle whose two ends are
//    at the same place the edge normal is the vertex pseudonormal of that place.
//    Counts of the same walk (rtk_dev_sign_info). For every (prim, edge) whose two ends are at different places, with m = the
//    number of OTHER triangle records (with or without a normal) that have a corner at each of the two places:
//        m == 0   a boundary side        m >= 2   a non-manifold side
//        m == 1   an inconsistent side iff the other record runs the edge in the same direction. A record (a, b, c) runs a -> b,
//                 b -> c, c -> a; the other record's direction is taken from its lowest corner at P and its lowest corner at Q.
//    (prim, edge) pairs whose ends are at one place are in none of the three. places = the number of distinct places (every
//    corner with a NaN coordinate is one of its own).
// 6. THE TABLE: 18 floats per primitive, at 18 * prim: the edge pseudonormals of ab, ac, bc, then the vertex pseudonormals of a, b,
//    c. It needs exactly one record per primitive id.
// 7. THE SIGN (rtk_sign_signed). Given the answer (prim, q) of the closest rule to the query p, rtk_closest_triangle(p, a, b, c) is
//    evaluated again on that record; its region picks N:
//        1, 2, 4   the vertex pseudonormals of a, b, c             3, 5, 6   the edge pseudonormals of ab, ac, bc
//        7         the raw cross product n of 2., NOT normalised
//    s = dot(p - q, N) with the rule's clamped q (componentwise differences first). The point is INSIDE iff s < 0; a zero or a NaN
//    s is outside. signed = inside ? 0 - sqrt(dist2) : sqrt(dist2). A miss of the closest rule (no triangle within max_dist2; a
//    query whose dist2 is a NaN never has an answer) has no side: signed = RTK_SIGN_INF, the record is the closest call's miss.
//
// WHAT IS PROMISED. On a closed, consistently wound, non-self-intersecting surface the sign is the true one, up to the float
// rounding of a dot product that is near zero only for points near the surface's tangent planes (there p - q is all but
// perpendicular to N and the distance itself is what matters). On an open or inconsistently wound mesh the evaluation still
// terminates and is deterministic; the sign near the defects means nothing. The counts of 5. tell which case a scene is in:
// closed = no boundary, no non-manifold and no inconsistent side.
#pragma once

#include <stdint.h>

#include "rtk_closest_rule.h"

// (the same on the device: under the library's flag the builtin is IEEE's root, while HIP's __fsqrt_rn is the native approximation)
#define RTK_SIGN_SQRT(x) __builtin_sqrtf((x))

#define RTK_SIGN_PIO2 1.57079637f          // 0x3fc90fdb
#define RTK_SIGN_PI 3.14159274f            // 0x40490fdb
#define RTK_SIGN_C0 0.999977231f           // 0x3f7ffe82
#define RTK_SIGN_C1 (-0.332622826f)        // 0xbeaa4d8a
#define RTK_SIGN_C2 0.193540394f           // 0x3e462f74
#define RTK_SIGN_C3 (-0.116426520f)        // 0xbdee7107
#define RTK_SIGN_C4 0.0526473969f          // 0x3d57a4cc
#define RTK_SIGN_C5 (-0.0117191551f)       // 0xbc4001b3
#define RTK_SIGN_INF 3.402823e+38f         // RTK_INF (rtk.h), the same literal: what a miss is given for a signed distance

// 1. the sort key of one coordinate: equal numbers give equal words (the order of the words means nothing)
RTK_CLOSEST_FN uint32_t rtk_sign_key(uint32_t bits) { return (bits & 0x7fffffffu) == 0u ? 0u : bits; }
RTK_CLOSEST_FN bool rtk_sign_same_place(const float *x, const float *y) { return x[0] == y[0] && x[1] == y[1] && x[2] == y[2]; }

RTK_CLOSEST_FN void rtk_sign_cross(const float *x, const float *y, float *n)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	n[0] = RTK_CL_SUB(RTK_CL_MUL(x[1], y[2]), RTK_CL_MUL(x[2], y[1]));
	n[1] = RTK_CL_SUB(RTK_CL_MUL(x[2], y[0]), RTK_CL_MUL(x[0], y[2]));
	n[2] = RTK_CL_SUB(RTK_CL_MUL(x[0], y[1]), RTK_CL_MUL(x[1], y[0]));
}

// 3. atan2(y, x) by the stated cases
RTK_CLOSEST_FN float rtk_sign_angle(float y, float x)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	const float ay = y < 0.0f ? RTK_CL_SUB(0.0f, y) : y, ax = x < 0.0f ? RTK_CL_SUB(0.0f, x) : x;
	const bool swap = ay > ax;
	const float mx = swap ? ay : ax, mn = swap ? ax : ay;
	if (mx == 0.0f) return 0.0f;                                                      // Z
	const float t = RTK_CL_DIV(mn, mx), s = RTK_CL_MUL(t, t);
	float r = RTK_SIGN_C5;
	r = RTK_CL_ADD(RTK_CL_MUL(r, s), RTK_SIGN_C4);
	r = RTK_CL_ADD(RTK_CL_MUL(r, s), RTK_SIGN_C3);
	r = RTK_CL_ADD(RTK_CL_MUL(r, s), RTK_SIGN_C2);
	r = RTK_CL_ADD(RTK_CL_MUL(r, s), RTK_SIGN_C1);
	r = RTK_CL_ADD(RTK_CL_MUL(r, s), RTK_SIGN_C0);
	r = RTK_CL_MUL(r, t);
	if (swap) r = RTK_CL_SUB(RTK_SIGN_PIO2, r);                                       // S
	if (x < 0.0f) r = RTK_CL_SUB(RTK_SIGN_PI, r);                                     // L
	if (y < 0.0f) r = RTK_CL_SUB(0.0f, r);                                            // N
	return r;
}

// 2. the raw cross product n[3] and the unit normal unit[3] of (a, b, c); false: the triangle has no normal (unit is then not to be used)
RTK_CLOSEST_FN bool rtk_sign_unit_normal(const float *a, const float *b, const float *c, float *n, float *unit)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	const float ab[3] = { RTK_CL_SUB(b[0], a[0]), RTK_CL_SUB(b[1], a[1]), RTK_CL_SUB(b[2], a[2]) };
	const float ac[3] = { RTK_CL_SUB(c[0], a[0]), RTK_CL_SUB(c[1], a[1]), RTK_CL_SUB(c[2], a[2]) };
	rtk_sign_cross(ab, ac, n);
	const float len = RTK_SIGN_SQRT(RTK_CL_DOT(n[0], n[1], n[2], n[0], n[1], n[2]));
	unit[0] = RTK_CL_DIV(n[0], len); unit[1] = RTK_CL_DIV(n[1], len); unit[2] = RTK_CL_DIV(n[2], len);
	return len > 0.0f && len < __builtin_inff();                                      // (a NaN fails both)
}

// 3. the angle at corner x between the edges to y and to z (at a: (a, b, c); at b: (b, c, a); at c: (c, a, b))
RTK_CLOSEST_FN float rtk_sign_corner_angle(const float *x, const float *y, const float *z)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	const float e1[3] = { RTK_CL_SUB(y[0], x[0]), RTK_CL_SUB(y[1], x[1]), RTK_CL_SUB(y[2], x[2]) };
	const float e2[3] = { RTK_CL_SUB(z[0], x[0]), RTK_CL_SUB(z[1], x[1]), RTK_CL_SUB(z[2], x[2]) };
	float k[3];
	rtk_sign_cross(e1, e2, k);
	return rtk_sign_angle(RTK_SIGN_SQRT(RTK_CL_DOT(k[0], k[1], k[2], k[0], k[1], k[2])), RTK_CL_DOT(e1[0], e1[1], e1[2], e2[0], e2[1], e2[2]));
}

// 4. the three terms angle * unit of a record that has a normal: term[3 * k + i], k the corner
RTK_CLOSEST_FN void rtk_sign_corner_terms(const float *a, const float *b, const float *c, const float *unit, float *term)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	const float w[3] = { rtk_sign_corner_angle(a, b, c), rtk_sign_corner_angle(b, c, a), rtk_sign_corner_angle(c, a, b) };
	for (int k = 0; k < 3; k++)
		for (int i = 0; i < 3; i++) term[3 * k + i] = RTK_CL_MUL(w[k], unit[i]);
}

// 5. does a record that has its corner kp at P and its corner kq at Q run the edge from P to Q? (a -> b, b -> c, c -> a)
RTK_CLOSEST_FN bool rtk_sign_runs_forward(int kp, int kq) { return kq == (kp + 1) % 3; }

// 7. the signed distance of p from the record (a, b, c) that answers it, tab its 18 floats of the table; q[3] the clamped closest
// point, region the case taken (1 .. 7). A dist2 that is a NaN cannot be an answer's.
RTK_CLOSEST_FN float rtk_sign_signed(const float *p, const float *a, const float *b, const float *c, const float *tab, float *q, int &region)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	float u, v;
	const float dist2 = rtk_closest_triangle(p, a, b, c, q, u, v, region);
	float N[3];
	if (region == 7) {
		const float ab[3] = { RTK_CL_SUB(b[0], a[0]), RTK_CL_SUB(b[1], a[1]), RTK_CL_SUB(b[2], a[2]) };
		const float ac[3] = { RTK_CL_SUB(c[0], a[0]), RTK_CL_SUB(c[1], a[1]), RTK_CL_SUB(c[2], a[2]) };
		rtk_sign_cross(ab, ac, N);
	} else {
		//                       region:   1  2  3   4  5  6
		const int at = region == 1 ? 9 : region == 2 ? 12 : region == 3 ? 0 : region == 4 ? 15 : region == 5 ? 3 : 6;
		N[0] = tab[at]; N[1] = tab[at + 1]; N[2] = tab[at + 2];
	}
	const float d0 = RTK_CL_SUB(p[0], q[0]), d1 = RTK_CL_SUB(p[1], q[1]), d2 = RTK_CL_SUB(p[2], q[2]);
	const float s = RTK_CL_DOT(d0, d1, d2, N[0], N[1], N[2]);
	const float r = RTK_SIGN_SQRT(dist2);
	return s < 0.0f ? RTK_CL_SUB(0.0f, r) : r;
}
