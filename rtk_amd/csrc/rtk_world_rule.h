// rtk_world_rule.h -- the rules of an instanced world (rtk_dev_world, rtk_amd.h), for the host and the device: the inverse of a
// placement, the ray an instance's scene is walked with, and the box an instance has in the top tree. k_world_instances and
// k_world (rtk_world.hip) and tests/world_rule_driver.cpp include this file and nothing else decides one of these bits.
// No HIP, no libm.
//
// A placement is rtk_place_rule.h's: 12 floats m[0..11], a 3 x 4 matrix row by row, A = its 3 x 3 part, T = (m3, m7, m11).
//
// THE INVERSE (rtk_world_inverse). Every entry of m is made double; every product, difference, sum and quotient below is ONE
// double operation, rounded on its own, in this order (no fused multiply-add):
//     a b c        c00 = e*i - f*h    c01 = c*h - b*i    c02 = b*f - c*e
//     d e f        c10 = f*g - d*i    c11 = a*i - c*g    c12 = c*d - a*f
//     g h i        c20 = d*h - e*g    c21 = b*g - a*h    c22 = a*e - b*d
//     det = (a*c00 + b*c10) + c*c20
//     r_jk = c_jk / det                                  (the adjugate over the determinant: row j, column k of the inverse)
//     t_j  = -((r_j0*T0 + r_j1*T1) + r_j2*T2)            (the doubles r, not their float roundings)
// and inv = { r00 r01 r02 t0, r10 r11 r12 t1, r20 r21 r22 t2 }, EACH ROUNDED TO FLOAT ONCE. It is what numpy float64 arithmetic
// in this order gives, followed by astype(float32). The result is false -- the instance is DEAD -- when det is 0 or not
// finite or when any of the twelve floats is not finite (an overflow of the rounding included); inv is then not to be used.
// Denormal entries are kept, not flushed.
//
// THE RAY (rtk_world_ray). With the ray as 8 floats (origin, direction, min_t, max_t):
//     o'_j = ((inv[4j] * ox + inv[4j+1] * oy) + inv[4j+2] * oz) + inv[4j+3]            (rtk_place_row: the placement rule itself)
//     d'_j =  (inv[4j] * dx + inv[4j+1] * dy) + inv[4j+2] * dz
// every product and every sum rounded to float on its own: numpy float32 arithmetic. min_t and max_t ARE COPIED: an affine map
// keeps the ray parameter, so t means the same in every instance and in the world, and nothing is rescaled. THE DIRECTION IS
// NOT RENORMALISED.
//
// THE BOX (rtk_world_box). The eight corners of the scene's root box (corner k: x from hi if k & 1 else lo, y by k & 2, z by
// k & 4) are placed by rtk_place_vertex in the order k = 0 .. 7; lo and hi start as corner 0 and take each later corner by
// `c < lo ? c : lo`, `c > hi ? c : hi`. Then THE PADDING: with
//     B = the largest of |lo_x| |lo_y| |lo_z| |hi_x| |hi_y| |hi_z|      (|x| is x < 0 ? -x : x; taken by `v > B ? v : B` from 0)
//     S = the largest of |m3| |m7| |m11|                                (the same way)
//     pad = RTK_WORLD_PAD * (B + S)                                      (one float sum, one float product; RTK_WORLD_PAD = 2^-11)
// every lo becomes lo - pad and every hi becomes hi + pad. Why 2^-11 covers what the inverse and the transformed ray round
// away for placements of condition number up to 100: DESIGN.md 3.23. The result is false when a bound is not finite.
//
// THE MARGIN OF THE TOP TREE'S SLAB TEST (rtk_world_margin) is the ray's half of the same bound: every box of the top tree is
// grown by  e = RTK_WORLD_PAD * (O + W),  O the largest |origin coordinate|, W the largest |plane| of the top tree.
#pragma once

#include <stdint.h>

#include "rtk_place_rule.h"

#define RTK_WORLD_PAD 0x1p-11f

#if defined(__HIP_DEVICE_COMPILE__)
#define RTK_WORLD_DMUL(a, b) __dmul_rn((a), (b))
#define RTK_WORLD_DADD(a, b) __dadd_rn((a), (b))
#define RTK_WORLD_DSUB(a, b) __dsub_rn((a), (b))
#define RTK_WORLD_DDIV(a, b) __ddiv_rn((a), (b))
#else
#define RTK_WORLD_DMUL(a, b) ((a) * (b))
#define RTK_WORLD_DADD(a, b) ((a) + (b))
#define RTK_WORLD_DSUB(a, b) ((a) - (b))
#define RTK_WORLD_DDIV(a, b) ((a) / (b))
#endif

// (x - x is 0 for every finite x and a NaN for an infinity or a NaN)
RTK_PLACE_FN bool rtk_world_finite(float x) { return x - x == 0.0f; }
RTK_PLACE_FN bool rtk_world_finite_d(double x) { return x - x == 0.0; }
RTK_PLACE_FN float rtk_world_abs(float x) { return x < 0.0f ? -x : x; }

// p*q - r*s: two products, one difference
RTK_PLACE_FN double rtk_world_cofactor(double p, double q, double r, double s)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	return RTK_WORLD_DSUB(RTK_WORLD_DMUL(p, q), RTK_WORLD_DMUL(r, s));
}

// (x*p + y*q) + z*r
RTK_PLACE_FN double rtk_world_dot(double x, double p, double y, double q, double z, double r)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	return RTK_WORLD_DADD(RTK_WORLD_DADD(RTK_WORLD_DMUL(x, p), RTK_WORLD_DMUL(y, q)), RTK_WORLD_DMUL(z, r));
}

// false: the placement is not invertible in float (the instance is dead)
RTK_PLACE_FN bool rtk_world_inverse(const float *m, float *inv)
{
	const double a = m[0], b = m[1], c = m[2], d = m[4], e = m[5], f = m[6], g = m[8], h = m[9], i = m[10];
	const double T0 = m[3], T1 = m[7], T2 = m[11];
	double co[9];
	co[0] = rtk_world_cofactor(e, i, f, h); co[1] = rtk_world_cofactor(c, h, b, i); co[2] = rtk_world_cofactor(b, f, c, e);
	co[3] = rtk_world_cofactor(f, g, d, i); co[4] = rtk_world_cofactor(a, i, c, g); co[5] = rtk_world_cofactor(c, d, a, f);
	co[6] = rtk_world_cofactor(d, h, e, g); co[7] = rtk_world_cofactor(b, g, a, h); co[8] = rtk_world_cofactor(a, e, b, d);
	const double det = rtk_world_dot(a, co[0], b, co[3], c, co[6]);
	bool live = det != 0.0 && rtk_world_finite_d(det);
	for (int j = 0; j < 3; j++) {
		const double r0 = RTK_WORLD_DDIV(co[3 * j], det), r1 = RTK_WORLD_DDIV(co[3 * j + 1], det), r2 = RTK_WORLD_DDIV(co[3 * j + 2], det);
		const double t = -rtk_world_dot(r0, T0, r1, T1, r2, T2);
		inv[4 * j] = (float)r0; inv[4 * j + 1] = (float)r1; inv[4 * j + 2] = (float)r2; inv[4 * j + 3] = (float)t;
	}
	for (int k = 0; k < 12; k++) live = live && rtk_world_finite(inv[k]);
	return live;
}

// ray_in, ray_out: origin, direction, min_t, max_t (8 floats; they may not overlap)
RTK_PLACE_FN void rtk_world_ray(const float *inv, const float *ray_in, float *ray_out)
{
	for (int j = 0; j < 3; j++) {
		ray_out[j] = rtk_place_row(inv[4 * j], inv[4 * j + 1], inv[4 * j + 2], inv[4 * j + 3], ray_in[0], ray_in[1], ray_in[2]);
		const float ax = RTK_PLACE_MUL(inv[4 * j], ray_in[3]), by = RTK_PLACE_MUL(inv[4 * j + 1], ray_in[4]), cz = RTK_PLACE_MUL(inv[4 * j + 2], ray_in[5]);
		ray_out[3 + j] = RTK_PLACE_ADD(RTK_PLACE_ADD(ax, by), cz);
	}
	ray_out[6] = ray_in[6];
	ray_out[7] = ray_in[7];
}

// the padded world box of a scene whose root box is [root_lo, root_hi] under placement m; false: a bound is not finite
RTK_PLACE_FN bool rtk_world_box(const float *root_lo, const float *root_hi, const float *m, float *lo, float *hi)
{
	for (int k = 0; k < 8; k++) {
		float c[3] = { (k & 1) ? root_hi[0] : root_lo[0], (k & 2) ? root_hi[1] : root_lo[1], (k & 4) ? root_hi[2] : root_lo[2] };
		rtk_place_vertex(m, c[0], c[1], c[2]);
		for (int a = 0; a < 3; a++) {
			if (k == 0) { lo[a] = hi[a] = c[a]; continue; }
			lo[a] = c[a] < lo[a] ? c[a] : lo[a];
			hi[a] = c[a] > hi[a] ? c[a] : hi[a];
		}
	}
	float B = 0.0f, S = 0.0f;
	for (int a = 0; a < 3; a++) {
		const float l = rtk_world_abs(lo[a]), u = rtk_world_abs(hi[a]), t = rtk_world_abs(m[4 * a + 3]);
		B = l > B ? l : B;
		B = u > B ? u : B;
		S = t > S ? t : S;
	}
	const float pad = RTK_PLACE_MUL(RTK_WORLD_PAD, RTK_PLACE_ADD(B, S));
	bool finite = true;
	for (int a = 0; a < 3; a++) {
		lo[a] = RTK_PLACE_ADD(lo[a], -pad);
		hi[a] = RTK_PLACE_ADD(hi[a], pad);
		finite = finite && rtk_world_finite(lo[a]) && rtk_world_finite(hi[a]);
	}
	return finite;
}

// what every box of the top tree is grown by for a ray from `origin`; world_bound: the largest |plane| of the top tree
RTK_PLACE_FN float rtk_world_margin(const float *origin, float world_bound)
{
	float O = 0.0f;
	for (int a = 0; a < 3; a++) { const float v = rtk_world_abs(origin[a]); O = v > O ? v : O; }
	return RTK_PLACE_MUL(RTK_WORLD_PAD, RTK_PLACE_ADD(O, world_bound));
}
