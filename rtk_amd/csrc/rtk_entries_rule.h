// rtk_entries_rule.h -- the interval slab test by which rtk_packet_entries_kernel (rtk_trace_packet.hip) decides whether a
// block's beam reaches a child box, and the lower bound of the entry distance it lists: for the device and for the host
// (tests/entries_rule_driver.cpp compares the two forms below, bit for bit).
//
// The beam of a 64x64-pixel block: a box of origins [olo, ohi], a box of reciprocal directions [rlo, rhi] with ONE SIGN PER
// AXIS (bit a of `neg`: both negative; rlo <= rhi, neither zero nor infinite), a margin m > 0 per axis and the smallest min_t.
// Per axis the near plane pn and the far plane pf of the child (by the sign) give
//     near = min over o in {olo, ohi}, r in {rlo, rhi} of (pn - o) * r        far = max over the same corners of (pf - o) * r
// and the child is reached if max(tmin, near_a - m_a) <= min(inf, far_a + m_a). Float subtraction and multiplication are
// monotone, so these bound what the slab test of any ray of the beam computes (rtk_trace_packet.hip).
//
// rtk_entries_child_full forms all eight products per axis. rtk_entries_child forms two: r has one sign, so (p - o) * r is
// monotone in o for either r -- the minimum is attained at o = ohi for r > 0 and at o = olo for r < 0 (the maximum at the
// other one) --, and for that difference d the product d * r is monotone in r with the direction given by the sign of d:
//     near = d * (d >= 0 ? rlo : rhi)      far = d * (d >= 0 ? rhi : rlo)
// The selected product IS one of the eight, and equal in value to their minimum / maximum; it can differ from what fminf /
// fmaxf pick only in the sign of a zero, which the margin (m > 0: x - m and x + m are the same for x = +0 and x = -0)
// removes before anything is compared or listed. Planes of +-inf (empty slots) give +-inf differences and products in both
// forms; a NaN cannot arise from finite origins and finite non-zero reciprocals.
// No fused multiply-add on either side: the library and the driver are compiled with -ffp-contract=off.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RTK_ENTRIES_FN __host__ __device__ inline
#else
#define RTK_ENTRIES_FN static inline
#endif

struct RtkEntriesBeam { float olo[3], ohi[3], rlo[3], rhi[3], m[3], tmin; uint32_t neg; };

// the specification: every corner of (origin box) x (reciprocal box)
RTK_ENTRIES_FN bool rtk_entries_child_full(const float lo[3], const float hi[3], const RtkEntriesBeam &b, float *tlo)
{
	float n = b.tmin, f = INFINITY;
	for (int a = 0; a < 3; a++) {
		const bool neg = (b.neg >> a) & 1u;
		const float pn = neg ? hi[a] : lo[a], pf = neg ? lo[a] : hi[a];
		const float n0 = (pn - b.olo[a]) * b.rlo[a], n1 = (pn - b.olo[a]) * b.rhi[a], n2 = (pn - b.ohi[a]) * b.rlo[a], n3 = (pn - b.ohi[a]) * b.rhi[a];
		const float f0 = (pf - b.olo[a]) * b.rlo[a], f1 = (pf - b.olo[a]) * b.rhi[a], f2 = (pf - b.ohi[a]) * b.rlo[a], f3 = (pf - b.ohi[a]) * b.rhi[a];
		n = fmaxf(n, fminf(fminf(n0, n1), fminf(n2, n3)) - b.m[a]);
		f = fminf(f, fmaxf(fmaxf(f0, f1), fmaxf(f2, f3)) + b.m[a]);
	}
	*tlo = n;
	return n <= f;
}

// what the kernel runs: the one corner per plane that can be the extreme
RTK_ENTRIES_FN bool rtk_entries_child(const float lo[3], const float hi[3], const RtkEntriesBeam &b, float *tlo)
{
	float n = b.tmin, f = INFINITY;
#if defined(__HIPCC__)
#pragma unroll
#endif
	for (int a = 0; a < 3; a++) {
		const bool neg = (b.neg >> a) & 1u;
		const float pn = neg ? hi[a] : lo[a], pf = neg ? lo[a] : hi[a];
		const float dn = pn - (neg ? b.olo[a] : b.ohi[a]), df = pf - (neg ? b.ohi[a] : b.olo[a]);
		const float nr = dn * (dn >= 0.0f ? b.rlo[a] : b.rhi[a]), fr = df * (df >= 0.0f ? b.rhi[a] : b.rlo[a]);
		n = fmaxf(n, nr - b.m[a]);
		f = fminf(f, fr + b.m[a]);
	}
	*tlo = n;
	return n <= f;
}
