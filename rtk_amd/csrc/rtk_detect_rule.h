// rtk_detect_rule.h -- is a batch a row-major image nobody told us about? The rule, once, for the device (rtk_detect.hip:
// k_detect_row, k_detect_check) and for the host (rtk_detect_host below, for rtk_trace_rays in rtk_host_calls.hip; tests/detect_rule_driver.cpp).
//
// The reference's interface has no notion of an image (rtk.h:129); a host that only hands over rays should still get the packet
// kernels. Along a row of an image the step from one ray to the next (origin and direction, six
// numbers) changes slowly; from the last ray of a row to the first of the next it jumps by about a row's width. The first such
// jump among the first RTK_DETECT_LOOK rays gives the candidate width. Then up to RTK_DETECT_ROWS rows are looked at: there must
// be a jump at the end of every one, and none at three places inside it. A wrong guess can only cost speed -- tiles whose rays
// do not form a beam are handed back by the packet kernels, records are the same on every path -- so this is a heuristic with
// a cheap test, not a proof.
#pragma once

#include "rtk.h"

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RTK_DETECT_FN __host__ __device__ inline
#else
#define RTK_DETECT_FN static inline
#endif

#define RTK_DETECT_LOOK ((size_t)1 << 17)      // rays among which the first jump is looked for
#define RTK_DETECT_ROWS 256u                   // rows whose ends and insides are looked at
#define RTK_DETECT_NO_JUMP 0xffffffffu

// batches the look is for at all; where it stops looking for the first jump
RTK_DETECT_FN bool rtk_detect_sized(unsigned long long n) { return n >= 4ull && n <= 0x40000000ull; }
RTK_DETECT_FN uint32_t rtk_detect_limit(unsigned long long n) { return (uint32_t)(n < RTK_DETECT_LOOK ? n : RTK_DETECT_LOOK); }

// rays i-1, i, i+1: does the step i -> i+1 differ from the step i-1 -> i by more than eight times the latter?
RTK_DETECT_FN bool rtk_detect_step_jumps(const rtk_ray *rays, size_t i)
{
	const float *a = reinterpret_cast<const float *>(rays + i - 1), *b = reinterpret_cast<const float *>(rays + i), *c = reinterpret_cast<const float *>(rays + i + 1);
	float m = 0.0f, dmax = 0.0f;
#if defined(__HIPCC__)
#pragma unroll
#endif
	for (int k = 0; k < 6; k++) {
		const float s0 = b[k] - a[k], s1 = c[k] - b[k];
		m = fmaxf(m, fabsf(s0));
		dmax = fmaxf(dmax, fabsf(s1 - s0));
	}
	return !(dmax <= 8.0f * m);
}

// The image a first jump at ray `first` (1 .. limit - 2, or RTK_DETECT_NO_JUMP) proposes: rows of first + 1 rays.
struct RtkDetectCandidate {
	uint32_t w;                    // rays per row
	unsigned long long rows;
	unsigned long long stride;     // every stride-th row is looked at
};
RTK_DETECT_FN bool rtk_detect_candidate(uint32_t first, unsigned long long n, RtkDetectCandidate *c)
{
	const uint32_t w = first + 1u;
	if (first == RTK_DETECT_NO_JUMP || w < 64u || (n % w) != 0ull || n / w < 2ull || n / w > 0xffffffffull) return false;
	c->w = w;
	c->rows = n / w;
	c->stride = c->rows > RTK_DETECT_ROWS ? c->rows / RTK_DETECT_ROWS : 1ull;
	return true;
}

// Look k (0 .. RTK_DETECT_ROWS - 1) speaks against the candidate: its row's end does not jump, or a place inside the row does.
// (The last row has no end to look at, and is not looked at.)
RTK_DETECT_FN bool rtk_detect_row_bad(const rtk_ray *rays, const RtkDetectCandidate &c, uint32_t k)
{
	const unsigned long long r = (unsigned long long)k * c.stride;
	if (r + 1ull >= c.rows) return false;
	bool bad = !rtk_detect_step_jumps(rays, (size_t)((r + 1ull) * c.w - 1ull));
	for (uint32_t q = 1; q < 4u; q++) bad = bad || rtk_detect_step_jumps(rays, (size_t)(r * c.w) + (size_t)q * (c.w / 4u));
	return bad;
}

// The whole look, on rays the host can read: *w_out x *h_out = the image the batch is (row-major, w * h = n), or 0 x 0.
static inline void rtk_detect_host(const rtk_ray *rays, size_t n, uint32_t *w_out, uint32_t *h_out)
{
	*w_out = *h_out = 0u;
	if (!rtk_detect_sized(n)) return;
	const uint32_t limit = rtk_detect_limit(n);
	uint32_t first = RTK_DETECT_NO_JUMP;
	for (uint32_t i = 1; i + 1 < limit; i++) if (rtk_detect_step_jumps(rays, i)) { first = i; break; }
	RtkDetectCandidate c;
	if (!rtk_detect_candidate(first, n, &c)) return;
	for (uint32_t k = 0; k < RTK_DETECT_ROWS; k++) if (rtk_detect_row_bad(rays, c, k)) return;
	*w_out = c.w;
	*h_out = (uint32_t)c.rows;
}
