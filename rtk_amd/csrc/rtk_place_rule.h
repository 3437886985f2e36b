// rtk_place_rule.h -- the one rule by which a placement moves a vertex (rtk_placement, rtk_amd.h), for the host and the device:
// the ingest of a build (k_ingest, and the host's decode of callback and tiny scenes: rtk_build_ingest.hip), the gather of a refit
// (refit_tri, rtk_refit.hip) and tests/place_rule_driver.cpp all include this file and nothing else decides a placed bit.
//
// A placement is 12 floats m[0..11], a 3 x 4 matrix row by row. The vertex is made float first, exactly as an unplaced
// ingest makes it ((float) of a double); then
//     x' = ((m0 * x + m1 * y) + m2  * z) + m3
//     y' = ((m4 * x + m5 * y) + m6  * z) + m7
//     z' = ((m8 * x + m9 * y) + m10 * z) + m11
// where every product and every sum is rounded to float on its own, in this order: no fused multiply-add anywhere. On the
// device that is __fmul_rn / __fadd_rn, which the compiler never contracts; on the host the file must be compiled with
// -ffp-contract=off (the library's flags; clang is told once more by the pragma below). It is what numpy float32 arithmetic
// gives, so a test can state the expected bits without a GPU.
//   - Denormal inputs and results are kept, not flushed: gfx950 code is built with f32 denormals on (the library passes no
//     -fgpu-flush-denormals-to-zero and no fast-math), the host sets no FTZ / DAZ.
//   - The identity matrix is NOT a bit-for-bit no-op: -0 comes out as +0 (-0 + 0 * y = +0), and 0 * inf is NaN, so a vertex
//     with an infinite coordinate turns into NaNs. A host that wants its positions taken as they are calls the unplaced sibling.
//   - Where a result is NaN only that is promised, not which NaN.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define RTK_PLACE_FN __host__ __device__ inline
#else
#define RTK_PLACE_FN static inline
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define RTK_PLACE_MUL(a, b) __fmul_rn((a), (b))
#define RTK_PLACE_ADD(a, b) __fadd_rn((a), (b))
#else
#define RTK_PLACE_MUL(a, b) ((a) * (b))
#define RTK_PLACE_ADD(a, b) ((a) + (b))
#endif

// one row: ((a * x + b * y) + c * z) + d
RTK_PLACE_FN float rtk_place_row(float a, float b, float c, float d, float x, float y, float z)
{
#if defined(__clang__) && !defined(__HIP_DEVICE_COMPILE__)
#pragma clang fp contract(off)
#endif
	const float ax = RTK_PLACE_MUL(a, x), by = RTK_PLACE_MUL(b, y), cz = RTK_PLACE_MUL(c, z);
	return RTK_PLACE_ADD(RTK_PLACE_ADD(RTK_PLACE_ADD(ax, by), cz), d);
}

// the vertex (x, y, z) under placement m[12], in place
RTK_PLACE_FN void rtk_place_vertex(const float *m, float &x, float &y, float &z)
{
	const float px = rtk_place_row(m[0], m[1], m[2], m[3], x, y, z);
	const float py = rtk_place_row(m[4], m[5], m[6], m[7], x, y, z);
	const float pz = rtk_place_row(m[8], m[9], m[10], m[11], x, y, z);
	x = px; y = py; z = pz;
}
