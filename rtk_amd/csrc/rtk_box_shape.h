// rtk_box_shape.h -- the axis-aligned box as a Shape of the overlap walks (rtk_overlap_walk.h says what a Shape supplies): its
// bounds with the centre and the half extents made once per query; the skip is box against box, comparisons only (rtk_box_skip);
// a record goes through the two calls of rtk_box_candidate. rtk_box.hip walks a scene with it, rtk_world_overlap.hip a world.
#ifndef RTK_BOX_SHAPE_H
#define RTK_BOX_SHAPE_H

#include "rtk_dev.h"
#include "rtk_box_rule.h"

namespace {

struct Box {
	typedef rtk_box_query Query;
	typedef void Filter;
	struct Extra {};
	struct Prepared { float lo[3], hi[3], c[3], h[3]; };
	static constexpr int FLOATS = 6;
	static constexpr const char *NAME_COUNT = "rtk_dev_triangles_in_box_count", *NAME_ALL = "rtk_dev_triangles_in_box_all",
		*NAME_COUNTED = "rtk_dev_triangles_in_box_counted", *NOUN = "boxes";

	static bool extras(const Filter *, const char *, Extra &) { return true; }
	static __device__ __forceinline__ bool prepare(const float *w, const Extra &, uint32_t, Prepared &Q)
	{
		for (int a = 0; a < 3; a++) { Q.lo[a] = w[a]; Q.hi[a] = w[3 + a]; }
		rtk_box_centre(Q.lo, Q.hi, Q.c, Q.h);
		return rtk_box_live(Q.lo, Q.hi);
	}
	static __device__ __forceinline__ bool skip(const Prepared &Q, const float *clo, const float *chi) { return rtk_box_skip(clo, chi, Q.lo, Q.hi); }
	// rtk_box_candidate(v0, v1, v2, Q.lo, Q.hi, Q.c, Q.h), its one line spelled out: with the rule's call one level further down
	// the compiler pairs the packed multiplies of the ten axes differently, and the kernels either need 4 VGPRs more (84 in the
	// fill form: a wave per SIMD) or, with Q by value, the fill is 1 % slower on the device. This form compiles to the
	// instructions rtk_box.hip had with a kernel of its own (profiles/overlap_walk_refactor.log)
	static __device__ __forceinline__ bool candidate(const Prepared &Q, const float *v0, const float *v1, const float *v2, uint32_t)
	{
		return rtk_box_boxes_touch(v0, v1, v2, Q.lo, Q.hi) && !rtk_box_separated(v0, v1, v2, Q.c, Q.h);
	}
};

} // namespace

#endif
