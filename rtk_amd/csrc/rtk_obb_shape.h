// rtk_obb_shape.h -- the oriented box as a Shape of the overlap walks (rtk_overlap_walk.h says what a Shape supplies). The node
// step is the axis-aligned walk's own: rtk_box_skip against the box's bounds in the tree's axes [qlo, qhi], made once per query
// from the reach of the turned box (rtk_obb_skip). What the box's own axes add is paid per triangle record only
// (rtk_obb_candidate). rtk_obb.hip walks a scene with it, rtk_world_overlap.hip a world.
#ifndef RTK_OBB_SHAPE_H
#define RTK_OBB_SHAPE_H

#include "rtk_dev.h"
#include "rtk_obb_rule.h"

namespace {

struct Obb {
	typedef rtk_obb_query Query;
	typedef void Filter;
	struct Extra {};
	typedef rtk_obb_prepared Prepared;
	static constexpr int FLOATS = 15;
	static constexpr const char *NAME_COUNT = "rtk_dev_triangles_in_obb_count", *NAME_ALL = "rtk_dev_triangles_in_obb_all",
		*NAME_COUNTED = "rtk_dev_triangles_in_obb_counted", *NOUN = "obbs";

	static bool extras(const Filter *, const char *, Extra &) { return true; }
	static __device__ __forceinline__ bool prepare(const float *w, const Extra &, uint32_t, Prepared &Q) { return rtk_obb_prepare(w, Q); }
	static __device__ __forceinline__ bool skip(const Prepared &Q, const float *clo, const float *chi) { return rtk_obb_skip(Q, clo, chi); }
	// (the walk only runs for a live query)
	static __device__ __forceinline__ bool candidate(const Prepared Q, const float *v0, const float *v1, const float *v2, uint32_t)
	{
		return rtk_obb_candidate(Q, true, v0, v1, v2);
	}
};

} // namespace

#endif
