// rtk_touch_shape.h -- the query triangle as a Shape of the overlap walks (rtk_overlap_walk.h says what a Shape supplies): the
// skip is rtk_box_skip against the query triangle's own box, a record goes through rtk_touch_candidate, and a launch carries the
// filter (the slots' first_prim and the flags). What is hoisted per query is said in rtk_touch.hip, which walks a scene with it;
// rtk_world_overlap.hip walks a world.
#ifndef RTK_TOUCH_SHAPE_H
#define RTK_TOUCH_SHAPE_H

#include "rtk_dev.h"
#include "rtk_box_rule.h"
#include "rtk_touch_rule.h"

static_assert(RTK_TOUCH_RULE_SKIP_SHARED_VERTEX == RTK_TOUCH_SKIP_SHARED_VERTEX, "the rule header's flag is the interface's");
static_assert(sizeof(rtk_tri_query) == 36, "a float32 [n, 9] tensor is a batch of queries");

namespace {

struct Touch {
	typedef rtk_tri_query Query;
	typedef rtk_touch_filter Filter;
	struct Extra {
		const uint32_t *first_prim;    // or NULL: 0 for every query; indexed by query slot
		uint32_t flags;                // RTK_TOUCH_SKIP_SHARED_VERTEX
	};
	struct Prepared {
		rtk_touch_hoist q;
		float a0[3], a1[3], a2[3];
		uint32_t first, flags;
	};
	static constexpr int FLOATS = 9;
	static constexpr const char *NAME_COUNT = "rtk_dev_triangles_touching_count", *NAME_ALL = "rtk_dev_triangles_touching_all",
		*NAME_COUNTED = "rtk_dev_triangles_touching_counted", *NOUN = "triangles";

	static bool extras(const Filter *filter, const char *who, Extra &x)
	{
		if (filter && (filter->struct_size < sizeof(rtk_touch_filter) || (filter->flags & ~(uint32_t)RTK_TOUCH_SKIP_SHARED_VERTEX) != 0u)) {
			rtk_set_error("%s: bad filter (struct_size %u, flags %#x)", who, filter->struct_size, filter->flags);
			return false;
		}
		x.first_prim = filter ? filter->d_first_prim : nullptr;
		x.flags = filter ? filter->flags : 0u;
		return true;
	}
	static __device__ __forceinline__ bool prepare(const float *w, const Extra &x, uint32_t r, Prepared &Q)
	{
		for (int a = 0; a < 3; a++) { Q.a0[a] = w[a]; Q.a1[a] = w[3 + a]; Q.a2[a] = w[6 + a]; }
		Q.first = x.first_prim ? x.first_prim[r] : 0u;
		Q.flags = x.flags;
		rtk_touch_hoist_query(Q.a0, Q.a1, Q.a2, Q.q);
		return rtk_touch_live(Q.a0, Q.a1, Q.a2);
	}
	static __device__ __forceinline__ bool skip(const Prepared &Q, const float *clo, const float *chi) { return rtk_box_skip(clo, chi, Q.q.lo, Q.q.hi); }
	static __device__ __forceinline__ bool candidate(const Prepared Q, const float *b0, const float *b1, const float *b2, uint32_t prim)
	{
		return rtk_touch_candidate(Q.q, Q.a0, Q.a1, Q.a2, b0, b1, b2, prim, Q.first, Q.flags);
	}
};

} // namespace

#endif
