// rtk_box.hip -- rtk_dev_triangles_in_box_count / rtk_dev_triangles_in_box_all: for every axis-aligned query box the triangles of
// a device scene that touch it, counted, or listed in ascending primitive id into the query's own segment -- all of them or the
// first `room` --, by the rule of rtk_box_rule.h. The result is a function of the scene's triangle records and the query alone
// (DESIGN.md "Triangles that touch a box"): the tree and the order of the walk only decide which records are never looked at.
//
// The walk, the stack and the launch are rtk_overlap_walk.h's; this file is the box: its bounds with the centre and the half
// extents made once per query; the skip is box against box, comparisons only (rtk_box_skip); a record goes through the
// two calls of rtk_box_candidate. tests/test_gpu_box.py makes a walk that needs the spill area.
//
// FLOATING POINT: the flags of rtk_closest.hip (no contraction); every bit is the rule header's.
#include "rtk_overlap_walk.h"

// BX_RESOURCES: the compiler's report (gfx950, -O3, -Rpass-analysis=kernel-resource-usage) for each instantiated form
// <FILL, COUNT>; scratch 0, no SGPR or VGPR spills and no AGPRs in every one of them:
//                          VGPRs  SGPRs  LDS per workgroup   waves per SIMD by registers / workgroups per CU by LDS
//   count          <0, 0>   76      88       16 384 B                 6                   /        10
//   fill           <1, 0>   80      96       16 384 B                 6                   /        10
//   count, counted <0, 1>   84      86       16 384 B                 5                   /        10
//   fill, counted  <1, 1>   86     100       16 384 B                 5                   /        10
// A workgroup is four waves, one per SIMD, so "workgroups per CU" and "waves per SIMD" are the same number: the registers
// (512 / 80 = 6) decide in every form, the 16 KB of the stack never do.

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

extern "C" uint32_t rtk_amd_box_stack_entries(void) { return OVERLAP_LDS_STACK; }

// d_offsets == NULL: the count form (d_counts the counts); else the fill form (d_counts the written numbers, or NULL)
int rtk_launch_box(const rtk_dev_scene *ds, const rtk_box_query *d_boxes, size_t num_queries, const rtk_ray_list *list,
	uint32_t *d_counts, const uint64_t *d_offsets, uint32_t *d_prims, bool fill, hipStream_t stream, rtk_trace_counters *counted)
{
	return rtk_launch_overlap_walk<Box>(ds, d_boxes, num_queries, list, nullptr, d_counts, d_offsets, d_prims, fill, stream, counted);
}
