// rtk_touch.hip -- rtk_dev_triangles_touching_count / rtk_dev_triangles_touching_all: for every query triangle the triangles of a
// device scene that it meets, counted, or listed in ascending primitive id into the query's own segment -- all of them or the
// first `room` --, by the rule of rtk_touch_rule.h. The result is a function of the scene's triangle records and the query alone
// (DESIGN.md "Triangles that touch a triangle"): the tree and the order of the walk only decide which records are never looked at.
//
// The walk, the stack and the launch are rtk_overlap_walk.h's; this file is the triangle: the skip is rtk_box_skip against the
// query triangle's own box, a record goes through rtk_touch_candidate, and a launch carries the filter (the slots' first_prim
// and the flags).
//
// WHAT IS HOISTED (rtk_touch_hoist, once per query, 45 floats of which 36 are distinct registers: ea0 is a1 - a0): the query's
// vertex 0, its box, a1 - a0 and a2 - a0, its three edges, nA and the three nA X ea_i; a1 and a2 themselves stay for the
// shared-vertex filter. Per pair, from one 48-byte record fetch: the record's box test first (six comparisons; most records of
// a leaf end here), then the filter, then B's three differences about a0, its edges and nB, and the seventeen axes, each of them
// five dot products and eighteen comparisons, the twelve axes that involve B with a cross product ahead. The projections of A
// on the four axes that are A's alone (nA, nA X ea_i) do not depend on the pair; they are left to the compiler, which may keep
// them in registers or form them again, the bits being the same.
//
// FLOATING POINT: the flags of rtk_closest.hip (no contraction); every bit is the rule header's.
#include "rtk_overlap_walk.h"
#include "rtk_touch_shape.h"

// TC_RESOURCES: the compiler's report (gfx950, -O3, -Rpass-analysis=kernel-resource-usage) for each instantiated form
// <FILL, COUNT>; scratch 0, no VGPR spills and no AGPRs in every one of them; the SGPRs past the 106 it may use go to lanes of a
// VGPR (counted in the VGPR column), not to memory:
//                          VGPRs  SGPRs (spilled)  LDS per workgroup   waves per SIMD by registers / workgroups per CU by LDS
//   count          <0, 0>   191    106 (12)            16 384 B                 2                   /        10
//   fill           <1, 0>   197    106 (18)            16 384 B                 2                   /        10
//   count, counted <0, 1>   197    106 (10)            16 384 B                 2                   /        10
//   fill, counted  <1, 1>   203    106 (22)            16 384 B                 2                   /        10
// A workgroup is four waves, one per SIMD, so "workgroups per CU" and "waves per SIMD" are the same number: the registers
// (512 / 192 = 2) decide in every form, the 16 KB of the stack never do. Two and a half times the box kernel's registers: 42 of
// them hold the query (what is hoisted, and a1 and a2), 30 the record, its differences about a0, its edges and nB, and the
// straight-line code of seventeen axes keeps them all alive. Asking for three or four waves (amdgpu_waves_per_eu) made the
// compiler spill 156 to 432 bytes per lane to scratch, which this kernel must not have; hoisting less or forming B's edges
// again per group of axes is the way to the next occupancy step (168 VGPRs for three waves) and has not been tried. Not tuned.

// THE SHAPE is rtk_touch_shape.h's Touch, which the walk of a world (rtk_world_overlap.hip) takes too: prepare is
// rtk_touch_hoist_query(..) and rtk_touch_live(..), skip is rtk_box_skip(..) against the query's own box, candidate is
// rtk_touch_candidate(..). The table above is of the struct as it stands there.

extern "C" uint32_t rtk_amd_touch_stack_entries(void) { return OVERLAP_LDS_STACK; }

// d_offsets == NULL: the count form (d_counts the counts); else the fill form (d_counts the written numbers, or NULL)
int rtk_launch_touch(const rtk_dev_scene *ds, const rtk_tri_query *d_tris, size_t num_queries, const rtk_ray_list *list,
	const rtk_touch_filter *filter, uint32_t *d_counts, const uint64_t *d_offsets, uint32_t *d_prims, bool fill, hipStream_t stream,
	rtk_trace_counters *counted)
{
	return rtk_launch_overlap_walk<Touch>(ds, d_tris, num_queries, list, filter, d_counts, d_offsets, d_prims, fill, stream, counted);
}
