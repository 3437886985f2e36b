// rtk_obb.hip -- rtk_dev_triangles_in_obb_count / rtk_dev_triangles_in_obb_all: for every oriented query box the triangles of a
// device scene that touch it, counted, or listed in ascending primitive id into the query's own segment -- all of them or the
// first `room` --, by the rule of rtk_obb_rule.h. The result is a function of the scene's triangle records and the query alone
// (DESIGN.md "Triangles that touch an oriented box"): the tree and the order of the walk only decide which records are never
// looked at.
//
// The walk, the stack and the launch are rtk_overlap_walk.h's; this file is the oriented box. The node step is the axis-aligned
// walk's own: rtk_box_skip against the box's bounds in the scene's axes [qlo, qhi], made once per query from the reach of the
// turned box (rtk_obb_skip). What the box's own axes add is paid per triangle record only: three differences and three dots per
// vertex, then thirteen axes (rtk_obb_candidate). The query's invariants -- centre, half, the nine axis floats, qlo, qhi: 27
// floats -- stay in registers across the walk.
//
// FLOATING POINT: the flags of rtk_closest.hip (no contraction); every bit is the rule header's.
#include "rtk_overlap_walk.h"
#include "rtk_obb_shape.h"

// OB_RESOURCES: the compiler's report (gfx950, -O3, -Rpass-analysis=kernel-resource-usage) for each instantiated form
// <FILL, COUNT>; scratch 0, no VGPR spills and no AGPRs in every one of them, so the node loop and the record loop touch no
// private memory: the per-triangle arrays of the rule are registers. (The counting fill form, which is not for timing, moves two
// SGPRs into lanes of a VGPR; the other three forms spill no SGPR.)
//                          VGPRs  SGPRs  LDS per workgroup   waves per SIMD by registers / workgroups per CU by LDS
//   count          <0, 0>   88      96       16 384 B                 5                   /        10
//   fill           <1, 0>   96     106       16 384 B                 5                   /        10
//   count, counted <0, 1>   94      98       16 384 B                 5                   /        10
//   fill, counted  <1, 1>  102     106       16 384 B                 4                   /        10
// A workgroup is four waves, one per SIMD, so "workgroups per CU" and "waves per SIMD" are the same number: the registers
// decide in every form (the 27 floats of a query against the axis-aligned walk's 12), the 16 KB of the stack never do.

// THE SHAPE is rtk_obb_shape.h's Obb, which the walk of a world (rtk_world_overlap.hip) takes too: prepare is rtk_obb_prepare(..),
// skip is rtk_obb_skip(..), candidate is rtk_obb_candidate(..). The table above is of the struct as it stands there.

extern "C" uint32_t rtk_amd_obb_stack_entries(void) { return OVERLAP_LDS_STACK; }

// d_offsets == NULL: the count form (d_counts the counts); else the fill form (d_counts the written numbers, or NULL)
int rtk_launch_obb(const rtk_dev_scene *ds, const rtk_obb_query *d_obbs, size_t num_queries, const rtk_ray_list *list,
	uint32_t *d_counts, const uint64_t *d_offsets, uint32_t *d_prims, bool fill, hipStream_t stream, rtk_trace_counters *counted)
{
	return rtk_launch_overlap_walk<Obb>(ds, d_obbs, num_queries, list, nullptr, d_counts, d_offsets, d_prims, fill, stream, counted);
}
