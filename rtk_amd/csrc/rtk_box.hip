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
#include "rtk_box_shape.h"

// BX_RESOURCES: the compiler's report (gfx950, -O3, -Rpass-analysis=kernel-resource-usage) for each instantiated form
// <FILL, COUNT>; scratch 0, no SGPR or VGPR spills and no AGPRs in every one of them:
//                          VGPRs  SGPRs  LDS per workgroup   waves per SIMD by registers / workgroups per CU by LDS
//   count          <0, 0>   76      88       16 384 B                 6                   /        10
//   fill           <1, 0>   80      96       16 384 B                 6                   /        10
//   count, counted <0, 1>   84      86       16 384 B                 5                   /        10
//   fill, counted  <1, 1>   86     100       16 384 B                 5                   /        10
// A workgroup is four waves, one per SIMD, so "workgroups per CU" and "waves per SIMD" are the same number: the registers
// (512 / 80 = 6) decide in every form, the 16 KB of the stack never do.

// THE SHAPE is rtk_box_shape.h's Box, which the walk of a world (rtk_world_overlap.hip) takes too: prepare is rtk_box_centre(..)
// and rtk_box_live(..), skip is rtk_box_skip(..), candidate is rtk_box_candidate(..) spelled out as rtk_box_boxes_touch(..) &&
// !rtk_box_separated(..) (that header says why). The table above is of the struct as it stands there.

extern "C" uint32_t rtk_amd_box_stack_entries(void) { return OVERLAP_LDS_STACK; }

// d_offsets == NULL: the count form (d_counts the counts); else the fill form (d_counts the written numbers, or NULL)
int rtk_launch_box(const rtk_dev_scene *ds, const rtk_box_query *d_boxes, size_t num_queries, const rtk_ray_list *list,
	uint32_t *d_counts, const uint64_t *d_offsets, uint32_t *d_prims, bool fill, hipStream_t stream, rtk_trace_counters *counted)
{
	return rtk_launch_overlap_walk<Box>(ds, d_boxes, num_queries, list, nullptr, d_counts, d_offsets, d_prims, fill, stream, counted);
}
