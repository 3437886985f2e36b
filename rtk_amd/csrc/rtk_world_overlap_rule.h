// rtk_world_overlap_rule.h -- the rule by which the three overlap queries are answered on an instanced world
// (rtk_dev_world_triangles_in_box_* / _in_obb_* / _touching_*, rtk_amd.h): which triangles of which instances touch this box,
// this oriented box, this triangle. For the host and the device: the kernel (rtk_world_overlap.hip) and
// tests/world_overlap_rule_driver.cpp include this file, and nothing but it and the rule headers it includes decides a bit of a
// result. tests/world_overlap_ref.py restates it in numpy. No HIP, no libm. DESIGN.md 3.23.2.
//
// 1. THE PLACED TRIANGLE (rtk_world_overlap_place). A record's v0 / v1 / v2, as the instance's scene holds them, are moved by
//    rtk_place_vertex under the instance's FORWARD placement (the rtk_placement the world was given, not the inverse the rays
//    use). The shape's own candidate rule then answers on the placed vertices, unchanged: rtk_box_candidate (rtk_box_rule.h),
//    rtk_obb_candidate (rtk_obb_rule.h) or rtk_touch_candidate (rtk_touch_rule.h; its shared-vertex filter compares the PLACED
//    vertices with the query's, and there is no first_prim on a world). The ingest of rtk_dev_scene_build_placed places the same
//    floats by the same rule, so these are the bits the scene call gives on the flat placed twin.
// 2. THE SKIP (rtk_world_overlap_skip). All three shapes skip a child box by rtk_box_skip against THE QUERY'S AXIS-ALIGNED BOUNDS
//    [qlo, qhi] in world coordinates: the box itself, the reach of the oriented box (rtk_obb_prepare), the query triangle's own
//    box (rtk_touch_hoist_query).
//      IN AN INSTANCE the child box [clo, chi] of the scene's tree is local: it goes through rtk_world_placed_box first, and
//    rtk_box_skip sees [wlo, whi].
//      AT THE TOP TREE AND AT A PROXY the box is taken as it is.
//    WHY NO MARGIN IS NEEDED. Every box above a triangle record contains the record's own box exactly (rtk_box_rule.h point 5),
//    so every vertex below a scene's node lies in [clo, chi]; by the monotonicity argument of rtk_world_closest_rule.h point 2
//    every such vertex is PLACED INSIDE [wlo, whi] EXACTLY -- as floats, no rounding left over. The placed triangle's own box is
//    selects of its placed vertices, so it lies in [wlo, whi], and a [wlo, whi] that is disjoint from [qlo, qhi] proves that
//    the shape's box test (rtk_box_boxes_touch against [qlo, qhi]: part of every shape's candidate rule) fails for everything
//    below the node. A proxy's box is rtk_world_box's: the placed root box, which is the min / max over the same eight placed
//    corners, grown by a pad; it contains the placed root box, hence every placed vertex of the instance. The top tree's
//    node boxes contain the proxies. ALL THREE SKIPS ARE COMPARISONS: nothing is rounded at the skip itself, so nothing needs a
//    margin. No condition number enters: any affine placement with finite placed vertices. (A NaN fails the comparisons of
//    rtk_box_skip and the child is entered.)
// 3. THE ENTRY AND THE ORDER (rtk_world_overlap_key). A candidate is named by one uint64_t key,
//        key = ((uint64_t)instance << 32) | prim,
//    prim the GLOBAL PRIMITIVE ID IN THE INSTANCE'S SCENE, as for the world's rays. The COUNT of a query is the number of its
//    candidates over all live instances the filter lets through; its LIST is its candidates in ASCENDING KEY, that is by
//    instance, then by primitive id. A segment with room for r entries keeps the first min(count, r) of the list. A torch int64
//    tensor is a segment buffer as it stands (an instance number is below 2^31).
// 4. THE INSERT (rtk_world_overlap_insert). rtk_box_insert's rule (rtk_box_rule.h point 6) on 64-bit keys: any key is dropped
//    if room is 0; into a full segment a key goes only if it is below the last entry, which is dropped; the entries above it
//    move up by one, from the back. An entry at or beyond `room` is never touched, and none at or beyond `kept` except the one
//    that is appended. The caller keeps `worst`, a copy of the segment's last entry, valid whenever kept == room != 0.
//    Because the skip is static (2.) and the insert is order-free, the kept entries are EXACTLY the first min(count, room) of
//    the full list, in any order of the walk.
// LIVENESS. A query's liveness is the shape's own (rtk_box_live, rtk_obb_prepare, rtk_touch_live): a query that is not live has
//    no candidates.
// DEAD INSTANCES. A dead instance (rtk_world_rule.h) is never answered, and neither is an instance of a scene without triangles.
// FILTER. rtk_world_filter as for closest points: the instance mask, and d_ignore_instance read AT THE QUERY'S SLOT.
// TREE INDEPENDENCE. The result is a function of the instances' records, the placements, the filter and the query alone.
//    Neither tree nor the order of the walk decides a byte.
// (All this for finite values. A placed vertex that is not finite promises nothing about results.)
#pragma once

#include "rtk_world_closest_rule.h"    // rtk_world_placed_box, rtk_place_vertex
#include "rtk_box_rule.h"
#include "rtk_obb_rule.h"
#include "rtk_touch_rule.h"

// 1. the record (a, b, c) of an instance placed by m[12]: the vertices every shape's candidate rule is given
RTK_CLOSEST_FN void rtk_world_overlap_place(const float *m, const float *a, const float *b, const float *c, float *pa, float *pb, float *pc)
{
	pa[0] = a[0]; pa[1] = a[1]; pa[2] = a[2];
	pb[0] = b[0]; pb[1] = b[1]; pb[2] = b[2];
	pc[0] = c[0]; pc[1] = c[1]; pc[2] = c[2];
	rtk_place_vertex(m, pa[0], pa[1], pa[2]);
	rtk_place_vertex(m, pb[0], pb[1], pb[2]);
	rtk_place_vertex(m, pc[0], pc[1], pc[2]);
}

// 2. (The kernel spells this function out -- rtk_world_placed_box, then its Shape's skip, which is rtk_box_skip against the same
// bounds -- because that form compiles to fewer registers; this is the rule's statement and what the host driver walks with.)
// may what lies below the child box [clo, chi] be left out for a query whose bounds are [qlo, qhi]? m: the placement of the
// instance whose scene the box belongs to, or NULL for a box of the top tree or a proxy (taken as it is)
RTK_CLOSEST_FN bool rtk_world_overlap_skip(const float *m, const float *clo, const float *chi, const float *qlo, const float *qhi)
{
	if (!m) return rtk_box_skip(clo, chi, qlo, qhi);
	float wlo[3], whi[3];
	rtk_world_placed_box(m, clo, chi, wlo, whi);
	return rtk_box_skip(wlo, whi, qlo, qhi);
}

// 3. the entry of a candidate
RTK_CLOSEST_FN uint64_t rtk_world_overlap_key(uint32_t instance, uint32_t prim) { return ((uint64_t)instance << 32) | (uint64_t)prim; }

// 4. returns the new `kept`
RTK_CLOSEST_FN uint32_t rtk_world_overlap_insert(uint64_t *seg, uint32_t room, uint32_t kept, uint64_t key, uint64_t &worst)
{
	if (room == 0u) return kept;
	uint32_t j = kept;
	if (kept >= room) {
		if (!(key < worst)) return kept;
		j = room - 1u;                                            // (the last entry is overwritten: dropped)
	}
	uint64_t last = key;                                          // what stands at room - 1 afterwards
	while (j > 0u) {
		const uint64_t e = seg[j - 1u];
		if (!(key < e)) break;
		if (j == room - 1u) last = e;
		seg[j] = e;
		j--;
	}
	seg[j] = key;
	if (kept < room) kept++;
	if (kept == room) worst = last;
	return kept;
}
