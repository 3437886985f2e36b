// rtk_within_rule.h -- the one rule by which "the triangles within a distance of a point" are counted and listed
// (rtk_dev_triangles_within_count / rtk_dev_triangles_within_all, rtk_amd.h), for the host and the device: the kernel
// (rtk_within.hip) and tests/within_rule_driver.cpp include this file and rtk_closest_rule.h, and nothing else decides a bit of a
// result. Everything about a point and ONE triangle or ONE box is rtk_closest_rule.h's, unchanged (its rules 1, 2 and 3); this
// file says what a SET of triangles per query is. The result is a pure function of the scene's triangle records and the query;
// the tree only decides how few of the records are looked at, and the order of the walk decides nothing.
//
// 4. CANDIDATE (rtk_within_live, rtk_within_candidate). A triangle record is a candidate of the query (p, max_dist2) iff
//    dist2 < max_dist2, dist2 from rtk_closest_triangle: strictly, as in closest points. A NaN dist2 fails the comparison and is
//    never a candidate. A query is LIVE iff max_dist2 > 0 (a NaN, a zero of either sign and a negative limit are not) and its
//    three coordinates are finite; a query that is not live has no candidates, and neither has any query of a scene without
//    triangles. The COUNT of a query is the number of its candidates.
// 5. ORDER. The LIST of a query is its candidates ascending in (dist2, prim) by rtk_closest_better: the smaller dist2 first, THE
//    LOWEST PRIMITIVE ID FIRST AMONG EQUAL dist2. A segment with room for r entries keeps the first min(count, r) of the list.
//    The first entry of a list is therefore, word for word, the record and the point rtk_dev_closest_points writes for the query.
// 6. SKIP (rtk_within_skip). A subtree whose box has the bound b (rtk_closest_box_bound) may be left out iff
//        b >= max_dist2,   or   the segment is full and b > worst.dist2    (worst: the last kept entry of a full segment)
//    Both are EXACT, because rule 2 gives bound <= dist2 for every triangle below the box WITHOUT A MARGIN: with b >= max_dist2
//    every dist2 below the box is >= max_dist2 and no triangle there is a candidate; with b > worst.dist2 every dist2 below
//    the box is > worst.dist2 and no triangle there beats the worst kept entry, now or later (the worst entry of a full
//    segment only ever gets better). The second comparison is STRICT: behind an equal bound a triangle at exactly worst.dist2
//    with a lower id can hide, and it belongs in front of worst. A NaN bound fails both comparisons and is not skipped.
//    Unlike the walk of "Every hit along a ray", whose bound must not shrink, this walk may cull with what it has kept.
// 7. INSERT (rtk_within_insert). The bounded sorted insertion of one candidate into a segment of `room` entries of which the
//    first `kept` are in use and sorted by 5.: a candidate with a NaN dist2, and any candidate if room is 0, is dropped; into a
//    full segment (kept == room) a candidate goes only if it beats the last entry (rtk_closest_better), which is dropped; the
//    entries it beats move up by one, from the back, and it takes the place they leave. An entry at or beyond `room` is never
//    touched, and none at or beyond `kept` except the one that is appended. Equal (dist2, prim) pairs keep their order of
//    arrival (no scene has two records of one id). The caller keeps `worst`, a copy of the segment's last entry, valid whenever
//    kept == room != 0: insert decides by it without reading the segment and brings it up to date, and 6. reads its dist2.
// Because of 6. and 7. the kept entries are EXACTLY the first min(count, room) of the full list, in any order of the walk.
#pragma once

#include "rtk_closest_rule.h"

// 4. can the query have candidates at all? ... and is a triangle at dist2 one?
RTK_CLOSEST_FN bool rtk_within_live(const float *p, float max_dist2)
{
	// (x - x is 0 for a finite x and a NaN for an infinity or a NaN)
	return max_dist2 > 0.0f && p[0] - p[0] == 0.0f && p[1] - p[1] == 0.0f && p[2] - p[2] == 0.0f;
}
RTK_CLOSEST_FN bool rtk_within_candidate(float dist2, float max_dist2) { return dist2 < max_dist2; }

// 6. may what lies behind `bound` be left out? full: the segment holds `room` entries, worst2 is the dist2 of the last of them
RTK_CLOSEST_FN bool rtk_within_skip(float bound, float max_dist2, bool full, float worst2)
{
	return bound >= max_dist2 || (full && bound > worst2);
}

// 7. REC is rtk_closest_record (float dist2, u, v; uint32_t prim). seg_points: NULL, or three floats per entry of the segment,
// q the candidate's point. Returns the new `kept`.
template <typename REC>
RTK_CLOSEST_FN uint32_t rtk_within_insert(REC *seg, float *seg_points, uint32_t room, uint32_t kept, const REC &cand, const float *q, REC &worst)
{
	if (room == 0u || !(cand.dist2 == cand.dist2)) return kept;
	uint32_t j = kept;
	if (kept >= room) {
		if (!rtk_closest_better(cand.dist2, cand.prim, worst.dist2, worst.prim)) return kept;
		j = room - 1u;                                            // (the last entry is overwritten: dropped)
	}
	REC last = cand;                                              // what stands at room - 1 afterwards
	while (j > 0u) {
		const REC e = seg[j - 1u];
		if (!rtk_closest_better(cand.dist2, cand.prim, e.dist2, e.prim)) break;
		if (j == room - 1u) last = e;
		seg[j] = e;
		if (seg_points) { float *d = seg_points + (uint64_t)j * 3u; d[0] = d[-3]; d[1] = d[-2]; d[2] = d[-1]; }
		j--;
	}
	seg[j] = cand;
	if (seg_points) { float *d = seg_points + (uint64_t)j * 3u; d[0] = q[0]; d[1] = q[1]; d[2] = q[2]; }
	if (kept < room) kept++;
	if (kept == room) worst = last;
	return kept;
}
