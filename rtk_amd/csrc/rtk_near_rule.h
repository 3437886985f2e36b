// rtk_near_rule.h -- the one rule by which "the triangles within a distance of a triangle" are counted and listed
// (rtk_dev_triangles_near_count / rtk_dev_triangles_near_all, rtk_amd.h), for the host and the device: the kernel
// (rtk_near.hip) and tests/near_rule_driver.cpp include this file, and nothing else decides a bit of a result. Everything about a
// query triangle and ONE record or ONE box is rtk_pair_rule.h's, unchanged (its rules 1 to 4 and 6: live, the fifteen features,
// piercing, the filter, the box bound); this file says what a SET of records per query is, as rtk_within_rule.h does for a point.
// The result is a pure function of the scene's triangle records and the query; the tree only decides how few of the records are
// looked at, and the order of the walk decides nothing.
//
// 7. CANDIDATE (rtk_near_candidate). A record is a candidate of the query (A, max_dist2) iff the query is live (rtk_touch_live),
//    max_dist2 > 0 (a NaN, a zero of either sign and a negative limit are not), the filter passes (rtk_touch_filter_passes, as it
//    is) and dist2 < max_dist2, dist2 from rtk_pair_evaluate: strictly, as in closest triangles. A NaN dist2 fails the comparison
//    and is never a candidate. A pierced pair has dist2 = 0 and is a candidate of every live query with a limit above 0. The
//    COUNT of a query is the number of its candidates; a scene without triangles gives every query the count 0.
// 8. ORDER. The LIST of a query is its candidates ascending in (dist2, prim) by rtk_closest_better: the smaller dist2 first, THE
//    LOWEST PRIMITIVE ID FIRST AMONG EQUAL dist2 -- pierced pairs, all at dist2 = 0, come first, by id. An entry is the record
//    {dist2, u, v, prim} and the two points qa, qb of rtk_pair_evaluate. A segment with room for r entries keeps the first
//    min(count, r) of the list. The first entry of a list is therefore, word for word, the record and the two points
//    rtk_dev_closest_triangles writes for the query (rule 5 of rtk_pair_rule.h picks the same minimum).
// 9. SKIP (rtk_near_skip). What lies behind the bound b -- a subtree behind the bound of its box, a record behind the bound of
//    ITS OWN box, both by rtk_pair_box_bound against A's box -- may be left out iff
//        b >= max_dist2,   or   the segment is full and b > worst.dist2    (worst: the last kept entry of a full segment)
//    Both are EXACT, because rule 6 of rtk_pair_rule.h gives bound <= dist2 for every record below the box WITHOUT A MARGIN (qa
//    lies in A's box, qb in the record's own box, which lies inside every box above it; a pierced pair's boxes touch, so its
//    bounds are 0): with b >= max_dist2 every dist2 below the box is >= max_dist2 and no record there is a candidate; with
//    b > worst.dist2 every dist2 below the box is > worst.dist2 and no record there beats the worst kept entry, now or later
//    (the worst entry of a full segment only ever gets better: an insertion into a full segment drops it for an entry that
//    beats it). The second comparison is STRICT: behind an equal bound a record at exactly worst.dist2 with a lower id can
//    hide, and it belongs in front of worst. A NaN bound fails both comparisons and is not skipped. A count keeps nothing and
//    is never full: only the first comparison holds for it, and its bound is static.
// 10. INSERT (rtk_near_insert). rtk_within_insert's bounded sorted insertion with TWO optional point arrays that move with
//    the records: into a segment of `room` entries of which the first `kept` are in use and sorted by 8., a candidate with a NaN
//    dist2, and any candidate if room is 0, is dropped; into a full segment (kept == room) a candidate goes only if it beats the
//    last entry (rtk_closest_better), which is dropped; the entries it beats move up by one, from the back, and it takes the
//    place they leave. An entry at or beyond `room` is never touched, and none at or beyond `kept` except the one that is
//    appended. Equal (dist2, prim) pairs keep their order of arrival (no scene has two records of one id). The caller keeps
//    `worst`, a copy of the segment's last entry, valid whenever kept == room != 0: insert decides by it without reading the
//    segment -- a candidate that does not get in costs no memory access -- and brings it up to date, and 9. reads its dist2.
// Because of 9. and 10. the kept entries are EXACTLY the first min(count, room) of the full list, in any order of the walk.
#pragma once

#include "rtk_pair_rule.h"

// 7. is a record at dist2 that the filter let through a candidate of a live query? (the caller has looked at max_dist2 > 0)
RTK_CLOSEST_FN bool rtk_near_candidate(float dist2, float max_dist2) { return dist2 < max_dist2; }

// 9. may what lies behind `bound` be left out? full: the segment holds `room` entries, worst2 is the dist2 of the last of them
RTK_CLOSEST_FN bool rtk_near_skip(float bound, float max_dist2, bool full, float worst2)
{
	return bound >= max_dist2 || (full && bound > worst2);
}

// 10. REC is rtk_closest_record (float dist2, u, v; uint32_t prim). seg_qa, seg_qb: NULL, or three floats per entry of the
// segment; qa, qb the candidate's two points. Returns the new `kept`.
template <typename REC>
RTK_CLOSEST_FN uint32_t rtk_near_insert(REC *seg, float *seg_qa, float *seg_qb, uint32_t room, uint32_t kept, const REC &cand,
	const float *qa, const float *qb, REC &worst)
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
		if (seg_qa) { float *d = seg_qa + (uint64_t)j * 3u; d[0] = d[-3]; d[1] = d[-2]; d[2] = d[-1]; }
		if (seg_qb) { float *d = seg_qb + (uint64_t)j * 3u; d[0] = d[-3]; d[1] = d[-2]; d[2] = d[-1]; }
		j--;
	}
	seg[j] = cand;
	if (seg_qa) { float *d = seg_qa + (uint64_t)j * 3u; d[0] = qa[0]; d[1] = qa[1]; d[2] = qa[2]; }
	if (seg_qb) { float *d = seg_qb + (uint64_t)j * 3u; d[0] = qb[0]; d[1] = qb[1]; d[2] = qb[2]; }
	if (kept < room) kept++;
	if (kept == room) worst = last;
	return kept;
}
