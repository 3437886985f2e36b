// rtk_box_rule.h -- the one rule by which "the triangles that touch an axis-aligned box" are counted and listed
// (rtk_dev_triangles_in_box_count / rtk_dev_triangles_in_box_all, rtk_amd.h), for the host and the device: the kernel
// (rtk_box.hip) and tests/box_rule_driver.cpp include this file, and nothing else decides a bit of a result. tests/box_ref.py
// restates it in numpy. The result is a pure function of the scene's triangle records and the query; the tree only decides how
// few of the records are looked at, and the order of the walk decides nothing.
//
// All arithmetic is float32. Every product, sum and difference below is ONE float operation, rounded on its own, in the order
// written: no fused multiply-add anywhere (rtk_closest_rule.h says how that is kept on the device and on the host; its macros
// are used here, nothing else of it is). |x| clears the sign bit. Denormal inputs and results are kept.
//
// 1. LIVE (rtk_box_live). The query (lo, hi) is live iff its six numbers are finite (x - x == 0) and lo[a] <= hi[a] on every
//    axis. lo == hi on one, two or three axes is legal: a rectangle, a segment, a point. A query that is not live has no
//    candidates, and neither has any query of a scene without triangles.
// 2. BOXES (rtk_box_boxes_touch). tlo / thi are the componentwise min / max of the three vertices, by comparison and select
//    (min(x, y) is "y < x ? y : x", max(x, y) is "y > x ? y : x"). The triangle passes iff
//        tlo[a] <= hi[a] && thi[a] >= lo[a]      on all three axes.
//    The test is CLOSED: touching counts. It is comparisons only, hence exact. A NaN coordinate fails it.
// 3. THE OTHER TEN AXES (rtk_box_separated), Akenine-Moller's test. With v0, v1, v2 the vertices as the scene holds them:
//        c = (lo + hi) * 0.5f   h = (hi - lo) * 0.5f   w_k = v_k - c          (rtk_box_centre: c and h once per query)
//        e0 = v1 - v0   e1 = v2 - v1   e2 = v0 - v2
//    For j = 0, 1, 2 with e = e_j, and k = 0, 1, 2:
//        unit_x X e:   p_k = e.y * w_k.z - e.z * w_k.y     r = h.y * |e.z| + h.z * |e.y|
//        unit_y X e:   p_k = e.z * w_k.x - e.x * w_k.z     r = h.x * |e.z| + h.z * |e.x|
//        unit_z X e:   p_k = e.x * w_k.y - e.y * w_k.x     r = h.x * |e.y| + h.y * |e.x|
//    (two products and one difference per projection; two products and one sum per radius). The axis separates iff
//    min(p) > r || max(p) < -r, evaluated as (p_0 > r && p_1 > r && p_2 > r) || (p_0 < -r && p_1 < -r && p_2 < -r).
//    For the plane:
//        n = e0 X e1:  n.x = e0.y * e1.z - e0.z * e1.y   n.y = e0.z * e1.x - e0.x * e1.z   n.z = e0.x * e1.y - e0.y * e1.x
//        d = (n.x * w_0.x + n.y * w_0.y) + n.z * w_0.z       r = (h.x * |n.x| + h.y * |n.y|) + h.z * |n.z|
//    The plane separates iff d > r || d < -r.
//    A COMPARISON WITH A NaN NEVER SEPARATES: a NaN among p, r or d (an overflowing hi - lo, an infinity times a zero) fails
//    the comparison it stands in, and that axis keeps the triangle.
// 4. CANDIDATE (rtk_box_candidate). A triangle record is a candidate of a live query iff 2. holds and none of the ten axes of 3.
//    separates. The COUNT of a query is the number of its candidates. The LIST of a query is its candidates in ASCENDING
//    PRIMITIVE ID; a segment with room for r entries keeps the first min(count, r) of the list.
// 5. SKIP (rtk_box_skip). A child box [clo, chi] is left out iff clo[a] > hi[a] || chi[a] < lo[a] on some axis. A NaN fails
//    both comparisons and the child is entered. Empty slots are told by the child word, not by their box. The skip is EXACT
//    WITHOUT A MARGIN: every box above a triangle contains the triangle's own box, tlo and thi are selects
//    of the stored coordinates, so clo[a] <= tlo[a] and thi[a] <= chi[a] hold exactly, and a node box that is disjoint from
//    the query proves that 2. fails for everything below it. Only the exact 128-byte nodes are used. Unlike the walk of
//    "Triangles within a distance" this walk cannot be culled by what it has kept: the tree is not ordered by id.
// 6. INSERT (rtk_box_insert). The bounded sorted insertion of one id into a segment of `room` entries of which the first
//    `kept` are in use and ascending: any id is dropped if room is 0; into a full segment (kept == room) an id goes only if it
//    is below the last entry, which is dropped; the entries above it move up by one, from the back, and it takes the place
//    they leave. An entry at or beyond `room` is never touched, and none at or beyond `kept` except the one that is appended.
//    Equal ids keep their order of arrival (no scene has two records of one id). The caller keeps `worst`, a copy of the
//    segment's last entry, valid whenever kept == room != 0: insert decides by it without reading the segment and brings it
//    up to date, so a candidate that does not get in costs no memory access.
// Because of 5. and 6. the kept entries are EXACTLY the first min(count, room) of the full list, in any order of the walk.
//
// WHAT THE RULE IS AND IS NOT.
//  * It is a FLOAT RULE, and the candidate set is DEFINED BY IT: where the rounded p, r and d of 3. put a triangle that passes
//    within half an ulp or so of a box's edge or corner on the other side of the comparison than real arithmetic would, the rule
//    wins. On inputs whose every intermediate is exact (small integers, say) the rule is the exact separating-axis answer, and
//    touching counts.
//  * A ZERO-AREA TRIANGLE has n = 0, so the plane separates nothing (d = r = 0). If its three vertices coincide every e is 0 and
//    step 3 separates nothing at all: a point triangle is a candidate whenever its box touches the query, which is the exact
//    answer. If it is a segment (collinear vertices) the nine edge axes are the segment's own separating axes and still decide,
//    exactly so in exact arithmetic; in floats a sliver's n, p and r can all round towards 0, and then it is kept whenever
//    its box touches the query.
//  * A box WITHOUT VOLUME has r = 0 on the axes its zero extents take part in, and there the comparison is with the rounding
//    error of p or d alone. A point box at a triangle's vertex 0 is always a candidate of that triangle (w_0 = 0, so every p_0
//    and d are 0); at vertex 1 or 2, on an edge or inside the face d is a rounded n . w_0 that is rarely exactly 0, and the
//    triangle is then not a candidate. Give such a query the extent the data's accuracy calls for.
//  * A scene with NON-FINITE vertex coordinates: the calls terminate and write only inside their outputs.
//    NOTHING ELSE IS PROMISED about their results.
#pragma once

#include "rtk_closest_rule.h"      // RTK_CLOSEST_FN, RTK_CL_MUL / _ADD / _SUB, RTK_CL_MIN / _MAX: the macros only

#define RTK_BOX_ABS(x) __builtin_fabsf(x)      // (the sign bit cleared, on the host and on the device)

// 1. can the query have candidates at all? (x - x is 0 for a finite x and a NaN for an infinity or a NaN)
RTK_CLOSEST_FN bool rtk_box_live(const float *lo, const float *hi)
{
	bool live = true;
	for (int a = 0; a < 3; a++) live = live && lo[a] - lo[a] == 0.0f && hi[a] - hi[a] == 0.0f && lo[a] <= hi[a];
	return live;
}

// 3. the query's centre and half extent, once per query
RTK_CLOSEST_FN void rtk_box_centre(const float *lo, const float *hi, float *c, float *h)
{
	for (int a = 0; a < 3; a++) {
		c[a] = RTK_CL_MUL(RTK_CL_ADD(lo[a], hi[a]), 0.5f);
		h[a] = RTK_CL_MUL(RTK_CL_SUB(hi[a], lo[a]), 0.5f);
	}
}

// 2. does the triangle's own box touch the query?
RTK_CLOSEST_FN bool rtk_box_boxes_touch(const float *v0, const float *v1, const float *v2, const float *lo, const float *hi)
{
	bool touch = true;
	for (int a = 0; a < 3; a++) {
		const float m0 = RTK_CL_MIN(v0[a], v1[a]), tlo = RTK_CL_MIN(m0, v2[a]);
		const float m1 = RTK_CL_MAX(v0[a], v1[a]), thi = RTK_CL_MAX(m1, v2[a]);
		touch = touch && tlo <= hi[a] && thi >= lo[a];
	}
	return touch;
}

// 3. one of the nine axes: the projections are ea * w_k[ib] - eb * w_k[ia], the radius ha * |eb| + hb * |ea|
RTK_CLOSEST_FN bool rtk_box_axis_separates(float ea, float eb, float wa0, float wb0, float wa1, float wb1, float wa2, float wb2, float ha, float hb)
{
	const float p0 = RTK_CL_SUB(RTK_CL_MUL(ea, wb0), RTK_CL_MUL(eb, wa0));
	const float p1 = RTK_CL_SUB(RTK_CL_MUL(ea, wb1), RTK_CL_MUL(eb, wa1));
	const float p2 = RTK_CL_SUB(RTK_CL_MUL(ea, wb2), RTK_CL_MUL(eb, wa2));
	const float r = RTK_CL_ADD(RTK_CL_MUL(ha, RTK_BOX_ABS(eb)), RTK_CL_MUL(hb, RTK_BOX_ABS(ea)));
	const float nr = -r;
	return (p0 > r && p1 > r && p2 > r) || (p0 < nr && p1 < nr && p2 < nr);
}

// 3. does one of the ten axes separate the triangle from the box (c, h)?
RTK_CLOSEST_FN bool rtk_box_separated(const float *v0, const float *v1, const float *v2, const float *c, const float *h)
{
	float w0[3], w1[3], w2[3], e[3][3];
	for (int a = 0; a < 3; a++) {
		w0[a] = RTK_CL_SUB(v0[a], c[a]); w1[a] = RTK_CL_SUB(v1[a], c[a]); w2[a] = RTK_CL_SUB(v2[a], c[a]);
		e[0][a] = RTK_CL_SUB(v1[a], v0[a]); e[1][a] = RTK_CL_SUB(v2[a], v1[a]); e[2][a] = RTK_CL_SUB(v0[a], v2[a]);
	}
	bool sep = false;
	for (int j = 0; j < 3; j++) {
		const float ex = e[j][0], ey = e[j][1], ez = e[j][2];
		// unit_x X e: p = e.y * w.z - e.z * w.y, r = h.y * |e.z| + h.z * |e.y|
		sep = sep || rtk_box_axis_separates(ey, ez, w0[1], w0[2], w1[1], w1[2], w2[1], w2[2], h[1], h[2]);
		// unit_y X e: p = e.z * w.x - e.x * w.z, r = h.x * |e.z| + h.z * |e.x|
		sep = sep || rtk_box_axis_separates(ez, ex, w0[2], w0[0], w1[2], w1[0], w2[2], w2[0], h[2], h[0]);
		// unit_z X e: p = e.x * w.y - e.y * w.x, r = h.x * |e.y| + h.y * |e.x|
		sep = sep || rtk_box_axis_separates(ex, ey, w0[0], w0[1], w1[0], w1[1], w2[0], w2[1], h[0], h[1]);
	}
	const float nx = RTK_CL_SUB(RTK_CL_MUL(e[0][1], e[1][2]), RTK_CL_MUL(e[0][2], e[1][1]));
	const float ny = RTK_CL_SUB(RTK_CL_MUL(e[0][2], e[1][0]), RTK_CL_MUL(e[0][0], e[1][2]));
	const float nz = RTK_CL_SUB(RTK_CL_MUL(e[0][0], e[1][1]), RTK_CL_MUL(e[0][1], e[1][0]));
	const float d = RTK_CL_ADD(RTK_CL_ADD(RTK_CL_MUL(nx, w0[0]), RTK_CL_MUL(ny, w0[1])), RTK_CL_MUL(nz, w0[2]));
	const float r = RTK_CL_ADD(RTK_CL_ADD(RTK_CL_MUL(h[0], RTK_BOX_ABS(nx)), RTK_CL_MUL(h[1], RTK_BOX_ABS(ny))), RTK_CL_MUL(h[2], RTK_BOX_ABS(nz)));
	return sep || d > r || d < -r;
}

// 4. (c, h) from rtk_box_centre(lo, hi)
RTK_CLOSEST_FN bool rtk_box_candidate(const float *v0, const float *v1, const float *v2, const float *lo, const float *hi, const float *c, const float *h)
{
	return rtk_box_boxes_touch(v0, v1, v2, lo, hi) && !rtk_box_separated(v0, v1, v2, c, h);
}

// 5. may what lies below the child box [clo, chi] be left out?
RTK_CLOSEST_FN bool rtk_box_skip(const float *clo, const float *chi, const float *lo, const float *hi)
{
	return clo[0] > hi[0] || chi[0] < lo[0] || clo[1] > hi[1] || chi[1] < lo[1] || clo[2] > hi[2] || chi[2] < lo[2];
}

// 6. returns the new `kept`
RTK_CLOSEST_FN uint32_t rtk_box_insert(uint32_t *seg, uint32_t room, uint32_t kept, uint32_t prim, uint32_t &worst)
{
	if (room == 0u) return kept;
	uint32_t j = kept;
	if (kept >= room) {
		if (!(prim < worst)) return kept;
		j = room - 1u;                                            // (the last entry is overwritten: dropped)
	}
	uint32_t last = prim;                                         // what stands at room - 1 afterwards
	while (j > 0u) {
		const uint32_t e = seg[j - 1u];
		if (!(prim < e)) break;
		if (j == room - 1u) last = e;
		seg[j] = e;
		j--;
	}
	seg[j] = prim;
	if (kept < room) kept++;
	if (kept == room) worst = last;
	return kept;
}
