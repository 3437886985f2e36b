// rtk_touch_rule.h -- the one rule by which "the triangles that touch a triangle" are counted and listed
// (rtk_dev_triangles_touching_count / rtk_dev_triangles_touching_all, rtk_amd.h), for the host and the device: the kernel
// (rtk_touch.hip) and tests/touch_rule_driver.cpp include this file, and nothing else decides a bit of a result.
// tests/touch_ref.py restates it in numpy. The result is a pure function of the scene's triangle records and the query; the
// tree only decides how few of the records are looked at, and the order of the walk decides nothing.
//
// All arithmetic is float32. Every product, sum and difference below is ONE float operation, rounded on its own, in the order
// written: no fused multiply-add anywhere (rtk_closest_rule.h says how that is kept on the device and on the host; its macros
// are used here, nothing else of it is). Denormal inputs and results are kept. min(x, y) is "y < x ? y : x", max(x, y) is
// "y > x ? y : x", as in rtk_box_rule.h. The query triangle is A = (a0, a1, a2); a scene record is B = (b0, b1, b2), its
// vertices as the scene holds them.
//
// 1. LIVE (rtk_touch_live). The query is live iff its nine numbers are finite (x - x == 0). A query that is not live has no
//    candidates, and neither has any query of a scene without triangles. A query without area (a segment, a point) is live.
// 2. BOXES (rtk_touch_boxes_touch). alo / ahi are the componentwise min / max of A's vertices (rtk_touch_hoist, once per
//    query), tlo / thi the same of B's. The pair passes iff
//        tlo[x] <= ahi[x] && thi[x] >= alo[x]      on all three axes.
//    The test is CLOSED: touching counts. It is comparisons only, hence exact. A NaN coordinate fails it.
// 3. SEVENTEEN AXES, one function for all of them (rtk_touch_axis_separates). The edges of either triangle are the box rule's:
//        e0 = v1 - v0   e1 = v2 - v1   e2 = v0 - v2
//    and the cross product has the box rule's component formulas, two products and one difference each:
//        (x X y).x = x.y * y.z - x.z * y.y   (x X y).y = x.z * y.x - x.x * y.z   (x X y).z = x.x * y.y - x.y * y.x
//    The axes, in this order:
//        nA = ea0 X ea1;   nB = eb0 X eb1;   the nine ea_i X eb_j, i outer and j inner;   nA X ea_0..2;   nB X eb_0..2
//    The projections of an axis m, all about a0, with dot(m, d) = (m.x * d.x + m.y * d.y) + m.z * d.z:
//        pA_0 = 0.0f   pA_1 = dot(m, a1 - a0)   pA_2 = dot(m, a2 - a0)   pB_k = dot(m, b_k - a0)
//    The five difference vectors are formed once per pair (A's two once per query). The axis separates iff
//        every pB_k > every pA_j   or   every pB_k < every pA_j
//    nine comparisons on each side joined with &&. A COMPARISON WITH A NaN NEVER SEPARATES: it is false, and that axis keeps
//    the pair. The six in-plane axes are always evaluated: there is no float decision "are they coplanar" anywhere.
// 4. CANDIDATE (rtk_touch_candidate). A record is a candidate of a live query iff 2. holds, none of the seventeen axes of 3.
//    separates, and the filter of 5. lets it through. The COUNT of a query is the number of its candidates. The LIST of a
//    query is its candidates in ASCENDING PRIMITIVE ID; a segment with room for r entries keeps the first min(count, r).
// 5. FILTER (rtk_touch_filter_passes), part of the rule, applied to the record's global primitive id and stored positions:
//      first_prim (d_first_prim[i], when given, else 0): a candidate of query i has prim >= first_prim.
//      RTK_TOUCH_SKIP_SHARED_VERTEX: a record is not a candidate if one of its vertices equals one of the query's on all three
//      coordinates by float == (so +0 equals -0 and a NaN equals nothing). Neighbours in a mesh share positions bit for bit,
//      and a triangle shares them with itself: the flag plus first_prim = own id + 1 gives each self-intersecting pair once.
// 6. SKIP. rtk_box_skip of rtk_box_rule.h with (alo, ahi) as the query: a child box is left out iff it is disjoint from A's
//    box by comparison. It is EXACT WITHOUT A MARGIN for the reason stated there: every box above a record contains the
//    record's own box, so a disjoint node box proves that 2. fails for everything below it. Only the exact 128-byte nodes are
//    used; empty slots are told by the child word. The walk is not culled by A's plane: that would have to be proven exact
//    against 3. first.
// 7. INSERT. rtk_box_insert of rtk_box_rule.h, as it is.
// Because of 6. and 7. the kept entries are EXACTLY the first min(count, room) of the full list, in any order of the walk.
//
// WHAT THE RULE IS AND IS NOT.
//  * It is a FLOAT RULE, and the candidate set is DEFINED BY IT: where the rounded projections of 3. put a pair within an ulp
//    or so of a contact on the other side of a comparison than real arithmetic would, the rule wins. Touching counts: the
//    comparisons of 3. are strict, so equal projections do not separate.
//  * Any separating axis is a proof of disjointness in exact arithmetic, so ON EXACT INPUTS (every intermediate exact: small
//    integers, say) the rule NEVER LOSES A PAIR THAT MEETS.
//  * For two triangles of NON-ZERO AREA on exact inputs it is THE EXACT ANSWER: the first eleven axes decide two triangles
//    whose planes are not parallel, nA decides parallel planes, and the six in-plane axes decide a common plane (there they
//    are the two triangles' edge normals, the separating axes of two convex polygons).
//  * If A or B has ZERO AREA some axes vanish and the rule may keep a pair that does not meet: a segment that lies in B's
//    plane and passes beside B has no in-plane normal of its own (nA = 0), and B's edge normals alone need not separate the
//    two. It never drops a pair that does meet.
//  * A scene with NON-FINITE vertex coordinates: the calls terminate and write only inside their outputs.
//    NOTHING ELSE IS PROMISED about their results.
#pragma once

#include "rtk_box_rule.h"          // rtk_box_skip, rtk_box_insert; through it the macros of rtk_closest_rule.h

#define RTK_TOUCH_RULE_SKIP_SHARED_VERTEX 1u      // (RTK_TOUCH_SKIP_SHARED_VERTEX of rtk_amd.h, which this header does not need)

// what is formed once per query: A's vertex 0, box, two differences, edges, normal and the three nA X ea_i
struct rtk_touch_hoist {
	float a0[3], lo[3], hi[3];
	float d1[3], d2[3];            // a1 - a0, a2 - a0
	float e[3][3];                 // ea0, ea1, ea2
	float n[3];                    // nA
	float ne[3][3];                // nA X ea_i
};

RTK_CLOSEST_FN void rtk_touch_cross(const float *x, const float *y, float *c)
{
	c[0] = RTK_CL_SUB(RTK_CL_MUL(x[1], y[2]), RTK_CL_MUL(x[2], y[1]));
	c[1] = RTK_CL_SUB(RTK_CL_MUL(x[2], y[0]), RTK_CL_MUL(x[0], y[2]));
	c[2] = RTK_CL_SUB(RTK_CL_MUL(x[0], y[1]), RTK_CL_MUL(x[1], y[0]));
}

// 3. the edges of a triangle
RTK_CLOSEST_FN void rtk_touch_edges(const float *v0, const float *v1, const float *v2, float e[3][3])
{
	for (int a = 0; a < 3; a++) { e[0][a] = RTK_CL_SUB(v1[a], v0[a]); e[1][a] = RTK_CL_SUB(v2[a], v1[a]); e[2][a] = RTK_CL_SUB(v0[a], v2[a]); }
}

// 1. can the query have candidates at all? (x - x is 0 for a finite x and a NaN for an infinity or a NaN)
RTK_CLOSEST_FN bool rtk_touch_live(const float *a0, const float *a1, const float *a2)
{
	bool live = true;
	for (int a = 0; a < 3; a++) live = live && a0[a] - a0[a] == 0.0f && a1[a] - a1[a] == 0.0f && a2[a] - a2[a] == 0.0f;
	return live;
}

// 2. and 3., the query's part
RTK_CLOSEST_FN void rtk_touch_hoist_query(const float *a0, const float *a1, const float *a2, rtk_touch_hoist &q)
{
	for (int a = 0; a < 3; a++) {
		const float m0 = RTK_CL_MIN(a0[a], a1[a]), m1 = RTK_CL_MAX(a0[a], a1[a]);
		q.a0[a] = a0[a];
		q.lo[a] = RTK_CL_MIN(m0, a2[a]);
		q.hi[a] = RTK_CL_MAX(m1, a2[a]);
		q.d1[a] = RTK_CL_SUB(a1[a], a0[a]);
		q.d2[a] = RTK_CL_SUB(a2[a], a0[a]);
	}
	rtk_touch_edges(a0, a1, a2, q.e);
	rtk_touch_cross(q.e[0], q.e[1], q.n);
	for (int i = 0; i < 3; i++) rtk_touch_cross(q.n, q.e[i], q.ne[i]);
}

// 2. does the record's own box touch the query's?
RTK_CLOSEST_FN bool rtk_touch_boxes_touch(const float *b0, const float *b1, const float *b2, const float *alo, const float *ahi)
{
	return rtk_box_boxes_touch(b0, b1, b2, alo, ahi);
}

// 3. one axis: m against A's differences (d1, d2) and B's (w0, w1, w2), all about a0
RTK_CLOSEST_FN bool rtk_touch_axis_separates(const float *m, const float *d1, const float *d2, const float *w0, const float *w1, const float *w2)
{
	const float pa0 = 0.0f;
	const float pa1 = RTK_CL_DOT(m[0], m[1], m[2], d1[0], d1[1], d1[2]);
	const float pa2 = RTK_CL_DOT(m[0], m[1], m[2], d2[0], d2[1], d2[2]);
	const float pb0 = RTK_CL_DOT(m[0], m[1], m[2], w0[0], w0[1], w0[2]);
	const float pb1 = RTK_CL_DOT(m[0], m[1], m[2], w1[0], w1[1], w1[2]);
	const float pb2 = RTK_CL_DOT(m[0], m[1], m[2], w2[0], w2[1], w2[2]);
	const bool above = pb0 > pa0 && pb0 > pa1 && pb0 > pa2 && pb1 > pa0 && pb1 > pa1 && pb1 > pa2 && pb2 > pa0 && pb2 > pa1 && pb2 > pa2;
	const bool below = pb0 < pa0 && pb0 < pa1 && pb0 < pa2 && pb1 < pa0 && pb1 < pa1 && pb1 < pa2 && pb2 < pa0 && pb2 < pa1 && pb2 < pa2;
	return above || below;
}

// 3. which of the seventeen axes separate the record from the query: bit k is axis k in the order of the rule
RTK_CLOSEST_FN uint32_t rtk_touch_separating_axes(const rtk_touch_hoist &q, const float *b0, const float *b1, const float *b2)
{
	float w0[3], w1[3], w2[3], eb[3][3], nb[3], m[3];
	for (int a = 0; a < 3; a++) { w0[a] = RTK_CL_SUB(b0[a], q.a0[a]); w1[a] = RTK_CL_SUB(b1[a], q.a0[a]); w2[a] = RTK_CL_SUB(b2[a], q.a0[a]); }
	rtk_touch_edges(b0, b1, b2, eb);
	rtk_touch_cross(eb[0], eb[1], nb);
	uint32_t sep = 0u, bit = 1u;
	sep |= rtk_touch_axis_separates(q.n, q.d1, q.d2, w0, w1, w2) ? bit : 0u; bit <<= 1;
	sep |= rtk_touch_axis_separates(nb, q.d1, q.d2, w0, w1, w2) ? bit : 0u; bit <<= 1;
	for (int i = 0; i < 3; i++) {
		for (int j = 0; j < 3; j++) {
			rtk_touch_cross(q.e[i], eb[j], m);
			sep |= rtk_touch_axis_separates(m, q.d1, q.d2, w0, w1, w2) ? bit : 0u; bit <<= 1;
		}
	}
	for (int i = 0; i < 3; i++) { sep |= rtk_touch_axis_separates(q.ne[i], q.d1, q.d2, w0, w1, w2) ? bit : 0u; bit <<= 1; }
	for (int j = 0; j < 3; j++) {
		rtk_touch_cross(nb, eb[j], m);
		sep |= rtk_touch_axis_separates(m, q.d1, q.d2, w0, w1, w2) ? bit : 0u; bit <<= 1;
	}
	return sep;
}

// 3. does one of the seventeen axes separate? (rtk_touch_separating_axes(...) != 0, leaving at the first group of axes that
// says so: the two normals, which decide most pairs whose boxes touch; the nine edge pairs, a row at a time; the six in-plane axes)
RTK_CLOSEST_FN bool rtk_touch_separated(const rtk_touch_hoist &q, const float *b0, const float *b1, const float *b2)
{
	float w0[3], w1[3], w2[3], eb[3][3], nb[3], m[3];
	for (int a = 0; a < 3; a++) { w0[a] = RTK_CL_SUB(b0[a], q.a0[a]); w1[a] = RTK_CL_SUB(b1[a], q.a0[a]); w2[a] = RTK_CL_SUB(b2[a], q.a0[a]); }
	rtk_touch_edges(b0, b1, b2, eb);
	rtk_touch_cross(eb[0], eb[1], nb);
	if (rtk_touch_axis_separates(q.n, q.d1, q.d2, w0, w1, w2)) return true;
	if (rtk_touch_axis_separates(nb, q.d1, q.d2, w0, w1, w2)) return true;
	for (int i = 0; i < 3; i++) {
		bool sep = false;
		for (int j = 0; j < 3; j++) {
			rtk_touch_cross(q.e[i], eb[j], m);
			sep = sep || rtk_touch_axis_separates(m, q.d1, q.d2, w0, w1, w2);
		}
		if (sep) return true;
	}
	bool sep = false;
	for (int i = 0; i < 3; i++) sep = sep || rtk_touch_axis_separates(q.ne[i], q.d1, q.d2, w0, w1, w2);
	for (int j = 0; j < 3; j++) {
		rtk_touch_cross(nb, eb[j], m);
		sep = sep || rtk_touch_axis_separates(m, q.d1, q.d2, w0, w1, w2);
	}
	return sep;
}

// 5. q.a0, q.d1 and q.d2 do not give a1 and a2 back: the query's vertices are passed as they are
RTK_CLOSEST_FN bool rtk_touch_shares_vertex(const float *a0, const float *a1, const float *a2, const float *b0, const float *b1, const float *b2)
{
	const float *const av[3] = { a0, a1, a2 }, *const bv[3] = { b0, b1, b2 };
	bool shared = false;
	for (int i = 0; i < 3; i++) {
		for (int j = 0; j < 3; j++) shared = shared || (av[i][0] == bv[j][0] && av[i][1] == bv[j][1] && av[i][2] == bv[j][2]);
	}
	return shared;
}

RTK_CLOSEST_FN bool rtk_touch_filter_passes(uint32_t prim, uint32_t first_prim, uint32_t flags, const float *a0, const float *a1, const float *a2,
	const float *b0, const float *b1, const float *b2)
{
	if (prim < first_prim) return false;
	return !((flags & RTK_TOUCH_RULE_SKIP_SHARED_VERTEX) && rtk_touch_shares_vertex(a0, a1, a2, b0, b1, b2));
}

// 4. q from rtk_touch_hoist_query(a0, a1, a2) of a LIVE query
RTK_CLOSEST_FN bool rtk_touch_candidate(const rtk_touch_hoist &q, const float *a0, const float *a1, const float *a2,
	const float *b0, const float *b1, const float *b2, uint32_t prim, uint32_t first_prim, uint32_t flags)
{
	return rtk_touch_boxes_touch(b0, b1, b2, q.lo, q.hi) && rtk_touch_filter_passes(prim, first_prim, flags, a0, a1, a2, b0, b1, b2)
		&& !rtk_touch_separated(q, b0, b1, b2);
}
