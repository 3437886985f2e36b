// rtk_split_rule.h -- how ONE leaf of more than max_leaf triangles becomes a small subtree of 4-wide nodes whose leaves hold at
// most max_leaf (rtk_dev_scene_split_leaves, rtk_split.hip). Plain C++ without HIP types: the device runs it inside a wave,
// tests/split_rule_driver.cpp runs the same text on the CPU under the sanitizers.
//
// The triangles of the leaf are numbered 0 .. count-1 in slot order. The result is a permutation of them (SplitShape::perm:
// which triangle moves to which position of the leaf's slot range) and the nodes over it, breadth-first, node 0 the subtree's
// root. Every node and every leaf of the subtree covers a CONTIGUOUS run of positions; a node's children are the runs between
// its cuts.
//
// The rule. A node over n > max_leaf triangles is cut in two, and each half that still holds more than max_leaf in two again:
// two to four children, never an empty one. Where a cut goes is a surface-area sweep: the run sorted by centroid on each axis
// (ties by triangle number), cost(i) = area(first i) * i + area(the rest) * (n - i), the cheapest (axis, i), the first one
// among equals. If a centroid of the leaf is not finite, or no candidate has a cost that is (areas that overflow), the run
// is taken in slot order and cut in the middle.
// The depth cap. Let D be the smallest d with max_leaf * 4^d >= count: what a plain four-way median split needs. The subtree
// gets a budget of B = 2 D node levels; a node with budget b hands b - 1 to its children. The sweep may only choose cuts
// after which every child holds at most C(b) = max_leaf * 4^(b-1) triangles: exactly what b - 1 further levels can always
// take apart (DESIGN.md 3.4c derives it). At b = 1 that is max_leaf: every child is a leaf, the budget is never overdrawn.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define RTK_SPLIT_FN __host__ __device__ inline
#else
#define RTK_SPLIT_FN inline
#endif

#define RTK_SPLIT_MAX_TRIS 63u           // a leaf holds 1 .. 63 triangles (6-bit count, rtk.c:188)
#define RTK_SPLIT_MAX_NODES 62u          // every node has two children or more: at most count - 1 nodes
#define RTK_SPLIT_CHILD_LEAF 0xffu       // SplitNode::child: the run is a leaf

// one leaf as the rule sees it: per triangle its box and centroid, and the three orders by centroid
struct SplitLeaf {
	float lo[3][64], hi[3][64];          // [axis][triangle]
	float cen[3][64];
	uint8_t order[3][64];                // [axis][rank] -> triangle (rtk_split_rank gives a triangle's rank)
	uint32_t finite;                     // every centroid of the leaf is finite
};

struct SplitNode {
	uint8_t cut[5];                      // child k covers positions [cut[k], cut[k+1])
	uint8_t child[4];                    // node number inside the subtree, or RTK_SPLIT_CHILD_LEAF
	uint8_t num_children;                // 2 .. 4; slots from here on are empty
	uint8_t budget;                      // node levels this node and what is below it may use
	uint8_t level;                       // 1 = the subtree's root
};

struct SplitShape {
	uint8_t perm[64];                    // position -> triangle number (a permutation of 0 .. count-1)
	SplitNode node[RTK_SPLIT_MAX_NODES];
	uint32_t num_nodes;
	uint32_t levels;                     // node levels of the subtree (0: the leaf stays)
};

struct SplitWork {                       // scratch of one run of the rule
	float right_area[64];
	uint8_t list[64];
};

// the smallest d with max_leaf * 4^d >= count: the levels a four-way median split needs
RTK_SPLIT_FN uint32_t rtk_split_median_levels(uint32_t count, uint32_t max_leaf)
{
	uint32_t d = 0;
	for (uint32_t cap = max_leaf; cap < count; cap *= 4u) d++;
	return d;
}
// the depth cap of the contract
RTK_SPLIT_FN uint32_t rtk_split_level_cap(uint32_t count, uint32_t max_leaf) { return 2u * rtk_split_median_levels(count, max_leaf); }

// how many triangles a child of a node with budget b may hold: max_leaf * 4^(b-1), saturated (no leaf has more than 63)
RTK_SPLIT_FN uint32_t rtk_split_child_cap(uint32_t max_leaf, uint32_t budget)
{
	uint32_t c = max_leaf;
	for (uint32_t k = 1; k < budget && c < 64u; k++) c *= 4u;
	return c < 64u ? c : 64u;
}

// rank of triangle t among the leaf's triangles by centroid on `axis`, ties by number (a strict total order while the centroids
// are finite; the orders are not used otherwise)
RTK_SPLIT_FN uint32_t rtk_split_rank(const SplitLeaf &in, uint32_t count, uint32_t axis, uint32_t t)
{
	const float c = in.cen[axis][t];
	uint32_t r = 0;
	for (uint32_t u = 0; u < count; u++) {
		const float d = in.cen[axis][u];
		r += (d < c || (d == c && u < t)) ? 1u : 0u;
	}
	return r;
}

RTK_SPLIT_FN bool rtk_split_is_finite(float x) { return x - x == 0.0f; }

// the serial form of what the wave does with one lane per triangle: in.finite and the three orders from in.cen
RTK_SPLIT_FN void rtk_split_prepare(SplitLeaf &in, uint32_t count)
{
	uint32_t finite = 1u;
	for (uint32_t t = 0; t < count; t++)
		for (uint32_t a = 0; a < 3u; a++) if (!rtk_split_is_finite(in.cen[a][t])) finite = 0u;
	in.finite = finite;
	for (uint32_t a = 0; a < 3u; a++) {
		for (uint32_t t = 0; t < count; t++) in.order[a][t] = (uint8_t)t;      // (something defined where ranks collide: NaN)
		if (finite) for (uint32_t t = 0; t < count; t++) in.order[a][rtk_split_rank(in, count, a, t)] = (uint8_t)t;
	}
}

struct SplitBox { float mn[3], mx[3]; };
RTK_SPLIT_FN void rtk_split_box_grow(SplitBox &b, const SplitLeaf &in, uint32_t t, bool first)
{
	for (uint32_t a = 0; a < 3u; a++) {
		const float l = in.lo[a][t], h = in.hi[a][t];
		b.mn[a] = first || l < b.mn[a] ? l : b.mn[a];
		b.mx[a] = first || h > b.mx[a] ? h : b.mx[a];
	}
}
RTK_SPLIT_FN float rtk_split_box_area(const SplitBox &b)
{
	const float dx = b.mx[0] - b.mn[0], dy = b.mx[1] - b.mn[1], dz = b.mx[2] - b.mn[2];
	return 2.0f * (dx * dy + dy * dz + dz * dx);
}

// the triangles of `members` (bit t) in the order of `axis` (3: by number) -> w.list
RTK_SPLIT_FN void rtk_split_gather(const SplitLeaf &in, uint32_t count, unsigned long long members, uint32_t axis, SplitWork &w)
{
	uint32_t m = 0;
	for (uint32_t r = 0; r < count; r++) {
		const uint32_t t = axis < 3u ? in.order[axis][r] : r;
		if ((members >> t) & 1ull) w.list[m++] = (uint8_t)t;
	}
}

// Cuts the run [begin, end) of sh.perm in two parts of at most `part_max` triangles each (end - begin <= 2 * part_max, >= 2):
// reorders the run and returns the first position of the second part.
RTK_SPLIT_FN uint32_t rtk_split_two(const SplitLeaf &in, uint32_t count, SplitShape &sh, SplitWork &w, uint32_t begin, uint32_t end, uint32_t part_max)
{
	const uint32_t n = end - begin;
	const uint32_t at_min = n > part_max + 1u ? n - part_max : 1u, at_max = n - 1u < part_max ? n - 1u : part_max;
	unsigned long long members = 0;
	for (uint32_t p = begin; p < end; p++) members |= 1ull << sh.perm[p];
	uint32_t best_axis = 3u, best_at = 0u;
	float best = 0.0f;
	if (in.finite) {
		for (uint32_t axis = 0; axis < 3u; axis++) {
			rtk_split_gather(in, count, members, axis, w);
			SplitBox box = {};
			for (uint32_t j = n - 1u; j >= 1u; j--) {
				rtk_split_box_grow(box, in, w.list[j], j == n - 1u);
				w.right_area[j] = rtk_split_box_area(box);
			}
			for (uint32_t i = 1; i <= at_max; i++) {
				rtk_split_box_grow(box, in, w.list[i - 1u], i == 1u);
				if (i < at_min) continue;
				const float cost = rtk_split_box_area(box) * (float)i + w.right_area[i] * (float)(n - i);
				if (rtk_split_is_finite(cost) && (best_axis == 3u || cost < best)) { best = cost; best_axis = axis; best_at = i; }
			}
		}
	}
	if (best_axis == 3u) {
		// slot order, the middle (inside what the cap allows)
		best_at = (n + 1u) / 2u;
		best_at = best_at < at_min ? at_min : best_at > at_max ? at_max : best_at;
	}
	rtk_split_gather(in, count, members, best_axis, w);
	for (uint32_t j = 0; j < n; j++) sh.perm[begin + j] = w.list[j];
	return begin + best_at;
}

// The whole subtree of one leaf. `in` prepared (rtk_split_prepare, or the wave's own form of it); 1 <= count <= 63,
// 1 <= max_leaf <= 63.
RTK_SPLIT_FN void rtk_split_rule(const SplitLeaf &in, uint32_t count, uint32_t max_leaf, SplitShape &sh, SplitWork &w)
{
	for (uint32_t p = 0; p < 64u; p++) sh.perm[p] = (uint8_t)p;
	sh.num_nodes = 0;
	sh.levels = 0;
	if (count <= max_leaf || count > RTK_SPLIT_MAX_TRIS || max_leaf == 0u) return;
	// (until a node is taken from the queue its run waits in cut[0], cut[1])
	sh.node[0].cut[0] = 0; sh.node[0].cut[1] = (uint8_t)count;
	sh.node[0].budget = (uint8_t)rtk_split_level_cap(count, max_leaf);
	sh.node[0].level = 1;
	sh.num_nodes = 1;
	for (uint32_t q = 0; q < sh.num_nodes; q++) {
		SplitNode &nd = sh.node[q];
		const uint32_t begin = nd.cut[0], end = nd.cut[1];
		const uint32_t child_max = rtk_split_child_cap(max_leaf, nd.budget);
		const uint32_t mid = rtk_split_two(in, count, sh, w, begin, end, 2u * child_max);
		uint32_t cuts[5], k = 0;
		cuts[k++] = begin;
		if (mid - begin > max_leaf) cuts[k++] = rtk_split_two(in, count, sh, w, begin, mid, child_max);
		cuts[k++] = mid;
		if (end - mid > max_leaf) cuts[k++] = rtk_split_two(in, count, sh, w, mid, end, child_max);
		cuts[k] = end;
		nd.num_children = (uint8_t)k;
		for (uint32_t c = 0; c <= 4u; c++) nd.cut[c] = (uint8_t)(c <= k ? cuts[c] : end);
		for (uint32_t c = 0; c < 4u; c++) {
			nd.child[c] = RTK_SPLIT_CHILD_LEAF;
			if (c >= k || cuts[c + 1u] - cuts[c] <= max_leaf || sh.num_nodes >= RTK_SPLIT_MAX_NODES) continue;
			SplitNode &ch = sh.node[sh.num_nodes];
			ch.cut[0] = (uint8_t)cuts[c]; ch.cut[1] = (uint8_t)cuts[c + 1u];
			ch.budget = (uint8_t)(nd.budget - 1u);
			ch.level = (uint8_t)(nd.level + 1u);
			nd.child[c] = (uint8_t)sh.num_nodes++;
		}
		if (nd.level > sh.levels) sh.levels = nd.level;
	}
}

// how many nodes the subtree of the leaf has (what the counting pass asks before anything is allocated)
RTK_SPLIT_FN uint32_t rtk_split_rule_count(const SplitLeaf &in, uint32_t count, uint32_t max_leaf, SplitShape &sh, SplitWork &w)
{
	rtk_split_rule(in, count, max_leaf, sh, w);
	return sh.num_nodes;
}
