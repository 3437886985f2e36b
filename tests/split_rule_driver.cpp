// split_rule_driver.cpp -- rtk_amd/csrc/rtk_split_rule.h on the CPU (tests/test_split_leaves_cpu.py builds this with the host
// compiler and the address and undefined-behaviour sanitizers, against that header alone, and runs it).
//
// Leaves: every count 1 .. 63 of scattered triangles at max_leaf 1, 3, 4, 62, 63; 63 identical triangles; centroids on a line in
// geometric progression (a free surface-area sweep peels one triangle per level there); NaN and inf coordinates.
// For each: the permutation is one, every leaf of the subtree holds 1 .. max_leaf triangles, every node has two to four
// children that tile its run, children come after their parent (breadth-first), the levels are within
// 2 * ceil(log4(count / max_leaf)), the counting entry point agrees, and a second run gives the same bytes.
// Prints one line per family and "ok"; the first failure is printed and the exit status is 1.
#include "rtk_split_rule.h"

#include <math.h>
#include <stdio.h>
#include <string.h>

static int g_failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_failures++ < 20) { printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static uint32_t g_seed = 12345u;
static float rnd() { g_seed = g_seed * 1664525u + 1013904223u; return (float)(g_seed >> 8) * (1.0f / 16777216.0f); }

// a triangle as three vertices -> its box and centroid, the way rtk_split.hip makes them
static void set_tri(SplitLeaf &in, uint32_t t, const float v[3][3])
{
	for (int a = 0; a < 3; a++) {
		in.lo[a][t] = fminf(fminf(v[0][a], v[1][a]), v[2][a]);
		in.hi[a][t] = fmaxf(fmaxf(v[0][a], v[1][a]), v[2][a]);
		in.cen[a][t] = 0.5f * (in.lo[a][t] + in.hi[a][t]);
	}
}

// ceil(log4(count / max_leaf)) by exact integer arithmetic, independent of the header's loop
static uint32_t median_levels(uint32_t count, uint32_t max_leaf)
{
	uint32_t d = 0;
	unsigned long long cap = max_leaf;
	while (cap < count) { cap *= 4; d++; }
	return d;
}

static void check_leaf(const char *what, SplitLeaf &in, uint32_t count, uint32_t max_leaf, uint32_t *levels_out)
{
	static SplitShape sh, again;
	static SplitWork w;
	rtk_split_prepare(in, count);
	memset(&sh, 0xab, sizeof(sh));
	memset(&again, 0xcd, sizeof(again));
	rtk_split_rule(in, count, max_leaf, sh, w);
	const uint32_t counted = rtk_split_rule_count(in, count, max_leaf, again, w);
	CHECK(counted == sh.num_nodes, "%s count %u max_leaf %u: counted %u, made %u", what, count, max_leaf, counted, sh.num_nodes);
	// a second run: the same permutation, the same nodes (the fields the rule defines)
	CHECK(memcmp(sh.perm, again.perm, sizeof(sh.perm)) == 0, "%s count %u max_leaf %u: second run permutes differently", what, count, max_leaf);
	CHECK(sh.levels == again.levels, "%s: levels differ between runs", what);
	for (uint32_t q = 0; q < sh.num_nodes && q < counted; q++) CHECK(memcmp(&sh.node[q], &again.node[q], sizeof(SplitNode)) == 0, "%s count %u max_leaf %u: node %u differs in the second run", what, count, max_leaf, q);
	// a permutation of 0 .. count-1 (and the identity beyond)
	unsigned long long seen = 0;
	for (uint32_t p = 0; p < count; p++) { CHECK(sh.perm[p] < count, "%s: perm[%u] = %u", what, p, sh.perm[p]); seen |= 1ull << (sh.perm[p] & 63u); }
	CHECK(seen == (count == 64u ? ~0ull : (1ull << count) - 1ull), "%s count %u max_leaf %u: not a permutation", what, count, max_leaf);
	if (count <= max_leaf) {
		CHECK(sh.num_nodes == 0 && sh.levels == 0, "%s count %u max_leaf %u: a leaf that fits was split", what, count, max_leaf);
		for (uint32_t p = 0; p < count; p++) CHECK(sh.perm[p] == p, "%s: a leaf that fits was permuted", what);
		if (levels_out) *levels_out = 0;
		return;
	}
	const uint32_t cap = 2u * median_levels(count, max_leaf);
	CHECK(rtk_split_level_cap(count, max_leaf) == cap, "%s: the header's cap", what);
	CHECK(sh.num_nodes >= 1 && sh.num_nodes <= RTK_SPLIT_MAX_NODES, "%s: %u nodes", what, sh.num_nodes);
	CHECK(sh.node[0].cut[0] == 0 && sh.node[0].cut[sh.node[0].num_children] == count, "%s: the root does not cover the leaf", what);
	uint32_t referenced[RTK_SPLIT_MAX_NODES] = {}, covered = 0, deepest = 0, next_child = 1;
	uint32_t level_of[RTK_SPLIT_MAX_NODES] = {};
	level_of[0] = 1;
	for (uint32_t q = 0; q < sh.num_nodes && q < RTK_SPLIT_MAX_NODES; q++) {
		const SplitNode &nd = sh.node[q];
		CHECK(nd.num_children >= 2 && nd.num_children <= 4, "%s count %u max_leaf %u: node %u has %u children", what, count, max_leaf, q, nd.num_children);
		CHECK(level_of[q] >= 1 && level_of[q] <= cap, "%s count %u max_leaf %u: node %u at level %u, cap %u", what, count, max_leaf, q, level_of[q], cap);
		if (level_of[q] > deepest) deepest = level_of[q];
		for (uint32_t k = 0; k < nd.num_children && k < 4u; k++) {
			CHECK(nd.cut[k] < nd.cut[k + 1], "%s count %u max_leaf %u: node %u child %u is empty", what, count, max_leaf, q, k);
			const uint32_t size = (uint32_t)nd.cut[k + 1] - nd.cut[k];
			if (nd.child[k] == RTK_SPLIT_CHILD_LEAF) {
				CHECK(size <= max_leaf, "%s count %u max_leaf %u: a leaf of %u", what, count, max_leaf, size);
				covered += size;
			} else {
				CHECK(size > max_leaf, "%s count %u max_leaf %u: %u triangles under a node", what, count, max_leaf, size);
				// breadth-first: children are handed out in the order they are met, so always after their parent
				CHECK(nd.child[k] == next_child && nd.child[k] > q && nd.child[k] < sh.num_nodes, "%s: node %u child %u is node %u, expected %u", what, q, k, nd.child[k], next_child);
				next_child++;
				if (nd.child[k] < sh.num_nodes) {
					referenced[nd.child[k]]++;
					level_of[nd.child[k]] = level_of[q] + 1;
					const SplitNode &ch = sh.node[nd.child[k]];
					CHECK(ch.cut[0] == nd.cut[k] && ch.cut[ch.num_children <= 4 ? ch.num_children : 4] == nd.cut[k + 1], "%s: node %u does not cover its parent's run", what, nd.child[k]);
				}
			}
		}
	}
	CHECK(next_child == sh.num_nodes, "%s: %u nodes referenced, %u made", what, next_child, sh.num_nodes);
	for (uint32_t q = 1; q < sh.num_nodes; q++) CHECK(referenced[q] == 1, "%s: node %u referenced %u times", what, q, referenced[q]);
	CHECK(covered == count, "%s count %u max_leaf %u: leaves cover %u triangles", what, count, max_leaf, covered);
	CHECK(deepest == sh.levels && sh.levels <= cap, "%s count %u max_leaf %u: %u levels (reported %u), cap %u", what, count, max_leaf, deepest, sh.levels, cap);
	if (levels_out) *levels_out = deepest;
}

static const uint32_t LIMITS[5] = { 1, 3, 4, 62, 63 };

int main()
{
	static SplitLeaf in;
	uint32_t leaves = 0;
	// scattered triangles, every count
	for (uint32_t count = 1; count <= 63; count++) {
		for (uint32_t li = 0; li < 5; li++) {
			memset(&in, 0, sizeof(in));
			for (uint32_t t = 0; t < count; t++) {
				float v[3][3];
				const float c[3] = { 10.0f * rnd() - 5.0f, 10.0f * rnd() - 5.0f, 4.0f * rnd() };
				for (int k = 0; k < 3; k++) for (int a = 0; a < 3; a++) v[k][a] = c[a] + 0.3f * (rnd() - 0.5f);
				set_tri(in, t, v);
			}
			check_leaf("scattered", in, count, LIMITS[li], nullptr);
			leaves++;
		}
	}
	printf("scattered: %u leaves\n", leaves);
	// 63 identical triangles: every cost ties, every centroid ties -> slot order must survive
	for (uint32_t li = 0; li < 5; li++) {
		memset(&in, 0, sizeof(in));
		const float v[3][3] = { { 1.0f, 2.0f, 3.0f }, { 2.0f, 2.0f, 3.5f }, { 1.0f, 3.0f, 3.0f } };
		for (uint32_t t = 0; t < 63; t++) set_tri(in, t, v);
		static SplitShape sh;
		static SplitWork w;
		uint32_t levels = 0;
		check_leaf("identical", in, 63, LIMITS[li], &levels);
		rtk_split_rule(in, 63, LIMITS[li], sh, w);
		for (uint32_t p = 0; p < 63; p++) CHECK(sh.perm[p] == p, "identical, max_leaf %u: position %u holds triangle %u (ties go by slot number)", LIMITS[li], p, sh.perm[p]);
		printf("identical: max_leaf %u -> %u nodes, %u levels\n", LIMITS[li], sh.num_nodes, levels);
	}
	// centroids at 2^t on a line, small triangles: the free sweep would take one triangle off per level (62 levels)
	for (uint32_t li = 0; li < 5; li++) {
		memset(&in, 0, sizeof(in));
		for (uint32_t t = 0; t < 63; t++) {
			const float x = ldexpf(1.0f, (int)t - 20);
			const float v[3][3] = { { x, 0.0f, 0.0f }, { x * 1.01f, 0.01f * x, 0.0f }, { x, 0.0f, 0.01f * x } };
			set_tri(in, (t * 29u) % 63u, v);                          // (29 is coprime to 63: slot order is not the line's order)
		}
		uint32_t levels = 0;
		check_leaf("geometric", in, 63, LIMITS[li], &levels);
		printf("geometric: max_leaf %u -> %u levels, cap %u\n", LIMITS[li], levels, rtk_split_level_cap(63, LIMITS[li]));
	}
	// NaN and inf coordinates: in some triangles, in all of them, as boxes that overflow
	for (int family = 0; family < 4; family++) {
		for (uint32_t li = 0; li < 5; li++) {
			memset(&in, 0, sizeof(in));
			for (uint32_t t = 0; t < 63; t++) {
				float v[3][3];
				for (int k = 0; k < 3; k++) for (int a = 0; a < 3; a++) v[k][a] = rnd();
				if (family == 0 && t % 7 == 3) v[1][t % 3] = NAN;
				if (family == 1 && t % 5 == 1) v[2][t % 3] = (t & 1) ? INFINITY : -INFINITY;
				if (family == 2) { v[0][0] = NAN; v[1][1] = INFINITY; v[2][2] = -INFINITY; }
				if (family == 3) { v[0][t % 3] = 3.0e38f; v[1][t % 3] = -3.0e38f; }   // finite planes, extents and areas that are not
				set_tri(in, t, v);
			}
			check_leaf("non-finite", in, 63, LIMITS[li], nullptr);
		}
	}
	printf("non-finite: 20 leaves\n");
	if (g_failures) { printf("%d failures\n", g_failures); return 1; }
	printf("ok\n");
	return 0;
}
