// pair_rule_driver.cpp -- rtk_amd/csrc/rtk_pair_rule.h on the CPU: tests/test_pair_cpu.py builds this with the host compiler,
// -ffp-contract=off as the library is built, and the address and undefined-behaviour sanitizers, against the rule headers alone.
//
//   pair_rule_driver -b FILE   FILE holds raw 32-bit words, 24 per case: a0[3] a1[3] a2[3] b0[3] b1[3] b2[3] lo[3] hi[3]. Prints per
//       case one line of hexadecimal words: dist2 u v qa[3] qb[3] of rtk_pair_evaluate, the bound of rtk_pair_box_bound([lo, hi]
//       against A's box), then the feature and rtk_touch_live(A) in decimal. Then "ok".
//   pair_rule_driver FILE      reads text cases; every number after the case letter and the decimal counts is the hexadecimal
//       bits of a 32-bit word:
//     n count   then count nodes of 28 words: xlo[4] xhi[4] ylo[4] yhi[4] zlo[4] zhi[4] child[4]   (replaces the tree)
//         a child word: 0xffffffff empty, bit 31 set: a leaf whose records begin at slot (word & 0x7fffffff), else a node index
//     t count   then count triangle records of 11 words: a[3] b[3] c[3] prim last (non-zero: the leaf's run ends here)
//     q order   then 12 words: a0[3] a1[3] a2[3] max_dist2 first_prim flags
//         a host walk of the tree from node 0 with rtk_touch_live / rtk_pair_box_bound / rtk_pair_skip / rtk_touch_filter_passes /
//         rtk_pair_evaluate / rtk_pair_wins; the children of a node are visited in slot order (order 0), in reverse slot order (1),
//         in an order drawn per node (2) or nearest bound first (3). A record whose own box is skipped is not evaluated.
//         prints: dist2 u v prim qa[3] qb[3] as the call would write them, then the number of records evaluated in decimal
// one line of output per q case; "ok" at the end. A line it cannot read ends the run with status 1.
#include "rtk_pair_rule.h"

#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

struct Node { float box[6][4]; uint32_t child[4]; };
struct Tri { float a[3], b[3], c[3]; uint32_t prim, last; };

static const uint32_t NONE = 0xffffffffu;

static float as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t as_word(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static bool read_words(FILE *in, uint32_t *w, size_t n)
{
	for (size_t k = 0; k < n; k++) if (fscanf(in, "%" SCNx32, &w[k]) != 1) return false;
	return true;
}

struct Walk {
	const std::vector<Node> &nodes;
	const std::vector<Tri> &tris;
	const float *a0, *a1, *a2;
	float max2;
	uint32_t first, flags;
	rtk_pair_hoist h;
	int order;
	uint32_t rnd;
	float best2, best_u, best_v, best_qa[3], best_qb[3];
	uint32_t best_prim;
	unsigned long evaluated;

	void leaf(uint32_t slot)
	{
		while (slot < tris.size()) {
			const Tri &t = tris[slot];
			float lo[3], hi[3];
			rtk_pair_box(t.a, t.b, t.c, lo, hi);
			if (rtk_touch_filter_passes(t.prim, first, flags, a0, a1, a2, t.a, t.b, t.c) && !rtk_pair_skip(rtk_pair_box_bound(lo, hi, h.lo, h.hi), best2, max2)) {
				rtk_pair_result r;
				rtk_pair_evaluate(h, t.a, t.b, t.c, r);
				evaluated++;
				if (rtk_pair_wins(r.dist2, t.prim, max2, best2, best_prim)) {
					best2 = r.dist2; best_u = r.u; best_v = r.v; best_prim = t.prim;
					for (int x = 0; x < 3; x++) { best_qa[x] = r.qa[x]; best_qb[x] = r.qb[x]; }
				}
			}
			if (t.last) break;
			slot++;
		}
	}
	void visit(uint32_t ref)
	{
		if (ref == NONE) return;
		if (ref & 0x80000000u) { leaf(ref & 0x7fffffffu); return; }
		if (ref >= nodes.size()) return;
		const Node &n = nodes[ref];
		int at[4] = { 0, 1, 2, 3 };
		float bound[4];
		for (int k = 0; k < 4; k++) {
			const float clo[3] = { n.box[0][k], n.box[2][k], n.box[4][k] }, chi[3] = { n.box[1][k], n.box[3][k], n.box[5][k] };
			bound[k] = rtk_pair_box_bound(clo, chi, h.lo, h.hi);
		}
		if (order == 1) { at[0] = 3; at[1] = 2; at[2] = 1; at[3] = 0; }
		if (order == 2) {
			for (int i = 3; i > 0; i--) {
				rnd = rnd * 1664525u + 1013904223u;
				const int j = (int)((rnd >> 16) % (uint32_t)(i + 1)), s = at[i];
				at[i] = at[j]; at[j] = s;
			}
		}
		if (order == 3) {
			for (int i = 1; i < 4; i++) for (int j = i; j > 0 && bound[at[j]] < bound[at[j - 1]]; j--) { const int s = at[j]; at[j] = at[j - 1]; at[j - 1] = s; }
		}
		for (int i = 0; i < 4; i++) {
			const int k = at[i];
			if (n.child[k] == NONE || rtk_pair_skip(bound[k], best2, max2)) continue;      // (best2 as it is by now)
			visit(n.child[k]);
		}
	}
};

static int bulk(const char *path)
{
	FILE *in = fopen(path, "rb");
	if (!in) { fprintf(stderr, "pair_rule_driver: cannot open %s\n", path); return 1; }
	uint32_t w[24];
	while (fread(w, sizeof(uint32_t), 24, in) == 24) {
		float f[24];
		for (int k = 0; k < 24; k++) f[k] = as_float(w[k]);
		rtk_pair_hoist h;
		rtk_pair_hoist_query(f, f + 3, f + 6, h);
		rtk_pair_result r;
		rtk_pair_evaluate(h, f + 9, f + 12, f + 15, r);
		const float bound = rtk_pair_box_bound(f + 18, f + 21, h.lo, h.hi);
		printf("%" PRIx32 " %" PRIx32 " %" PRIx32, as_word(r.dist2), as_word(r.u), as_word(r.v));
		for (int x = 0; x < 3; x++) printf(" %" PRIx32, as_word(r.qa[x]));
		for (int x = 0; x < 3; x++) printf(" %" PRIx32, as_word(r.qb[x]));
		printf(" %" PRIx32 " %d %d\n", as_word(bound), r.feature, rtk_touch_live(f, f + 3, f + 6) ? 1 : 0);
	}
	fclose(in);
	printf("ok\n");
	return 0;
}

int main(int argc, char **argv)
{
	if (argc > 2 && strcmp(argv[1], "-b") == 0) return bulk(argv[2]);
	FILE *in = argc > 1 ? fopen(argv[1], "r") : stdin;
	if (!in) { fprintf(stderr, "pair_rule_driver: cannot open %s\n", argv[1]); return 1; }
	std::vector<Node> nodes;
	std::vector<Tri> tris;
	char kind;
	unsigned long cases = 0;
	while (fscanf(in, " %c", &kind) == 1) {
		if (kind == 'n' || kind == 't') {
			unsigned count;
			if (fscanf(in, "%u", &count) != 1) { fprintf(stderr, "pair_rule_driver: case %lu: bad count\n", cases); return 1; }
			if (kind == 'n') {
				nodes.assign(count, Node());
				for (Node &nd : nodes) {
					uint32_t w[28];
					if (!read_words(in, w, 28)) { fprintf(stderr, "pair_rule_driver: case %lu: bad node\n", cases); return 1; }
					for (int r = 0; r < 6; r++) for (int k = 0; k < 4; k++) nd.box[r][k] = as_float(w[r * 4 + k]);
					for (int k = 0; k < 4; k++) nd.child[k] = w[24 + k];
				}
			} else {
				tris.assign(count, Tri());
				for (Tri &t : tris) {
					uint32_t w[11];
					if (!read_words(in, w, 11)) { fprintf(stderr, "pair_rule_driver: case %lu: bad triangle\n", cases); return 1; }
					for (int k = 0; k < 3; k++) { t.a[k] = as_float(w[k]); t.b[k] = as_float(w[3 + k]); t.c[k] = as_float(w[6 + k]); }
					t.prim = w[9]; t.last = w[10];
				}
			}
		} else if (kind == 'q') {
			int order;
			uint32_t w[12];
			if (fscanf(in, "%d", &order) != 1 || order < 0 || order > 3 || !read_words(in, w, 12)) { fprintf(stderr, "pair_rule_driver: case %lu: bad query\n", cases); return 1; }
			float a[9];
			for (int k = 0; k < 9; k++) a[k] = as_float(w[k]);
			const float max2 = as_float(w[9]);
			Walk wk = { nodes, tris, a, a + 3, a + 6, max2, w[10], w[11], rtk_pair_hoist(), order, (uint32_t)cases * 2654435761u + 1u,
				max2, 0.0f, 0.0f, { a[0], a[1], a[2] }, { a[0], a[1], a[2] }, NONE, 0ul };
			rtk_pair_hoist_query(a, a + 3, a + 6, wk.h);
			if (rtk_touch_live(a, a + 3, a + 6) && max2 > 0.0f && !nodes.empty() && !tris.empty()) wk.visit(0u);
			const bool miss = wk.best_prim == NONE;
			printf("%" PRIx32 " %" PRIx32 " %" PRIx32 " %" PRIx32, miss ? w[9] : as_word(wk.best2), as_word(wk.best_u), as_word(wk.best_v), wk.best_prim);
			for (int x = 0; x < 3; x++) printf(" %" PRIx32, miss ? w[x] : as_word(wk.best_qa[x]));
			for (int x = 0; x < 3; x++) printf(" %" PRIx32, miss ? w[x] : as_word(wk.best_qb[x]));
			printf(" %lu\n", wk.evaluated);
		} else { fprintf(stderr, "pair_rule_driver: case %lu: kind '%c'\n", cases, kind); return 1; }
		cases++;
	}
	if (in != stdin) fclose(in);
	printf("ok\n");
	return 0;
}
