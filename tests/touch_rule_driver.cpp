// touch_rule_driver.cpp -- rtk_amd/csrc/rtk_touch_rule.h on the CPU: tests/test_touch_cpu.py builds this with the host compiler,
// -ffp-contract=off as the library is built, and the address and undefined-behaviour sanitizers, against the rule headers alone.
//
//   touch_rule_driver -b FILE   FILE holds raw 32-bit words, 27 per case: a0[3] a1[3] a2[3] b0[3] b1[3] b2[3] clo[3] chi[3] prim
//       first_prim flags. Prints one hexadecimal number per case, one per line: bit 0 rtk_touch_live(A), bit 1
//       rtk_touch_boxes_touch, bit 2 rtk_box_skip(clo, chi, alo, ahi), bit 3 rtk_touch_filter_passes, bits 4 .. 20 the seventeen
//       axes of rtk_touch_separating_axes in the rule's order. The candidate of rule 4 is bits 0, 1 and 3 without any of bits
//       4 .. 20, and the driver ends with status 1 if rtk_touch_candidate or rtk_touch_separated says otherwise. Then "ok".
//   touch_rule_driver FILE      reads text cases; every number after the case letter and the decimal counts is the hexadecimal
//       bits of a 32-bit word:
//     n count   then count nodes of 28 words: xlo[4] xhi[4] ylo[4] yhi[4] zlo[4] zhi[4] child[4]   (replaces the tree)
//         a child word: 0xffffffff empty, bit 31 set: a leaf whose records begin at slot (word & 0x7fffffff), else a node index
//     t count   then count triangle records of 11 words: a[3] b[3] c[3] prim last (non-zero: the leaf's run ends here)
//     q order   then 12 words: a0[3] a1[3] a2[3] room first_prim flags
//         a host walk of the tree from node 0 with rtk_touch_live / rtk_box_skip / rtk_touch_candidate / rtk_box_insert; the
//         children of a node are visited in slot order (order 0), in reverse slot order (1) or in an order drawn per node (2).
//         The count is a walk of its own. The segment stands between GUARD entries filled with 0x7e on either side.
//         prints: count, kept, and the GUARD + room + GUARD words
// one line of output per q case; "ok" at the end. A line it cannot read ends the run with status 1.
#include "rtk_touch_rule.h"

#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

struct Node { float box[6][4]; uint32_t child[4]; };
struct Tri { float a[3], b[3], c[3]; uint32_t prim, last; };

static const uint32_t GUARD = 4, NONE = 0xffffffffu;

static float as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

static bool read_words(FILE *in, uint32_t *w, size_t n)
{
	for (size_t k = 0; k < n; k++) if (fscanf(in, "%" SCNx32, &w[k]) != 1) return false;
	return true;
}

struct Walk {
	const std::vector<Node> &nodes;
	const std::vector<Tri> &tris;
	const float *a0, *a1, *a2;
	uint32_t first, flags;
	rtk_touch_hoist q;
	int order;
	bool fill;
	uint32_t *seg;
	uint32_t room, kept, worst, rnd;

	void leaf(uint32_t slot)
	{
		while (slot < tris.size()) {
			const Tri &t = tris[slot];
			if (rtk_touch_candidate(q, a0, a1, a2, t.a, t.b, t.c, t.prim, first, flags)) {
				if (fill) kept = rtk_box_insert(seg, room, kept, t.prim, worst);
				else kept++;
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
		if (order == 1) { at[0] = 3; at[1] = 2; at[2] = 1; at[3] = 0; }
		if (order == 2) {
			for (int i = 3; i > 0; i--) {
				rnd = rnd * 1664525u + 1013904223u;
				const int j = (int)((rnd >> 16) % (uint32_t)(i + 1)), s = at[i];
				at[i] = at[j]; at[j] = s;
			}
		}
		for (int i = 0; i < 4; i++) {
			const int k = at[i];
			const float clo[3] = { n.box[0][k], n.box[2][k], n.box[4][k] }, chi[3] = { n.box[1][k], n.box[3][k], n.box[5][k] };
			if (n.child[k] == NONE || rtk_box_skip(clo, chi, q.lo, q.hi)) continue;
			visit(n.child[k]);
		}
	}
};

static int bulk(const char *path)
{
	FILE *in = fopen(path, "rb");
	if (!in) { fprintf(stderr, "touch_rule_driver: cannot open %s\n", path); return 1; }
	uint32_t w[27];
	unsigned long cases = 0;
	while (fread(w, sizeof(uint32_t), 27, in) == 27) {
		float f[24];
		for (int k = 0; k < 24; k++) f[k] = as_float(w[k]);
		const float *a0 = f, *a1 = f + 3, *a2 = f + 6, *b0 = f + 9, *b1 = f + 12, *b2 = f + 15, *clo = f + 18, *chi = f + 21;
		const uint32_t prim = w[24], first = w[25], flags = w[26];
		rtk_touch_hoist q;
		rtk_touch_hoist_query(a0, a1, a2, q);
		const bool live = rtk_touch_live(a0, a1, a2), touch = rtk_touch_boxes_touch(b0, b1, b2, q.lo, q.hi);
		const bool skip = rtk_box_skip(clo, chi, q.lo, q.hi), pass = rtk_touch_filter_passes(prim, first, flags, a0, a1, a2, b0, b1, b2);
		const uint32_t axes = rtk_touch_separating_axes(q, b0, b1, b2);
		if (rtk_touch_separated(q, b0, b1, b2) != (axes != 0u)) { fprintf(stderr, "touch_rule_driver: case %lu: rtk_touch_separated is not rule 3\n", cases); return 1; }
		if (rtk_touch_candidate(q, a0, a1, a2, b0, b1, b2, prim, first, flags) != (touch && pass && axes == 0u)) {
			fprintf(stderr, "touch_rule_driver: case %lu: rtk_touch_candidate is not rule 4\n", cases);
			return 1;
		}
		printf("%" PRIx32 "\n", (live ? 1u : 0u) | (touch ? 2u : 0u) | (skip ? 4u : 0u) | (pass ? 8u : 0u) | axes << 4);
		cases++;
	}
	fclose(in);
	printf("ok\n");
	return 0;
}

int main(int argc, char **argv)
{
	if (argc > 2 && strcmp(argv[1], "-b") == 0) return bulk(argv[2]);
	FILE *in = argc > 1 ? fopen(argv[1], "r") : stdin;
	if (!in) { fprintf(stderr, "touch_rule_driver: cannot open %s\n", argv[1]); return 1; }
	std::vector<Node> nodes;
	std::vector<Tri> tris;
	char kind;
	unsigned long cases = 0;
	while (fscanf(in, " %c", &kind) == 1) {
		if (kind == 'n' || kind == 't') {
			unsigned count;
			if (fscanf(in, "%u", &count) != 1) { fprintf(stderr, "touch_rule_driver: case %lu: bad count\n", cases); return 1; }
			if (kind == 'n') {
				nodes.assign(count, Node());
				for (Node &nd : nodes) {
					uint32_t w[28];
					if (!read_words(in, w, 28)) { fprintf(stderr, "touch_rule_driver: case %lu: bad node\n", cases); return 1; }
					for (int r = 0; r < 6; r++) for (int k = 0; k < 4; k++) nd.box[r][k] = as_float(w[r * 4 + k]);
					for (int k = 0; k < 4; k++) nd.child[k] = w[24 + k];
				}
			} else {
				tris.assign(count, Tri());
				for (Tri &t : tris) {
					uint32_t w[11];
					if (!read_words(in, w, 11)) { fprintf(stderr, "touch_rule_driver: case %lu: bad triangle\n", cases); return 1; }
					for (int k = 0; k < 3; k++) { t.a[k] = as_float(w[k]); t.b[k] = as_float(w[3 + k]); t.c[k] = as_float(w[6 + k]); }
					t.prim = w[9]; t.last = w[10];
				}
			}
		} else if (kind == 'q') {
			int order;
			uint32_t w[12];
			if (fscanf(in, "%d", &order) != 1 || order < 0 || order > 2 || !read_words(in, w, 12)) { fprintf(stderr, "touch_rule_driver: case %lu: bad query\n", cases); return 1; }
			float a[9];
			for (int k = 0; k < 9; k++) a[k] = as_float(w[k]);
			const uint32_t room = w[9], first = w[10], flags = w[11];
			std::vector<uint32_t> words(GUARD + room + GUARD, 0x7e7e7e7eu);
			Walk count = { nodes, tris, a, a + 3, a + 6, first, flags, rtk_touch_hoist(), order, false, nullptr, 0u, 0u, 0u, (uint32_t)cases * 2654435761u + 1u };
			Walk fill = { nodes, tris, a, a + 3, a + 6, first, flags, rtk_touch_hoist(), order, true, words.data() + GUARD, room, 0u, 0u, (uint32_t)cases * 40503u + 7u };
			rtk_touch_hoist_query(a, a + 3, a + 6, count.q);
			rtk_touch_hoist_query(a, a + 3, a + 6, fill.q);
			if (rtk_touch_live(a, a + 3, a + 6) && !nodes.empty() && !tris.empty()) {
				count.visit(0u);
				if (room) fill.visit(0u);
			}
			printf("%" PRIu32 " %" PRIu32, count.kept, fill.kept);
			for (uint32_t x : words) printf(" %08" PRIx32, x);
			printf("\n");
		} else { fprintf(stderr, "touch_rule_driver: case %lu: kind '%c'\n", cases, kind); return 1; }
		cases++;
	}
	if (in != stdin) fclose(in);
	printf("ok\n");
	return 0;
}
