// obb_rule_driver.cpp -- rtk_amd/csrc/rtk_obb_rule.h on the CPU: tests/test_obb_cpu.py builds this with the host compiler,
// -ffp-contract=off as the library is built, and the address and undefined-behaviour sanitizers, against the rule headers alone.
//
//   obb_rule_driver -b IN OUT   IN holds raw 32-bit words, 30 per case: v0[3] v1[3] v2[3] query[15] clo[3] chi[3]. OUT receives
//       7 words per case: the bits (bit 0 live by rtk_obb_prepare, bit 1 rtk_box_boxes_touch against [qlo, qhi], bit 2
//       rtk_obb_separated, bit 3 rtk_obb_skip(clo, chi)), then qlo[3] and qhi[3]. The candidate of rule 3 is bits 0 and 1
//       without bit 2, and the driver ends with status 1 if rtk_obb_candidate says otherwise. Prints "ok".
//   obb_rule_driver FILE        reads text cases; every number after the case letter and the decimal counts is the hexadecimal bits
//       of a 32-bit word:
//     n count   then count nodes of 28 words: xlo[4] xhi[4] ylo[4] yhi[4] zlo[4] zhi[4] child[4]   (replaces the tree)
//         a child word: 0xffffffff empty, bit 31 set: a leaf whose records begin at slot (word & 0x7fffffff), else a node index
//     t count   then count triangle records of 11 words: a[3] b[3] c[3] prim last (non-zero: the leaf's run ends here)
//     q order   then 16 words: query[15] room
//         a host walk of the tree from node 0 with rtk_obb_prepare / rtk_obb_skip / rtk_obb_candidate / rtk_box_insert; the
//         children of a node are visited in slot order (order 0), in reverse slot order (1) or in an order drawn per node (2).
//         The count is a walk of its own; the fill goes into a segment of `room` entries between GUARD entries of 0x7e.
//         prints: count, kept, the GUARD + room + GUARD words
// one line of output per q case; "ok" at the end. A line it cannot read ends the run with status 1.
#include "rtk_obb_rule.h"

#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

struct Node { float box[6][4]; uint32_t child[4]; };
struct Tri { float a[3], b[3], c[3]; uint32_t prim, last; };

static const uint32_t GUARD = 4, NONE = 0xffffffffu;

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
	const rtk_obb_prepared &Q;
	int order;
	bool fill;
	uint32_t *seg;
	uint32_t room, kept, worst, rnd;

	void leaf(uint32_t slot)
	{
		while (slot < tris.size()) {
			const Tri &t = tris[slot];
			if (rtk_obb_candidate(Q, true, t.a, t.b, t.c)) {
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
			if (n.child[k] == NONE || rtk_obb_skip(Q, clo, chi)) continue;
			visit(n.child[k]);
		}
	}
};

static int bulk(const char *path, const char *out_path)
{
	FILE *in = fopen(path, "rb"), *out = fopen(out_path, "wb");
	if (!in || !out) { fprintf(stderr, "obb_rule_driver: cannot open %s or %s\n", path, out_path); return 1; }
	uint32_t w[30];
	unsigned long cases = 0;
	while (fread(w, sizeof(uint32_t), 30, in) == 30) {
		float f[30];
		for (int k = 0; k < 30; k++) f[k] = as_float(w[k]);
		const float *v0 = f, *v1 = f + 3, *v2 = f + 6, *q = f + 9, *clo = f + 24, *chi = f + 27;
		rtk_obb_prepared Q;
		const bool live = rtk_obb_prepare(q, Q), touch = rtk_box_boxes_touch(v0, v1, v2, Q.qlo, Q.qhi), sep = rtk_obb_separated(Q, v0, v1, v2);
		const bool skip = rtk_obb_skip(Q, clo, chi);
		if (rtk_obb_candidate(Q, live, v0, v1, v2) != (live && touch && !sep)) { fprintf(stderr, "obb_rule_driver: case %lu: rtk_obb_candidate is not rule 3\n", cases); return 1; }
		uint32_t o[7] = { (live ? 1u : 0u) | (touch ? 2u : 0u) | (sep ? 4u : 0u) | (skip ? 8u : 0u) };
		for (int k = 0; k < 3; k++) { o[1 + k] = as_word(Q.qlo[k]); o[4 + k] = as_word(Q.qhi[k]); }
		if (fwrite(o, sizeof(uint32_t), 7, out) != 7) { fprintf(stderr, "obb_rule_driver: cannot write\n"); return 1; }
		cases++;
	}
	fclose(in);
	if (fclose(out) != 0) return 1;
	printf("ok\n");
	return 0;
}

int main(int argc, char **argv)
{
	if (argc > 3 && strcmp(argv[1], "-b") == 0) return bulk(argv[2], argv[3]);
	FILE *in = argc > 1 ? fopen(argv[1], "r") : stdin;
	if (!in) { fprintf(stderr, "obb_rule_driver: cannot open %s\n", argv[1]); return 1; }
	std::vector<Node> nodes;
	std::vector<Tri> tris;
	char kind;
	unsigned long cases = 0;
	while (fscanf(in, " %c", &kind) == 1) {
		if (kind == 'n' || kind == 't') {
			unsigned count;
			if (fscanf(in, "%u", &count) != 1) { fprintf(stderr, "obb_rule_driver: case %lu: bad count\n", cases); return 1; }
			if (kind == 'n') {
				nodes.assign(count, Node());
				for (Node &nd : nodes) {
					uint32_t w[28];
					if (!read_words(in, w, 28)) { fprintf(stderr, "obb_rule_driver: case %lu: bad node\n", cases); return 1; }
					for (int r = 0; r < 6; r++) for (int k = 0; k < 4; k++) nd.box[r][k] = as_float(w[r * 4 + k]);
					for (int k = 0; k < 4; k++) nd.child[k] = w[24 + k];
				}
			} else {
				tris.assign(count, Tri());
				for (Tri &t : tris) {
					uint32_t w[11];
					if (!read_words(in, w, 11)) { fprintf(stderr, "obb_rule_driver: case %lu: bad triangle\n", cases); return 1; }
					for (int k = 0; k < 3; k++) { t.a[k] = as_float(w[k]); t.b[k] = as_float(w[3 + k]); t.c[k] = as_float(w[6 + k]); }
					t.prim = w[9]; t.last = w[10];
				}
			}
		} else if (kind == 'q') {
			int order;
			uint32_t w[16];
			if (fscanf(in, "%d", &order) != 1 || order < 0 || order > 2 || !read_words(in, w, 16)) { fprintf(stderr, "obb_rule_driver: case %lu: bad query\n", cases); return 1; }
			float q[15];
			for (int k = 0; k < 15; k++) q[k] = as_float(w[k]);
			const uint32_t room = w[15];
			std::vector<uint32_t> words(GUARD + room + GUARD, 0x7e7e7e7eu);
			rtk_obb_prepared Q;
			const bool live = rtk_obb_prepare(q, Q);
			Walk count = { nodes, tris, Q, order, false, nullptr, 0u, 0u, 0u, (uint32_t)cases * 2654435761u + 1u };
			Walk fill = { nodes, tris, Q, order, true, words.data() + GUARD, room, 0u, 0u, (uint32_t)cases * 40503u + 7u };
			if (live && !nodes.empty() && !tris.empty()) {
				count.visit(0u);
				if (room) fill.visit(0u);
			}
			printf("%" PRIu32 " %" PRIu32, count.kept, fill.kept);
			for (uint32_t x : words) printf(" %08" PRIx32, x);
			printf("\n");
		} else { fprintf(stderr, "obb_rule_driver: case %lu: kind '%c'\n", cases, kind); return 1; }
		cases++;
	}
	if (in != stdin) fclose(in);
	printf("ok\n");
	return 0;
}
