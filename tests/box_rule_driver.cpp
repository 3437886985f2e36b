// box_rule_driver.cpp -- rtk_amd/csrc/rtk_box_rule.h on the CPU: tests/test_box_cpu.py builds this with the host compiler,
// -ffp-contract=off as the library is built, and the address and undefined-behaviour sanitizers, against the rule headers alone.
//
//   box_rule_driver -b FILE     FILE holds raw 32-bit words, 21 per case: v0[3] v1[3] v2[3] lo[3] hi[3] clo[3] chi[3]. Prints one
//       hexadecimal digit per case on one line: bit 0 rtk_box_live(lo, hi), bit 1 rtk_box_boxes_touch, bit 2 rtk_box_separated
//       (about rtk_box_centre(lo, hi)), bit 3 rtk_box_skip(clo, chi, lo, hi); the candidate of rule 4 is bits 0 and 1 without
//       bit 2, and the driver ends with status 1 if rtk_box_candidate says otherwise. Then "ok".
//   box_rule_driver FILE        reads text cases; every number after the case letter and the decimal counts is the hexadecimal bits
//       of a 32-bit word:
//     i room n  then n ids
//         the insertion alone: every id goes through rtk_box_insert, in the order given, into a segment of `room` entries that
//         stands between GUARD entries filled with 0x7e on either side; then once more into a segment that is an allocation of
//         exactly `room` entries (what the address sanitizer watches), and both must agree.
//         prints: kept, the GUARD + room + GUARD words
//     n count   then count nodes of 28 words: xlo[4] xhi[4] ylo[4] yhi[4] zlo[4] zhi[4] child[4]   (replaces the tree)
//         a child word: 0xffffffff empty, bit 31 set: a leaf whose records begin at slot (word & 0x7fffffff), else a node index
//     t count   then count triangle records of 11 words: a[3] b[3] c[3] prim last (non-zero: the leaf's run ends here)
//     q order   then 7 words: lo[3] hi[3] room
//         a host walk of the tree from node 0 with rtk_box_live / rtk_box_skip / rtk_box_candidate / rtk_box_insert; the children
//         of a node are visited in slot order (order 0), in reverse slot order (1) or in an order drawn per node (2). The count
//         is a walk of its own.
//         prints: count, kept, and the words of the guarded segment as for i
// one line of output per i and q case; "ok" at the end. A line it cannot read ends the run with status 1.
#include "rtk_box_rule.h"

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

// a segment of `room` entries between guards
struct Guarded {
	uint32_t room;
	std::vector<uint32_t> words;
	explicit Guarded(uint32_t room_) : room(room_), words(GUARD + room_ + GUARD, 0x7e7e7e7eu) {}
	uint32_t *seg() { return words.data() + GUARD; }
	void print() const
	{
		for (uint32_t w : words) printf(" %08" PRIx32, w);
		printf("\n");
	}
};

struct Walk {
	const std::vector<Node> &nodes;
	const std::vector<Tri> &tris;
	const float *lo, *hi;
	float c[3], h[3];
	int order;
	bool fill;
	uint32_t *seg;
	uint32_t room, kept, worst, rnd;

	void leaf(uint32_t slot)
	{
		while (slot < tris.size()) {
			const Tri &t = tris[slot];
			if (rtk_box_candidate(t.a, t.b, t.c, lo, hi, c, h)) {
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
			if (n.child[k] == NONE || rtk_box_skip(clo, chi, lo, hi)) continue;
			visit(n.child[k]);
		}
	}
};

static int bulk(const char *path)
{
	FILE *in = fopen(path, "rb");
	if (!in) { fprintf(stderr, "box_rule_driver: cannot open %s\n", path); return 1; }
	uint32_t w[21];
	unsigned long cases = 0;
	while (fread(w, sizeof(uint32_t), 21, in) == 21) {
		float f[21], c[3], h[3];
		for (int k = 0; k < 21; k++) f[k] = as_float(w[k]);
		const float *v0 = f, *v1 = f + 3, *v2 = f + 6, *lo = f + 9, *hi = f + 12, *clo = f + 15, *chi = f + 18;
		rtk_box_centre(lo, hi, c, h);
		const bool live = rtk_box_live(lo, hi), touch = rtk_box_boxes_touch(v0, v1, v2, lo, hi), sep = rtk_box_separated(v0, v1, v2, c, h);
		const bool skip = rtk_box_skip(clo, chi, lo, hi);
		if (rtk_box_candidate(v0, v1, v2, lo, hi, c, h) != (touch && !sep)) { fprintf(stderr, "box_rule_driver: case %lu: rtk_box_candidate is not rule 4\n", cases); return 1; }
		putchar("0123456789abcdef"[(live ? 1 : 0) | (touch ? 2 : 0) | (sep ? 4 : 0) | (skip ? 8 : 0)]);
		cases++;
	}
	fclose(in);
	printf("\nok\n");
	return 0;
}

int main(int argc, char **argv)
{
	if (argc > 2 && strcmp(argv[1], "-b") == 0) return bulk(argv[2]);
	FILE *in = argc > 1 ? fopen(argv[1], "r") : stdin;
	if (!in) { fprintf(stderr, "box_rule_driver: cannot open %s\n", argv[1]); return 1; }
	std::vector<Node> nodes;
	std::vector<Tri> tris;
	char kind;
	unsigned long cases = 0;
	while (fscanf(in, " %c", &kind) == 1) {
		if (kind == 'i') {
			unsigned room, n;
			if (fscanf(in, "%u %u", &room, &n) != 2) { fprintf(stderr, "box_rule_driver: case %lu: bad counts\n", cases); return 1; }
			Guarded g(room);
			uint32_t *exact = room ? static_cast<uint32_t *>(malloc((size_t)room * sizeof(uint32_t))) : nullptr;
			uint32_t kept = 0, kept2 = 0, worst = 0, worst2 = 0;
			for (unsigned k = 0; k < n; k++) {
				uint32_t prim;
				if (!read_words(in, &prim, 1)) { fprintf(stderr, "box_rule_driver: case %lu: bad id %u\n", cases, k); return 1; }
				kept = rtk_box_insert(g.seg(), room, kept, prim, worst);
				kept2 = rtk_box_insert(exact, room, kept2, prim, worst2);
			}
			bool same = kept == kept2 && kept <= room;
			if (kept) same = same && memcmp(g.seg(), exact, (size_t)kept * sizeof(uint32_t)) == 0;
			if (kept == room && room) same = same && worst == g.seg()[room - 1u] && worst2 == worst;
			free(exact);
			if (!same) { fprintf(stderr, "box_rule_driver: case %lu: the two segments differ, or worst is not the last entry\n", cases); return 1; }
			printf("%" PRIu32, kept);
			g.print();
		} else if (kind == 'n' || kind == 't') {
			unsigned count;
			if (fscanf(in, "%u", &count) != 1) { fprintf(stderr, "box_rule_driver: case %lu: bad count\n", cases); return 1; }
			if (kind == 'n') {
				nodes.assign(count, Node());
				for (Node &nd : nodes) {
					uint32_t w[28];
					if (!read_words(in, w, 28)) { fprintf(stderr, "box_rule_driver: case %lu: bad node\n", cases); return 1; }
					for (int r = 0; r < 6; r++) for (int k = 0; k < 4; k++) nd.box[r][k] = as_float(w[r * 4 + k]);
					for (int k = 0; k < 4; k++) nd.child[k] = w[24 + k];
				}
			} else {
				tris.assign(count, Tri());
				for (Tri &t : tris) {
					uint32_t w[11];
					if (!read_words(in, w, 11)) { fprintf(stderr, "box_rule_driver: case %lu: bad triangle\n", cases); return 1; }
					for (int k = 0; k < 3; k++) { t.a[k] = as_float(w[k]); t.b[k] = as_float(w[3 + k]); t.c[k] = as_float(w[6 + k]); }
					t.prim = w[9]; t.last = w[10];
				}
			}
		} else if (kind == 'q') {
			int order;
			uint32_t w[7];
			if (fscanf(in, "%d", &order) != 1 || order < 0 || order > 2 || !read_words(in, w, 7)) { fprintf(stderr, "box_rule_driver: case %lu: bad query\n", cases); return 1; }
			const float lo[3] = { as_float(w[0]), as_float(w[1]), as_float(w[2]) }, hi[3] = { as_float(w[3]), as_float(w[4]), as_float(w[5]) };
			const uint32_t room = w[6];
			Guarded g(room);
			Walk count = { nodes, tris, lo, hi, { 0, 0, 0 }, { 0, 0, 0 }, order, false, nullptr, 0u, 0u, 0u, (uint32_t)cases * 2654435761u + 1u };
			Walk fill = { nodes, tris, lo, hi, { 0, 0, 0 }, { 0, 0, 0 }, order, true, g.seg(), room, 0u, 0u, (uint32_t)cases * 40503u + 7u };
			rtk_box_centre(lo, hi, count.c, count.h);
			rtk_box_centre(lo, hi, fill.c, fill.h);
			if (rtk_box_live(lo, hi) && !nodes.empty() && !tris.empty()) {
				count.visit(0u);
				if (room) fill.visit(0u);
			}
			printf("%" PRIu32 " %" PRIu32, count.kept, fill.kept);
			g.print();
		} else { fprintf(stderr, "box_rule_driver: case %lu: kind '%c'\n", cases, kind); return 1; }
		cases++;
	}
	if (in != stdin) fclose(in);
	printf("ok\n");
	return 0;
}
