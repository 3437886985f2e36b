// within_rule_driver.cpp -- rtk_amd/csrc/rtk_within_rule.h (and rtk_closest_rule.h below it) on the CPU: tests/test_within_cpu.py
// builds this with the host compiler, -ffp-contract=off as the library is built, and the address and undefined-behaviour
// sanitizers, against those two headers alone.
//
// Reads cases from the file named on the command line (or stdin); every number after the case letter and the decimal counts is
// the hexadecimal bits of a 32-bit word:
//     i room n  then n candidates of 7 words: dist2 u v prim q0 q1 q2
//         the insertion alone: every candidate goes through rtk_within_insert, in the order given, into a segment of `room`
//         entries that stands between GUARD entries filled with 0x7e on either side; then once more into a segment that is an
//         allocation of exactly `room` entries (what the address sanitizer watches), and both must agree.
//         prints: kept, the (GUARD + room + GUARD) * 4 record words, the (GUARD + room + GUARD) * 3 point words
//     n count   then count nodes of 28 words: xlo[4] xhi[4] ylo[4] yhi[4] zlo[4] zhi[4] child[4]   (replaces the tree)
//         a child word: 0xffffffff empty, bit 31 set: a leaf whose records begin at slot (word & 0x7fffffff), else a node index
//     t count   then count triangle records of 11 words: a[3] b[3] c[3] prim last (non-zero: the leaf's run ends here)
//     q order   then 5 words: p0 p1 p2 max_dist2 room
//         a host walk of the tree from node 0 with rtk_within_live / rtk_closest_box_bound / rtk_within_skip /
//         rtk_closest_triangle / rtk_within_candidate / rtk_within_insert; the children of a node are visited in slot order
//         (order 0), in reverse slot order (1) or nearest bound first (2). The count is a walk of its own with a segment that
//         is never full.
//         prints: count, kept, and the words of the guarded segment as for i
// one line of output per i and q case; "ok" at the end. A line it cannot read ends the run with status 1.
#include "rtk_closest_rule.h"
#include "rtk_within_rule.h"

#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

struct Rec { float dist2, u, v; uint32_t prim; };
struct Node { float box[6][4]; uint32_t child[4]; };
struct Tri { float a[3], b[3], c[3]; uint32_t prim, last; };

static const uint32_t GUARD = 4, NONE = 0xffffffffu;

static float as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static bool read_words(FILE *in, uint32_t *w, size_t n)
{
	for (size_t k = 0; k < n; k++) if (fscanf(in, "%" SCNx32, &w[k]) != 1) return false;
	return true;
}

// a segment of `room` entries between guards
struct Guarded {
	uint32_t room;
	std::vector<Rec> rec;
	std::vector<float> pts;
	explicit Guarded(uint32_t room_) : room(room_), rec(GUARD + room_ + GUARD), pts((size_t)(GUARD + room_ + GUARD) * 3u)
	{
		memset(rec.data(), 0x7e, rec.size() * sizeof(Rec));
		memset(pts.data(), 0x7e, pts.size() * sizeof(float));
	}
	Rec *seg() { return rec.data() + GUARD; }
	float *seg_points() { return pts.data() + (size_t)GUARD * 3u; }
	void print() const
	{
		for (const Rec &r : rec) printf(" %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32, bits_of(r.dist2), bits_of(r.u), bits_of(r.v), r.prim);
		for (float f : pts) printf(" %08" PRIx32, bits_of(f));
		printf("\n");
	}
};

struct Walk {
	const std::vector<Node> &nodes;
	const std::vector<Tri> &tris;
	const float *p;
	float max2;
	int order;
	bool fill;
	Rec *seg;
	float *seg_points;
	uint32_t room, kept;
	Rec worst;

	void leaf(uint32_t slot)
	{
		while (slot < tris.size()) {
			const Tri &t = tris[slot];
			float q[3], u, v;
			int region;
			const float dist2 = rtk_closest_triangle(p, t.a, t.b, t.c, q, u, v, region);
			if (rtk_within_candidate(dist2, max2)) {
				const Rec cand = { dist2, u, v, t.prim };
				if (fill) kept = rtk_within_insert(seg, seg_points, room, kept, cand, q, worst);
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
		float bound[4];
		int at[4] = { 0, 1, 2, 3 };
		for (int k = 0; k < 4; k++) {
			const float lo[3] = { n.box[0][k], n.box[2][k], n.box[4][k] }, hi[3] = { n.box[1][k], n.box[3][k], n.box[5][k] };
			bound[k] = rtk_closest_box_bound(p, lo, hi);
		}
		if (order == 1) { at[0] = 3; at[1] = 2; at[2] = 1; at[3] = 0; }
		if (order == 2) {
			for (int i = 1; i < 4; i++) for (int j = i; j > 0 && bound[at[j]] < bound[at[j - 1]]; j--) { const int s = at[j]; at[j] = at[j - 1]; at[j - 1] = s; }
		}
		for (int i = 0; i < 4; i++) {
			const int k = at[i];
			// (looked at when the child's turn comes: the segment may have filled up since the node was entered)
			if (n.child[k] == NONE || rtk_within_skip(bound[k], max2, fill && kept == room, worst.dist2)) continue;
			visit(n.child[k]);
		}
	}
};

int main(int argc, char **argv)
{
	FILE *in = argc > 1 ? fopen(argv[1], "r") : stdin;
	if (!in) { fprintf(stderr, "within_rule_driver: cannot open %s\n", argv[1]); return 1; }
	std::vector<Node> nodes;
	std::vector<Tri> tris;
	char kind;
	unsigned long cases = 0;
	while (fscanf(in, " %c", &kind) == 1) {
		if (kind == 'i') {
			unsigned room, n;
			if (fscanf(in, "%u %u", &room, &n) != 2) { fprintf(stderr, "within_rule_driver: case %lu: bad counts\n", cases); return 1; }
			Guarded g(room);
			Rec *exact = room ? static_cast<Rec *>(malloc((size_t)room * sizeof(Rec))) : nullptr;
			float *exact_points = room ? static_cast<float *>(malloc((size_t)room * 3u * sizeof(float))) : nullptr;
			uint32_t kept = 0, kept2 = 0, kept3 = 0;
			Rec worst = { 0.0f, 0.0f, 0.0f, 0u }, worst2 = worst, worst3 = worst;
			std::vector<Rec> no_points(room);
			for (unsigned k = 0; k < n; k++) {
				uint32_t w[7];
				if (!read_words(in, w, 7)) { fprintf(stderr, "within_rule_driver: case %lu: bad candidate %u\n", cases, k); return 1; }
				const Rec cand = { as_float(w[0]), as_float(w[1]), as_float(w[2]), w[3] };
				const float q[3] = { as_float(w[4]), as_float(w[5]), as_float(w[6]) };
				kept = rtk_within_insert(g.seg(), g.seg_points(), room, kept, cand, q, worst);
				kept2 = rtk_within_insert(exact, exact_points, room, kept2, cand, q, worst2);
				kept3 = rtk_within_insert(no_points.data(), (float *)nullptr, room, kept3, cand, q, worst3);       // (no points: records alone)
			}
			bool same = kept == kept2 && kept == kept3 && kept <= room;
			if (kept) same = same && memcmp(g.seg(), exact, (size_t)kept * sizeof(Rec)) == 0 && memcmp(g.seg_points(), exact_points, (size_t)kept * 3u * sizeof(float)) == 0 &&
				memcmp(g.seg(), no_points.data(), (size_t)kept * sizeof(Rec)) == 0;
			if (kept == room && room) same = same && memcmp(&worst, g.seg() + (room - 1u), sizeof(Rec)) == 0;
			free(exact); free(exact_points);
			if (!same) { fprintf(stderr, "within_rule_driver: case %lu: the three segments differ, or worst is not the last entry\n", cases); return 1; }
			printf("%" PRIu32, kept);
			g.print();
		} else if (kind == 'n' || kind == 't') {
			unsigned count;
			if (fscanf(in, "%u", &count) != 1) { fprintf(stderr, "within_rule_driver: case %lu: bad count\n", cases); return 1; }
			if (kind == 'n') {
				nodes.assign(count, Node());
				for (Node &nd : nodes) {
					uint32_t w[28];
					if (!read_words(in, w, 28)) { fprintf(stderr, "within_rule_driver: case %lu: bad node\n", cases); return 1; }
					for (int r = 0; r < 6; r++) for (int k = 0; k < 4; k++) nd.box[r][k] = as_float(w[r * 4 + k]);
					for (int k = 0; k < 4; k++) nd.child[k] = w[24 + k];
				}
			} else {
				tris.assign(count, Tri());
				for (Tri &t : tris) {
					uint32_t w[11];
					if (!read_words(in, w, 11)) { fprintf(stderr, "within_rule_driver: case %lu: bad triangle\n", cases); return 1; }
					for (int k = 0; k < 3; k++) { t.a[k] = as_float(w[k]); t.b[k] = as_float(w[3 + k]); t.c[k] = as_float(w[6 + k]); }
					t.prim = w[9]; t.last = w[10];
				}
			}
		} else if (kind == 'q') {
			int order;
			uint32_t w[5];
			if (fscanf(in, "%d", &order) != 1 || order < 0 || order > 2 || !read_words(in, w, 5)) { fprintf(stderr, "within_rule_driver: case %lu: bad query\n", cases); return 1; }
			const float p[3] = { as_float(w[0]), as_float(w[1]), as_float(w[2]) };
			const float max2 = as_float(w[3]);
			const uint32_t room = w[4];
			Guarded g(room);
			const Rec none = { 0.0f, 0.0f, 0.0f, 0u };
			Walk count = { nodes, tris, p, max2, order, false, nullptr, nullptr, 0u, 0u, none };
			Walk fill = { nodes, tris, p, max2, order, true, g.seg(), g.seg_points(), room, 0u, none };
			if (rtk_within_live(p, max2) && !nodes.empty() && !tris.empty()) {
				count.visit(0u);
				if (room) fill.visit(0u);
			}
			printf("%" PRIu32 " %" PRIu32, count.kept, fill.kept);
			g.print();
		} else { fprintf(stderr, "within_rule_driver: case %lu: kind '%c'\n", cases, kind); return 1; }
		cases++;
	}
	if (in != stdin) fclose(in);
	printf("ok\n");
	return 0;
}
