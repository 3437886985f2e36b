// near_rule_driver.cpp -- rtk_amd/csrc/rtk_near_rule.h (and rtk_pair_rule.h below it) on the CPU: tests/test_near_cpu.py builds
// this with the host compiler, -ffp-contract=off as the library is built, and the address and undefined-behaviour sanitizers,
// against the rule headers alone.
//
// Reads cases from the file named on the command line (or stdin); every number after the case letter and the decimal counts is
// the hexadecimal bits of a 32-bit word:
//     i room n  then n candidates of 10 words: dist2 u v prim qa[3] qb[3]
//         the insertion alone: every candidate goes through rtk_near_insert, in the order given, into a segment of `room`
//         entries that stands between GUARD entries filled with 0x7e on either side; then once more into a segment that is an
//         allocation of exactly `room` entries (what the address sanitizer watches), once with the first point array alone,
//         once with the second alone and once with none; all must agree, and whenever the segment is full `worst` must be its
//         last entry.
//         prints: kept, the (GUARD + room + GUARD) * 4 record words, then as many * 3 words of either point array
//     s         then 4 words: bound max_dist2 full worst2.   prints rtk_near_skip as 0 or 1
//     n count   then count nodes of 28 words: xlo[4] xhi[4] ylo[4] yhi[4] zlo[4] zhi[4] child[4]   (replaces the tree)
//         a child word: 0xffffffff empty, bit 31 set: a leaf whose records begin at slot (word & 0x7fffffff), else a node index
//     t count   then count triangle records of 11 words: a[3] b[3] c[3] prim last (non-zero: the leaf's run ends here)
//     q order   then 13 words: a0[3] a1[3] a2[3] max_dist2 first_prim flags room
//         a host walk of the tree from node 0 with rtk_touch_live / rtk_pair_box_bound / rtk_near_skip / rtk_touch_filter_passes /
//         rtk_pair_evaluate / rtk_near_candidate / rtk_near_insert; the children of a node are visited in slot order (order 0),
//         in reverse slot order (1), in an order drawn per node (2) or nearest bound first (3). A record whose own box is skipped
//         is not evaluated. The count is a walk of its own with a segment that is never full.
//         prints: count, kept, the records the fill walk evaluated (decimal), and the words of the guarded segment as for i
// one line of output per i, s and q case; "ok" at the end. A line it cannot read ends the run with status 1.
#include "rtk_near_rule.h"

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
	std::vector<float> pa, pb;
	explicit Guarded(uint32_t room_) : room(room_), rec(GUARD + room_ + GUARD), pa((size_t)(GUARD + room_ + GUARD) * 3u), pb(pa.size())
	{
		memset(rec.data(), 0x7e, rec.size() * sizeof(Rec));
		memset(pa.data(), 0x7e, pa.size() * sizeof(float));
		memset(pb.data(), 0x7e, pb.size() * sizeof(float));
	}
	Rec *seg() { return rec.data() + GUARD; }
	float *seg_qa() { return pa.data() + (size_t)GUARD * 3u; }
	float *seg_qb() { return pb.data() + (size_t)GUARD * 3u; }
	void print() const
	{
		for (const Rec &r : rec) printf(" %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32, bits_of(r.dist2), bits_of(r.u), bits_of(r.v), r.prim);
		for (float f : pa) printf(" %08" PRIx32, bits_of(f));
		for (float f : pb) printf(" %08" PRIx32, bits_of(f));
		printf("\n");
	}
};

struct Walk {
	const std::vector<Node> &nodes;
	const std::vector<Tri> &tris;
	const float *a0, *a1, *a2;
	float max2;
	uint32_t first, flags;
	rtk_pair_hoist h;
	int order;
	uint32_t rnd;
	bool fill;
	Rec *seg;
	float *seg_qa, *seg_qb;
	uint32_t room, kept;
	Rec worst;
	unsigned long evaluated;

	void leaf(uint32_t slot)
	{
		while (slot < tris.size()) {
			const Tri &t = tris[slot];
			float lo[3], hi[3];
			rtk_pair_box(t.a, t.b, t.c, lo, hi);
			if (rtk_touch_filter_passes(t.prim, first, flags, a0, a1, a2, t.a, t.b, t.c)
				&& !rtk_near_skip(rtk_pair_box_bound(lo, hi, h.lo, h.hi), max2, fill && kept == room, worst.dist2)) {
				rtk_pair_result r;
				rtk_pair_evaluate(h, t.a, t.b, t.c, r);
				evaluated++;
				if (rtk_near_candidate(r.dist2, max2)) {
					const Rec cand = { r.dist2, r.u, r.v, t.prim };
					if (fill) {
						kept = rtk_near_insert(seg, seg_qa, seg_qb, room, kept, cand, r.qa, r.qb, worst);
						if (kept == room && memcmp(&worst, seg + (room - 1u), sizeof(Rec)) != 0) { fprintf(stderr, "near_rule_driver: worst is not the last entry\n"); exit(1); }
					} else kept++;
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
			// (looked at when the child's turn comes: the segment may have filled up since the node was entered)
			if (n.child[k] == NONE || rtk_near_skip(bound[k], max2, fill && kept == room, worst.dist2)) continue;
			visit(n.child[k]);
		}
	}
};

int main(int argc, char **argv)
{
	FILE *in = argc > 1 ? fopen(argv[1], "r") : stdin;
	if (!in) { fprintf(stderr, "near_rule_driver: cannot open %s\n", argv[1]); return 1; }
	std::vector<Node> nodes;
	std::vector<Tri> tris;
	char kind;
	unsigned long cases = 0;
	while (fscanf(in, " %c", &kind) == 1) {
		if (kind == 'i') {
			unsigned room, n;
			if (fscanf(in, "%u %u", &room, &n) != 2) { fprintf(stderr, "near_rule_driver: case %lu: bad counts\n", cases); return 1; }
			Guarded g(room);
			Rec *exact = room ? static_cast<Rec *>(malloc((size_t)room * sizeof(Rec))) : nullptr;
			float *exact_qa = room ? static_cast<float *>(malloc((size_t)room * 3u * sizeof(float))) : nullptr;
			float *exact_qb = room ? static_cast<float *>(malloc((size_t)room * 3u * sizeof(float))) : nullptr;
			std::vector<Rec> only_a(room), only_b(room), none(room);
			std::vector<float> pts_a((size_t)room * 3u), pts_b((size_t)room * 3u);
			uint32_t kept[5] = { 0, 0, 0, 0, 0 };
			Rec worst[5] = {};
			bool same = true;
			for (unsigned k = 0; k < n; k++) {
				uint32_t w[10];
				if (!read_words(in, w, 10)) { fprintf(stderr, "near_rule_driver: case %lu: bad candidate %u\n", cases, k); return 1; }
				const Rec cand = { as_float(w[0]), as_float(w[1]), as_float(w[2]), w[3] };
				const float qa[3] = { as_float(w[4]), as_float(w[5]), as_float(w[6]) }, qb[3] = { as_float(w[7]), as_float(w[8]), as_float(w[9]) };
				kept[0] = rtk_near_insert(g.seg(), g.seg_qa(), g.seg_qb(), room, kept[0], cand, qa, qb, worst[0]);
				kept[1] = rtk_near_insert(exact, exact_qa, exact_qb, room, kept[1], cand, qa, qb, worst[1]);
				kept[2] = rtk_near_insert(only_a.data(), pts_a.data(), (float *)nullptr, room, kept[2], cand, qa, qb, worst[2]);
				kept[3] = rtk_near_insert(only_b.data(), (float *)nullptr, pts_b.data(), room, kept[3], cand, qa, qb, worst[3]);
				kept[4] = rtk_near_insert(none.data(), (float *)nullptr, (float *)nullptr, room, kept[4], cand, qa, qb, worst[4]);
				// worst is the segment's last entry after EVERY insertion into a full segment
				if (kept[0] == room && room) same = same && memcmp(&worst[0], g.seg() + (room - 1u), sizeof(Rec)) == 0;
			}
			for (int v = 1; v < 5; v++) same = same && kept[v] == kept[0];
			same = same && kept[0] <= room;
			if (kept[0]) {
				const size_t rb = (size_t)kept[0] * sizeof(Rec), pb = (size_t)kept[0] * 3u * sizeof(float);
				same = same && memcmp(g.seg(), exact, rb) == 0 && memcmp(g.seg(), only_a.data(), rb) == 0 && memcmp(g.seg(), only_b.data(), rb) == 0 &&
					memcmp(g.seg(), none.data(), rb) == 0 && memcmp(g.seg_qa(), exact_qa, pb) == 0 && memcmp(g.seg_qb(), exact_qb, pb) == 0 &&
					memcmp(g.seg_qa(), pts_a.data(), pb) == 0 && memcmp(g.seg_qb(), pts_b.data(), pb) == 0;
			}
			if (kept[0] == room && room) for (int v = 1; v < 5; v++) same = same && memcmp(&worst[v], &worst[0], sizeof(Rec)) == 0;
			free(exact); free(exact_qa); free(exact_qb);
			if (!same) { fprintf(stderr, "near_rule_driver: case %lu: the segments differ, or worst is not the last entry\n", cases); return 1; }
			printf("%" PRIu32, kept[0]);
			g.print();
		} else if (kind == 's') {
			uint32_t w[4];
			if (!read_words(in, w, 4)) { fprintf(stderr, "near_rule_driver: case %lu: bad skip case\n", cases); return 1; }
			printf("%d\n", rtk_near_skip(as_float(w[0]), as_float(w[1]), w[2] != 0u, as_float(w[3])) ? 1 : 0);
		} else if (kind == 'n' || kind == 't') {
			unsigned count;
			if (fscanf(in, "%u", &count) != 1) { fprintf(stderr, "near_rule_driver: case %lu: bad count\n", cases); return 1; }
			if (kind == 'n') {
				nodes.assign(count, Node());
				for (Node &nd : nodes) {
					uint32_t w[28];
					if (!read_words(in, w, 28)) { fprintf(stderr, "near_rule_driver: case %lu: bad node\n", cases); return 1; }
					for (int r = 0; r < 6; r++) for (int k = 0; k < 4; k++) nd.box[r][k] = as_float(w[r * 4 + k]);
					for (int k = 0; k < 4; k++) nd.child[k] = w[24 + k];
				}
			} else {
				tris.assign(count, Tri());
				for (Tri &t : tris) {
					uint32_t w[11];
					if (!read_words(in, w, 11)) { fprintf(stderr, "near_rule_driver: case %lu: bad triangle\n", cases); return 1; }
					for (int k = 0; k < 3; k++) { t.a[k] = as_float(w[k]); t.b[k] = as_float(w[3 + k]); t.c[k] = as_float(w[6 + k]); }
					t.prim = w[9]; t.last = w[10];
				}
			}
			continue;                                                 // (no output line)
		} else if (kind == 'q') {
			int order;
			uint32_t w[13];
			if (fscanf(in, "%d", &order) != 1 || order < 0 || order > 3 || !read_words(in, w, 13)) { fprintf(stderr, "near_rule_driver: case %lu: bad query\n", cases); return 1; }
			float a[9];
			for (int k = 0; k < 9; k++) a[k] = as_float(w[k]);
			const float max2 = as_float(w[9]);
			const uint32_t room = w[12];
			Guarded g(room);
			const Rec zero = { 0.0f, 0.0f, 0.0f, 0u };
			const uint32_t seed = (uint32_t)cases * 2654435761u + 1u;
			Walk count = { nodes, tris, a, a + 3, a + 6, max2, w[10], w[11], rtk_pair_hoist(), order, seed, false, nullptr, nullptr, nullptr, 0u, 0u, zero, 0ul };
			Walk fill = { nodes, tris, a, a + 3, a + 6, max2, w[10], w[11], rtk_pair_hoist(), order, seed, true, g.seg(), g.seg_qa(), g.seg_qb(), room, 0u, zero, 0ul };
			rtk_pair_hoist_query(a, a + 3, a + 6, count.h);
			rtk_pair_hoist_query(a, a + 3, a + 6, fill.h);
			if (rtk_touch_live(a, a + 3, a + 6) && max2 > 0.0f && !nodes.empty() && !tris.empty()) {
				count.visit(0u);
				if (room) fill.visit(0u);
			}
			printf("%" PRIu32 " %" PRIu32 " %lu", count.kept, fill.kept, fill.evaluated);
			g.print();
		} else { fprintf(stderr, "near_rule_driver: case %lu: kind '%c'\n", cases, kind); return 1; }
		cases++;
	}
	if (in != stdin) fclose(in);
	printf("ok\n");
	return 0;
}
