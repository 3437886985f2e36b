// sign_rule_driver.cpp -- rtk_amd/csrc/rtk_sign_rule.h on the CPU (tests/test_sign_cpu.py builds this with the host compiler,
// -ffp-contract=off as the library is built, and the address and undefined-behaviour sanitizers, against that header alone).
// The table is made here the plain way -- every corner compared with every earlier one, the sums taken in (prim, corner) order --
// with the header's functions for every float: what the device makes by sorting must equal it.
//
// Reads the file named on the command line (or stdin); every float is the hexadecimal bits of a 32-bit word:
//     a y x                     rtk_sign_angle(y, x): prints its bits
//     m T                       a mesh of T records follows, one per line as a0 a1 a2 b0 b1 b2 c0 c1 c2 (prim = its number):
//                               prints T lines of 18 words, the table, and then the line
//                               "info boundary nonmanifold inconsistent degenerate places" (decimal)
//     q p0 p1 p2 max_dist2      a query against the last mesh, answered by the closest rule over ALL records and given its sign:
//                               prints signed, dist2, prim (hexadecimal) and the region (decimal; 0 for a miss)
// "ok" at the end. A line it cannot read ends the run with status 1.
#include "rtk_sign_rule.h"

#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <vector>

static float as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

struct Mesh {
	std::vector<float> tris;       // 9 per record
	std::vector<float> table;      // 18 per record
	size_t size() const { return tris.size() / 9; }
};

static bool read_words(FILE *in, int n, float *f)
{
	for (int k = 0; k < n; k++) {
		uint32_t w;
		if (fscanf(in, "%" SCNx32, &w) != 1) return false;
		f[k] = as_float(w);
	}
	return true;
}

static void add_to(float *sum, bool &first, const float *x)
{
	if (first) { sum[0] = x[0]; sum[1] = x[1]; sum[2] = x[2]; first = false; }
	else { sum[0] = RTK_CL_ADD(sum[0], x[0]); sum[1] = RTK_CL_ADD(sum[1], x[1]); sum[2] = RTK_CL_ADD(sum[2], x[2]); }
}

static void make_table(Mesh &m, unsigned long long *info)
{
	const size_t T = m.size(), C = 3 * T;
	std::vector<size_t> place(C);                  // the first corner at the same place (itself: a place's first)
	std::vector<float> unit(3 * T), term(9 * T);
	std::vector<char> has(T);
	for (int k = 0; k < 5; k++) info[k] = 0;
	for (size_t t = 0; t < T; t++) {
		const float *r = &m.tris[9 * t];
		float n[3];
		has[t] = rtk_sign_unit_normal(r, r + 3, r + 6, n, &unit[3 * t]);
		if (has[t]) rtk_sign_corner_terms(r, r + 3, r + 6, &unit[3 * t], &term[9 * t]);
		else info[3]++;
	}
	for (size_t c = 0; c < C; c++) {
		place[c] = c;
		for (size_t d = 0; d < c; d++) if (rtk_sign_same_place(&m.tris[3 * c], &m.tris[3 * d])) { place[c] = place[d]; break; }
		if (place[c] == c) info[4]++;
	}
	m.table.assign(18 * T, 0.0f);
	for (size_t c = 0; c < C; c++) {
		float sum[3] = { 0.0f, 0.0f, 0.0f };
		bool first = true;
		for (size_t d = 0; d < C; d++) if (place[d] == place[c] && has[d / 3]) add_to(sum, first, &term[3 * d]);
		memcpy(&m.table[18 * (c / 3) + 9 + 3 * (c % 3)], sum, 12);
	}
	static const int ends[3][2] = { { 0, 1 }, { 0, 2 }, { 1, 2 } };
	for (size_t t = 0; t < T; t++) {
		for (int e = 0; e < 3; e++) {
			const size_t P = place[3 * t + ends[e][0]], Q = place[3 * t + ends[e][1]];
			float *dst = &m.table[18 * t + 3 * e];
			if (P == Q) { memcpy(dst, &m.table[18 * t + 9 + 3 * ends[e][0]], 12); continue; }
			float sum[3] = { 0.0f, 0.0f, 0.0f };
			bool first = true, other_forward = false;
			unsigned others = 0;
			for (size_t s = 0; s < T; s++) {
				int kp = -1, kq = -1;
				for (int k = 2; k >= 0; k--) { if (place[3 * s + k] == P) kp = k; if (place[3 * s + k] == Q) kq = k; }
				if (kp < 0 || kq < 0) continue;
				if (has[s]) add_to(sum, first, &unit[3 * s]);
				if (s != t) { others++; other_forward = rtk_sign_runs_forward(kp, kq); }
			}
			memcpy(dst, sum, 12);
			if (others == 0) info[0]++;
			else if (others >= 2) info[1]++;
			else if (other_forward == rtk_sign_runs_forward(ends[e][0], ends[e][1])) info[2]++;
		}
	}
}

int main(int argc, char **argv)
{
	FILE *in = argc > 1 ? fopen(argv[1], "r") : stdin;
	if (!in) { fprintf(stderr, "sign_rule_driver: cannot open %s\n", argv[1]); return 1; }
	Mesh mesh;
	char kind;
	unsigned long cases = 0;
	while (fscanf(in, " %c", &kind) == 1) {
		float f[9];
		if (kind == 'a') {
			if (!read_words(in, 2, f)) { fprintf(stderr, "sign_rule_driver: case %lu: bad word\n", cases); return 1; }
			printf("%08" PRIx32 "\n", bits_of(rtk_sign_angle(f[0], f[1])));
		} else if (kind == 'm') {
			unsigned long T;
			if (fscanf(in, "%lu", &T) != 1) { fprintf(stderr, "sign_rule_driver: case %lu: bad count\n", cases); return 1; }
			mesh.tris.clear();
			for (unsigned long t = 0; t < T; t++) {
				if (!read_words(in, 9, f)) { fprintf(stderr, "sign_rule_driver: case %lu: bad record %lu\n", cases, t); return 1; }
				mesh.tris.insert(mesh.tris.end(), f, f + 9);
			}
			unsigned long long info[5];
			make_table(mesh, info);
			for (unsigned long t = 0; t < T; t++) {
				for (int k = 0; k < 18; k++) printf("%08" PRIx32 "%c", bits_of(mesh.table[18 * t + k]), k == 17 ? '\n' : ' ');
			}
			printf("info %llu %llu %llu %llu %llu\n", info[0], info[1], info[2], info[3], info[4]);
		} else if (kind == 'q') {
			if (!read_words(in, 4, f)) { fprintf(stderr, "sign_rule_driver: case %lu: bad word\n", cases); return 1; }
			const float max2 = f[3];
			float best2 = max2;
			uint32_t best = 0xffffffffu;
			const bool live = max2 > 0.0f && f[0] - f[0] == 0.0f && f[1] - f[1] == 0.0f && f[2] - f[2] == 0.0f;
			for (size_t t = 0; live && t < mesh.size(); t++) {
				const float *r = &mesh.tris[9 * t];
				float q[3], u, v;
				int region;
				const float dist2 = rtk_closest_triangle(f, r, r + 3, r + 6, q, u, v, region);
				if (dist2 < max2 && rtk_closest_better(dist2, (uint32_t)t, best2, best)) { best2 = dist2; best = (uint32_t)t; }
			}
			float out = RTK_SIGN_INF;
			int region = 0;
			if (best != 0xffffffffu) {
				const float *r = &mesh.tris[9 * best];
				float q[3];
				out = rtk_sign_signed(f, r, r + 3, r + 6, &mesh.table[18 * best], q, region);
			}
			printf("%08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %d\n", bits_of(out), bits_of(best2), best, region);
		} else { fprintf(stderr, "sign_rule_driver: case %lu: kind '%c'\n", cases, kind); return 1; }
		cases++;
	}
	if (in != stdin) fclose(in);
	printf("ok\n");
	return 0;
}
