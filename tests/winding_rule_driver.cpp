// winding_rule_driver.cpp -- rtk_amd/csrc/rtk_winding_rule.h on the CPU (tests/test_winding_cpu.py builds this with the host
// compiler, -ffp-contract=off as the library is built, once plain and once with the address and undefined-behaviour sanitizers,
// against that header alone).
//
// Reads the file named on the command line (or stdin); every float is the hexadecimal bits of a 32-bit word:
//     t p0 p1 p2 a0 a1 a2 b0 b1 b2 c0 c1 c2      rtk_winding_triangle: prints its bits
//     f p0 p1 p2 N0 N1 N2 P0 P1 P2               rtk_winding_far: prints its bits
//     c r2 beta R                                rtk_winding_accept: prints 0 or 1
//     m a0 a1 a2 b0 b1 b2 c0 c1 c2               rtk_winding_tri_moments: prints 7 words
//     s s0 .. s6 lo0 lo1 lo2 hi0 hi1 hi2         rtk_winding_slot: prints 7 words (N, P, R)
//     w T                                        a mesh of T records follows, one per line as a0 a1 a2 b0 b1 b2 c0 c1 c2
//     q p0 p1 p2                                 the sum of the triangle terms of the last mesh in row order from +0: prints its bits
// "ok" at the end. A line it cannot read ends the run with status 1.
#include "rtk_winding_rule.h"

#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <vector>

static float as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static bool read_words(FILE *in, int n, float *f)
{
	for (int k = 0; k < n; k++) {
		uint32_t w;
		if (fscanf(in, "%" SCNx32, &w) != 1) return false;
		f[k] = as_float(w);
	}
	return true;
}

static void print_words(const float *f, int n)
{
	for (int k = 0; k < n; k++) printf("%08" PRIx32 "%c", bits_of(f[k]), k == n - 1 ? '\n' : ' ');
}

int main(int argc, char **argv)
{
	FILE *in = argc > 1 ? fopen(argv[1], "r") : stdin;
	if (!in) { fprintf(stderr, "winding_rule_driver: cannot open %s\n", argv[1]); return 1; }
	std::vector<float> mesh;       // 9 per record
	char kind;
	unsigned long cases = 0;
	while (fscanf(in, " %c", &kind) == 1) {
		float f[13], out[7];
		bool ok = true;
		if (kind == 't') {
			if ((ok = read_words(in, 12, f))) { out[0] = rtk_winding_triangle(f, f + 3, f + 6, f + 9); print_words(out, 1); }
		} else if (kind == 'f') {
			if ((ok = read_words(in, 9, f))) { out[0] = rtk_winding_far(f, f + 3, f + 6); print_words(out, 1); }
		} else if (kind == 'c') {
			if ((ok = read_words(in, 3, f))) printf("%d\n", rtk_winding_accept(f[0], f[1], f[2]) ? 1 : 0);
		} else if (kind == 'm') {
			if ((ok = read_words(in, 9, f))) { rtk_winding_tri_moments(f, f + 3, f + 6, out); print_words(out, 7); }
		} else if (kind == 's') {
			if ((ok = read_words(in, 13, f))) { rtk_winding_slot(f, f + 7, f + 10, out); print_words(out, 7); }
		} else if (kind == 'w') {
			unsigned long T;
			if (fscanf(in, "%lu", &T) != 1) { fprintf(stderr, "winding_rule_driver: case %lu: bad count\n", cases); return 1; }
			mesh.clear();
			for (unsigned long t = 0; ok && t < T; t++) {
				if ((ok = read_words(in, 9, f))) mesh.insert(mesh.end(), f, f + 9);
			}
		} else if (kind == 'q') {
			if ((ok = read_words(in, 3, f))) {
				float w = 0.0f;
				for (size_t t = 0; t < mesh.size() / 9; t++) {
					const float *r = &mesh[9 * t];
					w = RTK_CL_ADD(w, rtk_winding_triangle(f, r, r + 3, r + 6));
				}
				print_words(&w, 1);
			}
		} else { fprintf(stderr, "winding_rule_driver: case %lu: kind '%c'\n", cases, kind); return 1; }
		if (!ok) { fprintf(stderr, "winding_rule_driver: case %lu: bad word\n", cases); return 1; }
		cases++;
	}
	if (in != stdin) fclose(in);
	printf("ok\n");
	return 0;
}
