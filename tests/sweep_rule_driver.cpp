// sweep_rule_driver.cpp -- rtk_amd/csrc/rtk_sweep_rule.h on the CPU (tests/test_sweep_cpu.py builds this with the host compiler,
// -ffp-contract=off as the library is built, and the address and undefined-behaviour sanitizers, against the rule headers alone).
//
// Reads cases from the file named on the command line (or stdin), one per line, every number as the hexadecimal bits of a 32-bit
// word; w0 .. w8 are the nine floats of a rtk_sphere_sweep (origin, direction, min_t, max_t, radius):
//     q w0 .. w8                                  the query: prints r2 dd s0 s1 s2 and whether it is live (decimal, 1 or 0)
//     b w0 .. w8 lo0 lo1 lo2 hi0 hi1 hi2          path and box: prints te and whether the interval is not empty (decimal)
//     t w0 .. w8 a0 a1 a2 b0 b1 b2 c0 c1 c2       ball and triangle: prints t and the feature (decimal, 0 .. 8)
//     c t prim best_t best_prim                   better than: prints 1 or 0
//     s te best_t                                 may be skipped: prints 1 or 0
// one line of output per case, in the order of the cases; "ok" at the end. A line it cannot read ends the run with status 1.
#include "rtk_sweep_rule.h"

#include <inttypes.h>
#include <stdio.h>
#include <string.h>

static float as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

int main(int argc, char **argv)
{
	FILE *in = argc > 1 ? fopen(argv[1], "r") : stdin;
	if (!in) { fprintf(stderr, "sweep_rule_driver: cannot open %s\n", argv[1]); return 1; }
	char kind;
	unsigned long cases = 0;
	while (fscanf(in, " %c", &kind) == 1) {
		const int words = kind == 'q' ? 9 : kind == 'b' ? 15 : kind == 't' ? 18 : kind == 'c' ? 4 : kind == 's' ? 2 : 0;
		if (!words) { fprintf(stderr, "sweep_rule_driver: case %lu: kind '%c'\n", cases, kind); return 1; }
		uint32_t w[18];
		float f[18];
		for (int k = 0; k < words; k++) {
			if (fscanf(in, "%" SCNx32, &w[k]) != 1) { fprintf(stderr, "sweep_rule_driver: case %lu: bad word %d\n", cases, k); return 1; }
			f[k] = as_float(w[k]);
		}
		if (kind == 'q' || kind == 'b' || kind == 't') {
			rtk_sweep_query Q;
			const bool live = rtk_sweep_prepare(f, Q);
			if (kind == 'q') {
				printf("%08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %d\n", bits_of(Q.r2), bits_of(Q.dd), bits_of(Q.S[0]),
					bits_of(Q.S[1]), bits_of(Q.S[2]), live ? 1 : 0);
			} else if (kind == 'b') {
				float te = 0.0f;
				const bool some = rtk_sweep_slab(Q, f + 9, f + 12, te);
				printf("%08" PRIx32 " %d\n", bits_of(te), some ? 1 : 0);
			} else {
				float t = 0.0f;
				const int feature = rtk_sweep_triangle(Q, f + 9, f + 12, f + 15, t);
				printf("%08" PRIx32 " %d\n", bits_of(t), feature);
			}
		} else if (kind == 'c') {
			printf("%d\n", rtk_sweep_better(f[0], w[1], f[2], w[3]) ? 1 : 0);
		} else {
			printf("%d\n", rtk_sweep_skip(f[0], f[1]) ? 1 : 0);
		}
		cases++;
	}
	if (in != stdin) fclose(in);
	printf("ok\n");
	return 0;
}
