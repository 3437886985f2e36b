// capsule_rule_driver.cpp -- rtk_amd/csrc/rtk_capsule_rule.h on the CPU (tests/test_capsule_cpu.py builds this with the host
// compiler, -ffp-contract=off as the library is built, and the address and undefined-behaviour sanitizers, against the rule
// headers alone).
//
// Reads cases from the file named on the command line (or stdin), one per line, every number as the hexadecimal bits of a 32-bit
// word; w0 .. w11 are the twelve floats of a rtk_capsule_sweep (origin, direction, min_t, max_t, radius, half_axis):
//     q w0 .. w11                                 the query: prints r2 dd s[3] g[3] p0[3] p1[3] and whether it is live (decimal)
//     b w0 .. w11 lo0 lo1 lo2 hi0 hi1 hi2         path and box: prints te and whether the interval is not empty (decimal)
//     t w0 .. w11 a0 a1 a2 b0 b1 b2 c0 c1 c2      capsule and triangle: prints t and the feature (decimal, 0 .. 27)
//     r w0 .. w11 a0 .. c2 t                      the record at time t: prints dist2 u v qt[3] qa[3] and the item (decimal)
//     c t prim best_t best_prim                   better than: prints 1 or 0
//     s te best_t                                 may be skipped: prints 1 or 0
// one line of output per case, in the order of the cases; "ok" at the end. A line it cannot read ends the run with status 1.
#include "rtk_capsule_rule.h"

#include <inttypes.h>
#include <stdio.h>
#include <string.h>

static float as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static void put(const float *f, int n) { for (int k = 0; k < n; k++) printf("%08" PRIx32 " ", bits_of(f[k])); }

int main(int argc, char **argv)
{
	FILE *in = argc > 1 ? fopen(argv[1], "r") : stdin;
	if (!in) { fprintf(stderr, "capsule_rule_driver: cannot open %s\n", argv[1]); return 1; }
	char kind;
	unsigned long cases = 0;
	while (fscanf(in, " %c", &kind) == 1) {
		const int words = kind == 'q' ? 12 : kind == 'b' ? 18 : kind == 't' ? 21 : kind == 'r' ? 22 : kind == 'c' ? 4 : kind == 's' ? 2 : 0;
		if (!words) { fprintf(stderr, "capsule_rule_driver: case %lu: kind '%c'\n", cases, kind); return 1; }
		uint32_t w[22];
		float f[22];
		for (int k = 0; k < words; k++) {
			if (fscanf(in, "%" SCNx32, &w[k]) != 1) { fprintf(stderr, "capsule_rule_driver: case %lu: bad word %d\n", cases, k); return 1; }
			f[k] = as_float(w[k]);
		}
		if (kind == 'c') printf("%d\n", rtk_sweep_better(f[0], w[1], f[2], w[3]) ? 1 : 0);
		else if (kind == 's') printf("%d\n", rtk_sweep_skip(f[0], f[1]) ? 1 : 0);
		else {
			rtk_capsule_query Q;
			const bool live = rtk_capsule_prepare(f, Q);
			if (kind == 'q') {
				put(&Q.S.r2, 1); put(&Q.S.dd, 1); put(Q.S.S, 3); put(Q.g, 3); put(Q.p0, 3); put(Q.p1, 3);
				printf("%d\n", live ? 1 : 0);
			} else if (kind == 'b') {
				float te = 0.0f;
				const bool some = rtk_capsule_slab(Q, f + 12, f + 15, te);
				printf("%08" PRIx32 " %d\n", bits_of(te), some ? 1 : 0);
			} else if (kind == 't') {
				float t = 0.0f;
				const int feature = rtk_capsule_triangle(Q, f + 12, f + 15, f + 18, t);
				printf("%08" PRIx32 " %d\n", bits_of(t), feature);
			} else {
				rtk_capsule_contact r;
				rtk_capsule_record(Q, f[21], f + 12, f + 15, f + 18, r);
				put(&r.dist2, 1); put(&r.u, 1); put(&r.v, 1); put(r.qt, 3); put(r.qa, 3);
				printf("%d\n", r.item);
			}
		}
		cases++;
	}
	if (in != stdin) fclose(in);
	printf("ok\n");
	return 0;
}
