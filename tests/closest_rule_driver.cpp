// closest_rule_driver.cpp -- rtk_amd/csrc/rtk_closest_rule.h on the CPU (tests/test_closest_cpu.py builds this with the host
// compiler, -ffp-contract=off as the library is built, and the address and undefined-behaviour sanitizers, against that header alone).
//
// Reads cases from the file named on the command line (or stdin), one per line, every number as the hexadecimal bits of a 32-bit word:
//     t p0 p1 p2 a0 a1 a2 b0 b1 b2 c0 c1 c2      point and triangle: prints dist2 u v q0 q1 q2 and the region (decimal, 1 .. 7)
//     b p0 p1 p2 lo0 lo1 lo2 hi0 hi1 hi2         point and box: prints bound
//     c dist2 prim best2 best_prim               better than: prints 1 or 0
//     s bound best2                              may be skipped: prints 1 or 0
// one line of output per case, in the order of the cases; "ok" at the end. A line it cannot read ends the run with status 1.
#include "rtk_closest_rule.h"

#include <inttypes.h>
#include <stdio.h>
#include <string.h>

static float as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

int main(int argc, char **argv)
{
	FILE *in = argc > 1 ? fopen(argv[1], "r") : stdin;
	if (!in) { fprintf(stderr, "closest_rule_driver: cannot open %s\n", argv[1]); return 1; }
	char kind;
	unsigned long cases = 0;
	while (fscanf(in, " %c", &kind) == 1) {
		const int words = kind == 't' ? 12 : kind == 'b' ? 9 : kind == 'c' ? 4 : kind == 's' ? 2 : 0;
		if (!words) { fprintf(stderr, "closest_rule_driver: case %lu: kind '%c'\n", cases, kind); return 1; }
		uint32_t w[12];
		float f[12];
		for (int k = 0; k < words; k++) {
			if (fscanf(in, "%" SCNx32, &w[k]) != 1) { fprintf(stderr, "closest_rule_driver: case %lu: bad word %d\n", cases, k); return 1; }
			f[k] = as_float(w[k]);
		}
		if (kind == 't') {
			float q[3], u, v;
			int region = 0;
			const float dist2 = rtk_closest_triangle(f, f + 3, f + 6, f + 9, q, u, v, region);
			printf("%08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %d\n", bits_of(dist2), bits_of(u), bits_of(v),
				bits_of(q[0]), bits_of(q[1]), bits_of(q[2]), region);
		} else if (kind == 'b') {
			printf("%08" PRIx32 "\n", bits_of(rtk_closest_box_bound(f, f + 3, f + 6)));
		} else if (kind == 'c') {
			printf("%d\n", rtk_closest_better(f[0], w[1], f[2], w[3]) ? 1 : 0);
		} else {
			printf("%d\n", rtk_closest_skip(f[0], f[1]) ? 1 : 0);
		}
		cases++;
	}
	if (in != stdin) fclose(in);
	printf("ok\n");
	return 0;
}
