// obbsweep_rule_driver.cpp -- rtk_amd/csrc/rtk_obbsweep_rule.h on the CPU (tests/test_obbsweep_cpu.py builds this with the host
// compiler, -ffp-contract=off as the library is built, and the address and undefined-behaviour sanitizers, against the rule
// headers alone).
//
// Reads cases from the file named on the command line (or stdin), one per line, every number as the hexadecimal bits of a 32-bit
// word; w0 .. w19 are the twenty floats of a rtk_obb_sweep (origin, direction, min_t, max_t, half, axes):
//     q w0 .. w19                                 the query: prints the centre at min_t, D' and g, then whether it is live (decimal, 1 or 0)
//     b w0 .. w19 lo0 lo1 lo2 hi0 hi1 hi2         path and box: prints te tx, then whether the interval is not empty
//     t w0 .. w19 a0 a1 a2 b0 b1 b2 c0 c1 c2      box and triangle: prints t n0 n1 n2 (the normal), then the axis (decimal, 0 .. 15)
// one line of output per case, in the order of the cases; "ok" at the end. A line it cannot read ends the run with status 1.
// For millions of cases: obbsweep_rule_driver --binary IN OUT reads `t` cases as records of twenty-nine 32-bit words and writes
// five words per case, t n0 n1 n2 axis.
#include "rtk_obbsweep_rule.h"

#include <inttypes.h>
#include <stdio.h>
#include <string.h>

static float as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static int binary(const char *in_path, const char *out_path)
{
	FILE *in = fopen(in_path, "rb"), *out = fopen(out_path, "wb");
	if (!in || !out) { fprintf(stderr, "obbsweep_rule_driver: cannot open %s or %s\n", in_path, out_path); return 1; }
	uint32_t w[29];
	while (fread(w, 4, 29, in) == 29) {
		float f[29], t = 0.0f, n[3];
		for (int k = 0; k < 29; k++) f[k] = as_float(w[k]);
		rtk_obbsweep_query Q;
		(void)rtk_obbsweep_prepare(f, Q);
		const int axis = rtk_obbsweep_triangle(Q, f + 20, f + 23, f + 26, t);
		rtk_obbsweep_normal(Q, f + 20, f + 23, f + 26, axis, n);
		const uint32_t r[5] = { bits_of(t), bits_of(n[0]), bits_of(n[1]), bits_of(n[2]), (uint32_t)axis };
		if (fwrite(r, 4, 5, out) != 5) { fprintf(stderr, "obbsweep_rule_driver: cannot write %s\n", out_path); return 1; }
	}
	fclose(in);
	return fclose(out) == 0 ? 0 : 1;
}

int main(int argc, char **argv)
{
	if (argc == 4 && strcmp(argv[1], "--binary") == 0) return binary(argv[2], argv[3]);
	FILE *in = argc > 1 ? fopen(argv[1], "r") : stdin;
	if (!in) { fprintf(stderr, "obbsweep_rule_driver: cannot open %s\n", argv[1]); return 1; }
	char kind;
	unsigned long cases = 0;
	while (fscanf(in, " %c", &kind) == 1) {
		const int words = kind == 'q' ? 20 : kind == 'b' ? 26 : kind == 't' ? 29 : 0;
		if (!words) { fprintf(stderr, "obbsweep_rule_driver: case %lu: kind '%c'\n", cases, kind); return 1; }
		uint32_t w[29];
		float f[29];
		for (int k = 0; k < words; k++) {
			if (fscanf(in, "%" SCNx32, &w[k]) != 1) { fprintf(stderr, "obbsweep_rule_driver: case %lu: bad word %d\n", cases, k); return 1; }
			f[k] = as_float(w[k]);
		}
		rtk_obbsweep_query Q;
		const bool live = rtk_obbsweep_prepare(f, Q);
		if (kind == 'q') {
			float s[3];
			rtk_obbsweep_centre(Q, Q.S.tmin, s);
			for (int k = 0; k < 3; k++) printf("%08" PRIx32 " ", bits_of(s[k]));
			for (int k = 0; k < 3; k++) printf("%08" PRIx32 " ", bits_of(Q.F.D[k]));
			for (int k = 0; k < 3; k++) printf("%08" PRIx32 " ", bits_of(Q.S.H[k]));
			printf("%d\n", live ? 1 : 0);
		} else if (kind == 'b') {
			float te = 0.0f, tx = 0.0f;
			const bool some = rtk_obbsweep_slab(Q, f + 20, f + 23, te, tx);
			printf("%08" PRIx32 " %08" PRIx32 " %d\n", bits_of(te), bits_of(tx), some ? 1 : 0);
		} else {
			float t = 0.0f, n[3];
			const int axis = rtk_obbsweep_triangle(Q, f + 20, f + 23, f + 26, t);
			rtk_obbsweep_normal(Q, f + 20, f + 23, f + 26, axis, n);
			printf("%08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %d\n", bits_of(t), bits_of(n[0]), bits_of(n[1]), bits_of(n[2]), axis);
		}
		cases++;
	}
	if (in != stdin) fclose(in);
	printf("ok\n");
	return 0;
}
