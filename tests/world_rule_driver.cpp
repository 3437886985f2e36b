// world_rule_driver.cpp -- rtk_amd/csrc/rtk_world_rule.h on the CPU (tests/test_world_cpu.py builds this with the host compiler,
// -ffp-contract=off as the library is built, once plain and once with the address and undefined-behaviour sanitizers, against
// that header and the placement rule it includes alone).
//
// Reads the file named on the command line (or stdin); every float is the hexadecimal bits of a 32-bit word:
//     i m0 .. m11                                rtk_world_inverse: prints 0 or 1 (live) and the 12 words of the inverse
//     r inv0 .. inv11 o0 o1 o2 d0 d1 d2 tmin tmax   rtk_world_ray: prints 8 words
//     b lo0 lo1 lo2 hi0 hi1 hi2 m0 .. m11        rtk_world_box: prints 0 or 1 (finite) and 6 words (lo, hi)
//     g o0 o1 o2 bound                           rtk_world_margin: prints its bits
// "ok" at the end. A line it cannot read ends the run with status 1.
#include "rtk_world_rule.h"

#include <inttypes.h>
#include <stdio.h>
#include <string.h>

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
	if (!in) { fprintf(stderr, "world_rule_driver: cannot open %s\n", argv[1]); return 1; }
	char kind;
	unsigned long cases = 0;
	while (fscanf(in, " %c", &kind) == 1) {
		float f[20], out[12];
		bool ok = true;
		if (kind == 'i') {
			if ((ok = read_words(in, 12, f))) { printf("%d ", rtk_world_inverse(f, out) ? 1 : 0); print_words(out, 12); }
		} else if (kind == 'r') {
			if ((ok = read_words(in, 20, f))) { rtk_world_ray(f, f + 12, out); print_words(out, 8); }
		} else if (kind == 'b') {
			if ((ok = read_words(in, 18, f))) { printf("%d ", rtk_world_box(f, f + 3, f + 6, out, out + 3) ? 1 : 0); print_words(out, 6); }
		} else if (kind == 'g') {
			if ((ok = read_words(in, 4, f))) { out[0] = rtk_world_margin(f, f[3]); print_words(out, 1); }
		} else { fprintf(stderr, "world_rule_driver: case %lu: kind '%c'\n", cases, kind); return 1; }
		if (!ok) { fprintf(stderr, "world_rule_driver: case %lu: bad word\n", cases); return 1; }
		cases++;
	}
	if (in != stdin) fclose(in);
	printf("ok\n");
	return 0;
}
