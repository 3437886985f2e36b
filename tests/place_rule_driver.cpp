// place_rule_driver.cpp -- rtk_amd/csrc/rtk_place_rule.h on the CPU (tests/test_place_cpu.py builds this with the host compiler,
// -ffp-contract=off as the library is built, and the address and undefined-behaviour sanitizers, against that header alone).
//
// Reads cases from the file named on the command line (or stdin), one per line, every number as the hexadecimal bits of its type:
//     f m0 .. m11 x y z        a placement and a float vertex (15 words of 32 bits)
//     d m0 .. m11 x y z        the same with a double vertex (12 words of 32 bits, 3 of 64): made float first, as an ingest does
// and prints the bits of the placed vertex, three 32-bit words per line, in the order of the cases; "ok" at the end. A line it
// cannot read ends the run with status 1.
#include "rtk_place_rule.h"

#include <inttypes.h>
#include <stdio.h>
#include <string.h>

static float as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static double as_double(uint64_t u) { double d; memcpy(&d, &u, 8); return d; }
static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

int main(int argc, char **argv)
{
	FILE *in = argc > 1 ? fopen(argv[1], "r") : stdin;
	if (!in) { fprintf(stderr, "place_rule_driver: cannot open %s\n", argv[1]); return 1; }
	char kind;
	unsigned long cases = 0;
	while (fscanf(in, " %c", &kind) == 1) {
		uint32_t mw[12];
		float m[12], v[3];
		for (int k = 0; k < 12; k++) {
			if (fscanf(in, "%" SCNx32, &mw[k]) != 1) { fprintf(stderr, "place_rule_driver: case %lu: bad placement\n", cases); return 1; }
			m[k] = as_float(mw[k]);
		}
		for (int k = 0; k < 3; k++) {
			if (kind == 'f') {
				uint32_t w;
				if (fscanf(in, "%" SCNx32, &w) != 1) { fprintf(stderr, "place_rule_driver: case %lu: bad vertex\n", cases); return 1; }
				v[k] = as_float(w);
			} else if (kind == 'd') {
				uint64_t w;
				if (fscanf(in, "%" SCNx64, &w) != 1) { fprintf(stderr, "place_rule_driver: case %lu: bad vertex\n", cases); return 1; }
				v[k] = (float)as_double(w);
			} else { fprintf(stderr, "place_rule_driver: case %lu: kind '%c'\n", cases, kind); return 1; }
		}
		rtk_place_vertex(m, v[0], v[1], v[2]);
		printf("%08" PRIx32 " %08" PRIx32 " %08" PRIx32 "\n", bits_of(v[0]), bits_of(v[1]), bits_of(v[2]));
		cases++;
	}
	if (in != stdin) fclose(in);
	printf("ok\n");
	return 0;
}
