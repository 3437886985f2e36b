// node_finish_driver.cpp -- rtk_amd/csrc/rtk_node_finish.h on the CPU (tests/test_node_finish_cpu.py builds this with the host
// compiler, -ffp-contract=off as the library is built, and the address and undefined-behaviour sanitizers, against that header
// and rtk_node.h alone: no HIP include path).
//
// Reads nodes from the file named on the command line (or stdin), one per line, every number as the hexadecimal bits of a 32-bit
// word: the 24 box floats in the order of DevNode (bx[min][4], bx[max][4], by.., bz..) and the four child words. Prints per node,
// on one line: the 16 words of the DevNodeQ, the four order words, the misfit flag (1: quantize_node returned false) and the bits
// of root_bound(node, 0); "ok" at the end. A line it cannot read ends the run with status 1.
#include "rtk_node_finish.h"

#include <inttypes.h>
#include <stdio.h>
#include <string.h>

static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

int main(int argc, char **argv)
{
	FILE *in = argc > 1 ? fopen(argv[1], "r") : stdin;
	if (!in) { fprintf(stderr, "node_finish_driver: cannot open %s\n", argv[1]); return 1; }
	unsigned long cases = 0;
	for (;;) {
		uint32_t w[28];
		int got = 0;
		while (got < 28 && fscanf(in, "%" SCNx32, &w[got]) == 1) got++;
		if (got == 0 && feof(in)) break;
		if (got != 28) { fprintf(stderr, "node_finish_driver: node %lu: %d of 28 words\n", cases, got); return 1; }
		DevNode nd;
		memset(&nd, 0, sizeof(nd));
		memcpy(&nd, w, sizeof(w));                           // boxes and child words lie at the front of the node, in this order
		DevNodeQ q;
		memset(&q, 0xee, sizeof(q));                         // (every word must be written)
		const bool fits = quantize_node(nd, q);
		uint32_t order[4] = { 0xeeeeeeeeu, 0xeeeeeeeeu, 0xeeeeeeeeu, 0xeeeeeeeeu };
		child_order(nd, order);
		uint32_t qw[16];
		memcpy(qw, &q, sizeof(qw));
		for (int k = 0; k < 16; k++) printf("%08" PRIx32 " ", qw[k]);
		for (int k = 0; k < 4; k++) printf("%08" PRIx32 " ", order[k]);
		printf("%d %08" PRIx32 "\n", fits ? 0 : 1, bits_of(root_bound(nd, 0.0f)));
		cases++;
	}
	if (in != stdin) fclose(in);
	printf("ok\n");
	return 0;
}
