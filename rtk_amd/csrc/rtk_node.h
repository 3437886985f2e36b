// rtk_node.h -- the two node records of the device BVH and the child words they hold, without any HIP: included by rtk_dev.h,
// and by rtk_node_finish.h, whose arithmetic also runs on the host under a test (tests/node_finish_driver.cpp).
#pragma once

#include <stdint.h>

#define RTK_REF_NONE 0xffffffffu  // empty child slot / "no node"
#define RTK_REF_LEAF 0x80000000u  // leaf: low 31 bits = first triangle slot

struct DevNode {
	float bx[2][4];
	float by[2][4];
	float bz[2][4];
	uint32_t child[4];
	// Front-to-back order of the four children for each of the eight direction-sign octants (octant o: bit 0 = x negative,
	// bit 1 = y negative, bit 2 = z negative), written by k_quantize from the child boxes alone (centre of the box along
	// the octant's diagonal; empty slots last). order[o >> 1], half (o & 1): bits 0-7 = the permutation (position q, nearest
	// first -> child slot, two bits each), bits 8-13 = for each pair of slots (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) whether the
	// SECOND comes before the first. The packet kernel orders the children a tile enters by these instead of sorting entry
	// distances (any order gives the same hits: DESIGN.md 3.2); not part of the content hash, not exported.
	uint32_t order[4];
};
#define RTK_ORDER_PAIR_SHIFT 8
static_assert(sizeof(DevNode) == 128, "node must be one 128 B line");

// Compressed node for the per-lane kernels, 64 B = half a cache line (two children of one parent share a line):
// child boxes quantised to 8 bits per plane on a per-node, per-axis power-of-two grid anchored at the node's own
// min corner. Decoded plane = org + q * scale; low planes round down, high planes round up, so a decoded box
// always CONTAINS the exact one (checked in double precision when it is made, and again by the validator).
// Incoherent and shadow rays are bound by bytes through the fabric; this halves the bytes of a
// node visit. Hits do not change: culling only ever gets more conservative, the triangles decide the result.
struct DevNodeQ {
	float org[3];
	float scale[3];           // powers of two
	uint32_t q[3][2];         // [axis][0 = low planes, 1 = high planes], byte k = child k
	uint32_t child[4];
};
static_assert(sizeof(DevNodeQ) == 64, "quantised node must be half a 128 B line");
