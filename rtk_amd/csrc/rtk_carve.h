// rtk_carve.h -- internal, host only (no HIP): tables that share one device allocation, sized and placed by one carve.
//
// Every piece begins on a 256-byte step and a piece of 0 bytes still takes one, so no two tables share an address. Whoever
// takes a piece has added it to both sums: a table cannot be placed without being allocated and counted.
// (rtk_build_layout.h keeps a take of its own on purpose: it pads the offset, not the size, and a 0-byte buffer takes nothing
// there. tests/test_build_layout_cpu.py pins those offsets, tests/test_carve_cpu.py these.)
#pragma once

#include <stddef.h>

static inline size_t rtk_padded(size_t bytes) { return ((bytes ? bytes : 1) + 255u) & ~(size_t)255u; }   // sizes inside one allocation: 256-byte steps

struct Carve {
	size_t bytes = 0;      // what to allocate: every piece padded, the last one included
	size_t counted = 0;    // the unpadded sum of the pieces: what the ledger reports at the sites that count that way (rtk_scene_mem.h)
	size_t take(size_t piece_bytes) { const size_t at = bytes; bytes += rtk_padded(piece_bytes); counted += piece_bytes; return at; }   // the piece's offset
};
