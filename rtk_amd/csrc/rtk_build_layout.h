// rtk_build_layout.h -- where every temporary of a device build lies in the build workspace (rtk_build.hip owns it, the stage files
// rtk_build_*.hip take their buffers from it).
//
// Host only, no HIP: one carve both sizes the workspace (BuildLayout::bytes) and places every buffer in it (byte offsets from
// the workspace's base), so a buffer cannot be placed without being counted. tests/test_build_layout_cpu.py checks the carve
// over a table of scene sizes with the host compiler alone.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#define RTK_BUILD_REFIT_TILE 1024u       // sorted triangles per refit tile (REFIT_TILE of rtk_build_internal.h)
#define RTK_BUILD_COLLAPSE_BLOCK 256u    // jobs per workgroup of the level-by-level collapse (COLLAPSE_BLOCK)
#define RTK_BUILD_COLLAPSE_RING 64u      // level states in flight (COLLAPSE_RING)
#define RTK_BUILD_COLLAPSE_SMALL_JOBS 64u   // largest level the one-workgroup collapse kernel takes (COLLAPSE_SMALL_JOBS)

// sizes of the records the build kernels define (rtk_build_internal.h asserts its structs against these)
#define RTK_BUILD_SIZEOF_INTRI 48u
#define RTK_BUILD_SIZEOF_BINNODE 32u
#define RTK_BUILD_SIZEOF_CLIMB 12u
#define RTK_BUILD_SIZEOF_LEVELSTATE 32u
#define RTK_BUILD_SIZEOF_MESHSRC 16u
#define RTK_BUILD_SIZEOF_DEVNODE 128u

// bytes of one mesh's raw buffers that a build copies to the device as they are (0: nothing to copy -- the buffer is device
// memory already, the mesh has no indices, or it is decoded on the host)
struct BuildUpload { size_t ibytes, pbytes; };

struct BuildLayout {
	// 1 ingest
	size_t in_tris;          // InTri x n: staged triangles in input order
	size_t cent;             // float x 3n: doubled centroids
	size_t bounds;           // uint32 x 16: centroid bounds (six words used)
	std::vector<size_t> mesh_idx, mesh_pos;     // per mesh: its uploaded index / position bytes (only where BuildUpload says so)
	// 3 morton, 4 sort
	size_t keys_a, keys_b;   // uint64 x n each
	size_t vals_a, vals_b;   // uint32 x n each, only when not `packed` (the words carry the triangle's number themselves)
	size_t sort_scratch;     // uint32 x sort_words
	size_t mesh_src;         // MeshSrc x (meshes + 1)
	// 6 + 7 refit
	size_t lr, range;        // int2, uint2 x n
	size_t climbers;         // Climb x n
	size_t half;             // uint64 x 2n
	size_t arrive;           // uint32 x n
	size_t root;             // int x 4
	size_t bin;              // BinNode x n
	size_t tile_count, tile_base;               // uint32 x (tiles + 1) each
	size_t depth_word;       // uint32 x 4
	size_t area;             // float x n, only in tile mode
	size_t tile_nclimb;      // uint32 x (tiles + 1)
	// n nodes' worth of workspace: every node of the tree without tile mode (worst case). In tile mode it holds the nodes above
	// the tiles until k_top_finish moves them to their places (at most top_cap <= n / 2 of them; a tree with more goes the other
	// way), their tile-root and level words, a word per binary node for what k_collapse_tile tells k_top_finish about the tile
	// roots, and the tiles' lists of roots (k_refit_tile):
	size_t nodes_tmp;        // DevNode x n; in tile mode its first top_cap nodes only, followed by
	size_t top_refs;         //   uint4 x top_cap
	size_t top_level;        //   uint32 x top_cap
	size_t root_info;        //   uint64 x n
	size_t root_list;        //   int x n
	size_t tile_nroots;      // uint32 x (tiles + 1)
	// 8 collapse
	size_t jobs;             // int x n
	size_t dec;              // int4 x n
	size_t info;             // uint32 x n
	size_t sums;             // uint32 x ceil(n / RTK_BUILD_COLLAPSE_BLOCK)
	size_t ring;             // LevelState x RTK_BUILD_COLLAPSE_RING
	size_t bytes;            // the workspace a build with these inputs needs
};

static const size_t RTK_BUILD_NO_BUFFER = ~(size_t)0;      // the offset of a buffer this build does not have

// Buffers follow one another in the order of the struct, each on a 256-byte step. n >= 2 triangles; `uploads` has one entry per
// mesh; sort_words = rtk_sort_scratch_words(n); tile_mode needs more than one refit tile. False (and nothing to rely on in *L):
// the tile-mode pieces would not fit the n-node region they share -- n / 2 * 148 + 8 n + 4 n + padding <= 128 n holds from n = 7
// on, far below two tiles, so that is an internal error.
static inline bool rtk_build_layout(uint32_t n, const std::vector<BuildUpload> &uploads, bool packed, bool tile_mode, uint32_t top_cap,
	size_t sort_words, BuildLayout *L)
{
	const size_t N = n, tiles1 = (N + RTK_BUILD_REFIT_TILE - 1u) / RTK_BUILD_REFIT_TILE + 1u, meshes = uploads.size();
	size_t off = 0;
	auto take = [&off](size_t bytes) { off = (off + 255u) & ~(size_t)255u; const size_t at = off; off += bytes; return at; };
	L->in_tris = take(N * RTK_BUILD_SIZEOF_INTRI);
	L->cent = take(3 * N * 4);
	L->bounds = take(16 * 4);
	L->mesh_idx.assign(meshes, RTK_BUILD_NO_BUFFER);
	L->mesh_pos.assign(meshes, RTK_BUILD_NO_BUFFER);
	for (size_t m = 0; m < meshes; m++) {
		if (uploads[m].ibytes) L->mesh_idx[m] = take(uploads[m].ibytes);
		if (uploads[m].pbytes) L->mesh_pos[m] = take(uploads[m].pbytes);
	}
	L->keys_a = take(N * 8);
	L->keys_b = take(N * 8);
	L->vals_a = packed ? RTK_BUILD_NO_BUFFER : take(N * 4);
	L->vals_b = packed ? RTK_BUILD_NO_BUFFER : take(N * 4);
	L->sort_scratch = take(sort_words * 4);
	L->mesh_src = take((meshes + 1) * RTK_BUILD_SIZEOF_MESHSRC);
	L->lr = take(N * 8);
	L->range = take(N * 8);
	L->climbers = take(N * RTK_BUILD_SIZEOF_CLIMB);
	L->half = take(2 * N * 8);
	L->arrive = take(N * 4);
	L->root = take(4 * 4);
	L->bin = take(N * RTK_BUILD_SIZEOF_BINNODE);
	L->tile_count = take(tiles1 * 4);
	L->tile_base = take(tiles1 * 4);
	L->depth_word = take(4 * 4);
	L->area = tile_mode ? take(N * 4) : RTK_BUILD_NO_BUFFER;
	L->tile_nclimb = take(tiles1 * 4);
	L->nodes_tmp = take(N * RTK_BUILD_SIZEOF_DEVNODE);
	L->top_refs = L->top_level = L->root_info = L->root_list = RTK_BUILD_NO_BUFFER;
	if (tile_mode) {
		const size_t cap = top_cap;
		L->top_refs = L->nodes_tmp + cap * RTK_BUILD_SIZEOF_DEVNODE;
		L->top_level = L->top_refs + cap * 16;
		L->root_info = L->nodes_tmp + ((cap * (RTK_BUILD_SIZEOF_DEVNODE + 16u + 4u) + 255u) & ~(size_t)255u);
		L->root_list = L->root_info + N * 8;
		if (cap > N / 2 || L->root_list + N * 4 > L->nodes_tmp + N * RTK_BUILD_SIZEOF_DEVNODE) return false;
	}
	L->tile_nroots = take(tiles1 * 4);
	L->jobs = take(N * 4);
	L->dec = take(N * 16);
	L->info = take(N * 4);
	L->sums = take((N + RTK_BUILD_COLLAPSE_BLOCK - 1u) / RTK_BUILD_COLLAPSE_BLOCK * 4);
	L->ring = take(RTK_BUILD_COLLAPSE_RING * RTK_BUILD_SIZEOF_LEVELSTATE);
	L->bytes = off;
	return true;
}
