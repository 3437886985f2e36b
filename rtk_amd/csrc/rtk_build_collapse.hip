// rtk_build_collapse.hip -- the device build's last stage (rtk_build_internal.h has the map): the binary tree collapsed to 128 B
// 4-wide nodes, level by level for the whole tree or, in tile mode, for the nodes above the refit tiles beside the tile-local collapse.
#include "rtk_build_internal.h"
#include "rtk_node_finish.h"

#include <string.h>

#include <algorithm>

using namespace rtk_bld;

namespace {

// ---------------------------------------------------------------------------------- 8 collapse
// Binary tree -> 128 B 4-wide nodes, breadth first. A job is one wide node = one binary node that gets opened:
// its two children, then twice more the largest-area child that is still an inner node (the reference collapses
// exactly two binary levels, rtk.c:1572-1592; the greedy rule costs 2 % fewer node visits on the benchmark
// scene). Wide-node numbers come from prefix sums, not from an atomic counter, so the node array is the same for
// every build of the same input. A node is written in two steps, each in whole 32-B sectors:
//   k_collapse_open    one thread per job of a level: reads the binary records (the dependent-load chain, so it gets
//                      all the parallelism there is), writes the node's boxes (96 B), marks its leaves in the triangle
//                      array, and leaves behind what depends on a prefix sum: the four child words with binary
//                      references in the slots of inner children (dec), which slots those are (info), and per 256
//                      jobs their number
//   k_collapse_number  per job: prefix sum of the inner children -> their node numbers; writes the child words
//                      (32 B) and the next level's job list. A block adds up the block sums before it by itself.
//   k_collapse_small   levels of at most 1024 jobs -- the top six and the last few -- both steps in ONE workgroup,
//                      several levels per launch (also opens the root)
// Level bookkeeping lives in device memory: launch number `step` reads ring entry step and writes entry step+1,
// so nothing a running kernel reads is written by it. The host reads the ring once per round.

__global__ void k_publish(BuildResults *out, const uint32_t *tiles_total, const uint32_t *depth_word, const DevSceneConsts *consts)
{
	out->tiles_total = tiles_total ? *tiles_total : 0u;
	out->depth = depth_word[0];
	out->equal_codes = depth_word[1];
	out->consts = *consts;
}

struct Cand {
	int ref;          // binary child: >= 0 inner, < 0 leaf ~slot
	float area;       // > 0 only if the child may still be opened
	float mn[3], mx[3];
	bool tile_job;    // tile mode: an inner node inside one refit tile -- a wide node that k_collapse_tile makes, not opened here
};

// The subtree is left alone by the level-by-level collapse if it lies inside one refit tile (tile mode).
__device__ __forceinline__ bool in_one_tile(const uint2 rg) { return rg.x / REFIT_TILE == rg.y / REFIT_TILE; }

__device__ __forceinline__ Cand make_cand(int ref, const BinNode *bin, const DevTri *tris, const uint2 *range, bool tile_mode)
{
	Cand c;
	c.ref = ref;
	c.area = -1.0f;
	c.tile_job = false;
	if (ref >= 0) {
		const BinNode b = bin[ref];
		c.mn[0] = b.mn[0]; c.mn[1] = b.mn[1]; c.mn[2] = b.mn[2];
		c.mx[0] = b.mx[0]; c.mx[1] = b.mx[1]; c.mx[2] = b.mx[2];
		// An inner node that is not one leaf can always be opened; the area only ranks the candidates. It can be ZERO
		// (a box flat on two axes: triangles in a row, or extents that underflow) -- taking "area > 0" for "may be opened"
		// turned such subtrees into single leaves of any size, which the 6-bit leaf count of the blob cannot even hold.
		if (!(b.cnt_flag & 0x80000000u)) {
			if (tile_mode && in_one_tile(range[ref])) c.tile_job = true;
			else c.area = fmaxf(half_area(b.mn, b.mx), 1e-37f);
		}
	} else tri_box(tris, (uint32_t)~ref, c.mn, c.mx);
	return c;
}

// a subtree the SAH rule turned into one leaf of the sorted triangles [rg.x, rg.y]: the count goes into its first record,
// and only the last one keeps the end mark (every record starts out as a leaf of its own, k_emit_tris)
__device__ __forceinline__ void mark_leaf(DevTri *tris, const uint2 rg)
{
	tris[rg.x].spare = rg.y - rg.x + 1u;
	for (uint32_t t = rg.x; t < rg.y; t++) { tris[t].flags &= ~RTK_TRI_LAST; tris[t + 1u].spare = 0u; }
}

// Opens binary node b as wide node `node_index`: chooses its (up to four) children and writes the node except for the
// numbers of the children that are wide nodes themselves. Returns how many those are.
// aux.tile_refs != NULL: tile mode -- the nodes ABOVE the refit tiles, written to a stretch of the workspace with numbers of
// their own (k_top_finish moves them behind the tiles' nodes, which k_collapse_tile makes at the same time on another stream).
// Children that are tile jobs keep an empty child word; WHICH binary node hangs in the slot goes to aux.tile_refs[node]
// (+ 1; 0: not a tile job) and the node's level to aux.level[node], for k_top_finish.
__device__ __forceinline__ uint32_t collapse_open(int b, uint32_t node_index, const int2 *lr, const uint2 *range, const BinNode *bin,
	DevTri *tris, DevNode *nodes, uint32_t node_cap, int4 &dec, uint32_t &info, TopAux aux = TopAux{ nullptr, nullptr }, uint32_t level = 0)
{
	const bool tile_mode = aux.tile_refs != nullptr;
	uint32_t tref[4] = { 0u, 0u, 0u, 0u };
	Cand c[4];
	int nc;
	const BinNode self = bin[b];
	if (self.cnt_flag & 0x80000000u) {
		// the whole (sub)tree is one leaf: only the root of a tiny scene
		c[0].ref = b; c[0].area = -1.0f;
		c[0].mn[0] = self.mn[0]; c[0].mn[1] = self.mn[1]; c[0].mn[2] = self.mn[2];
		c[0].mx[0] = self.mx[0]; c[0].mx[1] = self.mx[1]; c[0].mx[2] = self.mx[2];
		c[0].tile_job = false;
		nc = 1;
	} else {
		const int2 ch = lr[b];
		c[0] = make_cand(ch.x, bin, tris, range, tile_mode);
		c[1] = make_cand(ch.y, bin, tris, range, tile_mode);
		nc = 2;
		// (every index into c[] below is a compile-time constant after unrolling: a run-time index would put the 32-dword
		// array into scratch memory, which made this function several times slower)
#pragma unroll
		for (int round = 0; round < 2; round++) {
			int best = -1, best_ref = 0;
			float best_area = 0.0f;
#pragma unroll
			for (int k = 0; k < 4; k++) if (k < nc && c[k].area > best_area) { best_area = c[k].area; best = k; best_ref = c[k].ref; }
			if (best >= 0) {
				const int2 o = lr[best_ref];
				const Cand left = make_cand(o.x, bin, tris, range, tile_mode), right = make_cand(o.y, bin, tris, range, tile_mode);
#pragma unroll
				for (int k = 0; k < 4; k++) {
					if (k == best) c[k] = left;
					if (k == nc) c[k] = right;
				}
				nc++;
			}
		}
	}
	uint32_t mask = 0, n_inner = 0;
	int r[4] = { 0, 0, 0, 0 };
	float4 rows[6];      // bx[0], bx[1], by[0], by[1], bz[0], bz[1]: the first 96 bytes of the node
	float *out = reinterpret_cast<float *>(rows);
#pragma unroll
	for (int k = 0; k < 4; k++) {
		if (k >= nc) {
			out[0 + k] = out[8 + k] = out[16 + k] = +1.0f;        // inverted = never hit (rtk.c:1612-1620)
			out[4 + k] = out[12 + k] = out[20 + k] = -1.0f;
			continue;
		}
		const int ref = c[k].ref;
		if (ref < 0) {
			// a leaf of one triangle: k_emit_tris wrote every record as exactly that (count 1, last-of-leaf set), so
			// there is nothing to mark -- two 4-byte read-modify-writes per leaf here were the bulk of this kernel's time
			r[k] = (int)(RTK_REF_LEAF | (uint32_t)~ref);
		} else if (c[k].area > 0.0f) {
			mask |= 1u << k;
			n_inner++;
			r[k] = ref;                                           // binary reference; becomes a node number when this level is numbered
		} else if (c[k].tile_job) {
			r[k] = (int)RTK_REF_NONE;                             // k_top_finish writes the number of the wide node k_collapse_tile makes of it
#pragma unroll
			for (int q = 0; q < 4; q++) if (q == k) tref[q] = (uint32_t)ref + 1u;
		} else {
			const uint2 rg = range[ref];
			mark_leaf(tris, rg);
			r[k] = (int)(RTK_REF_LEAF | rg.x);
		}
		out[0 + k] = c[k].mn[0]; out[4 + k] = c[k].mx[0];
		out[8 + k] = c[k].mn[1]; out[12 + k] = c[k].mx[1];
		out[16 + k] = c[k].mn[2]; out[20 + k] = c[k].mx[2];
	}
	// the boxes now (96 B = three whole 32-B sectors); the child words follow in ONE 32-B store when this node's level
	// is numbered -- patching single words of a node written earlier made every patch a read-modify-write in memory
	// (node_cap: the collapse writes straight into the scene's node array, sized from an estimate; should a tree have more
	// nodes than that, the writes beyond it are dropped and the host repeats the collapse into the workspace)
	if (node_index < node_cap) {
		float4 *dst = reinterpret_cast<float4 *>(nodes + node_index);
#pragma unroll
		for (int q = 0; q < 6; q++) dst[q] = rows[q];
		if (tile_mode) {
			aux.tile_refs[node_index] = make_uint4(tref[0], tref[1], tref[2], tref[3]);
			aux.level[node_index] = level;
		}
	}
	for (int k = nc; k < 4; k++) r[k] = (int)RTK_REF_NONE;
	dec = make_int4(r[0], r[1], r[2], r[3]);                      // final child words, except the slots in `mask`: binary references
	info = (mask << 4) | (n_inner << 8);
	return n_inner;
}

// Job `node_index`: its inner children get the numbers next_base + off, ...; the child words go out as one sector and
// the children's binary references to next_jobs[off ...].
__device__ __forceinline__ void collapse_number_children(uint32_t node_index, uint32_t next_base, uint32_t off, const int4 d,
	uint32_t inf, DevNode *nodes, uint32_t node_cap, int *next_jobs)
{
	uint32_t ref[4] = { (uint32_t)d.x, (uint32_t)d.y, (uint32_t)d.z, (uint32_t)d.w };
	const uint32_t mask = (inf >> 4) & 15u;
#pragma unroll
	for (int k = 0; k < 4; k++) {
		if (!(mask & (1u << k))) continue;
		next_jobs[off] = (int)ref[k];
		ref[k] = next_base + off;
		off++;
	}
	// child[4] and pad[4]: the last 32 bytes of the node, one sector
	if (node_index >= node_cap) return;
	uint4 *dst = reinterpret_cast<uint4 *>(&nodes[node_index].child[0]);
	dst[0] = make_uint4(ref[0], ref[1], ref[2], ref[3]);
	dst[1] = make_uint4(0u, 0u, 0u, 0u);
}

__device__ __forceinline__ LevelState next_level(const LevelState &L, uint32_t next_count)
{
	LevelState N = L;
	N.count = next_count;
	N.base = L.base + L.count;
	N.level = L.level + 1u;
	if (L.count) { N.total_nodes = L.base + L.count; N.depth = L.level + 1u; }
	return N;
}

__global__ void __launch_bounds__(COLLAPSE_BLOCK) k_collapse_open(CollapseBufs B, const LevelState *ring, uint32_t step, const int2 *lr, const uint2 *range,
	const BinNode *bin, DevTri *tris, DevNode *nodes, uint32_t node_cap, TopAux aux)
{
	__shared__ uint32_t s_w[COLLAPSE_BLOCK / 64];
	const LevelState L = ring[step % COLLAPSE_RING];
	const uint32_t count = L.count;
	for (uint32_t vb = blockIdx.x; vb * COLLAPSE_BLOCK < count; vb += gridDim.x) {
		const uint32_t j = vb * COLLAPSE_BLOCK + threadIdx.x;
		uint32_t n_inner = 0;
		if (j < count) {
			int4 d;
			uint32_t inf;
			n_inner = collapse_open(B.jobs[j], L.base + j, lr, range, bin, tris, nodes, node_cap, d, inf, aux, L.level);
			B.dec[j] = d;
			B.info[j] = inf;
		}
		uint32_t sum = n_inner;
		for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
		if ((threadIdx.x & 63u) == 0u) s_w[threadIdx.x >> 6] = sum;
		__syncthreads();
		if (threadIdx.x == 0) {
			uint32_t t = 0;
			for (int w = 0; w < COLLAPSE_BLOCK / 64; w++) t += s_w[w];
			B.sums[vb] = t;
		}
		__syncthreads();
	}
}

// Sum of a[lo..hi) for the whole workgroup (COLLAPSE_BLOCK threads).
__device__ __forceinline__ uint32_t block_range_sum(const uint32_t *a, uint32_t lo, uint32_t hi, uint32_t *s_w)
{
	uint32_t t = 0;
	for (uint32_t i = lo + threadIdx.x; i < hi; i += COLLAPSE_BLOCK) t += a[i];
	for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
	__syncthreads();                                    // s_w may still be read from the previous use
	if ((threadIdx.x & 63u) == 0u) s_w[threadIdx.x >> 6] = t;
	__syncthreads();
	uint32_t r = 0;
	for (int w = 0; w < COLLAPSE_BLOCK / 64; w++) r += s_w[w];
	return r;
}

__global__ void __launch_bounds__(COLLAPSE_BLOCK) k_collapse_number(CollapseBufs B, LevelState *ring, uint32_t step, DevNode *nodes, uint32_t node_cap)
{
	__shared__ uint32_t s_w[COLLAPSE_BLOCK / 64];
	__shared__ uint32_t s_r[COLLAPSE_BLOCK / 64];
	const LevelState L = ring[step % COLLAPSE_RING];
	const uint32_t count = L.count, base = L.base, next_base = base + count;
	const uint32_t nb = (count + COLLAPSE_BLOCK - 1u) / COLLAPSE_BLOCK;
	// inner children of the jobs before this workgroup's first block of 256
	uint32_t before = block_range_sum(B.sums, 0u, blockIdx.x < nb ? blockIdx.x : nb, s_r);
	for (uint32_t vb = blockIdx.x; vb * COLLAPSE_BLOCK < count; vb += gridDim.x) {
		const uint32_t j = vb * COLLAPSE_BLOCK + threadIdx.x;
		const uint32_t inf = j < count ? B.info[j] : 0u;
		const int4 d = j < count ? B.dec[j] : make_int4(0, 0, 0, 0);
		const uint32_t n_inner = inf >> 8;
		const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
		uint32_t inc = n_inner;
		for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(inc, o); if (lane >= (uint32_t)o) inc += t; }
		if (lane == 63u) s_w[wave] = inc;
		__syncthreads();
		uint32_t off = before;
		for (uint32_t w = 0; w < wave; w++) off += s_w[w];
		off += inc - n_inner;
		__syncthreads();
		// (the job list is written over the one this level was opened from: nothing reads that any more)
		if (j < count) collapse_number_children(base + j, next_base, off, d, inf, nodes, node_cap, B.jobs);
		const uint32_t hi = vb + gridDim.x < nb ? vb + gridDim.x : nb;
		before += block_range_sum(B.sums, vb, hi, s_r);
	}
	// workgroup 0 has walked over every block sum: `before` is the size of the next level
	if (blockIdx.x == 0 && threadIdx.x == 0) ring[(step + 1u) % COLLAPSE_RING] = next_level(L, before);
}

// Up to max_levels levels, as long as a level has at most COLLAPSE_SMALL jobs; one workgroup. It takes over a level
// that is already opened (dec/info valid) and hands over one that is opened too, block sums included. Launch 0 of a
// build opens the root first.
__global__ void __launch_bounds__(COLLAPSE_SMALL) k_collapse_small(CollapseBufs B, LevelState *ring, uint32_t step, uint32_t max_levels,
	const int2 *lr, const uint2 *range, const BinNode *bin, DevTri *tris, DevNode *nodes, uint32_t node_cap, const int *root, TopAux aux, LevelState *host_out)
{
	__shared__ uint32_t s_w[COLLAPSE_SMALL / 64];
	__shared__ int s_ref[COLLAPSE_SMALL * 4];
	__shared__ uint32_t s_sums[COLLAPSE_SMALL * 4 / COLLAPSE_BLOCK];
	LevelState L;
	if (step == 0u) {
		// level 0 is the root job (the binary node the refit pass ended at), wide node 0
		L.count = 1u; L.base = 0u; L.level = 0u; L.total_nodes = 0u; L.depth = 0u; L.pad[0] = L.pad[1] = L.pad[2] = 0u;
		if (threadIdx.x == 0) {
			int4 d;
			uint32_t inf;
			B.sums[0] = collapse_open(*root, 0u, lr, range, bin, tris, nodes, node_cap, d, inf, aux, 0u);
			B.dec[0] = d;
			B.info[0] = inf;
		}
		__syncthreads();           // (workgroup scope is all that is needed: one workgroup, and the kernel boundary does the rest)
	} else L = ring[step % COLLAPSE_RING];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	for (uint32_t it = 0; it < max_levels && L.count != 0u && L.count <= COLLAPSE_SMALL_JOBS; it++) {
		// number this level's jobs ...
		const uint32_t j = threadIdx.x;
		const uint32_t inf = j < L.count ? B.info[j] : 0u;
		const int4 d = j < L.count ? B.dec[j] : make_int4(0, 0, 0, 0);
		const uint32_t n_inner = inf >> 8;
		uint32_t inc = n_inner;
		for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(inc, o); if (lane >= (uint32_t)o) inc += t; }
		if (lane == 63u) s_w[wave] = inc;
		if (threadIdx.x < COLLAPSE_SMALL * 4 / COLLAPSE_BLOCK) s_sums[threadIdx.x] = 0u;
		__syncthreads();
		uint32_t off = 0, total = 0;
		for (uint32_t w = 0; w < COLLAPSE_SMALL / 64; w++) { if (w < wave) off += s_w[w]; total += s_w[w]; }
		off += inc - n_inner;
		if (j < L.count) collapse_number_children(L.base + j, L.base + L.count, off, d, inf, nodes, node_cap, s_ref);
		const LevelState N = next_level(L, total);
		__syncthreads();
		// ... and open the next level's (every dec/info of this level is in registers by now)
		for (uint32_t i = threadIdx.x; i < total; i += COLLAPSE_SMALL) {
			int4 d2;
			uint32_t inf2;
			const uint32_t n2 = collapse_open(s_ref[i], N.base + i, lr, range, bin, tris, nodes, node_cap, d2, inf2, aux, N.level);
			B.dec[i] = d2;
			B.info[i] = inf2;
			if (n2) atomicAdd(&s_sums[i / COLLAPSE_BLOCK], n2);
		}
		__syncthreads();
		if (threadIdx.x < (total + COLLAPSE_BLOCK - 1u) / COLLAPSE_BLOCK) B.sums[threadIdx.x] = s_sums[threadIdx.x];
		L = N;
		// dec/info/sums of the next level are read by other threads of THIS workgroup (the barrier's workgroup-scope fence
		// covers that) or by the next launch (the kernel boundary does). A device-scope __threadfence() here wrote back and
		// invalidated the L2 at every level: ~25 us per level, a fifth of a 1M-triangle build.
		__syncthreads();
	}
	if (threadIdx.x == 0) {
		ring[(step + 1u) % COLLAPSE_RING] = L;
		if (host_out) *host_out = L;              // (pinned host memory: the last launch of a round)
	}
}

// ---- tile-local collapse (binary -> 4-wide): what k_count_tile and k_collapse_tile share ----
// A binary node whose sorted range lies inside one tile (a node pass 1 finishes) is never opened INSIDE a wide node that
// lies above the tile: the maximal such subtrees ("tile roots") always become wide nodes of their own, so everything
// below them can be collapsed by the tile's workgroup alone, out of LDS, while the few nodes above (the ones pass 2
// finishes) go through the level-by-level collapse. Costs ~1 % more node visits than the unconstrained greedy collapse
// (scripts/bvh_lab.cpp -ft 1024) and replaces a dozen launches of dependent random reads over the whole tree.
//
// Chooses the (up to four) children of wide-node job b, a tile-contained binary node: its two children, then twice the
// largest-area child that is still an openable inner node -- the rule of collapse_open below, on LDS copies of the
// tile's child links and areas (lr_, area_ indexed by node - lo; open_area).
__device__ __forceinline__ int tile_open(int b, int lo, const int2 *lr_, const float *area_, int c[4])
{
	const int2 ch = lr_[b - lo];
	c[0] = ch.x; c[1] = ch.y; c[2] = 0; c[3] = 0;
	int nc = 2;
#pragma unroll
	for (int round = 0; round < 2; round++) {
		int best = -1;
		float best_area = 0.0f;
#pragma unroll
		for (int k = 0; k < 4; k++) {
			if (k >= nc || c[k] < 0) continue;
			const float a = area_[c[k] - lo];                              // <= 0: one leaf, not opened
			if (a > best_area) { best_area = a; best = k; }
		}
		if (best >= 0) {
			int bref = 0;
#pragma unroll
			for (int k = 0; k < 4; k++) if (k == best) bref = c[k];
			const int2 o = lr_[bref - lo];
#pragma unroll
			for (int k = 0; k < 4; k++) {
				if (k == best) c[k] = o.x;
				if (k == nc) c[k] = o.y;
			}
			nc++;
		}
	}
	return nc;
}

// The tile-local collapse: a SMALL workgroup per refit tile turns the tile's forest of finished binary subtrees into
// 4-wide nodes, out of LDS. Small on purpose: what a tile needs is a dozen rounds of a few dependent LDS reads each (which
// binary nodes become wide nodes is marked top-down from the tile roots, one level per round) -- latency, not throughput --
// so the chip is filled with many tiles at once (21 KB of LDS and one wave each: seven or more per CU) rather than with
// many threads per tile (a 1024-thread workgroup per tile left 90 % of its lanes waiting at barriers: 1.5 ms at 10M
// triangles; the level-by-level collapse over the whole tree, which this replaces, took 1.05 + 0.29 ms).
//   k_count_tile     marks, and counts the tile's wide nodes; a prefix sum over the counts (k_scan_tiles) gives every tile
//                    the number of its first node
//   k_collapse_tile  marks again (same code, same result), numbers the tile's wide nodes in pre-order and writes each of
//                    them ONCE and complete: boxes (the records pass 1 wrote), final child numbers, front-to-back order
//                    words and the 64-byte compressed copy (k_quantize would re-read what was just written). Dense: thread
//                    j makes node j of the tile. The roots of the forest are children of nodes the level-by-level collapse
//                    made before: their numbers are written into those nodes' child words.
#define TILE_THREADS 256       // k_collapse_tile: the first wave marks and numbers, all four finish nodes (k_count_tile: one wave)

// loads the tile's child links and areas into LDS and its roots (root_list / nroots: k_refit_tile listed them -- the subtrees
// its climbers carried to the tile's borders and the halves that are in the tile of nodes that reach beyond it; their order does
// not matter: numbers come from the tree alone. Inner nodes with disjoint ranges: at most REFIT_TILE / 2 of them). Nothing
// pass 2 writes is used: the area of a node that pass 1 did not complete is -1, and no root's subtree leads to one.
// (THREADS = the workgroup's size. All of a thread's global loads are issued before the first one is used -- left as a loop the
// compiler waits for each position's loads before it asks for the next: 16 dependent memory round trips per thread in the
// 64-thread counting kernel, 22 us of a tile's 118 in k_collapse_tile.)
template <int THREADS>
__device__ __forceinline__ void tile_load(int lo, int hi, const int2 *lr, const uint2 *range, const float *area, const int *root_list, uint32_t nroots,
	int2 *s_lr, float *s_area, uint16_t *s_start, int *s_roots, uint32_t *s_nroots)
{
	constexpr int ITER = REFIT_TILE / THREADS;
	const int t = (int)threadIdx.x;
	if (t == 0) *s_nroots = nroots;
	int2 v_lr[ITER];
	uint2 v_rg[ITER];
	float v_a[ITER];
#pragma unroll
	for (int q = 0; q < ITER; q++) {
		const int i = lo + t + q * THREADS;
		const int ic = i < hi ? i : (hi > lo ? hi - 1 : lo);       // (a position that exists: the values of positions beyond the tile are not used)
		v_lr[q] = lr[ic]; v_a[q] = area[ic];
		v_rg[q] = s_start ? range[ic] : make_uint2(0u, 0u);
	}
	for (uint32_t j = (uint32_t)t; j < nroots; j += THREADS) s_roots[j] = root_list[lo + (int)j];
#pragma unroll
	for (int q = 0; q < ITER; q++) {
		const int k = t + q * THREADS, i = lo + k;
		// (entries of nodes that are not complete inside the tile are never followed; their ranges may be anything)
		if (i < hi) { s_lr[k] = v_lr[q]; s_area[k] = v_a[q]; }
		else { s_lr[k] = make_int2(INT_MIN, INT_MIN); s_area[k] = -1.0f; }
		if (s_start) s_start[k] = (uint16_t)((i < hi && (int)v_rg[q].x >= lo && (int)v_rg[q].x <= hi) ? (int)v_rg[q].x - lo : 0);
	}
	__syncthreads();
}

// Which binary nodes of the tile become wide nodes ("jobs"): breadth-first from the tile roots, by ONE wave (the first of the
// workgroup; the others wait at the caller's barrier) -- a level is a handful to a few hundred jobs, each a chain of four
// dependent LDS reads, so what counts is not to touch anything but the jobs: s_q[0 .. count) lists them level by level
// (node - lo), appended with the wave's own prefix sums (ballots), no barriers, no scan over the tile's 1024 positions per
// level (that form of this loop took 100 us per tile). Returns count.
//   s_spine / s_lvl / s_cnt may be NULL (counting only). s_spine[k]: how many jobs above node lo + k share its range start;
//   s_cnt (packed 16-bit counters): jobs per range start; with these two the caller numbers the jobs in the PRE-ORDER of
//   the forest (range start ascending, larger range first): every node after its parent, subtrees contiguous, numbers that
//   depend on the tree alone. s_lvl[k]: level of the node below its tile root (the root: 0); s_rootof[k]: which root that is
//   (its place in s_roots); s_rdepth[r]: the deepest level below root r -- where a root hangs in the tree is not known
//   here (the nodes above the tiles are collapsed at the same time, on another stream): k_top_finish adds the two.
__device__ __forceinline__ uint32_t tile_bfs(int lo, const int2 *s_lr, const float *s_area, const uint16_t *s_start, const int *s_roots, uint32_t nroots,
	uint16_t *s_q, uint16_t *s_spine, uint8_t *s_lvl, uint32_t *s_cnt, uint16_t *s_rootof, uint32_t *s_rdepth)
{
	const uint32_t lane = threadIdx.x & 63u;
	for (uint32_t r = lane; r < nroots; r += 64u) {
		const int k = s_roots[r] - lo;
		s_q[r] = (uint16_t)k;
		if (s_spine) {
			s_spine[k] = 0u;
			s_lvl[k] = 0u;
			s_rootof[k] = (uint16_t)r;
			s_rdepth[r] = 0u;
			atomicAdd(s_cnt + ((uint32_t)s_start[k] >> 1), (s_start[k] & 1u) ? 0x10000u : 1u);
		}
	}
	uint32_t begin = 0, end = nroots, tail = nroots;
	while (begin < end) {
		for (uint32_t j0 = begin; j0 < end; j0 += 64u) {
			const uint32_t j = j0 + lane;
			int c[4] = { -1, -1, -1, -1 };
			int nc = 0, t = 0;
			if (j < end) { t = (int)s_q[j]; nc = tile_open(lo + t, lo, s_lr, s_area, c); }
#pragma unroll
			for (int k = 0; k < 4; k++) {
				const bool inner = k < nc && c[k] >= 0 && s_area[c[k] - lo] > 0.0f;
				const unsigned long long m = __builtin_amdgcn_ballot_w64(inner);
				if (inner) {
					const uint32_t pos = tail + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
					const int ck = c[k] - lo;
					s_q[pos] = (uint16_t)ck;
					if (s_spine) {
						s_spine[ck] = s_start[ck] == s_start[t] ? (uint16_t)(s_spine[t] + 1u) : (uint16_t)0u;
						const uint32_t l = s_lvl[t] < 255u ? s_lvl[t] + 1u : 255u;
						s_lvl[ck] = (uint8_t)l;
						s_rootof[ck] = s_rootof[t];
						atomicMax(s_rdepth + s_rootof[t], l);
						atomicAdd(s_cnt + ((uint32_t)s_start[ck] >> 1), (s_start[ck] & 1u) ? 0x10000u : 1u);
					}
				}
				tail += (uint32_t)__builtin_popcountll(m);
			}
		}
		begin = end;
		end = tail;
	}
	return tail;
}

__global__ void __launch_bounds__(64) k_count_tile(int n, const int2 *lr, const float *area, const int *root_list, const uint32_t *tile_nroots, uint32_t *tile_count)
{
	__shared__ int2 s_lr[REFIT_TILE];
	__shared__ float s_area[REFIT_TILE];
	__shared__ uint16_t s_q[REFIT_TILE];
	__shared__ int s_roots[REFIT_TILE / 2];
	__shared__ uint32_t s_nroots;
	const int lo = (int)blockIdx.x * REFIT_TILE;
	const int hi = (lo + REFIT_TILE < n ? lo + REFIT_TILE : n) - 1;
	tile_load<64>(lo, hi, lr, nullptr, area, root_list, tile_nroots[blockIdx.x], s_lr, s_area, nullptr, s_roots, &s_nroots);
	if (threadIdx.x < 64u) {
		const uint32_t count = tile_bfs(lo, s_lr, s_area, nullptr, s_roots, s_nroots, s_q, nullptr, nullptr, nullptr, nullptr, nullptr);
		if (threadIdx.x == 0) tile_count[blockIdx.x] = count;
	}
}

// exclusive prefix sum of `v` over the threads of the workgroup (at most 1024; s_w: 16 words of LDS); *total = the sum
__device__ __forceinline__ uint32_t block_exclusive_scan_1024(uint32_t v, uint32_t *s_w, uint32_t *total)
{
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
	uint32_t inc = v;
	for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(inc, o); if (lane >= (uint32_t)o) inc += t; }
	__syncthreads();                                   // s_w may still be read from the previous use
	if (lane == 63u) s_w[wave] = inc;
	__syncthreads();
	uint32_t off = 0, tot = 0;
	for (uint32_t w = 0; w < waves; w++) { if (w < wave) off += s_w[w]; tot += s_w[w]; }
	*total = tot;
	return off + inc - v;
}

// exclusive prefix sums of the tiles' wide-node counts (one workgroup; a build has at most n / 1024 tiles); out[num] = total
__global__ void __launch_bounds__(1024) k_scan_tiles(const uint32_t *count, uint32_t num, uint32_t *base)
{
	__shared__ uint32_t s_w[16];
	uint32_t carry = 0;
	for (uint32_t at = 0; at < num; at += 1024u) {
		const uint32_t i = at + threadIdx.x;
		const uint32_t v = i < num ? count[i] : 0u;
		uint32_t total = 0;
		const uint32_t ex = block_exclusive_scan_1024(v, s_w, &total);
		if (i < num) base[i] = carry + ex;
		carry += total;
	}
	if (threadIdx.x == 0) base[num] = carry;
}

// Transposes the W x W matrix of 16-byte pieces that W neighbouring lanes hold (lane i of the group: pieces p[0 .. W) of ITS
// record) so that lane i ends up with piece i of each of the W records: p[k] = piece i of the record of lane k of the group.
// A store of p[k] then writes the whole record of lane k from W neighbouring lanes -- W * 16 contiguous bytes -- instead of one
// 16-byte piece per lane at the stride of the records (64 partial lines per instruction). All lanes of the wave take part.
template <int W>
__device__ __forceinline__ void transpose_pieces(uint4 (&p)[W])
{
	const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
	for (int s = 1; s < W; s <<= 1) {
		const bool up = (lane & (uint32_t)s) != 0u;
#pragma unroll
		for (int h = 0; h < W / 2; h++) {
			const int a = ((h & ~(s - 1)) << 1) | (h & (s - 1));       // the h-th piece number without bit s
			// (values first, then the select: `up ? p[a] : p[b]` selects between two ADDRESSES, and the array lands in scratch memory)
			uint4 &lo_p = p[a], &hi_p = p[a ^ s];
#define SWAP_PIECE(c_) { const uint32_t l_ = lo_p.c_, h_ = hi_p.c_; const uint32_t send = up ? l_ : h_; const uint32_t recv = (uint32_t)__shfl_xor((int)send, s); lo_p.c_ = up ? recv : l_; hi_p.c_ = up ? h_ : recv; }
			SWAP_PIECE(x) SWAP_PIECE(y) SWAP_PIECE(z) SWAP_PIECE(w)
#undef SWAP_PIECE
		}
	}
}

#ifdef RTK_TILE_PHASES
__device__ unsigned long long g_tile_phase[8];
#define PHASE_MARK(i_) do { if (threadIdx.x == 0) ph[i_] = wall_clock64(); } while (0)
#else
#define PHASE_MARK(i_)
#endif
#ifdef RTK_TILE_WAVES
#define TILE_WAVES_ATTR __attribute__((amdgpu_waves_per_eu(RTK_TILE_WAVES, RTK_TILE_WAVES)))
#else
#define TILE_WAVES_ATTR
#endif
__global__ void __launch_bounds__(TILE_THREADS) TILE_WAVES_ATTR k_collapse_tile(DevTri *tris, int n, const int2 *lr, const uint2 *range, const BinNode *bin, const float *area,
	const int *root_list, const uint32_t *tile_nroots, unsigned long long *root_info, const uint32_t *tile_base, uint32_t node_offset,
	DevNode *nodes, DevNodeQ *qnodes, uint32_t node_cap, DevSceneConsts *consts)
{
	__shared__ int2 s_lr[REFIT_TILE];          //  8 KB
	__shared__ float s_area[REFIT_TILE];       //  4 KB
	__shared__ uint16_t s_start[REFIT_TILE];   //  2 KB: first sorted triangle of node lo + k's range, minus lo
	__shared__ uint16_t s_base[REFIT_TILE];    //  2 KB: jobs whose range starts at lo + k, then their exclusive prefix sums
	__shared__ uint16_t s_round[REFIT_TILE], s_spine[REFIT_TILE], s_map[REFIT_TILE];   // the jobs in breadth-first order; ...; number -> node
	__shared__ uint8_t s_lvl[REFIT_TILE];
	__shared__ uint16_t s_rootof[REFIT_TILE];  //  2 KB: the tile root above node lo + k (its place in s_roots)
	__shared__ uint32_t s_rdepth[REFIT_TILE / 2];   //  2 KB: deepest level below each root
	__shared__ int s_roots[REFIT_TILE / 2];    //  2 KB: the tile roots
	__shared__ uint32_t s_nroots, s_count;
	const int lo = (int)blockIdx.x * REFIT_TILE;
	const int hi = (lo + REFIT_TILE < n ? lo + REFIT_TILE : n) - 1;
	const int t = (int)threadIdx.x;
#ifdef RTK_TILE_PHASES
	unsigned long long ph[6];
#endif
	PHASE_MARK(0);
	tile_load<TILE_THREADS>(lo, hi, lr, range, area, root_list, tile_nroots[blockIdx.x], s_lr, s_area, s_start, s_roots, &s_nroots);
	for (int k = t; k < REFIT_TILE; k += TILE_THREADS) s_base[k] = 0u;
	__syncthreads();
	PHASE_MARK(1);
	if (t < 64) {
		const uint32_t cnt = tile_bfs(lo, s_lr, s_area, s_start, s_roots, s_nroots, s_round, s_spine, s_lvl, reinterpret_cast<uint32_t *>(s_base), s_rootof, s_rdepth);
		// pre-order numbers: jobs that start further left (prefix sums over the per-start counters, 16 per lane) + jobs above
		// with the same start
		uint32_t sum = 0;
		uint32_t v[16];
#pragma unroll
		for (int q = 0; q < 16; q++) { v[q] = s_base[16 * t + q]; sum += v[q]; }
		uint32_t inc = sum;
		for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(inc, o); if (t >= o) inc += u; }
		uint32_t run = inc - sum;
#pragma unroll
		for (int q = 0; q < 16; q++) { s_base[16 * t + q] = (uint16_t)run; run += v[q]; }
		if (t == 0) s_count = cnt;
	}
	__syncthreads();
	PHASE_MARK(2);
	const uint32_t count = s_count;
	const uint32_t base = node_offset + tile_base[blockIdx.x];
#define TILE_LOCAL(k_) ((uint32_t)s_base[s_start[k_]] + (uint32_t)s_spine[k_])
	// the number of each root's node and the levels of its subtree, for the node above the tiles that it hangs in (k_top_finish)
	for (uint32_t r = (uint32_t)t; r < s_nroots; r += TILE_THREADS)
		root_info[s_roots[r]] = ((unsigned long long)(s_rdepth[r] + 1u) << 32) | (unsigned long long)(base + TILE_LOCAL(s_roots[r] - lo));
	// number -> binary node (s_map), then the nodes themselves, dense: thread j makes wide nodes j, j + blockDim, ... of the tile
	for (uint32_t j = (uint32_t)t; j < count; j += TILE_THREADS) { const uint32_t k = s_round[j]; s_map[TILE_LOCAL(k)] = (uint16_t)k; }
	__syncthreads();
	PHASE_MARK(3);
	bool misfit = false;
	// (every lane of a wave goes through the loop as long as one of them has a node to make: the stores below are shared)
	for (uint32_t j = (uint32_t)t; (j & ~63u) < count; j += TILE_THREADS) {
		const bool made = j < count;
		const int bk = made ? (int)s_map[j] : (int)s_map[0];
		int ch4[4];
		const int nc = tile_open(lo + bk, lo, s_lr, s_area, ch4);
		DevNode nd;
		// the boxes of the (up to four) children: a 32-byte binary record or a 48-byte triangle each. All twelve 16-byte loads
		// are issued before the first one is used (one memory round trip per node instead of one per child: the finishing loop
		// was 74 us of a tile's 118)
		float4 r0[4], r1[4], r2[4];
#pragma unroll
		for (int k = 0; k < 4; k++) {
			const bool leaf = k < nc && ch4[k] < 0;
			const float4 *src = leaf ? reinterpret_cast<const float4 *>(tris + (uint32_t)~ch4[k]) : reinterpret_cast<const float4 *>(bin + (k < nc ? ch4[k] : lo));
			r0[k] = src[0]; r1[k] = src[1];
			r2[k] = leaf ? src[2] : r1[k];
		}
#pragma unroll
		for (int k = 0; k < 4; k++) {
			float mn[3], mx[3];
			uint32_t ref;
			if (k >= nc) {
				mn[0] = mn[1] = mn[2] = 1.0f; mx[0] = mx[1] = mx[2] = -1.0f;      // inverted = never hit (rtk.c:1612-1620)
				ref = RTK_REF_NONE;
			} else if (ch4[k] < 0) {
				// a leaf of one triangle (marked as such by k_emit_tris): v0 | v1 | v2 in the first three floats of its rows (tri_box)
				mn[0] = fminf(fminf(r0[k].x, r1[k].x), r2[k].x); mx[0] = fmaxf(fmaxf(r0[k].x, r1[k].x), r2[k].x);
				mn[1] = fminf(fminf(r0[k].y, r1[k].y), r2[k].y); mx[1] = fmaxf(fmaxf(r0[k].y, r1[k].y), r2[k].y);
				mn[2] = fminf(fminf(r0[k].z, r1[k].z), r2[k].z); mx[2] = fmaxf(fmaxf(r0[k].z, r1[k].z), r2[k].z);
				ref = RTK_REF_LEAF | (uint32_t)~ch4[k];
			} else {
				const float4 b0 = r0[k], b1 = r1[k];                              // mn.xyz cnt_flag | mx.xyz cost
				mn[0] = b0.x; mn[1] = b0.y; mn[2] = b0.z; mx[0] = b1.x; mx[1] = b1.y; mx[2] = b1.z;
				if (s_area[ch4[k] - lo] > 0.0f) ref = base + TILE_LOCAL(ch4[k] - lo);
				else {
					const uint2 lf = range[ch4[k]];                                // a subtree the SAH rule turned into one leaf
					if (made) mark_leaf(tris, lf);
					ref = RTK_REF_LEAF | lf.x;
				}
			}
			nd.bx[0][k] = mn[0]; nd.bx[1][k] = mx[0];
			nd.by[0][k] = mn[1]; nd.by[1][k] = mx[1];
			nd.bz[0][k] = mn[2]; nd.bz[1][k] = mx[2];
			nd.child[k] = ref;
		}
		child_order(nd, nd.order);
		DevNodeQ q;
		if (!quantize_node(nd, q) && made) misfit = true;
		// (a tree with more nodes than the scene's arrays were sized for drops the writes beyond them; the host repeats)
		// the stores: eight neighbouring lanes write one node (its eight 16-byte rows), four its compressed copy
		{
			uint4 p[8], pq[4];
#define ROW_F(a_) make_uint4(__float_as_uint((a_)[0]), __float_as_uint((a_)[1]), __float_as_uint((a_)[2]), __float_as_uint((a_)[3]))
#define ROW_U(a_) make_uint4((a_)[0], (a_)[1], (a_)[2], (a_)[3])
			p[0] = ROW_F(nd.bx[0]); p[1] = ROW_F(nd.bx[1]); p[2] = ROW_F(nd.by[0]); p[3] = ROW_F(nd.by[1]);
			p[4] = ROW_F(nd.bz[0]); p[5] = ROW_F(nd.bz[1]); p[6] = ROW_U(nd.child); p[7] = ROW_U(nd.order);
			pq[0] = make_uint4(__float_as_uint(q.org[0]), __float_as_uint(q.org[1]), __float_as_uint(q.org[2]), __float_as_uint(q.scale[0]));
			pq[1] = make_uint4(__float_as_uint(q.scale[1]), __float_as_uint(q.scale[2]), q.q[0][0], q.q[0][1]);
			pq[2] = make_uint4(q.q[1][0], q.q[1][1], q.q[2][0], q.q[2][1]);
			pq[3] = ROW_U(q.child);
#undef ROW_F
#undef ROW_U
			transpose_pieces<8>(p);
			transpose_pieces<4>(pq);
			const uint32_t lane = (uint32_t)t & 63u, j0 = j - lane;
#pragma unroll
			for (uint32_t k = 0; k < 8u; k++) {
				const uint32_t jn = j0 + (lane & ~7u) + k;                                           // the node of lane k of this group of eight
				if (jn < count && base + jn < node_cap) reinterpret_cast<uint4 *>(nodes + base + jn)[lane & 7u] = p[k];
			}
#pragma unroll
			for (uint32_t k = 0; k < 4u; k++) {
				const uint32_t jn = j0 + (lane & ~3u) + k;
				if (jn < count && base + jn < node_cap) reinterpret_cast<uint4 *>(qnodes + base + jn)[lane & 3u] = pq[k];
			}
		}
	}
#undef TILE_LOCAL
	if (misfit) atomicAdd(&consts->qnode_misfits, 1u);
#ifdef RTK_TILE_PHASES
	__syncthreads();
	PHASE_MARK(4);
	if (threadIdx.x == 0) {
		for (int i = 0; i < 4; i++) atomicAdd(&g_tile_phase[i], ph[i + 1] - ph[i]);
		atomicAdd(&g_tile_phase[4], 1ull);
		atomicAdd(&g_tile_phase[5], (unsigned long long)count);
		atomicMax(&g_tile_phase[6], ((ph[4] - ph[0]) << 32) | blockIdx.x);
		atomicMax(&g_tile_phase[7], ((ph[4] - ph[3]) << 32) | count);
	}
#endif
}

// The nodes above the tiles, from the workspace to their places in the scene's arrays, complete: node 0 stays the root, the
// others go BEHIND the tiles' nodes ([1, 1 + *tiles_total): k_collapse_tile, which ran beside the collapse of these) -- so
// neither of the two collapses has to wait for the other one's node count. Child words: a node above the tiles moves with
// the rest, a tile root gets the number k_collapse_tile gave it (root_info), leaves stay. Order words, compressed copy, scene
// bound (node 0) as k_quantize does them; the depth of the tree = the deepest (level of a node here + levels of a tile subtree).
__global__ void __launch_bounds__(256) k_top_finish(const DevNode *top, const uint4 *tile_refs, const uint32_t *level, uint32_t count, const uint32_t *tiles_total,
	const unsigned long long *root_info, DevNode *nodes, DevNodeQ *qnodes, uint32_t node_cap, DevSceneConsts *consts, uint32_t *depth_word)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	uint32_t deepest = 0u;
	bool misfit = false;
	if (i < count) {
		const uint32_t shift = *tiles_total;
		DevNode nd = top[i];
		const uint4 tr4 = tile_refs[i];
		const uint32_t tr[4] = { tr4.x, tr4.y, tr4.z, tr4.w };
		const uint32_t lvl = level[i];
		deepest = lvl + 1u;                                                       // (the scene's depth counts levels from 1)
#pragma unroll
		for (int k = 0; k < 4; k++) {
			if (tr[k]) {
				const unsigned long long info = root_info[tr[k] - 1u];
				nd.child[k] = (uint32_t)info;
				const uint32_t d = lvl + 1u + (uint32_t)(info >> 32);
				deepest = deepest > d ? deepest : d;
			} else if (nd.child[k] != RTK_REF_NONE && !(nd.child[k] & RTK_REF_LEAF)) nd.child[k] += shift;   // (never the root)
		}
		child_order(nd, nd.order);
		if (i == 0u) {
			const float b = root_bound(nd, 0.0f);
			consts->bound_raw = b;
			consts->bound_abs = fmaxf(b, 1.0f);
		}
		DevNodeQ q;
		misfit = !quantize_node(nd, q);
		const uint32_t at = i ? i + shift : 0u;
		if (at < node_cap) { nodes[at] = nd; qnodes[at] = q; }
	}
	if (misfit) atomicAdd(&consts->qnode_misfits, 1u);
	for (int o = 32; o > 0; o >>= 1) { const uint32_t u = __shfl_xor(deepest, o); deepest = deepest > u ? deepest : u; }
	if ((threadIdx.x & 63u) == 0u && deepest) atomicMax(depth_word, deepest);
}

} // namespace

namespace rtk_bld {

// ---- 8 collapse ----
// The node arrays of the scene, [DevNode x node_cap | DevNodeQ x node_cap], are allocated before the collapse -- the GPU is still
// busy with the refit -- at the size 4-wide trees over n triangles usually have (0.47 n on the benchmark scenes), and the
// collapse writes its nodes straight into them. A tree with more nodes than that drops the writes beyond the capacity
// (the kernels check) and is collapsed once more: into an exact allocation (tile mode) or into the workspace.
// (no node memory afterwards: the estimate could not be allocated -- a dry round gives the exact size)
void alloc_node_estimate(Build &b)
{
	b.node_cap = plan_first_node_capacity(b.n, b.knobs.est_div);
	if (!b.node_alloc()) { (void)hipGetLastError(); b.node_cap = 0; }
}

// The level-by-level collapse into `target` (room for `cap` nodes; more are counted but not written). False: a launch or the
// wait failed (nothing is cleaned up here). b.h_state: the last level, with the number of nodes.
static bool run_collapse(Build &b, DevNode *target, uint32_t cap, uint64_t jobs_hint)
{
	const hipStream_t bs = b.bs;
	const unsigned big_blocks = (unsigned)std::min<uint64_t>((jobs_hint + COLLAPSE_BLOCK - 1) / COLLAPSE_BLOCK, (uint64_t)b.num_cus * 16);
	unsigned big_levels = plan_big_levels(jobs_hint);
	const CollapseBufs cb = { b.at<int>(b.L.jobs), b.at<int4>(b.L.dec), b.at<uint32_t>(b.L.info), b.at<uint32_t>(b.L.sums) };
	LevelState *d_ring = b.at<LevelState>(b.L.ring);
	uint32_t step = 0;
	for (unsigned round = 0;; round++) {
		hipLaunchKernelGGL(k_collapse_small, dim3(1), dim3(COLLAPSE_SMALL), 0, bs, cb, d_ring, step++, 16u, b.d_lr, b.d_range, b.d_bin, b.d_tris, target, cap, b.d_root, b.top_aux, (LevelState *)nullptr);
		for (unsigned k = 0; k < big_levels; k++) {
			// number the level of ring entry `step` (-> entry step + 1: the next level, not opened yet), then open that
			hipLaunchKernelGGL(k_collapse_number, dim3(big_blocks), dim3(COLLAPSE_BLOCK), 0, bs, cb, d_ring, step, target, cap);
			step++;
			hipLaunchKernelGGL(k_collapse_open, dim3(big_blocks), dim3(COLLAPSE_BLOCK), 0, bs, cb, d_ring, step, b.d_lr, b.d_range, b.d_bin, b.d_tris, target, cap, b.top_aux);
		}
		// (the level the round ends at goes straight into pinned host memory)
		hipLaunchKernelGGL(k_collapse_small, dim3(1), dim3(COLLAPSE_SMALL), 0, bs, cb, d_ring, step++, 16u, b.d_lr, b.d_range, b.d_bin, b.d_tris, target, cap, b.d_root, b.top_aux, &b.results->level);
		if (hipGetLastError() != hipSuccess || hipStreamSynchronize(bs) != hipSuccess) return false;
		memcpy(&b.h_state, const_cast<const LevelState *>(&b.results->level), sizeof(b.h_state));
		if (b.h_state.count == 0) return true;
		if (round > 4096) return false;
		big_levels = 4;
	}
}

// Tile mode, called by the refit between its two passes: how many wide nodes every tile makes, and where they start (the tiles' nodes
// themselves: collapse_tiles). b.cs: the side stream if it could be forked off, else the build's.
void count_tiles(Build &b)
{
	Workspace &ws = *b.ws;
	const hipStream_t bs = b.bs;
	const uint32_t num_tiles = b.plan.num_tiles;
	// how many wide nodes every tile makes, and where they start, then (collapse_tiles, once the node arrays are allocated) the tiles' nodes
	// themselves: on a stream of their own, beside pass 2 of the refit and the collapse of the nodes above the tiles -- a chain of
	// latency-bound launches with host round trips between them, 0.3 ms at 10M triangles in which the chip would have next to
	// nothing to do. (The tiles' kernels read what pass 1 wrote and nothing that pass 2 writes: k_refit_tile lists the roots.)
	if (!ws.side && (hipStreamCreateWithFlags(&ws.side, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&ws.fork, hipEventDisableTiming) != hipSuccess ||
			hipEventCreateWithFlags(&ws.join, hipEventDisableTiming) != hipSuccess)) {
		(void)hipGetLastError();
		if (ws.side) (void)hipStreamDestroy(ws.side);
		ws.side = nullptr;                       // (events created so far are kept for the next attempt: a handful of bytes)
	}
	b.forked = ws.side && hipEventRecord(ws.fork, bs) == hipSuccess && hipStreamWaitEvent(ws.side, ws.fork, 0) == hipSuccess;
	b.cs = b.forked ? ws.side : bs;
	hipLaunchKernelGGL(k_count_tile, dim3(num_tiles), dim3(64), 0, b.cs, (int)b.n, b.d_lr, b.d_area, b.d_root_list, b.d_tile_nroots, b.d_tile_count);
	hipLaunchKernelGGL(k_scan_tiles, dim3(1), dim3(1024), 0, b.cs, b.d_tile_count, num_tiles, b.d_tile_base);
	if (b.forked) b.side_busy = true;
}

// Tile mode: the tiles' nodes by k_collapse_tile beside the level-by-level collapse of the nodes above them (into the workspace),
// then k_top_finish moves those behind the tiles' nodes. Once more into an exact allocation if the estimate was too small.
// b.tiles_done stays false if there are more nodes above the tiles than the workspace holds: collapse_levels does everything then.
bool collapse_tiles(Build &b)
{
	Workspace &ws = *b.ws;
	const hipStream_t bs = b.bs;
	const uint32_t num_tiles = b.plan.num_tiles;
	BuildResults *const results = b.results;
	DevSceneConsts *consts = const_cast<DevSceneConsts *>(b.ds->view.consts);
	unsigned long long *d_root_info = b.at<unsigned long long>(b.L.root_info);      // what k_collapse_tile tells k_top_finish about the tile roots
	uint32_t top_nodes = 0;
	for (int attempt = 0;; attempt++) {
		DevNode *d_nodes_ = (DevNode *)b.node_mem;
		DevNodeQ *d_qnodes_ = (DevNodeQ *)(d_nodes_ + b.node_cap);
		// the tiles' nodes, numbers 1 ... (0 is the root): beside the collapse of the nodes above them the first time
		const hipStream_t ts = attempt == 0 ? b.cs : bs;
		hipLaunchKernelGGL(k_collapse_tile, dim3(num_tiles), dim3(TILE_THREADS), 0, ts, b.d_tris, (int)b.n, b.d_lr, b.d_range, b.d_bin, b.d_area, b.d_root_list, b.d_tile_nroots, d_root_info,
			b.d_tile_base, 1u, d_nodes_, d_qnodes_, (uint32_t)b.node_cap, consts);
		if (hipGetLastError() != hipSuccess) return b.fail("tile collapse launch");
		if (attempt == 0) {
			if (b.forked && hipEventRecord(ws.join, ws.side) != hipSuccess) return b.fail("event record");
			// the nodes above the tiles (~4 per tile; ~15 tile roots per tile hang below them), into the workspace
			if (!run_collapse(b, b.d_nodes_tmp, b.plan.top_cap, (uint64_t)num_tiles * 16u)) return b.fail("collapse");
			top_nodes = b.h_state.total_nodes;
			if (b.forked && hipStreamWaitEvent(bs, ws.join, 0) != hipSuccess) return b.fail("stream wait");
			if (top_nodes > b.plan.top_cap) break;           // (more of them than the workspace holds: everything level by level)
		}
		hipLaunchKernelGGL(k_top_finish, dim3((top_nodes + 255u) / 256u), dim3(256), 0, bs, b.d_nodes_tmp, b.top_aux.tile_refs, b.top_aux.level, top_nodes, b.d_tile_base + num_tiles, d_root_info,
			d_nodes_, d_qnodes_, (uint32_t)b.node_cap, consts, b.d_depth_word);
		hipLaunchKernelGGL(k_publish, dim3(1), dim3(1), 0, bs, results, b.d_tile_base + num_tiles, b.d_depth_word, consts);
		if (hipGetLastError() != hipSuccess || hipStreamSynchronize(bs) != hipSuccess) return b.fail("tile collapse");
		const uint32_t tile_nodes = results->tiles_total;      // wide nodes of all tiles
		b.depth = results->depth;
		b.equal_codes = results->equal_codes;
		b.ds->tree.consts_readback = results->consts;
#ifdef RTK_TILE_PHASES
		{
			unsigned long long h[8] = {}, z[8] = {};
			(void)hipMemcpyFromSymbol(h, HIP_SYMBOL(g_tile_phase), sizeof(h));
			(void)hipMemcpyToSymbol(HIP_SYMBOL(g_tile_phase), z, sizeof(z));
			if (h[4]) fprintf(stderr, "rtk_amd tile phases (10 ns ticks per tile): load %.0f bfs %.0f number %.0f finish %.0f; tiles %llu jobs/tile %.0f\n",
				(double)h[0] / h[4], (double)h[1] / h[4], (double)h[2] / h[4], (double)h[3] / h[4], h[4], (double)h[5] / h[4]);
			fprintf(stderr, "rtk_amd tile phases: slowest tile %llu ticks (tile %llu); slowest finish %llu ticks (%llu jobs)\n", h[6] >> 32, h[6] & 0xffffffffull, h[7] >> 32, h[7] & 0xffffffffull);
		}
#endif
		if (b.knobs.timing) {
			std::vector<uint32_t> hc(num_tiles + 1), hb(num_tiles + 1);
			(void)hipMemcpy(hc.data(), b.d_tile_count, (num_tiles) * 4, hipMemcpyDeviceToHost);
			(void)hipMemcpy(hb.data(), b.d_tile_base, (num_tiles + 1) * 4, hipMemcpyDeviceToHost);
			fprintf(stderr, "rtk_amd build: top %u tiles %u tail %u depth %u cap %zu counts %u %u %u bases %u %u %u\n", top_nodes, num_tiles, tile_nodes, b.depth, b.node_cap,
				hc[0], hc[1], hc[num_tiles - 1], hb[0], hb[1], hb[num_tiles]);
		}
		b.total_nodes = top_nodes + tile_nodes;
		if (b.total_nodes <= b.node_cap) {
			b.ds->view.nodes = d_nodes_;
			b.ds->view.qnodes = d_qnodes_;
			b.ds->view.num_nodes = b.total_nodes;
			b.ds->tree.first_top = 1u + tile_nodes;
			b.tiles_done = true;
			break;
		}
		if (attempt > 0) return b.fail("collapse (internal error: node count changed between two runs)");
		// the estimate was too small: an exact allocation, and the tiles and the move once more (the nodes above the tiles stay
		// where they are in the workspace; every pass is deterministic)
		b.node_cap = b.total_nodes;
		if (!b.node_alloc()) return b.fail("out of device memory");
		if (hipMemsetAsync(consts, 0, sizeof(DevSceneConsts), bs) != hipSuccess || hipMemsetAsync(b.d_depth_word, 0, 4, bs) != hipSuccess) return b.fail("memset");
	}
	if (b.tiles_done) b.stage("collapse");
	else {
		// (the other way needs the level-by-level kernels without their tile-mode arguments, and clean counters)
		b.top_aux = TopAux{ nullptr, nullptr };
		if (hipMemsetAsync(b.d_depth_word, 0, 4, bs) != hipSuccess) return b.fail("memset");
	}
	return true;
}

// Every node level by level, straight into the scene's node array; through the workspace and then into an exact allocation if
// the estimate was too small (or could not be had). The compressed nodes follow (rtk_quantize_nodes).
bool collapse_levels(Build &b)
{
	const hipStream_t bs = b.bs;
	bool in_place = b.node_mem != nullptr;
	if (!run_collapse(b, in_place ? (DevNode *)b.node_mem : b.d_nodes_tmp, in_place ? (uint32_t)b.node_cap : b.n, b.n)) return b.fail("collapse");
	if (in_place && b.h_state.total_nodes > b.node_cap) {
		// the estimate was too small: once more, into the workspace; then an exact allocation
		b.ds->mem.release(b.node_mem);
		b.node_mem = nullptr;
		in_place = false;
		if (!run_collapse(b, b.d_nodes_tmp, b.n, b.n)) return b.fail("collapse");
	}
	b.total_nodes = b.h_state.total_nodes;
	b.depth = b.h_state.depth;
	b.stage("collapse");
	if (!b.node_mem) {
		b.node_cap = b.total_nodes ? b.total_nodes : 1;
		if (!b.node_alloc()) return b.fail("out of device memory");
	}
	DevNode *d_nodes_ = (DevNode *)b.node_mem;
	b.ds->view.nodes = d_nodes_;
	b.ds->view.num_nodes = b.total_nodes;
	// compressed nodes beside the exact ones (and, if the collapse had to go through the workspace, the exact ones out of it)
	DevSceneConsts *consts = const_cast<DevSceneConsts *>(b.ds->view.consts);
	if (b.plan.tile_mode && hipMemsetAsync(consts, 0, sizeof(DevSceneConsts), bs) != hipSuccess) return b.fail("memset");     // (the way back from tile mode: its kernels have counted in there)
	if (rtk_quantize_nodes(b.ds, bs, in_place ? nullptr : b.d_nodes_tmp, (DevNodeQ *)(d_nodes_ + b.node_cap), 0.0f, 0xffffffffu, true, false) != RTK_AMD_OK) return b.give_up();
	hipLaunchKernelGGL(k_publish, dim3(1), dim3(1), 0, bs, b.results, (const uint32_t *)nullptr, b.d_depth_word, consts);
	if (hipGetLastError() != hipSuccess) return b.fail("publish launch");
	return true;
}

} // namespace rtk_bld
