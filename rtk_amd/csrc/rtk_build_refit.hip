// rtk_build_refit.hip -- the device build's middle stages (rtk_build_internal.h has the map): the triangle records in Morton order
// (made inside the refit's first kernel: that is why emit and refit share a file), the binary radix tree built bottom-up together
// with its boxes and the SAH leaf decision, the tiles' wide-node counts; and the side arrays of a finished scene.
#include "rtk_build_internal.h"

#include <math.h>

using namespace rtk_bld;

namespace {

// ---------------------------------------------------------------------------------- 5 emit

// the record of sorted triangle s: its positions gathered from the caller's position buffer (implicit float meshes), the staged records,
// or the records of the scene that is being rebuilt
__device__ __forceinline__ DevTri make_tri(const EmitSrc &e, uint32_t s)
{
	const uint32_t g = e.vals ? e.vals[s] : (uint32_t)(e.words[s] & 0xffffffull);     // packed sort words carry the index in their low 24 bits
	// mesh of global primitive g: last m with mesh_base[m] <= g
	uint32_t lo = 0, hi = e.num_meshes;
	while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (e.mesh_base[mid] <= g) lo = mid; else hi = mid; }
	const MeshSrc ms = e.old_tris ? MeshSrc{ nullptr, 0ull } : e.src[lo];
	DevTri t;
	if (e.old_tris) {
		const float4 *rec = reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(e.old_tris) + (size_t)e.slot_of[g] * RTK_TRI_STRIDE);
		const float4 a = rec[0], b = rec[1], c = rec[2];      // v0 prim | v1 flags | v2 spare
		t.v0[0] = a.x; t.v0[1] = a.y; t.v0[2] = a.z;
		t.v1[0] = b.x; t.v1[1] = b.y; t.v1[2] = b.z;
		t.v2[0] = c.x; t.v2[1] = c.y; t.v2[2] = c.z;
	} else if (ms.pos) {
		const size_t first = 3u * (size_t)(g - (uint32_t)e.mesh_base[lo]);
		const float *p0 = reinterpret_cast<const float *>(ms.pos + first * ms.stride);
		const float *p1 = reinterpret_cast<const float *>(ms.pos + (first + 1u) * ms.stride);
		const float *p2 = reinterpret_cast<const float *>(ms.pos + (first + 2u) * ms.stride);
		t.v0[0] = p0[0]; t.v0[1] = p0[1]; t.v0[2] = p0[2];
		t.v1[0] = p1[0]; t.v1[1] = p1[1]; t.v1[2] = p1[2];
		t.v2[0] = p2[0]; t.v2[1] = p2[1]; t.v2[2] = p2[2];
	} else {
		const float4 *rec = reinterpret_cast<const float4 *>(e.in_tris + g);
		const float4 a = rec[0], b = rec[1], c = rec[2];      // p0 p1 p2 p3 | p4 p5 p6 p7 | p8 vi0 vi1 vi2
		t.v0[0] = a.x; t.v0[1] = a.y; t.v0[2] = a.z;
		t.v1[0] = a.w; t.v1[1] = b.x; t.v1[2] = b.y;
		t.v2[0] = b.z; t.v2[1] = b.w; t.v2[2] = c.x;
	}
	// every record starts out as a leaf of its own (count 1, last of its leaf); the collapse rewrites only the
	// members of multi-triangle leaves
	t.prim = g;
	t.flags = (lo << 8) | RTK_TRI_LAST;   // mesh index above the flag bits (RTK_TRI_MESH_SHIFT)
	t.spare = 1u;
#if RTK_TRI_STRIDE == 64
	t.pad[0] = t.pad[1] = t.pad[2] = t.pad[3] = 0u;
#endif
	return t;
}

// stores the records of one wave (lane l: sorted triangle s_own, record t; n triangles in all). Every lane of the wave takes part.
__device__ __forceinline__ void store_tris(DevTri *tris, uint32_t s_own, uint32_t n, const DevTri &t)
{
#if RTK_TRI_STRIDE == 64
	if (s_own < n) tris[s_own] = t;
#else
	// The wave's 64 records are 192 16-byte pieces in a row: store k writes pieces 64 k + lane, 1 KB without a gap (a record per
	// lane is three stores of 16 bytes at a stride of 48: 64 partial lines each). Piece w of the record of lane r is number
	// 3 r + w: it goes to lane (3 r + w) mod 64 -- one to one, 3 and 64 have no common factor -- which receives one piece for
	// each of its three stores: the one of store k has w = (lane + k) mod 3 (64 = 1 mod 3).
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t piece[3][4] = {
		{ __float_as_uint(t.v0[0]), __float_as_uint(t.v0[1]), __float_as_uint(t.v0[2]), t.prim },
		{ __float_as_uint(t.v1[0]), __float_as_uint(t.v1[1]), __float_as_uint(t.v1[2]), t.flags },
		{ __float_as_uint(t.v2[0]), __float_as_uint(t.v2[1]), __float_as_uint(t.v2[2]), t.spare } };
	uint32_t got[3][4];
#pragma unroll
	for (uint32_t w = 0; w < 3u; w++) {
		const int to = (int)(((3u * lane + w) & 63u) << 2);
#pragma unroll
		for (int c = 0; c < 4; c++) got[w][c] = (uint32_t)__builtin_amdgcn_ds_permute(to, (int)piece[w][c]);
	}
	if (s_own - lane >= n) return;
	uint4 *out = reinterpret_cast<uint4 *>(tris + (s_own - lane));
	const uint32_t left = n - (s_own - lane);                               // records of this wave that exist
	const uint32_t w0 = lane % 3u;
#pragma unroll
	for (uint32_t k = 0; k < 3u; k++) {
		const uint32_t w = (w0 + k) % 3u, m = 64u * k + lane;
		uint4 v;
		const uint32_t a0 = got[0][0], a1 = got[1][0], a2 = got[2][0], b0 = got[0][1], b1 = got[1][1], b2 = got[2][1];
		const uint32_t c0 = got[0][2], c1 = got[1][2], c2 = got[2][2], d0 = got[0][3], d1 = got[1][3], d2 = got[2][3];
		v.x = w == 0u ? a0 : (w == 1u ? a1 : a2);
		v.y = w == 0u ? b0 : (w == 1u ? b1 : b2);
		v.z = w == 0u ? c0 : (w == 1u ? c1 : c2);
		v.w = w == 0u ? d0 : (w == 1u ? d1 : d2);
		if (m / 3u < left) out[m] = v;
	}
#endif
}

// (A/B only, RTK_AMD_FUSED_EMIT=0: the records are normally made inside k_refit_tile, which needs them next)
__global__ void k_emit_tris(EmitSrc e, uint32_t n, DevTri *tris)
{
	const uint32_t s_own = blockIdx.x * blockDim.x + threadIdx.x;
	if ((s_own & ~63u) >= n) return;                                            // (whole waves only: the stores are shared by the wave)
	const uint32_t s = s_own < n ? s_own : n - 1u;                              // (lanes behind the last triangle make a copy of it that is not written)
	store_tris(tris, s_own, n, make_tri(e, s));
	// (the side arrays -- original vertex indices, primitive -> slot, slot -> mesh / triangle -- were written here, 52 bytes per
	// triangle with one scattered word: rtk_scene_side_arrays makes them when something asks for a full rtk_hit, a validation or
	// an export, not in every build)
}

// The view's side arrays from the finished triangle records (DevTri carries the primitive id and the mesh index), once per scene.
__global__ void k_side_arrays(const DevTri *tris, uint32_t n, const unsigned long long *mesh_base, const uint32_t *vidx_in,
	uint32_t *vertex_index, uint32_t *prim_slot, uint32_t *slot_mesh, uint32_t *slot_tri)
{
	const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= n) return;
	const uint32_t *w = reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(tris) + (size_t)s * RTK_TRI_STRIDE);
	const uint32_t g = w[3], mesh = w[7] >> 8;
	const uint32_t tri = g - (uint32_t)mesh_base[mesh];
	for (uint32_t c = 0; c < 3u; c++) vertex_index[3 * (size_t)s + c] = vidx_in ? vidx_in[3 * (size_t)g + c] : 3u * tri + c;
	prim_slot[g] = s;
	slot_mesh[s] = mesh;
	slot_tri[s] = tri;
}

// ---------------------------------------------------------------------------------- 6 tree topology
// The binary radix tree over the sorted keys (Karras 2012 defines it) is not built by a pass of its own any more: the
// refit pass below builds it bottom-up while it merges boxes (Apetrei 2014). A finished subtree over the sorted range
// [L, R] looks at the two keys on either side of its borders: it is the LEFT child of node R if its right neighbour is
// the more similar one (longer common prefix), else the RIGHT child of node L-1 -- an inner node is numbered by its split
// position (node m separates sorted triangles m and m+1). Two subtrees meet at every node; the second to arrive merges
// and climbs on. Same tree as the top-down search gives, without the search (0.33 ms at 10M triangles) and without the
// parent arrays.
//
// similarity of sorted keys i and i+1: length of their common prefix; equal keys (only on the (key, index) pair path) are
// told apart by their positions, as if the position were appended to the key. -1 outside the array.
__device__ __forceinline__ int key_delta(const unsigned long long *keys, int n, int i)
{
	if (i < 0 || i >= n - 1) return -1;
	const unsigned long long a = keys[i], b = keys[i + 1];
	if (a == b) return 64 + __clz((unsigned)(i ^ (i + 1)));
	return __clzll((long long)(a ^ b));
}

// ---------------------------------------------------------------------------------- 7 refit + SAH

// Record of a single sorted triangle seen as a subtree.
__device__ __forceinline__ BinNode leaf_record(const DevTri *tris, uint32_t s, const BuildParams &bp)
{
	BinNode b;
	tri_box(tris, s, b.mn, b.mx);
	b.cnt_flag = 1u;
	b.cost = bp.cost_tri * half_area(b.mn, b.mx);
	return b;
}

__device__ __forceinline__ BinNode leaf_record_of(const DevTri &t, const BuildParams &bp)
{
	BinNode b;
#pragma unroll
	for (int a = 0; a < 3; a++) {
		b.mn[a] = fminf(fminf(t.v0[a], t.v1[a]), t.v2[a]);
		b.mx[a] = fmaxf(fmaxf(t.v0[a], t.v1[a]), t.v2[a]);
	}
	b.cnt_flag = 1u;
	b.cost = bp.cost_tri * half_area(b.mn, b.mx);
	return b;
}

// Record of an inner node from the records of its two children: box union, triangle count and the SAH
// decision "one leaf of cnt triangles" vs "split" (cost model of rtk.c:931-949 with working constants,
// SURVEY.md appendix B9). min/max/+ are commutative, so the result does not depend on which child is a.
__device__ __forceinline__ BinNode combine_records(const BinNode &a, const BinNode &b, const BuildParams &bp)
{
	BinNode out;
#pragma unroll
	for (int k = 0; k < 3; k++) { out.mn[k] = fminf(a.mn[k], b.mn[k]); out.mx[k] = fmaxf(a.mx[k], b.mx[k]); }
	const uint32_t cnt = (a.cnt_flag & 0x7fffffffu) + (b.cnt_flag & 0x7fffffffu);
	const float cost = a.cost + b.cost;
	const float area = half_area(out.mn, out.mx);
	const float split = bp.cost_node * area + cost;
	// (the size limit is tested by itself: with an infinite or NaN area -- non-finite vertices -- "INFINITY <= split" would
	// be true and the whole scene one leaf)
	const bool may_be_leaf = cnt <= bp.max_leaf;
	const float leaf = may_be_leaf ? bp.cost_tri * (float)cnt * area : INFINITY;
	out.cnt_flag = cnt | ((may_be_leaf && leaf <= split) ? 0x80000000u : 0u);
	out.cost = fminf(leaf, split);
	return out;
}

// what tile_open ranks openable children by: the half area of the node's box, never zero (a box flat on two axes must stay
// openable); negative for a subtree the SAH rule turned into one leaf
__device__ __forceinline__ float open_area(const BinNode &r)
{
	return (r.cnt_flag & 0x80000000u) ? -1.0f : fmaxf(half_area(r.mn, r.mx), 1e-37f);
}

// Pass 1, tile-local. The sorted triangles are cut into tiles of REFIT_TILE; one 1024-thread workgroup owns a tile and
// builds every inner node whose two children lie inside it (split positions lo .. hi-1 with ranges inside [lo, hi]):
// similarities, child links, range ends, arrival counters and the 32-B node records of the tile live in LDS, so a climb
// waits for no global memory, and the hand-off between the two subtrees that meet at a node never leaves the CU (the
// all-global version of round 1 cost ~14 memory-side atomics per node, 3.8 ms at 10M triangles). Finished nodes are
// written out once, coalesced. A subtree whose parent lies across the tile border is left for pass 2 as a "climber":
// (subtree, L, R), stored at the leaf that carried it.

// meet[node]: 0 until the first of the node's two subtrees has arrived, then (its reference << 32 | the range end it brings) + 1
// (never 0: a range end is below 2^32 - 1). Which side it is the second arriver knows: the other one.
__device__ __forceinline__ unsigned long long meet_word(int ref, int end) { return (((unsigned long long)(uint32_t)ref << 32) | (uint32_t)end) + 1ull; }

// emit.src != NULL: the kernel first MAKES the tile's triangle records (what k_emit_tris does: positions gathered in sorted order) and
// writes them out; each thread keeps its own in registers for the leaf record. A separate pass wrote 48 bytes per triangle that this
// one read straight back, and its gather (bound by the CU's vector memory pipe) ran apart from this kernel's climb (bound by LDS round
// trips): side by side on a CU's two workgroups the two overlap.
__global__ void __launch_bounds__(REFIT_BLOCK) k_refit_tile(DevTri *tris, int n, const unsigned long long *keys, int2 *lr, uint2 *range,
	BinNode *bin, Climb *climbers, unsigned long long *meet, int *climb_idx, uint32_t *tile_nclimb, int *root, BuildParams bp, float *area,
	uint32_t *equal_codes, int *root_list, uint32_t *tile_nroots, EmitSrc emit)
{
	__shared__ uint32_t s_nclimb, s_nroot;
	__shared__ BinNode s_bin[REFIT_TILE];      // 32 KB
	__shared__ uint32_t s_arrive[REFIT_TILE];
	__shared__ int2 s_lr[REFIT_TILE];                            // children of node lo + k (x left, y right)
	__shared__ int s_rl[REFIT_TILE], s_rr[REFIT_TILE];          // its range
	__shared__ int s_delta[REFIT_TILE + 1];                     // [k] = similarity across the border between lo+k-1 and lo+k
	const int lo = (int)blockIdx.x * REFIT_TILE;
	const int hi = (lo + REFIT_TILE < n ? lo + REFIT_TILE : n) - 1;     // last sorted triangle of the tile
	const int t = (int)threadIdx.x;
	DevTri mine = {};
	if (emit.src) {
		const uint32_t s_own = (uint32_t)(lo + t);
		mine = make_tri(emit, s_own < (uint32_t)n ? s_own : (uint32_t)n - 1u);
		store_tris(tris, s_own, (uint32_t)n, mine);      // (visible to the other waves of the workgroup behind the barrier below: the climb reads sibling leaves)
	}
	s_arrive[t] = 0u;
	if (t == 0) { s_nclimb = 0u; s_nroot = 0u; }
	s_lr[t] = make_int2(INT_MIN, INT_MIN);
	int my_delta = -1;
	if (lo + t - 1 <= hi) s_delta[t] = my_delta = key_delta(keys, n, lo + t - 1);
	if (t == 0 && hi - lo + 1 == REFIT_TILE) s_delta[REFIT_TILE] = key_delta(keys, n, hi);
	{
		// how many neighbours in sorted order share their whole Morton code (a common prefix of 40 bits or more: the packed
		// words carry the code above a 24-bit index, equal pair keys count 64+): where that is common the key was too narrow for
		// the scene -- a dense mesh in a corner of the scene box -- and the host builds again with the full 40 bits
		const unsigned long long same = __ballot(t > 0 && my_delta >= 40);
		if ((t & 63) == 0 && same) atomicAdd(equal_codes, (uint32_t)__popcll(same));
	}
	__syncthreads();
	const int i = lo + t;
	Climb left_over;
	left_over.cur_ref = INT_MIN; left_over.l = left_over.r = 0;
	if (i <= hi) {
		BinNode cur = emit.src ? leaf_record_of(mine, bp) : leaf_record(tris, (uint32_t)i, bp);
		int cur_ref = ~i, L = i, R = i;
		for (;;) {
			if (L == 0 && R == n - 1) { *root = cur_ref; break; }          // the whole scene inside one tile
			const int dl = s_delta[L - lo], dr = s_delta[R - lo + 1];
			const bool go_right = L == 0 || (R != n - 1 && dr > dl);        // (never equal for the borders of a real subtree)
			const int parent = go_right ? R : L - 1;
			if (parent < lo || parent >= hi) {                               // its other child lies in a neighbouring tile
				left_over.cur_ref = cur_ref; left_over.l = L; left_over.r = R;
				break;
			}
			const int k = parent - lo;
			if (go_right) { s_lr[k].x = cur_ref; s_rl[k] = L; } else { s_lr[k].y = cur_ref; s_rr[k] = R; }
			// (cur, if it is an inner node, sits in s_bin[cur_ref - lo] already: LDS is in order, the arrival below publishes it)
			const uint32_t old = __hip_atomic_fetch_add(&s_arrive[k], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
			if (old == 0u) break;                                            // first arriver: the sibling's thread carries on
			const int sib = go_right ? s_lr[k].y : s_lr[k].x;
			if (go_right) R = s_rr[k]; else L = s_rl[k];
			const BinNode other = sib < 0 ? leaf_record(tris, (uint32_t)~sib, bp) : s_bin[sib - lo];
			cur = combine_records(cur, other, bp);
			cur_ref = parent;
			s_bin[k] = cur;
		}
		// a climber is stored at the leaf that carried it, and where pass 2 and the tile collapse find the tile's climbers without
		// looking at every triangle: their positions, packed at the start of the tile's stretch of climb_idx (any order: the tree
		// does not depend on who climbs first). (Round 4 wrote all 1024 records of a tile, 12 bytes per triangle, and both
		// collapse kernels read them all back to find the two dozen that are there.)
		if (left_over.cur_ref != INT_MIN) {
			climbers[i] = left_over; climb_idx[lo + (int)atomicAdd(&s_nclimb, 1u)] = i;
			// tile mode: the subtree it carried to the border is one of the tile's roots (below), unless it is one leaf
			if (root_list && left_over.cur_ref >= 0 && open_area(cur) > 0.0f) root_list[lo + (int)atomicAdd(&s_nroot, 1u)] = left_over.cur_ref;
		}
	}
	__syncthreads();
	if (t == 0) tile_nclimb[blockIdx.x] = s_nclimb;
	// the finished records, 16 bytes per thread and store in the order they lie in LDS and in memory (a 32-byte record per
	// thread is two stores of half lines at a stride of 32)
	static_assert(sizeof(BinNode) == 32 && REFIT_BLOCK == REFIT_TILE, "two 16-byte pieces per record, one record per thread");
#pragma unroll
	for (int m = t; m < 2 * REFIT_TILE; m += REFIT_BLOCK) {
		const int rec = m >> 1;
		if (lo + rec < hi && s_arrive[rec] == 2u) reinterpret_cast<uint4 *>(bin + lo)[m] = reinterpret_cast<const uint4 *>(s_bin)[m];
	}
	// The tile's ROOTS (tile mode): the largest subtrees that lie inside the tile -- what its climbers carried to the border
	// (above) and the half that is here of a node whose other child arrives in pass 2 -- are all known now. The tile-local
	// collapse (k_count_tile, k_collapse_tile) reads this list and the records of the nodes that are complete here, nothing
	// that pass 2 writes: it runs beside pass 2 and the collapse of the nodes above the tiles. area < 0: not a node to open
	// (one leaf: open_area; not complete in this pass: -1).
	unsigned long long meet_here = 0ull;
	if (i < hi && s_arrive[t] == 2u) {
		if (area) area[i] = open_area(s_bin[t]);      // what the tile-local collapse ranks children by (4 bytes instead of the 32-byte record)
		lr[i] = s_lr[t];
		range[i] = make_uint2((uint32_t)s_rl[t], (uint32_t)s_rr[t]);
	} else if (i < hi) {
		if (area) area[i] = -1.0f;
		if (s_arrive[t] == 1u) {
			// one child came, the other one's subtree reaches into a neighbouring tile and arrives in pass 2: hand the half that
			// is here over in the form pass 2 uses (plain stores, the kernel boundary publishes them)
			const bool left_here = s_lr[t].x != INT_MIN;
			const int ref = left_here ? s_lr[t].x : s_lr[t].y, end = left_here ? s_rl[t] : s_rr[t];
			meet_here = meet_word(ref, end);
			if (root_list && ref >= 0 && open_area(s_bin[ref - lo]) > 0.0f) root_list[lo + (int)atomicAdd(&s_nroot, 1u)] = ref;
		}
	}
	// (every word of the tile's stretch is written: 0 = nobody has arrived at this node yet -- a memset of the whole array before
	// the kernel was 13 us at 10M triangles)
	if (i <= hi) meet[i] = meet_here;
	__syncthreads();
	if (t == 0 && tile_nroots) tile_nroots[blockIdx.x] = s_nroot;
}

// Pass 2: the few nodes whose children lie in different tiles (about two per tile plus chains). The hand-off of the
// first arriver's half -- its child reference, its range end and its 32-byte record -- has to cross CUs and XCDs here
// (per-CU L1 and per-XCD L2 are not coherent with each other): everything travels as 8-byte device-scope atomics, which
// execute at the memory side and are therefore coherent everywhere, and the arrival counter stays relaxed. Records
// written by pass 1 are plain stores made visible by the kernel boundary.
__device__ __forceinline__ void bin_store(BinNode *dst, const BinNode &v)
{
	unsigned long long *d = reinterpret_cast<unsigned long long *>(dst);
	const unsigned long long *sv = reinterpret_cast<const unsigned long long *>(&v);
#pragma unroll
	for (int k = 0; k < 4; k++) (void)__hip_atomic_exchange(d + k, sv[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// a real read-modify-write (hipcc folds fetch_add(p, 0) into an sc1 load): compare-and-swap of a value with itself
// returns the memory-side copy and never changes it
__device__ __forceinline__ unsigned long long mem_load64(unsigned long long *p)
{
	unsigned long long expect = ~0ull;
	(void)__hip_atomic_compare_exchange_strong(p, &expect, ~0ull, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	return expect;
}

__device__ __forceinline__ BinNode bin_load(BinNode *src)
{
	BinNode v;
	unsigned long long *d = reinterpret_cast<unsigned long long *>(src);
	unsigned long long *dv = reinterpret_cast<unsigned long long *>(&v);
#pragma unroll
	for (int k = 0; k < 4; k++) dv[k] = mem_load64(d + k);
	return v;
}

// One 64-wide workgroup per tile takes the tile's climbers (a few to a few dozen; climb_idx / tile_nclimb from pass 1) -- the
// launch used to cover every triangle to find them. Two subtrees meet at a node through ONE compare-and-swap on meet[node]:
// the first arriver swaps its (reference, range end) in and is done, the second gets the first one's word back (round 2: an
// exchange, a wait, a counter increment and a load -- three memory-side round trips per level of a chain that is ~20 levels deep).
// never_leaf (tile mode): a node finished here -- one that reaches across a tile border -- is never ONE leaf. Its finished
// children are the roots that k_collapse_tile turns into wide nodes (k_refit_tile counted them before this pass knew the
// node's cost), so the node above them must stay a node: a leaf of two or three triangles straddling a border would
// otherwise swallow a subtree that already has a number. (One such node at 17M triangles; found by the validator.)
__global__ void __launch_bounds__(64) k_refit_top(const DevTri *tris, int n, const unsigned long long *keys, const Climb *climbers, const int *climb_idx,
	const uint32_t *tile_nclimb, unsigned long long *meet, BinNode *bin, int2 *lr, uint2 *range, int *root, BuildParams bp, bool never_leaf)
{
	const int lo = (int)blockIdx.x * REFIT_TILE;
	const uint32_t count = tile_nclimb[blockIdx.x];
	for (uint32_t j = threadIdx.x; j < count; j += blockDim.x) {
		const Climb c = climbers[climb_idx[lo + (int)j]];
		int cur_ref = c.cur_ref, L = c.l, R = c.r;
		BinNode cur = cur_ref < 0 ? leaf_record(tris, (uint32_t)~cur_ref, bp) : bin[cur_ref];      // finished by pass 1: plain load
		for (;;) {
			if (L == 0 && R == n - 1) { *root = cur_ref; break; }
			const int dl = key_delta(keys, n, L - 1), dr = key_delta(keys, n, R);
			const bool go_right = L == 0 || (R != n - 1 && dr > dl);
			const int parent = go_right ? R : L - 1;
			// (an inner node finished in THIS pass has its record at the memory side already: bin_store and the wait below)
			unsigned long long seen = 0ull;
			(void)__hip_atomic_compare_exchange_strong(meet + parent, &seen, meet_word(cur_ref, go_right ? L : R), __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			if (seen == 0ull) break;                                           // first arriver: the sibling's thread carries on
			const unsigned long long theirs = seen - 1ull;
			const int sib = (int)(uint32_t)(theirs >> 32);
			if (go_right) R = (int)(uint32_t)theirs; else L = (int)(uint32_t)theirs;
			const BinNode other = sib < 0 ? leaf_record(tris, (uint32_t)~sib, bp) : bin_load(&bin[sib]);
			cur = combine_records(cur, other, bp);
			if (never_leaf) cur.cnt_flag &= 0x7fffffffu;
			bin_store(&bin[parent], cur);
			// topology of the finished node: read by the collapse only (later launches), plain stores
			lr[parent] = go_right ? make_int2(cur_ref, sib) : make_int2(sib, cur_ref);
			range[parent] = make_uint2((uint32_t)L, (uint32_t)R);
			cur_ref = parent;
			// everything this thread published is complete at the memory side before it announces the node one level up
			asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
		}
	}
}

} // namespace

namespace rtk_bld {

// ---- 5 emit: final triangle records in Morton order ----
bool emit(Build &b)
{
	const uint32_t n = b.n;
	b.mb.assign(b.mesh_base.begin(), b.mesh_base.end());
	// the triangle records; the mesh table (a few words the scene keeps: rtk_scene_side_arrays reads it)
	Carve c;
	const size_t o_tris = c.take((size_t)n * sizeof(DevTri)), o_mb = c.take(b.mb.size() * 8);
	char *tri_mem = b.dev_alloc(c.bytes);
	if (!tri_mem) return b.fail("out of device memory");
	b.d_tris = (DevTri *)(tri_mem + o_tris);
	unsigned long long *d_mesh_base = (unsigned long long *)(tri_mem + o_mb);
	MeshSrc *d_mesh_src = b.at<MeshSrc>(b.L.mesh_src);
	b.ds->tree.d_mesh_base = d_mesh_base;
	if (hipMemcpyAsync(d_mesh_base, b.mb.data(), b.mb.size() * 8, hipMemcpyHostToDevice, b.bs) != hipSuccess ||
		hipMemcpyAsync(d_mesh_src, b.mesh_src.data(), b.mesh_src.size() * sizeof(MeshSrc), hipMemcpyHostToDevice, b.bs) != hipSuccess) return b.fail("copy");
	// the triangle records in sorted order are made by k_refit_tile, which needs them next (RTK_AMD_FUSED_EMIT=0: by a pass of their own, A/B)
	b.emit_src = EmitSrc{ b.in_tris, d_mesh_src, b.vals, b.keys, d_mesh_base, (uint32_t)b.num_meshes, b.old_tris, b.slot_of };
	if (!b.knobs.fused_emit) {
		hipLaunchKernelGGL(k_emit_tris, dim3((n + 255u) / 256u), dim3(256), 0, b.bs, b.emit_src, n, b.d_tris);
		if (hipGetLastError() != hipSuccess) return b.fail("emit launch");
		b.emit_src.src = nullptr;
	}
	b.stage("emit");
	return true;
}

// ---- 6 + 7 tree topology and refit in one bottom-up pass (no separate tree-building kernel), then the nodes that cross tile borders ----
bool refit(Build &b)
{
	const hipStream_t bs = b.bs;
	const uint32_t num_tiles = b.plan.num_tiles;
	// what only the two passes of the refit hand to one another: the climbers pass 1 left at the tile borders, their positions packed
	// per tile (pass 2 finds them through these and d_tile_nclimb), and the words two subtrees meet through (the first n of `half`)
	Climb *d_climbers = b.at<Climb>(b.L.climbers);
	int *d_climb_idx = b.at<int>(b.L.arrive);
	uint32_t *d_tile_nclimb = b.at<uint32_t>(b.L.tile_nclimb);
	unsigned long long *d_half = b.at<unsigned long long>(b.L.half);
	if (hipMemsetAsync(b.d_depth_word, 0, 16, bs) != hipSuccess) return b.fail("memset");
	// (the scene's constants block: allocated and cleared here, not between the collapse and the last kernel -- a hipMalloc there was 40 us
	// in which the GPU waited; in tile mode also before the second stream forks off. The callee's error text stands.)
	if (rtk_scene_consts(b.ds, bs) != RTK_AMD_OK) return b.give_up();
	hipLaunchKernelGGL(k_refit_tile, dim3(num_tiles), dim3(REFIT_BLOCK), 0, bs, b.d_tris, (int)b.n, b.keys, b.d_lr, b.d_range,
		b.d_bin, d_climbers, d_half, d_climb_idx, d_tile_nclimb, b.d_root, b.bp, b.d_area, b.d_depth_word + 1, b.d_root_list,
		b.plan.tile_mode ? b.d_tile_nroots : (uint32_t *)nullptr, b.emit_src);
	// (tile mode: the tiles' node counts fork off here, beside pass 2: count_tiles, rtk_build_collapse.hip)
	if (b.plan.tile_mode) count_tiles(b);
	hipLaunchKernelGGL(k_refit_top, dim3(num_tiles), dim3(64), 0, bs, b.d_tris, (int)b.n, b.keys, d_climbers, d_climb_idx, d_tile_nclimb, d_half, b.d_bin, b.d_lr, b.d_range,
		b.d_root, b.bp, b.plan.tile_mode);
	if (hipGetLastError() != hipSuccess) return b.fail("refit");
	b.stage("refit");
	return true;
}

} // namespace rtk_bld

// The four side arrays of a device-built scene, made when something first needs them (the expansion of hit records into rtk_hit,
// rtk_trace_ray's one-ray kernel, the validator, the exporter). One kernel over the triangle records; the calling thread waits
// for it that one time, so that launches on any other stream may use the arrays as soon as this returns.
int rtk_scene_side_arrays(const rtk_dev_scene *ds_c, hipStream_t stream)
{
	rtk_dev_scene *ds = const_cast<rtk_dev_scene *>(ds_c);
	if (!ds) return RTK_AMD_ERR_BAD_ARG;
	std::lock_guard<std::mutex> lock(ds->side_mutex);
	if (ds->side_ready) return RTK_AMD_OK;
	const size_t n = ds->view.num_tris, np = ds->view.num_prims;
	Carve c;
	const size_t o_vidx = c.take(3 * n * 4), o_pslot = c.take(np * 4), o_smesh = c.take(n * 4), o_stri = c.take(n * 4);
	char *base = (char *)ds->mem.own(c.bytes, c.bytes);
	if (!base) { rtk_set_error("rtk_scene_side_arrays: %s", hipGetErrorString(hipGetLastError())); return RTK_AMD_ERR_OOM; }
	uint32_t *vertex_index = (uint32_t *)(base + o_vidx), *prim_slot = (uint32_t *)(base + o_pslot), *slot_mesh = (uint32_t *)(base + o_smesh), *slot_tri = (uint32_t *)(base + o_stri);
	if (n) {
		hipLaunchKernelGGL(k_side_arrays, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, ds->view.tris, (uint32_t)n, ds->tree.d_mesh_base, ds->tree.d_vidx_in,
			vertex_index, prim_slot, slot_mesh, slot_tri);
		if (hipGetLastError() != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) {
			rtk_set_error("rtk_scene_side_arrays: %s", hipGetErrorString(hipGetLastError()));
			ds->mem.release(base);
			return RTK_AMD_ERR_HIP;
		}
	}
	ds->view.vertex_index = vertex_index;
	ds->view.prim_slot = prim_slot;
	ds->view.slot_mesh = slot_mesh;
	ds->view.slot_tri = slot_tri;
	ds->side_ready = true;
	return RTK_AMD_OK;
}
