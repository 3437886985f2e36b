// rtk_split.hip -- rtk_dev_scene_split_leaves: every leaf of more than max_leaf triangles becomes a small subtree of 4-wide
// nodes with leaves of at most max_leaf, on the device, in place. What an imported blob needs (its builder made leaves of 4
// to 63 triangles; the packet kernels are made for leaves of at most three): DESIGN.md 3.4c.
//
//   k_split_stats     leaves, leaves over three, leaves over the limit and the largest leaf, from the sizes the first record of
//                     every leaf carries (DevTri.spare). Run before (nothing over the limit: the call is over) and after.
//   k_split_mark      one word per slot: 1 where a leaf over the limit begins. Its exclusive running sum numbers the big
//   scan_exclusive    leaves in the order of their first slot -- the order the new nodes are numbered in, whatever order the
//                     old nodes name the leaves in.
//   k_split_list      one lane per child word: a big leaf's first slot and who names it.
//   k_split_depth     the level of every old node, top-down, one sweep per level (for the new max_depth).
//   k_split_leaves    ONE WAVE PER BIG LEAF, run twice. The leaf's records are loaded one per lane; boxes and centroids go to
//                     LDS; every lane ranks its own centroid on the three axes (the 63 keys are ordered inside the wave without
//                     a sort); lane 0 walks the partition rule (rtk_split_rule.h, the text the CPU test runs) over the LDS
//                     copy. First run: the node count of the leaf and the depth its subtree reaches. After the running sum of
//                     the counts and the allocation of the longer node array, second run: the same walk, then all lanes emit
//                     -- a lane per child slot forms the exact box of its run of triangles (fminf / fmaxf over the vertices,
//                     the validator's rule) and stores the node; a lane per position pulls its record and side-array
//                     entries out of the lane that loaded them (no record is read after one was written) and stores them
//                     with the new end-of-leaf flag and leaf size; lane 0 patches the parent's child word.
//   k_quantize        (rtk_quant.hip) compressed nodes, order words and constants over the whole new tree.
// Everything is allocated before the scene is written; the old node arrays are freed at the end. DETERMINISTIC: which node
// gets which number follows from the two running sums, what is in it from the rule; no atomic decides anything but three
// maxima and the counts of k_split_stats.
#include "rtk_dev.h"
#include "rtk_split_rule.h"

#include <math.h>
#include <string.h>

#include <algorithm>

namespace {

#define SPLIT_WAVES 4                          // big leaves per workgroup of k_split_leaves
#define SCAN_THREADS 256
#define SCAN_ITEMS 4                           // words per thread of the running sum's first and last pass

enum { W_LEAVES, W_OVER3, W_OVER_LIMIT, W_LARGEST, W_WORDS };   // k_split_stats
struct SplitWords {                            // the small block the host reads back
	uint32_t before[W_WORDS], after[W_WORDS];
	uint32_t big_leaves;                       // total of the first running sum
	uint32_t nodes_added;                      // total of the second
	uint32_t depth;                            // deepest level a new node reaches
	uint32_t bound_bits;                       // largest |plane| of the new nodes as float bits (0x7f800000: one is not finite)
	uint32_t pad[4];
};
static_assert(sizeof(SplitWords) == 64, "SplitWords");

// a leaf the split may touch: a well-formed header over the limit
__device__ __forceinline__ bool is_big_leaf(const DevTri *tris, uint32_t num_tris, uint32_t s, uint32_t limit)
{
	const uint32_t cnt = tris[s].spare;
	return cnt > limit && cnt <= RTK_SPLIT_MAX_TRIS && (unsigned long long)s + cnt <= num_tris;
}

__global__ void __launch_bounds__(256) k_split_stats(const DevTri *tris, uint32_t num_tris, uint32_t limit, uint32_t *out)
{
	const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t cnt = s < num_tris ? tris[s].spare : 0u;
	const bool big = s < num_tris && is_big_leaf(tris, num_tris, s, limit);
	const unsigned long long leaves = __builtin_amdgcn_ballot_w64(cnt != 0u), over3 = __builtin_amdgcn_ballot_w64(cnt > 3u), over = __builtin_amdgcn_ballot_w64(big);
	uint32_t largest = cnt;
	for (int o = 32; o > 0; o >>= 1) { const uint32_t t = __shfl_xor(largest, o); largest = t > largest ? t : largest; }
	if ((threadIdx.x & 63u) == 0u && leaves) {
		atomicAdd(out + W_LEAVES, (uint32_t)__popcll(leaves));
		if (over3) atomicAdd(out + W_OVER3, (uint32_t)__popcll(over3));
		if (over) atomicAdd(out + W_OVER_LIMIT, (uint32_t)__popcll(over));
		atomicMax(out + W_LARGEST, largest);
	}
}

__global__ void __launch_bounds__(256) k_split_mark(const DevTri *tris, uint32_t num_tris, uint32_t limit, uint32_t *mark)
{
	const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
	if (s < num_tris) mark[s] = is_big_leaf(tris, num_tris, s, limit) ? 1u : 0u;
}

// ---- exclusive running sum of n words, in place: per workgroup, over the workgroups' totals (one workgroup), and the add

__device__ __forceinline__ uint32_t block_exclusive(uint32_t v, uint32_t *s, uint32_t *total)
{
	const uint32_t t = threadIdx.x;
	s[t] = v;
	__syncthreads();
	for (uint32_t o = 1; o < blockDim.x; o <<= 1) {
		const uint32_t x = t >= o ? s[t - o] : 0u;
		__syncthreads();
		s[t] += x;
		__syncthreads();
	}
	const uint32_t incl = s[t];
	*total = s[blockDim.x - 1u];
	__syncthreads();
	return incl - v;
}

__global__ void __launch_bounds__(SCAN_THREADS) k_scan_local(uint32_t *data, uint32_t n, uint32_t *block_total)
{
	__shared__ uint32_t s[SCAN_THREADS];
	const unsigned long long base = ((unsigned long long)blockIdx.x * SCAN_THREADS + threadIdx.x) * SCAN_ITEMS;
	uint32_t v[SCAN_ITEMS], sum = 0;
	for (int k = 0; k < SCAN_ITEMS; k++) { v[k] = base + k < n ? data[base + k] : 0u; sum += v[k]; }
	uint32_t total;
	uint32_t run = block_exclusive(sum, s, &total);
	for (int k = 0; k < SCAN_ITEMS; k++) { if (base + k < n) data[base + k] = run; run += v[k]; }
	if (threadIdx.x == 0u) block_total[blockIdx.x] = total;
}

__global__ void __launch_bounds__(1024) k_scan_totals(uint32_t *block_total, uint32_t blocks, uint32_t *grand_total)
{
	__shared__ uint32_t s[1024];
	uint32_t carry = 0;
	for (uint32_t first = 0; first < blocks; first += 1024u) {
		const uint32_t i = first + threadIdx.x;
		const uint32_t v = i < blocks ? block_total[i] : 0u;
		uint32_t total;
		const uint32_t run = block_exclusive(v, s, &total);
		if (i < blocks) block_total[i] = carry + run;
		carry += total;
	}
	if (threadIdx.x == 0u) *grand_total = carry;
}

__global__ void __launch_bounds__(SCAN_THREADS) k_scan_add(uint32_t *data, uint32_t n, const uint32_t *block_total)
{
	const unsigned long long base = ((unsigned long long)blockIdx.x * SCAN_THREADS + threadIdx.x) * SCAN_ITEMS;
	const uint32_t add = block_total[blockIdx.x];
	for (int k = 0; k < SCAN_ITEMS; k++) if (base + k < n) data[base + k] += add;
}

uint32_t scan_blocks(uint32_t n) { return (uint32_t)(((unsigned long long)n + SCAN_THREADS * SCAN_ITEMS - 1u) / (SCAN_THREADS * SCAN_ITEMS)); }

void scan_exclusive(uint32_t *data, uint32_t n, uint32_t *block_total, uint32_t *grand_total, hipStream_t stream)
{
	const uint32_t blocks = scan_blocks(n);
	if (blocks) hipLaunchKernelGGL(k_scan_local, dim3(blocks), dim3(SCAN_THREADS), 0, stream, data, n, block_total);
	hipLaunchKernelGGL(k_scan_totals, dim3(1), dim3(1024), 0, stream, block_total, blocks, grand_total);
	if (blocks) hipLaunchKernelGGL(k_scan_add, dim3(blocks), dim3(SCAN_THREADS), 0, stream, data, n, block_total);
}

// ---- the big leaves and who names them

__global__ void __launch_bounds__(256) k_split_list(const DevNode *nodes, uint32_t num_nodes, const DevTri *tris, uint32_t num_tris, uint32_t limit,
	const uint32_t *leaf_number, uint32_t num_big, uint32_t *leaf_first, uint32_t *leaf_parent)
{
	const unsigned long long e = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (e >= (unsigned long long)num_nodes * 4u) return;
	const uint32_t ref = nodes[e >> 2].child[e & 3u];
	if (ref == RTK_REF_NONE || !(ref & RTK_REF_LEAF)) return;
	const uint32_t first = ref & 0x7fffffffu;
	if (first >= num_tris || !is_big_leaf(tris, num_tris, first, limit)) return;
	const uint32_t j = leaf_number[first];
	if (j >= num_big) return;
	leaf_first[j] = first;
	leaf_parent[j] = (uint32_t)e;              // node * 4 + slot
}

// level[child] = level[node] + 1 for every node whose own level is known: after k sweeps the levels 1 .. k + 1 are final
__global__ void __launch_bounds__(256) k_split_depth(const DevNode *nodes, uint32_t num_nodes, uint32_t *level)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= num_nodes) return;
	const uint32_t l = i == 0u ? 1u : level[i];
	if (i == 0u) level[0] = 1u;
	if (l == 0u) return;
	const uint4 c = *reinterpret_cast<const uint4 *>(nodes[i].child);
	const uint32_t ref[4] = { c.x, c.y, c.z, c.w };
	for (int k = 0; k < 4; k++) if (ref[k] != RTK_REF_NONE && !(ref[k] & RTK_REF_LEAF) && ref[k] < num_nodes && ref[k] != 0u) level[ref[k]] = l + 1u;
}

// ---- one wave per big leaf

struct SplitArgs {
	DevTri *tris;
	uint32_t *vertex_index, *prim_slot, *slot_mesh, *slot_tri;   // the side arrays, or all NULL (a device-built scene that has not made them)
	DevNode *new_nodes;                        // EMIT: the longer array, the old nodes already in it
	const uint32_t *leaf_first, *leaf_parent, *level;
	uint32_t *node_count;                      // COUNT: written; EMIT: its running sum
	SplitWords *words;
	uint32_t num_tris, num_prims, num_big, limit, old_nodes, new_nodes_total;
};

template <bool EMIT>
__global__ void __launch_bounds__(64 * SPLIT_WAVES) k_split_leaves(SplitArgs a)
{
	__shared__ SplitLeaf s_in[SPLIT_WAVES];
	__shared__ SplitShape s_sh[SPLIT_WAVES];
	__shared__ SplitWork s_w[SPLIT_WAVES];
	__shared__ uint8_t s_head[SPLIT_WAVES][64], s_last[SPLIT_WAVES][64];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const uint32_t j = blockIdx.x * SPLIT_WAVES + wave;
	SplitLeaf &in = s_in[wave];
	SplitShape &sh = s_sh[wave];
	// (a wave without a leaf goes through the barriers with count 0; a leaf the list pass found nobody to name stays as it is)
	uint32_t first = 0, count = 0, parent = RTK_REF_NONE;
	if (j < a.num_big) {
		first = a.leaf_first[j];
		parent = a.leaf_parent[j];
		if (parent != RTK_REF_NONE && first < a.num_tris && is_big_leaf(a.tris, a.num_tris, first, a.limit)) count = a.tris[first].spare;
	}
	// the records, one per lane: they stay in registers until they are stored at their new place
	float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = r0, r2 = r0;
	if (lane < count) {
		const float4 *rec = reinterpret_cast<const float4 *>(a.tris + first + lane);
		r0 = rec[0]; r1 = rec[1]; r2 = rec[2];
	}
	{
		const float v[3][3] = { { r0.x, r0.y, r0.z }, { r1.x, r1.y, r1.z }, { r2.x, r2.y, r2.z } };
		bool finite = true;
		for (int ax = 0; ax < 3; ax++) {
			const float lo = fminf(fminf(v[0][ax], v[1][ax]), v[2][ax]), hi = fmaxf(fmaxf(v[0][ax], v[1][ax]), v[2][ax]);
			const float c = 0.5f * (lo + hi);
			in.lo[ax][lane] = lo; in.hi[ax][lane] = hi; in.cen[ax][lane] = c;
			in.order[ax][lane] = (uint8_t)lane;
			finite = finite && rtk_split_is_finite(c);
		}
		const unsigned long long bad = __builtin_amdgcn_ballot_w64(lane < count && !finite);
		if (lane == 0u) in.finite = bad == 0ull ? 1u : 0u;
		s_head[wave][lane] = 0; s_last[wave][lane] = 0;
	}
	__syncthreads();
	// every lane ranks its own centroid: the three orders, without a sort (ranks are distinct while the centroids are finite)
	if (lane < count && in.finite) {
		uint32_t rank[3];
		for (uint32_t ax = 0; ax < 3u; ax++) rank[ax] = rtk_split_rank(in, count, ax, lane);
		// (all ranks are taken before the first is stored: nobody reads `order` in between, but `cen` must not be behind a store)
		for (uint32_t ax = 0; ax < 3u; ax++) in.order[ax][rank[ax]] = (uint8_t)lane;
	}
	__syncthreads();
	if (lane == 0u) rtk_split_rule(in, count, a.limit, sh, s_w[wave]);
	__syncthreads();
	const uint32_t num_nodes = sh.num_nodes;
	if (!EMIT) {
		if (lane == 0u && j < a.num_big) {
			a.node_count[j] = num_nodes;
			if (num_nodes) atomicMax(&a.words->depth, a.level[parent >> 2] + sh.levels);
		}
		return;
	}
	// (a wave with nothing to emit still goes through the barrier below; that the nodes fit cannot fail: the same walk counted them)
	const uint32_t base = a.old_nodes + (j < a.num_big ? a.node_count[j] : 0u);
	const bool emit = num_nodes != 0u && (unsigned long long)base + num_nodes <= a.new_nodes_total;
	// ---- the nodes: a lane per child slot
	float plane_max = 0.0f;
	for (uint32_t e = lane; emit && e < num_nodes * 4u; e += 64u) {
		const uint32_t q = e >> 2, k = e & 3u;
		const SplitNode nd = sh.node[q];
		float mn[3] = { 1.0f, 1.0f, 1.0f }, mx[3] = { -1.0f, -1.0f, -1.0f };   // an empty slot: the inverted box every producer writes
		uint32_t ref = RTK_REF_NONE;
		if (k < nd.num_children) {
			const uint32_t from = nd.cut[k], to = nd.cut[k + 1u];
			for (int ax = 0; ax < 3; ax++) { mn[ax] = INFINITY; mx[ax] = -INFINITY; }
			for (uint32_t p = from; p < to; p++) {
				const uint32_t t = sh.perm[p];
				for (int ax = 0; ax < 3; ax++) { mn[ax] = fminf(mn[ax], in.lo[ax][t]); mx[ax] = fmaxf(mx[ax], in.hi[ax][t]); }
			}
			ref = nd.child[k] == RTK_SPLIT_CHILD_LEAF ? (RTK_REF_LEAF | (first + from)) : base + nd.child[k];
			if (nd.child[k] == RTK_SPLIT_CHILD_LEAF) { s_head[wave][from] = (uint8_t)(to - from); s_last[wave][to - 1u] = 1; }
			for (int ax = 0; ax < 3; ax++) {
				const float m = fmaxf(fabsf(mn[ax]), fabsf(mx[ax]));
				plane_max = (fabsf(mn[ax]) <= 1.7e38f && fabsf(mx[ax]) <= 1.7e38f) ? fmaxf(plane_max, m) : INFINITY;   // (the upload's rule for a plane that is not finite)
			}
		}
		DevNode *out = a.new_nodes + base + q;
		out->bx[0][k] = mn[0]; out->bx[1][k] = mx[0];
		out->by[0][k] = mn[1]; out->by[1][k] = mx[1];
		out->bz[0][k] = mn[2]; out->bz[1][k] = mx[2];
		out->child[k] = ref;
		out->order[k] = 0u;                    // (k_quantize writes the order words)
	}
	for (int o = 32; o > 0; o >>= 1) plane_max = fmaxf(plane_max, __shfl_xor(plane_max, o));
	if (lane == 0u && emit) atomicMax(&a.words->bound_bits, __float_as_uint(plane_max));   // (not negative: the bits order as the values)
	__syncthreads();
	if (!emit) return;
	// ---- the records and the side arrays: position `lane` takes what lane perm[lane] loaded
	const uint32_t src = lane < count ? sh.perm[lane] : lane;
	uint32_t vi[3] = { 0u, 0u, 0u }, smesh = 0u, stri = 0u;
	const bool side = a.vertex_index != nullptr;
	if (side && lane < count) {
		const size_t s = (size_t)first + lane;
		vi[0] = a.vertex_index[3 * s]; vi[1] = a.vertex_index[3 * s + 1]; vi[2] = a.vertex_index[3 * s + 2];
		smesh = a.slot_mesh[s]; stri = a.slot_tri[s];
	}
	float4 n0, n1, n2;
	n0.x = __shfl(r0.x, src); n0.y = __shfl(r0.y, src); n0.z = __shfl(r0.z, src); n0.w = __shfl(r0.w, src);
	n1.x = __shfl(r1.x, src); n1.y = __shfl(r1.y, src); n1.z = __shfl(r1.z, src); n1.w = __shfl(r1.w, src);
	n2.x = __shfl(r2.x, src); n2.y = __shfl(r2.y, src); n2.z = __shfl(r2.z, src); n2.w = __shfl(r2.w, src);
	for (int c = 0; c < 3; c++) vi[c] = __shfl(vi[c], src);
	smesh = __shfl(smesh, src); stri = __shfl(stri, src);
	if (lane < count) {
		const uint32_t slot = first + lane;
		const uint32_t prim = __float_as_uint(n0.w);
		n1.w = __uint_as_float((__float_as_uint(n1.w) & ~RTK_TRI_LAST) | (s_last[wave][lane] ? RTK_TRI_LAST : 0u));
		n2.w = __uint_as_float((uint32_t)s_head[wave][lane]);
		float4 *rec = reinterpret_cast<float4 *>(a.tris + slot);
		rec[0] = n0; rec[1] = n1; rec[2] = n2;
		if (side) {
			a.vertex_index[3 * (size_t)slot] = vi[0]; a.vertex_index[3 * (size_t)slot + 1] = vi[1]; a.vertex_index[3 * (size_t)slot + 2] = vi[2];
			a.slot_mesh[slot] = smesh; a.slot_tri[slot] = stri;
			if (prim < a.num_prims) a.prim_slot[prim] = slot;
		}
	}
	// ---- the parent names the subtree's root now
	if (lane == 0u) a.new_nodes[parent >> 2].child[parent & 3u] = base;
}

// device memory of one call, freed when it returns
struct Temporaries {
	void *small = nullptr, *tables = nullptr, *new_nodes = nullptr;
	~Temporaries() { if (small) (void)hipFree(small); if (tables) (void)hipFree(tables); if (new_nodes) (void)hipFree(new_nodes); }
};

// everything behind the argument checks, inside a ScenePass on the scene's device
int split_on_device(rtk_dev_scene *ds, uint32_t limit, hipStream_t stream, rtk_dev_split_info *info)
{
	const DevSceneView v = ds->view;
	info->max_depth_before = info->max_depth_after = ds->tree.max_depth;
	if (v.num_tris == 0u || v.num_nodes == 0u) return RTK_AMD_OK;
	Temporaries tmp;
	SplitWords h = {};
	RTK_PASS_CHECK("rtk_dev_scene_split_leaves", hipMalloc(&tmp.small, sizeof(SplitWords)));
	SplitWords *words = (SplitWords *)tmp.small;
	const unsigned tri_blocks = (v.num_tris + 255u) / 256u;
	RTK_PASS_CHECK("rtk_dev_scene_split_leaves", hipMemsetAsync(words, 0, sizeof(SplitWords), stream));
	hipLaunchKernelGGL(k_split_stats, dim3(tri_blocks), dim3(256), 0, stream, v.tris, v.num_tris, limit, words->before);
	RTK_PASS_CHECK("rtk_dev_scene_split_leaves", hipGetLastError());
	RTK_PASS_CHECK("rtk_dev_scene_split_leaves", hipMemcpyAsync(&h, words, sizeof(h), hipMemcpyDeviceToHost, stream));
	RTK_PASS_CHECK("rtk_dev_scene_split_leaves", hipStreamSynchronize(stream));
	info->largest_leaf_before = info->largest_leaf_after = h.before[W_LARGEST];
	const uint32_t num_big = h.before[W_OVER_LIMIT];
	if (num_big == 0u) return RTK_AMD_OK;      // nothing to split: no bit changes, nothing is dropped

	// ---- the big leaves in slot order, who names them, how many nodes each becomes, how deep that reaches
	const uint32_t tri_scan = scan_blocks(v.num_tris), big_scan = scan_blocks(num_big);
	Carve c;
	const size_t o_number = c.take((size_t)v.num_tris * 4), o_tri_totals = c.take(((size_t)tri_scan + 1) * 4), o_first = c.take((size_t)num_big * 4),
		o_parent = c.take((size_t)num_big * 4), o_count = c.take((size_t)num_big * 4), o_big_totals = c.take(((size_t)big_scan + 1) * 4),
		o_level = c.take((size_t)v.num_nodes * 4);
	RTK_PASS_CHECK("rtk_dev_scene_split_leaves", hipMalloc(&tmp.tables, c.bytes));
	char *tb = (char *)tmp.tables;
	uint32_t *leaf_number = (uint32_t *)(tb + o_number), *tri_totals = (uint32_t *)(tb + o_tri_totals), *leaf_first = (uint32_t *)(tb + o_first),
		*leaf_parent = (uint32_t *)(tb + o_parent), *node_count = (uint32_t *)(tb + o_count), *big_totals = (uint32_t *)(tb + o_big_totals),
		*level = (uint32_t *)(tb + o_level);
	hipLaunchKernelGGL(k_split_mark, dim3(tri_blocks), dim3(256), 0, stream, v.tris, v.num_tris, limit, leaf_number);
	scan_exclusive(leaf_number, v.num_tris, tri_totals, &words->big_leaves, stream);
	RTK_PASS_CHECK("rtk_dev_scene_split_leaves", hipMemsetAsync(tb + o_first, 0xff, o_count - o_first, stream));       // (RTK_REF_NONE: a leaf nobody names)
	RTK_PASS_CHECK("rtk_dev_scene_split_leaves", hipMemsetAsync(tb + o_count, 0, o_big_totals - o_count, stream));
	RTK_PASS_CHECK("rtk_dev_scene_split_leaves", hipMemsetAsync(level, 0, (size_t)v.num_nodes * 4, stream));
	hipLaunchKernelGGL(k_split_list, dim3((unsigned)(((size_t)v.num_nodes * 4 + 255) / 256)), dim3(256), 0, stream, v.nodes, v.num_nodes, v.tris, v.num_tris, limit,
		leaf_number, num_big, leaf_first, leaf_parent);
	for (uint32_t k = 0; k < ds->tree.max_depth; k++) hipLaunchKernelGGL(k_split_depth, dim3((v.num_nodes + 255u) / 256u), dim3(256), 0, stream, v.nodes, v.num_nodes, level);
	SplitArgs a = {};
	a.tris = const_cast<DevTri *>(v.tris);
	a.leaf_first = leaf_first; a.leaf_parent = leaf_parent; a.level = level; a.node_count = node_count; a.words = words;
	a.num_tris = v.num_tris; a.num_prims = v.num_prims; a.num_big = num_big; a.limit = limit; a.old_nodes = v.num_nodes;
	const unsigned leaf_blocks = (num_big + SPLIT_WAVES - 1u) / SPLIT_WAVES;
	hipLaunchKernelGGL((k_split_leaves<false>), dim3(leaf_blocks), dim3(64 * SPLIT_WAVES), 0, stream, a);
	scan_exclusive(node_count, num_big, big_totals, &words->nodes_added, stream);
	RTK_PASS_CHECK("rtk_dev_scene_split_leaves", hipGetLastError());
	RTK_PASS_CHECK("rtk_dev_scene_split_leaves", hipMemcpyAsync(&h, words, sizeof(h), hipMemcpyDeviceToHost, stream));
	RTK_PASS_CHECK("rtk_dev_scene_split_leaves", hipStreamSynchronize(stream));
	if (h.big_leaves != num_big) { rtk_set_error("rtk_dev_scene_split_leaves: internal error: %u big leaves counted, %u numbered", num_big, h.big_leaves); return RTK_AMD_ERR_HIP; }
	const uint64_t new_total = (uint64_t)v.num_nodes + h.nodes_added;
	if (new_total >= 0x7ffffff0ull) { rtk_set_error("rtk_dev_scene_split_leaves: %llu nodes are too many for 31-bit references", (unsigned long long)new_total); return RTK_AMD_ERR_UNSUPPORTED; }
	if (h.nodes_added == 0u) return RTK_AMD_OK;                     // (big leaves that nobody names: not a tree the upload accepts)

	// ---- the longer node arrays (exact nodes, compressed nodes behind them): the last thing that can be refused
	if (hipMalloc(&tmp.new_nodes, (size_t)new_total * (sizeof(DevNode) + sizeof(DevNodeQ))) != hipSuccess) {
		(void)hipGetLastError();
		rtk_set_error("rtk_dev_scene_split_leaves: out of device memory (%llu nodes)", (unsigned long long)new_total);
		return RTK_AMD_ERR_OOM;
	}
	DevNode *new_nodes = (DevNode *)tmp.new_nodes;
	DevNodeQ *new_qnodes = (DevNodeQ *)(new_nodes + new_total);

	// ---- from here on the scene is written
	std::lock_guard<std::mutex> side_lock(ds->side_mutex);          // (nobody makes the side arrays while they are permuted)
	RTK_PASS_CHECK("rtk_dev_scene_split_leaves", hipMemcpyAsync(new_nodes, v.nodes, (size_t)v.num_nodes * sizeof(DevNode), hipMemcpyDeviceToDevice, stream));
	a.new_nodes = new_nodes;
	a.new_nodes_total = (uint32_t)new_total;
	if (ds->side_ready && v.vertex_index && v.prim_slot && v.slot_mesh && v.slot_tri) {
		a.vertex_index = const_cast<uint32_t *>(v.vertex_index); a.prim_slot = const_cast<uint32_t *>(v.prim_slot);
		a.slot_mesh = const_cast<uint32_t *>(v.slot_mesh); a.slot_tri = const_cast<uint32_t *>(v.slot_tri);
	}
	hipLaunchKernelGGL((k_split_leaves<true>), dim3(leaf_blocks), dim3(64 * SPLIT_WAVES), 0, stream, a);
	hipLaunchKernelGGL(k_split_stats, dim3(tri_blocks), dim3(256), 0, stream, v.tris, v.num_tris, limit, words->after);
	RTK_PASS_CHECK("rtk_dev_scene_split_leaves", hipGetLastError());
	RTK_PASS_CHECK("rtk_dev_scene_split_leaves", hipMemcpyAsync(&h, words, sizeof(h), hipMemcpyDeviceToHost, stream));
	RTK_PASS_CHECK("rtk_dev_scene_split_leaves", hipStreamSynchronize(stream));

	// ---- the scene names the new arrays; compressed nodes, order words and constants over the whole new tree. Boxes of a blob
	// need not nest: the bound is the one the scene had (over every old node for an upload) widened by the new nodes' planes.
	const DevNode *old_nodes = v.nodes;
	const DevNodeQ *old_qnodes = ds->tree.qnodes_mem;
	float new_bound;
	memcpy(&new_bound, &h.bound_bits, 4);
	const float bound_hint = fmaxf(ds->tree.bound_raw, new_bound);      // (either may be INFINITY: the scene keeps to its exact nodes then)
	int rc;
	{
		std::lock_guard<std::mutex> lock(ds->scratch_mutex);      // (the trace path reads these fields under it)
		ds->view.nodes = new_nodes;
		ds->view.num_nodes = (uint32_t)new_total;
		ds->view.qnodes = new_qnodes;
		ds->tree.qnodes_mem = new_qnodes;
		rc = rtk_quantize_nodes(ds, stream, nullptr, new_qnodes, bound_hint, 0xffffffffu, false, true);
		if (rc == RTK_AMD_OK && hipStreamSynchronize(stream) != hipSuccess) { rtk_set_error("rtk_dev_scene_split_leaves: %s", hipGetErrorString(hipGetLastError())); rc = RTK_AMD_ERR_HIP; }
		if (rc == RTK_AMD_OK) rtk_quantize_finish(ds);
		ds->mem.adopt(tmp.new_nodes, (size_t)new_total * (sizeof(DevNode) + sizeof(DevNodeQ)));
		tmp.new_nodes = nullptr;
		const uint32_t depth = h.depth > ds->tree.max_depth ? h.depth : ds->tree.max_depth;
		ds->tree.max_depth = depth;
		ds->tree.big_leaf_fraction = h.after[W_LEAVES] ? (double)h.after[W_OVER3] / (double)h.after[W_LEAVES] : 0.0;
		// (appended nodes follow their parents in number, but a tile's node of a device-built tree may now name one outside its
		// run: the validator is told where the appended ones begin)
		if (ds->tree.first_split == 0u) ds->tree.first_split = v.num_nodes;
	}
	// the old arrays: an upload owns them one by one, a device build as one allocation (the compressed nodes behind the exact
	// ones: no entry of their own). What was derived from the old tree goes with them.
	ds->mem.release(old_nodes);
	ds->mem.release(old_qnodes);
	rtk_scene_forget_derived(ds, RTK_FORGET_TREE);
	if (rc != RTK_AMD_OK) return rc;
	info->leaves_split = num_big;
	info->nodes_added = h.nodes_added;
	info->largest_leaf_after = h.after[W_LARGEST];
	info->max_depth_after = ds->tree.max_depth;
	return RTK_AMD_OK;
}

} // namespace

extern "C" int rtk_dev_scene_split_leaves(rtk_dev_scene *ds, uint32_t max_leaf, rtk_dev_split_info *out, void *stream)
{
	// ---- everything that can be refused is refused here, before HIP is touched
	if (!ds) { rtk_set_error("rtk_dev_scene_split_leaves: NULL scene"); return RTK_AMD_ERR_BAD_ARG; }
	if (max_leaf > RTK_SPLIT_MAX_TRIS) { rtk_set_error("rtk_dev_scene_split_leaves: max_leaf %u (0 = the device builder's limit, else 1 .. 63)", max_leaf); return RTK_AMD_ERR_BAD_ARG; }
	if (out && out->struct_size < sizeof(rtk_dev_split_info)) {
		rtk_set_error("rtk_dev_scene_split_leaves: struct_size %u, rtk_dev_split_info has %zu bytes", out->struct_size, sizeof(rtk_dev_split_info));
		return RTK_AMD_ERR_BAD_ARG;
	}
	const uint32_t limit = max_leaf ? max_leaf : rtk_build_max_leaf();
	rtk_dev_split_info info = {};
	info.struct_size = out ? out->struct_size : (uint32_t)sizeof(info);
	info.max_leaf = limit;
	ScenePass pass(ds, stream);                                    // never beside a refit or a measurement
	if (!pass.on_device()) return RTK_AMD_ERR_NO_DEVICE;
	const int rc = pass.end(split_on_device(ds, limit, pass.stream, &info));
	if (rc != RTK_AMD_OK) return rc;
	info.split_ms = pass.ms();
	if (out) *out = info;
	return RTK_AMD_OK;
}
