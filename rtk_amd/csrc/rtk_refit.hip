// rtk_refit.hip -- new vertex positions for a finished device scene, in place (rtk_dev_scene_refit).
//
// The tree stays: slots, primitive ids, node numbers, child words, depth. What depends on positions is made again:
//   k_refit_tris    the 36 position bytes of every 48-byte triangle record, gathered through the vertex indices the scene
//                   recorded (view.vertex_index), prim / flags / spare kept;
//   k_refit_level   the child boxes of every node, bottom-up BY HEIGHT: a node's height is 0 if none of its children is an
//   k_refit_small   inner node, else 1 + the largest height among them, so every inner child of a node of height h was
//                   written by the launch of a lower height. One launch per height while a height has many nodes; the
//                   heights near the root (a few hundred nodes over a dozen heights) share ONE launch of one workgroup
//                   with a barrier between heights. Visibility between launches comes from the kernel boundary alone
//                   (the XCD L2s are not coherent; a counter per node climbing inside one launch would need an
//                   agent-scope release and acquire per hand-off);
//   k_quantize      (rtk_quant.hip) the 64-byte compressed nodes, the child order words and the scene constants.
// The heights and the node numbers grouped by them (RefitSchedule) are made by the first refit of a scene and kept.
// rtk_dev_scene_refit_meshes does the same for SOME meshes, with work in proportion to them: only their slots are regathered
// (k_refit_tris_listed, through per-mesh slot lists), every node above one of their leaves is marked dirty by climbing
// parent[] with plain idempotent stores, the schedule's node list is compacted by that flag with its order kept
// (k_dirty_count / k_dirty_scan / k_dirty_scatter), and boxes, compressed nodes and order words are remade for the dirty nodes
// alone, height by height as above. The result is bit for bit the full refit's; DESIGN.md 3.4a has the reasoning.
// A box is made by the validator's rule (rtk_validate.hip: fminf / fmaxf over the vertices of a leaf, over the non-empty
// slots of an inner child), so after a refit every box is the exact union of what is below it.
#include "rtk_dev.h"
#include "rtk_place_rule.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

namespace {

// where one mesh's positions are read from (device memory: the caller's own buffer or its copy in the workspace)
struct RefitMesh {
	const char *pos;
	unsigned long long stride;
	uint32_t f64;
	uint32_t pad;
};
static_assert(sizeof(RefitMesh) == 24, "RefitMesh");

#define REFIT_SMALL_THREADS 1024                 // k_refit_small: four lanes per node, 256 nodes per trip
#define REFIT_SMALL_LEVEL 1024u                // heights of at most this many nodes go to k_refit_small

// ---------------------------------------------------------------------------------- schedule (once per scene)

// One Jacobi sweep of height[i] = max over inner children (height[child] + 1). Heights only grow and a stale read is a
// lower bound, so the sweeps converge whatever a launch sees of its own stores: after sweep k every node of height < k is
// final (the kernel boundary makes sweep k - 1 visible).
__global__ void k_refit_heights(const DevNode *nodes, uint32_t n, uint32_t *height, uint32_t *changed)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const uint4 c = *reinterpret_cast<const uint4 *>(nodes[i].child);
	const uint32_t ref[4] = { c.x, c.y, c.z, c.w };
	uint32_t h = 0;
	for (int k = 0; k < 4; k++) {
		if (ref[k] == RTK_REF_NONE || (ref[k] & RTK_REF_LEAF) || ref[k] >= n) continue;
		const uint32_t hc = height[ref[k]] + 1u;
		h = hc > h ? hc : h;
	}
	if (h > height[i]) { height[i] = h; *changed = 1u; }
}

__global__ void k_refit_keys(const uint32_t *height, uint32_t n, unsigned long long *keys)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) keys[i] = ((unsigned long long)height[i] << 32) | i;
}

// sorted (height, node) words -> the node numbers, and where each height begins (every height up to the largest occurs: a
// node of height h has a child of height h - 1)
__global__ void k_refit_order(const unsigned long long *keys, uint32_t n, uint32_t *order, uint32_t *level_start)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const unsigned long long k = keys[i];
	const uint32_t h = (uint32_t)(k >> 32);
	order[i] = (uint32_t)k;
	if (i == 0u || (uint32_t)(keys[i - 1u] >> 32) != h) level_start[h] = i;
	if (i == n - 1u) level_start[h + 1u] = n;
}

// the largest vertex index each mesh's triangles use (how far a host-resident position buffer has to be copied)
__global__ void k_refit_max_vertex(const uint32_t *vertex_index, const uint32_t *slot_mesh, uint32_t n, uint32_t num_meshes, uint32_t *max_vertex)
{
	const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
	uint32_t mesh = 0xffffffffu, v = 0;
	if (s < n) {
		mesh = slot_mesh[s];
		const uint32_t a = vertex_index[3 * (size_t)s], b = vertex_index[3 * (size_t)s + 1], c = vertex_index[3 * (size_t)s + 2];
		v = a > b ? a : b;
		v = c > v ? c : v;
	}
	// slots follow the tree, so a wave is mostly inside one mesh: one atomic per wave then
	const uint32_t first = __shfl(mesh, 0);
	if (__builtin_amdgcn_ballot_w64(mesh != first) == 0ull) {
		for (int o = 32; o > 0; o >>= 1) { const uint32_t t = __shfl_xor(v, o); v = t > v ? t : v; }
		if ((threadIdx.x & 63u) == 0u && mesh < num_meshes) atomicMax(&max_vertex[mesh], v);
	} else if (mesh < num_meshes) atomicMax(&max_vertex[mesh], v);
}

// ---------------------------------------------------------------------------------- triangles

// MODE 0: every mesh has float positions, 1: every mesh doubles, 2: per mesh (RefitMesh::f64, a flag the host derived from
// validated type codes). Doubles are converted as k_ingest converts them.
// PLACED (the _placed entry points): place = the mesh's entry of a table beside `meshes`, applied to every vertex as soon as it
// is a float (rtk_place_rule.h, as k_ingest does in a placed build). The table lives in the borrowed workspace for the length of
// the call: the scene keeps no placement and allocates nothing for one.
template <int MODE, bool PLACED>
__device__ __forceinline__ void refit_tri(DevTri *tris, uint32_t s, const uint32_t *vertex_index, const RefitMesh &ms, const rtk_placement *place)
{
	rtk_placement pl;
	if (PLACED) pl = *place;
	const uint32_t vi[3] = { vertex_index[3 * (size_t)s], vertex_index[3 * (size_t)s + 1], vertex_index[3 * (size_t)s + 2] };
	float p[3][3];
	const bool f64 = MODE == 1 || (MODE == 2 && ms.f64 != 0u);
#pragma unroll
	for (int c = 0; c < 3; c++) {
		if (f64) {
			const double *q = reinterpret_cast<const double *>(ms.pos + (size_t)vi[c] * ms.stride);
			p[c][0] = (float)q[0]; p[c][1] = (float)q[1]; p[c][2] = (float)q[2];
		} else {
			const float *q = reinterpret_cast<const float *>(ms.pos + (size_t)vi[c] * ms.stride);
			p[c][0] = q[0]; p[c][1] = q[1]; p[c][2] = q[2];
		}
		if (PLACED) rtk_place_vertex(pl.m, p[c][0], p[c][1], p[c][2]);
	}
	// (the w lanes -- prim, flags, spare -- stay; a record is RTK_TRI_STRIDE bytes apart, 48 of them payload)
	float4 *rec = reinterpret_cast<float4 *>(tris + s);
	float4 r0 = rec[0], r1 = rec[1], r2 = rec[2];
	r0.x = p[0][0]; r0.y = p[0][1]; r0.z = p[0][2];
	r1.x = p[1][0]; r1.y = p[1][1]; r1.z = p[1][2];
	r2.x = p[2][0]; r2.y = p[2][1]; r2.z = p[2][2];
	rec[0] = r0; rec[1] = r1; rec[2] = r2;
}

template <int MODE, bool PLACED>
__global__ void __launch_bounds__(256) k_refit_tris(DevTri *tris, uint32_t n, const uint32_t *vertex_index, const uint32_t *slot_mesh,
	const RefitMesh *meshes, uint32_t num_meshes, const rtk_placement *places)
{
	const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= n) return;
	const uint32_t mesh = slot_mesh[s];
	if (mesh >= num_meshes) return;
	const RefitMesh ms = meshes[mesh];
	refit_tri<MODE, PLACED>(tris, s, vertex_index, ms, PLACED ? places + mesh : nullptr);
}

// A run of listed meshes that are neighbours in mesh_slots: its entries from entry_begin on belong to the threads from
// thread_begin on (the last run is followed by one that begins at the thread count).
struct RefitRange { uint32_t entry_begin, thread_begin; };

// The slots of the listed meshes only, one thread each (RefitMesh::pos of a mesh that is not listed is NULL), and the dirty
// set: every node from the slot's leaf up to the root gets dirty[node] = epoch. Plain stores of one and the same value by
// every writer; whoever finds a node marked stops, because the one who marked it goes on to the parent (by induction the
// parent of every marked node is marked when the launch ends). A stale read -- another CU's store not seen yet -- only means
// climbing further. Nothing is handed from one workgroup to another inside the launch: the flags are read by LATER launches.
// MARK false: the triangles only (the full box passes follow, which ask nobody what is dirty).
template <int MODE, bool MARK, bool PLACED>
__global__ void __launch_bounds__(256) k_refit_tris_listed(DevTri *tris, uint32_t n, const uint32_t *vertex_index, const uint32_t *slot_mesh,
	const RefitMesh *meshes, uint32_t num_meshes, const uint32_t *mesh_slots, const uint32_t *slot_node, const RefitRange *ranges, uint32_t num_ranges,
	uint32_t total, const uint32_t *parent, uint32_t *dirty, uint32_t num_nodes, uint32_t epoch, const rtk_placement *places)
{
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	uint32_t node = RTK_REF_NONE;
	if (t < total) {
		uint32_t lo = 0, hi = num_ranges;                      // the last run that begins at or before this thread
		while (hi - lo > 1u) {
			const uint32_t mid = (lo + hi) >> 1;
			if (ranges[mid].thread_begin <= t) lo = mid; else hi = mid;
		}
		const uint32_t e = ranges[lo].entry_begin + (t - ranges[lo].thread_begin);
		const uint32_t s = e < n ? mesh_slots[e] : RTK_REF_NONE;
		const uint32_t mesh = s < n ? slot_mesh[s] : RTK_REF_NONE;
		if (mesh < num_meshes) {
			const RefitMesh ms = meshes[mesh];
			if (ms.pos) {
				refit_tri<MODE, PLACED>(tris, s, vertex_index, ms, PLACED ? places + mesh : nullptr);
				if (MARK) node = slot_node[s];
			}
		}
	}
	if (!MARK) return;
	// neighbouring slots mostly share their leaf: one lane of each run of equal nodes climbs
	const uint32_t before = __shfl_up(node, 1);
	if ((threadIdx.x & 63u) != 0u && before == node) node = RTK_REF_NONE;
	while (node < num_nodes) {
		if (dirty[node] == epoch) break;
		dirty[node] = epoch;
		node = parent[node];
	}
}

// ---------------------------------------------------------------------------------- tables of the per-mesh refit (once per scene)

// four lanes per node, one per child slot: the parent of an inner child, the holder of every slot of a leaf child
__global__ void k_refit_parents(const DevNode *nodes, uint32_t n, const DevTri *tris, uint32_t num_tris, uint32_t *parent, uint32_t *slot_node)
{
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t i = t >> 2;
	if (i >= n) return;
	const uint32_t ref = nodes[i].child[t & 3u];
	if (ref == RTK_REF_NONE) return;
	if (ref & RTK_REF_LEAF) {
		const uint32_t first = ref & 0x7fffffffu;                // (the slots refit_child reads for this child)
		uint32_t cnt = first < num_tris ? tris[first].spare : 0u;
		if (cnt > 63u) cnt = 63u;
		if (cnt > num_tris - first) cnt = num_tris - first;
		for (uint32_t k = 0; k < cnt; k++) slot_node[first + k] = i;
	} else if (ref < n) parent[ref] = i;
}

__global__ void k_refit_mesh_keys(const uint32_t *slot_mesh, uint32_t n, unsigned long long *keys)
{
	const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
	if (s < n) keys[s] = ((unsigned long long)slot_mesh[s] << 32) | s;
}

__global__ void k_refit_mesh_slots(const unsigned long long *keys, uint32_t n, uint32_t *mesh_slots)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) mesh_slots[i] = (uint32_t)keys[i];
}

// ---------------------------------------------------------------------------------- dirty nodes by height

// entries e0 .. e0 + 3 of the schedule: bit k = node order[e0 + k] is dirty
__device__ __forceinline__ uint32_t dirty_mask4(const uint32_t *order, uint32_t n, const uint32_t *dirty, uint32_t epoch, uint32_t e0, uint32_t node[4])
{
	uint32_t mask = 0;
	if (e0 + 3u < n) {
		const uint4 o = *reinterpret_cast<const uint4 *>(order + e0);    // (e0 is a multiple of four)
		node[0] = o.x; node[1] = o.y; node[2] = o.z; node[3] = o.w;
	} else {
#pragma unroll
		for (int k = 0; k < 4; k++) node[k] = e0 + k < n ? order[e0 + k] : RTK_REF_NONE;
	}
#pragma unroll
	for (int k = 0; k < 4; k++) if (node[k] < n && dirty[node[k]] == epoch) mask |= 1u << k;
	return mask;
}

// exclusive running sum of v over the 256 threads of a workgroup; *all = the sum over all of them
__device__ __forceinline__ uint32_t block_scan_256(uint32_t v, uint32_t *all)
{
	__shared__ uint32_t wave_sum[4];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint32_t incl = v;
	for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(incl, o); if (lane >= (uint32_t)o) incl += t; }
	if (lane == 63u) wave_sum[wave] = incl;
	__syncthreads();
	uint32_t base = 0, sum = 0;
	for (uint32_t w = 0; w < 4u; w++) { if (w < wave) base += wave_sum[w]; sum += wave_sum[w]; }
	*all = sum;
	return base + incl - v;
}

// RTK_DIRTY_BLOCK entries of the schedule per workgroup: how many of them are dirty
__global__ void __launch_bounds__(256) k_dirty_count(const uint32_t *order, uint32_t n, const uint32_t *dirty, uint32_t epoch, uint32_t *block)
{
	uint32_t node[4], all;
	const uint32_t mask = dirty_mask4(order, n, dirty, epoch, blockIdx.x * RTK_DIRTY_BLOCK + threadIdx.x * 4u, node);
	(void)block_scan_256(__popc(mask), &all);
	if (threadIdx.x == 0u) block[blockIdx.x] = all;
}

// One workgroup: the counts become their exclusive running sums (block[nb] = the number of dirty nodes), then one wave per
// height finds where that height begins in the compacted list: the dirty entries before level_start[h].
__global__ void __launch_bounds__(1024) k_dirty_scan(uint32_t *block, uint32_t nb, const uint32_t *order, uint32_t n, const uint32_t *dirty, uint32_t epoch,
	const uint32_t *level_start, uint32_t heights, uint32_t *list_start)
{
	__shared__ uint32_t wave_sum[16];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint32_t carry = 0;
	for (uint32_t b0 = 0; b0 < nb; b0 += 1024u) {
		const uint32_t i = b0 + threadIdx.x;
		const uint32_t v = i < nb ? block[i] : 0u;
		uint32_t incl = v;
		for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(incl, o); if (lane >= (uint32_t)o) incl += t; }
		if (lane == 63u) wave_sum[wave] = incl;
		__syncthreads();
		uint32_t base = 0, sum = 0;
		for (uint32_t w = 0; w < 16u; w++) { if (w < wave) base += wave_sum[w]; sum += wave_sum[w]; }
		if (i < nb) block[i] = carry + base + incl - v;
		carry += sum;
		__syncthreads();
	}
	if (threadIdx.x == 0u) block[nb] = carry;
	__syncthreads();                                           // (one workgroup: its own stores are what it reads below)
	for (uint32_t h = wave; h <= heights; h += 16u) {
		const uint32_t p = level_start[h] < n ? level_start[h] : n;
		const uint32_t b = p / RTK_DIRTY_BLOCK;                  // (p == n on a block boundary: b == nb, the total)
		uint32_t c = 0;
		for (uint32_t e = b * RTK_DIRTY_BLOCK + lane; e < p; e += 64u) { const uint32_t node = order[e]; c += (node < n && dirty[node] == epoch) ? 1u : 0u; }
		for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
		if (lane == 0u) list_start[h] = block[b] + c;
	}
}

// the dirty nodes of the workgroup's entries, in the schedule's order, to where the running sums say
__global__ void __launch_bounds__(256) k_dirty_scatter(const uint32_t *order, uint32_t n, const uint32_t *dirty, uint32_t epoch, const uint32_t *block, uint32_t *list)
{
	uint32_t node[4], all;
	const uint32_t mask = dirty_mask4(order, n, dirty, epoch, blockIdx.x * RTK_DIRTY_BLOCK + threadIdx.x * 4u, node);
	uint32_t at = block[blockIdx.x] + block_scan_256(__popc(mask), &all);
#pragma unroll
	for (int k = 0; k < 4; k++) if ((mask >> k & 1u) && at < n) list[at++] = node[k];
}

// ---------------------------------------------------------------------------------- boxes

// Child slot k of `node`: its box from what is below it, stored into the node (the four lanes of a node store four
// neighbouring words each time). The child words are left alone.
__device__ __forceinline__ void refit_child(DevNode *nodes, const DevTri *tris, uint32_t num_nodes, uint32_t num_tris, uint32_t node, uint32_t k)
{
	DevNode *nd = nodes + node;
	const uint32_t ref = nd->child[k];
	float mn[3] = { 1.0f, 1.0f, 1.0f }, mx[3] = { -1.0f, -1.0f, -1.0f };         // an empty slot keeps the inverted box
	if (ref != RTK_REF_NONE) {
		// The union starts from its first member, as the build's does, and grows by fminf / fmaxf: a NaN is skipped unless
		// EVERY member is one (a leaf of all-NaN triangles gets the NaN box a build gives it, which the validator reports
		// for both); with nothing below the slot -- a broken reference -- the box is the empty union.
		bool first_member = true;
		mn[0] = mn[1] = mn[2] = INFINITY;
		mx[0] = mx[1] = mx[2] = -INFINITY;
		if (ref & RTK_REF_LEAF) {
			const uint32_t first = ref & 0x7fffffffu;
			uint32_t cnt = first < num_tris ? tris[first].spare : 0u;
			if (cnt > 63u) cnt = 63u;
			if (cnt > num_tris - first) cnt = num_tris - first;
			for (uint32_t t = 0; t < cnt; t++) {
				const float4 *rec = reinterpret_cast<const float4 *>(tris + first + t);
				const float4 a = rec[0], b = rec[1], c = rec[2];
				const float lo[3] = { fminf(fminf(a.x, b.x), c.x), fminf(fminf(a.y, b.y), c.y), fminf(fminf(a.z, b.z), c.z) };
				const float hi[3] = { fmaxf(fmaxf(a.x, b.x), c.x), fmaxf(fmaxf(a.y, b.y), c.y), fmaxf(fmaxf(a.z, b.z), c.z) };
#pragma unroll
				for (int ax = 0; ax < 3; ax++) {
					mn[ax] = first_member ? lo[ax] : fminf(mn[ax], lo[ax]);
					mx[ax] = first_member ? hi[ax] : fmaxf(mx[ax], hi[ax]);
				}
				first_member = false;
			}
		} else if (ref < num_nodes) {
			const DevNode *ch = nodes + ref;
			const float4 *w = reinterpret_cast<const float4 *>(ch);
			const float4 xl = w[0], xh = w[1], yl = w[2], yh = w[3], zl = w[4], zh = w[5];
			const uint4 cc = *reinterpret_cast<const uint4 *>(ch->child);
			const float bl[3][4] = { { xl.x, xl.y, xl.z, xl.w }, { yl.x, yl.y, yl.z, yl.w }, { zl.x, zl.y, zl.z, zl.w } };
			const float bh[3][4] = { { xh.x, xh.y, xh.z, xh.w }, { yh.x, yh.y, yh.z, yh.w }, { zh.x, zh.y, zh.z, zh.w } };
			const uint32_t cr[4] = { cc.x, cc.y, cc.z, cc.w };
#pragma unroll
			for (int q = 0; q < 4; q++) {
				if (cr[q] == RTK_REF_NONE) continue;
#pragma unroll
				for (int ax = 0; ax < 3; ax++) {
					mn[ax] = first_member ? bl[ax][q] : fminf(mn[ax], bl[ax][q]);
					mx[ax] = first_member ? bh[ax][q] : fmaxf(mx[ax], bh[ax][q]);
				}
				first_member = false;
			}
		}
	}
	nd->bx[0][k] = mn[0]; nd->bx[1][k] = mx[0];
	nd->by[0][k] = mn[1]; nd->by[1][k] = mx[1];
	nd->bz[0][k] = mn[2]; nd->bz[1][k] = mx[2];
}

// one height: entries [begin, end) of `order`, four lanes per node
__global__ void __launch_bounds__(256) k_refit_level(DevNode *nodes, const DevTri *tris, uint32_t num_nodes, uint32_t num_tris,
	const uint32_t *order, uint32_t begin, uint32_t end)
{
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t e = begin + (t >> 2);
	if (e >= end) return;
	const uint32_t node = order[e];
	if (node < num_nodes) refit_child(nodes, tris, num_nodes, num_tris, node, t & 3u);
}

// one height of the dirty nodes: entries [list_start[h], list_start[h + 1]) of `list`, four lanes per node, grid-stride (the
// host does not know how many there are)
__global__ void __launch_bounds__(256) k_refit_level_list(DevNode *nodes, const DevTri *tris, uint32_t num_nodes, uint32_t num_tris,
	const uint32_t *list, const uint32_t *list_start, uint32_t h)
{
	const uint32_t begin = list_start[h];
	uint32_t end = list_start[h + 1u];
	if (end > num_nodes) end = num_nodes;
	for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; begin < end && (t >> 2) < end - begin; t += gridDim.x * blockDim.x) {
		const uint32_t node = list[begin + (t >> 2)];
		if (node < num_nodes) refit_child(nodes, tris, num_nodes, num_tris, node, t & 3u);
	}
}

// heights [h0, h1) in one workgroup: what a height stores is read by the next one behind a barrier (workgroup scope is all
// that is needed: one workgroup; the kernel boundary does the rest)
__global__ void __launch_bounds__(REFIT_SMALL_THREADS) k_refit_small(DevNode *nodes, const DevTri *tris, uint32_t num_nodes, uint32_t num_tris,
	const uint32_t *order, const uint32_t *level_start, uint32_t h0, uint32_t h1)
{
	for (uint32_t h = h0; h < h1; h++) {
		const uint32_t begin = level_start[h], end = level_start[h + 1u];
		for (uint32_t e = begin + (threadIdx.x >> 2); e < end; e += REFIT_SMALL_THREADS / 4) {
			const uint32_t node = order[e];
			if (node < num_nodes) refit_child(nodes, tris, num_nodes, num_tris, node, threadIdx.x & 3u);
		}
		__syncthreads();
	}
}

// ---------------------------------------------------------------------------------- host

// temporaries of the schedule: heights, the changed word, two key arrays, the sort's scratch, level starts
struct ScheduleTmp { size_t o_height, o_changed, o_ka, o_kb, o_sort, o_ls, bytes; };
ScheduleTmp schedule_tmp(uint32_t n)
{
	Carve c;       // (a braced list is evaluated left to right: the pieces in the order of the members, then their sum)
	return ScheduleTmp{ c.take((size_t)n * 4), c.take(4), c.take((size_t)n * 8), c.take((size_t)n * 8), c.take(rtk_sort_scratch_words(n) * 4), c.take(((size_t)n + 2) * 4), c.bytes };
}

// heights, node numbers grouped by height, the mesh table's memory: once per scene. tmp: schedule_tmp(num_nodes).bytes of
// device memory (the borrowed workspace: no allocation of a quarter of a gigabyte at 10M triangles, freed again at once)
int make_schedule(rtk_dev_scene *ds, hipStream_t stream, char *tmp)
{
	RefitSchedule &rs = ds->refit;
	if (rs.ready) return RTK_AMD_OK;
	const uint32_t n = ds->view.num_nodes;
	const size_t num_meshes = ds->mesh_base.empty() ? 0 : ds->mesh_base.size() - 1;
	const ScheduleTmp T = schedule_tmp(n);
	uint32_t *d_height = (uint32_t *)(tmp + T.o_height), *d_changed = (uint32_t *)(tmp + T.o_changed), *d_ls = (uint32_t *)(tmp + T.o_ls);
	unsigned long long *keys_a = (unsigned long long *)(tmp + T.o_ka), *keys_b = (unsigned long long *)(tmp + T.o_kb);
	void *d_order = nullptr, *d_small = nullptr;
	int rc = RTK_AMD_OK;
	std::vector<uint32_t> level_start;
	Carve small;
	do {
#define SCHED_CHECK(expr) if ((expr) != hipSuccess) { rtk_set_error("rtk_dev_scene_refit: schedule: %s failed: %s", #expr, hipGetErrorString(hipGetLastError())); rc = RTK_AMD_ERR_HIP; break; }
		const unsigned blocks = (n + 255u) / 256u;
		SCHED_CHECK(hipMemsetAsync(d_height, 0, (size_t)n * 4, stream));
		// A tree has no cycle and its heights are below max_depth, so max_depth sweeps settle them; one more, which must change
		// nothing, is the proof, and the one wait of the host. (Should a scene's max_depth be too small the rounds go on, eight
		// sweeps at a time.)
		uint32_t sweeps = 0, round = ds->tree.max_depth < 4096u ? ds->tree.max_depth + 1u : 4096u;
		bool converged = false;
		while (!converged && rc == RTK_AMD_OK) {
			uint32_t h_changed = 0;
			for (uint32_t k = 0; k + 1u < round; k++) hipLaunchKernelGGL(k_refit_heights, dim3(blocks), dim3(256), 0, stream, ds->view.nodes, n, d_height, d_changed);
			if (hipMemsetAsync(d_changed, 0, 4, stream) != hipSuccess) { rc = RTK_AMD_ERR_HIP; break; }
			hipLaunchKernelGGL(k_refit_heights, dim3(blocks), dim3(256), 0, stream, ds->view.nodes, n, d_height, d_changed);
			sweeps += round;
			round = 8u;
			if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&h_changed, d_changed, 4, hipMemcpyDeviceToHost, stream) != hipSuccess ||
				hipStreamSynchronize(stream) != hipSuccess) { rc = RTK_AMD_ERR_HIP; break; }
			converged = h_changed == 0u;
			if (!converged && sweeps > n + 8u) { rc = RTK_AMD_ERR_BAD_SCENE; break; }
		}
		if (rc != RTK_AMD_OK) { rtk_set_error("rtk_dev_scene_refit: schedule: heights did not settle (%s)", rc == RTK_AMD_ERR_HIP ? hipGetErrorString(hipGetLastError()) : "not a tree"); break; }
		hipLaunchKernelGGL(k_refit_keys, dim3(blocks), dim3(256), 0, stream, d_height, n, keys_a);
		// heights are below n: that many bits of the upper word, in whole 8-bit passes; stable, so numbers stay in order
		const unsigned long long bound = n;
		uint32_t bits = 1;
		while (bits < 32u && (1ull << bits) <= bound) bits++;
		const unsigned long long *sorted = keys_a;
		if (n > 1u) sorted = rtk_sort_words_async(keys_a, keys_b, n, 32u, 32u + bits, (uint32_t *)(tmp + T.o_sort), stream) ? keys_b : keys_a;
		SCHED_CHECK(hipMalloc(&d_order, (size_t)n * 4));
		hipLaunchKernelGGL(k_refit_order, dim3(blocks), dim3(256), 0, stream, sorted, n, (uint32_t *)d_order, d_ls);
		unsigned long long last = 0;
		SCHED_CHECK(hipGetLastError());
		SCHED_CHECK(hipMemcpyAsync(&last, sorted + (n - 1u), 8, hipMemcpyDeviceToHost, stream));
		SCHED_CHECK(hipStreamSynchronize(stream));
		const uint32_t heights = (uint32_t)(last >> 32) + 1u;
		if (heights > n) { rtk_set_error("rtk_dev_scene_refit: schedule: %u heights for %u nodes", heights, n); rc = RTK_AMD_ERR_BAD_SCENE; break; }
		level_start.resize((size_t)heights + 1);
		SCHED_CHECK(hipMemcpy(level_start.data(), d_ls, level_start.size() * 4, hipMemcpyDeviceToHost));
		bool sane = level_start.front() == 0u && level_start.back() == n;
		for (size_t h = 0; h + 1 < level_start.size(); h++) sane = sane && level_start[h] < level_start[h + 1];
		if (!sane) { rtk_set_error("rtk_dev_scene_refit: schedule: heights are not contiguous"); rc = RTK_AMD_ERR_BAD_SCENE; break; }
		// the level starts and the mesh table share one small allocation. The table lies behind the carve: the last piece, not
		// padded, with room for one record even where there is no mesh, which the ledger does not count
		small.take(level_start.size() * 4);
		SCHED_CHECK(hipMalloc(&d_small, small.bytes + (num_meshes ? num_meshes : 1) * sizeof(RefitMesh)));
		SCHED_CHECK(hipMemcpy(d_small, level_start.data(), level_start.size() * 4, hipMemcpyHostToDevice));
		rs.d_meshes = (char *)d_small + small.bytes;
#undef SCHED_CHECK
	} while (0);
	if (rc != RTK_AMD_OK) {
		if (d_order) (void)hipFree(d_order);
		if (d_small) (void)hipFree(d_small);
		rs.d_meshes = nullptr;
		return rc;
	}
	ds->mem.adopt(d_order, (size_t)n * 4);
	ds->mem.adopt(d_small, small.counted + num_meshes * sizeof(RefitMesh));
	rs.d_order = (uint32_t *)d_order;
	rs.d_level_start = (uint32_t *)d_small;
	rs.level_start.swap(level_start);
	rs.ready = true;
	return RTK_AMD_OK;
}

int make_max_vertex(rtk_dev_scene *ds, hipStream_t stream)
{
	RefitSchedule &rs = ds->refit;
	if (rs.max_vertex_ready) return RTK_AMD_OK;
	const size_t num_meshes = ds->mesh_base.size() - 1;
	const uint32_t n = ds->view.num_tris;
	std::vector<uint32_t> mv(num_meshes, 0u);
	if (n) {
		uint32_t *d = nullptr;
		if (hipMalloc(&d, num_meshes * 4) != hipSuccess) { (void)hipGetLastError(); rtk_set_error("rtk_dev_scene_refit: out of device memory"); return RTK_AMD_ERR_OOM; }
		bool ok = hipMemsetAsync(d, 0, num_meshes * 4, stream) == hipSuccess;
		if (ok) hipLaunchKernelGGL(k_refit_max_vertex, dim3((n + 255u) / 256u), dim3(256), 0, stream, ds->view.vertex_index, ds->view.slot_mesh, n, (uint32_t)num_meshes, d);
		ok = ok && hipGetLastError() == hipSuccess && hipMemcpyAsync(mv.data(), d, num_meshes * 4, hipMemcpyDeviceToHost, stream) == hipSuccess &&
			hipStreamSynchronize(stream) == hipSuccess;
		(void)hipFree(d);
		if (!ok) { rtk_set_error("rtk_dev_scene_refit: %s", hipGetErrorString(hipGetLastError())); return RTK_AMD_ERR_HIP; }
	}
	rs.max_vertex.swap(mv);
	rs.max_vertex_ready = true;
	return RTK_AMD_OK;
}

// temporaries of the per-mesh tables: two key arrays over the slots and the sort's scratch
struct TablesTmp { size_t o_ka, o_kb, o_sort, bytes; };
TablesTmp tables_tmp(uint32_t num_tris)
{
	Carve c;
	return TablesTmp{ c.take((size_t)num_tris * 8), c.take((size_t)num_tris * 8), c.take(rtk_sort_scratch_words(num_tris) * 4), c.bytes };
}

// parent[], the node of every slot's leaf, the slots grouped by mesh, and the memory of the dirty set: once per scene, after
// the schedule. tmp: tables_tmp(num_tris).bytes of device memory (the borrowed workspace).
int make_partial_tables(rtk_dev_scene *ds, hipStream_t stream, char *tmp)
{
	RefitPartial &rp = ds->partial;
	if (rp.ready) return RTK_AMD_OK;
	const DevSceneView &v = ds->view;
	const uint32_t n = v.num_nodes, nt = v.num_tris;
	const size_t num_meshes = ds->mesh_base.size() - 1;
	const uint32_t nb = (n + RTK_DIRTY_BLOCK - 1u) / RTK_DIRTY_BLOCK;
	const size_t heights = ds->refit.level_start.size() - 1;
	Carve c;
	const size_t o_parent = c.take((size_t)n * 4), o_slot_node = c.take((size_t)nt * 4), o_mesh_slots = c.take((size_t)nt * 4), o_dirty = c.take((size_t)n * 4),
		o_list = c.take((size_t)n * 4), o_block = c.take(((size_t)nb + 1) * 4), o_list_start = c.take((heights + 1) * 4), o_ranges = c.take((num_meshes + 1) * sizeof(RefitRange));
	void *mem = nullptr;
	if (hipMalloc(&mem, c.bytes) != hipSuccess) { (void)hipGetLastError(); rtk_set_error("rtk_dev_scene_refit_meshes: out of device memory"); return RTK_AMD_ERR_OOM; }
	char *base = (char *)mem;
	uint32_t *d_parent = (uint32_t *)(base + o_parent), *d_slot_node = (uint32_t *)(base + o_slot_node), *d_mesh_slots = (uint32_t *)(base + o_mesh_slots);
	const TablesTmp T = tables_tmp(nt);
	unsigned long long *keys_a = (unsigned long long *)(tmp + T.o_ka), *keys_b = (unsigned long long *)(tmp + T.o_kb);
	// (RTK_REF_NONE everywhere first: the root has no parent, and a slot no leaf names stays without a node)
	bool ok = hipMemsetAsync(base, 0xff, o_mesh_slots, stream) == hipSuccess && hipMemsetAsync(base + o_dirty, 0, o_list - o_dirty, stream) == hipSuccess;
	if (ok) {
		hipLaunchKernelGGL(k_refit_parents, dim3((unsigned)(((size_t)n * 4 + 255) / 256)), dim3(256), 0, stream, v.nodes, n, v.tris, nt, d_parent, d_slot_node);
		const unsigned blocks = (nt + 255u) / 256u;
		hipLaunchKernelGGL(k_refit_mesh_keys, dim3(blocks), dim3(256), 0, stream, v.slot_mesh, nt, keys_a);
		// mesh numbers are below num_meshes: that many bits of the upper word; stable, so the slots of a mesh stay ascending
		uint32_t bits = 0;
		while (bits < 32u && (1ull << bits) < (unsigned long long)num_meshes) bits++;
		const unsigned long long *sorted = keys_a;
		if (bits) sorted = rtk_sort_words_async(keys_a, keys_b, nt, 32u, 32u + bits, (uint32_t *)(tmp + T.o_sort), stream) ? keys_b : keys_a;
		hipLaunchKernelGGL(k_refit_mesh_slots, dim3(blocks), dim3(256), 0, stream, sorted, nt, d_mesh_slots);
		ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(stream) == hipSuccess;
	}
	if (!ok) {
		rtk_set_error("rtk_dev_scene_refit_meshes: tables: %s", hipGetErrorString(hipGetLastError()));
		(void)hipFree(mem);
		return RTK_AMD_ERR_HIP;
	}
	ds->mem.adopt(mem, c.counted);
	rp.d_parent = d_parent; rp.d_slot_node = d_slot_node; rp.d_mesh_slots = d_mesh_slots;
	rp.d_dirty = (uint32_t *)(base + o_dirty); rp.d_list = (uint32_t *)(base + o_list); rp.d_block = (uint32_t *)(base + o_block);
	rp.d_list_start = (uint32_t *)(base + o_list_start); rp.d_ranges = base + o_ranges;
	rp.epoch = 0;
	rp.ready = true;
	return RTK_AMD_OK;
}

// Above this share of the scene's triangles in the listed meshes the dirty-set passes lose against the full box and finish
// passes, which then run instead (the triangles are still regathered for the listed meshes only). Where the two measured
// curves meet, rounded down to a power of two: profiles/refit_meshes_timing.log. RTK_AMD_REFIT_MESHES_SHARE overrides it
// (0: always the full passes, 1: never), for A/B; read at every call, so one process can measure both.
#define REFIT_MESHES_MAX_SHARE 0.25
double partial_max_share()
{
	const char *e = getenv("RTK_AMD_REFIT_MESHES_SHARE");
	return e ? atof(e) : REFIT_MESHES_MAX_SHARE;
}

// everything behind the argument checks; the scene's device is current. listed: NULL = every mesh (rtk_dev_scene_refit), else
// one flag per mesh (rtk_dev_scene_refit_meshes), with listed_tris triangles (not zero) in the flagged ones. placements: NULL, or
// one per mesh (the _placed entry points; only the entries of meshes that are read are looked at).
int refit_on_device(rtk_dev_scene *ds, const rtk_scene_desc *desc, const rtk_placement *placements, hipStream_t stream, WorkspaceLoan &loan, const uint8_t *listed, uint64_t listed_tris)
{
	int rc = rtk_scene_side_arrays(ds, stream);
	if (rc != RTK_AMD_OK) return rc;
	RefitSchedule &rs = ds->refit;
	if (ds->view.num_nodes == 0u) { rtk_set_error("rtk_dev_scene_refit: scene without a root node"); return RTK_AMD_ERR_BAD_SCENE; }
	const DevSceneView &v = ds->view;
	const size_t num_meshes = desc->num_meshes;

	// ---- where every mesh's positions are read from
	std::vector<RefitMesh> table(num_meshes ? num_meshes : 1, RefitMesh{ nullptr, 0ull, 0u, 0u });
	std::vector<size_t> upload(num_meshes, 0);
	size_t upload_bytes = 0;
	bool any_device = false, any_f32 = false, any_f64 = false;
	for (size_t mi = 0; mi < num_meshes; mi++) {
		const rtk_mesh *m = &desc->meshes[mi];
		if (m->num_triangles == 0 || (listed && !listed[mi])) continue;
		RefitMesh &t = table[mi];
		t.f64 = m->position.type == RTK_TYPE_F64 ? 1u : 0u;
		t.stride = m->position.stride ? m->position.stride : (t.f64 ? 24 : 12);
		t.pos = (const char *)m->position.data;
		(t.f64 ? any_f64 : any_f32) = true;
		if (rtk_is_device_ptr(m->position.data)) { any_device = true; continue; }
		rc = make_max_vertex(ds, stream);
		if (rc != RTK_AMD_OK) return rc;
		upload[mi] = (size_t)rs.max_vertex[mi] * t.stride + (t.f64 ? 24 : 12);
		upload_bytes += rtk_padded(upload[mi]);
	}
	// the placements of the meshes that are read go to the device beside the staged positions (entries of other meshes: zeros)
	std::vector<rtk_placement> places;
	if (placements) {
		places.assign(num_meshes ? num_meshes : 1, rtk_placement{});
		for (size_t mi = 0; mi < num_meshes; mi++) if (table[mi].pos) places[mi] = placements[mi];
		upload_bytes += rtk_padded(places.size() * sizeof(rtk_placement));
	}
	// the workspace: first the temporaries of the schedule (the first refit of a scene; over when make_schedule returns), then
	// those of the per-mesh tables (the first refit of some meshes), then the staged positions and placements
	const size_t schedule_bytes = rs.ready ? 0 : schedule_tmp(ds->view.num_nodes).bytes;
	const size_t tables_bytes = listed && !ds->partial.ready ? tables_tmp(v.num_tris).bytes : 0;
	size_t borrow = schedule_bytes > upload_bytes ? schedule_bytes : upload_bytes;
	if (tables_bytes > borrow) borrow = tables_bytes;
	if (borrow && !loan.take(ds->device, borrow)) return RTK_AMD_ERR_OOM;
	rc = make_schedule(ds, stream, loan.base);
	if (rc != RTK_AMD_OK) return rc;
	if (listed) {
		rc = make_partial_tables(ds, stream, loan.base);
		if (rc != RTK_AMD_OK) return rc;
	}
	const rtk_placement *d_places = nullptr;
	if (upload_bytes) {
		char *base = loan.base;
		size_t off = 0;
		for (size_t mi = 0; mi < num_meshes; mi++) {
			if (!upload[mi]) continue;
			RTK_PASS_CHECK("rtk_dev_scene_refit", hipMemcpyAsync(base + off, table[mi].pos, upload[mi], hipMemcpyHostToDevice, stream));
			table[mi].pos = base + off;
			off += rtk_padded(upload[mi]);
		}
		if (placements) {
			RTK_PASS_CHECK("rtk_dev_scene_refit", hipMemcpyAsync(base + off, places.data(), places.size() * sizeof(rtk_placement), hipMemcpyHostToDevice, stream));
			d_places = (const rtk_placement *)(base + off);
		}
	}
	// a mesh in device memory was written by the caller's own work, possibly still in flight on the NULL stream (as in a build)
	if (any_device && stream != nullptr) RTK_PASS_CHECK("rtk_dev_scene_refit", hipStreamSynchronize(nullptr));
	if (num_meshes) RTK_PASS_CHECK("rtk_dev_scene_refit", hipMemcpyAsync(rs.d_meshes, table.data(), num_meshes * sizeof(RefitMesh), hipMemcpyHostToDevice, stream));

	// Until this call has succeeded nobody may take the boxes it leaves alone for exact unions.
	const bool were_exact = ds->tree.boxes_exact;
	ds->tree.boxes_exact = false;
	// the dirty set pays while the listed meshes are a small part of the scene and the other boxes can be trusted
	const bool dirty_set = listed && were_exact && (double)listed_tris <= partial_max_share() * (double)v.num_tris;

	// ---- triangles
	DevTri *tris = const_cast<DevTri *>(v.tris);
	DevNode *nodes = const_cast<DevNode *>(v.nodes);
	const RefitMesh *dm = (const RefitMesh *)rs.d_meshes;
	const int mode = any_f64 && any_f32 ? 2 : any_f64 ? 1 : 0;
	if (listed) {
		RefitPartial &rp = ds->partial;
		// runs of listed meshes that are neighbours in mesh_slots, one thread per slot
		std::vector<RefitRange> ranges;
		uint64_t threads = 0, run_end = 0;
		for (size_t mi = 0; mi < num_meshes; mi++) {
			if (!listed[mi] || ds->mesh_base[mi + 1] == ds->mesh_base[mi]) continue;
			if (ranges.empty() || run_end != ds->mesh_base[mi]) ranges.push_back(RefitRange{ (uint32_t)ds->mesh_base[mi], (uint32_t)threads });
			threads += ds->mesh_base[mi + 1] - ds->mesh_base[mi];
			run_end = ds->mesh_base[mi + 1];
		}
		RTK_PASS_CHECK("rtk_dev_scene_refit", hipMemcpyAsync(rp.d_ranges, ranges.data(), ranges.size() * sizeof(RefitRange), hipMemcpyHostToDevice, stream));
		if (++rp.epoch == 0u) {                                  // (every 2^32 calls the flags start over)
			RTK_PASS_CHECK("rtk_dev_scene_refit", hipMemsetAsync(rp.d_dirty, 0, (size_t)v.num_nodes * 4, stream));
			rp.epoch = 1u;
		}
		const uint32_t total = (uint32_t)threads;
		const dim3 grid((total + 255u) / 256u), block(256);
		const RefitRange *dr = (const RefitRange *)rp.d_ranges;
		// (MODE and PLACED are compile-time variants: the unplaced instantiations are what they were before there were placements)
#define LISTED_LAUNCH(MODE, MARK, PLACED) hipLaunchKernelGGL((k_refit_tris_listed<MODE, MARK, PLACED>), grid, block, 0, stream, tris, v.num_tris, v.vertex_index, v.slot_mesh, dm, \
	(uint32_t)num_meshes, rp.d_mesh_slots, rp.d_slot_node, dr, (uint32_t)ranges.size(), total, rp.d_parent, rp.d_dirty, v.num_nodes, rp.epoch, d_places)
#define LISTED_MODES(MARK, PLACED) do { if (mode == 2) LISTED_LAUNCH(2, MARK, PLACED); else if (mode == 1) LISTED_LAUNCH(1, MARK, PLACED); else LISTED_LAUNCH(0, MARK, PLACED); } while (0)
		if (dirty_set && d_places) LISTED_MODES(true, true);
		else if (dirty_set) LISTED_MODES(true, false);
		else if (d_places) LISTED_MODES(false, true);
		else LISTED_MODES(false, false);
#undef LISTED_MODES
#undef LISTED_LAUNCH
		RTK_PASS_CHECK("rtk_dev_scene_refit", hipGetLastError());
	} else if (v.num_tris) {
		const dim3 grid((v.num_tris + 255u) / 256u), block(256);
#define TRIS_LAUNCH(MODE, PLACED) hipLaunchKernelGGL((k_refit_tris<MODE, PLACED>), grid, block, 0, stream, tris, v.num_tris, v.vertex_index, v.slot_mesh, dm, (uint32_t)num_meshes, d_places)
#define TRIS_MODES(PLACED) do { if (mode == 2) TRIS_LAUNCH(2, PLACED); else if (mode == 1) TRIS_LAUNCH(1, PLACED); else TRIS_LAUNCH(0, PLACED); } while (0)
		if (d_places) TRIS_MODES(true); else TRIS_MODES(false);
#undef TRIS_MODES
#undef TRIS_LAUNCH
		RTK_PASS_CHECK("rtk_dev_scene_refit", hipGetLastError());
	}

	const uint32_t heights = (uint32_t)rs.level_start.size() - 1u;
	bool full_finish = true;
	if (dirty_set) {
		// ---- the dirty nodes in the schedule's order, and where each height begins among them (all of it stays on the device)
		RefitPartial &rp = ds->partial;
		const uint32_t n = v.num_nodes, nb = (n + RTK_DIRTY_BLOCK - 1u) / RTK_DIRTY_BLOCK;
		hipLaunchKernelGGL(k_dirty_count, dim3(nb), dim3(256), 0, stream, rs.d_order, n, rp.d_dirty, rp.epoch, rp.d_block);
		hipLaunchKernelGGL(k_dirty_scan, dim3(1), dim3(1024), 0, stream, rp.d_block, nb, rs.d_order, n, rp.d_dirty, rp.epoch, rs.d_level_start, heights, rp.d_list_start);
		hipLaunchKernelGGL(k_dirty_scatter, dim3(nb), dim3(256), 0, stream, rs.d_order, n, rp.d_dirty, rp.epoch, rp.d_block, rp.d_list);
		// ---- their boxes, height by height. Which heights get a launch of their own is the full schedule's decision (the host
		// does not know the dirty counts): a height that is small there is small here.
		for (uint32_t h = 0; h < heights;) {
			const uint32_t begin = rs.level_start[h], end = rs.level_start[h + 1];
			if (end - begin > REFIT_SMALL_LEVEL) {
				size_t blocks = ((size_t)(end - begin) * 4 + 255) / 256;
				if (blocks > 2048) blocks = 2048;
				hipLaunchKernelGGL(k_refit_level_list, dim3((unsigned)blocks), dim3(256), 0, stream, nodes, tris, v.num_nodes, v.num_tris, rp.d_list, rp.d_list_start, h);
				h++;
			} else {
				uint32_t h1 = h + 1;
				while (h1 < heights && rs.level_start[h1 + 1] - rs.level_start[h1] <= REFIT_SMALL_LEVEL) h1++;
				hipLaunchKernelGGL(k_refit_small, dim3(1), dim3(REFIT_SMALL_THREADS), 0, stream, nodes, tris, v.num_nodes, v.num_tris, rp.d_list, rp.d_list_start, h, h1);
				h = h1;
			}
		}
		RTK_PASS_CHECK("rtk_dev_scene_refit", hipGetLastError());
		RTK_PASS_CHECK("rtk_dev_scene_refit", hipMemcpyAsync(&ds->partial_readback, rp.d_block + nb, 4, hipMemcpyDeviceToHost, stream));
		// ---- compressed nodes and order words of the dirty nodes, the constants from the root (dirty whenever anything moved).
		// The misfit count is one over ALL nodes: the list form is the whole answer only if the others have none (the scene is on
		// its compressed nodes now) and none of the dirty ones has one either; else the full pass below.
		if (v.qnodes && ds->tree.qnodes_mem) {
			rc = rtk_quantize_node_list(ds, stream, rp.d_list, rp.d_block + nb);
			if (rc != RTK_AMD_OK) return rc;
			RTK_PASS_CHECK("rtk_dev_scene_refit", hipStreamSynchronize(stream));
			full_finish = ds->tree.consts_readback.qnode_misfits != 0u;
		}
	} else {
		// ---- boxes, height by height; runs of small heights share one launch of one workgroup
		for (uint32_t h = 0; h < heights;) {
			const uint32_t begin = rs.level_start[h], end = rs.level_start[h + 1];
			if (end - begin > REFIT_SMALL_LEVEL) {
				const unsigned blocks = (unsigned)(((size_t)(end - begin) * 4 + 255) / 256);
				hipLaunchKernelGGL(k_refit_level, dim3(blocks), dim3(256), 0, stream, nodes, tris, v.num_nodes, v.num_tris, rs.d_order, begin, end);
				h++;
			} else {
				uint32_t h1 = h + 1;
				while (h1 < heights && rs.level_start[h1 + 1] - rs.level_start[h1] <= REFIT_SMALL_LEVEL) h1++;
				hipLaunchKernelGGL(k_refit_small, dim3(1), dim3(REFIT_SMALL_THREADS), 0, stream, nodes, tris, v.num_nodes, v.num_tris, rs.d_order, rs.d_level_start, h, h1);
				h = h1;
			}
		}
		RTK_PASS_CHECK("rtk_dev_scene_refit", hipGetLastError());
	}

	if (full_finish) {
		// ---- compressed nodes, order words, constants (the block is cleared first: the misfit count starts at zero); every box
		// lies inside the root's now, so no bound is passed in
		rc = rtk_quantize_nodes(ds, stream, nullptr, const_cast<DevNodeQ *>(ds->tree.qnodes_mem), 0.0f, 0xffffffffu, false, true);
		if (rc != RTK_AMD_OK) return rc;
		RTK_PASS_CHECK("rtk_dev_scene_refit", hipStreamSynchronize(stream));
	}
	{
		// (the trace path reads these host fields under the same mutex when it enqueues a launch)
		std::lock_guard<std::mutex> lock(ds->scratch_mutex);
		rtk_quantize_finish(ds);
	}
	rtk_scene_forget_derived(ds, RTK_FORGET_BOXES);
	ds->tree.boxes_exact = true;
	ds->refit_nodes = dirty_set ? ds->partial_readback : v.num_nodes;
	return RTK_AMD_OK;
}

// what both entry points do once nothing can be refused any more
int refit_in_pass(ScenePass &pass, const rtk_scene_desc *desc, const rtk_placement *placements, const uint8_t *listed, uint64_t listed_tris)
{
	if (!pass.on_device()) return RTK_AMD_ERR_NO_DEVICE;
	WorkspaceLoan loan;
	// (a failed pass has waited for whatever reads the workspace before the loan ends; the time is taken after it has)
	const int rc = pass.end(refit_on_device(pass.ds, desc, placements, pass.stream, loan, listed, listed_tris));
	loan.release();
	if (rc == RTK_AMD_OK) pass.ds->refit_ms = pass.ms();
	return rc;
}

// the rules for the positions of a mesh that is read
int check_mesh_positions(const char *who, const rtk_mesh *m, size_t mi)
{
	if (m->position_cb) { rtk_set_error("%s: mesh %zu: position callbacks are not supported by a refit", who, mi); return RTK_AMD_ERR_UNSUPPORTED; }
	if (m->num_triangles == 0) return RTK_AMD_OK;
	if (m->position.type != RTK_TYPE_DEFAULT && m->position.type != RTK_TYPE_REAL && m->position.type != RTK_TYPE_F32 && m->position.type != RTK_TYPE_F64) {
		rtk_set_error("%s: mesh %zu: bad position type %d", who, mi, (int)m->position.type);
		return RTK_AMD_ERR_BAD_ARG;
	}
	if (!m->position.data) { rtk_set_error("%s: mesh %zu has no positions", who, mi); return RTK_AMD_ERR_BAD_ARG; }
	return RTK_AMD_OK;
}

// the description against the scene it claims to describe
int check_desc(const char *who, const rtk_dev_scene *ds, const rtk_scene_desc *desc)
{
	if (!desc->meshes && desc->num_meshes) { rtk_set_error("%s: NULL meshes", who); return RTK_AMD_ERR_BAD_ARG; }
	const size_t scene_meshes = ds->mesh_base.empty() ? 0 : ds->mesh_base.size() - 1;
	if (desc->num_meshes != scene_meshes) {
		rtk_set_error("%s: %zu meshes, the scene was made from %zu", who, (size_t)desc->num_meshes, scene_meshes);
		return RTK_AMD_ERR_BAD_ARG;
	}
	for (size_t mi = 0; mi < desc->num_meshes; mi++) {
		const uint64_t have = ds->mesh_base[mi + 1] - ds->mesh_base[mi];
		if ((uint64_t)desc->meshes[mi].num_triangles != have) {
			rtk_set_error("%s: mesh %zu has %zu triangles, the scene's has %llu", who, mi, (size_t)desc->meshes[mi].num_triangles, (unsigned long long)have);
			return RTK_AMD_ERR_BAD_ARG;
		}
	}
	return RTK_AMD_OK;
}

} // namespace

// (what make_schedule and make_partial_tables made, given back: rtk_scene_forget_derived)
void RefitSchedule::reset(SceneMem &mem)
{
	mem.release(d_order);
	mem.release(d_level_start);                // (the mesh table lies behind the level starts)
	ready = false;
	d_order = d_level_start = nullptr;
	d_meshes = nullptr;
	level_start.clear();
}

void RefitPartial::reset(SceneMem &mem)
{
	mem.release(d_parent);                     // (one allocation; the table of parents is its first)
	*this = RefitPartial();
}

// Both full refits. who: the public function the error texts name; placements: NULL (rtk_dev_scene_refit) or one per mesh.
static int refit_all(const char *who, rtk_dev_scene *ds, const rtk_scene_desc *desc, const rtk_placement *placements, bool placed, void *stream)
{
	// ---- everything that can be refused is refused here, before HIP is touched
	if (!ds || !desc || (placed && !placements)) { rtk_set_error("%s: NULL argument", who); return RTK_AMD_ERR_BAD_ARG; }
	int rc = check_desc(who, ds, desc);
	if (rc != RTK_AMD_OK) return rc;
	for (size_t mi = 0; mi < desc->num_meshes; mi++) {
		rc = check_mesh_positions(who, &desc->meshes[mi], mi);
		if (rc != RTK_AMD_OK) return rc;
	}
	ScenePass pass(ds, stream);
	return refit_in_pass(pass, desc, placements, nullptr, 0);
}

// Both per-mesh refits, likewise.
static int refit_some(const char *who, rtk_dev_scene *ds, const rtk_scene_desc *desc, const rtk_placement *placements, bool placed, const uint32_t *mesh_ids,
	size_t num_ids, void *stream)
{
	// ---- as above: every refusal before HIP is touched; only the listed meshes' positions (and placements) are looked at
	if (!ds || !desc || (placed && !placements)) { rtk_set_error("%s: NULL argument", who); return RTK_AMD_ERR_BAD_ARG; }
	if (!mesh_ids && num_ids) { rtk_set_error("%s: NULL mesh_ids with %zu ids", who, num_ids); return RTK_AMD_ERR_BAD_ARG; }
	int rc = check_desc(who, ds, desc);
	if (rc != RTK_AMD_OK) return rc;
	std::vector<uint8_t> listed(desc->num_meshes ? desc->num_meshes : 1, 0);
	for (size_t k = 0; k < num_ids; k++) {
		if (mesh_ids[k] >= desc->num_meshes) { rtk_set_error("%s: mesh id %u, the scene has %zu meshes", who, mesh_ids[k], (size_t)desc->num_meshes); return RTK_AMD_ERR_BAD_ARG; }
		listed[mesh_ids[k]] = 1;                                 // (an id that repeats counts once)
	}
	uint64_t listed_tris = 0;
	for (size_t mi = 0; mi < desc->num_meshes; mi++) {
		if (!listed[mi]) continue;
		rc = check_mesh_positions(who, &desc->meshes[mi], mi);
		if (rc != RTK_AMD_OK) return rc;
		listed_tris += desc->meshes[mi].num_triangles;
	}
	ScenePass pass(ds, stream);
	if (listed_tris == 0) {
		// nothing moves: no bit changes, nothing is launched
		ds->refit_nodes = 0;
		ds->refit_ms = 0.0;
		return RTK_AMD_OK;
	}
	// every mesh that has a triangle is listed: that IS the full refit (no mesh it would read is one this call may not read)
	return refit_in_pass(pass, desc, placements, listed_tris == ds->mesh_base.back() ? nullptr : listed.data(), listed_tris);
}

extern "C" int rtk_dev_scene_refit(rtk_dev_scene *ds, const rtk_scene_desc *desc, void *stream)
{
	return refit_all("rtk_dev_scene_refit", ds, desc, nullptr, false, stream);
}

extern "C" int rtk_dev_scene_refit_meshes(rtk_dev_scene *ds, const rtk_scene_desc *desc, const uint32_t *mesh_ids, size_t num_ids, void *stream)
{
	return refit_some("rtk_dev_scene_refit_meshes", ds, desc, nullptr, false, mesh_ids, num_ids, stream);
}

// the placed forms (rtk_amd.h): the same passes, the vertices through rtk_place_rule.h where refit_tri reads them
extern "C" int rtk_dev_scene_refit_placed(rtk_dev_scene *ds, const rtk_scene_desc *desc, const rtk_placement *placements, void *stream)
{
	return refit_all("rtk_dev_scene_refit_placed", ds, desc, placements, true, stream);
}

extern "C" int rtk_dev_scene_refit_meshes_placed(rtk_dev_scene *ds, const rtk_scene_desc *desc, const rtk_placement *placements, const uint32_t *mesh_ids,
	size_t num_ids, void *stream)
{
	return refit_some("rtk_dev_scene_refit_meshes_placed", ds, desc, placements, true, mesh_ids, num_ids, stream);
}

extern "C" double rtk_dev_scene_last_refit_ms(const rtk_dev_scene *ds)
{
	return ds ? ds->refit_ms : 0.0;
}

extern "C" uint64_t rtk_dev_scene_last_refit_nodes(const rtk_dev_scene *ds)
{
	return ds ? ds->refit_nodes : 0;
}
