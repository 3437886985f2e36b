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
// This file holds the kernels and the HIP calls. What the host decides between them -- refusals, where positions are read from
// and staged, sizes and offsets, the workspace to borrow, runs, the dirty-set decision, which heights share a launch -- is
// rtk_refit_plan.h, which includes no HIP; refit_on_device carries one plan out as stage_inputs, gather_triangles, remake_boxes,
// finish_refit.
#include "rtk_dev.h"
#include "rtk_place_rule.h"
#include "rtk_refit_plan.h"

#include <math.h>
#include <string.h>

#include <vector>

namespace {

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

// ---------------------------------------------------------------------------------- host: tables made once per scene
// (sizes, offsets, sort widths and the rules of the sweeps: rtk_refit_plan.h)

// what make_schedule allocates, given back on every way out that has not handed it to the scene
struct FreeUnlessKept { void *&p; ~FreeUnlessKept() { if (p) (void)hipFree(p); } };
#define SCHEDULE_CHECK(expr) do { if ((expr) != hipSuccess) { rtk_set_error("rtk_dev_scene_refit: schedule: %s failed: %s", #expr, hipGetErrorString(hipGetLastError())); return RTK_AMD_ERR_HIP; } } while (0)

// heights, node numbers grouped by height, the mesh table's memory: once per scene. tmp: schedule_tmp(num_nodes).bytes of
// device memory (the borrowed workspace: no allocation of a quarter of a gigabyte at 10M triangles, freed again at once)
int make_schedule(rtk_dev_scene *ds, hipStream_t stream, char *tmp)
{
	RefitSchedule &rs = ds->refit;
	if (rs.ready) return RTK_AMD_OK;
	const uint32_t n = ds->view.num_nodes;
	const size_t num_meshes = ds->mesh_base.empty() ? 0 : ds->mesh_base.size() - 1;
	const ScheduleTmp T = schedule_tmp(n, rtk_sort_scratch_words(n));
	uint32_t *d_height = (uint32_t *)(tmp + T.o_height), *d_changed = (uint32_t *)(tmp + T.o_changed), *d_ls = (uint32_t *)(tmp + T.o_ls);
	unsigned long long *keys_a = (unsigned long long *)(tmp + T.o_ka), *keys_b = (unsigned long long *)(tmp + T.o_kb);
	void *d_order = nullptr, *d_small = nullptr;
	FreeUnlessKept free_order{ d_order }, free_small{ d_small };
	const unsigned blocks = (n + 255u) / 256u;
	SCHEDULE_CHECK(hipMemsetAsync(d_height, 0, (size_t)n * 4, stream));
	// the last sweep of a round must change nothing: the one wait of the host
	int rc = RTK_AMD_OK;
	uint32_t sweeps = 0;
	for (bool first = true, converged = false; !converged && rc == RTK_AMD_OK; first = false) {
		const uint32_t round = sweep_round(first, ds->tree.max_depth);
		uint32_t h_changed = 0;
		for (uint32_t k = 0; k + 1u < round; k++) hipLaunchKernelGGL(k_refit_heights, dim3(blocks), dim3(256), 0, stream, ds->view.nodes, n, d_height, d_changed);
		if (hipMemsetAsync(d_changed, 0, 4, stream) != hipSuccess) { rc = RTK_AMD_ERR_HIP; break; }
		hipLaunchKernelGGL(k_refit_heights, dim3(blocks), dim3(256), 0, stream, ds->view.nodes, n, d_height, d_changed);
		sweeps += round;
		if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&h_changed, d_changed, 4, hipMemcpyDeviceToHost, stream) != hipSuccess ||
			hipStreamSynchronize(stream) != hipSuccess) { rc = RTK_AMD_ERR_HIP; break; }
		converged = h_changed == 0u;
		if (!converged && sweeps_exhausted(sweeps, n)) rc = RTK_AMD_ERR_BAD_SCENE;
	}
	if (rc != RTK_AMD_OK) { rtk_set_error("rtk_dev_scene_refit: schedule: heights did not settle (%s)", rc == RTK_AMD_ERR_HIP ? hipGetErrorString(hipGetLastError()) : "not a tree"); return rc; }
	hipLaunchKernelGGL(k_refit_keys, dim3(blocks), dim3(256), 0, stream, d_height, n, keys_a);
	const unsigned long long *sorted = keys_a;
	if (n > 1u) sorted = rtk_sort_words_async(keys_a, keys_b, n, 32u, 32u + height_sort_bits(n), (uint32_t *)(tmp + T.o_sort), stream) ? keys_b : keys_a;
	SCHEDULE_CHECK(hipMalloc(&d_order, (size_t)n * 4));
	hipLaunchKernelGGL(k_refit_order, dim3(blocks), dim3(256), 0, stream, sorted, n, (uint32_t *)d_order, d_ls);
	unsigned long long last = 0;
	SCHEDULE_CHECK(hipGetLastError());
	SCHEDULE_CHECK(hipMemcpyAsync(&last, sorted + (n - 1u), 8, hipMemcpyDeviceToHost, stream));
	SCHEDULE_CHECK(hipStreamSynchronize(stream));
	const uint32_t heights = (uint32_t)(last >> 32) + 1u;
	if (heights > n) { rtk_set_error("rtk_dev_scene_refit: schedule: %u heights for %u nodes", heights, n); return RTK_AMD_ERR_BAD_SCENE; }
	std::vector<uint32_t> level_start;
	level_start.resize((size_t)heights + 1);
	SCHEDULE_CHECK(hipMemcpy(level_start.data(), d_ls, level_start.size() * 4, hipMemcpyDeviceToHost));
	if (!level_starts_sane(level_start, n)) { rtk_set_error("rtk_dev_scene_refit: schedule: heights are not contiguous"); return RTK_AMD_ERR_BAD_SCENE; }
	const ScheduleSmall small = schedule_small(heights, num_meshes);
	SCHEDULE_CHECK(hipMalloc(&d_small, small.bytes));
	SCHEDULE_CHECK(hipMemcpy(d_small, level_start.data(), level_start.size() * 4, hipMemcpyHostToDevice));
	ds->mem.adopt(d_order, (size_t)n * 4);
	ds->mem.adopt(d_small, small.counted);
	rs.d_order = (uint32_t *)d_order;
	rs.d_level_start = (uint32_t *)d_small;
	rs.d_meshes = (char *)d_small + small.o_meshes;
	rs.level_start.swap(level_start);
	rs.ready = true;
	d_order = d_small = nullptr;                               // (the scene's now)
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

// parent[], the node of every slot's leaf, the slots grouped by mesh, and the memory of the dirty set: once per scene, after
// the schedule. tmp: tables_tmp(num_tris).bytes of device memory (the borrowed workspace).
int make_partial_tables(rtk_dev_scene *ds, hipStream_t stream, char *tmp)
{
	RefitPartial &rp = ds->partial;
	if (rp.ready) return RTK_AMD_OK;
	const DevSceneView &v = ds->view;
	const uint32_t n = v.num_nodes, nt = v.num_tris;
	const size_t num_meshes = ds->mesh_base.size() - 1;
	const PartialTables P = partial_tables(n, nt, num_meshes, ds->refit.level_start.size() - 1, (n + RTK_DIRTY_BLOCK - 1u) / RTK_DIRTY_BLOCK);
	void *mem = nullptr;
	if (hipMalloc(&mem, P.bytes) != hipSuccess) { (void)hipGetLastError(); rtk_set_error("rtk_dev_scene_refit_meshes: out of device memory"); return RTK_AMD_ERR_OOM; }
	char *base = (char *)mem;
	uint32_t *d_parent = (uint32_t *)(base + P.o_parent), *d_slot_node = (uint32_t *)(base + P.o_slot_node), *d_mesh_slots = (uint32_t *)(base + P.o_mesh_slots);
	const TablesTmp T = tables_tmp(nt, rtk_sort_scratch_words(nt));
	unsigned long long *keys_a = (unsigned long long *)(tmp + T.o_ka), *keys_b = (unsigned long long *)(tmp + T.o_kb);
	// (RTK_REF_NONE everywhere first: the root has no parent, and a slot no leaf names stays without a node)
	bool ok = hipMemsetAsync(base, 0xff, P.o_mesh_slots, stream) == hipSuccess && hipMemsetAsync(base + P.o_dirty, 0, P.o_list - P.o_dirty, stream) == hipSuccess;
	if (ok) {
		hipLaunchKernelGGL(k_refit_parents, dim3((unsigned)(((size_t)n * 4 + 255) / 256)), dim3(256), 0, stream, v.nodes, n, v.tris, nt, d_parent, d_slot_node);
		const unsigned blocks = (nt + 255u) / 256u;
		hipLaunchKernelGGL(k_refit_mesh_keys, dim3(blocks), dim3(256), 0, stream, v.slot_mesh, nt, keys_a);
		const uint32_t bits = mesh_sort_bits(num_meshes);
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
	ds->mem.adopt(mem, P.counted);
	rp.d_parent = d_parent; rp.d_slot_node = d_slot_node; rp.d_mesh_slots = d_mesh_slots;
	rp.d_dirty = (uint32_t *)(base + P.o_dirty); rp.d_list = (uint32_t *)(base + P.o_list); rp.d_block = (uint32_t *)(base + P.o_block);
	rp.d_list_start = (uint32_t *)(base + P.o_list_start); rp.d_ranges = base + P.o_ranges;
	rp.epoch = 0;
	rp.ready = true;
	return RTK_AMD_OK;
}

// ---------------------------------------------------------------------------------- host: one refit, step by step

// One call between its steps. listed: NULL = every mesh (rtk_dev_scene_refit), else one flag per mesh
// (rtk_dev_scene_refit_meshes), with listed_tris triangles (not zero) in the flagged ones.
struct RefitCall {
	rtk_dev_scene *ds;
	hipStream_t stream;
	const uint8_t *listed;
	uint64_t listed_tris;
	RefitSource src;                           // where the positions are read from (plan_source)
	const rtk_placement *d_places = nullptr;   // the placed forms: the placement table in the borrowed workspace, for the length of the call
	bool dirty_set = false;                    // boxes and compressed nodes are remade for the nodes above the listed meshes alone
};

// The workspace, what is made once per scene in it, then the caller's host-resident positions and the placements in it, and
// the mesh table that says where each mesh is read from.
int stage_inputs(RefitCall &c, WorkspaceLoan &loan)
{
	rtk_dev_scene *ds = c.ds;
	const DevSceneView &v = ds->view;
	RefitSource &src = c.src;
	const size_t borrow = plan_borrow(ds->refit.ready, schedule_tmp(v.num_nodes, rtk_sort_scratch_words(v.num_nodes)),
		c.listed && !ds->partial.ready, tables_tmp(v.num_tris, rtk_sort_scratch_words(v.num_tris)), src.upload_bytes);
	if (borrow && !loan.take(ds->device, borrow)) return RTK_AMD_ERR_OOM;
	int rc = make_schedule(ds, c.stream, loan.base);
	if (rc == RTK_AMD_OK && c.listed) rc = make_partial_tables(ds, c.stream, loan.base);
	if (rc != RTK_AMD_OK) return rc;
	for (size_t mi = 0; mi < src.staged.size(); mi++) {
		if (!src.staged[mi]) continue;
		RTK_PASS_CHECK("rtk_dev_scene_refit", hipMemcpyAsync(loan.base + src.staged_at[mi], src.table[mi].pos, src.staged[mi], hipMemcpyHostToDevice, c.stream));
		src.table[mi].pos = loan.base + src.staged_at[mi];
	}
	if (!src.places.empty()) {
		RTK_PASS_CHECK("rtk_dev_scene_refit", hipMemcpyAsync(loan.base + src.places_at, src.places.data(), src.places.size() * sizeof(rtk_placement), hipMemcpyHostToDevice, c.stream));
		c.d_places = (const rtk_placement *)(loan.base + src.places_at);
	}
	// a mesh in device memory was written by the caller's own work, possibly still in flight on the NULL stream (as in a build)
	if (src.any_device && c.stream != nullptr) RTK_PASS_CHECK("rtk_dev_scene_refit", hipStreamSynchronize(nullptr));
	if (!src.staged.empty()) RTK_PASS_CHECK("rtk_dev_scene_refit", hipMemcpyAsync(ds->refit.d_meshes, src.table.data(), src.staged.size() * sizeof(RefitMesh), hipMemcpyHostToDevice, c.stream));
	return RTK_AMD_OK;
}

// MODE, MARK and PLACED are compile-time variants, picked by the plan's mode and the call's flags: [!MARK][!PLACED][2 - MODE] and
// [!PLACED][2 - MODE]. (The code object holds the instantiations in the order they are first named in, so the tables name them
// in the order the launches always did: its bytes stay what they were.) The unplaced ones are what they were before there were
// placements.
typedef void (*RefitListedKernel)(DevTri *, uint32_t, const uint32_t *, const uint32_t *, const RefitMesh *, uint32_t, const uint32_t *, const uint32_t *, const RefitRange *, uint32_t,
	uint32_t, const uint32_t *, uint32_t *, uint32_t, uint32_t, const rtk_placement *);
typedef void (*RefitTrisKernel)(DevTri *, uint32_t, const uint32_t *, const uint32_t *, const RefitMesh *, uint32_t, const rtk_placement *);
const RefitListedKernel LISTED_KERNELS[2][2][3] = {
	{ { k_refit_tris_listed<2, true, true>, k_refit_tris_listed<1, true, true>, k_refit_tris_listed<0, true, true> },
	  { k_refit_tris_listed<2, true, false>, k_refit_tris_listed<1, true, false>, k_refit_tris_listed<0, true, false> } },
	{ { k_refit_tris_listed<2, false, true>, k_refit_tris_listed<1, false, true>, k_refit_tris_listed<0, false, true> },
	  { k_refit_tris_listed<2, false, false>, k_refit_tris_listed<1, false, false>, k_refit_tris_listed<0, false, false> } } };
const RefitTrisKernel TRIS_KERNELS[2][3] = {
	{ k_refit_tris<2, true>, k_refit_tris<1, true>, k_refit_tris<0, true> }, { k_refit_tris<2, false>, k_refit_tris<1, false>, k_refit_tris<0, false> } };

// The position bytes of the triangle records: of every slot, or of the listed meshes' slots, which also mark the dirty set.
int gather_triangles(RefitCall &c)
{
	rtk_dev_scene *ds = c.ds;
	const DevSceneView &v = ds->view;
	DevTri *tris = const_cast<DevTri *>(v.tris);
	const RefitMesh *dm = (const RefitMesh *)ds->refit.d_meshes;
	const uint32_t num_meshes = (uint32_t)c.src.staged.size();
	if (c.listed) {
		RefitPartial &rp = ds->partial;
		const RefitRuns runs = plan_runs(c.listed, ds->mesh_base, num_meshes);
		RTK_PASS_CHECK("rtk_dev_scene_refit", hipMemcpyAsync(rp.d_ranges, runs.ranges.data(), runs.ranges.size() * sizeof(RefitRange), hipMemcpyHostToDevice, c.stream));
		const EpochStep step = next_epoch(rp.epoch);
		if (step.clear) RTK_PASS_CHECK("rtk_dev_scene_refit", hipMemsetAsync(rp.d_dirty, 0, (size_t)v.num_nodes * 4, c.stream));
		rp.epoch = step.epoch;                                     // (after the clear: one that fails is tried again by the next call)
		const uint32_t total = (uint32_t)runs.threads;
		hipLaunchKernelGGL(LISTED_KERNELS[!c.dirty_set][!c.d_places][2 - c.src.mode], dim3((total + 255u) / 256u), dim3(256), 0, c.stream, tris, v.num_tris, v.vertex_index,
			v.slot_mesh, dm, num_meshes, rp.d_mesh_slots, rp.d_slot_node, (const RefitRange *)rp.d_ranges, (uint32_t)runs.ranges.size(), total, rp.d_parent, rp.d_dirty,
			v.num_nodes, rp.epoch, c.d_places);
	} else if (v.num_tris)
		hipLaunchKernelGGL(TRIS_KERNELS[!c.d_places][2 - c.src.mode], dim3((v.num_tris + 255u) / 256u), dim3(256), 0, c.stream, tris, v.num_tris, v.vertex_index, v.slot_mesh, dm,
			num_meshes, c.d_places);
	RTK_PASS_CHECK("rtk_dev_scene_refit", hipGetLastError());
	return RTK_AMD_OK;
}

// The child boxes, bottom-up by height: one walk over the launches the schedule's level starts give (plan_levels). The dirty-set
// form first compacts the dirty nodes in the schedule's order and finds where each height begins among them (all of it stays on
// the device); it then differs in the kernel of a large height, whose grid is capped because it strides, and in the node list and
// starts k_refit_small is handed.
int remake_boxes(RefitCall &c)
{
	rtk_dev_scene *ds = c.ds;
	const DevSceneView &v = ds->view;
	const RefitSchedule &rs = ds->refit;
	const RefitPartial &rp = ds->partial;
	DevTri *tris = const_cast<DevTri *>(v.tris);
	DevNode *nodes = const_cast<DevNode *>(v.nodes);
	if (c.dirty_set) {
		const uint32_t n = v.num_nodes, nb = (n + RTK_DIRTY_BLOCK - 1u) / RTK_DIRTY_BLOCK, heights = (uint32_t)rs.level_start.size() - 1u;
		hipLaunchKernelGGL(k_dirty_count, dim3(nb), dim3(256), 0, c.stream, rs.d_order, n, rp.d_dirty, rp.epoch, rp.d_block);
		hipLaunchKernelGGL(k_dirty_scan, dim3(1), dim3(1024), 0, c.stream, rp.d_block, nb, rs.d_order, n, rp.d_dirty, rp.epoch, rs.d_level_start, heights, rp.d_list_start);
		hipLaunchKernelGGL(k_dirty_scatter, dim3(nb), dim3(256), 0, c.stream, rs.d_order, n, rp.d_dirty, rp.epoch, rp.d_block, rp.d_list);
	}
	const uint32_t *order = c.dirty_set ? rp.d_list : rs.d_order, *starts = c.dirty_set ? rp.d_list_start : rs.d_level_start;
	for (const LevelStep &s : plan_levels(rs.level_start)) {
		if (s.small) hipLaunchKernelGGL(k_refit_small, dim3(1), dim3(REFIT_SMALL_THREADS), 0, c.stream, nodes, tris, v.num_nodes, v.num_tris, order, starts, s.h, s.h1);
		else if (c.dirty_set) hipLaunchKernelGGL(k_refit_level_list, dim3((unsigned)(s.blocks > 2048 ? 2048 : s.blocks)), dim3(256), 0, c.stream, nodes, tris, v.num_nodes, v.num_tris, order, starts, s.h);
		else hipLaunchKernelGGL(k_refit_level, dim3((unsigned)s.blocks), dim3(256), 0, c.stream, nodes, tris, v.num_nodes, v.num_tris, order, s.begin, s.end);
	}
	RTK_PASS_CHECK("rtk_dev_scene_refit", hipGetLastError());
	return RTK_AMD_OK;
}

// Compressed nodes, order words and constants, and the host fields that follow from them.
int finish_refit(RefitCall &c)
{
	rtk_dev_scene *ds = c.ds;
	const DevSceneView &v = ds->view;
	bool full_finish = true;
	if (c.dirty_set) {
		const RefitPartial &rp = ds->partial;
		const uint32_t nb = (v.num_nodes + RTK_DIRTY_BLOCK - 1u) / RTK_DIRTY_BLOCK;
		RTK_PASS_CHECK("rtk_dev_scene_refit", hipMemcpyAsync(&ds->partial_readback, rp.d_block + nb, 4, hipMemcpyDeviceToHost, c.stream));
		// Of the dirty nodes, the constants from the root (dirty whenever anything moved). The misfit count is one over ALL nodes:
		// the list form is the whole answer only if the others have none (the scene is on its compressed nodes now) and none of
		// the dirty ones has one either; else the full pass below.
		if (v.qnodes && ds->tree.qnodes_mem) {
			const int rc = rtk_quantize_node_list(ds, c.stream, rp.d_list, rp.d_block + nb);
			if (rc != RTK_AMD_OK) return rc;
			RTK_PASS_CHECK("rtk_dev_scene_refit", hipStreamSynchronize(c.stream));
			full_finish = ds->tree.consts_readback.qnode_misfits != 0u;
		}
	}
	if (full_finish) {
		// (the block is cleared first: the misfit count starts at zero); every box lies inside the root's now, so no bound is passed in
		const int rc = rtk_quantize_nodes(ds, c.stream, nullptr, const_cast<DevNodeQ *>(ds->tree.qnodes_mem), 0.0f, 0xffffffffu, false, true);
		if (rc != RTK_AMD_OK) return rc;
		RTK_PASS_CHECK("rtk_dev_scene_refit", hipStreamSynchronize(c.stream));
	}
	{
		// (the trace path reads these host fields under the same mutex when it enqueues a launch)
		std::lock_guard<std::mutex> lock(ds->scratch_mutex);
		rtk_quantize_finish(ds);
	}
	rtk_scene_forget_derived(ds, RTK_FORGET_BOXES);
	ds->tree.boxes_exact = true;
	ds->refit_nodes = c.dirty_set ? ds->partial_readback : v.num_nodes;
	return RTK_AMD_OK;
}

// everything behind the argument checks; the scene's device is current. placements: NULL, or one per mesh (the _placed entry
// points; only the entries of meshes that are read are looked at).
int refit_on_device(rtk_dev_scene *ds, const rtk_scene_desc *desc, const rtk_placement *placements, hipStream_t stream, WorkspaceLoan &loan, const uint8_t *listed, uint64_t listed_tris)
{
	int rc = rtk_scene_side_arrays(ds, stream);
	if (rc != RTK_AMD_OK) return rc;
	if (ds->view.num_nodes == 0u) { rtk_set_error("rtk_dev_scene_refit: scene without a root node"); return RTK_AMD_ERR_BAD_SCENE; }
	RefitCall c{ ds, stream, listed, listed_tris, plan_source(desc, placements, listed, rtk_is_device_ptr, ds->refit.max_vertex_ready ? ds->refit.max_vertex.data() : nullptr) };
	if (c.src.need_max_vertex) {
		rc = make_max_vertex(ds, stream);
		if (rc != RTK_AMD_OK) return rc;
		c.src = plan_source(desc, placements, listed, rtk_is_device_ptr, ds->refit.max_vertex.data());
	}
	rc = stage_inputs(c, loan);
	if (rc != RTK_AMD_OK) return rc;
	// Until this call has succeeded nobody may take the boxes it leaves alone for exact unions.
	c.dirty_set = plan_dirty_set(listed != nullptr, ds->tree.boxes_exact, listed_tris, ds->view.num_tris, partial_max_share());
	ds->tree.boxes_exact = false;
	rc = gather_triangles(c);
	if (rc == RTK_AMD_OK) rc = remake_boxes(c);
	if (rc == RTK_AMD_OK) rc = finish_refit(c);
	return rc;
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
// Everything that can be refused is refused by the check, before HIP is touched.
static int refit_all(const char *who, rtk_dev_scene *ds, const rtk_scene_desc *desc, const rtk_placement *placements, bool placed, void *stream)
{
	const RefitScope scope = check_refit_all(rtk_set_error, who, ds ? &ds->mesh_base : nullptr, desc, placements, placed);
	if (scope.rc != RTK_AMD_OK) return scope.rc;
	ScenePass pass(ds, stream);
	return refit_in_pass(pass, desc, placements, nullptr, 0);
}

// Both per-mesh refits, likewise.
static int refit_some(const char *who, rtk_dev_scene *ds, const rtk_scene_desc *desc, const rtk_placement *placements, bool placed, const uint32_t *mesh_ids,
	size_t num_ids, void *stream)
{
	const RefitScope scope = check_refit_some(rtk_set_error, who, ds ? &ds->mesh_base : nullptr, desc, placements, placed, mesh_ids, num_ids);
	if (scope.rc != RTK_AMD_OK) return scope.rc;
	ScenePass pass(ds, stream);
	if (scope.nothing) {
		ds->refit_nodes = 0;
		ds->refit_ms = 0.0;
		return RTK_AMD_OK;
	}
	return refit_in_pass(pass, desc, placements, scope.listed(), scope.listed_tris);
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
