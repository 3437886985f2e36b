// rtk_winding.hip -- rtk_dev_winding_numbers: the generalized winding number of every query point about a device scene, by the
// rule of rtk_winding_rule.h, and the table of per-subtree moments behind it.
//
// THE TABLE: one 128-byte DevWinding per 128-byte DevNode, at the same index: for each of the node's four child slots the area
// vector N, the centre P and the radius R of everything under the slot, and a copy of the node's four child words, so that a
// node step of the walk reads this ONE line and never the node's boxes. Made on the device, bottom-up over the finished tree:
//   k_wn_leaves    four lanes per node, one per slot (as k_quality_partials has them). A leaf slot sums the moments of its
//                  records and is finished; an empty slot is all zero; an inner slot waits. A node without inner children is
//                  of HEIGHT 0 and says so in level[node].
//   k_wn_level     launched once per height h = 1, 2, ... up to the tree's depth, over all nodes: a node that has no level
//                  yet and whose inner children all have a level BELOW h -- written by an earlier launch, so visible through
//                  the kernel boundary, no fence and no atomic -- sums each inner child's four slots into its own slot and
//                  takes level h. A level written by this very launch is == h and does not count.
//   k_wn_check     counts the nodes left without a level (not a tree: a cycle, a child beyond the array): the making fails.
// The sums of a slot (N, area, area * centroid: 32 bytes per slot) and the levels live in the device's workspace for the time
// of the making (WorkspaceLoan); the table is one entry of the scene's ledger. The root's four sums come home for
// rtk_dev_winding_info.
//
// THE WALK: one query per lane, a fixed grid of resident workgroups (rtk_closest.hip's shape, its leaf decoding, list handling,
// scratch set and status word). No ordering: every child is either accepted by its far term or entered / pushed, so the walk is
// a plain depth-first sum, and a stack entry is one child word. WN_LDS_STACK entries per lane in LDS, [entry][lane], deeper
// ones in the spill area of the (scene, stream) scratch set.
#include "rtk_dev.h"
#include "rtk_winding_rule.h"

#include <atomic>
#include <chrono>
#include <mutex>

#define WN_THREADS 256u
#define WN_WAVES (WN_THREADS / 64u)
#define WN_LDS_STACK 16u           // entries per lane held in LDS: 16 KB per workgroup, never what limits residency
#define WN_TABLE_THREADS 256u      // four lanes per node: 64 nodes per workgroup

namespace {

typedef float wn_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t wn_u32x4 __attribute__((ext_vector_type(4)));

// the sums of one slot while the table is made: N, area, area * centroid (rtk_winding_rule.h 4.)
struct WnSums { float m[8]; };
static_assert(sizeof(WnSums) == 32, "WnSums");

#define WN_NO_LEVEL 0xffffffffu

__device__ __forceinline__ void wn_store_slot(DevWinding *table, const DevNode *nodes, uint32_t node, uint32_t k, const float *sum)
{
	const DevNode *nd = nodes + node;
	const float lo[3] = { nd->bx[0][k], nd->by[0][k], nd->bz[0][k] }, hi[3] = { nd->bx[1][k], nd->by[1][k], nd->bz[1][k] };
	float out[7];
	rtk_winding_slot(sum, lo, hi, out);
	DevWinding *w = table + node;
	w->nx[k] = out[0]; w->ny[k] = out[1]; w->nz[k] = out[2];
	w->px[k] = out[3]; w->py[k] = out[4]; w->pz[k] = out[5];
	w->r[k] = out[6];
}

__global__ void __launch_bounds__(WN_TABLE_THREADS) k_wn_leaves(const DevNode *nodes, uint32_t num_nodes, const DevTri *tris, uint32_t num_tris,
	DevWinding *table, WnSums *sums, uint32_t *level)
{
	const uint32_t idx = blockIdx.x * WN_TABLE_THREADS + threadIdx.x;
	const uint32_t node = idx >> 2, k = idx & 3u;
	if (node >= num_nodes) return;
	const wn_u32x4 ch = *reinterpret_cast<const wn_u32x4 *>(nodes[node].child);
	const uint32_t ref = ch[k];
	table[node].child[k] = ref;
	float sum[8] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };
	const bool inner = ref != RTK_REF_NONE && !(ref & RTK_REF_LEAF);
	if (ref != RTK_REF_NONE && (ref & RTK_REF_LEAF)) {
		uint32_t slot = ref & 0x7fffffffu;
		while (slot < num_tris) {
			const wn_f32x4 *t = reinterpret_cast<const wn_f32x4 *>(reinterpret_cast<const char *>(tris) + (size_t)slot * RTK_TRI_STRIDE);
			const wn_f32x4 A = t[0], B = t[1], C = t[2];
			const float a[3] = { A.x, A.y, A.z }, b[3] = { B.x, B.y, B.z }, c[3] = { C.x, C.y, C.z };
			float m[7];
			rtk_winding_tri_moments(a, b, c, m);
			rtk_winding_add(sum, m);
			if (__float_as_uint(B.w) & RTK_TRI_LAST) break;
			slot++;
		}
	}
	if (!inner) {
		WnSums s;
		for (int i = 0; i < 8; i++) s.m[i] = sum[i];
		sums[(size_t)node * 4u + k] = s;
		if (ref == RTK_REF_NONE) {
			DevWinding *w = table + node;
			w->nx[k] = w->ny[k] = w->nz[k] = w->px[k] = w->py[k] = w->pz[k] = w->r[k] = 0.0f;
		} else wn_store_slot(table, nodes, node, k, sum);
	}
	if (k == 0u) {
		bool any_inner = false;
		for (int j = 0; j < 4; j++) any_inner = any_inner || (ch[j] != RTK_REF_NONE && !(ch[j] & RTK_REF_LEAF));
		level[node] = any_inner ? WN_NO_LEVEL : 0u;
	}
}

__global__ void __launch_bounds__(WN_TABLE_THREADS) k_wn_level(const DevNode *nodes, uint32_t num_nodes, DevWinding *table, WnSums *sums, uint32_t *level, uint32_t h)
{
	const uint32_t idx = blockIdx.x * WN_TABLE_THREADS + threadIdx.x;
	const uint32_t node = idx >> 2, k = idx & 3u;
	if (node >= num_nodes || level[node] != WN_NO_LEVEL) return;
	const wn_u32x4 ch = *reinterpret_cast<const wn_u32x4 *>(table[node].child);
	bool ready = true;
	for (int j = 0; j < 4; j++) {
		const uint32_t c = ch[j];
		if (c == RTK_REF_NONE || (c & RTK_REF_LEAF)) continue;
		ready = ready && c < num_nodes && c != node && level[c] < h;
	}
	if (!ready) return;                                           // (the four lanes of a node decide alike: they read the same words)
	const uint32_t ref = ch[k];
	if (ref != RTK_REF_NONE && !(ref & RTK_REF_LEAF)) {
		const WnSums *cs = sums + (size_t)ref * 4u;
		float sum[8];
		const WnSums first = cs[0];
		for (int i = 0; i < 8; i++) sum[i] = first.m[i];
		for (int j = 1; j < 4; j++) { const WnSums s = cs[j]; rtk_winding_add(sum, s.m); }
		WnSums s;
		for (int i = 0; i < 8; i++) s.m[i] = sum[i];
		s.m[7] = 0.0f;
		sums[(size_t)node * 4u + k] = s;
		wn_store_slot(table, nodes, node, k, sum);
	}
	// (after the reads above in program order, and the four lanes run in one wave: nobody of this node reads level[node] after this)
	if (k == 0u) level[node] = h;
}

__global__ void __launch_bounds__(WN_TABLE_THREADS) k_wn_check(const uint32_t *level, uint32_t num_nodes, unsigned long long *unfinished)
{
	const uint32_t node = blockIdx.x * WN_TABLE_THREADS + threadIdx.x;
	const unsigned long long open = __ballot(node < num_nodes && level[node] == WN_NO_LEVEL);
	if ((threadIdx.x & 63u) == 0u && open) atomicAdd(unfinished, (unsigned long long)__popcll(open));
}

struct WindingParams {
	const DevWinding *table;
	const DevTri *tris;
	uint32_t num_nodes;
	uint32_t num_tris;
	const rtk_point_query *queries;
	const unsigned long long *ids;     // or NULL: 0, 1, 2, ...
	const unsigned long long *count;   // or NULL: n
	float *out;
	unsigned long long *counter;       // the stream's counter words: [RTK_ERROR_WORD] is set by a dropped push
	uint2 *spill;                      // [entry][lane of the launch]; an entry is one child word in .x (the area is the one the other walks size for uint2)
	uint32_t spill_stride;
	uint32_t spill_cap;                // entries per lane
	uint32_t n;
	float beta;
	uint32_t exact;                    // RTK_WINDING_EXACT: no far term is ever taken
};

// COUNT: the visit counts of rtk_dev_winding_numbers_counted, summed per lane and added to the stream's counter words at the end
template <bool COUNT>
__global__ void __launch_bounds__(WN_THREADS) k_winding(WindingParams p)
{
	__shared__ uint32_t s_stack[WN_WAVES][WN_LDS_STACK][64];

	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint32_t (*stk)[64] = s_stack[wave];
	const uint32_t glane = blockIdx.x * WN_THREADS + threadIdx.x;
	uint32_t m = p.n;
	if (p.count) { const unsigned long long listed = *p.count; m = listed < p.n ? (uint32_t)listed : p.n; }
	const unsigned long long step = (unsigned long long)gridDim.x * WN_THREADS;
	uint32_t c_queries = 0, c_nodes = 0, c_leaves = 0, c_tris = 0, c_hits = 0, c_spills = 0;

	for (unsigned long long i = glane; i < m; i += step) {
		const uint32_t r = p.ids ? (uint32_t)p.ids[i] : (uint32_t)i;
		if (r >= p.n) continue;                                   // (the caller's error; nothing is read or written out of range)
		const wn_u32x4 qw = __builtin_nontemporal_load(reinterpret_cast<const wn_u32x4 *>(p.queries + r));
		const float P[3] = { __uint_as_float(qw.x), __uint_as_float(qw.y), __uint_as_float(qw.z) };      // (max_dist2, qw.w, is not read)
		const bool finite = (qw.x & 0x7f800000u) != 0x7f800000u && (qw.y & 0x7f800000u) != 0x7f800000u && (qw.z & 0x7f800000u) != 0x7f800000u;
		if (COUNT) c_queries++;
		if (!finite) { p.out[r] = __uint_as_float(RTK_WINDING_NAN_BITS); continue; }
		float w = 0.0f;
		uint32_t top = (p.num_nodes != 0u && p.num_tris != 0u) ? 0u : RTK_REF_NONE;
		uint32_t sp = 0;

		while (top != RTK_REF_NONE) {
			if ((int32_t)top < 0) {
				// ---------------------------------------------------------------- leaf: its records up to RTK_TRI_LAST
				uint32_t slot = top & 0x7fffffffu;
				if (COUNT) c_leaves++;
				while (slot < p.num_tris) {
					const wn_f32x4 *t = reinterpret_cast<const wn_f32x4 *>(reinterpret_cast<const char *>(p.tris) + (size_t)slot * RTK_TRI_STRIDE);
					const wn_f32x4 A = t[0], B = t[1], C = t[2];
					const float a[3] = { A.x, A.y, A.z }, b[3] = { B.x, B.y, B.z }, c[3] = { C.x, C.y, C.z };
					w = RTK_CL_ADD(w, rtk_winding_triangle(P, a, b, c));
					if (COUNT) c_tris++;
					if (__float_as_uint(B.w) & RTK_TRI_LAST) break;
					slot++;
				}
				top = RTK_REF_NONE;
			} else if (top < p.num_nodes) {
				// ---------------------------------------------------------------- node: one line of the table, four accept tests
				const wn_f32x4 *rec = reinterpret_cast<const wn_f32x4 *>(p.table + top);
				const wn_f32x4 nx = rec[0], ny = rec[1], nz = rec[2], px = rec[3], py = rec[4], pz = rec[5], rr = rec[6];
				const wn_u32x4 ch = *reinterpret_cast<const wn_u32x4 *>(rec + 7);
				if (COUNT) c_nodes++;
				top = RTK_REF_NONE;
#pragma unroll
				for (int k = 0; k < 4; k++) {
					const uint32_t ref = ch[k];
					if (ref == RTK_REF_NONE) continue;
					const float C[3] = { px[k], py[k], pz[k] }, N[3] = { nx[k], ny[k], nz[k] };
					float d[3];
					const float r2 = rtk_winding_r2(P, C, d);
					if (!p.exact && rtk_winding_accept(r2, p.beta, rr[k])) {
						w = RTK_CL_ADD(w, rtk_winding_far_of(N, d, r2));
						if (COUNT) c_hits++;
						continue;
					}
					if (top == RTK_REF_NONE) { top = ref; continue; }
					// A push that does not fit LDS or the spill area is dropped WITHOUT advancing sp and flagged
					if (sp < WN_LDS_STACK) { stk[sp][lane] = ref; sp++; }
					else if (sp - WN_LDS_STACK < p.spill_cap) { p.spill[(size_t)(sp - WN_LDS_STACK) * p.spill_stride + glane].x = ref; sp++; if (COUNT) c_spills++; }
					else p.counter[RTK_ERROR_WORD] = 1ull;
				}
			} else top = RTK_REF_NONE;                                // (a child word beyond the array: not a tree; nothing is read)
			if (top == RTK_REF_NONE && sp != 0u) {
				--sp;
				top = sp < WN_LDS_STACK ? stk[sp][lane] : p.spill[(size_t)(sp - WN_LDS_STACK) * p.spill_stride + glane].x;
			}
		}
		p.out[r] = w;
	}
	if (COUNT) {
		// (the words rtk_dev_closest_points_counted uses; hits: far terms taken)
		atomicAdd(p.counter + 1, (unsigned long long)c_queries);
		atomicAdd(p.counter + 2, (unsigned long long)c_nodes);
		atomicAdd(p.counter + 3, (unsigned long long)c_leaves);
		atomicAdd(p.counter + 4, (unsigned long long)c_tris);
		atomicAdd(p.counter + 5, (unsigned long long)c_hits);
		atomicAdd(p.counter + 6, (unsigned long long)c_spills);
	}
}

// workgroups of k_winding a CU holds, asked once per device
int winding_blocks_per_cu(int device)
{
	static std::atomic<int> known[RTK_MAX_DEVICES];
	if (device < 0 || device >= RTK_MAX_DEVICES) return 4;
	int b = known[device].load(std::memory_order_relaxed);
	if (b == 0) {
		if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, k_winding<false>, (int)WN_THREADS, 0) != hipSuccess || b < 1) b = 4;
		known[device].store(b, std::memory_order_relaxed);
	}
	return b;
}

// the same test as rtk_sign.hip's: a triangle named twice would be counted twice
int winding_refusals(const char *who, const rtk_dev_scene *ds)
{
	if (!ds->records_once || ds->view.num_tris != ds->view.num_prims) {
		rtk_set_error("%s: the scene does not hold exactly one triangle record per primitive (%u records, %u primitives)", who, ds->view.num_tris, ds->view.num_prims);
		return RTK_AMD_ERR_UNSUPPORTED;
	}
	return RTK_AMD_OK;
}

// beta and flags of a call; RTK_AMD_OK or the refusal
int winding_opts(const char *who, const rtk_winding_opts *opts, float *beta, uint32_t *exact)
{
	*beta = 2.0f; *exact = 0u;
	if (!opts) return RTK_AMD_OK;
	if (opts->struct_size != sizeof(rtk_winding_opts) || (opts->flags & ~RTK_WINDING_EXACT) || !(opts->beta >= 0.0f)) {
		rtk_set_error("%s: bad opts (struct_size %u, flags %#x, beta %g)", who, opts->struct_size, opts->flags, (double)opts->beta);
		return RTK_AMD_ERR_BAD_ARG;
	}
	if (opts->beta != 0.0f) *beta = opts->beta;
	*exact = opts->flags & RTK_WINDING_EXACT;
	return RTK_AMD_OK;
}

} // namespace

extern "C" uint32_t rtk_amd_winding_stack_entries(void) { return WN_LDS_STACK; }

// Makes the table if it is not there. The calling thread waits for `stream` that one time: the workspace goes back when this
// returns, and launches on any other stream may use the table as soon as it does.
int rtk_scene_winding_table(const rtk_dev_scene *ds_c, hipStream_t stream)
{
	rtk_dev_scene *ds = const_cast<rtk_dev_scene *>(ds_c);
	if (!ds) return RTK_AMD_ERR_BAD_ARG;
	// LOCK ORDER: scratch_mutex before winding_mutex, never the other way round -- a rebuild drops the table
	// (rtk_scene_forget_derived) while it holds scratch_mutex. So the view is read first, under the lock a rebuild replaces it
	// under, and that lock is let go before the table's own is taken.
	const DevNode *nodes;
	const DevTri *tris;
	uint32_t num_nodes, num_tris, depth;
	{
		std::lock_guard<std::mutex> view_lock(ds->scratch_mutex);
		nodes = ds->view.nodes; tris = ds->view.tris; num_nodes = ds->view.num_nodes; num_tris = ds->view.num_tris; depth = ds->tree.max_depth;
	}
	std::lock_guard<std::mutex> lock(ds->winding_mutex);
	if (ds->winding.d_table) return RTK_AMD_OK;
	int rc = winding_refusals("rtk_scene_winding_table", ds);
	if (rc != RTK_AMD_OK) return rc;
	const auto t_begin = std::chrono::steady_clock::now();
	const size_t table_bytes = (size_t)num_nodes * sizeof(DevWinding);
	DevWinding *table = (DevWinding *)ds->mem.own(table_bytes ? table_bytes : sizeof(DevWinding), table_bytes);
	if (!table) { (void)hipGetLastError(); rtk_set_error("rtk_scene_winding_table: out of device memory (%zu bytes)", table_bytes); return RTK_AMD_ERR_OOM; }
	rtk_dev_winding_info info = {};
	info.nodes = num_nodes;
	info.table_bytes = table_bytes;
	if (num_nodes != 0u) {
		Carve c;
		const size_t o_sums = c.take((size_t)num_nodes * 4u * sizeof(WnSums)), o_level = c.take((size_t)num_nodes * 4u), o_open = c.take(8u);
		WorkspaceLoan loan;
		if (!loan.take(ds->device, c.bytes)) { ds->mem.release(table); return RTK_AMD_ERR_OOM; }
		WnSums *sums = (WnSums *)(loan.base + o_sums);
		uint32_t *level = (uint32_t *)(loan.base + o_level);
		unsigned long long *d_open = (unsigned long long *)(loan.base + o_open);
		const dim3 block(WN_TABLE_THREADS), grid_slots((unsigned)(((size_t)num_nodes * 4u + WN_TABLE_THREADS - 1u) / WN_TABLE_THREADS)),
			grid_nodes((num_nodes + WN_TABLE_THREADS - 1u) / WN_TABLE_THREADS);
		WnSums root[4] = {};
		unsigned long long open = 0;
		hipError_t e = hipMemsetAsync(d_open, 0, 8u, stream);
		if (e == hipSuccess) {
			hipLaunchKernelGGL(k_wn_leaves, grid_slots, block, 0, stream, nodes, num_nodes, tris, num_tris, table, sums, level);
			// one launch per height: a node's height is at most the tree's depth (a node too many costs one idle launch)
			for (uint32_t h = 1; h <= depth + 1u; h++)
				hipLaunchKernelGGL(k_wn_level, grid_slots, block, 0, stream, nodes, num_nodes, table, sums, level, h);
			hipLaunchKernelGGL(k_wn_check, grid_nodes, block, 0, stream, level, num_nodes, d_open);
			e = hipGetLastError();
		}
		if (e == hipSuccess) e = hipMemcpyAsync(root, sums, sizeof(root), hipMemcpyDeviceToHost, stream);
		if (e == hipSuccess) e = hipMemcpyAsync(&open, d_open, sizeof(open), hipMemcpyDeviceToHost, stream);
		// (also on a failure: whatever was enqueued on the workspace is over before the loan ends)
		const hipError_t e_sync = hipStreamSynchronize(stream);
		if (e == hipSuccess) e = e_sync;
		if (e != hipSuccess) {
			rtk_set_error("rtk_scene_winding_table: %s", hipGetErrorString(e));
			ds->mem.release(table);
			return e == hipErrorOutOfMemory ? RTK_AMD_ERR_OOM : RTK_AMD_ERR_HIP;
		}
		if (open != 0ull) {
			rtk_set_error("rtk_scene_winding_table: %llu nodes are not above a finished subtree within %u levels (not a tree)", open, depth + 1u);
			ds->mem.release(table);
			return RTK_AMD_ERR_BAD_SCENE;
		}
		for (int k = 0; k < 4; k++) {
			for (int i = 0; i < 3; i++) info.total_area_vector[i] += (double)root[k].m[i];
			info.total_area += (double)root[k].m[3];
		}
	}
	info.table_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
	ds->winding.info = info;
	ds->winding.d_table = table;
	return RTK_AMD_OK;
}

int rtk_launch_winding(const rtk_dev_scene *ds_c, const rtk_point_query *d_queries, size_t num_queries, const rtk_ray_list *list,
	const rtk_winding_opts *opts, float *d_winding, hipStream_t stream, rtk_trace_counters *counted)
{
	rtk_dev_scene *ds = const_cast<rtk_dev_scene *>(ds_c);
	// everything the host can see is refused here, before any HIP call (rtk_launch_closest's own list, d_winding and the opts)
	if (!ds || (num_queries && (!d_queries || !d_winding))) { rtk_set_error("rtk_dev_winding_numbers: NULL scene, queries or d_winding"); return RTK_AMD_ERR_BAD_ARG; }
	if (list && (list->struct_size < sizeof(rtk_ray_list) || list->flags != 0u || !list->d_count)) {
		rtk_set_error("rtk_dev_winding_numbers: bad list (struct_size %u, flags %#x, d_count %p)", list->struct_size, list->flags, (const void *)list->d_count);
		return RTK_AMD_ERR_BAD_ARG;
	}
	if (num_queries >= ((size_t)1 << 32)) { rtk_set_error("rtk_dev_winding_numbers: %zu queries: a batch holds fewer than 2^32", num_queries); return RTK_AMD_ERR_BAD_ARG; }
	WindingParams p = {};
	int rc = winding_opts("rtk_dev_winding_numbers", opts, &p.beta, &p.exact);
	if (rc != RTK_AMD_OK) return rc;
	if (counted) *counted = rtk_trace_counters();
	if (num_queries == 0) return RTK_AMD_OK;
	if ((rc = winding_refusals("rtk_dev_winding_numbers", ds)) != RTK_AMD_OK) return rc;
	if (!rtk_on_scene_device(ds, "rtk_dev_winding_numbers")) return RTK_AMD_ERR_BAD_ARG;
	if ((rc = rtk_scene_winding_table(ds, stream)) != RTK_AMD_OK) return rc;

	p.queries = d_queries;
	p.ids = list ? reinterpret_cast<const unsigned long long *>(list->d_ids) : nullptr;
	p.count = list ? reinterpret_cast<const unsigned long long *>(list->d_count) : nullptr;
	p.out = d_winding;
	p.n = (uint32_t)num_queries;
	const size_t blocks_needed = (num_queries + WN_THREADS - 1u) / WN_THREADS;
	size_t grid = (size_t)(ds->num_cus > 0 ? ds->num_cus : 1) * (size_t)winding_blocks_per_cu(ds->device);
	if (grid > blocks_needed) grid = blocks_needed;

	// the scratch set of (scene, stream) and the view under the lock a rebuild replaces them under, then the table under its own
	// (the order stated at rtk_scene_winding_table), both held until the launch is enqueued
	std::lock_guard<std::mutex> lock(ds->scratch_mutex);
	std::lock_guard<std::mutex> table_lock(ds->winding_mutex);
	p.table = ds->winding.d_table;
	if (!p.table || ds->winding.info.nodes != ds->view.num_nodes) { rtk_set_error("rtk_dev_winding_numbers: the scene was refitted, split or rebuilt while the call ran"); return RTK_AMD_ERR_BAD_ARG; }
	p.tris = ds->view.tris; p.num_nodes = ds->view.num_nodes; p.num_tris = ds->view.num_tris;
	const size_t entries = ds->tree.stack_entries();
	const size_t spill_cap = entries > WN_LDS_STACK ? entries - WN_LDS_STACK : 0;
	LaunchScratch *sc = ds->scratch.get(stream);
	if (!sc) return RTK_AMD_ERR_OOM;
	if (spill_cap) {
		// (sized for uint2 entries as every other walk sizes it: the area is shared, its two measures do not say an entry's bytes)
		rc = sc->grow_spill(grid * WN_THREADS, spill_cap, sizeof(uint2));
		if (rc != RTK_AMD_OK) return rc;
	}
	p.spill = sc->spill.as<uint2>();
	p.spill_stride = (uint32_t)(spill_cap ? sc->spill.capacity : 0);
	p.spill_cap = (uint32_t)spill_cap;
	p.counter = sc->d_counter;
	if (!counted) {
		hipLaunchKernelGGL(k_winding<false>, dim3((unsigned)grid), dim3(WN_THREADS), 0, stream, p);
		RTK_HIP_CHECK(hipGetLastError(), RTK_AMD_ERR_HIP);
		return RTK_AMD_OK;
	}
	// the counting form: the visit counters start from zero, are brought home and the stream is waited for
	unsigned long long c[8], err = 0;
	RTK_HIP_CHECK(hipMemsetAsync(sc->d_counter, 0, RTK_COUNTER_WORDS * sizeof(unsigned long long), stream), RTK_AMD_ERR_HIP);
	hipLaunchKernelGGL(k_winding<true>, dim3((unsigned)grid), dim3(WN_THREADS), 0, stream, p);
	RTK_HIP_CHECK(hipGetLastError(), RTK_AMD_ERR_HIP);
	RTK_HIP_CHECK(hipMemcpyAsync(c, sc->d_counter, sizeof(c), hipMemcpyDeviceToHost, stream), RTK_AMD_ERR_HIP);
	RTK_HIP_CHECK(hipMemcpyAsync(&err, sc->d_counter + RTK_ERROR_WORD, sizeof(err), hipMemcpyDeviceToHost, stream), RTK_AMD_ERR_HIP);
	RTK_HIP_CHECK(hipStreamSynchronize(stream), RTK_AMD_ERR_HIP);
	counted->rays = c[1]; counted->nodes = c[2]; counted->leaves = c[3]; counted->triangles = c[4]; counted->hits = c[5]; counted->stack_spills = c[6];
	if (err) {
		(void)hipMemsetAsync(sc->d_counter + RTK_ERROR_WORD, 0, sizeof(err), stream);
		rtk_set_error("rtk_dev_winding_numbers_counted: traversal stack overflow (corrupted scene)");
		return RTK_AMD_ERR_BAD_SCENE;
	}
	return RTK_AMD_OK;
}

extern "C" int rtk_dev_scene_prepare_winding(const rtk_dev_scene *ds_c, rtk_dev_winding_info *out, void *stream)
{
	rtk_dev_scene *ds = const_cast<rtk_dev_scene *>(ds_c);
	if (!ds) { rtk_set_error("rtk_dev_scene_prepare_winding: NULL scene"); return RTK_AMD_ERR_BAD_ARG; }
	int rc = winding_refusals("rtk_dev_scene_prepare_winding", ds);
	if (rc != RTK_AMD_OK) return rc;
	bool made;
	{
		std::lock_guard<std::mutex> lock(ds->winding_mutex);
		made = ds->winding.d_table != nullptr;
	}
	if (!made) {
		if (!rtk_on_scene_device(ds, "rtk_dev_scene_prepare_winding")) return RTK_AMD_ERR_BAD_ARG;
		if ((rc = rtk_scene_winding_table(ds, (hipStream_t)stream)) != RTK_AMD_OK) return rc;
	}
	if (out) {
		std::lock_guard<std::mutex> lock(ds->winding_mutex);
		*out = ds->winding.info;
		if (made) out->table_ms = 0.0;
	}
	return RTK_AMD_OK;
}

extern "C" int rtk_dev_scene_winding_moments(const rtk_dev_scene *ds_c, float *d_out, void *stream)
{
	rtk_dev_scene *ds = const_cast<rtk_dev_scene *>(ds_c);
	if (!ds || !d_out) { rtk_set_error("rtk_dev_scene_winding_moments: NULL scene or d_out"); return RTK_AMD_ERR_BAD_ARG; }
	int rc = winding_refusals("rtk_dev_scene_winding_moments", ds);
	if (rc != RTK_AMD_OK) return rc;
	if (!rtk_on_scene_device(ds, "rtk_dev_scene_winding_moments")) return RTK_AMD_ERR_BAD_ARG;
	if ((rc = rtk_scene_winding_table(ds, (hipStream_t)stream)) != RTK_AMD_OK) return rc;
	std::lock_guard<std::mutex> lock(ds->winding_mutex);
	if (!ds->winding.d_table) { rtk_set_error("rtk_dev_scene_winding_moments: the scene was refitted, split or rebuilt while the call ran"); return RTK_AMD_ERR_BAD_ARG; }
	if (ds->winding.info.table_bytes)
		RTK_HIP_CHECK(hipMemcpyAsync(d_out, ds->winding.d_table, ds->winding.info.table_bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream), RTK_AMD_ERR_HIP);
	return RTK_AMD_OK;
}

extern "C" int rtk_dev_winding_numbers(const rtk_dev_scene *ds, const rtk_point_query *d_queries, size_t num_queries, const rtk_ray_list *list,
	const rtk_winding_opts *opts, float *d_winding, void *stream)
{
	return rtk_launch_winding(ds, d_queries, num_queries, list, opts, d_winding, (hipStream_t)stream, nullptr);
}

extern "C" int rtk_dev_winding_numbers_counted(const rtk_dev_scene *ds, const rtk_point_query *d_queries, size_t num_queries,
	const rtk_winding_opts *opts, float *d_winding, rtk_trace_counters *out)
{
	if (!out) { rtk_set_error("rtk_dev_winding_numbers_counted: NULL out"); return RTK_AMD_ERR_BAD_ARG; }
	return rtk_launch_winding(ds, d_queries, num_queries, nullptr, opts, d_winding, nullptr, out);
}
