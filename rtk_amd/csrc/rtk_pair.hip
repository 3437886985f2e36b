// rtk_pair.hip -- rtk_dev_closest_triangles: for every query triangle (or segment, or point) the nearest triangle of a device
// scene, its squared distance, the barycentrics on it and the two nearest points, by the rule of rtk_pair_rule.h. The result is
// a function of the scene's triangle records and the query alone (DESIGN.md "Closest triangles"): the tree and the order of the
// walk only decide which records are never looked at.
//
// k_closest's frame (rtk_closest.hip): one query per lane of a 64-wide wave, a fixed grid of resident workgroups that steps
// through the batch, exact 128-byte nodes only, the bound of all four child boxes against the query's box
// (rtk_pair_box_bound), empty slots and children that rtk_pair_skip rules out left out, the nearest child entered, the others
// pushed far to near with their bounds, and the bound looked at again at the pop because the best distance has shrunk since the
// push. A leaf is its run of DevTri records up to RTK_TRI_LAST. The stack is [entry][lane] in LDS, 8 bytes an entry, with the
// deeper part in the spill area of the (scene, stream) scratch set; a push that fits neither is dropped WITHOUT advancing and
// flagged in the stream's launch-error word. A child word beyond the node array and a slot beyond the triangle array are not
// followed.
//
// WHAT IS HOISTED (rtk_pair_hoist, once per query, 30 floats): the query's vertices, its box, its three edges, their squared
// lengths and nA. Per record, from one 48-byte fetch: the filter (an integer comparison, and nine vertex comparisons under the
// flag), then the bound of the record's OWN box against the query's -- the node skip's inequality: a record whose box bound
// exceeds the best distance so far, or reaches the limit, cannot win and is not evaluated --, then rtk_pair_evaluate: the closed
// box test and the six edge-against-triangle crossings first, then six point-triangle walks and nine edge pairs.
//
// FLOATING POINT: the flags of rtk_closest.hip (no contraction, IEEE quotients); every bit is the rule header's.
#include "rtk_dev.h"
#include "rtk_pair_rule.h"

#include <atomic>
#include <mutex>

// PC_RESOURCES: the compiler's report (gfx950, -O3, -Rpass-analysis=kernel-resource-usage, and the code object's metadata) for
// the two instantiated forms; scratch 0 and no VGPR spills in both, so neither the node loop nor the record loop touches
// private memory; the SGPRs past the 106 it may use go to lanes of a VGPR (counted in the VGPR column), not to memory:
//                     VGPRs   AGPRs   SGPRs (spilled)   scratch   LDS per workgroup   waves per SIMD
//   plain    <0>       254      0       106 (14)          0 B         32 768 B              2
//   counted  <1>       254      4       106 (10)          0 B         32 768 B              1
// A workgroup is four waves, one per SIMD, so "workgroups per CU" and "waves per SIMD" are the same number: the registers
// decide (512 / 256 = 2; the counting form's AGPRs begin at 256, 260 registers in all, which leaves room for one), the LDS (160 KB / 32 KB) would hold five. rtk_touch.hip
// sits at 191 to 203 VGPRs: here 30 hoisted floats of the query, the record's vertices, box, edges and squared edge lengths and
// the running best (nine floats and an id) are alive across the straight-line code of six crossings, six point-triangle walks and
// nine edge pairs. The six crossings are six calls with constant indices (rtk_pair_evaluate): as a loop that picked its edge
// through a selected pointer they kept the hoisted arrays and the record in 208 bytes of private memory per lane, written per
// query and per record fetched. Hoisting less is the way to a third wave (168 VGPRs) and has not been tried. Not tuned.

#define PC_THREADS 256u
#define PC_WAVES (PC_THREADS / 64u)
#define PC_LDS_STACK 16u           // entries per lane held in LDS, 8 bytes each: 32 KB per workgroup

static_assert(RTK_TOUCH_RULE_SKIP_SHARED_VERTEX == RTK_TOUCH_SKIP_SHARED_VERTEX, "the rule header's flag is the interface's");
static_assert(sizeof(rtk_tri_query) == 36, "a float32 [n, 9] tensor is a batch of queries");

namespace {

struct PairParams {
	const DevNode *nodes;
	const DevTri *tris;
	uint32_t num_nodes;
	uint32_t num_tris;
	const rtk_tri_query *queries;
	const float *max_dist2;            // or NULL: RTK_INF for every query; indexed by query slot
	const uint32_t *first_prim;        // or NULL: 0 for every query; indexed by query slot
	const unsigned long long *ids;     // or NULL: 0, 1, 2, ...
	const unsigned long long *count;   // or NULL: n
	rtk_closest_record *records;
	float *points_query;               // or NULL
	float *points_scene;               // or NULL
	unsigned long long *counter;       // the stream's counter words: [RTK_ERROR_WORD] is set by a dropped push
	uint2 *spill;                      // [entry][lane of the launch]
	uint32_t spill_stride;
	uint32_t spill_cap;                // entries per lane
	uint32_t n;
	uint32_t flags;                    // RTK_TOUCH_SKIP_SHARED_VERTEX
};

typedef float pc_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t pc_u32x4 __attribute__((ext_vector_type(4)));

// ascending by key; the reference travels with it
__device__ __forceinline__ void pc_cswap(uint32_t &ka, uint32_t &ra, uint32_t &kb, uint32_t &rb)
{
	const bool swap = kb < ka;
	const uint32_t k0 = swap ? kb : ka, k1 = swap ? ka : kb, r0 = swap ? rb : ra, r1 = swap ? ra : rb;
	ka = k0; kb = k1; ra = r0; rb = r1;
}

// COUNT: the visit counts of rtk_dev_closest_triangles_counted, summed per lane and added to the stream's counter words at the end
// (triangles = records fetched; a record that its own box rules out is fetched and counted, not evaluated)
template <bool COUNT>
__global__ void __launch_bounds__(PC_THREADS) k_pair(PairParams p)
{
	__shared__ uint2 s_stack[PC_WAVES][PC_LDS_STACK][64];

	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint2 (*stk)[64] = s_stack[wave];
	const uint32_t glane = blockIdx.x * PC_THREADS + threadIdx.x;
	uint32_t m = p.n;
	if (p.count) { const unsigned long long listed = *p.count; m = listed < p.n ? (uint32_t)listed : p.n; }
	const unsigned long long step = (unsigned long long)gridDim.x * PC_THREADS;
	uint32_t c_queries = 0, c_nodes = 0, c_leaves = 0, c_tris = 0, c_hits = 0, c_spills = 0;

	for (unsigned long long i = glane; i < m; i += step) {
		const uint32_t r = p.ids ? (uint32_t)p.ids[i] : (uint32_t)i;
		if (r >= p.n) continue;                                   // (the caller's error; nothing is read or written out of range)
		// (36 bytes at a stride of 36: a query is only 4-byte aligned)
		const float *qw = reinterpret_cast<const float *>(p.queries + r);
		const float a0[3] = { qw[0], qw[1], qw[2] }, a1[3] = { qw[3], qw[4], qw[5] }, a2[3] = { qw[6], qw[7], qw[8] };
		const uint32_t max_bits = p.max_dist2 ? reinterpret_cast<const uint32_t *>(p.max_dist2)[r] : __float_as_uint(RTK_INF);
		const float max2 = __uint_as_float(max_bits);
		const uint32_t first = p.first_prim ? p.first_prim[r] : 0u;
		rtk_pair_hoist h;
		rtk_pair_hoist_query(a0, a1, a2, h);
		float best2 = max2, best_u = 0.0f, best_v = 0.0f;
		float best_qa[3] = { a0[0], a0[1], a0[2] }, best_qb[3] = { a0[0], a0[1], a0[2] };
		uint32_t best_prim = RTK_PRIM_NONE;
		// a limit that is NaN, zero or negative and a query that is not live are misses without a walk
		uint32_t top = (max2 > 0.0f && rtk_touch_live(a0, a1, a2) && p.num_nodes != 0u && p.num_tris != 0u) ? 0u : RTK_REF_NONE;
		uint32_t sp = 0;
		if (COUNT) c_queries++;

		while (top != RTK_REF_NONE) {
			if ((int32_t)top < 0) {
				// ---------------------------------------------------------------- leaf: its records up to RTK_TRI_LAST
				uint32_t slot = top & 0x7fffffffu;
				if (COUNT) c_leaves++;
				while (slot < p.num_tris) {
					const pc_f32x4 *t = reinterpret_cast<const pc_f32x4 *>(reinterpret_cast<const char *>(p.tris) + (size_t)slot * RTK_TRI_STRIDE);
					const pc_f32x4 A = t[0], B = t[1], C = t[2];
					const float b0[3] = { A.x, A.y, A.z }, b1[3] = { B.x, B.y, B.z }, b2[3] = { C.x, C.y, C.z };
					const uint32_t prim = __float_as_uint(A.w);
					if (COUNT) c_tris++;
					float blo[3], bhi[3];
					rtk_pair_box(b0, b1, b2, blo, bhi);
					if (rtk_touch_filter_passes(prim, first, p.flags, a0, a1, a2, b0, b1, b2)
						&& !rtk_pair_skip(rtk_pair_box_bound(blo, bhi, h.lo, h.hi), best2, max2)) {
						rtk_pair_result pr;
						rtk_pair_evaluate(h, b0, b1, b2, pr);
						if (rtk_pair_wins(pr.dist2, prim, max2, best2, best_prim)) {
							best2 = pr.dist2; best_prim = prim; best_u = pr.u; best_v = pr.v;
							best_qa[0] = pr.qa[0]; best_qa[1] = pr.qa[1]; best_qa[2] = pr.qa[2];
							best_qb[0] = pr.qb[0]; best_qb[1] = pr.qb[1]; best_qb[2] = pr.qb[2];
						}
					}
					if (__float_as_uint(B.w) & RTK_TRI_LAST) break;
					slot++;
				}
				top = RTK_REF_NONE;
			} else if (top < p.num_nodes) {
				// ---------------------------------------------------------------- node: four bounds, nearest first
				const pc_f32x4 *nd = reinterpret_cast<const pc_f32x4 *>(p.nodes + top);
				const pc_f32x4 xl = nd[0], xh = nd[1], yl = nd[2], yh = nd[3], zl = nd[4], zh = nd[5];
				const pc_u32x4 ch = *reinterpret_cast<const pc_u32x4 *>(nd + 6);
				uint32_t key[4], ref[4];
				if (COUNT) c_nodes++;
#pragma unroll
				for (int k = 0; k < 4; k++) {
					const float lo[3] = { xl[k], yl[k], zl[k] }, hi[3] = { xh[k], yh[k], zh[k] };
					const float bound = rtk_pair_box_bound(lo, hi, h.lo, h.hi);
					const bool enter = ch[k] != RTK_REF_NONE && !rtk_pair_skip(bound, best2, max2);
					// (bounds are >= +0: their bits order like their values; a NaN bound is entered, first)
					key[k] = enter ? (bound == bound ? __float_as_uint(bound) : 0u) : 0xffffffffu;
					ref[k] = enter ? ch[k] : RTK_REF_NONE;
				}
				pc_cswap(key[0], ref[0], key[1], ref[1]);
				pc_cswap(key[2], ref[2], key[3], ref[3]);
				pc_cswap(key[0], ref[0], key[2], ref[2]);
				pc_cswap(key[1], ref[1], key[3], ref[3]);
				pc_cswap(key[1], ref[1], key[2], ref[2]);
				top = ref[0];
				// the others far to near. A push that does not fit LDS or the spill area is dropped WITHOUT advancing sp and flagged
#pragma unroll
				for (int k = 3; k >= 1; k--) {
					if (ref[k] == RTK_REF_NONE) continue;
					const uint2 e = make_uint2(ref[k], key[k]);
					if (sp < PC_LDS_STACK) { stk[sp][lane] = e; sp++; }
					else if (sp - PC_LDS_STACK < p.spill_cap) { p.spill[(size_t)(sp - PC_LDS_STACK) * p.spill_stride + glane] = e; sp++; if (COUNT) c_spills++; }
					else p.counter[RTK_ERROR_WORD] = 1ull;
				}
			} else top = RTK_REF_NONE;                                // (a child word beyond the array: not a tree; nothing is read)
			// ---------------------------------------------------------------- pop: the bound again, best2 has shrunk since the push
			while (top == RTK_REF_NONE && sp != 0u) {
				--sp;
				const uint2 e = sp < PC_LDS_STACK ? stk[sp][lane] : p.spill[(size_t)(sp - PC_LDS_STACK) * p.spill_stride + glane];
				if (!rtk_pair_skip(__uint_as_float(e.y), best2, max2)) top = e.x;
			}
		}

		// a miss leaves dist2 = max_dist2 as given, u = v = 0, RTK_PRIM_NONE and the query's vertex 0 as given, twice
		const bool miss = best_prim == RTK_PRIM_NONE;
		if (COUNT && !miss) c_hits++;
		pc_u32x4 out;
		out.x = miss ? max_bits : __float_as_uint(best2);
		out.y = __float_as_uint(best_u); out.z = __float_as_uint(best_v); out.w = best_prim;
		*reinterpret_cast<pc_u32x4 *>(p.records + r) = out;
		const uint32_t *v0 = reinterpret_cast<const uint32_t *>(p.queries + r);
		if (p.points_query) {
			uint32_t *dst = reinterpret_cast<uint32_t *>(p.points_query + (size_t)r * 3u);
			for (int x = 0; x < 3; x++) dst[x] = miss ? v0[x] : __float_as_uint(best_qa[x]);
		}
		if (p.points_scene) {
			uint32_t *dst = reinterpret_cast<uint32_t *>(p.points_scene + (size_t)r * 3u);
			for (int x = 0; x < 3; x++) dst[x] = miss ? v0[x] : __float_as_uint(best_qb[x]);
		}
	}
	if (COUNT) {
		// (the words k_closest's counting build uses)
		atomicAdd(p.counter + 1, (unsigned long long)c_queries);
		atomicAdd(p.counter + 2, (unsigned long long)c_nodes);
		atomicAdd(p.counter + 3, (unsigned long long)c_leaves);
		atomicAdd(p.counter + 4, (unsigned long long)c_tris);
		atomicAdd(p.counter + 5, (unsigned long long)c_hits);
		atomicAdd(p.counter + 6, (unsigned long long)c_spills);
	}
}

// workgroups of a form a CU holds, asked once per device
int pair_blocks_per_cu(int device, bool counted)
{
	static std::atomic<int> known[RTK_MAX_DEVICES][2];
	if (device < 0 || device >= RTK_MAX_DEVICES) return 2;
	int b = known[device][counted].load(std::memory_order_relaxed);
	if (b == 0) {
		const hipError_t rc = counted ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, k_pair<true>, (int)PC_THREADS, 0)
			: hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, k_pair<false>, (int)PC_THREADS, 0);
		if (rc != hipSuccess || b < 1) b = 2;
		known[device][counted].store(b, std::memory_order_relaxed);
	}
	return b;
}

} // namespace

extern "C" uint32_t rtk_amd_pair_stack_entries(void) { return PC_LDS_STACK; }

int rtk_launch_pair(const rtk_dev_scene *ds_c, const rtk_tri_query *d_tris, size_t num_queries, const rtk_ray_list *list,
	const rtk_touch_filter *filter, const float *d_max_dist2, rtk_closest_record *d_records, float *d_points_query, float *d_points_scene,
	hipStream_t stream, rtk_trace_counters *counted)
{
	rtk_dev_scene *ds = const_cast<rtk_dev_scene *>(ds_c);
	const char *const who = counted ? "rtk_dev_closest_triangles_counted" : "rtk_dev_closest_triangles";
	// everything the host can see is refused here, before any HIP call
	if (!ds) { rtk_set_error("%s: NULL scene", who); return RTK_AMD_ERR_BAD_ARG; }
	if (num_queries && (!d_tris || !d_records)) { rtk_set_error("%s: NULL triangles or records", who); return RTK_AMD_ERR_BAD_ARG; }
	if (list && (list->struct_size < sizeof(rtk_ray_list) || list->flags != 0u || !list->d_count)) {
		rtk_set_error("%s: bad list (struct_size %u, flags %#x, d_count %p)", who, list->struct_size, list->flags, (const void *)list->d_count);
		return RTK_AMD_ERR_BAD_ARG;
	}
	if (filter && (filter->struct_size < sizeof(rtk_touch_filter) || (filter->flags & ~(uint32_t)RTK_TOUCH_SKIP_SHARED_VERTEX) != 0u)) {
		rtk_set_error("%s: bad filter (struct_size %u, flags %#x)", who, filter->struct_size, filter->flags);
		return RTK_AMD_ERR_BAD_ARG;
	}
	if (num_queries >= ((size_t)1 << 32)) { rtk_set_error("%s: %zu queries: a batch holds fewer than 2^32", who, num_queries); return RTK_AMD_ERR_BAD_ARG; }
	if (counted) *counted = rtk_trace_counters();
	if (num_queries == 0) return RTK_AMD_OK;
	if (!rtk_on_scene_device(ds, who)) return RTK_AMD_ERR_BAD_ARG;

	PairParams p = {};
	p.queries = d_tris;
	p.max_dist2 = d_max_dist2;
	p.first_prim = filter ? filter->d_first_prim : nullptr;
	p.flags = filter ? filter->flags : 0u;
	p.ids = list ? reinterpret_cast<const unsigned long long *>(list->d_ids) : nullptr;
	p.count = list ? reinterpret_cast<const unsigned long long *>(list->d_count) : nullptr;
	p.records = d_records;
	p.points_query = d_points_query;
	p.points_scene = d_points_scene;
	p.n = (uint32_t)num_queries;
	const size_t blocks_needed = (num_queries + PC_THREADS - 1u) / PC_THREADS;
	size_t grid = (size_t)(ds->num_cus > 0 ? ds->num_cus : 1) * (size_t)pair_blocks_per_cu(ds->device, counted != nullptr);
	if (grid > blocks_needed) grid = blocks_needed;

	// the scratch set of (scene, stream), held until the launch is enqueued; the view and the tree record are read under the
	// same lock a rebuild replaces them under (rtk_launch_closest does the same)
	std::lock_guard<std::mutex> lock(ds->scratch_mutex);
	p.nodes = ds->view.nodes; p.tris = ds->view.tris; p.num_nodes = ds->view.num_nodes; p.num_tris = ds->view.num_tris;
	const size_t entries = ds->tree.stack_entries();
	const size_t spill_cap = entries > PC_LDS_STACK ? entries - PC_LDS_STACK : 0;
	LaunchScratch *sc = ds->scratch.get(stream);
	if (!sc) return RTK_AMD_ERR_OOM;
	if (spill_cap) {
		const int rc = sc->grow_spill(grid * PC_THREADS, spill_cap, sizeof(uint2));
		if (rc != RTK_AMD_OK) return rc;
	}
	p.spill = sc->spill.as<uint2>();
	p.spill_stride = (uint32_t)(spill_cap ? sc->spill.capacity : 0);
	p.spill_cap = (uint32_t)spill_cap;
	p.counter = sc->d_counter;
	if (!counted) {
		hipLaunchKernelGGL(k_pair<false>, dim3((unsigned)grid), dim3(PC_THREADS), 0, stream, p);
		RTK_HIP_CHECK(hipGetLastError(), RTK_AMD_ERR_HIP);
		return RTK_AMD_OK;
	}
	// the counting form: the visit counters start from zero, are brought home and the stream is waited for
	unsigned long long c[8], err = 0;
	RTK_HIP_CHECK(hipMemsetAsync(sc->d_counter, 0, RTK_COUNTER_WORDS * sizeof(unsigned long long), stream), RTK_AMD_ERR_HIP);
	hipLaunchKernelGGL(k_pair<true>, dim3((unsigned)grid), dim3(PC_THREADS), 0, stream, p);
	RTK_HIP_CHECK(hipGetLastError(), RTK_AMD_ERR_HIP);
	RTK_HIP_CHECK(hipMemcpyAsync(c, sc->d_counter, sizeof(c), hipMemcpyDeviceToHost, stream), RTK_AMD_ERR_HIP);
	RTK_HIP_CHECK(hipMemcpyAsync(&err, sc->d_counter + RTK_ERROR_WORD, sizeof(err), hipMemcpyDeviceToHost, stream), RTK_AMD_ERR_HIP);
	RTK_HIP_CHECK(hipStreamSynchronize(stream), RTK_AMD_ERR_HIP);
	counted->rays = c[1]; counted->nodes = c[2]; counted->leaves = c[3]; counted->triangles = c[4]; counted->hits = c[5]; counted->stack_spills = c[6];
	if (err) {
		(void)hipMemsetAsync(sc->d_counter + RTK_ERROR_WORD, 0, sizeof(err), stream);
		rtk_set_error("%s: traversal stack overflow (corrupted scene)", who);
		return RTK_AMD_ERR_BAD_SCENE;
	}
	return RTK_AMD_OK;
}
