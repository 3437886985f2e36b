// rtk_closest.hip -- rtk_dev_closest_points: for every query point the nearest triangle of a device scene, its squared distance,
// barycentrics and the point on it, by the rule of rtk_closest_rule.h. The result is a function of the scene's triangle records
// and the query alone (DESIGN.md "Closest points"): the tree only decides which records are never looked at.
//
// One query per lane of a 64-wide wave; a fixed grid of resident workgroups whose waves take 64-query chunks in turn (so that the
// spill area is sized by the grid, not by the batch). The walk is nearest first over the exact 128-byte nodes: the bound of all
// four child boxes (rtk_closest_box_bound), empty slots and children whose bound exceeds the best distance so far left out, the
// nearest child entered, the others pushed far to near with their bounds, and the bound looked at again at the pop, because the
// best distance has shrunk since the push. A leaf is its run of DevTri records up to RTK_TRI_LAST.
// The stack is rtk_trace.hip's: CL_LDS_STACK entries per lane in LDS, [entry][lane], so that a wave's push or pop is one
// conflict-free 8-byte access per lane; deeper entries in the spill area of the (scene, stream) scratch set; a push that fits
// neither (impossible for a tree) is dropped and flagged in the stream's launch-error word.
// Exact nodes, not the 64-byte compressed ones: the exact boxes of a device build are the tightest bounds there are, and the
// skip is only as good as the bound.
#include "rtk_dev.h"
#include "rtk_closest_rule.h"

#include <atomic>
#include <mutex>

#define CL_THREADS 256u
#define CL_WAVES (CL_THREADS / 64u)
#define CL_LDS_STACK 16u           // entries per lane held in LDS: 32 KB per workgroup, five workgroups share a CU's 160 KB

namespace {

struct ClosestParams {
	const DevNode *nodes;
	const DevTri *tris;
	uint32_t num_nodes;
	uint32_t num_tris;
	const rtk_point_query *queries;
	const unsigned long long *ids;     // or NULL: 0, 1, 2, ...
	const unsigned long long *count;   // or NULL: n
	rtk_closest_record *records;
	float *points;                     // or NULL
	unsigned long long *counter;       // the stream's counter words: [RTK_ERROR_WORD] is set by a dropped push
	uint2 *spill;                      // [entry][lane of the launch]
	uint32_t spill_stride;
	uint32_t spill_cap;                // entries per lane
	uint32_t n;
};

typedef float cl_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t cl_u32x4 __attribute__((ext_vector_type(4)));

// ascending by key; the reference travels with it
__device__ __forceinline__ void cl_cswap(uint32_t &ka, uint32_t &ra, uint32_t &kb, uint32_t &rb)
{
	const bool swap = kb < ka;
	const uint32_t k0 = swap ? kb : ka, k1 = swap ? ka : kb, r0 = swap ? rb : ra, r1 = swap ? ra : rb;
	ka = k0; kb = k1; ra = r0; rb = r1;
}

// COUNT: the visit counts of rtk_dev_closest_points_counted, summed per lane and added to the stream's counter words at the end
template <bool COUNT>
__global__ void __launch_bounds__(CL_THREADS) k_closest(ClosestParams p)
{
	__shared__ uint2 s_stack[CL_WAVES][CL_LDS_STACK][64];

	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint2 (*stk)[64] = s_stack[wave];
	const uint32_t glane = blockIdx.x * CL_THREADS + threadIdx.x;
	uint32_t m = p.n;
	if (p.count) { const unsigned long long listed = *p.count; m = listed < p.n ? (uint32_t)listed : p.n; }
	const unsigned long long step = (unsigned long long)gridDim.x * CL_THREADS;
	uint32_t c_queries = 0, c_nodes = 0, c_leaves = 0, c_tris = 0, c_hits = 0, c_spills = 0;

	for (unsigned long long i = glane; i < m; i += step) {
		const uint32_t r = p.ids ? (uint32_t)p.ids[i] : (uint32_t)i;
		if (r >= p.n) continue;                                   // (the caller's error; nothing is read or written out of range)
		const cl_u32x4 qw = __builtin_nontemporal_load(reinterpret_cast<const cl_u32x4 *>(p.queries + r));
		const float P[3] = { __uint_as_float(qw.x), __uint_as_float(qw.y), __uint_as_float(qw.z) };
		const float max2 = __uint_as_float(qw.w);
		float best2 = max2, best_u = 0.0f, best_v = 0.0f;
		float best_q[3] = { P[0], P[1], P[2] };
		uint32_t best_prim = RTK_PRIM_NONE;
		// a limit that is NaN, zero or negative and a point with a non-finite coordinate are misses without a walk
		const bool finite = (qw.x & 0x7f800000u) != 0x7f800000u && (qw.y & 0x7f800000u) != 0x7f800000u && (qw.z & 0x7f800000u) != 0x7f800000u;
		uint32_t top = (max2 > 0.0f && finite && p.num_nodes != 0u && p.num_tris != 0u) ? 0u : RTK_REF_NONE;
		uint32_t sp = 0;
		if (COUNT) c_queries++;

		while (top != RTK_REF_NONE) {
			if ((int32_t)top < 0) {
				// ---------------------------------------------------------------- leaf: its records up to RTK_TRI_LAST
				uint32_t slot = top & 0x7fffffffu;
				if (COUNT) c_leaves++;
				while (slot < p.num_tris) {
					const cl_f32x4 *t = reinterpret_cast<const cl_f32x4 *>(reinterpret_cast<const char *>(p.tris) + (size_t)slot * RTK_TRI_STRIDE);
					const cl_f32x4 A = t[0], B = t[1], C = t[2];
					const float a[3] = { A.x, A.y, A.z }, b[3] = { B.x, B.y, B.z }, c[3] = { C.x, C.y, C.z };
					float q[3], u, v;
					int region;
					const float dist2 = rtk_closest_triangle(P, a, b, c, q, u, v, region);
					const uint32_t prim = __float_as_uint(A.w);
					if (COUNT) c_tris++;
					if (dist2 < max2 && rtk_closest_better(dist2, prim, best2, best_prim)) {
						best2 = dist2; best_prim = prim; best_u = u; best_v = v;
						best_q[0] = q[0]; best_q[1] = q[1]; best_q[2] = q[2];
					}
					if (__float_as_uint(B.w) & RTK_TRI_LAST) break;
					slot++;
				}
				top = RTK_REF_NONE;
			} else if (top < p.num_nodes) {
				// ---------------------------------------------------------------- node: four bounds, nearest first
				const cl_f32x4 *nd = reinterpret_cast<const cl_f32x4 *>(p.nodes + top);
				const cl_f32x4 xl = nd[0], xh = nd[1], yl = nd[2], yh = nd[3], zl = nd[4], zh = nd[5];
				const cl_u32x4 ch = *reinterpret_cast<const cl_u32x4 *>(nd + 6);
				uint32_t key[4], ref[4];
				if (COUNT) c_nodes++;
#pragma unroll
				for (int k = 0; k < 4; k++) {
					const float lo[3] = { xl[k], yl[k], zl[k] }, hi[3] = { xh[k], yh[k], zh[k] };
					const float bound = rtk_closest_box_bound(P, lo, hi);
					const bool enter = ch[k] != RTK_REF_NONE && !rtk_closest_skip(bound, best2);
					// (bounds are >= +0: their bits order like their values; a NaN bound is entered, first)
					key[k] = enter ? (bound == bound ? __float_as_uint(bound) : 0u) : 0xffffffffu;
					ref[k] = enter ? ch[k] : RTK_REF_NONE;
				}
				cl_cswap(key[0], ref[0], key[1], ref[1]);
				cl_cswap(key[2], ref[2], key[3], ref[3]);
				cl_cswap(key[0], ref[0], key[2], ref[2]);
				cl_cswap(key[1], ref[1], key[3], ref[3]);
				cl_cswap(key[1], ref[1], key[2], ref[2]);
				top = ref[0];
				// the others far to near. A push that does not fit LDS or the spill area is dropped WITHOUT advancing sp and flagged
#pragma unroll
				for (int k = 3; k >= 1; k--) {
					if (ref[k] == RTK_REF_NONE) continue;
					const uint2 e = make_uint2(ref[k], key[k]);
					if (sp < CL_LDS_STACK) { stk[sp][lane] = e; sp++; }
					else if (sp - CL_LDS_STACK < p.spill_cap) { p.spill[(size_t)(sp - CL_LDS_STACK) * p.spill_stride + glane] = e; sp++; if (COUNT) c_spills++; }
					else p.counter[RTK_ERROR_WORD] = 1ull;
				}
			} else top = RTK_REF_NONE;                                // (a child word beyond the array: not a tree; nothing is read)
			// ---------------------------------------------------------------- pop: the bound again, best2 has shrunk since the push
			while (top == RTK_REF_NONE && sp != 0u) {
				--sp;
				const uint2 e = sp < CL_LDS_STACK ? stk[sp][lane] : p.spill[(size_t)(sp - CL_LDS_STACK) * p.spill_stride + glane];
				if (!rtk_closest_skip(__uint_as_float(e.y), best2)) top = e.x;
			}
		}

		// a miss leaves best2 = max_dist2 as given, u = v = 0, RTK_PRIM_NONE and the query point itself
		if (COUNT && best_prim != RTK_PRIM_NONE) c_hits++;
		cl_u32x4 out;
		out.x = best_prim == RTK_PRIM_NONE ? qw.w : __float_as_uint(best2);
		out.y = __float_as_uint(best_u); out.z = __float_as_uint(best_v); out.w = best_prim;
		*reinterpret_cast<cl_u32x4 *>(p.records + r) = out;
		if (p.points) {
			float *dst = p.points + (size_t)r * 3u;
			if (best_prim == RTK_PRIM_NONE) {
				reinterpret_cast<uint32_t *>(dst)[0] = qw.x; reinterpret_cast<uint32_t *>(dst)[1] = qw.y; reinterpret_cast<uint32_t *>(dst)[2] = qw.z;
			} else { dst[0] = best_q[0]; dst[1] = best_q[1]; dst[2] = best_q[2]; }
		}
	}
	if (COUNT) {
		// (the words rtk_trace_kernel's counting build uses: rtk_launch.hip reads them the same way)
		atomicAdd(p.counter + 1, (unsigned long long)c_queries);
		atomicAdd(p.counter + 2, (unsigned long long)c_nodes);
		atomicAdd(p.counter + 3, (unsigned long long)c_leaves);
		atomicAdd(p.counter + 4, (unsigned long long)c_tris);
		atomicAdd(p.counter + 5, (unsigned long long)c_hits);
		atomicAdd(p.counter + 6, (unsigned long long)c_spills);
	}
}

// workgroups of k_closest a CU holds (LDS allows five), asked once per device
int closest_blocks_per_cu(int device)
{
	static std::atomic<int> known[RTK_MAX_DEVICES];
	if (device < 0 || device >= RTK_MAX_DEVICES) return 4;
	int b = known[device].load(std::memory_order_relaxed);
	if (b == 0) {
		if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, k_closest<false>, (int)CL_THREADS, 0) != hipSuccess || b < 1) b = 4;
		known[device].store(b, std::memory_order_relaxed);
	}
	return b;
}

} // namespace

extern "C" uint32_t rtk_amd_closest_stack_entries(void) { return CL_LDS_STACK; }

int rtk_launch_closest(const rtk_dev_scene *ds_c, const rtk_point_query *d_queries, size_t num_queries, const rtk_ray_list *list,
	rtk_closest_record *d_records, float *d_points, hipStream_t stream, rtk_trace_counters *counted)
{
	rtk_dev_scene *ds = const_cast<rtk_dev_scene *>(ds_c);
	// everything the host can see is refused here, before any HIP call
	if (!ds || (num_queries && (!d_queries || !d_records))) { rtk_set_error("rtk_dev_closest_points: NULL scene, queries or records"); return RTK_AMD_ERR_BAD_ARG; }
	if (list && (list->struct_size < sizeof(rtk_ray_list) || list->flags != 0u || !list->d_count)) {
		rtk_set_error("rtk_dev_closest_points: bad list (struct_size %u, flags %#x, d_count %p)", list->struct_size, list->flags, (const void *)list->d_count);
		return RTK_AMD_ERR_BAD_ARG;
	}
	if (num_queries >= ((size_t)1 << 32)) { rtk_set_error("rtk_dev_closest_points: %zu queries: a batch holds fewer than 2^32", num_queries); return RTK_AMD_ERR_BAD_ARG; }
	if (counted) *counted = rtk_trace_counters();
	if (num_queries == 0) return RTK_AMD_OK;
	if (!rtk_on_scene_device(ds, "rtk_dev_closest_points")) return RTK_AMD_ERR_BAD_ARG;

	ClosestParams p = {};
	p.queries = d_queries;
	p.ids = list ? reinterpret_cast<const unsigned long long *>(list->d_ids) : nullptr;
	p.count = list ? reinterpret_cast<const unsigned long long *>(list->d_count) : nullptr;
	p.records = d_records;
	p.points = d_points;
	p.n = (uint32_t)num_queries;
	const size_t blocks_needed = (num_queries + CL_THREADS - 1u) / CL_THREADS;
	size_t grid = (size_t)(ds->num_cus > 0 ? ds->num_cus : 1) * (size_t)closest_blocks_per_cu(ds->device);
	if (grid > blocks_needed) grid = blocks_needed;

	// the scratch set of (scene, stream), held until the launch is enqueued (rtk_launch_trace does the same); the view and the
	// tree record are read under the same lock a rebuild replaces them under
	std::lock_guard<std::mutex> lock(ds->scratch_mutex);
	p.nodes = ds->view.nodes; p.tris = ds->view.tris; p.num_nodes = ds->view.num_nodes; p.num_tris = ds->view.num_tris;
	const size_t entries = ds->tree.stack_entries();
	const size_t spill_cap = entries > CL_LDS_STACK ? entries - CL_LDS_STACK : 0;
	LaunchScratch *sc = ds->scratch.get(stream);
	if (!sc) return RTK_AMD_ERR_OOM;
	if (spill_cap) {
		const int rc = sc->grow_spill(grid * CL_THREADS, spill_cap, sizeof(uint2));
		if (rc != RTK_AMD_OK) return rc;
	}
	p.spill = sc->spill.as<uint2>();
	p.spill_stride = (uint32_t)(spill_cap ? sc->spill.capacity : 0);
	p.spill_cap = (uint32_t)spill_cap;
	p.counter = sc->d_counter;
	if (!counted) {
		hipLaunchKernelGGL(k_closest<false>, dim3((unsigned)grid), dim3(CL_THREADS), 0, stream, p);
		RTK_HIP_CHECK(hipGetLastError(), RTK_AMD_ERR_HIP);
		return RTK_AMD_OK;
	}
	// the counting form: the visit counters start from zero, are brought home and the stream is waited for
	unsigned long long c[8], err = 0;
	RTK_HIP_CHECK(hipMemsetAsync(sc->d_counter, 0, RTK_COUNTER_WORDS * sizeof(unsigned long long), stream), RTK_AMD_ERR_HIP);
	hipLaunchKernelGGL(k_closest<true>, dim3((unsigned)grid), dim3(CL_THREADS), 0, stream, p);
	RTK_HIP_CHECK(hipGetLastError(), RTK_AMD_ERR_HIP);
	RTK_HIP_CHECK(hipMemcpyAsync(c, sc->d_counter, sizeof(c), hipMemcpyDeviceToHost, stream), RTK_AMD_ERR_HIP);
	RTK_HIP_CHECK(hipMemcpyAsync(&err, sc->d_counter + RTK_ERROR_WORD, sizeof(err), hipMemcpyDeviceToHost, stream), RTK_AMD_ERR_HIP);
	RTK_HIP_CHECK(hipStreamSynchronize(stream), RTK_AMD_ERR_HIP);
	counted->rays = c[1]; counted->nodes = c[2]; counted->leaves = c[3]; counted->triangles = c[4]; counted->hits = c[5]; counted->stack_spills = c[6];
	if (err) {
		(void)hipMemsetAsync(sc->d_counter + RTK_ERROR_WORD, 0, sizeof(err), stream);
		rtk_set_error("rtk_dev_closest_points_counted: traversal stack overflow (corrupted scene)");
		return RTK_AMD_ERR_BAD_SCENE;
	}
	return RTK_AMD_OK;
}
