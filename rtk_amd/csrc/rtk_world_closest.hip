// rtk_world_closest.hip -- rtk_dev_world_closest_points: for every query point the nearest triangle over all live instances of a
// world, by the rule of rtk_world_closest_rule.h. The answer has the bits rtk_dev_closest_points gives on the flat
// placed twin (rtk_dev_scene_build_placed of the same meshes under the same placements), for any affine placement; it is a function
// of the instances' records, the placements, the filter and the query alone: neither tree decides more than which records are
// never looked at.
//
// THE WALK, k_world_closest<COUNT, FILT>: k_world's frame (rtk_world.hip) -- one query per lane, a fixed grid of resident
// workgroups striding over the batch, 8-byte stack entries (reference, bound), WD_LDS_STACK per lane in LDS as [entry][lane], deeper
// ones in the spill area of the (top tree, stream) scratch set, a push that fits neither dropped without advancing sp and flagged in
// that set's error word, the WD_REF_TOP sentinel to come back from an instance to the rest of a top leaf -- with the keys of
// rtk_closest.hip: a child's key is the bound of its box (rtk_closest_box_bound), children are walked nearest bound first, a child
// is left out iff its bound > the best dist2 so far, strictly, and the bound is looked at again at the pop.
//   Top level: the exact 128-byte nodes of the top tree as they are: no margin (rtk_world_closest_rule.h point 2). A top leaf is a
// run of proxy records: lo from v0, hi from v1, the instance from prim. A proxy whose bound is not beyond the best, whose
// instance is live and passes the filter ENTERS THE INSTANCE: the sentinel (WD_REF_TOP, the next proxy slot of the leaf or none)
// is pushed, the lane loads the 12 floats of the instance's FORWARD placement and walks the instance's scene from its root on the
// same stack. The query is never transformed.
//   In an instance: every child's box goes through rtk_world_placed_box (six rows) before the bound, every record's vertices
// through rtk_place_vertex before rtk_closest_triangle. A leaf is its run of records up to RTK_TRI_LAST, as in rtk_closest.hip.
//   Scene base pointers differ per lane: nodes and records are addressed by 64-bit per-lane pointers, as in k_world.
//
// FLOATING POINT: only the rule headers' routines decide a bit (__fmul_rn / __fadd_rn through their macros); -ffp-contract=off
// like every traversal.
// Compiler's resource report (gfx950, -O3, kernel-resource-usage): WC_RESOURCES below.
#include "rtk_world_internal.h"
#include "rtk_world_closest_rule.h"

#include <atomic>

// WC_RESOURCES (plain / FILT / counting): VGPRs 116 / 117 / 118, scratch 0 and no VGPR spills in every form (0 / 2 / 4 SGPRs spill
// into VGPR lanes), LDS 32 768 B per workgroup: LDS places five workgroups of four waves on a CU, the registers allow 4 waves per SIMD.

namespace {

struct WorldClosestParams {
	const DevNode *top_nodes;
	const DevTri *top_tris;
	uint32_t top_num_nodes, top_num_tris;
	const DevWorldInstance *inst;
	const DevWorldScene *scenes;
	const rtk_placement *place;            // the forward placements, as last given
	uint32_t num_instances, num_scenes;
	uint32_t n;
	const rtk_point_query *queries;
	const unsigned long long *ids;         // or NULL: 0, 1, 2, ...
	const unsigned long long *count;       // or NULL: n
	rtk_closest_record *records;
	uint32_t *instances;                   // or NULL
	float *points;                         // or NULL
	const uint32_t *mask;                  // or NULL: bit i set = instance i is walked
	uint32_t mask_bits;
	const uint32_t *ignore_instance;       // or NULL: per query slot
	unsigned long long *counter;           // the stream's counter words: [RTK_ERROR_WORD] is set by a dropped push
	uint2 *spill;                          // [entry][lane of the launch]
	uint32_t spill_stride;
	uint32_t spill_cap;                    // entries per lane
};

typedef float wc_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t wc_u32x4 __attribute__((ext_vector_type(4)));

// ascending by key; the reference travels with it
__device__ __forceinline__ void wc_cswap(uint32_t &ka, uint32_t &ra, uint32_t &kb, uint32_t &rb)
{
	const bool swap = kb < ka;
	const uint32_t k0 = swap ? kb : ka, k1 = swap ? ka : kb, r0 = swap ? rb : ra, r1 = swap ? ra : rb;
	ka = k0; kb = k1; ra = r0; rb = r1;
}

// COUNT: the visit counts of rtk_dev_world_closest_points_counted. FILT: the instance mask and the per-query ignored instance
template <bool COUNT, bool FILT>
__global__ void __launch_bounds__(WD_THREADS) k_world_closest(WorldClosestParams p)
{
	__shared__ uint2 s_stack[WD_WAVES][WD_LDS_STACK][64];

	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint2 (*stk)[64] = s_stack[wave];
	const uint32_t glane = blockIdx.x * WD_THREADS + threadIdx.x;
	uint32_t m = p.n;
	if (p.count) { const unsigned long long listed = *p.count; m = listed < p.n ? (uint32_t)listed : p.n; }
	const unsigned long long step = (unsigned long long)gridDim.x * WD_THREADS;
	uint32_t c_queries = 0, c_nodes = 0, c_leaves = 0, c_tris = 0, c_hits = 0, c_spills = 0;

	for (unsigned long long qi = glane; qi < m; qi += step) {
		const uint32_t r = p.ids ? (uint32_t)p.ids[qi] : (uint32_t)qi;
		if (r >= p.n) continue;                                   // (the caller's error; nothing is read or written out of range)
		const wc_u32x4 qw = __builtin_nontemporal_load(reinterpret_cast<const wc_u32x4 *>(p.queries + r));
		const float P[3] = { __uint_as_float(qw.x), __uint_as_float(qw.y), __uint_as_float(qw.z) };
		const float max2 = __uint_as_float(qw.w);
		const uint32_t skip_inst = (FILT && p.ignore_instance) ? p.ignore_instance[r] : RTK_PRIM_NONE;
		float best2 = max2, best_u = 0.0f, best_v = 0.0f;
		float best_q[3] = { P[0], P[1], P[2] };
		uint32_t best_prim = RTK_PRIM_NONE, best_inst = RTK_PRIM_NONE;
		// where the walk is: the top tree (in_inst false), or the scene of instance cur_inst under placement pm
		bool in_inst = false;
		uint32_t cur_inst = RTK_PRIM_NONE;
		float pm[12];
#pragma unroll
		for (int k = 0; k < 12; k++) pm[k] = 0.0f;
		const char *nodes = reinterpret_cast<const char *>(p.top_nodes), *tris = reinterpret_cast<const char *>(p.top_tris);
		uint32_t num_nodes = p.top_num_nodes, num_tris = p.top_num_tris;
		// a limit that is NaN, zero or negative and a point with a non-finite coordinate are misses without a walk
		const bool finite = (qw.x & 0x7f800000u) != 0x7f800000u && (qw.y & 0x7f800000u) != 0x7f800000u && (qw.z & 0x7f800000u) != 0x7f800000u;
		uint32_t top = (max2 > 0.0f && finite && p.top_num_nodes != 0u && p.top_num_tris != 0u) ? 0u : RTK_REF_NONE;
		uint32_t sp = 0;
		if (COUNT) c_queries++;

		while (top != RTK_REF_NONE) {
			if ((int32_t)top >= 0) {
				// ------------------------------------------------------------ node, of the top tree or of a scene: four bounds, nearest first
				if (top < num_nodes) {
					const wc_f32x4 *nd = reinterpret_cast<const wc_f32x4 *>(nodes + (size_t)top * 128u);
					const wc_f32x4 xl = nd[0], xh = nd[1], yl = nd[2], yh = nd[3], zl = nd[4], zh = nd[5];
					const wc_u32x4 ch = *reinterpret_cast<const wc_u32x4 *>(nd + 6);
					uint32_t key[4], ref[4];
					if (COUNT) c_nodes++;
#pragma unroll
					for (int k = 0; k < 4; k++) {
						const float lo[3] = { xl[k], yl[k], zl[k] }, hi[3] = { xh[k], yh[k], zh[k] };
						float bound;
						if (in_inst) {
							// a scene's box is local: its exact world bounds under the instance's placement
							float wlo[3], whi[3];
							rtk_world_placed_box(pm, lo, hi, wlo, whi);
							bound = rtk_closest_box_bound(P, wlo, whi);
						} else bound = rtk_closest_box_bound(P, lo, hi);  // the top tree's boxes as they are: no margin
						const bool enter = ch[k] != RTK_REF_NONE && !rtk_closest_skip(bound, best2);
						// (bounds are >= +0: their bits order like their values; a NaN bound is entered, first)
						key[k] = enter ? (bound == bound ? __float_as_uint(bound) : 0u) : 0xffffffffu;
						ref[k] = enter ? ch[k] : RTK_REF_NONE;
					}
					wc_cswap(key[0], ref[0], key[1], ref[1]);
					wc_cswap(key[2], ref[2], key[3], ref[3]);
					wc_cswap(key[0], ref[0], key[2], ref[2]);
					wc_cswap(key[1], ref[1], key[3], ref[3]);
					wc_cswap(key[1], ref[1], key[2], ref[2]);
					top = ref[0];
					// the others far to near
#pragma unroll
					for (int k = 3; k >= 1; k--) {
						if (ref[k] == RTK_REF_NONE) continue;
						const uint2 en = make_uint2(ref[k], key[k]);
						WD_PUSH(en);
					}
				} else top = RTK_REF_NONE;                            // (a child word beyond the array: not a tree; nothing is read)
			} else if (!in_inst) {
				// ------------------------------------------------------------ a leaf of the top tree: proxies up to RTK_TRI_LAST
				uint32_t slot = top & 0x7fffffffu;
				if (COUNT) c_leaves++;
				top = RTK_REF_NONE;
				while (slot < num_tris) {
					const wc_f32x4 *t = reinterpret_cast<const wc_f32x4 *>(tris + (size_t)slot * RTK_TRI_STRIDE);
					const wc_f32x4 A = t[0], B = t[1];
					const uint32_t inst = __float_as_uint(A.w), flags = __float_as_uint(B.w);
					const bool last = (flags & RTK_TRI_LAST) != 0u;
					if (COUNT) c_tris++;
					bool wanted = inst < p.num_instances;
					if (FILT) {
						wanted = wanted && inst != skip_inst;
						if (p.mask) wanted = wanted && inst < p.mask_bits && ((p.mask[inst >> 5] >> (inst & 31u)) & 1u);
					}
					if (wanted) {
						// lo is v0, hi is v1: the padded world box of the instance, as it is
						const float lo[3] = { A.x, A.y, A.z }, hi[3] = { B.x, B.y, B.z };
						wanted = !rtk_closest_skip(rtk_closest_box_bound(P, lo, hi), best2);
					}
					if (wanted) {
						const wc_u32x4 i3 = reinterpret_cast<const wc_u32x4 *>(p.inst + inst)[3];
						wanted = (i3.y & WD_DEAD) == 0u && i3.x < p.num_scenes;
						if (wanted) {
							const DevWorldScene sc = p.scenes[i3.x];
							wanted = sc.num_nodes != 0u && sc.num_tris != 0u;
							if (wanted) {
								// ENTER: the sentinel remembers where the leaf goes on; the instance's placement; its scene from the root
								const uint2 en = make_uint2(WD_REF_TOP, last ? RTK_REF_NONE : slot + 1u);
								const uint32_t sp_before = sp;
								WD_PUSH(en);
								if (sp != sp_before) {                        // (a dropped sentinel: the instance is not entered, the error word says so)
									const wc_f32x4 *pr = reinterpret_cast<const wc_f32x4 *>(p.place + inst);
									const wc_f32x4 m0 = pr[0], m1 = pr[1], m2 = pr[2];
									pm[0] = m0.x; pm[1] = m0.y; pm[2] = m0.z; pm[3] = m0.w;
									pm[4] = m1.x; pm[5] = m1.y; pm[6] = m1.z; pm[7] = m1.w;
									pm[8] = m2.x; pm[9] = m2.y; pm[10] = m2.z; pm[11] = m2.w;
									in_inst = true; cur_inst = inst;
									nodes = reinterpret_cast<const char *>(sc.nodes); tris = reinterpret_cast<const char *>(sc.tris);
									num_nodes = sc.num_nodes; num_tris = sc.num_tris;
									top = 0u;
									break;
								}
							}
						}
					}
					if (last) break;
					slot++;
				}
			} else {
				// ------------------------------------------------------------ a leaf of a scene: its records up to RTK_TRI_LAST, placed
				uint32_t slot = top & 0x7fffffffu;
				if (COUNT) c_leaves++;
				while (slot < num_tris) {
					const wc_f32x4 *t = reinterpret_cast<const wc_f32x4 *>(tris + (size_t)slot * RTK_TRI_STRIDE);
					const wc_f32x4 A = t[0], B = t[1], C = t[2];
					const float a[3] = { A.x, A.y, A.z }, b[3] = { B.x, B.y, B.z }, c[3] = { C.x, C.y, C.z };
					float q[3], u, v;
					const float dist2 = rtk_world_closest_triangle(P, pm, a, b, c, q, u, v);
					const uint32_t prim = __float_as_uint(A.w);
					if (COUNT) c_tris++;
					if (dist2 < max2 && rtk_world_closest_better(dist2, cur_inst, prim, best2, best_inst, best_prim)) {
						best2 = dist2; best_inst = cur_inst; best_prim = prim; best_u = u; best_v = v;
						best_q[0] = q[0]; best_q[1] = q[1]; best_q[2] = q[2];
					}
					if (__float_as_uint(B.w) & RTK_TRI_LAST) break;
					slot++;
				}
				top = RTK_REF_NONE;
			}
			// ---------------------------------------------------------------- pop: the bound again, best2 has shrunk since the push
			while (top == RTK_REF_NONE && sp != 0u) {
				--sp;
				const uint2 en = sp < WD_LDS_STACK ? stk[sp][lane] : p.spill[(size_t)(sp - WD_LDS_STACK) * p.spill_stride + glane];
				if (en.x == WD_REF_TOP) {
					// back in the top tree, at the rest of the leaf the instance was entered from
					in_inst = false; cur_inst = RTK_PRIM_NONE;
					nodes = reinterpret_cast<const char *>(p.top_nodes); tris = reinterpret_cast<const char *>(p.top_tris);
					num_nodes = p.top_num_nodes; num_tris = p.top_num_tris;
					if (en.y != RTK_REF_NONE) top = RTK_REF_LEAF | en.y;
				} else if (!rtk_closest_skip(__uint_as_float(en.y), best2)) top = en.x;
			}
		}

		// a miss leaves max_dist2 as given, u = v = 0, RTK_PRIM_NONE for the primitive and the instance, and the query point itself
		const bool hit = best_prim != RTK_PRIM_NONE;
		if (COUNT && hit) c_hits++;
		wc_u32x4 out;
		out.x = hit ? __float_as_uint(best2) : qw.w;
		out.y = __float_as_uint(best_u); out.z = __float_as_uint(best_v); out.w = best_prim;
		*reinterpret_cast<wc_u32x4 *>(p.records + r) = out;
		if (p.instances) p.instances[r] = best_inst;
		if (p.points) {
			uint32_t *dst = reinterpret_cast<uint32_t *>(p.points + (size_t)r * 3u);
			dst[0] = hit ? __float_as_uint(best_q[0]) : qw.x;
			dst[1] = hit ? __float_as_uint(best_q[1]) : qw.y;
			dst[2] = hit ? __float_as_uint(best_q[2]) : qw.z;
		}
	}
	if (COUNT) {
		// (the words rtk_trace_kernel's counting build uses)
		atomicAdd(p.counter + 1, (unsigned long long)c_queries);
		atomicAdd(p.counter + 2, (unsigned long long)c_nodes);
		atomicAdd(p.counter + 3, (unsigned long long)c_leaves);
		atomicAdd(p.counter + 4, (unsigned long long)c_tris);
		atomicAdd(p.counter + 5, (unsigned long long)c_hits);
		atomicAdd(p.counter + 6, (unsigned long long)c_spills);
	}
}

// workgroups of k_world_closest a CU holds, asked once per device
int world_closest_blocks_per_cu(int device)
{
	static std::atomic<int> known[RTK_MAX_DEVICES];
	if (device < 0 || device >= RTK_MAX_DEVICES) return 2;
	int b = known[device].load(std::memory_order_relaxed);
	if (b == 0) {
		if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, k_world_closest<false, true>, (int)WD_THREADS, 0) != hipSuccess || b < 1) b = 2;
		known[device].store(b, std::memory_order_relaxed);
	}
	return b;
}

} // namespace

extern "C" uint32_t rtk_amd_world_closest_stack_entries(void) { return WD_LDS_STACK; }

int rtk_launch_world_closest(const rtk_dev_world *w_c, const rtk_point_query *d_queries, size_t n, const rtk_ray_list *list,
	const rtk_world_filter *filter, rtk_closest_record *d_records, uint32_t *d_instances, float *d_points, hipStream_t stream,
	rtk_trace_counters *counted)
{
	rtk_dev_world *w = const_cast<rtk_dev_world *>(w_c);
	const char *who = counted ? "rtk_dev_world_closest_points_counted" : "rtk_dev_world_closest_points";
	// everything the host can see is refused here, before any HIP call
	const int refused = rtk_world_refuse(who, "queries", w, n, d_queries && d_records, list, filter);
	if (refused != RTK_AMD_OK) return refused;
	if (counted) *counted = rtk_trace_counters();
	if (n == 0) return RTK_AMD_OK;
	if (!rtk_on_scene_device(w->top, who)) return RTK_AMD_ERR_BAD_ARG;

	WorldClosestParams p = {};
	p.queries = d_queries;
	p.n = (uint32_t)n;
	p.ids = list ? reinterpret_cast<const unsigned long long *>(list->d_ids) : nullptr;
	p.count = list ? reinterpret_cast<const unsigned long long *>(list->d_count) : nullptr;
	p.records = d_records;
	p.instances = d_instances;
	p.points = d_points;
	p.place = w->d_place;
	const bool filtered = filter && (filter->d_instance_mask || filter->d_ignore_instance);
	if (filtered) { p.mask = filter->d_instance_mask; p.mask_bits = filter->instance_mask_bits; p.ignore_instance = filter->d_ignore_instance; }
	return rtk_world_launch(w, n, stream, world_closest_blocks_per_cu(w->device), filtered ? k_world_closest<false, true> : k_world_closest<false, false>,
		k_world_closest<true, true>, p, [](const rtk_dev_scene *, WorldClosestParams &) {}, counted, who);
}
