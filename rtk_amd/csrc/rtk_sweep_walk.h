// rtk_sweep_walk.h -- the walk and the launch of the four swept shapes (rtk_sweep.hip, rtk_boxsweep.hip, rtk_capsule.hip,
// rtk_obbsweep.hip), once. A shape's file holds what is the shape's alone, as a struct of static functions (below); the result
// is a function of the scene's triangle records, the filter and the query alone, by the shape's rule header: the tree only
// decides which records are never looked at.
//
// THE WALK is rtk_closest.hip's: one query per lane of a 64-wide wave; a fixed grid of resident workgroups whose waves take
// 64-query chunks in turn (so that the spill area is sized by the grid, not by the batch); the exact 128-byte nodes only. The
// four child boxes of a node are tested by the shape's slab routine (the box grown by the shape's reach against the path of
// the centre), empty slots, empty intervals and children entered later than the best time so far left out, the child entered
// first walked next, the others pushed far to near with their entry times, and the entry time looked at again at the pop,
// because the best time has shrunk since the push. A leaf is its run of DevTri records up to RTK_TRI_LAST; a record the filter
// rejects is not evaluated. THE ANY-HIT FORM retires a query at its first candidate and skips by empty intervals alone.
// THE STACK is rtk_closest.hip's: SWEEP_LDS_STACK entries per lane in LDS, [entry][lane], one conflict-free 8-byte access per
// lane and push or pop; deeper entries in THE SPILL area of the (scene, stream) scratch set; a push that fits neither
// (impossible for a tree) is dropped and flagged in the stream's launch-error word.
//
// A SHAPE supplies
//     Sweep, Query, FLOATS     the query record as the caller holds it, as the rule prepares it, and the record's width in floats
//     NAME, NAME_ANY, NAME_COUNTED   the three entry points, for the error texts
//     prepare(w, Q)            the rule's prepare: false = the query touches nothing
//     tmax(Q)                  the time the walk starts from
//     slab(Q, lo, hi, te)      the path against a node's child box: the entry time
//     touches(Q, a, b, c, time)   the shape against one triangle
//     record(Q, w, hit, best_t, best_prim, a, b, c, out, side0, side1)   the hit record and the two 3-float side arrays of the
//                              answer (a, b, c: its triangle), or of a miss (a, b, c: NULL)
#ifndef RTK_SWEEP_WALK_H
#define RTK_SWEEP_WALK_H

#include "rtk_dev.h"
#include "rtk_trace_shared.h"      // RTK_TRI_MESH_SHIFT
#include "rtk_sweep_rule.h"        // rtk_sweep_better, rtk_sweep_skip

#include <atomic>
#include <mutex>

#define SWEEP_THREADS 256u
#define SWEEP_WAVES (SWEEP_THREADS / 64u)
#define SWEEP_LDS_STACK 16u        // entries per lane held in LDS: 32 KB per workgroup

namespace {

template <class Shape>
struct SweepWalkParams {
	const DevNode *nodes;
	const DevTri *tris;
	uint32_t num_nodes;
	uint32_t num_tris;
	const typename Shape::Sweep *sweeps;
	const unsigned long long *ids;     // or NULL: 0, 1, 2, ...
	const unsigned long long *count;   // or NULL: n
	rtk_hit_record *records;           // the closest form
	float *side0;                      // or NULL: points, centres, points, centres (sphere, box, capsule, oriented box)
	float *side1;                      // or NULL: centres, normals, axis points, normals
	uint8_t *blocked;                  // the any-hit form
	const uint32_t *mesh_mask;         // or NULL: bit m set = triangles of mesh m are candidates
	uint32_t mesh_mask_bits;
	const uint32_t *ignore_prim;       // or NULL: per query slot
	unsigned long long *counter;       // the stream's counter words: [RTK_ERROR_WORD] is set by a dropped push
	uint2 *spill;                      // [entry][lane of the launch]
	uint32_t spill_stride;
	uint32_t spill_cap;                // entries per lane
	uint32_t n;
};

typedef float sweep_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t sweep_u32x4 __attribute__((ext_vector_type(4)));

// ascending by key; the reference travels with it
__device__ __forceinline__ void sweep_cswap(float &ka, uint32_t &ra, float &kb, uint32_t &rb)
{
	const bool swap = kb < ka;
	const float k0 = swap ? kb : ka, k1 = swap ? ka : kb;
	const uint32_t r0 = swap ? rb : ra, r1 = swap ? ra : rb;
	ka = k0; kb = k1; ra = r0; rb = r1;
}

// ANY: one byte per query, the walk ends at the first candidate. COUNT: the visit counts of the shape's _counted entry point,
// summed per lane and added to the stream's counter words at the end
template <class Shape, bool ANY, bool COUNT>
__global__ void __launch_bounds__(SWEEP_THREADS) k_sweep_walk(SweepWalkParams<Shape> p)
{
	__shared__ uint2 s_stack[SWEEP_WAVES][SWEEP_LDS_STACK][64];

	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint2 (*stk)[64] = s_stack[wave];
	const uint32_t glane = blockIdx.x * SWEEP_THREADS + threadIdx.x;
	uint32_t m = p.n;
	if (p.count) { const unsigned long long listed = *p.count; m = listed < p.n ? (uint32_t)listed : p.n; }
	const unsigned long long step = (unsigned long long)gridDim.x * SWEEP_THREADS;
	uint32_t c_queries = 0, c_nodes = 0, c_leaves = 0, c_tris = 0, c_hits = 0, c_spills = 0;

	for (unsigned long long i = glane; i < m; i += step) {
		const uint32_t r = p.ids ? (uint32_t)p.ids[i] : (uint32_t)i;
		if (r >= p.n) continue;                                   // (the caller's error; nothing is read or written out of range)
		const float *src = reinterpret_cast<const float *>(p.sweeps + r);
		float w[Shape::FLOATS];
#pragma unroll
		for (int k = 0; k < Shape::FLOATS; k++) w[k] = src[k];
		typename Shape::Query Q;
		const bool live = Shape::prepare(w, Q);
		const uint32_t skip_prim = p.ignore_prim ? p.ignore_prim[r] : RTK_PRIM_NONE;
		float best_t = Shape::tmax(Q);
		uint32_t best_prim = RTK_PRIM_NONE, best_slot = 0;
		uint32_t top = (live && p.num_nodes != 0u && p.num_tris != 0u) ? 0u : RTK_REF_NONE;
		uint32_t sp = 0;
		if (COUNT) c_queries++;

		while (top != RTK_REF_NONE) {
			if ((int32_t)top < 0) {
				// ---------------------------------------------------------------- leaf: its records up to RTK_TRI_LAST
				uint32_t slot = top & 0x7fffffffu;
				if (COUNT) c_leaves++;
				while (slot < p.num_tris) {
					const sweep_f32x4 *t = reinterpret_cast<const sweep_f32x4 *>(reinterpret_cast<const char *>(p.tris) + (size_t)slot * RTK_TRI_STRIDE);
					const sweep_f32x4 A = t[0], B = t[1], C = t[2];
					const uint32_t prim = __float_as_uint(A.w), flags = __float_as_uint(B.w);
					bool wanted = prim != skip_prim;
					if (p.mesh_mask) {
						const uint32_t mesh = flags >> RTK_TRI_MESH_SHIFT;
						wanted = wanted && mesh < p.mesh_mask_bits && ((p.mesh_mask[mesh >> 5] >> (mesh & 31u)) & 1u);
					}
					if (COUNT) c_tris++;
					if (wanted) {
						const float a[3] = { A.x, A.y, A.z }, b[3] = { B.x, B.y, B.z }, c[3] = { C.x, C.y, C.z };
						float time;
						if (Shape::touches(Q, a, b, c, time) && rtk_sweep_better(time, prim, best_t, best_prim)) { best_t = time; best_prim = prim; best_slot = slot; }
					}
					if (ANY && best_prim != RTK_PRIM_NONE) break;
					if (flags & RTK_TRI_LAST) break;
					slot++;
				}
				top = RTK_REF_NONE;
				if (ANY && best_prim != RTK_PRIM_NONE) break;
			} else if (top < p.num_nodes) {
				// ---------------------------------------------------------------- node: four entry times, the first one first
				const sweep_f32x4 *nd = reinterpret_cast<const sweep_f32x4 *>(p.nodes + top);
				const sweep_f32x4 xl = nd[0], xh = nd[1], yl = nd[2], yh = nd[3], zl = nd[4], zh = nd[5];
				const sweep_u32x4 ch = *reinterpret_cast<const sweep_u32x4 *>(nd + 6);
				float key[4];
				uint32_t ref[4];
				if (COUNT) c_nodes++;
#pragma unroll
				for (int k = 0; k < 4; k++) {
					const float lo[3] = { xl[k], yl[k], zl[k] }, hi[3] = { xh[k], yh[k], zh[k] };
					float te;
					const bool some = Shape::slab(Q, lo, hi, te);
					const bool enter = ch[k] != RTK_REF_NONE && some && (ANY || !rtk_sweep_skip(te, best_t));
					// (an entry time of a live query is never a NaN; one of a scene with non-finite boxes is entered, first)
					key[k] = enter ? (te == te ? te : -INFINITY) : INFINITY;
					ref[k] = enter ? ch[k] : RTK_REF_NONE;
				}
				sweep_cswap(key[0], ref[0], key[1], ref[1]);
				sweep_cswap(key[2], ref[2], key[3], ref[3]);
				sweep_cswap(key[0], ref[0], key[2], ref[2]);
				sweep_cswap(key[1], ref[1], key[3], ref[3]);
				sweep_cswap(key[1], ref[1], key[2], ref[2]);
				top = ref[0];
				// the others far to near. A push that does not fit LDS or the spill area is dropped WITHOUT advancing sp and flagged
#pragma unroll
				for (int k = 3; k >= 1; k--) {
					if (ref[k] == RTK_REF_NONE) continue;
					const uint2 e = make_uint2(ref[k], __float_as_uint(key[k]));
					if (sp < SWEEP_LDS_STACK) { stk[sp][lane] = e; sp++; }
					else if (sp - SWEEP_LDS_STACK < p.spill_cap) { p.spill[(size_t)(sp - SWEEP_LDS_STACK) * p.spill_stride + glane] = e; sp++; if (COUNT) c_spills++; }
					else p.counter[RTK_ERROR_WORD] = 1ull;
				}
			} else top = RTK_REF_NONE;                                // (a child word beyond the array: not a tree; nothing is read)
			// ---------------------------------------------------------------- pop: the entry time again, best_t has shrunk since the push
			while (top == RTK_REF_NONE && sp != 0u) {
				--sp;
				const uint2 e = sp < SWEEP_LDS_STACK ? stk[sp][lane] : p.spill[(size_t)(sp - SWEEP_LDS_STACK) * p.spill_stride + glane];
				if (ANY || !rtk_sweep_skip(__uint_as_float(e.y), best_t)) top = e.x;
			}
		}

		const bool hit = best_prim != RTK_PRIM_NONE;
		if (COUNT && hit) c_hits++;
		if (ANY) { p.blocked[r] = hit ? 1 : 0; continue; }
		// the record, by the shape, from the answer's triangle alone
		sweep_u32x4 out;
		float side0[3], side1[3];
		if (hit) {
			const sweep_f32x4 *t = reinterpret_cast<const sweep_f32x4 *>(reinterpret_cast<const char *>(p.tris) + (size_t)best_slot * RTK_TRI_STRIDE);
			const sweep_f32x4 A = t[0], B = t[1], C = t[2];
			const float a[3] = { A.x, A.y, A.z }, b[3] = { B.x, B.y, B.z }, c[3] = { C.x, C.y, C.z };
			Shape::record(Q, w, true, best_t, best_prim, a, b, c, out, side0, side1);
		} else Shape::record(Q, w, false, best_t, best_prim, nullptr, nullptr, nullptr, out, side0, side1);   // (a miss has no triangle)
		*reinterpret_cast<sweep_u32x4 *>(p.records + r) = out;
		if (p.side0) { float *dst = p.side0 + (size_t)r * 3u; dst[0] = side0[0]; dst[1] = side0[1]; dst[2] = side0[2]; }
		if (p.side1) { float *dst = p.side1 + (size_t)r * 3u; dst[0] = side1[0]; dst[1] = side1[1]; dst[2] = side1[2]; }
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

// workgroups of the shape's kernel a CU holds, asked once per device
template <class Shape>
int sweep_walk_blocks_per_cu(int device)
{
	static std::atomic<int> known[RTK_MAX_DEVICES];
	if (device < 0 || device >= RTK_MAX_DEVICES) return 2;
	int b = known[device].load(std::memory_order_relaxed);
	if (b == 0) {
		if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, k_sweep_walk<Shape, false, false>, (int)SWEEP_THREADS, 0) != hipSuccess || b < 1) b = 2;
		known[device].store(b, std::memory_order_relaxed);
	}
	return b;
}

// the closest form writes d_records (d_side0, d_side1: each or NULL), the any-hit form d_blocked; a non-null `counted` makes it
// the counting form of the closest one
template <class Shape>
int rtk_launch_sweep_walk(const rtk_dev_scene *ds_c, const typename Shape::Sweep *d_sweeps, size_t num_sweeps, const rtk_ray_list *list,
	rtk_hit_record *d_records, float *d_side0, float *d_side1, uint8_t *d_blocked, bool any_hit, const rtk_dev_filter *filter,
	hipStream_t stream, rtk_trace_counters *counted)
{
	rtk_dev_scene *ds = const_cast<rtk_dev_scene *>(ds_c);
	const char *who = any_hit ? Shape::NAME_ANY : counted ? Shape::NAME_COUNTED : Shape::NAME;
	// everything the host can see is refused here, before any HIP call
	if (!ds || (num_sweeps && (!d_sweeps || (any_hit ? !d_blocked : !d_records)))) { rtk_set_error("%s: NULL scene, sweeps or output", who); return RTK_AMD_ERR_BAD_ARG; }
	if (list && (list->struct_size < sizeof(rtk_ray_list) || list->flags != 0u || !list->d_count)) {
		rtk_set_error("%s: bad list (struct_size %u, flags %#x, d_count %p)", who, list->struct_size, list->flags, (const void *)list->d_count);
		return RTK_AMD_ERR_BAD_ARG;
	}
	if (filter && filter->struct_size < sizeof(rtk_dev_filter)) { rtk_set_error("%s: rtk_dev_filter.struct_size is too small", who); return RTK_AMD_ERR_BAD_ARG; }
	if (filter && filter->d_after) { rtk_set_error("%s: rtk_dev_filter.d_after is not a filter of a sweep", who); return RTK_AMD_ERR_BAD_ARG; }
	if (filter && filter->d_mesh_mask && filter->mesh_mask_bits == 0) { rtk_set_error("%s: mesh mask without mesh_mask_bits", who); return RTK_AMD_ERR_BAD_ARG; }
	if (num_sweeps >= ((size_t)1 << 32)) { rtk_set_error("%s: %zu sweeps: a batch holds fewer than 2^32", who, num_sweeps); return RTK_AMD_ERR_BAD_ARG; }
	if (counted) *counted = rtk_trace_counters();
	if (num_sweeps == 0) return RTK_AMD_OK;
	if (!rtk_on_scene_device(ds, who)) return RTK_AMD_ERR_BAD_ARG;

	SweepWalkParams<Shape> p = {};
	p.sweeps = d_sweeps;
	p.ids = list ? reinterpret_cast<const unsigned long long *>(list->d_ids) : nullptr;
	p.count = list ? reinterpret_cast<const unsigned long long *>(list->d_count) : nullptr;
	p.records = d_records;
	p.side0 = d_side0;
	p.side1 = d_side1;
	p.blocked = d_blocked;
	if (filter) { p.mesh_mask = filter->d_mesh_mask; p.mesh_mask_bits = filter->mesh_mask_bits; p.ignore_prim = filter->d_ignore_prim; }
	p.n = (uint32_t)num_sweeps;
	const size_t blocks_needed = (num_sweeps + SWEEP_THREADS - 1u) / SWEEP_THREADS;
	size_t grid = (size_t)(ds->num_cus > 0 ? ds->num_cus : 1) * (size_t)sweep_walk_blocks_per_cu<Shape>(ds->device);
	if (grid > blocks_needed) grid = blocks_needed;

	// the scratch set of (scene, stream), held until the launch is enqueued (rtk_launch_closest does the same); the view and the
	// tree record are read under the same lock a rebuild replaces them under
	std::lock_guard<std::mutex> lock(ds->scratch_mutex);
	p.nodes = ds->view.nodes; p.tris = ds->view.tris; p.num_nodes = ds->view.num_nodes; p.num_tris = ds->view.num_tris;
	const size_t entries = ds->tree.stack_entries();
	const size_t spill_cap = entries > SWEEP_LDS_STACK ? entries - SWEEP_LDS_STACK : 0;
	LaunchScratch *sc = ds->scratch.get(stream);
	if (!sc) return RTK_AMD_ERR_OOM;
	if (spill_cap) {
		const int rc = sc->grow_spill(grid * SWEEP_THREADS, spill_cap, sizeof(uint2));
		if (rc != RTK_AMD_OK) return rc;
	}
	p.spill = sc->spill.as<uint2>();
	p.spill_stride = (uint32_t)(spill_cap ? sc->spill.capacity : 0);
	p.spill_cap = (uint32_t)spill_cap;
	p.counter = sc->d_counter;
	if (!counted) {
		if (any_hit) hipLaunchKernelGGL((k_sweep_walk<Shape, true, false>), dim3((unsigned)grid), dim3(SWEEP_THREADS), 0, stream, p);
		else hipLaunchKernelGGL((k_sweep_walk<Shape, false, false>), dim3((unsigned)grid), dim3(SWEEP_THREADS), 0, stream, p);
		RTK_HIP_CHECK(hipGetLastError(), RTK_AMD_ERR_HIP);
		return RTK_AMD_OK;
	}
	// the counting form: the visit counters start from zero, are brought home and the stream is waited for
	unsigned long long c[8], err = 0;
	RTK_HIP_CHECK(hipMemsetAsync(sc->d_counter, 0, RTK_COUNTER_WORDS * sizeof(unsigned long long), stream), RTK_AMD_ERR_HIP);
	hipLaunchKernelGGL((k_sweep_walk<Shape, false, true>), dim3((unsigned)grid), dim3(SWEEP_THREADS), 0, stream, p);
	RTK_HIP_CHECK(hipGetLastError(), RTK_AMD_ERR_HIP);
	RTK_HIP_CHECK(hipMemcpyAsync(c, sc->d_counter, sizeof(c), hipMemcpyDeviceToHost, stream), RTK_AMD_ERR_HIP);
	RTK_HIP_CHECK(hipMemcpyAsync(&err, sc->d_counter + RTK_ERROR_WORD, sizeof(err), hipMemcpyDeviceToHost, stream), RTK_AMD_ERR_HIP);
	RTK_HIP_CHECK(hipStreamSynchronize(stream), RTK_AMD_ERR_HIP);
	counted->rays = c[1]; counted->nodes = c[2]; counted->leaves = c[3]; counted->triangles = c[4]; counted->hits = c[5]; counted->stack_spills = c[6];
	if (err) {
		(void)hipMemsetAsync(sc->d_counter + RTK_ERROR_WORD, 0, sizeof(err), stream);
		rtk_set_error("%s: traversal stack overflow (corrupted scene)", Shape::NAME_COUNTED);
		return RTK_AMD_ERR_BAD_SCENE;
	}
	return RTK_AMD_OK;
}

} // namespace

#endif
