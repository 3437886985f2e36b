// rtk_overlap_walk.h -- the walk and the launch of the three overlap queries (rtk_box.hip, rtk_obb.hip, rtk_touch.hip: which
// triangles of the scene touch this box, this oriented box, this triangle), once. A shape's file holds what is the shape's alone,
// as a struct of static functions (below); the result is a function of the scene's triangle records, the filter and the query
// alone, by the shape's rule header: the tree and the order of the walk only decide which records are never looked at.
//
// THE WALK is k_within's frame (rtk_within.hip): one query per lane of a 64-wide wave; a fixed grid of resident workgroups that
// steps through the batch (so that the spill area is sized by the grid, not by the batch); the exact 128-byte nodes only. The
// four child boxes of a node are tested by the shape's skip, which is static: nothing the walk has kept can cull it, because the
// tree is not ordered by id. So a stack entry is a bare 4-byte reference, nothing is looked at again at the pop and the order of
// the walk is irrelevant: the first admitted child is entered, the others are pushed. A leaf is its run of DevTri records up to
// RTK_TRI_LAST, one at a time through the shape's candidate test. A child word beyond the node array and a slot beyond the
// triangle array are not followed.
//   the count form (FILL = false)  counts the candidates.
//   the fill form (FILL = true)    a candidate's id goes into the query's segment through rtk_box_insert, the same function the
//       host drivers call; the lane keeps the segment's last entry (`worst`) in a register, so a candidate that does not get in
//       costs no memory access. A query without room does not walk. Lanes write disjoint segments; a list that names a query
//       twice is the exception, and there the first lane to claim the query (one bit per query in the scratch set, cleared ahead
//       of the launch) answers it and the others leave it alone: the bytes are the same whoever wins.
// THE STACK: OVERLAP_LDS_STACK entries per lane in LDS, [entry][lane], 4 bytes each: one ds_write_b32 / ds_read_b32 per wave and
// push or pop, the 64 lanes on consecutive words (no bank conflict); 16 * 64 * 4 B * 4 waves = 16 384 B per workgroup, never the
// limit of a shape's occupancy (see the shapes' *_RESOURCES). Deeper entries -- a deep, lopsided tree, a query that covers much
// of the scene -- go to THE SPILL area of the (scene, stream) scratch set; a push that fits neither (impossible for a tree) is
// dropped WITHOUT advancing and flagged in the stream's launch-error word.
//
// A SHAPE supplies
//     Query, FLOATS            the query record as the caller holds it and its width in floats (records are only 4-byte aligned)
//     Filter, Extra            the caller's filter record (void: the shape takes none) and what a launch keeps of it
//     Prepared                 what the rule keeps in registers across the walk
//     NAME_COUNT, NAME_ALL, NAME_COUNTED, NOUN   the three entry points and the queries' noun, for the error texts
//     extras(filter, who, x)   host: x from the filter (or NULL), or false with the error text set
//     prepare(w, x, r, Q)      Q of query slot r from its floats w: false = the query touches nothing
//     skip(Q, clo, chi)        true = nothing inside this child box can be a candidate
//     candidate(Q, v0, v1, v2, prim)   the shape against one triangle record
// How a shape's function takes Q (by reference or by value) is the shape's choice: all of them are forced inline, and the form
// decides only how the compiler pairs the rule's packed arithmetic (profiles/overlap_walk_refactor.log says what was tried).
#ifndef RTK_OVERLAP_WALK_H
#define RTK_OVERLAP_WALK_H

#include "rtk_dev.h"
#include "rtk_box_rule.h"          // rtk_box_insert

#include <atomic>
#include <mutex>

#define OVERLAP_THREADS 256u
#define OVERLAP_WAVES (OVERLAP_THREADS / 64u)
#define OVERLAP_LDS_STACK 16u      // entries per lane held in LDS, 4 bytes each: 16 KB per workgroup

namespace {

template <class Shape>
struct OverlapParams {
	const DevNode *nodes;
	const DevTri *tris;
	uint32_t num_nodes;
	uint32_t num_tris;
	const typename Shape::Query *queries;
	const unsigned long long *ids;     // or NULL: 0, 1, 2, ...
	const unsigned long long *count;   // or NULL: n
	uint32_t *counts;                  // the count form: one word per query slot; the fill form: d_written or NULL
	const unsigned long long *offsets; // the fill form: n + 1 entries
	uint32_t *prims;                   // the fill form
	uint32_t *claim;                   // the fill form with ids: one bit per query slot, cleared ahead of the launch; else NULL
	unsigned long long *counter;       // the stream's counter words: [RTK_ERROR_WORD] is set by a dropped push
	uint32_t *spill;                   // [entry][lane of the launch]
	uint32_t spill_stride;
	uint32_t spill_cap;                // entries per lane
	uint32_t n;
	typename Shape::Extra extra;       // the shape's own, per launch
};

typedef float overlap_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t overlap_u32x4 __attribute__((ext_vector_type(4)));

// FILL: the list into the query's segment (else the count); COUNT: the visit counts of the shape's _counted entry point, summed
// per lane and added to the stream's counter words at the end
template <class Shape, bool FILL, bool COUNT>
__global__ void __launch_bounds__(OVERLAP_THREADS) k_overlap_walk(OverlapParams<Shape> p)
{
	__shared__ uint32_t s_stack[OVERLAP_WAVES][OVERLAP_LDS_STACK][64];

	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint32_t (*stk)[64] = s_stack[wave];
	const uint32_t glane = blockIdx.x * OVERLAP_THREADS + threadIdx.x;
	uint32_t m = p.n;
	if (p.count) { const unsigned long long listed = *p.count; m = listed < p.n ? (uint32_t)listed : p.n; }
	const unsigned long long step = (unsigned long long)gridDim.x * OVERLAP_THREADS;
	uint32_t c_queries = 0, c_nodes = 0, c_leaves = 0, c_tris = 0, c_hits = 0, c_spills = 0;

	for (unsigned long long i = glane; i < m; i += step) {
		const uint32_t r = p.ids ? (uint32_t)p.ids[i] : (uint32_t)i;
		if (r >= p.n) continue;                                   // (the caller's error; nothing is read or written out of range)
		if (FILL && p.claim) {
			// a query the list names twice is answered once: two lanes must not sort into one segment
			const uint32_t bit = 1u << (r & 31u);
			if (atomicOr(p.claim + (r >> 5), bit) & bit) continue;
		}
		// (a query is only 4-byte aligned, so FLOATS float loads)
		const float *qw = reinterpret_cast<const float *>(p.queries + r);
		float w[Shape::FLOATS];
#pragma unroll
		for (int k = 0; k < Shape::FLOATS; k++) w[k] = qw[k];
		typename Shape::Prepared Q;
		const bool live = Shape::prepare(w, p.extra, r, Q);
		uint32_t kept = 0;                                        // candidates counted, or entries of the segment in use
		uint32_t room = 0;
		uint32_t *seg = nullptr;
		uint32_t worst = 0u;                                      // the segment's last entry once kept == room
		bool walk = live && p.num_nodes != 0u && p.num_tris != 0u;
		if (FILL) {
			// (offsets that decrease are the caller's error: such a query has no room, nothing is written for it)
			const unsigned long long o0 = p.offsets[r], o1 = p.offsets[(size_t)r + 1u];
			const unsigned long long space = o1 > o0 ? o1 - o0 : 0ull;
			room = space < 0xffffffffull ? (uint32_t)space : 0xffffffffu;
			seg = p.prims + o0;
			walk = walk && room != 0u;                            // nothing can be kept: no walk
		}
		uint32_t top = walk ? 0u : RTK_REF_NONE;
		uint32_t sp = 0;
		if (COUNT) c_queries++;

		while (top != RTK_REF_NONE) {
			if ((int32_t)top < 0) {
				// ---------------------------------------------------------------- leaf: its records up to RTK_TRI_LAST
				uint32_t slot = top & 0x7fffffffu;
				if (COUNT) c_leaves++;
				while (slot < p.num_tris) {
					const overlap_f32x4 *t = reinterpret_cast<const overlap_f32x4 *>(reinterpret_cast<const char *>(p.tris) + (size_t)slot * RTK_TRI_STRIDE);
					const overlap_f32x4 A = t[0], B = t[1], C = t[2];
					const float v0[3] = { A.x, A.y, A.z }, v1[3] = { B.x, B.y, B.z }, v2[3] = { C.x, C.y, C.z };
					if (COUNT) c_tris++;
					if (Shape::candidate(Q, v0, v1, v2, __float_as_uint(A.w))) {
						if (FILL) kept = rtk_box_insert(seg, room, kept, __float_as_uint(A.w), worst);
						else kept++;
					}
					if (__float_as_uint(B.w) & RTK_TRI_LAST) break;
					slot++;
				}
				top = RTK_REF_NONE;
			} else if (top < p.num_nodes) {
				// ---------------------------------------------------------------- node: four boxes
				const overlap_f32x4 *nd = reinterpret_cast<const overlap_f32x4 *>(p.nodes + top);
				const overlap_f32x4 xl = nd[0], xh = nd[1], yl = nd[2], yh = nd[3], zl = nd[4], zh = nd[5];
				const overlap_u32x4 ch = *reinterpret_cast<const overlap_u32x4 *>(nd + 6);
				uint32_t ref[4];
				if (COUNT) c_nodes++;
#pragma unroll
				for (int k = 0; k < 4; k++) {
					const float clo[3] = { xl[k], yl[k], zl[k] }, chi[3] = { xh[k], yh[k], zh[k] };
					ref[k] = ch[k] != RTK_REF_NONE && !Shape::skip(Q, clo, chi) ? ch[k] : RTK_REF_NONE;
				}
				// any order gives the same result: the first admitted slot is entered
				top = RTK_REF_NONE;
#pragma unroll
				for (int k = 0; k < 4; k++) {
					if (top == RTK_REF_NONE && ref[k] != RTK_REF_NONE) { top = ref[k]; ref[k] = RTK_REF_NONE; }
				}
				// the others. A push that does not fit LDS or the spill area is dropped WITHOUT advancing sp and flagged
#pragma unroll
				for (int k = 3; k >= 0; k--) {
					if (ref[k] == RTK_REF_NONE) continue;
					if (sp < OVERLAP_LDS_STACK) { stk[sp][lane] = ref[k]; sp++; }
					else if (sp - OVERLAP_LDS_STACK < p.spill_cap) { p.spill[(size_t)(sp - OVERLAP_LDS_STACK) * p.spill_stride + glane] = ref[k]; sp++; if (COUNT) c_spills++; }
					else p.counter[RTK_ERROR_WORD] = 1ull;
				}
			} else top = RTK_REF_NONE;                                // (a child word beyond the array: not a tree; nothing is read)
			// ---------------------------------------------------------------- pop
			if (top == RTK_REF_NONE && sp != 0u) {
				--sp;
				top = sp < OVERLAP_LDS_STACK ? stk[sp][lane] : p.spill[(size_t)(sp - OVERLAP_LDS_STACK) * p.spill_stride + glane];
			}
		}

		if (COUNT && kept != 0u) c_hits++;
		if (p.counts) __builtin_nontemporal_store(kept, p.counts + r);
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

// form: fill | counted << 1
template <class Shape>
void (*overlap_form(int form))(OverlapParams<Shape>)
{
	switch (form & 3) {
	case 0: return k_overlap_walk<Shape, false, false>;
	case 1: return k_overlap_walk<Shape, true, false>;
	case 2: return k_overlap_walk<Shape, false, true>;
	default: return k_overlap_walk<Shape, true, true>;
	}
}

// workgroups of a shape's form a CU holds, asked once per device
template <class Shape>
int overlap_blocks_per_cu(int device, int form)
{
	static std::atomic<int> known[RTK_MAX_DEVICES][4];
	if (device < 0 || device >= RTK_MAX_DEVICES) return 4;
	int b = known[device][form & 3].load(std::memory_order_relaxed);
	if (b == 0) {
		if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, overlap_form<Shape>(form), (int)OVERLAP_THREADS, 0) != hipSuccess || b < 1) b = 4;
		known[device][form & 3].store(b, std::memory_order_relaxed);
	}
	return b;
}

// !fill: the count form (d_counts the counts); else the fill form (d_counts the written numbers, or NULL). A non-null `counted`
// makes it the counting form of either
template <class Shape>
int rtk_launch_overlap_walk(const rtk_dev_scene *ds_c, const typename Shape::Query *d_queries, size_t num_queries, const rtk_ray_list *list,
	const typename Shape::Filter *filter, uint32_t *d_counts, const uint64_t *d_offsets, uint32_t *d_prims, bool fill, hipStream_t stream,
	rtk_trace_counters *counted)
{
	rtk_dev_scene *ds = const_cast<rtk_dev_scene *>(ds_c);
	const char *const who = counted ? Shape::NAME_COUNTED : fill ? Shape::NAME_ALL : Shape::NAME_COUNT;
	// everything the host can see is refused here, before any HIP call
	if (!ds) { rtk_set_error("%s: NULL scene", who); return RTK_AMD_ERR_BAD_ARG; }
	if (num_queries && (!d_queries || (fill ? (!d_offsets || !d_prims) : !d_counts))) {
		rtk_set_error("%s: NULL %s, %s", who, Shape::NOUN, fill ? "offsets or prims" : "counts");
		return RTK_AMD_ERR_BAD_ARG;
	}
	if (list && (list->struct_size < sizeof(rtk_ray_list) || list->flags != 0u || !list->d_count)) {
		rtk_set_error("%s: bad list (struct_size %u, flags %#x, d_count %p)", who, list->struct_size, list->flags, (const void *)list->d_count);
		return RTK_AMD_ERR_BAD_ARG;
	}
	OverlapParams<Shape> p = {};
	if (!Shape::extras(filter, who, p.extra)) return RTK_AMD_ERR_BAD_ARG;
	if (num_queries >= ((size_t)1 << 32)) { rtk_set_error("%s: %zu queries: a batch holds fewer than 2^32", who, num_queries); return RTK_AMD_ERR_BAD_ARG; }
	if (counted) *counted = rtk_trace_counters();
	if (num_queries == 0) return RTK_AMD_OK;
	if (!rtk_on_scene_device(ds, who)) return RTK_AMD_ERR_BAD_ARG;

	p.queries = d_queries;
	p.ids = list ? reinterpret_cast<const unsigned long long *>(list->d_ids) : nullptr;
	p.count = list ? reinterpret_cast<const unsigned long long *>(list->d_count) : nullptr;
	p.counts = d_counts;
	p.offsets = reinterpret_cast<const unsigned long long *>(d_offsets);
	p.prims = d_prims;
	p.n = (uint32_t)num_queries;
	const int form = (fill ? 1 : 0) | (counted ? 2 : 0);
	const size_t blocks_needed = (num_queries + OVERLAP_THREADS - 1u) / OVERLAP_THREADS;
	size_t grid = (size_t)(ds->num_cus > 0 ? ds->num_cus : 1) * (size_t)overlap_blocks_per_cu<Shape>(ds->device, form);
	if (grid > blocks_needed) grid = blocks_needed;

	// the scratch set of (scene, stream), held until the launch is enqueued; the view and the tree record are read under the
	// same lock a rebuild replaces them under (rtk_launch_within does the same)
	std::lock_guard<std::mutex> lock(ds->scratch_mutex);
	p.nodes = ds->view.nodes; p.tris = ds->view.tris; p.num_nodes = ds->view.num_nodes; p.num_tris = ds->view.num_tris;
	const size_t entries = ds->tree.stack_entries();
	const size_t spill_cap = entries > OVERLAP_LDS_STACK ? entries - OVERLAP_LDS_STACK : 0;
	LaunchScratch *sc = ds->scratch.get(stream);
	if (!sc) return RTK_AMD_ERR_OOM;
	if (spill_cap) {
		// (sized in 8-byte entries although these are 4: the area is shared with the other walks of the stream, which hold such entries)
		const int rc = sc->grow_spill(grid * OVERLAP_THREADS, spill_cap, sizeof(uint2));
		if (rc != RTK_AMD_OK) return rc;
	}
	p.spill = sc->spill.as<uint32_t>();
	p.spill_stride = (uint32_t)(spill_cap ? sc->spill.capacity : 0);
	p.spill_cap = (uint32_t)spill_cap;
	p.counter = sc->d_counter;
	if (fill && p.ids) {
		// one bit per query slot, in the area rtk_dev_select_rays keeps its masks in: launches of one stream are ordered
		const size_t claim_bytes = ((num_queries + 31u) / 32u) * sizeof(uint32_t);
		const int rc = sc->grow(sc->select, claim_bytes, claim_bytes);
		if (rc != RTK_AMD_OK) return rc;
		p.claim = sc->select.as<uint32_t>();
		RTK_HIP_CHECK(hipMemsetAsync(p.claim, 0, claim_bytes, stream), RTK_AMD_ERR_HIP);
	}
	if (!counted) {
		hipLaunchKernelGGL(overlap_form<Shape>(form), dim3((unsigned)grid), dim3(OVERLAP_THREADS), 0, stream, p);
		RTK_HIP_CHECK(hipGetLastError(), RTK_AMD_ERR_HIP);
		return RTK_AMD_OK;
	}
	// the counting form: the visit counters start from zero, are brought home and the stream is waited for
	unsigned long long c[8], err = 0;
	RTK_HIP_CHECK(hipMemsetAsync(sc->d_counter, 0, RTK_COUNTER_WORDS * sizeof(unsigned long long), stream), RTK_AMD_ERR_HIP);
	hipLaunchKernelGGL(overlap_form<Shape>(form), dim3((unsigned)grid), dim3(OVERLAP_THREADS), 0, stream, p);
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

} // namespace

#endif
