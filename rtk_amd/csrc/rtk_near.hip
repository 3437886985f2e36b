// rtk_near.hip -- rtk_dev_triangles_near_count / rtk_dev_triangles_near_all: for every query triangle (or segment, or point) the
// triangles of a device scene nearer than its limit, counted, or listed in ascending (dist2, prim) order with the two nearest
// points of each pair into the query's own segment -- all of them or the first `room` --, by the rule of rtk_near_rule.h on top
// of rtk_pair_rule.h. The result is a function of the scene's triangle records and the query alone (DESIGN.md "Triangles near a
// triangle"): the tree and the order of the walk only decide which records are never looked at.
//
// The family's frame (rtk_pair.hip, rtk_within.hip): one query per lane of a 64-wide wave, a fixed grid of resident workgroups
// that steps through the batch, exact 128-byte nodes only (the skip is only as good as the bound), rtk_pair_hoist_query once per
// query, a leaf as its run of DevTri records up to RTK_TRI_LAST, the stack [entry][lane] in LDS with the deeper part in the
// spill area of the (scene, stream) scratch set, a push that fits neither dropped WITHOUT advancing and flagged in the stream's
// launch-error word. Per record, from one 48-byte fetch: the filter first (an integer comparison, and nine vertex comparisons
// under the flag), then the bound of the record's OWN box through rtk_near_skip, then rtk_pair_evaluate.
//   the count form (FILL = false)  the bound is static -- a child is entered iff its box bound is below max_dist2 --, so no key
//       travels with a reference (4-byte entries), the order of the walk is irrelevant (the first admitted child is entered, the
//       others are pushed) and no best or worst entry is kept.
//   the fill form (FILL = true)    (reference, bound) entries: the nearest child is entered, the others are pushed far to near,
//       and a popped entry's bound is looked at again, because the segment may have filled up and its worst entry improved since
//       the push. A candidate goes into the segment through rtk_near_insert, the function the host driver calls; the lane keeps
//       the segment's last entry (`worst`) in registers, so a record that does not get in costs no memory access. A query without
//       room does not walk. Lanes write disjoint segments; a list that names a query twice is the exception, and there the first
//       lane to claim the query (one bit per query in the scratch set's select area, cleared ahead of the launch, as
//       rtk_launch_within does) answers it and the others leave it alone: the bytes are the same whoever wins.
// The two point arrays are looked at through their pointers at run time (NULL: not written), not through a template parameter:
// one fill form instead of four.
//
// FLOATING POINT: the flags of rtk_pair.hip (no contraction, IEEE quotients); every bit is the rule headers'.
#include "rtk_dev.h"
#include "rtk_near_rule.h"

#include <atomic>
#include <mutex>

// NR_RESOURCES: the compiler's report (gfx950, -O3, -Rpass-analysis=kernel-resource-usage) for each instantiated form
// <FILL, COUNT>; scratch 0 and no VGPR spills in every one of them, so neither the node loop, the record loop nor the insertion
// touches private memory; the SGPRs past the 106 a wave may use go to lanes of a VGPR (counted in the VGPR column), not to memory:
//                         VGPRs   AGPRs   SGPRs (spilled)   scratch   LDS per workgroup   waves per SIMD
//   count          <0, 0>  256     17       106 (8)           0 B         16 384 B              1
//   fill           <1, 0>  247      0       106 (32)          0 B         32 768 B              2
//   count, counted <0, 1>  254     23       106 (4)           0 B         16 384 B              1
//   fill, counted  <1, 1>  253      0       106 (36)          0 B         32 768 B              2
// A workgroup is four waves, one per SIMD, so "workgroups per CU" and "waves per SIMD" are the same number, and the registers
// decide it (512 / 256 = 2; the LDS would hold five and ten). The fill form stands where k_pair stands (254 VGPRs, 2 waves): the
// running best of k_pair (nine floats and an id) gives way to `worst`'s dist2 and id, kept, room and the segment's offset, and
// the two points of a candidate live only until rtk_near_insert has stored them. THE COUNT FORM MISSES ITS TARGET: it keeps
// less state alive than k_pair and should need no more registers, but the compiler gives it all 256 VGPRs and parks 17 more
// values in AGPRs (register copies, not memory), which leaves room for one wave per SIMD instead of two. Asked for two waves
// (__launch_bounds__(256, 2)) it stays within 256 registers by spilling 18 VGPRs to 76 bytes of private memory per lane (100
// bytes in the counting build; where in the walk they are touched has not been looked up); the fill form is unchanged by the
// request. Scratch 0 was preferred to the second wave; which of the two is faster has not been measured. The six crossings of
// rtk_pair_evaluate stay six calls with constant indices (rtk_pair.hip says why). Not tuned.

#define NR_THREADS 256u
#define NR_WAVES (NR_THREADS / 64u)
#define NR_LDS_STACK 16u           // entries per lane held in LDS (4 bytes each in the count form, 8 in the fill form)

static_assert(RTK_TOUCH_RULE_SKIP_SHARED_VERTEX == RTK_TOUCH_SKIP_SHARED_VERTEX, "the rule header's flag is the interface's");
static_assert(sizeof(rtk_tri_query) == 36, "a float32 [n, 9] tensor is a batch of queries");

namespace {

struct NearParams {
	const DevNode *nodes;
	const DevTri *tris;
	uint32_t num_nodes;
	uint32_t num_tris;
	const rtk_tri_query *queries;
	const float *max_dist2;            // or NULL: RTK_INF for every query; indexed by query slot
	const uint32_t *first_prim;        // or NULL: 0 for every query; indexed by query slot
	const unsigned long long *ids;     // or NULL: 0, 1, 2, ...
	const unsigned long long *count;   // or NULL: n
	uint32_t *counts;                  // the count form: one word per query slot; the fill form: d_written or NULL
	const unsigned long long *offsets; // the fill form: n + 1 entries
	rtk_closest_record *records;       // the fill form
	float *points_query;               // the fill form, or NULL
	float *points_scene;               // the fill form, or NULL
	uint32_t *claim;                   // the fill form with ids: one bit per query slot, cleared ahead of the launch; else NULL
	unsigned long long *counter;       // the stream's counter words: [RTK_ERROR_WORD] is set by a dropped push
	void *spill;                       // [entry][lane of the launch], uint32_t or uint2
	uint32_t spill_stride;
	uint32_t spill_cap;                // entries per lane
	uint32_t n;
	uint32_t flags;                    // RTK_TOUCH_SKIP_SHARED_VERTEX
};

typedef float nr_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t nr_u32x4 __attribute__((ext_vector_type(4)));

// ascending by key; the reference travels with it
__device__ __forceinline__ void nr_cswap(uint32_t &ka, uint32_t &ra, uint32_t &kb, uint32_t &rb)
{
	const bool swap = kb < ka;
	const uint32_t k0 = swap ? kb : ka, k1 = swap ? ka : kb, r0 = swap ? rb : ra, r1 = swap ? ra : rb;
	ka = k0; kb = k1; ra = r0; rb = r1;
}

template <bool FILL> struct NrEntry { typedef uint32_t type; };
template <> struct NrEntry<true> { typedef uint2 type; };

// FILL: the list into the query's segment (else the count); COUNT: the visit counts of rtk_dev_triangles_near_counted, summed per
// lane and added to the stream's counter words at the end (triangles = records fetched; a record that the filter or its own box
// rules out is fetched and counted, not evaluated)
template <bool FILL, bool COUNT>
__global__ void __launch_bounds__(NR_THREADS) k_near(NearParams p)
{
	typedef typename NrEntry<FILL>::type entry_t;
	__shared__ entry_t s_stack[NR_WAVES][NR_LDS_STACK][64];

	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	entry_t (*stk)[64] = s_stack[wave];
	entry_t *const spill = static_cast<entry_t *>(p.spill);
	const uint32_t glane = blockIdx.x * NR_THREADS + threadIdx.x;
	uint32_t m = p.n;
	if (p.count) { const unsigned long long listed = *p.count; m = listed < p.n ? (uint32_t)listed : p.n; }
	const unsigned long long step = (unsigned long long)gridDim.x * NR_THREADS;
	uint32_t c_queries = 0, c_nodes = 0, c_leaves = 0, c_tris = 0, c_hits = 0, c_spills = 0;

	for (unsigned long long i = glane; i < m; i += step) {
		const uint32_t r = p.ids ? (uint32_t)p.ids[i] : (uint32_t)i;
		if (r >= p.n) continue;                                   // (the caller's error; nothing is read or written out of range)
		if (FILL && p.claim) {
			// a query the list names twice is answered once: two lanes must not sort into one segment
			const uint32_t bit = 1u << (r & 31u);
			if (atomicOr(p.claim + (r >> 5), bit) & bit) continue;
		}
		// (36 bytes at a stride of 36: a query is only 4-byte aligned)
		const float *qw = reinterpret_cast<const float *>(p.queries + r);
		const float a0[3] = { qw[0], qw[1], qw[2] }, a1[3] = { qw[3], qw[4], qw[5] }, a2[3] = { qw[6], qw[7], qw[8] };
		const float max2 = p.max_dist2 ? p.max_dist2[r] : RTK_INF;
		const uint32_t first = p.first_prim ? p.first_prim[r] : 0u;
		rtk_pair_hoist h;
		rtk_pair_hoist_query(a0, a1, a2, h);
		uint32_t kept = 0;                                        // candidates counted, or entries of the segment in use
		uint32_t room = 0;
		rtk_closest_record *seg = nullptr;
		float *seg_qa = nullptr, *seg_qb = nullptr;
		rtk_closest_record worst = { 0.0f, 0.0f, 0.0f, 0u };       // the segment's last entry once kept == room
		// a limit that is NaN, zero or negative and a query that is not live have no candidates: no walk
		bool walk = max2 > 0.0f && rtk_touch_live(a0, a1, a2) && p.num_nodes != 0u && p.num_tris != 0u;
		if (FILL) {
			// (offsets that decrease are the caller's error: such a query has no room, nothing is written for it)
			const unsigned long long o0 = p.offsets[r], o1 = p.offsets[(size_t)r + 1u];
			const unsigned long long space = o1 > o0 ? o1 - o0 : 0ull;
			room = space < 0xffffffffull ? (uint32_t)space : 0xffffffffu;
			seg = p.records + o0;
			if (p.points_query) seg_qa = p.points_query + o0 * 3ull;
			if (p.points_scene) seg_qb = p.points_scene + o0 * 3ull;
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
					const nr_f32x4 *t = reinterpret_cast<const nr_f32x4 *>(reinterpret_cast<const char *>(p.tris) + (size_t)slot * RTK_TRI_STRIDE);
					const nr_f32x4 A = t[0], B = t[1], C = t[2];
					const float b0[3] = { A.x, A.y, A.z }, b1[3] = { B.x, B.y, B.z }, b2[3] = { C.x, C.y, C.z };
					const uint32_t prim = __float_as_uint(A.w);
					if (COUNT) c_tris++;
					float blo[3], bhi[3];
					rtk_pair_box(b0, b1, b2, blo, bhi);
					if (rtk_touch_filter_passes(prim, first, p.flags, a0, a1, a2, b0, b1, b2)
						&& !rtk_near_skip(rtk_pair_box_bound(blo, bhi, h.lo, h.hi), max2, FILL && kept == room, worst.dist2)) {
						rtk_pair_result pr;
						rtk_pair_evaluate(h, b0, b1, b2, pr);
						if (rtk_near_candidate(pr.dist2, max2)) {
							if (FILL) {
								const rtk_closest_record cand = { pr.dist2, pr.u, pr.v, prim };
								kept = rtk_near_insert(seg, seg_qa, seg_qb, room, kept, cand, pr.qa, pr.qb, worst);
							} else kept++;
						}
					}
					if (__float_as_uint(B.w) & RTK_TRI_LAST) break;
					slot++;
				}
				top = RTK_REF_NONE;
			} else if (top < p.num_nodes) {
				// ---------------------------------------------------------------- node: four bounds
				const nr_f32x4 *nd = reinterpret_cast<const nr_f32x4 *>(p.nodes + top);
				const nr_f32x4 xl = nd[0], xh = nd[1], yl = nd[2], yh = nd[3], zl = nd[4], zh = nd[5];
				const nr_u32x4 ch = *reinterpret_cast<const nr_u32x4 *>(nd + 6);
				uint32_t key[4], ref[4];
				if (COUNT) c_nodes++;
#pragma unroll
				for (int k = 0; k < 4; k++) {
					const float lo[3] = { xl[k], yl[k], zl[k] }, hi[3] = { xh[k], yh[k], zh[k] };
					const float bound = rtk_pair_box_bound(lo, hi, h.lo, h.hi);
					const bool enter = ch[k] != RTK_REF_NONE && !rtk_near_skip(bound, max2, FILL && kept == room, worst.dist2);
					// (bounds are >= +0: their bits order like their values; a NaN bound is entered, first)
					key[k] = enter ? (bound == bound ? __float_as_uint(bound) : 0u) : 0xffffffffu;
					ref[k] = enter ? ch[k] : RTK_REF_NONE;
				}
				if (FILL) {
					// nearest first: the segment fills with near records and its worst entry starts to cull
					nr_cswap(key[0], ref[0], key[1], ref[1]);
					nr_cswap(key[2], ref[2], key[3], ref[3]);
					nr_cswap(key[0], ref[0], key[2], ref[2]);
					nr_cswap(key[1], ref[1], key[3], ref[3]);
					nr_cswap(key[1], ref[1], key[2], ref[2]);
					top = ref[0];
				} else {
					// any order gives the same count: the first admitted slot is entered
					top = RTK_REF_NONE;
#pragma unroll
					for (int k = 0; k < 4; k++) {
						if (top == RTK_REF_NONE && ref[k] != RTK_REF_NONE) { top = ref[k]; ref[k] = RTK_REF_NONE; }
					}
				}
				// the others (far to near in the fill form). A push that does not fit LDS or the spill area is dropped WITHOUT advancing sp and flagged
#pragma unroll
				for (int k = 3; k >= (FILL ? 1 : 0); k--) {
					if (ref[k] == RTK_REF_NONE) continue;
					entry_t e;
					if constexpr (FILL) e = make_uint2(ref[k], key[k]); else e = ref[k];
					if (sp < NR_LDS_STACK) { stk[sp][lane] = e; sp++; }
					else if (sp - NR_LDS_STACK < p.spill_cap) { spill[(size_t)(sp - NR_LDS_STACK) * p.spill_stride + glane] = e; sp++; if (COUNT) c_spills++; }
					else p.counter[RTK_ERROR_WORD] = 1ull;
				}
			} else top = RTK_REF_NONE;                                // (a child word beyond the array: not a tree; nothing is read)
			// ---------------------------------------------------------------- pop; the fill form looks at the bound again
			while (top == RTK_REF_NONE && sp != 0u) {
				--sp;
				const entry_t e = sp < NR_LDS_STACK ? stk[sp][lane] : spill[(size_t)(sp - NR_LDS_STACK) * p.spill_stride + glane];
				if constexpr (FILL) {
					if (!rtk_near_skip(__uint_as_float(e.y), max2, kept == room, worst.dist2)) top = e.x;
				} else top = e;
			}
		}

		if (COUNT && kept != 0u) c_hits++;
		if (p.counts) p.counts[r] = kept;
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

typedef void (*near_kernel_fn)(NearParams);

// form: fill | counted << 1
near_kernel_fn near_form(int form)
{
	switch (form & 3) {
	case 0: return k_near<false, false>;
	case 1: return k_near<true, false>;
	case 2: return k_near<false, true>;
	default: return k_near<true, true>;
	}
}

// workgroups of a form a CU holds, asked once per device
int near_blocks_per_cu(int device, int form)
{
	static std::atomic<int> known[RTK_MAX_DEVICES][4];
	if (device < 0 || device >= RTK_MAX_DEVICES) return 2;
	int b = known[device][form & 3].load(std::memory_order_relaxed);
	if (b == 0) {
		if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, near_form(form), (int)NR_THREADS, 0) != hipSuccess || b < 1) b = 2;
		known[device][form & 3].store(b, std::memory_order_relaxed);
	}
	return b;
}

} // namespace

extern "C" uint32_t rtk_amd_near_stack_entries(void) { return NR_LDS_STACK; }

// fill: the fill form (d_counts the written numbers, or NULL); else the count form (d_counts the counts)
int rtk_launch_near(const rtk_dev_scene *ds_c, const rtk_tri_query *d_tris, size_t num_queries, const rtk_ray_list *list,
	const rtk_touch_filter *filter, const float *d_max_dist2, uint32_t *d_counts, const uint64_t *d_offsets, rtk_closest_record *d_records,
	float *d_points_query, float *d_points_scene, bool fill, hipStream_t stream, rtk_trace_counters *counted)
{
	rtk_dev_scene *ds = const_cast<rtk_dev_scene *>(ds_c);
	const char *const who = counted ? "rtk_dev_triangles_near_counted" : fill ? "rtk_dev_triangles_near_all" : "rtk_dev_triangles_near_count";
	// everything the host can see is refused here, before any HIP call
	if (!ds) { rtk_set_error("%s: NULL scene", who); return RTK_AMD_ERR_BAD_ARG; }
	if (num_queries && (!d_tris || (fill ? (!d_offsets || !d_records) : !d_counts))) {
		rtk_set_error("%s: NULL triangles, %s", who, fill ? "offsets or records" : "counts");
		return RTK_AMD_ERR_BAD_ARG;
	}
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

	NearParams p = {};
	p.queries = d_tris;
	p.max_dist2 = d_max_dist2;
	p.first_prim = filter ? filter->d_first_prim : nullptr;
	p.flags = filter ? filter->flags : 0u;
	p.ids = list ? reinterpret_cast<const unsigned long long *>(list->d_ids) : nullptr;
	p.count = list ? reinterpret_cast<const unsigned long long *>(list->d_count) : nullptr;
	p.counts = d_counts;
	p.offsets = reinterpret_cast<const unsigned long long *>(d_offsets);
	p.records = d_records;
	p.points_query = fill ? d_points_query : nullptr;
	p.points_scene = fill ? d_points_scene : nullptr;
	p.n = (uint32_t)num_queries;
	const int form = (fill ? 1 : 0) | (counted ? 2 : 0);
	const size_t blocks_needed = (num_queries + NR_THREADS - 1u) / NR_THREADS;
	size_t grid = (size_t)(ds->num_cus > 0 ? ds->num_cus : 1) * (size_t)near_blocks_per_cu(ds->device, form);
	if (grid > blocks_needed) grid = blocks_needed;

	// the scratch set of (scene, stream), held until the launch is enqueued; the view and the tree record are read under the
	// same lock a rebuild replaces them under (rtk_launch_closest does the same)
	std::lock_guard<std::mutex> lock(ds->scratch_mutex);
	p.nodes = ds->view.nodes; p.tris = ds->view.tris; p.num_nodes = ds->view.num_nodes; p.num_tris = ds->view.num_tris;
	const size_t entries = ds->tree.stack_entries();
	const size_t spill_cap = entries > NR_LDS_STACK ? entries - NR_LDS_STACK : 0;
	LaunchScratch *sc = ds->scratch.get(stream);
	if (!sc) return RTK_AMD_ERR_OOM;
	if (spill_cap) {
		// (sized in 8-byte entries whatever the form: the area is shared with the other walks of the stream, which hold such entries)
		const int rc = sc->grow_spill(grid * NR_THREADS, spill_cap, sizeof(uint2));
		if (rc != RTK_AMD_OK) return rc;
	}
	p.spill = sc->spill.p;
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
		hipLaunchKernelGGL(near_form(form), dim3((unsigned)grid), dim3(NR_THREADS), 0, stream, p);
		RTK_HIP_CHECK(hipGetLastError(), RTK_AMD_ERR_HIP);
		return RTK_AMD_OK;
	}
	// the counting form: the visit counters start from zero, are brought home and the stream is waited for
	unsigned long long c[8], err = 0;
	RTK_HIP_CHECK(hipMemsetAsync(sc->d_counter, 0, RTK_COUNTER_WORDS * sizeof(unsigned long long), stream), RTK_AMD_ERR_HIP);
	hipLaunchKernelGGL(near_form(form), dim3((unsigned)grid), dim3(NR_THREADS), 0, stream, p);
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
