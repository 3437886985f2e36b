// rtk_within.hip -- rtk_dev_triangles_within_count / rtk_dev_triangles_within_all: for every query point the triangles of a device
// scene nearer than its limit, counted, or listed in ascending (dist2, prim) order into the query's own segment -- all of them or
// the first `room` --, by the rule of rtk_within_rule.h on top of rtk_closest_rule.h. The result is a function of the scene's
// triangle records and the query alone (DESIGN.md "Triangles within a distance"): the tree and the order of the walk only decide
// which records are never looked at.
//
// k_closest's frame (rtk_closest.hip): one query per lane of a 64-wide wave, a fixed grid of resident workgroups that steps through
// the batch, exact 128-byte nodes only (the skip is only as good as the bound), a leaf as its run of DevTri records up to
// RTK_TRI_LAST, the stack [entry][lane] in LDS with the deeper part in the spill area of the (scene, stream) scratch set, a push
// that fits neither dropped WITHOUT advancing and flagged in the stream's launch-error word.
//   the count form (FILL = false)  the bound is static -- a child is entered iff its box bound is below max_dist2 --, so no key
//       travels with a reference (4-byte entries) and the order of the walk is irrelevant: the first admitted child is entered,
//       the others are pushed.
//   the fill form (FILL = true)    (reference, bound) entries as in k_closest: the nearest child is entered, the others are
//       pushed far to near, and a popped entry's bound is looked at again, because the segment may have filled up and its worst
//       entry improved since the push (rtk_within_skip). A candidate goes into the segment through rtk_within_insert, the same
//       function the host driver calls; the lane keeps the segment's last entry (`worst`) in registers, so a triangle that does
//       not get in costs no memory access. A query without room does not walk. Lanes write disjoint segments; a list that names
//       a query twice is the exception, and there the first lane to claim the query (one bit per query in the scratch set,
//       cleared ahead of the launch) answers it and the others leave it alone: the bytes are the same whoever wins.
//
// PER-LANE DRAIN, not the "leaves wait" interleaving of rtk_allhits.hip. That kernel interleaves because its walk is not culled
// and a lane meets many leaves; here a radius far smaller than the scene, or a full segment of k entries, cuts the walk down to
// a few leaves per query as in k_closest (whose cost per query is the yardstick of scripts/within_timing.py), and the wave
// spends its trips in the node branch. The simple form was chosen for that reason and for sharing k_closest's proven frame; the
// interleaved form has not been measured against it.
//
// The on-chip stack: WI_LDS_STACK = 16 entries per lane in both forms. [entry][lane] puts the 64 lanes of a push or pop on
// consecutive words: the 8-byte entries of the fill form are one ds_write_b64 / ds_read_b64 per wave (256 B per 32-lane half: every
// bank once, no conflict), the 4-byte entries of the count form one ds_write_b32 / ds_read_b32. The fill form's 16 * 64 * 8 B * 4
// waves = 32 768 B per workgroup let FIVE workgroups share a CU's 160 KB, which is k_closest's figure and exactly what the fill
// form's registers allow (see WI_RESOURCES): a deeper on-chip part would cost waves, a shallower one would gain none. The count
// form's 16 KB are never the limit. 16 entries are what k_closest's culled walk lives on; a walk that needs more -- a deep,
// lopsided tree, a count with a large radius -- goes to the spill area, and tests/test_gpu_within.py makes one.
//
// FLOATING POINT: the flags of rtk_closest.hip (correctly rounded divide, no contraction); every bit is the rule headers'.
#include "rtk_dev.h"
#include "rtk_within_rule.h"

#include <atomic>
#include <mutex>

// WI_RESOURCES: the compiler's report (gfx950, -O3, -Rpass-analysis=kernel-resource-usage) for each instantiated form
// <FILL, POINTS, COUNT>; scratch 0, no SGPR or VGPR spills and no AGPRs in every one of them:
//                                 VGPRs  SGPRs  LDS per workgroup   waves per SIMD by registers / workgroups per CU by LDS
//   count          <0, 0, 0>       78     70       16 384 B                 6                   /        10
//   fill           <1, 0, 0>       84     84       32 768 B                 5                   /         5
//   fill, points   <1, 1, 0>       80     90       32 768 B                 6 (reported 5: LDS) /         5
//   count, counted <0, 0, 1>       82     70       16 384 B                 5                   /        10
//   fill, counted  <1, 0, 1>       90     88       32 768 B                 5                   /         5
//   fill, points, counted <1,1,1>  86     94       32 768 B                 5                   /         5
// A workgroup is four waves, one per SIMD, so "workgroups per CU" and "waves per SIMD" are the same number. The fill forms sit at
// five either way (512 VGPRs / 88 = 5; 160 KB / 32 KB = 5): registers and LDS agree, which is why the depth is 16 and not more. The
// count form is held by its registers at six (512 / 80); its stack would fit 26 entries before LDS came below that, but one
// depth for both forms keeps rtk_amd_within_stack_entries one number, and its walk is the shallow one when the radius is small.

#define WI_THREADS 256u
#define WI_WAVES (WI_THREADS / 64u)
#define WI_LDS_STACK 16u           // entries per lane held in LDS (4 bytes each in the count form, 8 in the fill form)

namespace {

struct WithinParams {
	const DevNode *nodes;
	const DevTri *tris;
	uint32_t num_nodes;
	uint32_t num_tris;
	const rtk_point_query *queries;
	const unsigned long long *ids;     // or NULL: 0, 1, 2, ...
	const unsigned long long *count;   // or NULL: n
	uint32_t *counts;                  // the count form: one word per query slot; the fill form: d_written or NULL
	const unsigned long long *offsets; // the fill form: n + 1 entries
	rtk_closest_record *records;       // the fill form
	float *points;                     // the fill form, or NULL
	uint32_t *claim;                   // the fill form with ids: one bit per query slot, cleared ahead of the launch; else NULL
	unsigned long long *counter;       // the stream's counter words: [RTK_ERROR_WORD] is set by a dropped push
	void *spill;                       // [entry][lane of the launch], uint32_t or uint2
	uint32_t spill_stride;
	uint32_t spill_cap;                // entries per lane
	uint32_t n;
};

typedef float wi_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t wi_u32x4 __attribute__((ext_vector_type(4)));

// ascending by key; the reference travels with it
__device__ __forceinline__ void wi_cswap(uint32_t &ka, uint32_t &ra, uint32_t &kb, uint32_t &rb)
{
	const bool swap = kb < ka;
	const uint32_t k0 = swap ? kb : ka, k1 = swap ? ka : kb, r0 = swap ? rb : ra, r1 = swap ? ra : rb;
	ka = k0; kb = k1; ra = r0; rb = r1;
}

template <bool FILL> struct WiEntry { typedef uint32_t type; };
template <> struct WiEntry<true> { typedef uint2 type; };

// FILL: the list into the query's segment (else the count); POINTS: d_points is there (FILL only); COUNT: the visit counts of
// rtk_dev_triangles_within_counted, summed per lane and added to the stream's counter words at the end
template <bool FILL, bool POINTS, bool COUNT>
__global__ void __launch_bounds__(WI_THREADS) k_within(WithinParams p)
{
	typedef typename WiEntry<FILL>::type entry_t;
	__shared__ entry_t s_stack[WI_WAVES][WI_LDS_STACK][64];

	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	entry_t (*stk)[64] = s_stack[wave];
	entry_t *const spill = static_cast<entry_t *>(p.spill);
	const uint32_t glane = blockIdx.x * WI_THREADS + threadIdx.x;
	uint32_t m = p.n;
	if (p.count) { const unsigned long long listed = *p.count; m = listed < p.n ? (uint32_t)listed : p.n; }
	const unsigned long long step = (unsigned long long)gridDim.x * WI_THREADS;
	uint32_t c_queries = 0, c_nodes = 0, c_leaves = 0, c_tris = 0, c_hits = 0, c_spills = 0;

	for (unsigned long long i = glane; i < m; i += step) {
		const uint32_t r = p.ids ? (uint32_t)p.ids[i] : (uint32_t)i;
		if (r >= p.n) continue;                                   // (the caller's error; nothing is read or written out of range)
		if (FILL && p.claim) {
			// a query the list names twice is answered once: two lanes must not sort into one segment
			const uint32_t bit = 1u << (r & 31u);
			if (atomicOr(p.claim + (r >> 5), bit) & bit) continue;
		}
		const wi_u32x4 qw = __builtin_nontemporal_load(reinterpret_cast<const wi_u32x4 *>(p.queries + r));
		const float P[3] = { __uint_as_float(qw.x), __uint_as_float(qw.y), __uint_as_float(qw.z) };
		const float max2 = __uint_as_float(qw.w);
		uint32_t kept = 0;                                        // candidates counted, or entries of the segment in use
		uint32_t room = 0;
		rtk_closest_record *seg = nullptr;
		float *seg_points = nullptr;
		rtk_closest_record worst = { 0.0f, 0.0f, 0.0f, 0u };       // the segment's last entry once kept == room
		bool walk = rtk_within_live(P, max2) && p.num_nodes != 0u && p.num_tris != 0u;
		if (FILL) {
			// (offsets that decrease are the caller's error: such a query has no room, nothing is written for it)
			const unsigned long long o0 = p.offsets[r], o1 = p.offsets[(size_t)r + 1u];
			const unsigned long long space = o1 > o0 ? o1 - o0 : 0ull;
			room = space < 0xffffffffull ? (uint32_t)space : 0xffffffffu;
			seg = p.records + o0;
			if (POINTS) seg_points = p.points + o0 * 3ull;
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
					const wi_f32x4 *t = reinterpret_cast<const wi_f32x4 *>(reinterpret_cast<const char *>(p.tris) + (size_t)slot * RTK_TRI_STRIDE);
					const wi_f32x4 A = t[0], B = t[1], C = t[2];
					const float a[3] = { A.x, A.y, A.z }, b[3] = { B.x, B.y, B.z }, c[3] = { C.x, C.y, C.z };
					float q[3], u, v;
					int region;
					const float dist2 = rtk_closest_triangle(P, a, b, c, q, u, v, region);
					if (COUNT) c_tris++;
					if (rtk_within_candidate(dist2, max2)) {
						if (FILL) {
							const rtk_closest_record cand = { dist2, u, v, __float_as_uint(A.w) };
							kept = rtk_within_insert(seg, seg_points, room, kept, cand, q, worst);
						} else kept++;
					}
					if (__float_as_uint(B.w) & RTK_TRI_LAST) break;
					slot++;
				}
				top = RTK_REF_NONE;
			} else if (top < p.num_nodes) {
				// ---------------------------------------------------------------- node: four bounds
				const wi_f32x4 *nd = reinterpret_cast<const wi_f32x4 *>(p.nodes + top);
				const wi_f32x4 xl = nd[0], xh = nd[1], yl = nd[2], yh = nd[3], zl = nd[4], zh = nd[5];
				const wi_u32x4 ch = *reinterpret_cast<const wi_u32x4 *>(nd + 6);
				uint32_t key[4], ref[4];
				if (COUNT) c_nodes++;
#pragma unroll
				for (int k = 0; k < 4; k++) {
					const float lo[3] = { xl[k], yl[k], zl[k] }, hi[3] = { xh[k], yh[k], zh[k] };
					const float bound = rtk_closest_box_bound(P, lo, hi);
					const bool enter = ch[k] != RTK_REF_NONE && !rtk_within_skip(bound, max2, FILL && kept == room, worst.dist2);
					// (bounds are >= +0: their bits order like their values; a NaN bound is entered, first)
					key[k] = enter ? (bound == bound ? __float_as_uint(bound) : 0u) : 0xffffffffu;
					ref[k] = enter ? ch[k] : RTK_REF_NONE;
				}
				if (FILL) {
					// nearest first: the segment fills with near triangles and its worst entry starts to cull
					wi_cswap(key[0], ref[0], key[1], ref[1]);
					wi_cswap(key[2], ref[2], key[3], ref[3]);
					wi_cswap(key[0], ref[0], key[2], ref[2]);
					wi_cswap(key[1], ref[1], key[3], ref[3]);
					wi_cswap(key[1], ref[1], key[2], ref[2]);
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
					if (sp < WI_LDS_STACK) { stk[sp][lane] = e; sp++; }
					else if (sp - WI_LDS_STACK < p.spill_cap) { spill[(size_t)(sp - WI_LDS_STACK) * p.spill_stride + glane] = e; sp++; if (COUNT) c_spills++; }
					else p.counter[RTK_ERROR_WORD] = 1ull;
				}
			} else top = RTK_REF_NONE;                                // (a child word beyond the array: not a tree; nothing is read)
			// ---------------------------------------------------------------- pop; the fill form looks at the bound again
			while (top == RTK_REF_NONE && sp != 0u) {
				--sp;
				const entry_t e = sp < WI_LDS_STACK ? stk[sp][lane] : spill[(size_t)(sp - WI_LDS_STACK) * p.spill_stride + glane];
				if constexpr (FILL) {
					if (!rtk_within_skip(__uint_as_float(e.y), max2, kept == room, worst.dist2)) top = e.x;
				} else top = e;
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

typedef void (*within_kernel_fn)(WithinParams);

// form: fill | points << 1 | counted << 2 (points only with fill)
within_kernel_fn within_form(int form)
{
	switch (form & 7) {
	case 0: case 2: return k_within<false, false, false>;
	case 1: return k_within<true, false, false>;
	case 3: return k_within<true, true, false>;
	case 4: case 6: return k_within<false, false, true>;
	case 5: return k_within<true, false, true>;
	default: return k_within<true, true, true>;
	}
}

// workgroups of a form a CU holds, asked once per device
int within_blocks_per_cu(int device, int form)
{
	static std::atomic<int> known[RTK_MAX_DEVICES][8];
	if (device < 0 || device >= RTK_MAX_DEVICES) return 4;
	int b = known[device][form & 7].load(std::memory_order_relaxed);
	if (b == 0) {
		if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, within_form(form), (int)WI_THREADS, 0) != hipSuccess || b < 1) b = 4;
		known[device][form & 7].store(b, std::memory_order_relaxed);
	}
	return b;
}

} // namespace

extern "C" uint32_t rtk_amd_within_stack_entries(void) { return WI_LDS_STACK; }

// d_offsets == NULL: the count form (d_counts the counts); else the fill form (d_counts the written numbers, or NULL)
int rtk_launch_within(const rtk_dev_scene *ds_c, const rtk_point_query *d_queries, size_t num_queries, const rtk_ray_list *list,
	uint32_t *d_counts, const uint64_t *d_offsets, rtk_closest_record *d_records, float *d_points, bool fill, hipStream_t stream,
	rtk_trace_counters *counted)
{
	rtk_dev_scene *ds = const_cast<rtk_dev_scene *>(ds_c);
	const char *const who = counted ? "rtk_dev_triangles_within_counted" : fill ? "rtk_dev_triangles_within_all" : "rtk_dev_triangles_within_count";
	// everything the host can see is refused here, before any HIP call
	if (!ds) { rtk_set_error("%s: NULL scene", who); return RTK_AMD_ERR_BAD_ARG; }
	if (num_queries && (!d_queries || (fill ? (!d_offsets || !d_records) : !d_counts))) {
		rtk_set_error("%s: NULL queries, %s", who, fill ? "offsets or records" : "counts");
		return RTK_AMD_ERR_BAD_ARG;
	}
	if (list && (list->struct_size < sizeof(rtk_ray_list) || list->flags != 0u || !list->d_count)) {
		rtk_set_error("%s: bad list (struct_size %u, flags %#x, d_count %p)", who, list->struct_size, list->flags, (const void *)list->d_count);
		return RTK_AMD_ERR_BAD_ARG;
	}
	if (num_queries >= ((size_t)1 << 32)) { rtk_set_error("%s: %zu queries: a batch holds fewer than 2^32", who, num_queries); return RTK_AMD_ERR_BAD_ARG; }
	if (counted) *counted = rtk_trace_counters();
	if (num_queries == 0) return RTK_AMD_OK;
	if (!rtk_on_scene_device(ds, who)) return RTK_AMD_ERR_BAD_ARG;

	WithinParams p = {};
	p.queries = d_queries;
	p.ids = list ? reinterpret_cast<const unsigned long long *>(list->d_ids) : nullptr;
	p.count = list ? reinterpret_cast<const unsigned long long *>(list->d_count) : nullptr;
	p.counts = d_counts;
	p.offsets = reinterpret_cast<const unsigned long long *>(d_offsets);
	p.records = d_records;
	p.points = fill ? d_points : nullptr;
	p.n = (uint32_t)num_queries;
	const int form = (fill ? 1 : 0) | (p.points ? 2 : 0) | (counted ? 4 : 0);
	const size_t blocks_needed = (num_queries + WI_THREADS - 1u) / WI_THREADS;
	size_t grid = (size_t)(ds->num_cus > 0 ? ds->num_cus : 1) * (size_t)within_blocks_per_cu(ds->device, form);
	if (grid > blocks_needed) grid = blocks_needed;

	// the scratch set of (scene, stream), held until the launch is enqueued; the view and the tree record are read under the
	// same lock a rebuild replaces them under (rtk_launch_closest does the same)
	std::lock_guard<std::mutex> lock(ds->scratch_mutex);
	p.nodes = ds->view.nodes; p.tris = ds->view.tris; p.num_nodes = ds->view.num_nodes; p.num_tris = ds->view.num_tris;
	const size_t entries = ds->tree.stack_entries();
	const size_t spill_cap = entries > WI_LDS_STACK ? entries - WI_LDS_STACK : 0;
	LaunchScratch *sc = ds->scratch.get(stream);
	if (!sc) return RTK_AMD_ERR_OOM;
	if (spill_cap) {
		// (sized in 8-byte entries whatever the form: the area is shared with the other walks of the stream, which hold such entries)
		const int rc = sc->grow_spill(grid * WI_THREADS, spill_cap, sizeof(uint2));
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
		hipLaunchKernelGGL(within_form(form), dim3((unsigned)grid), dim3(WI_THREADS), 0, stream, p);
		RTK_HIP_CHECK(hipGetLastError(), RTK_AMD_ERR_HIP);
		return RTK_AMD_OK;
	}
	// the counting form: the visit counters start from zero, are brought home and the stream is waited for
	unsigned long long c[8], err = 0;
	RTK_HIP_CHECK(hipMemsetAsync(sc->d_counter, 0, RTK_COUNTER_WORDS * sizeof(unsigned long long), stream), RTK_AMD_ERR_HIP);
	hipLaunchKernelGGL(within_form(form), dim3((unsigned)grid), dim3(WI_THREADS), 0, stream, p);
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
