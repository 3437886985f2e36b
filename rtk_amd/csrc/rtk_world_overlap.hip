// rtk_world_overlap.hip -- rtk_dev_world_triangles_in_box_* / _in_obb_* / _touching_*: for every query box, oriented box or
// triangle the triangles of all live instances of a world that touch it, counted, or listed as 64-bit entries
// (instance << 32 | prim) in ascending order into the query's own segment -- all of them or the first `room` --, by the rule of
// rtk_world_overlap_rule.h. The answer has the bits the scene call gives on the flat placed twin
// (rtk_dev_scene_build_placed of the same meshes under the same placements), for any affine placement; it is a function of the
// instances' records, the placements, the filter and the query alone: neither tree decides more than which records are never
// looked at.
//
// THE WALK, k_world_overlap<Shape, FILL, COUNT, FILT>: k_world_closest's frame (rtk_world_closest.hip) -- one query per lane, a
// fixed grid of resident workgroups striding over the batch, per-lane 64-bit node and record pointers, 8-byte stack entries,
// WD_LDS_STACK per lane in LDS as [entry][lane], deeper ones in the spill area of the (top tree, stream) scratch set, a push that
// fits neither dropped without advancing sp and flagged in that set's error word, the WD_REF_TOP sentinel (with the next proxy
// slot of the leaf, or none) to come back from an instance to the rest of a top leaf, the 12 floats of the instance's FORWARD
// placement loaded on entering it, the query never transformed -- with k_overlap_walk's body (rtk_overlap_walk.h): the Shape's
// skip is static, so nothing is looked at again at the pop and the order of the walk is irrelevant; the first admitted child is
// entered, the others are pushed (their second word is not used); a leaf is its run of records up to RTK_TRI_LAST; the count
// form counts, the fill form inserts the candidate's key into the query's own segment through rtk_world_overlap_insert with
// `worst` in a register; a query without room does not walk; a list that names a query twice is answered once, through the claim
// bits of the scratch set, cleared ahead of the launch.
//   Top level: the exact 128-byte nodes of the top tree and the proxies' boxes (lo from v0, hi from v1, the instance from prim)
// through the Shape's skip AS THEY ARE: no margin (rtk_world_overlap_rule.h point 2). A proxy
// that is not skipped, whose instance is live and passes the filter, enters the instance.
//   In an instance: every child's box goes through rtk_world_placed_box (six rows) before the Shape's skip, every record's
// vertices through rtk_world_overlap_place before the Shape's candidate.
// The Shapes are the scene walks' own: rtk_box_shape.h, rtk_obb_shape.h, rtk_touch_shape.h (the touching calls of a world carry
// the flags alone: first_prim is 0 for every query).
//
// FLOATING POINT: only the rule headers' routines decide a bit (__fmul_rn / __fadd_rn through their macros); -ffp-contract=off
// like every traversal.
// Compiler's resource report (gfx950, -O3, kernel-resource-usage): WO_RESOURCES below.
#include "rtk_world_internal.h"
#include "rtk_world_overlap_rule.h"
#include "rtk_box_shape.h"
#include "rtk_obb_shape.h"
#include "rtk_touch_shape.h"

#include <atomic>

// WO_RESOURCES: the compiler's report (gfx950, -O3, -Rpass-analysis=kernel-resource-usage) for each instantiated form
// <FILL, COUNT, FILT>; scratch 0, no VGPR spills and no AGPRs in every one of them; LDS 32 768 B per workgroup in every one
// (five workgroups of four waves on a CU by LDS). VGPRs, and in brackets the SGPRs that went to lanes of a VGPR (counted in the
// VGPR column), not to memory; then the waves per SIMD the registers allow:
//                              box            oriented box     triangle
//   count          <0, 0, 0>   122 (0)   4    146 (4)    3     239 (22)   2
//   fill           <1, 0, 0>   130 (2)   3    156 (14)   3     246 (38)   2
//   count, filter  <0, 0, 1>   122 (0)   4    147 (14)   3     240 (30)   2
//   fill, filter   <1, 0, 1>   131 (10)  3    156 (24)   3     247 (42)   2
//   count, counted <0, 1, 1>   129 (2)   3    154 (16)   3     248 (32)   2
//   fill, counted  <1, 1, 1>   137 (14)  3    162 (30)   3     254 (46)   2
// Against the scene walks (BX_ / OB_ / TC_RESOURCES) a world's lane carries the 12 floats of the placement, two 64-bit base
// pointers with their counts, the instance and the 64-bit `worst`, and the six rows of a placed box are live across a node's four
// children: 46 to 60 VGPRs more. The registers decide the occupancy in every form. Not tuned.
// SKIP: the walk spells rtk_world_overlap_skip (rtk_world_overlap_rule.h point 2) out as rtk_world_placed_box followed by the
// Shape's skip, which for all three shapes is rtk_box_skip against the query's bounds: the same comparisons on the same floats.
// Calling the rule's function with the bounds handed over as pointers was built and measured: 6 to 8 VGPRs more in most forms
// and the box fill 11 % slower on the device (950 ms against 852 ms, profiles/world_overlap_timing.log), so this form stays;
// tests/test_gpu_world_overlap.py holds the walk to the brute force that has no skip at all.

namespace {

template <class Shape>
struct WorldOverlapParams {
	const DevNode *top_nodes;
	const DevTri *top_tris;
	uint32_t top_num_nodes, top_num_tris;
	const DevWorldInstance *inst;
	const DevWorldScene *scenes;
	const rtk_placement *place;            // the forward placements, as last given
	uint32_t num_instances, num_scenes;
	uint32_t n;
	const typename Shape::Query *queries;
	const unsigned long long *ids;         // or NULL: 0, 1, 2, ...
	const unsigned long long *count;       // or NULL: n
	uint32_t *counts;                      // the count form: one word per query slot; the fill form: d_written or NULL
	const unsigned long long *offsets;     // the fill form: n + 1 entries
	uint64_t *entries;                     // the fill form
	uint32_t *claim;                       // the fill form with ids: one bit per query slot, cleared ahead of the launch; else NULL
	const uint32_t *mask;                  // or NULL: bit i set = instance i is walked
	uint32_t mask_bits;
	const uint32_t *ignore_instance;       // or NULL: per query slot
	unsigned long long *counter;           // the stream's counter words: [RTK_ERROR_WORD] is set by a dropped push
	uint2 *spill;                          // [entry][lane of the launch]
	uint32_t spill_stride;
	uint32_t spill_cap;                    // entries per lane
	typename Shape::Extra extra;           // the shape's own, per launch
};

typedef float wo_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t wo_u32x4 __attribute__((ext_vector_type(4)));

// FILL: the list into the query's segment (else the count); COUNT: the visit counts of the _counted entry points; FILT: the
// instance mask and the per-query ignored instance
template <class Shape, bool FILL, bool COUNT, bool FILT>
__global__ void __launch_bounds__(WD_THREADS) k_world_overlap(WorldOverlapParams<Shape> p)
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
		const uint32_t skip_inst = (FILT && p.ignore_instance) ? p.ignore_instance[r] : RTK_PRIM_NONE;
		uint32_t kept = 0;                                        // candidates counted, or entries of the segment in use
		uint32_t room = 0;
		uint64_t *seg = nullptr;
		uint64_t worst = 0ull;                                    // the segment's last entry once kept == room
		bool walk = live && p.top_num_nodes != 0u && p.top_num_tris != 0u;
		if (FILL) {
			// (offsets that decrease are the caller's error: such a query has no room, nothing is written for it)
			const unsigned long long o0 = p.offsets[r], o1 = p.offsets[(size_t)r + 1u];
			const unsigned long long space = o1 > o0 ? o1 - o0 : 0ull;
			room = space < 0xffffffffull ? (uint32_t)space : 0xffffffffu;
			seg = p.entries + o0;
			walk = walk && room != 0u;                            // nothing can be kept: no walk
		}
		// where the walk is: the top tree (in_inst false), or the scene of instance cur_inst under placement pm
		bool in_inst = false;
		uint32_t cur_inst = RTK_PRIM_NONE;
		float pm[12];
#pragma unroll
		for (int k = 0; k < 12; k++) pm[k] = 0.0f;
		const char *nodes = reinterpret_cast<const char *>(p.top_nodes), *tris = reinterpret_cast<const char *>(p.top_tris);
		uint32_t num_nodes = p.top_num_nodes, num_tris = p.top_num_tris;
		uint32_t top = walk ? 0u : RTK_REF_NONE;
		uint32_t sp = 0;
		if (COUNT) c_queries++;

		while (top != RTK_REF_NONE) {
			if ((int32_t)top >= 0) {
				// ------------------------------------------------------------ node, of the top tree or of a scene: four boxes
				if (top < num_nodes) {
					const wo_f32x4 *nd = reinterpret_cast<const wo_f32x4 *>(nodes + (size_t)top * 128u);
					const wo_f32x4 xl = nd[0], xh = nd[1], yl = nd[2], yh = nd[3], zl = nd[4], zh = nd[5];
					const wo_u32x4 ch = *reinterpret_cast<const wo_u32x4 *>(nd + 6);
					uint32_t ref[4];
					if (COUNT) c_nodes++;
#pragma unroll
					for (int k = 0; k < 4; k++) {
						const float lo[3] = { xl[k], yl[k], zl[k] }, hi[3] = { xh[k], yh[k], zh[k] };
						// rtk_world_overlap_skip, spelled out (SKIP below says why)
						bool skip;
						if (in_inst) {
							// a scene's box is local: its exact world bounds under the instance's placement, then the shape's skip
							float wlo[3], whi[3];
							rtk_world_placed_box(pm, lo, hi, wlo, whi);
							skip = Shape::skip(Q, wlo, whi);
						} else skip = Shape::skip(Q, lo, hi);             // the top tree's boxes as they are: no margin
						ref[k] = ch[k] != RTK_REF_NONE && !skip ? ch[k] : RTK_REF_NONE;
					}
					// any order gives the same result: the first admitted slot is entered
					top = RTK_REF_NONE;
#pragma unroll
					for (int k = 0; k < 4; k++) {
						if (top == RTK_REF_NONE && ref[k] != RTK_REF_NONE) { top = ref[k]; ref[k] = RTK_REF_NONE; }
					}
					// the others
#pragma unroll
					for (int k = 3; k >= 0; k--) {
						if (ref[k] == RTK_REF_NONE) continue;
						const uint2 en = make_uint2(ref[k], 0u);
						WD_PUSH(en);
					}
				} else top = RTK_REF_NONE;                            // (a child word beyond the array: not a tree; nothing is read)
			} else if (!in_inst) {
				// ------------------------------------------------------------ a leaf of the top tree: proxies up to RTK_TRI_LAST
				uint32_t slot = top & 0x7fffffffu;
				if (COUNT) c_leaves++;
				top = RTK_REF_NONE;
				while (slot < num_tris) {
					const wo_f32x4 *t = reinterpret_cast<const wo_f32x4 *>(tris + (size_t)slot * RTK_TRI_STRIDE);
					const wo_f32x4 A = t[0], B = t[1];
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
						wanted = !Shape::skip(Q, lo, hi);
					}
					if (wanted) {
						const wo_u32x4 i3 = reinterpret_cast<const wo_u32x4 *>(p.inst + inst)[3];
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
									const wo_f32x4 *pr = reinterpret_cast<const wo_f32x4 *>(p.place + inst);
									const wo_f32x4 m0 = pr[0], m1 = pr[1], m2 = pr[2];
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
					const wo_f32x4 *t = reinterpret_cast<const wo_f32x4 *>(tris + (size_t)slot * RTK_TRI_STRIDE);
					const wo_f32x4 A = t[0], B = t[1], C = t[2];
					const float a[3] = { A.x, A.y, A.z }, b[3] = { B.x, B.y, B.z }, c[3] = { C.x, C.y, C.z };
					float v0[3], v1[3], v2[3];
					rtk_world_overlap_place(pm, a, b, c, v0, v1, v2);
					const uint32_t prim = __float_as_uint(A.w);
					if (COUNT) c_tris++;
					if (Shape::candidate(Q, v0, v1, v2, prim)) {
						if (FILL) kept = rtk_world_overlap_insert(seg, room, kept, rtk_world_overlap_key(cur_inst, prim), worst);
						else kept++;
					}
					if (__float_as_uint(B.w) & RTK_TRI_LAST) break;
					slot++;
				}
				top = RTK_REF_NONE;
			}
			// ---------------------------------------------------------------- pop: nothing is looked at again
			while (top == RTK_REF_NONE && sp != 0u) {
				--sp;
				const uint2 en = sp < WD_LDS_STACK ? stk[sp][lane] : p.spill[(size_t)(sp - WD_LDS_STACK) * p.spill_stride + glane];
				if (en.x == WD_REF_TOP) {
					// back in the top tree, at the rest of the leaf the instance was entered from
					in_inst = false; cur_inst = RTK_PRIM_NONE;
					nodes = reinterpret_cast<const char *>(p.top_nodes); tris = reinterpret_cast<const char *>(p.top_tris);
					num_nodes = p.top_num_nodes; num_tris = p.top_num_tris;
					if (en.y != RTK_REF_NONE) top = RTK_REF_LEAF | en.y;
				} else top = en.x;
			}
		}

		if (COUNT && kept != 0u) c_hits++;
		if (p.counts) __builtin_nontemporal_store(kept, p.counts + r);
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

// form: fill | filtered << 1; the counting forms are always the filtered ones
template <class Shape>
void (*world_overlap_form(int form, bool counted))(WorldOverlapParams<Shape>)
{
	if (counted) return (form & 1) ? k_world_overlap<Shape, true, true, true> : k_world_overlap<Shape, false, true, true>;
	switch (form & 3) {
	case 0: return k_world_overlap<Shape, false, false, false>;
	case 1: return k_world_overlap<Shape, true, false, false>;
	case 2: return k_world_overlap<Shape, false, false, true>;
	default: return k_world_overlap<Shape, true, false, true>;
	}
}

// workgroups of a shape's form a CU holds, asked once per device. The plain form is asked, and a _counted launch is sized by it
// too, as the other walks of a world are: the counting kernels need a few more registers (WO_RESOURCES), so such a launch may
// hold more workgroups than are resident at once. That costs nothing but order: no lane waits for another, and the spill area
// is sized by the grid that is launched, not by what is resident
template <class Shape>
int world_overlap_blocks_per_cu(int device, int form)
{
	static std::atomic<int> known[RTK_MAX_DEVICES][4];
	if (device < 0 || device >= RTK_MAX_DEVICES) return 2;
	int b = known[device][form & 3].load(std::memory_order_relaxed);
	if (b == 0) {
		if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, world_overlap_form<Shape>(form, false), (int)WD_THREADS, 0) != hipSuccess || b < 1) b = 2;
		known[device][form & 3].store(b, std::memory_order_relaxed);
	}
	return b;
}

// the entry points' names, for the error texts (the queries' noun is the Shape's)
template <class Shape> struct WorldOverlapNames;
template <> struct WorldOverlapNames<Box> {
	static constexpr const char *COUNT = "rtk_dev_world_triangles_in_box_count", *ALL = "rtk_dev_world_triangles_in_box_all",
		*COUNTED = "rtk_dev_world_triangles_in_box_counted";
};
template <> struct WorldOverlapNames<Obb> {
	static constexpr const char *COUNT = "rtk_dev_world_triangles_in_obb_count", *ALL = "rtk_dev_world_triangles_in_obb_all",
		*COUNTED = "rtk_dev_world_triangles_in_obb_counted";
};
template <> struct WorldOverlapNames<Touch> {
	static constexpr const char *COUNT = "rtk_dev_world_triangles_touching_count", *ALL = "rtk_dev_world_triangles_touching_all",
		*COUNTED = "rtk_dev_world_triangles_touching_counted";
};

// !fill: the count form (d_counts the counts); else the fill form (d_counts the written numbers, or NULL). A non-null `counted`
// makes it the counting form of either. `extra` is the shape's own (the touching calls' flags)
template <class Shape>
int world_overlap_launch(const rtk_dev_world *w_c, const typename Shape::Query *d_queries, size_t n, const rtk_ray_list *list,
	const rtk_world_filter *filter, const typename Shape::Extra &extra, uint32_t *d_counts, const uint64_t *d_offsets, uint64_t *d_entries,
	bool fill, hipStream_t stream, rtk_trace_counters *counted, const char *who)
{
	rtk_dev_world *w = const_cast<rtk_dev_world *>(w_c);
	if (counted) *counted = rtk_trace_counters();
	if (n == 0) return RTK_AMD_OK;
	if (!rtk_on_scene_device(w->top, who)) return RTK_AMD_ERR_BAD_ARG;

	WorldOverlapParams<Shape> p = {};
	p.queries = d_queries;
	p.n = (uint32_t)n;
	p.ids = list ? reinterpret_cast<const unsigned long long *>(list->d_ids) : nullptr;
	p.count = list ? reinterpret_cast<const unsigned long long *>(list->d_count) : nullptr;
	p.counts = d_counts;
	p.offsets = reinterpret_cast<const unsigned long long *>(d_offsets);
	p.entries = d_entries;
	p.place = w->d_place;
	p.extra = extra;
	const bool filtered = filter && (filter->d_instance_mask || filter->d_ignore_instance);
	if (filtered) { p.mask = filter->d_instance_mask; p.mask_bits = filter->instance_mask_bits; p.ignore_instance = filter->d_ignore_instance; }
	const int form = (fill ? 1 : 0) | (filtered ? 2 : 0);
	const bool claims = fill && p.ids;
	return rtk_world_launch(w, n, stream, world_overlap_blocks_per_cu<Shape>(w->device, form), world_overlap_form<Shape>(form, false),
		world_overlap_form<Shape>(form, true), p, [](const rtk_dev_scene *, WorldOverlapParams<Shape> &) {},
		[claims, n](LaunchScratch *sc, hipStream_t s, WorldOverlapParams<Shape> &q) {
			if (!claims) return (int)RTK_AMD_OK;
			// one bit per query slot, in the area rtk_dev_select_rays keeps its masks in: launches of one stream are ordered
			const size_t claim_bytes = ((n + 31u) / 32u) * sizeof(uint32_t);
			const int rc = sc->grow(sc->select, claim_bytes, claim_bytes);
			if (rc != RTK_AMD_OK) return rc;
			q.claim = sc->select.as<uint32_t>();
			RTK_HIP_CHECK(hipMemsetAsync(q.claim, 0, claim_bytes, s), (int)RTK_AMD_ERR_HIP);
			return (int)RTK_AMD_OK;
		}, counted, who);
}

// everything the host can see is refused here, before any HIP call: rtk_world_refuse's, then the shape's
template <class Shape>
int world_overlap_refuse(const char *who, const rtk_dev_world *w, const void *d_queries, size_t n, const rtk_ray_list *list, const rtk_world_filter *filter,
	const uint32_t *d_counts, const uint64_t *d_offsets, const uint64_t *d_entries, bool fill)
{
	return rtk_world_refuse(who, Shape::NOUN, w, n, d_queries && (fill ? (d_offsets && d_entries) : d_counts != nullptr), list, filter);
}

template <class Shape>
const char *world_overlap_who(bool fill, const rtk_trace_counters *counted)
{
	return counted ? WorldOverlapNames<Shape>::COUNTED : fill ? WorldOverlapNames<Shape>::ALL : WorldOverlapNames<Shape>::COUNT;
}

} // namespace

extern "C" uint32_t rtk_amd_world_overlap_stack_entries(void) { return WD_LDS_STACK; }

int rtk_launch_world_box(const rtk_dev_world *w, const rtk_box_query *d_boxes, size_t n, const rtk_ray_list *list, const rtk_world_filter *filter,
	uint32_t *d_counts, const uint64_t *d_offsets, uint64_t *d_entries, bool fill, hipStream_t stream, rtk_trace_counters *counted)
{
	const char *who = world_overlap_who<Box>(fill, counted);
	const int refused = world_overlap_refuse<Box>(who, w, d_boxes, n, list, filter, d_counts, d_offsets, d_entries, fill);
	if (refused != RTK_AMD_OK) return refused;
	return world_overlap_launch<Box>(w, d_boxes, n, list, filter, Box::Extra(), d_counts, d_offsets, d_entries, fill, stream, counted, who);
}

int rtk_launch_world_obb(const rtk_dev_world *w, const rtk_obb_query *d_obbs, size_t n, const rtk_ray_list *list, const rtk_world_filter *filter,
	uint32_t *d_counts, const uint64_t *d_offsets, uint64_t *d_entries, bool fill, hipStream_t stream, rtk_trace_counters *counted)
{
	const char *who = world_overlap_who<Obb>(fill, counted);
	const int refused = world_overlap_refuse<Obb>(who, w, d_obbs, n, list, filter, d_counts, d_offsets, d_entries, fill);
	if (refused != RTK_AMD_OK) return refused;
	return world_overlap_launch<Obb>(w, d_obbs, n, list, filter, Obb::Extra(), d_counts, d_offsets, d_entries, fill, stream, counted, who);
}

int rtk_launch_world_touch(const rtk_dev_world *w, const rtk_tri_query *d_tris, size_t n, const rtk_ray_list *list, const rtk_world_filter *filter,
	uint32_t touch_flags, uint32_t *d_counts, const uint64_t *d_offsets, uint64_t *d_entries, bool fill, hipStream_t stream, rtk_trace_counters *counted)
{
	const char *who = world_overlap_who<Touch>(fill, counted);
	const int refused = world_overlap_refuse<Touch>(who, w, d_tris, n, list, filter, d_counts, d_offsets, d_entries, fill);
	if (refused != RTK_AMD_OK) return refused;
	if ((touch_flags & ~(uint32_t)RTK_TOUCH_SKIP_SHARED_VERTEX) != 0u) {
		rtk_set_error("%s: bad touch_flags %#x (an unknown bit)", who, touch_flags);
		return RTK_AMD_ERR_BAD_ARG;
	}
	Touch::Extra x;
	x.first_prim = nullptr;                // (no first_prim on a world: d_ignore_instance leaves a body's own triangles out)
	x.flags = touch_flags;
	return world_overlap_launch<Touch>(w, d_tris, n, list, filter, x, d_counts, d_offsets, d_entries, fill, stream, counted, who);
}
