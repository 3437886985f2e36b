// rtk_allhits.hip -- rtk_dev_trace_rays_count / rtk_dev_trace_rays_all: EVERY candidate of a ray, counted or listed, in one walk.
//
// What it computes (include/rtk_amd.h, "Every hit along a ray"): a candidate is a triangle of a leaf the walk enters that rtk's
// watertight test accepts inside (min_t, max_t) and every filter lets through; a child is entered if its slot is not empty and
// the slab test of the exact 128-byte node passes with the far bound at the ray's max_t. That set is a function of the scene's
// bits and the ray, not of the order of the walk, so nothing is sorted and no entry distance is kept: every admitted child but
// one is pushed, the walk continues into the one that is left (the first admitted slot). The arithmetic is rtk_trace.hip's, copied
// operation for operation: ray_setup, the exact-node slab test in both forms (v_max3 / v_min3 for ordinary rays, the SSE
// operand order for special ones), the triangle test with the group-of-four rule as MODE 2 states it (a partial last group in
// double; a full group scanned for an exact zero, then evaluated: a count or a written record cannot be undone).
// Exact nodes only: the compressed ones admit a superset of boxes, and the set would depend on the node format.
//
// How it runs: rtk_trace_kernel's frame. One ray per lane, persistent waves that take 64-ray chunks from the RTK_QUEUES queue
// heads and refill idle lanes by ballot rank; LEAVES WAIT, node steps first (node_exit), the interleaved form of
// rtk_trace_kernel and not k_closest's per-lane drain. Why: a lane's walk here is long and its leaves are many (nothing is
// culled: 28 candidates per incoherent ray of the 1M-triangle scene, profiles/allhits_timing.log), and in the per-lane form
// a wave runs the node branch and the leaf branch one after the other on EVERY trip while any two lanes disagree -- divergent
// branches serialise across the exec mask --, each with the lanes of the other switched off. Letting leaves wait fills the node steps -- one 128-byte request per lane and a wait, the longest
// latency of the loop -- with up to 64 lanes and the triangle loop with every lane that has a leaf. k_closest can afford the
// simple form because its bound shrinks fast and a query sees few leaves.
//
// The stack holds child references only (4 bytes, no key): AH_LDS_STACK = 30 entries per lane in LDS, [entry][lane], one
// conflict-free ds_write_b32 / ds_read_b32 per push or pop; 30 * 64 * 4 B * 4 waves = 30 720 B per workgroup, so FIVE workgroups
// share a CU's 160 KB as for rtk_trace_kernel, with twice its depth on chip -- this walk pushes every admitted child and runs
// deeper than a culled one. Deeper entries go to the spill area of the (scene, stream) scratch set, sized from the tree's
// stack_entries; a push that fits neither is dropped WITHOUT advancing and sets the launch-error word (RTK_PUSH's rule).
// Compiler's resource report (gfx950, -O3, kernel-resource-usage): see AH_RESOURCES below.
//
// FLOATING POINT: compiled with -ffp-contract=off like rtk_trace.hip; the operation order of the triangle test is normative.
#include "rtk_dev.h"
#include "rtk_trace_shared.h"

#include <math.h>

#include <mutex>

#include "rtk_trace_lane.h"

// AH_RESOURCES (count / count FILT / fill / fill FILT): VGPRs 84 / 86 / 86 / 89, scratch 0, no VGPR spills (the filtered fill form
// spills 8 SGPRs into a VGPR), LDS 30 720 B per workgroup, occupancy 5 waves per SIMD: LDS places five workgroups of four waves on
// a CU, 20 waves = 5 per SIMD, which is the launch bound (102 VGPRs would still fit it), so LDS and registers agree.

#define AH_PUSH(e_)                                                                                       \
	do {                                                                                                  \
		if (sp < AH_LDS_STACK) { stk[sp][lane] = (e_); sp++; }                                            \
		else if (sp - AH_LDS_STACK < p.spill_cap) {                                                       \
			p.spill[(size_t)(sp - AH_LDS_STACK) * p.spill_stride + glane] = (e_); sp++;                   \
		} else p.counter[RTK_ERROR_WORD] = 1ull;                                                          \
	} while (0)

// (always an LDS read; the spilled entry is read once, past the caches)
#define AH_POP()                                                                                          \
	do {                                                                                                  \
		if (sp == 0u) top = RTK_REF_NONE;                                                                 \
		else {                                                                                            \
			--sp;                                                                                         \
			uint32_t e_ = stk[sp < AH_LDS_STACK ? sp : AH_LDS_STACK - 1u][lane];                          \
			if (sp >= AH_LDS_STACK) e_ = __builtin_nontemporal_load(p.spill + (size_t)(sp - AH_LDS_STACK) * p.spill_stride + glane); \
			top = e_;                                                                                     \
		}                                                                                                 \
	} while (0)

#define AH_IS_LEAF(top_) ((top_) != RTK_REF_NONE && (int32_t)(top_) < 0)

template <bool FILL /*false: count; true: the closest candidates into the ray's segment*/, bool FILT /*built-in candidate filters*/>
__global__ void __launch_bounds__(BLOCK_THREADS, 5) rtk_allhits_kernel(AllHitsParams p)
{
	__shared__ uint32_t s_stack[WAVES_PER_BLOCK][AH_LDS_STACK][64];

	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t wave = threadIdx.x >> 6;
	uint32_t (*stk)[64] = s_stack[wave];
	const uint32_t glane = blockIdx.x * BLOCK_THREADS + threadIdx.x;
	const char *const nodes = reinterpret_cast<const char *>(p.nodes);
	const char *const tris = reinterpret_cast<const char *>(p.tris);

	// wave-uniform ray range owned by this wave (rtk_trace_kernel's deal: static for one workgroup, else the queue heads)
	unsigned long long w_next, w_end;
	bool pool_empty;
	uint32_t queue = blockIdx.x % RTK_QUEUES, queues_left = RTK_QUEUES;
	if (p.dynamic) {
		w_next = w_end = 0;
		pool_empty = false;
	} else {
		w_next = ((unsigned long long)blockIdx.x * WAVES_PER_BLOCK + wave) * 64ull;
		w_end = w_next + 64ull < p.n ? w_next + 64ull : p.n;
		if (w_next > p.n) w_next = p.n;
		pool_empty = true;
	}

	// per-lane ray state
	bool active = false;
	uint32_t ray_index = 0;
	float ox = 0, oy = 0, oz = 0, rdx = 0, rdy = 0, rdz = 0, tmin_ray = 0, tmax_ray = 0;
	float sox = 0, soy = 0, soz = 0, shx = 0, shy = 0, shz = 0;
	bool kz0 = false, kz1 = false;
	uint32_t onx = 0, ony = 0, onz = 0;     // byte offset of the NEAR plane row of each axis inside a node; far = the other row
	float far_t = 0;                        // the slab test's far bound: the ray's max_t, for the whole walk
	uint32_t cand_n = 0;                    // candidates counted, or records kept (<= room)
	rtk_hit_record *list = nullptr;         // FILL: the ray's segment ...
	uint32_t room = 0;                      // ... and its size
	float after_t = 0;
	uint32_t after_prim = 0, skip_prim = RTK_PRIM_NONE;
	bool has_after = false;
	uint32_t top = RTK_REF_NONE;
	uint32_t sp = 0;
	bool special = false;                   // slab products can be NaN (0 * inf) or the inputs are not finite: the SSE operand order matters
	bool wave_fast = true;                  // wave-uniform: no active lane is special

	for (;;) {
		// ---------------------------------------------------------------- refill
		const unsigned long long idle = __builtin_amdgcn_ballot_w64(!active);
		const uint32_t n_idle = (uint32_t)__popcll(idle);
		if (n_idle == 64u || (n_idle >= p.refill_min && !(pool_empty && w_next >= w_end))) {
			if (w_next >= w_end && !pool_empty) {
				const unsigned long long num_chunks = ((unsigned long long)p.n + 63ull) >> 6;
				pool_empty = true;
				while (queues_left) {
					unsigned long long got = 0;
					if (lane == 0) got = atomicAdd(p.counter + RTK_QUEUE_WORD(queue), 1ull);
					got = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(got >> 32)) << 32) |
						(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)got);
					const unsigned long long chunk = got * RTK_QUEUES + queue;
					if (chunk < num_chunks) {
						w_next = chunk << 6;
						w_end = w_next + 64ull < p.n ? w_next + 64ull : p.n;
						pool_empty = false;
						break;
					}
					queue = (queue + 1u) % RTK_QUEUES;
					queues_left--;
				}
			}
			const unsigned long long avail = w_end - w_next;
			if (avail) {
				const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32),
					__builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
				const uint32_t take = n_idle < avail ? n_idle : (uint32_t)avail;
				if (!active && rank < take) {
					ray_index = (uint32_t)(w_next + rank);
					const float4 r0 = ld_f4_stream(reinterpret_cast<const char *>(p.rays + ray_index));
					const float4 r1 = ld_f4_stream(reinterpret_cast<const char *>(p.rays + ray_index) + 16);
					ox = r0.x; oy = r0.y; oz = r0.z;
					const float dx = r0.w, dy = r1.x, dz = r1.y;
					tmin_ray = r1.z; tmax_ray = r1.w;
					// rtk.c:550-566
					const float ax = fabsf(dx), ay = fabsf(dy), az = fabsf(dz);
					const float m = sse_max(sse_max(ax, ay), az);
					kz0 = ax == m;
					kz1 = !kz0 && ay == m;
					const float dkx = kz0 ? dy : (kz1 ? dz : dx);
					const float dky = kz0 ? dz : (kz1 ? dx : dy);
					const float dkz = kz0 ? dx : (kz1 ? dy : dz);
					shx = -dkx / dkz;
					shy = -dky / dkz;
					sox = kz0 ? oy : (kz1 ? oz : ox);
					soy = kz0 ? oz : (kz1 ? ox : oy);
					soz = kz0 ? ox : (kz1 ? oy : oz);
					// rtk.c:410: true divides
					rdx = 1.0f / dx; rdy = 1.0f / dy; rdz = 1.0f / dz;
					shz = kz0 ? rdx : (kz1 ? rdy : rdz);
					// near/far plane offsets inside the node by direction sign BIT (rtk.c:152-154, 458-463)
					const uint32_t sx = __float_as_uint(dx) >> 31, sy = __float_as_uint(dy) >> 31, sz = __float_as_uint(dz) >> 31;
					onx = sx * 16u;
					ony = 32u + sy * 16u;
					onz = 64u + sz * 16u;
					special = !(isfinite(rdx) && isfinite(rdy) && isfinite(rdz) && rdx != 0.0f && rdy != 0.0f && rdz != 0.0f &&
						isfinite(ox) && isfinite(oy) && isfinite(oz) && tmin_ray == tmin_ray && tmax_ray == tmax_ray);
					far_t = tmax_ray;
					if (FILT) {
						has_after = p.after != nullptr;
						if (has_after) { const rtk_hit_record a = p.after[ray_index]; after_t = a.t; after_prim = a.prim; has_after = a.prim != RTK_PRIM_NONE; }
						skip_prim = p.ignore_prim ? p.ignore_prim[ray_index] : RTK_PRIM_NONE;
					}
					top = p.num_nodes != 0u ? 0u : RTK_REF_NONE;  // root node
					if (FILL) {
						// (offsets that decrease are the caller's error: such a ray has no room, nothing is written for it)
						const unsigned long long o0 = p.offsets[ray_index], o1 = p.offsets[(size_t)ray_index + 1u];
						const unsigned long long r = o1 > o0 ? o1 - o0 : 0ull;
						room = r < 0xffffffffull ? (uint32_t)r : 0xffffffffu;
						list = p.records + o0;
						if (room == 0u) top = RTK_REF_NONE;       // nothing can be kept: no walk
					}
					sp = 0u;
					cand_n = 0u;
					active = true;
				}
				w_next += take;
			}
			wave_fast = __builtin_amdgcn_ballot_w64(active && special) == 0ull;
			if (__builtin_amdgcn_ballot_w64(active) == 0ull) {
				if (pool_empty && w_next >= w_end) break;
				continue;
			}
		}

		const unsigned long long m_act_ = __builtin_amdgcn_ballot_w64(active);
		const unsigned long long m_active = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(m_act_ >> 32)) << 32) |
			(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)m_act_);
		// ---------------------------------------------------------------- inner nodes
		for (;;) {
			// lanes that reached a leaf wait here for the others; when only a few still descend and leaves are waiting, the leaves go first
			const unsigned long long m_node = __builtin_amdgcn_ballot_w64((int32_t)top >= 0) & m_active;
			const bool want_node = __builtin_amdgcn_inverse_ballot_w64(m_node);
			if (m_node == 0ull) break;
			if ((uint32_t)__popcll(m_node) < p.node_exit && (__builtin_amdgcn_ballot_w64(AH_IS_LEAF(top)) & m_active) != 0ull) break;
			if (!want_node) continue;
			const uint32_t a_node = top << 7;
			f32x4 nx, fx, ny, fy, nz, fz;
			u32x4 ch;
			load_node(nodes, a_node + onx, (a_node + 16u) - onx, a_node + ony, (a_node + 80u) - ony, a_node + onz, (a_node + 144u) - onz, a_node,
				nx, fx, ny, fy, nz, fz, ch);
			bool enter[4];
			if (wave_fast) {
				// No NaN can arise for these rays, so min/max are order-free: v_max3/v_min3.
#pragma unroll
				for (int i = 0; i < 4; i++) {
					const float ax = (nx[i] - ox) * rdx, bx = (fx[i] - ox) * rdx;
					const float ay = (ny[i] - oy) * rdy, by = (fy[i] - oy) * rdy;
					const float az = (nz[i] - oz) * rdz, bz = (fz[i] - oz) * rdz;
					const float tn = fmaxf(fmaxf(fmaxf(ax, ay), az), tmin_ray);
					const float tf = fminf(fminf(fminf(bx, by), bz), far_t);
					enter[i] = (tn <= tf) && (ch[i] != RTK_REF_NONE);
				}
			} else {
#pragma unroll
				for (int i = 0; i < 4; i++) {
					// rtk.c:458-465 with _mm_max_ps/_mm_min_ps operand order (decides what a NaN from 0*inf does)
					const float ax = (nx[i] - ox) * rdx, bx = (fx[i] - ox) * rdx;
					const float ay = (ny[i] - oy) * rdy, by = (fy[i] - oy) * rdy;
					const float az = (nz[i] - oz) * rdz, bz = (fz[i] - oz) * rdz;
					const float tn = sse_max(sse_max(ax, ay), sse_max(az, tmin_ray));
					const float tf = sse_min(sse_min(bx, by), sse_min(bz, far_t));
					enter[i] = (tn <= tf) && (ch[i] != RTK_REF_NONE);
				}
			}
			// the first admitted slot is entered, the others wait on the stack: any order gives the same set
			uint32_t next = RTK_REF_NONE;
#pragma unroll
			for (int i = 0; i < 4; i++) {
				if (enter[i]) {
					if (next == RTK_REF_NONE) next = ch[i];
					else AH_PUSH(ch[i]);
				}
			}
			if (next == RTK_REF_NONE) AH_POP();
			else top = next;
		}

		// ---------------------------------------------------------------- leaf
		// rtk.c's groups of four (rtk.c:212, 302-336) as rtk_trace_kernel's MODE 2 takes them: a partial last group is evaluated in
		// double; a full group is first scanned for an exact zero among its edge functions, then evaluated, in double if there was one.
		if (active && AH_IS_LEAF(top)) {
			const uint32_t slot0 = top & 0x7fffffffu;
			uint32_t i = 0, n = 1;
			bool force = false, scan = false, scanned = false, zero_in_group = false;
			while (i < n) {
				f32x4 A, B, C;
				load_tri(tris, (slot0 + i) * (uint32_t)RTK_TRI_STRIDE, A, B, C);
				if (i == 0u) n = __float_as_uint(C.w);          // leaf size rides in the first record
				if ((i & 3u) == 0u) {
					if (scanned) scanned = false;                      // second pass over the group: `force` is decided
					else { force = (n - i) < 4u; scan = !force; zero_in_group = false; }
				}
				// permute to (kx,ky,kz) and move the origin (rtk.c:232-280)
				const float v0x = (kz0 ? A.y : (kz1 ? A.z : A.x)) - sox;
				const float v0y = (kz0 ? A.z : (kz1 ? A.x : A.y)) - soy;
				const float v0z = (kz0 ? A.x : (kz1 ? A.y : A.z)) - soz;
				const float v1x = (kz0 ? B.y : (kz1 ? B.z : B.x)) - sox;
				const float v1y = (kz0 ? B.z : (kz1 ? B.x : B.y)) - soy;
				const float v1z = (kz0 ? B.x : (kz1 ? B.y : B.z)) - soz;
				const float v2x = (kz0 ? C.y : (kz1 ? C.z : C.x)) - sox;
				const float v2y = (kz0 ? C.z : (kz1 ? C.x : C.y)) - soy;
				const float v2z = (kz0 ? C.x : (kz1 ? C.y : C.z)) - soz;
				// shear (rtk.c:284-292)
				const float x0 = v0x + shx * v0z, y0 = v0y + shy * v0z, z0 = shz * v0z;
				const float x1 = v1x + shx * v1z, y1 = v1y + shy * v1z, z1 = shz * v1z;
				const float x2 = v2x + shx * v2z, y2 = v2y + shy * v2z, z2 = shz * v2z;
				// edge functions (rtk.c:298-300)
				float u, v, w;
				if (scan) {
					u = x1 * y2 - y1 * x2;
					v = x2 * y0 - y2 * x0;
					w = x0 * y1 - y0 * x1;
					zero_in_group = zero_in_group || u == 0.0f || v == 0.0f || w == 0.0f;
					if ((i & 3u) == 3u) { scan = false; scanned = true; force = zero_in_group; i &= ~3u; }   // rtk.c:306
					else i++;
					continue;
				}
				if (!force) {
					u = x1 * y2 - y1 * x2;
					v = x2 * y0 - y2 * x0;
					w = x0 * y1 - y0 * x1;
				} else {
					const double xd0 = x0, yd0 = y0, xd1 = x1, yd1 = y1, xd2 = x2, yd2 = y2;
					u = (float)(xd1 * yd2 - yd1 * xd2);
					v = (float)(xd2 * yd0 - yd2 * xd0);
					w = (float)(xd0 * yd1 - yd0 * xd1);
				}
				// rtk.c:340-342
				const bool neg = sse_min(sse_min(u, v), w) < 0.0f;
				const bool pos = sse_max(sse_max(u, v), w) > 0.0f;
				// rtk.c:346-353
				const float det = (u + v) + w;
				const float rcp = 1.0f / det;
				float zz = u * z0;
				zz = zz + v * z1;
				zz = zz + w * z2;
				const float t = zz * rcp;
				const uint32_t prim = __float_as_uint(A.w);
				bool in_range = !(neg && pos) && t > tmin_ray && t < tmax_ray;   // rtk.c:354
				if (FILT) {
					if (has_after) in_range = in_range && (t > after_t || (t == after_t && prim > after_prim));
					in_range = in_range && prim != skip_prim;
					if (p.mesh_mask) {
						const uint32_t mesh = __float_as_uint(B.w) >> RTK_TRI_MESH_SHIFT;
						in_range = in_range && mesh < p.mesh_mask_bits && ((p.mesh_mask[mesh >> 5] >> (mesh & 31u)) & 1u);
					}
				}
				if (FILL) {
					// the `room` closest candidates of the ray, sorted by (t, prim), in the ray's own segment: lanes write disjoint
					// segments. Once it is full a candidate must beat the last entry. The far bound of the walk STAYS at max_t (MODE 2
					// shrinks it to the last entry's t): a box's entry distance and a triangle's t are rounded differently, so a
					// triangle in a face of its box can have t one ulp in front of the box, and with a shrunk bound which of two such
					// neighbours is kept would depend on the order of the walk. As it is, the kept records are the first of the full list.
					if (in_range && cand_n == room) {
						const rtk_hit_record last = list[room - 1u];
						in_range = t < last.t || (t == last.t && prim < last.prim);
					}
					if (in_range) {
						uint32_t j = cand_n < room ? cand_n : room - 1u;
						while (j > 0u) {
							const rtk_hit_record e = list[j - 1u];
							if (e.t < t || (e.t == t && e.prim < prim)) break;
							list[j] = e;
							j--;
						}
						rtk_hit_record r;
						r.t = t; r.u = u * rcp; r.v = v * rcp; r.prim = prim;
						list[j] = r;
						if (cand_n < room) cand_n++;
					}
				} else {
					cand_n += in_range ? 1u : 0u;
				}
				i++;
			}
			AH_POP();
		}

		// ---------------------------------------------------------------- retire
		if (active && top == RTK_REF_NONE) {
			if (FILL) { if (p.written) __builtin_nontemporal_store(cand_n, p.written + ray_index); }
			else __builtin_nontemporal_store(cand_n, p.counts + ray_index);
			active = false;
		}
	}
}

// ------------------------------------------------------------------------------------
// host side: the kernel's two doors (rtk_trace_shared.h)
// ------------------------------------------------------------------------------------

namespace {

typedef void (*allhits_kernel_fn)(AllHitsParams);

// form: fill | filtered << 1
allhits_kernel_fn allhits_form(int form)
{
	switch (form) {
	case 0: return rtk_allhits_kernel<false, false>;
	case 1: return rtk_allhits_kernel<true, false>;
	case 2: return rtk_allhits_kernel<false, true>;
	default: return rtk_allhits_kernel<true, true>;
	}
}

std::mutex g_occ_mutex;
int g_occ[RTK_MAX_DEVICES][4];

} // namespace

extern "C" uint32_t rtk_amd_allhits_stack_entries(void) { return AH_LDS_STACK; }

int rtk_allhits_occupancy(int device, int form)
{
	std::lock_guard<std::mutex> lock(g_occ_mutex);
	if (device < 0 || device >= RTK_MAX_DEVICES) device = 0;
	int &o = g_occ[device][form & 3];
	if (o == 0) {
		int nb = 0;
		if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, allhits_form(form & 3), BLOCK_THREADS, 0) != hipSuccess) nb = 0;
		o = nb >= 1 ? nb : 1;
	}
	return o;
}

void rtk_allhits_kernel_launch(int form, const AllHitsParams &p, unsigned blocks, hipStream_t stream)
{
	hipLaunchKernelGGL(allhits_form(form & 3), dim3(blocks), dim3(BLOCK_THREADS), 0, stream, p);
}
