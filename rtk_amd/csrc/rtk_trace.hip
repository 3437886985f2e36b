// rtk_trace.hip -- BVH4 traversal + watertight triangle test for gfx950 (MI355X).
//
// What it computes is the reference's rtk_trace_ray (rtk.c:543-577) for a whole batch:
//   ray setup        rtk.c:550-566   -> ray_setup()
//   4-wide slab test rtk.c:457-472   -> node_step()
//   triangle test    rtk.c:284-364   -> tri_test()   (per triangle, not per group of 4)
//   closest update   rtk.c:366-386   -> canonical tie rule, DESIGN.md "Ties"
// How it runs is CDNA4-specific: one ray per lane of a 64-wide wave, persistent waves
// that pull ray chunks from a global counter and re-fill idle lanes by ballot rank, the
// per-lane traversal stack in LDS ([entry][lane] so that a wave's push/pop is one
// conflict-free ds_write_b64/ds_read_b64), 128 B nodes = one cache line per visit.
//
// FLOATING POINT: this file must be compiled with -ffp-contract=off. The float operation
// order in tri_test() is normative (sign of u,v,w decides hit/miss); see SURVEY.md
// section 0. Divisions are IEEE (hipcc default -fhip-fp32-correctly-rounded-divide-sqrt).
#include "rtk_dev.h"

#include <algorithm>
#include "rtk_trace_shared.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <mutex>

#include "rtk_trace_lane.h"

// A push that does not fit the stack (LDS entries + the global spill area sized from the tree depth) is
// dropped WITHOUT advancing sp and flagged; it cannot happen for a tree (at most three pushes per level,
// rtk_upload.hip rejects blobs that are not trees), so a set flag means a corrupted scene, never an
// out-of-bounds access.
#define RTK_PUSH(e_)                                                                                        \
	do {                                                                                                    \
		if (sp < LDS_STACK) { stk[sp][lane] = (e_); sp++; }                                                 \
		else if (sp - LDS_STACK < p.spill_cap) {                                                            \
			p.spill[(size_t)(sp - LDS_STACK) * p.spill_stride + glane] = (e_); sp++; if (COUNT) c_spills++; \
		} else p.counter[RTK_ERROR_WORD] = 1ull;                                                            \
	} while (0)

// Next node from the stack: ONE entry per call. An entry that starts behind the current hit (rtk.c:432; canonical ties:
// an entry AT the hit distance may still hold an equal-t candidate with a lower id) leaves top = RTK_REF_RETRY and the
// lane pops again at the head of the next node-loop trip, beside the other lanes' node steps. A `while` here cost 5.4
// wave-level trips per step on incoherent rays (7 of a ray's ~27 pops are culled, and the wave waits for its unluckiest
// lane): as many instructions as the box tests. top = NONE when the stack is empty.
#define RTK_REF_RETRY 0xfffffffeu
#define RTK_POP()                                                                                           \
	do {                                                                                                    \
		if (sp == 0u) top = RTK_REF_NONE;                                                                   \
		else {                                                                                              \
			--sp;                                                                                           \
			uint2 e_ = stk[sp < LDS_STACK ? sp : LDS_STACK - 1u][lane];          /* always an LDS read (ds_read_b64), never a flat one */ \
			if (sp >= LDS_STACK) {                       /* nontemporal: read once, and keeps hipcc from merging both into a flat load */ \
				const unsigned long long w_ = __builtin_nontemporal_load(reinterpret_cast<const unsigned long long *>(p.spill + (size_t)(sp - LDS_STACK) * p.spill_stride + glane)); \
				e_ = make_uint2((uint32_t)w_, (uint32_t)(w_ >> 32));                                                \
			}                                                                                                   \
			/* (reference, entry distance). Any-hit: an entry never lies behind best_t, which stays max_t until the ray is over */ \
			top = (MODE != 1 && __uint_as_float(e_.y) > best_t) ? RTK_REF_RETRY : e_.x;                                    \
		}                                                                                                   \
	} while (0)
// One child of a node step: the lane enters it if its slab test passed and the slot is not empty; its key is the entry
// distance (+inf otherwise) and nhit counts the children entered. The condition is kept as the wave's mask so that the
// select reads it directly and the count is ONE add-with-carry (as a bool: a 0/1 select and an add).
#define RTK_CHILD_HIT(slab_ok_, i_)                                                                                   \
	do {                                                                                                              \
		const unsigned long long hm_ = __builtin_amdgcn_ballot_w64(slab_ok_) & __builtin_amdgcn_ballot_w64(ref[i_] != RTK_REF_NONE); \
		key[i_] = __builtin_amdgcn_inverse_ballot_w64(hm_) ? tn : __builtin_inff();                                   \
		asm("v_addc_co_u32_e64 %0, vcc, 0, %0, %1" : "+v"(nhit) : "s"(hm_) : "vcc");                                 \
	} while (0)
#define RTK_IS_LEAF(top_) ((top_) < RTK_REF_RETRY && (int32_t)(top_) < 0)

#ifndef PL_MIN_WAVES
#define PL_MIN_WAVES 5             // waves per SIMD the register allocator must leave room for (78 VGPRs used; LDS allows five workgroups per CU)
#endif

template <int MODE /*0 closest, 1 any, 2 collect the k closest candidates*/, bool COUNT, bool FILT /*built-in candidate filters*/, bool QN /*64 B compressed nodes*/>
__global__ void __launch_bounds__(BLOCK_THREADS, PL_MIN_WAVES) rtk_trace_kernel(TraceParams p)
{
	__shared__ uint2 s_stack[WAVES_PER_BLOCK][LDS_STACK][64];

	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t wave = threadIdx.x >> 6;
	uint2 (*stk)[64] = s_stack[wave];
	const uint32_t glane = blockIdx.x * BLOCK_THREADS + threadIdx.x;
	const char *const nodes = reinterpret_cast<const char *>(p.sc.nodes);
	const char *const qnodes = reinterpret_cast<const char *>(p.sc.qnodes);
	const char *const tris = reinterpret_cast<const char *>(p.sc.tris);

	// (a list whose length earlier work on the stream wrote: the rays the assembly kernel, rtk_lane_hot.S, left over, or the caller's
	// own list, rtk_ray_list. p.n is what the arrays hold: a larger count is clamped to it)
	if (p.n_indirect) { const unsigned long long listed = *p.n_indirect; p.n = listed < p.n ? listed : p.n; }
	// wave-uniform ray range owned by this wave
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
	uint32_t ray_index = 0;               // the launcher keeps batches below 2^32 rays
	float ox = 0, oy = 0, oz = 0, rdx = 0, rdy = 0, rdz = 0, tmin_ray = 0, tmax_ray = 0;
	float sox = 0, soy = 0, soz = 0, shx = 0, shy = 0, shz = 0;
	bool kz0 = false, kz1 = false;
	uint32_t onx = 0, ony = 0, onz = 0;     // byte offset of the NEAR plane row of each axis inside a node; far = the other row
	float best_t = 0, best_u = 0, best_v = 0;
	uint32_t best_prim = RTK_PRIM_NONE;
	uint32_t cand_n = 0;                                  // MODE 2: candidates collected for this ray (<= p.cand_k), best_t = what the k-th one beats
	float after_t = 0;                                    // FILT: candidates must come after (after_t, after_prim)
	uint32_t after_prim = 0, skip_prim = RTK_PRIM_NONE;   // FILT: ... and must not be skip_prim
	bool has_after = false;
	uint32_t top = RTK_REF_NONE;
	uint32_t sp = 0;
	uint32_t c_nodes = 0, c_leaves = 0, c_tris = 0, c_spills = 0;
	unsigned long long w_node_steps = 0, w_tri_steps = 0;   // COUNT only: wave-level loop trips (divergence diagnostics)
	// A ray is "special" if its slab products can be NaN (0*inf) or its inputs are not finite;
	// only then does the SSE operand order of min/max matter (see node step).
	bool special = false;
	bool wave_fast = true;   // wave-uniform: no active lane is special

	for (;;) {
		// ---------------------------------------------------------------- refill
		const unsigned long long idle = __builtin_amdgcn_ballot_w64(!active);
		const uint32_t n_idle = (uint32_t)__popcll(idle);
		if (n_idle == 64u || (n_idle >= p.refill_min && !(pool_empty && w_next >= w_end))) {
			if (w_next >= w_end && !pool_empty) {
				// chunks of 64 rays are dealt through RTK_QUEUES queue heads (chunk c belongs to queue c % 8,
				// a wave starts on blockIdx % 8 and moves on when a queue is drained): one word only
				// serves ~88 atomics/us, and bigger chunks per atomic unbalance the tail
				const unsigned long long num_chunks = (p.n + 63ull) >> 6;
				pool_empty = true;
				while (queues_left) {
					unsigned long long got = 0;
					if (lane == 0) got = atomicAdd(p.counter + RTK_QUEUE_WORD(queue), 1ull);
					// all 64 lanes are converged here; lane 0's value becomes wave-uniform (SGPRs)
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
					ray_index = p.perm ? (uint32_t)p.perm[w_next + rank] : (uint32_t)map_index(w_next + rank, p.image_w, p.image_h, p.tile_blocks);   // perm: sort words, ray number in the low half
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
					// (kx,ky,kz): kz==2 -> (x,y,z); kz==0 -> (y,z,x); kz==1 -> (z,x,y)
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
					shz = kz0 ? rdx : (kz1 ? rdy : rdz);          // 1 / d[kz] is one of the three reciprocals above, bit for bit
					// near/far plane offsets inside the node by direction sign BIT (rtk.c:152-154, 458-463)
					const uint32_t sx = __float_as_uint(dx) >> 31, sy = __float_as_uint(dy) >> 31, sz = __float_as_uint(dz) >> 31;
					onx = sx * 16u;
					ony = 32u + sy * 16u;
					onz = 64u + sz * 16u;
					special = !(isfinite(rdx) && isfinite(rdy) && isfinite(rdz) && rdx != 0.0f && rdy != 0.0f && rdz != 0.0f &&
						isfinite(ox) && isfinite(oy) && isfinite(oz) && tmin_ray == tmin_ray && tmax_ray == tmax_ray);
					best_t = tmax_ray; best_u = 0.0f; best_v = 0.0f; best_prim = RTK_PRIM_NONE;
					if (FILT) {
						has_after = p.after != nullptr;
						if (has_after) { const rtk_hit_record a = p.after[ray_index]; after_t = a.t; after_prim = a.prim; has_after = a.prim != RTK_PRIM_NONE; }
						skip_prim = p.ignore_prim ? p.ignore_prim[ray_index] : RTK_PRIM_NONE;
					}
					top = 0u;  // root node
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

		// the active lanes as a wave mask in SCALAR registers (first-lane reads: left to itself hipcc keeps this loop-carried
		// value in a vector register pair): the votes below are votes on plain comparisons ANDed with it on the scalar unit
		// -- a vote on `active && ...` rebuilds the mask from a 0/1 vector register, two vector instructions each
		const unsigned long long m_act_ = __builtin_amdgcn_ballot_w64(active);
		const unsigned long long m_active = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(m_act_ >> 32)) << 32) |
			(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)m_act_);
		// ---------------------------------------------------------------- inner nodes
		for (;;) {
			// Lanes that reached a leaf wait here for the others. When only a few lanes are
			// still descending and leaves are waiting, go and do the leaves first.
			const bool retry = MODE != 1 && active && top == RTK_REF_RETRY;
			if (retry) RTK_POP();
			const unsigned long long m_node = __builtin_amdgcn_ballot_w64((int32_t)top >= 0) & m_active;
			const bool want_node = __builtin_amdgcn_inverse_ballot_w64(m_node);
			if (m_node == 0ull) {
				if (MODE != 1 && (__builtin_amdgcn_ballot_w64(top == RTK_REF_RETRY) & m_active) != 0ull) continue;   // somebody is still popping
				break;
			}
			// (lanes still popping are not counted as descending: counting them was 1 % slower)
			// (RTK_IS_LEAF as one signed comparison: sign bit set and below RTK_REF_RETRY = -2)
			if ((uint32_t)__popcll(m_node) < p.node_exit && (__builtin_amdgcn_ballot_w64((int32_t)top < (int32_t)RTK_REF_RETRY) & m_active) != 0ull) break;
			if (COUNT) w_node_steps++;
			if (!want_node) continue;
			uint32_t ref[4];
			float key[4];
			uint32_t nhit = 0;
			if (COUNT) c_nodes++;
			if (QN && wave_fast) {
				// Compressed node: plane = org + q * scale, so its ray parameter is A + q * S with A = (org - o) * rcp,
				// S = scale * rcp. Low planes were rounded down and high planes up when the node was made, so the
				// decoded slab interval contains the exact one; a small margin covers the rounding of this arithmetic,
				// so that every child the exact test admits is admitted here too.
				f32x4 l0;
				u32x4 l1, l2, l3;
				load_qnode(qnodes, top << 6, l0, l1, l2, l3);
				const float Ax = (l0.x - ox) * rdx, Ay = (l0.y - oy) * rdy, Az = (l0.z - oz) * rdz;
				const float Sx = l0.w * rdx, Sy = __uint_as_float(l1.x) * rdy, Sz = __uint_as_float(l1.y) * rdz;
				// per axis: the rounding of A + q * S (and of the exact test it stands in for) is below 2^-22 of
				// |A| + 255 |S|; near planes start from A - e, far planes from A + e. Per AXIS on purpose: one tiny
				// direction component makes that axis' A and S huge, and a common margin would open every box.
				const float ex = 0x1p-21f * __builtin_fmaf(fabsf(Sx), 255.0f, fabsf(Ax));
				const float ey = 0x1p-21f * __builtin_fmaf(fabsf(Sy), 255.0f, fabsf(Ay));
				const float ez = 0x1p-21f * __builtin_fmaf(fabsf(Sz), 255.0f, fabsf(Az));
				const float Anx = Ax - ex, Afx = Ax + ex, Any = Ay - ey, Afy = Ay + ey, Anz = Az - ez, Afz = Az + ez;
				const bool ngx = onx != 0u, ngy = ony != 32u, ngz = onz != 64u;      // direction sign bits
				const uint32_t wnx = ngx ? l1.w : l1.z, wfx = ngx ? l1.z : l1.w;
				const uint32_t wny = ngy ? l2.y : l2.x, wfy = ngy ? l2.x : l2.y;
				const uint32_t wnz = ngz ? l2.w : l2.z, wfz = ngz ? l2.z : l2.w;
				ref[0] = l3.x; ref[1] = l3.y; ref[2] = l3.z; ref[3] = l3.w;
#pragma unroll
				for (int i = 0; i < 4; i++) {
					// near and far plane of one axis in one v_pk_fma_f32 (each half is the same single-rounded fma)
					const f32x2 px = __builtin_elementwise_fma((f32x2){ ubyte_f32(wnx, i), ubyte_f32(wfx, i) }, (f32x2){ Sx, Sx }, (f32x2){ Anx, Afx });
					const f32x2 py = __builtin_elementwise_fma((f32x2){ ubyte_f32(wny, i), ubyte_f32(wfy, i) }, (f32x2){ Sy, Sy }, (f32x2){ Any, Afy });
					const f32x2 pz = __builtin_elementwise_fma((f32x2){ ubyte_f32(wnz, i), ubyte_f32(wfz, i) }, (f32x2){ Sz, Sz }, (f32x2){ Anz, Afz });
					const float tn = fmaxf(fmaxf(fmaxf(px.x, py.x), pz.x), tmin_ray);
					const float tf = fminf(fminf(fminf(px.y, py.y), pz.y), best_t);
					RTK_CHILD_HIT(tn <= tf, i);
				}
			} else {
			const uint32_t a_node = top << 7;
			f32x4 nx, fx, ny, fy, nz, fz;
			u32x4 ch;
			load_node(nodes, a_node + onx, (a_node + 16u) - onx, a_node + ony, (a_node + 80u) - ony, a_node + onz, (a_node + 144u) - onz, a_node,
				nx, fx, ny, fy, nz, fz, ch);
			ref[0] = ch.x; ref[1] = ch.y; ref[2] = ch.z; ref[3] = ch.w;
			if (wave_fast) {
				// No NaN can arise for these rays, so min/max are order-free: v_max3/v_min3.
#pragma unroll
				for (int i = 0; i < 4; i++) {
					const float ax = (nx[i] - ox) * rdx, bx = (fx[i] - ox) * rdx;
					const float ay = (ny[i] - oy) * rdy, by = (fy[i] - oy) * rdy;
					const float az = (nz[i] - oz) * rdz, bz = (fz[i] - oz) * rdz;
					const float tn = fmaxf(fmaxf(fmaxf(ax, ay), az), tmin_ray);
					const float tf = fminf(fminf(fminf(bx, by), bz), best_t);
					RTK_CHILD_HIT(tn <= tf, i);
				}
			} else {
#pragma unroll
				for (int i = 0; i < 4; i++) {
					// rtk.c:458-465: (bound - origin) * rcp_dir, then the folded interval test with
					// _mm_max_ps/_mm_min_ps operand order (decides what a NaN from 0*inf does)
					const float ax = (nx[i] - ox) * rdx, bx = (fx[i] - ox) * rdx;
					const float ay = (ny[i] - oy) * rdy, by = (fy[i] - oy) * rdy;
					const float az = (nz[i] - oz) * rdz, bz = (fz[i] - oz) * rdz;
					const float tn = sse_max(sse_max(ax, ay), sse_max(az, tmin_ray));
					const float tf = sse_min(sse_min(bx, by), sse_min(bz, best_t));
					const bool h = (tn <= tf) && (ref[i] != RTK_REF_NONE);
					key[i] = h ? tn : __builtin_inff();
					nhit += h ? 1u : 0u;
				}
			}
			}
			// nearest first (rtk.c:496-517 orders by entry distance)
			// ... as a 5-comparator network on (distance, reference) PAIRS held as one 64-bit value each, distance in the high
			// half: read as a double such a pair orders like its distance (the bit patterns of non-NaN floats order like their
			// values under a sign-magnitude compare, which is what a double compare of the pair is; +inf, the key of a child that
			// is not entered, becomes a large finite double; equal distances fall back on the reference, any order of which is
			// right), so a comparator is one v_min_f64 and one v_max_f64 instead of a compare and four selects. No key is a NaN.
			double pr[4];
#pragma unroll
			for (int i = 0; i < 4; i++) pr[i] = __hiloint2double((int)__float_as_uint(key[i]), (int)ref[i]);
			cswap_pair(pr[0], pr[1]);
			cswap_pair(pr[2], pr[3]);
			cswap_pair(pr[0], pr[2]);
			cswap_pair(pr[1], pr[3]);
			cswap_pair(pr[1], pr[2]);
			if (nhit == 0u) {
				RTK_POP();
			} else {
				top = (uint32_t)__double2loint(pr[0]);
				const uint32_t np = nhit - 1u;              // sorted slots np..1 go on the stack, far to near
				if (sp + 3u <= LDS_STACK) {
					// Branch-free: rows sp..sp+2 all exist. Slot i <= np goes to row sp+np-i; the others (misses) are
					// written too, to the distinct rows sp+np..sp+2 above the new top, where garbage is harmless.
#pragma unroll
					for (int i = 1; i <= 3; i++) {
						const uint32_t row = sp + np - (uint32_t)i + ((uint32_t)i > np ? 3u : 0u);
						stk[row][lane] = make_uint2((uint32_t)__double2loint(pr[i]), (uint32_t)__double2hiint(pr[i]));
					}
					sp += np;
				} else {
#pragma unroll
					for (int i = 3; i >= 1; i--) {
						if (nhit > (uint32_t)i) {
							const uint2 e = make_uint2((uint32_t)__double2loint(pr[i]), (uint32_t)__double2hiint(pr[i]));
							RTK_PUSH(e);
						}
					}
				}
			}
		}

		// ---------------------------------------------------------------- leaf
		// Triangles are taken one at a time but in the reference's groups of four
		// (rtk.c:212): if any slot of a group -- padding slots of a partial last group
		// included -- has an edge function that is exactly zero, ALL slots of the group
		// use the double-precision edge functions (rtk.c:302-336). A partial group is
		// known up front; a zero inside a full group is rare, so the group is simply
		// redone from a snapshot of the best hit. This keeps t/u/v bit-identical to
		// rtk.c traversing the same leaves.
		if (active && RTK_IS_LEAF(top)) {
			const uint32_t slot0 = top & 0x7fffffffu;
			if (COUNT) c_leaves++;
			uint32_t i = 0, n = 1;
			bool force = false, redo = false;
			// MODE 2 cannot undo list insertions, so a full group is first scanned for exact zeros, then evaluated
			bool scan = false, scanned = false, zero_in_group = false;
			float sn_t = best_t, sn_u = best_u, sn_v = best_v;
			uint32_t sn_prim = best_prim;
			while (i < n) {
				f32x4 A, B, C;
				load_tri(tris, (slot0 + i) * (uint32_t)RTK_TRI_STRIDE, A, B, C);
				if (COUNT && lane == (uint32_t)__ffsll((long long)__builtin_amdgcn_ballot_w64(true)) - 1u) w_tri_steps++;
				if (i == 0u) n = __float_as_uint(C.w);          // leaf size rides in the first record
				if (MODE == 2 && (i & 3u) == 0u) {
					if (scanned) scanned = false;                      // second pass over the group: `force` is decided
					else { force = (n - i) < 4u; scan = !force; zero_in_group = false; }
				} else if ((i & 3u) == 0u) {
					if (redo) { force = true; redo = false; }
					else {
						if (MODE == 1 && best_prim != RTK_PRIM_NONE) break;   // any-hit: a whole group accepted something
						force = (n - i) < 4u;
						sn_t = best_t; sn_u = best_u; sn_v = best_v; sn_prim = best_prim;
					}
				}
				if (COUNT) c_tris++;
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
				if (MODE == 2 && scan) {
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
					if (MODE != 2 && (u == 0.0f || v == 0.0f || w == 0.0f)) {
						// rtk.c:306: the whole group switches to double precision
						best_t = sn_t; best_u = sn_u; best_v = sn_v; best_prim = sn_prim;
						redo = true;
						i &= ~3u;
						continue;
					}
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
					// built-in filters: the candidate is offered only if every filter accepts it (rtk.h:117 semantics
					// with the filter evaluated on the device)
					if (has_after) in_range = in_range && (t > after_t || (t == after_t && prim > after_prim));
					in_range = in_range && prim != skip_prim;
					if (p.mesh_mask) {
						const uint32_t mesh = __float_as_uint(B.w) >> RTK_TRI_MESH_SHIFT;
						in_range = in_range && mesh < p.mesh_mask_bits && ((p.mesh_mask[mesh >> 5] >> (mesh & 31u)) & 1u);
					}
				}
				if (MODE == 2) {
					// keep the k closest candidates of this ray, sorted by (t, prim), in the ray's slice of p.cand; once the
					// list is full, best_t (the culling distance) is the last entry's t
					rtk_hit_record *list = p.cand + (size_t)ray_index * p.cand_k;
					if (in_range && cand_n == p.cand_k) {
						const rtk_hit_record last = list[p.cand_k - 1u];
						in_range = t < last.t || (t == last.t && prim < last.prim);
					}
					if (in_range) {
						uint32_t j = cand_n < p.cand_k ? cand_n : p.cand_k - 1u;
						while (j > 0u) {
							const rtk_hit_record e = list[j - 1u];
							if (e.t < t || (e.t == t && e.prim < prim)) break;
							list[j] = e;
							j--;
						}
						rtk_hit_record r;
						r.t = t; r.u = u * rcp; r.v = v * rcp; r.prim = prim;
						list[j] = r;
						if (cand_n < p.cand_k) cand_n++;
						if (cand_n == p.cand_k) best_t = list[p.cand_k - 1u].t;
					}
				} else if (MODE == 1) {
					if (in_range && best_prim == RTK_PRIM_NONE) { best_prim = prim; best_t = t; }
				} else {
					// rtk.c:371 with the canonical tie rule: lowest primitive id among bit-equal t
					if (in_range && (t < best_t || (t == best_t && prim < best_prim))) {
						best_t = t; best_u = u * rcp; best_v = v * rcp; best_prim = prim;
					}
				}
				i++;
			}
			if (MODE == 1 && best_prim != RTK_PRIM_NONE) {
				top = RTK_REF_NONE;
				sp = 0u;
			} else {
				RTK_POP();
			}
		}

		// ---------------------------------------------------------------- retire
		if (active && top == RTK_REF_NONE) {
			if (MODE == 2) {
				p.cand_count[ray_index] = cand_n;
			} else if (MODE == 1) {
				p.occluded[ray_index] = best_prim != RTK_PRIM_NONE ? 1 : 0;
			} else {
				rtk_hit_record r;
				r.t = best_t; r.u = best_u; r.v = best_v; r.prim = best_prim;
				st_f4_stream(p.hits + ray_index, r.t, r.u, r.v, __uint_as_float(r.prim));
			}
			if (COUNT) {
				atomicAdd(p.counter + 1, 1ull);
				atomicAdd(p.counter + 2, (unsigned long long)c_nodes);
				atomicAdd(p.counter + 3, (unsigned long long)c_leaves);
				atomicAdd(p.counter + 4, (unsigned long long)c_tris);
				atomicAdd(p.counter + 5, best_prim != RTK_PRIM_NONE ? 1ull : 0ull);
				atomicAdd(p.counter + 6, (unsigned long long)c_spills);
				c_nodes = c_leaves = c_tris = c_spills = 0;
			}
			active = false;
		}
	}
	if (COUNT) {
		// wave-level trip counts: node steps are counted on a wave-uniform variable, triangle steps
		// on whichever lane was first in the leaf loop; rays/64 gives steps per 64 rays
		if (lane == 0) atomicAdd(p.counter + 7, w_node_steps);
		atomicAdd(p.counter + 8, w_tri_steps);
	}
}

// ---- ray reordering (RTK_TRACE_SORT_RAYS): 16-bit key = 4 bits of origin cell per axis inside the
// batch's origin bounds + direction octant; rays of one key start close together and head the same way,
// so the 64 rays a wave pulls from the sorted order share nodes (L1/L2 hits instead of fabric traffic).
__device__ __forceinline__ uint32_t f2ord_(float f) { const uint32_t b = __float_as_uint(f); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
__device__ __forceinline__ float ord2f_(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

// Origin bounds from every `stride`-th ray: the cells only have to spread the batch over the key range, outliers are
// clamped into the border cells by the key kernel.
__global__ void rtk_ray_bounds_kernel(const rtk_ray *rays, unsigned long long n, unsigned long long stride, uint32_t *bounds)
{
	__shared__ float s_mn[3][4], s_mx[3][4];
	float mn[3] = { INFINITY, INFINITY, INFINITY }, mx[3] = { -INFINITY, -INFINITY, -INFINITY };
	for (unsigned long long k = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; k * stride < n; k += (unsigned long long)gridDim.x * blockDim.x) {
		const unsigned long long i = k * stride;
		const float4 r0 = *reinterpret_cast<const float4 *>(rays + i);
		const float o[3] = { r0.x, r0.y, r0.z };
		for (int a = 0; a < 3; a++) if (isfinite(o[a])) { mn[a] = fminf(mn[a], o[a]); mx[a] = fmaxf(mx[a], o[a]); }
	}
	for (int a = 0; a < 3; a++) {
		for (int o = 32; o > 0; o >>= 1) { mn[a] = fminf(mn[a], __shfl_xor(mn[a], o)); mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], o)); }
		if ((threadIdx.x & 63u) == 0) { s_mn[a][threadIdx.x >> 6] = mn[a]; s_mx[a][threadIdx.x >> 6] = mx[a]; }
	}
	__syncthreads();
	if (threadIdx.x < 3) {
		const int a = threadIdx.x;
		float lo = s_mn[a][0], hi = s_mx[a][0];
		for (int w = 1; w < 4; w++) { lo = fminf(lo, s_mn[a][w]); hi = fmaxf(hi, s_mx[a][w]); }
		atomicMin(&bounds[a], f2ord_(lo));
		atomicMax(&bounds[3 + a], f2ord_(hi));
	}
}

__device__ __forceinline__ uint32_t morton_cells_(const uint32_t q[3], uint32_t cell_bits)
{
	// Morton-interleave the cell coordinates (x lowest) so that consecutive keys are neighbours in space
	uint32_t key = 0;
	for (uint32_t b = 0; b < cell_bits; b++)
		key |= (((q[0] >> b) & 1u) << (3u * b)) | (((q[1] >> b) & 1u) << (3u * b + 1u)) | (((q[2] >> b) & 1u) << (3u * b + 2u));
	return key;
}

__device__ __forceinline__ uint32_t cell_of_(float x, float lo, float hi, uint32_t cells)
{
	const float ext = hi - lo;
	float t = ext > 0.0f ? (x - lo) / ext : 0.0f;
	t = t >= 0.0f ? (t <= 1.0f ? t : 1.0f) : 0.0f;           // NaN -> 0
	const uint32_t c = (uint32_t)(t * (float)cells);
	return c > cells - 1u ? cells - 1u : c;
}

// Key = cell of the ray's origin inside the batch's (sampled) origin bounds.
__global__ void rtk_ray_keys_kernel(const rtk_ray *rays, uint32_t n, const uint32_t *bounds, unsigned long long *keys,
	uint32_t cell_bits, uint32_t with_octant)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const float4 r0 = *reinterpret_cast<const float4 *>(rays + i);
	const float o[3] = { r0.x, r0.y, r0.z };
	uint32_t q[3];
	for (int a = 0; a < 3; a++) q[a] = cell_of_(o[a], ord2f_(bounds[a]), ord2f_(bounds[3 + a]), 1u << cell_bits);
	uint32_t key = morton_cells_(q, cell_bits);
	if (with_octant) {
		const float4 r1 = *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(rays + i) + 16);
		key = (key << 3) | ((__float_as_uint(r0.w) >> 31) | ((__float_as_uint(r1.x) >> 31) << 1) | ((__float_as_uint(r1.y) >> 31) << 2));
	}
	keys[i] = ((unsigned long long)key << 32) | i;      // sorted by the key, the ray's number rides below it
}

// Key = cell, inside the SCENE's bounds (union of the root's child boxes), of the point where the ray's [min_t, max_t]
// interval enters those bounds: the origin itself for rays that start inside (shadow / bounce rays), the entry point for
// rays that start outside (camera rays, config 3). That is where traversal starts doing work, so rays of one key share
// the nodes and leaves they touch. Rays that miss the bounds get the largest key: they end at the root, together.
__global__ void rtk_ray_entry_keys_kernel(const rtk_ray *rays, uint32_t n, const DevNode *root, unsigned long long *keys,
	uint32_t cell_bits, uint32_t with_octant)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
	for (int k = 0; k < 4; k++) {
		if (root->child[k] == RTK_REF_NONE) continue;
		lo[0] = fminf(lo[0], root->bx[0][k]); hi[0] = fmaxf(hi[0], root->bx[1][k]);
		lo[1] = fminf(lo[1], root->by[0][k]); hi[1] = fmaxf(hi[1], root->by[1][k]);
		lo[2] = fminf(lo[2], root->bz[0][k]); hi[2] = fmaxf(hi[2], root->bz[1][k]);
	}
	const float4 r0 = *reinterpret_cast<const float4 *>(rays + i);
	const float4 r1 = *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(rays + i) + 16);
	const float o[3] = { r0.x, r0.y, r0.z }, d[3] = { r0.w, r1.x, r1.y };
	float tn = r1.z, tf = r1.w;
	bool miss = false;
	for (int a = 0; a < 3; a++) {
		if (d[a] != 0.0f) {
			const float t0 = (lo[a] - o[a]) / d[a], t1 = (hi[a] - o[a]) / d[a];
			tn = fmaxf(tn, fminf(t0, t1));
			tf = fminf(tf, fmaxf(t0, t1));
		} else if (!(o[a] >= lo[a] && o[a] <= hi[a])) miss = true;
	}
	miss = miss || !(tn <= tf);                                   // NaN anywhere -> miss
	const uint32_t key_bits = 3u * cell_bits + (with_octant ? 3u : 0u);
	uint32_t key = (1u << key_bits) - 1u;
	if (!miss) {
		uint32_t q[3];
		for (int a = 0; a < 3; a++) q[a] = cell_of_(o[a] + d[a] * tn, lo[a], hi[a], 1u << cell_bits);
		key = morton_cells_(q, cell_bits);
		if (with_octant) key = (key << 3) | ((__float_as_uint(d[0]) >> 31) | ((__float_as_uint(d[1]) >> 31) << 1) | ((__float_as_uint(d[2]) >> 31) << 2));
	}
	keys[i] = ((unsigned long long)key << 32) | i;      // sorted by the key, the ray's number rides below it
}

// Full rtk_hit from a compact record (rtk.c:372-380 copy-out).
__device__ __forceinline__ void rtk_expand_one(const DevSceneView &sc, const rtk_hit_record *rec, unsigned long long i, rtk_hit *hits, uint8_t *mask)
{
	const rtk_hit_record r = rec[i];
	const bool hit = r.prim != RTK_PRIM_NONE && r.prim < sc.num_prims;
	if (mask) mask[i] = hit ? 1 : 0;
	if (!hit || !hits) return;
	const uint32_t slot = sc.prim_slot[r.prim];
	const DevTri tr = sc.tris[slot];
	rtk_hit h;
	h.t = r.t; h.u = r.u; h.v = r.v;
	h.vertex[0].position.x = tr.v0[0]; h.vertex[0].position.y = tr.v0[1]; h.vertex[0].position.z = tr.v0[2];
	h.vertex[1].position.x = tr.v1[0]; h.vertex[1].position.y = tr.v1[1]; h.vertex[1].position.z = tr.v1[2];
	h.vertex[2].position.x = tr.v2[0]; h.vertex[2].position.y = tr.v2[1]; h.vertex[2].position.z = tr.v2[2];
	h.vertex[0].index = sc.vertex_index[3u * slot + 0u];
	h.vertex[1].index = sc.vertex_index[3u * slot + 1u];
	h.vertex[2].index = sc.vertex_index[3u * slot + 2u];
	h.mesh_index = sc.slot_mesh[slot];
	h.triangle_index = sc.slot_tri[slot];
	hits[i] = h;
}

// status_out (host-visible memory): the launch-error word of this stream's trace launches is copied there as well, so that a
// host call needs no transfer of its own to read it (rtk_trace_ray: one copy and ~10 us less per call). A one-workgroup
// launch with ticket != 0 writes (ticket << 32 | error) there AFTER all its results: the host may poll for the ticket
// instead of waiting for the stream.
__global__ void rtk_expand_kernel(DevSceneView sc, const rtk_hit_record *rec, unsigned long long n, rtk_hit *hits, uint8_t *mask,
	const unsigned long long *status_word, unsigned long long *status_out, uint32_t ticket)
{
	const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
	if (status_out && ticket == 0u && i == 0) *status_out = *status_word;
	if (i < n) rtk_expand_one(sc, rec, i, hits, mask);
	if (status_out && ticket != 0u) {
		__threadfence_system();
		__syncthreads();
		if (threadIdx.x == 0) {
			__hip_atomic_store(status_out, ((unsigned long long)ticket << 32) | (*status_word ? 1ull : 0ull), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
		}
	}
}


// ---- rtk_trace_ray: ONE ray, one wave (reference rtk.h:129, rtk.c:543-577) --------------------------------------------------
// A per-ray call is a chain of dependent fetches: rtk_trace_kernel walks ~20 nodes and leaves one after the other for a single
// ray, ~1 us each from a cold start. Here the wave's 64 lanes walk the ray's FRONTIER breadth first: every node of a level the
// ray enters is fetched and tested at once (one lane each), the leaves found on the way are tested (one lane each) before the
// next level so that the hit culls what is behind it, and the best candidate is agreed on by the wave with the canonical tie
// rule. The chain is then as long as the tree is deep along the ray, not as long as the list of nodes visited. Exact 128-byte
// nodes and the reference's slab arithmetic with its SSE operand order (rtk.c:458-470) for every ray, the triangle groups of
// rtk_trace_kernel (rtk.c:212-386): the result is what the exact path of rtk_trace_kernel returns. The same wave expands the
// hit into the caller-visible rtk_hit and signs off with the ticket (one launch per call instead of two). A frontier that does
// not fit LDS (a degenerate scene: thousands of boxes on one ray) is reported as "not done" and the host takes the batch path.
#define ONE_FRONTIER 512
#define RTK_ONE_NOT_DONE 2ull

__device__ __forceinline__ void one_leaf(const char *tris, uint32_t slot0, bool kz0, bool kz1, float sox, float soy, float soz, float shx, float shy,
	float shz, float tmin_ray, float tmax_ray, float &best_t, float &best_u, float &best_v, uint32_t &best_prim)
{
	uint32_t i = 0, n = 1;
	bool force = false, redo = false;
	float sn_t = best_t, sn_u = best_u, sn_v = best_v;
	uint32_t sn_prim = best_prim;
	while (i < n) {
		f32x4 A, B, C;
		load_tri(tris, (slot0 + i) * (uint32_t)RTK_TRI_STRIDE, A, B, C);
		if (i == 0u) n = __float_as_uint(C.w);          // leaf size rides in the first record
		if ((i & 3u) == 0u) {
			if (redo) { force = true; redo = false; }
			else { force = (n - i) < 4u; sn_t = best_t; sn_u = best_u; sn_v = best_v; sn_prim = best_prim; }
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
		float u, v, w;
		if (!force) {
			u = x1 * y2 - y1 * x2;
			v = x2 * y0 - y2 * x0;
			w = x0 * y1 - y0 * x1;
			if (u == 0.0f || v == 0.0f || w == 0.0f) {
				// rtk.c:306: the whole group switches to double precision
				best_t = sn_t; best_u = sn_u; best_v = sn_v; best_prim = sn_prim;
				redo = true;
				i &= ~3u;
				continue;
			}
		} else {
			const double xd0 = x0, yd0 = y0, xd1 = x1, yd1 = y1, xd2 = x2, yd2 = y2;
			u = (float)(xd1 * yd2 - yd1 * xd2);
			v = (float)(xd2 * yd0 - yd2 * xd0);
			w = (float)(xd0 * yd1 - yd0 * xd1);
		}
		const bool neg = sse_min(sse_min(u, v), w) < 0.0f;          // rtk.c:340-342
		const bool pos = sse_max(sse_max(u, v), w) > 0.0f;
		const float det = (u + v) + w;                              // rtk.c:346-353
		const float rcp = 1.0f / det;
		float zz = u * z0;
		zz = zz + v * z1;
		zz = zz + w * z2;
		const float t = zz * rcp;
		const uint32_t prim = __float_as_uint(A.w);
		const bool in_range = !(neg && pos) && t > tmin_ray && t < tmax_ray;   // rtk.c:354
		// rtk.c:371 with the canonical tie rule: lowest primitive id among bit-equal t
		if (in_range && (t < best_t || (t == best_t && prim < best_prim))) { best_t = t; best_u = u * rcp; best_v = v * rcp; best_prim = prim; }
		i++;
	}
}

__global__ void __launch_bounds__(64) rtk_trace_one_kernel(DevSceneView sc, rtk_ray ray_in, rtk_hit *hit_out, uint8_t *mask_out,
	unsigned long long *status_out, uint32_t ticket)
{
	__shared__ uint32_t s_front[2][ONE_FRONTIER];
	__shared__ uint32_t s_leaf[2][ONE_FRONTIER];
	const uint32_t lane = threadIdx.x;
	const char *const nodes = reinterpret_cast<const char *>(sc.nodes);
	const char *const tris = reinterpret_cast<const char *>(sc.tris);
	// (the ray travels in the kernel argument: a load from the host's pinned memory would be a PCIe round trip of ~2 us)
	const float ox = ray_in.origin.x, oy = ray_in.origin.y, oz = ray_in.origin.z, dx = ray_in.direction.x, dy = ray_in.direction.y, dz = ray_in.direction.z,
		tmin_ray = ray_in.min_t, tmax_ray = ray_in.max_t;
	// rtk.c:550-566 (as rtk_trace_kernel)
	const float ax_ = fabsf(dx), ay_ = fabsf(dy), az_ = fabsf(dz);
	const float m = sse_max(sse_max(ax_, ay_), az_);
	const bool kz0 = ax_ == m, kz1 = !kz0 && ay_ == m;
	const float dkx = kz0 ? dy : (kz1 ? dz : dx), dky = kz0 ? dz : (kz1 ? dx : dy), dkz = kz0 ? dx : (kz1 ? dy : dz);
	const float shx = -dkx / dkz, shy = -dky / dkz;
	const float sox = kz0 ? oy : (kz1 ? oz : ox), soy = kz0 ? oz : (kz1 ? ox : oy), soz = kz0 ? ox : (kz1 ? oy : oz);
	const float rdx = 1.0f / dx, rdy = 1.0f / dy, rdz = 1.0f / dz;      // rtk.c:410: true divides
	const float shz = kz0 ? rdx : (kz1 ? rdy : rdz);
	const uint32_t onx = (__float_as_uint(dx) >> 31) * 16u, ony = 32u + (__float_as_uint(dy) >> 31) * 16u, onz = 64u + (__float_as_uint(dz) >> 31) * 16u;
	float best_t = tmax_ray, best_u = 0.0f, best_v = 0.0f;
	uint32_t best_prim = RTK_PRIM_NONE;
	uint32_t n_cur = sc.num_nodes ? 1u : 0u, cur = 0u, n_leaf = 0u;
	bool not_done = false;
	if (lane == 0) s_front[0][0] = 0u;
	__syncthreads();
	// One round = one memory round trip: the nodes of the current level AND the leaves the previous level found are fetched and
	// tested together (leaves one lane each, then nodes one lane each); what a leaf's hit culls it culls one level later.
	while ((n_cur != 0u || n_leaf != 0u) && !not_done) {
		uint32_t n_next = 0u, n_leaf_next = 0u;
		const bool had_leaves = n_leaf != 0u;
		for (uint32_t base = 0; base < n_leaf; base += 64u)
			if (base + lane < n_leaf) one_leaf(tris, s_leaf[cur][base + lane], kz0, kz1, sox, soy, soz, shx, shy, shz, tmin_ray, tmax_ray, best_t, best_u, best_v, best_prim);
		for (uint32_t base = 0; base < n_cur; base += 64u) {
			const bool have = base + lane < n_cur;
			const uint32_t a_node = (have ? s_front[cur][base + lane] : 0u) << 7;
			f32x4 nx, fx, ny, fy, nz, fz;
			u32x4 ch;
			load_node(nodes, a_node + onx, (a_node + 16u) - onx, a_node + ony, (a_node + 80u) - ony, a_node + onz, (a_node + 144u) - onz, a_node,
				nx, fx, ny, fy, nz, fz, ch);
			const uint32_t ref[4] = { ch.x, ch.y, ch.z, ch.w };
			const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
			for (int i = 0; i < 4; i++) {
				// rtk.c:458-465: (bound - origin) * rcp_dir, the folded interval test with _mm_max_ps / _mm_min_ps operand order
				// (best_t here is the lane's own: at least as far as the wave's -- the test only gets more conservative)
				const float ax = (nx[i] - ox) * rdx, bx = (fx[i] - ox) * rdx;
				const float ay = (ny[i] - oy) * rdy, by = (fy[i] - oy) * rdy;
				const float az = (nz[i] - oz) * rdz, bz = (fz[i] - oz) * rdz;
				const float tn = sse_max(sse_max(ax, ay), sse_max(az, tmin_ray));
				const float tf = sse_min(sse_min(bx, by), sse_min(bz, best_t));
				const bool h = have && (tn <= tf) && ref[i] != RTK_REF_NONE;
				const bool leaf = (ref[i] & RTK_REF_LEAF) != 0u;
				const unsigned long long m_leaf = __builtin_amdgcn_ballot_w64(h && leaf), m_node = __builtin_amdgcn_ballot_w64(h && !leaf);
				if (h && leaf) { const uint32_t at = n_leaf_next + (uint32_t)__popcll(m_leaf & below); if (at < ONE_FRONTIER) s_leaf[cur ^ 1u][at] = ref[i] & 0x7fffffffu; }
				if (h && !leaf) { const uint32_t at = n_next + (uint32_t)__popcll(m_node & below); if (at < ONE_FRONTIER) s_front[cur ^ 1u][at] = ref[i]; }
				n_leaf_next += (uint32_t)__popcll(m_leaf);
				n_next += (uint32_t)__popcll(m_node);
			}
		}
		if (n_leaf_next > ONE_FRONTIER || n_next > ONE_FRONTIER) { not_done = true; break; }
		// the wave agrees on the best candidate (lowest t, lowest primitive id among equals)
		if (had_leaves) {
			float t_min = best_t;
			for (int o = 32; o > 0; o >>= 1) t_min = fminf(t_min, __shfl_xor(t_min, o));
			uint32_t p_min = best_t == t_min ? best_prim : RTK_PRIM_NONE;
			for (int o = 32; o > 0; o >>= 1) { const uint32_t q = (uint32_t)__shfl_xor((int)p_min, o); p_min = q < p_min ? q : p_min; }
			const unsigned long long owner = __builtin_amdgcn_ballot_w64(best_t == t_min && best_prim == p_min);
			const int src = owner ? (int)__builtin_ctzll(owner) : 0;
			best_u = __shfl(best_u, src);
			best_v = __shfl(best_v, src);
			best_t = t_min;
			best_prim = p_min;
		}
		cur ^= 1u;
		n_cur = n_next;
		n_leaf = n_leaf_next;
		__syncthreads();
	}
	if (lane == 0) {
		if (!not_done) {
			const bool hit = best_prim != RTK_PRIM_NONE && best_prim < sc.num_prims;
			*mask_out = hit ? 1 : 0;
			if (hit) {
				const uint32_t slot = sc.prim_slot[best_prim];
				const DevTri tr = sc.tris[slot];
				rtk_hit h;
				h.t = best_t; h.u = best_u; h.v = best_v;
				h.vertex[0].position.x = tr.v0[0]; h.vertex[0].position.y = tr.v0[1]; h.vertex[0].position.z = tr.v0[2];
				h.vertex[1].position.x = tr.v1[0]; h.vertex[1].position.y = tr.v1[1]; h.vertex[1].position.z = tr.v1[2];
				h.vertex[2].position.x = tr.v2[0]; h.vertex[2].position.y = tr.v2[1]; h.vertex[2].position.z = tr.v2[2];
				h.vertex[0].index = sc.vertex_index[3u * slot + 0u];
				h.vertex[1].index = sc.vertex_index[3u * slot + 1u];
				h.vertex[2].index = sc.vertex_index[3u * slot + 2u];
				h.mesh_index = sc.slot_mesh[slot];
				h.triangle_index = sc.slot_tri[slot];
				*hit_out = h;
			}
		}
		__threadfence_system();
		__hip_atomic_store(status_out, ((unsigned long long)ticket << 32) | (not_done ? RTK_ONE_NOT_DONE : 0ull), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
	}
}

// ------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------

namespace {

typedef void (*trace_kernel_fn)(TraceParams);

// variant index: any_hit | counted << 1 | filtered << 2 | compressed nodes << 3
trace_kernel_fn trace_variant(int v)
{
	switch (v) {
	case 0: return rtk_trace_kernel<0, false, false, false>;
	case 1: return rtk_trace_kernel<1, false, false, false>;
	case 2: return rtk_trace_kernel<0, true, false, false>;
	case 3: return rtk_trace_kernel<1, true, false, false>;
	case 4: return rtk_trace_kernel<0, false, true, false>;
	case 5: return rtk_trace_kernel<1, false, true, false>;
	case 6: return rtk_trace_kernel<0, true, true, false>;
	case 7: return rtk_trace_kernel<1, true, true, false>;
	case 8: return rtk_trace_kernel<0, false, false, true>;
	case 9: return rtk_trace_kernel<1, false, false, true>;
	case 10: return rtk_trace_kernel<0, true, false, true>;
	case 11: return rtk_trace_kernel<1, true, false, true>;
	case 12: return rtk_trace_kernel<0, false, true, true>;
	case 13: return rtk_trace_kernel<1, false, true, true>;
	case 14: return rtk_trace_kernel<0, true, true, true>;
	case 15: return rtk_trace_kernel<1, true, true, true>;
	case 16: return rtk_trace_kernel<2, false, true, false>;      // collect the k closest candidates (host-callback filters)
	default: return rtk_trace_kernel<2, false, true, true>;
	}
}

// resident workgroups per CU of each kernel variant, per device; filled on first use
std::mutex g_occ_mutex;
int g_occ[RTK_MAX_DEVICES][NUM_VARIANTS];

int blocks_per_cu_of(int device, int variant)
{
	std::lock_guard<std::mutex> lock(g_occ_mutex);
	if (device < 0 || device >= RTK_MAX_DEVICES) device = 0;
	int &o = g_occ[device][variant];
	if (o == 0) {
		int nb = 0;
		if (variant >= VARIANT_PACKET) nb = rtk_packet_occupancy(variant == VARIANT_PACKET_COUNTED);
		else if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, trace_variant(variant), BLOCK_THREADS, 0) != hipSuccess) nb = 0;
		o = nb >= 1 ? nb : 1;
	}
	return o;
}

// The scratch set of (scene, stream). Called with ds->scratch_mutex held.
// ---- is the batch a row-major image nobody told us about? (the reference's interface has no notion of an image, rtk.h:129; a host
// that only hands over rays should still get the packet kernels: VERDICT round 4, item 5)
// Along a row of an image the step from one ray to the next (origin and direction, six numbers) changes slowly; from the last ray
// of a row to the first of the next it jumps by about a row's width. k_detect_row finds the first such jump among the first
// 2^17 rays: the candidate width. k_detect_check then looks at up to 256 row ends (there must be a jump at every one) and at
// places inside rows (there must be none). A wrong guess can only cost speed -- tiles whose rays do not form a beam are handed
// back by the packet kernels, records are the same on every path -- so this is a heuristic with a cheap test, not a proof.
#define RTK_DETECT_WORDS 4
#define RTK_DETECT_WORD (RTK_ERROR_WORD + 1)
__device__ __forceinline__ bool ray_step_jumps(const rtk_ray *rays, size_t i)
{
	// rays i-1, i, i+1: does the step i -> i+1 differ from the step i-1 -> i by more than eight times the latter?
	const float *a = reinterpret_cast<const float *>(rays + i - 1), *b = reinterpret_cast<const float *>(rays + i), *c = reinterpret_cast<const float *>(rays + i + 1);
	float m = 0.0f, dmax = 0.0f;
#pragma unroll
	for (int k = 0; k < 6; k++) {
		const float s0 = b[k] - a[k], s1 = c[k] - b[k];
		m = fmaxf(m, fabsf(s0));
		dmax = fmaxf(dmax, fabsf(s1 - s0));
	}
	return !(dmax <= 8.0f * m);          // (NaN anywhere: a jump)
}

__global__ void k_detect_row(const rtk_ray *rays, uint32_t limit, uint32_t *first_jump)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x + 1u;
	if (i + 1u >= limit) return;
	if (ray_step_jumps(rays, i)) atomicMin(first_jump, i);
}

// word[0] = first jump (set by k_detect_row). One workgroup: up to 256 rows' ends must jump, places inside those rows must not;
// the verdict goes straight into host-visible memory (verdict[0] = width or 0, verdict[1] = height): no copy behind the kernel.
__global__ void __launch_bounds__(256) k_detect_check(const rtk_ray *rays, unsigned long long n, const uint32_t *word, uint32_t *verdict)
{
	__shared__ uint32_t s_bad;
	if (threadIdx.x == 0) s_bad = 0u;
	__syncthreads();
	const uint32_t w = word[0] + 1u;                                      // candidate width
	const bool candidate = word[0] != 0xffffffffu && w >= 64u && (n % w) == 0ull && n / w >= 2ull && n / w <= 0xffffffffull;
	if (candidate) {
		const unsigned long long rows = n / w;
		const unsigned long long stride = rows > 256ull ? rows / 256ull : 1ull;
		const unsigned long long r = (unsigned long long)threadIdx.x * stride;
		if (r + 1ull < rows) {
			const size_t end = (size_t)((r + 1ull) * w - 1ull);
			bool bad = !ray_step_jumps(rays, end);
			for (uint32_t q = 1; q < 4u; q++) bad = bad || ray_step_jumps(rays, (size_t)(r * w) + (size_t)q * (w / 4u));
			if (bad) atomicAdd(&s_bad, 1u);
		}
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		const bool ok = candidate && s_bad == 0u;
		verdict[0] = ok ? w : 0u;
		verdict[1] = ok ? (uint32_t)(n / w) : 0u;
		__threadfence_system();
	}
}

LaunchScratch *scratch_for(rtk_dev_scene *ds, hipStream_t stream)
{
	for (LaunchScratch *s : ds->scratch) if (s->stream == stream) return s;
	LaunchScratch *s = new LaunchScratch();
	s->stream = stream;
	// (cleared ON THE LAUNCH STREAM: a hipMemset goes to the NULL stream, which non-blocking streams do not wait for -- behind
	// another thread's device build there it ran milliseconds late, and a first launch read a stale error word: an intermittent
	// "traversal stack overflow" in test_builds_and_traces_from_several_threads_at_once)
	if (hipMalloc(&s->d_counter, (RTK_COUNTER_WORDS + 1 + RTK_DETECT_WORDS) * sizeof(unsigned long long)) != hipSuccess ||
		hipMemsetAsync(s->d_counter, 0, (RTK_COUNTER_WORDS + 1 + RTK_DETECT_WORDS) * sizeof(unsigned long long), stream) != hipSuccess) {
		rtk_set_error("rtk_dev_trace: out of device memory (launch scratch)");
		delete s;
		return nullptr;
	}
	ds->scratch.push_back(s);
	return s;
}

} // namespace

// ---- the hand-written kernels' code objects (AsmModule, rtk_trace_shared.h). The per-lane ones (rtk_lane_hot.S) belong to this file.
#include "rtk_lane_hot_image.h"

const TraceKnobs &rtk_trace_knobs()
{
	static const TraceKnobs knobs = [] {
		const auto env = [](const char *name, int value) { const char *v = getenv(name); return v ? atoi(v) : value; };
		TraceKnobs k;
		k.detect_image = env("RTK_AMD_DETECT_IMAGE", k.detect_image);
		k.tile_blocks = env("RTK_AMD_TILE_BLOCKS", k.tile_blocks);
		k.any_packets = env("RTK_AMD_ANY_PACKETS", k.any_packets);
		k.qnodes = env("RTK_AMD_QNODES", k.qnodes);
		k.packet_asm = env("RTK_AMD_PACKET_ASM", k.packet_asm);
		// (a number below 0 is the C++ kernel, one above 2 is 2: the counting and any-hit forms are not for choosing)
		const int wanted = env("RTK_AMD_PACKET_BEAM", (int)k.packet_beam);
		k.packet_beam = wanted < 0 ? PacketKernel::Cpp : wanted > (int)PacketKernel::Beam2 ? PacketKernel::Beam2 : (PacketKernel)wanted;
		k.log_path = getenv("RTK_AMD_LOG_PATH") != nullptr;
		k.lane_asm = env("RTK_AMD_LANE_ASM", k.lane_asm);
		k.lane_lds = (size_t)env("RTK_AMD_LANE_LDS", (int)k.lane_lds);
		k.sort_cell_bits = (uint32_t)env("RTK_AMD_SORT_CELL_BITS", (int)k.sort_cell_bits);
		k.sort_octant = (uint32_t)env("RTK_AMD_SORT_OCTANT", (int)k.sort_octant);
		k.sort_key = env("RTK_AMD_SORT_KEY", k.sort_key);
		k.packet_entries = env("RTK_AMD_PACKET_ENTRIES", k.packet_entries);
		k.entry_target = (unsigned)env("RTK_AMD_ENTRY_TARGET", (int)k.entry_target);
		k.entry_levels = (unsigned)env("RTK_AMD_ENTRY_LEVELS", (int)k.entry_levels);
		k.hot_blocks_per_cu = env("RTK_AMD_HOT_BLOCKS_PER_CU", k.hot_blocks_per_cu);
		k.lane_stats = env("RTK_AMD_LANE_STATS", k.lane_stats);
		k.lane_blocks = env("RTK_AMD_LANE_BLOCKS", k.lane_blocks);
		return k;
	}();
	return knobs;
}

AsmModule &rtk_lane_module()
{
	// 80 VGPRs, 30 KB of LDS per workgroup: five workgroups per CU; the any-hit kernel is launched on the same figure
	static const AsmKernel table[4] = { { "rtk_lane_hot_closest", rtk_trace_knobs().lane_blocks }, { "rtk_lane_hot_any", 0 },
		{ "rtk_lane_hot_closest_listed", 0 }, { "rtk_lane_hot_any_listed", 0 } };
	static AsmModule m(rtk_lane_hot_image, table, 4, "rtk_dev_trace: the assembly per-lane kernels are not loaded");
	return m;
}

const AsmModule::Loaded *AsmModule::on(int device)
{
	if (device < 0 || device >= RTK_MAX_DEVICES) return nullptr;
	std::lock_guard<std::mutex> lock(mutex);
	Loaded &h = slot[device];
	if (!h.tried) {
		int cur = -1;
		if (hipGetDevice(&cur) != hipSuccess || cur != device) return nullptr;
		h.tried = true;
		if (hipModuleLoadData(&h.mod, image) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
		for (int k = 0; k < count; k++) {
			if (hipModuleGetFunction(&h.fn[k], h.mod, table[k].name) != hipSuccess) { (void)hipGetLastError(); h.fn[k] = nullptr; continue; }
			if (table[k].cap == 0) continue;
			int nb = 0;
			if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&nb, h.fn[k], TRACE_BLOCK_THREADS, 0) != hipSuccess || nb < 1) nb = 1;
			h.blocks_per_cu[k] = nb > table[k].cap ? table[k].cap : nb;
		}
	}
	return h.fn[0] ? &h : nullptr;
}

int AsmModule::launch(int device, int kernel, void *params, size_t size, unsigned blocks, hipStream_t stream)
{
	const Loaded *h = on(device);
	if (!h || kernel < 0 || kernel >= count || !h->fn[kernel]) { rtk_set_error("%s", not_loaded); return RTK_AMD_ERR_HIP; }
	void *config[] = { HIP_LAUNCH_PARAM_BUFFER_POINTER, params, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END };
	RTK_HIP_CHECK(hipModuleLaunchKernel(h->fn[kernel], blocks, 1, 1, TRACE_BLOCK_THREADS, 1, 1, 0, stream, nullptr, config), RTK_AMD_ERR_HIP);
	return RTK_AMD_OK;
}

void rtk_scratch_free(LaunchScratch *s)
{
	if (!s) return;
	if (s->d_counter) (void)hipFree(s->d_counter);
	if (s->h_verdict) (void)hipHostFree((void *)s->h_verdict);
	if (s->d_spill) (void)hipFree(s->d_spill);
	if (s->d_sort) (void)hipFree(s->d_sort);
	if (s->d_leftover) (void)hipFree(s->d_leftover);
	if (s->d_entries) (void)hipFree(s->d_entries);
	if (s->d_select) (void)hipFree(s->d_select);
	delete s;
}

// *w, *h = the image the batch is (row-major, w * h = n), or 0, 0. Two small launches and a wait for `stream`.
int rtk_detect_image(const rtk_dev_scene *ds_c, const rtk_ray *d_rays, size_t n, hipStream_t stream, uint32_t *w_out, uint32_t *h_out)
{
	rtk_dev_scene *ds = const_cast<rtk_dev_scene *>(ds_c);
	*w_out = *h_out = 0u;
	if (!ds || !d_rays || n < 4u || n > 0x40000000ull) return RTK_AMD_OK;
	// (the look uses two words of the (scene, stream) scratch set and its pinned verdict: the scene's scratch mutex is held until the
	// verdict has been read, so that two host threads feeding one stream cannot interleave their looks; ~30 us)
	std::lock_guard<std::mutex> lock(ds->scratch_mutex);
	LaunchScratch *sc0 = scratch_for(ds, stream);
	if (!sc0) return RTK_AMD_ERR_OOM;
	uint32_t *d_word = reinterpret_cast<uint32_t *>(sc0->d_counter + RTK_DETECT_WORD);
	if (!sc0->h_verdict) RTK_HIP_CHECK(hipHostMalloc((void **)&sc0->h_verdict, 64, hipHostMallocDefault), RTK_AMD_ERR_OOM);     // (pinned: the kernel writes the verdict there)
	volatile uint32_t *h_verdict = sc0->h_verdict;
	const uint32_t limit = (uint32_t)std::min<size_t>(n, (size_t)1 << 17);
	RTK_HIP_CHECK(hipMemsetAsync(d_word, 0xff, 4, stream), RTK_AMD_ERR_HIP);
	hipLaunchKernelGGL(k_detect_row, dim3((limit + 255u) / 256u), dim3(256), 0, stream, d_rays, limit, d_word);
	hipLaunchKernelGGL(k_detect_check, dim3(1), dim3(256), 0, stream, d_rays, (unsigned long long)n, d_word, const_cast<uint32_t *>(h_verdict));
	RTK_HIP_CHECK(hipGetLastError(), RTK_AMD_ERR_HIP);
	RTK_HIP_CHECK(hipStreamSynchronize(stream), RTK_AMD_ERR_HIP);
	*w_out = h_verdict[0];
	*h_out = h_verdict[1];
	return RTK_AMD_OK;
}

namespace {

// the scene's memory, its scratch and the stream must all belong to the device this thread has current: a launch from a
// thread on another GPU would read the scene across devices (a fault without peer access)
bool on_scene_device(const rtk_dev_scene *ds, const char *caller)
{
	int cur = -1;
	if (hipGetDevice(&cur) == hipSuccess && cur == ds->device) return true;
	rtk_set_error("%s: the scene lives on device %d, the calling thread's current device is %d", caller, ds->device, cur);
	return false;
}

// the kernels address nodes and triangles as SGPR base + 32-bit byte offset
bool within_4gib(const DevSceneView &v)
{
	return (uint64_t)v.num_nodes * 128u <= 0xffffff00ull && (uint64_t)v.num_tris * RTK_TRI_STRIDE <= 0xffffff00ull;
}

DeviceKernels device_kernels(int device)
{
	DeviceKernels dk;
	if (const AsmModule::Loaded *h = rtk_packet_module().on(device)) {
		for (int k = 0; k < NUM_PACKET_KERNELS; k++) {
			dk.packet[k] = h->fn[k] != nullptr;
			dk.packet_blocks_per_cu[k] = h->blocks_per_cu[k > (int)PacketKernel::Beam2 ? (int)PacketKernel::Beam2 : k];
		}
	}
	if (const AsmModule::Loaded *h = rtk_lane_module().on(device)) {
		dk.lane = h->fn[0] && h->fn[1];
		dk.lane_listed = h->fn[2] && h->fn[3];
		dk.lane_blocks_per_cu = h->blocks_per_cu[0];
	}
	return dk;
}

// A scratch buffer of (scene, stream) that holds `need` units in `bytes` bytes, grown on demand.
int grow(void **ptr, size_t *capacity, size_t need, size_t bytes, hipStream_t stream)
{
	if (*capacity >= need) return RTK_AMD_OK;
	// an earlier launch on this stream may still be using the old area
	if (*ptr) { RTK_HIP_CHECK(hipStreamSynchronize(stream), RTK_AMD_ERR_HIP); (void)hipFree(*ptr); }
	*ptr = nullptr;
	*capacity = 0;
	RTK_HIP_CHECK(hipMalloc(ptr, bytes), RTK_AMD_ERR_OOM);
	*capacity = need;
	return RTK_AMD_OK;
}

int grow_scratch(LaunchScratch *sc, const TracePlan &plan, size_t n, hipStream_t stream)
{
	int rc = RTK_AMD_OK;
	if (plan.spill_cap && (sc->spill_lanes < plan.spill_lanes || sc->spill_entries_per_lane < plan.spill_cap)) {
		sc->spill_lanes = sc->spill_entries_per_lane = 0;       // (two measures: made anew when either is short)
		rc = grow((void **)&sc->d_spill, &sc->spill_lanes, plan.spill_lanes, plan.spill_lanes * plan.spill_cap * sizeof(uint2), stream);
		if (rc == RTK_AMD_OK) sc->spill_entries_per_lane = plan.spill_cap;
	}
	// [words_a | words_b] 8 B each, bounds 6 words + sort scratch
	if (rc == RTK_AMD_OK && plan.sort_rays) rc = grow(&sc->d_sort, &sc->sort_capacity, n, n * 16 + (rtk_sort_scratch_words((uint32_t)n) + 16) * 4, stream);
	if (rc == RTK_AMD_OK && plan.entries) {
		const size_t nblk = (size_t)(plan.image_w >> 6) * (plan.image_h >> 6);
		rc = grow(&sc->d_entries, &sc->entries_capacity, nblk, nblk * sizeof(PkBlockEntries), stream);
	}
	// one list serves both hand-overs: tile numbers (4 bytes each) or one 8-byte word per left-over ray
	const size_t left_bytes = plan.hot ? (n >> 6) * sizeof(uint32_t) : plan.lane_hot ? n * sizeof(unsigned long long) : 0;
	if (rc == RTK_AMD_OK) rc = grow((void **)&sc->d_leftover, &sc->leftover_capacity, left_bytes, left_bytes, stream);
	return rc;
}

// optional ray reordering pre-pass (per-lane kernels only): *perm = the order to trace the rays in
int enqueue_sort(const rtk_dev_scene *ds, LaunchScratch *sc, const rtk_ray *d_rays, size_t n, const TraceKnobs &knobs, hipStream_t stream, const unsigned long long **perm)
{
	const uint32_t n32 = (uint32_t)n;
	unsigned long long *keys_a = (unsigned long long *)sc->d_sort, *keys_b = keys_a + sc->sort_capacity;
	uint32_t *bounds = (uint32_t *)(keys_b + sc->sort_capacity), *scratch = bounds + 16;
	const uint32_t cell_bits = knobs.sort_cell_bits, with_octant = knobs.sort_octant;
	if (knobs.sort_key && ds->view.num_nodes) {
		hipLaunchKernelGGL(rtk_ray_entry_keys_kernel, dim3((n32 + 255u) / 256u), dim3(256), 0, stream, d_rays, n32, ds->view.nodes, keys_a,
			cell_bits, with_octant);
	} else {
		static const uint32_t init[6] = { 0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u };
		RTK_HIP_CHECK(hipMemcpyAsync(bounds, init, sizeof(init), hipMemcpyHostToDevice, stream), RTK_AMD_ERR_HIP);
		hipLaunchKernelGGL(rtk_ray_bounds_kernel, dim3((unsigned)(ds->num_cus * 2)), dim3(256), 0, stream, d_rays, (unsigned long long)n,
			(unsigned long long)(n >= (1u << 16) ? 61 : 1), bounds);
		hipLaunchKernelGGL(rtk_ray_keys_kernel, dim3((n32 + 255u) / 256u), dim3(256), 0, stream, d_rays, n32, bounds, keys_a,
			cell_bits, with_octant);
	}
	// one 8-byte word per ray (key over the ray's number), no value array: two passes of 16 B per ray
	const bool in_b = rtk_sort_words_async(keys_a, keys_b, n32, 32u, 32u + 3u * cell_bits + (with_octant ? 3u : 0u), scratch, stream);
	*perm = in_b ? keys_b : keys_a;
	return RTK_AMD_OK;
}

// The four ways a batch is traced. `p` is complete; each enqueues on `stream` and leaves launch errors to the caller's hipGetLastError.

// a hand-written packet kernel, then the C++ kernel on the tiles it handed back (mixed signs or axes, untame rays, a big leaf, a deep stack)
int enqueue_packet_hot(const rtk_dev_scene *ds, LaunchScratch *sc, TraceParams &p, const TracePlan &plan, bool any_hit, bool pk_counted, hipStream_t stream)
{
	const size_t tiles = (size_t)p.n >> 6;
	PkHotParams hp = {};
	hp.nodes = p.sc.nodes; hp.tris = p.sc.tris; hp.rays = p.rays; hp.hits = any_hit ? reinterpret_cast<rtk_hit_record *>(p.occluded) : p.hits; hp.counter = p.counter; hp.leftover = sc->d_leftover;
	hp.num_blocks = (uint32_t)(tiles >> 6);
	hp.image_w = p.image_w;
	hp.blocks_per_row = p.image_w >> 6;
	hp.bpr_magic = (uint32_t)((0x100000000ull + hp.blocks_per_row - 1u) / hp.blocks_per_row);
	hp.bound_abs = ds->tree.bound_abs > 1.0f ? ds->tree.bound_abs : 1.0f;
	hp.entries = p.entries;
	const int rc = rtk_packet_module().launch(ds->device, (int)plan.kernel, &hp, sizeof(hp), (unsigned)plan.hot_grid, stream);
	if (rc != RTK_AMD_OK) return rc;
	// (a small grid: the list is empty for most batches, and a launch that only finds that out should cost next to nothing)
	p.tile_list = sc->d_leftover;
	const size_t left_blocks = std::min<size_t>(plan.grid, (size_t)ds->num_cus * 2u);
	rtk_packet_launch(p, (unsigned)left_blocks, stream, pk_counted);      // (counting: the handed-back tiles' steps are counted too)
	return RTK_AMD_OK;
}

// a hand-written per-lane kernel, then rtk_trace_kernel on the rays it left over
int enqueue_lane_hot(const rtk_dev_scene *ds, LaunchScratch *sc, const TraceParams &p, const TracePlan &plan, bool any_hit, bool refill_given,
	const TraceKnobs &knobs, hipStream_t stream)
{
	LnHotListedParams lhp = {};
	LnHotParams &hp = lhp.hot;
	hp.qnodes = p.sc.qnodes; hp.tris = p.sc.tris; hp.rays = p.rays;
	hp.out = any_hit ? (void *)p.occluded : (void *)p.hits;
	hp.counter = p.counter;
	hp.leftover = reinterpret_cast<unsigned long long *>(sc->d_leftover);
	hp.perm = p.perm;
	hp.n = (uint32_t)p.n;
	// (re-swept for these kernels: refill at 16 idle lanes instead of 8 is +1 % / +2 %, profiles/r04_lane_sweep.log)
	hp.refill_min = refill_given ? p.refill_min : 16u;
	hp.node_exit = p.node_exit;
	hp.bound_abs = ds->tree.bound_raw;             // (no floor of 1: these kernels test child words, not inverted boxes)
	hp.spill = p.spill;
	hp.spill_stride = p.spill_stride;
	hp.spill_cap = p.spill_cap;
	// (a listed batch: the kernel reads how many entries of `perm` -- or how many of the rays themselves -- it traces)
	lhp.count = p.n_indirect;
	const int rc = p.n_indirect ? rtk_lane_module().launch(ds->device, any_hit ? 3 : 2, &lhp, sizeof(lhp), (unsigned)plan.lane_grid, stream)
		: rtk_lane_module().launch(ds->device, any_hit ? 1 : 0, &hp, sizeof(hp), (unsigned)plan.lane_grid, stream);
	if (rc != RTK_AMD_OK) return rc;
	if (knobs.lane_stats) {           // (diagnostics: how many rays the assembly kernel handed back; synchronises the stream)
		unsigned long long left = 0;
		(void)hipMemcpyAsync(&left, p.counter + RTK_LANE_LEFTOVER_WORD, sizeof(left), hipMemcpyDeviceToHost, stream);
		(void)hipStreamSynchronize(stream);
		fprintf(stderr, "rtk_lane_hot: %llu of %zu rays handed back (%.3f %%)\n", left, (size_t)p.n, 100.0 * (double)left / (double)p.n);
	}
	// (none in most batches: a small grid that finds an empty list costs next to nothing)
	TraceParams lp = p;
	lp.perm = hp.leftover;
	lp.n_indirect = p.counter + RTK_LANE_LEFTOVER_WORD;      // (never more than the p.n it is clamped to: a ray is handed back once)
	const size_t left_blocks = std::min<size_t>(plan.grid, (size_t)ds->num_cus);
	hipLaunchKernelGGL(trace_variant(plan.variant), dim3((unsigned)left_blocks), dim3(BLOCK_THREADS), 0, stream, lp);
	return RTK_AMD_OK;
}

int read_packet_counters(LaunchScratch *sc, size_t n, hipStream_t stream, rtk_packet_counters *out)
{
	unsigned long long c[16];
	RTK_HIP_CHECK(hipMemcpyAsync(c, sc->d_counter, sizeof(c), hipMemcpyDeviceToHost, stream), RTK_AMD_ERR_HIP);
	RTK_HIP_CHECK(hipStreamSynchronize(stream), RTK_AMD_ERR_HIP);
	out->pairs = c[11]; out->node_steps = c[12]; out->triangles_fetched = c[13]; out->triangle_group_tests = c[14];
	out->tiles_handed_back = c[RTK_LEFTOVER_COUNT_WORD];
	out->handed_back_node_steps = c[7]; out->handed_back_triangle_steps = c[8];
	out->tiles = n >> 6;
	return RTK_AMD_OK;
}

int read_counters(LaunchScratch *sc, hipStream_t stream, rtk_trace_counters *out)
{
	unsigned long long c[16], err = 0;
	RTK_HIP_CHECK(hipMemcpyAsync(c, sc->d_counter, sizeof(c), hipMemcpyDeviceToHost, stream), RTK_AMD_ERR_HIP);
	RTK_HIP_CHECK(hipMemcpyAsync(&err, sc->d_counter + RTK_ERROR_WORD, sizeof(err), hipMemcpyDeviceToHost, stream), RTK_AMD_ERR_HIP);
	RTK_HIP_CHECK(hipStreamSynchronize(stream), RTK_AMD_ERR_HIP);
	out->rays = c[1]; out->nodes = c[2]; out->leaves = c[3];
	out->triangles = c[4]; out->hits = c[5]; out->stack_spills = c[6];
	out->wave_node_steps = c[7]; out->wave_triangle_steps = c[8]; out->wave_rays = c[9];
	if (err) {
		(void)hipMemsetAsync(sc->d_counter + RTK_ERROR_WORD, 0, sizeof(err), stream);
		rtk_set_error("rtk_dev_trace: traversal stack overflow (corrupted scene)");
		return RTK_AMD_ERR_BAD_SCENE;
	}
	return RTK_AMD_OK;
}

} // namespace

LaunchScratch *rtk_scratch_for(rtk_dev_scene *ds, hipStream_t stream) { return scratch_for(ds, stream); }
int rtk_scratch_grow(void **ptr, size_t *capacity, size_t need, size_t bytes, hipStream_t stream) { return grow(ptr, capacity, need, bytes, stream); }

int rtk_launch_trace(const rtk_dev_scene *ds_c, const rtk_ray *d_rays, size_t n, rtk_hit_record *d_hits,
	uint8_t *d_occluded, const rtk_trace_opts *opts, hipStream_t stream, bool any_hit, rtk_trace_counters *counted,
	const rtk_dev_filter *filter, rtk_hit_record *d_cand, uint32_t *d_cand_count, uint32_t cand_k, rtk_packet_counters *pk_counted,
	const rtk_ray_list *list)
{
	rtk_dev_scene *ds = const_cast<rtk_dev_scene *>(ds_c);
	const bool collect = d_cand != nullptr;
	if (pk_counted && (counted || any_hit || filter || collect)) { rtk_set_error("rtk_dev_trace_rays_packet_counted: closest-hit batches only"); return RTK_AMD_ERR_BAD_ARG; }
	if (pk_counted) *pk_counted = rtk_packet_counters();
	if (collect && (!d_cand_count || cand_k == 0 || any_hit || counted)) { rtk_set_error("rtk_dev_trace: bad collect arguments"); return RTK_AMD_ERR_BAD_ARG; }
	if (!ds || (!d_rays && n) || (!collect && (any_hit ? !d_occluded : !d_hits) && n)) { rtk_set_error("rtk_dev_trace: bad argument"); return RTK_AMD_ERR_BAD_ARG; }
	// (a listed batch: rtk_dev_trace_rays*_listed have checked the list; n is the size of the arrays, below 2^32)
	if (list && (counted || pk_counted || collect)) { rtk_set_error("rtk_dev_trace: a ray list with a counted or collecting launch"); return RTK_AMD_ERR_BAD_ARG; }
	if (n == 0) { if (counted) *counted = rtk_trace_counters(); return RTK_AMD_OK; }
	if (!on_scene_device(ds, "rtk_dev_trace")) return RTK_AMD_ERR_BAD_ARG;
	if (!within_4gib(ds->view)) {
		rtk_set_error("rtk_dev_trace: scene exceeds 4 GiB of nodes or triangles (%u nodes, %u triangles)", ds->view.num_nodes, ds->view.num_tris);
		return RTK_AMD_ERR_UNSUPPORTED;
	}
	TraceParams p = {};
	p.sc = ds->view;
	p.rays = d_rays;
	p.hits = d_hits;
	p.occluded = d_occluded;
	p.cand = d_cand;
	p.cand_count = d_cand_count;
	p.cand_k = cand_k;
	p.n = n;
	if (list) { p.perm = reinterpret_cast<const unsigned long long *>(list->d_ids); p.n_indirect = reinterpret_cast<const unsigned long long *>(list->d_count); }
	if (filter) {
		if (filter->struct_size < sizeof(rtk_dev_filter)) { rtk_set_error("rtk_dev_trace: rtk_dev_filter.struct_size is too small"); return RTK_AMD_ERR_BAD_ARG; }
		if (filter->d_mesh_mask && filter->mesh_mask_bits == 0) { rtk_set_error("rtk_dev_trace: mesh mask without mesh_mask_bits"); return RTK_AMD_ERR_BAD_ARG; }
		p.mesh_mask = filter->d_mesh_mask;
		p.mesh_mask_bits = filter->mesh_mask_bits;
		p.ignore_prim = filter->d_ignore_prim;
		p.after = filter->d_after;
	}

	// what is asked, of which scene, on which device: the plan (rtk_trace_plan.h)
	const TraceKnobs &knobs = rtk_trace_knobs();
	const TraceOpts o = decode_opts(opts);
	TraceRequest rq;
	rq.n = n; rq.any_hit = any_hit; rq.counted = counted != nullptr; rq.pk_counted = pk_counted != nullptr; rq.collect = collect;
	rq.filtered = p.mesh_mask || p.ignore_prim || p.after; rq.has_filter = filter != nullptr;
	rq.listed = list != nullptr;
	SceneFacts facts;
	facts.num_nodes = ds->view.num_nodes; facts.num_tris = ds->view.num_tris; facts.has_qnodes = ds->view.qnodes != nullptr;
	facts.stack_entries = ds->tree.stack_entries(); facts.bound_abs = ds->tree.bound_abs; facts.big_leaf_fraction = ds->tree.big_leaf_fraction;
	facts.num_cus = ds->num_cus; facts.tri_stride = RTK_TRI_STRIDE;
	uint32_t look_w = 0, look_h = 0;
	if (wants_image_look(rq, o, facts, knobs)) {
		const int rc = rtk_detect_image(ds, d_rays, n, stream, &look_w, &look_h);
		if (rc != RTK_AMD_OK) return rc;
	}
	const DeviceKernels kernels = device_kernels(ds->device);
	const int occ = blocks_per_cu_of(ds->device, variant_of(rq, o, look_w, look_h, facts, kernels, knobs));
	const TracePlan plan = plan_trace(rq, o, look_w, look_h, facts, kernels, knobs, occ);
	if (plan.error != RTK_AMD_OK) { rtk_set_error("%s", plan.message); return plan.error; }
	if (knobs.log_path) fprintf(stderr, "rtk_dev_trace: n %zu image %u x %u packet %d hot %d beam %d opts %p flags %x\n", n, plan.image_w, plan.image_h, (int)plan.packet, (int)plan.hot, (int)plan.kernel, (const void *)opts, o.flags);
	p.dynamic = plan.dynamic;
	p.refill_min = plan.refill_min;
	p.node_exit = plan.node_exit;
	p.image_w = plan.image_w;
	p.image_h = plan.image_h;
	p.tile_blocks = plan.tile_blocks;

	// From here on the launch uses the scratch set of (scene, stream); the mutex is held until everything is
	// enqueued, so that two host threads feeding one stream cannot interleave "reset queue heads" and "launch".
	std::lock_guard<std::mutex> lock(ds->scratch_mutex);
	LaunchScratch *sc = scratch_for(ds, stream);
	if (!sc) return RTK_AMD_ERR_OOM;
	int rc = grow_scratch(sc, plan, n, stream);
	if (rc != RTK_AMD_OK) return rc;
	p.spill = sc->d_spill;
	p.spill_stride = (uint32_t)(plan.spill_cap ? sc->spill_lanes : 0);
	p.spill_cap = (uint32_t)plan.spill_cap;
	p.counter = sc->d_counter;
	if (plan.sort_rays && (rc = enqueue_sort(ds, sc, d_rays, n, knobs, stream, &p.perm)) != RTK_AMD_OK) return rc;
	// queue heads and visit counters start from zero; a one-block static launch uses neither. (With entry lists the pre-pass
	// kernel clears them itself: a 4.6 us fill kernel and its launch gap less per frame.)
	if ((plan.dynamic || plan.packet || counted) && !plan.entries) RTK_HIP_CHECK(hipMemsetAsync(sc->d_counter, 0, RTK_COUNTER_WORDS * sizeof(unsigned long long), stream), RTK_AMD_ERR_HIP);
	if (plan.entries) {
		rtk_packet_entries_launch(p, (PkBlockEntries *)sc->d_entries, ds->tree.bound_abs > 1.0f ? ds->tree.bound_abs : 1.0f, knobs.entry_target, knobs.entry_levels, stream);
		p.entries = (const PkBlockEntries *)sc->d_entries;
	}
	if (plan.hot) rc = enqueue_packet_hot(ds, sc, p, plan, any_hit, pk_counted != nullptr, stream);
	else if (plan.packet) rtk_packet_launch(p, (unsigned)plan.grid, stream, counted != nullptr);
	else if (plan.lane_hot) rc = enqueue_lane_hot(ds, sc, p, plan, any_hit, o.refill_given, knobs, stream);
	else hipLaunchKernelGGL(trace_variant(plan.variant), dim3((unsigned)plan.grid), dim3(BLOCK_THREADS), 0, stream, p);
	if (rc != RTK_AMD_OK) return rc;
	RTK_HIP_CHECK(hipGetLastError(), RTK_AMD_ERR_HIP);
	if (pk_counted && (rc = read_packet_counters(sc, n, stream, pk_counted)) != RTK_AMD_OK) return rc;
	if (counted) return read_counters(sc, stream, counted);
	return RTK_AMD_OK;
}

// rtk_dev_debug_packet_entries: the pre-pass of an image frame alone, on the null stream's scratch set, and its lists copied to the host
int rtk_debug_packet_entries(const rtk_dev_scene *ds_c, const rtk_ray *d_rays, uint32_t image_w, uint32_t image_h, uint32_t target, uint32_t max_levels, void *host_out)
{
	rtk_dev_scene *ds = const_cast<rtk_dev_scene *>(ds_c);
	if (!ds || !d_rays || !host_out) { rtk_set_error("rtk_dev_debug_packet_entries: NULL argument"); return RTK_AMD_ERR_BAD_ARG; }
	if (image_w == 0 || image_h == 0 || (image_w & 63u) || (image_h & 63u) || (unsigned long long)image_w * image_h > 0xffffffffull) {
		rtk_set_error("rtk_dev_debug_packet_entries: %u x %u is not an image of whole 64x64-pixel blocks", image_w, image_h);
		return RTK_AMD_ERR_BAD_ARG;
	}
	if (!on_scene_device(ds, "rtk_dev_debug_packet_entries")) return RTK_AMD_ERR_BAD_ARG;
	if (ds->view.num_nodes == 0) { rtk_set_error("rtk_dev_debug_packet_entries: the scene has no nodes"); return RTK_AMD_ERR_BAD_ARG; }
	const hipStream_t stream = nullptr;
	std::lock_guard<std::mutex> lock(ds->scratch_mutex);
	LaunchScratch *sc = scratch_for(ds, stream);
	if (!sc) return RTK_AMD_ERR_OOM;
	const size_t nblk = (size_t)(image_w >> 6) * (image_h >> 6);
	const int rc = grow(&sc->d_entries, &sc->entries_capacity, nblk, nblk * sizeof(PkBlockEntries), stream);
	if (rc != RTK_AMD_OK) return rc;
	TraceParams p = {};
	p.sc = ds->view;
	p.rays = d_rays;
	p.image_w = image_w;
	p.image_h = image_h;
	p.counter = sc->d_counter;
	rtk_packet_entries_launch(p, (PkBlockEntries *)sc->d_entries, ds->tree.bound_abs > 1.0f ? ds->tree.bound_abs : 1.0f, target, max_levels, stream);
	RTK_HIP_CHECK(hipGetLastError(), RTK_AMD_ERR_HIP);
	RTK_HIP_CHECK(hipMemcpyAsync(host_out, sc->d_entries, nblk * sizeof(PkBlockEntries), hipMemcpyDeviceToHost, stream), RTK_AMD_ERR_HIP);
	RTK_HIP_CHECK(hipStreamSynchronize(stream), RTK_AMD_ERR_HIP);
	return RTK_AMD_OK;
}

// Did any launch of this scene on `stream` since the last call overflow a traversal stack? Synchronises the stream.
int rtk_trace_status(const rtk_dev_scene *ds_c, hipStream_t stream)
{
	rtk_dev_scene *ds = const_cast<rtk_dev_scene *>(ds_c);
	if (!ds) { rtk_set_error("rtk_dev_trace_status: NULL scene"); return RTK_AMD_ERR_BAD_ARG; }
	// the error word's address is looked up under the lock; the wait for the stream happens outside it, so that threads
	// tracing one scene on their own streams do not queue up behind each other's synchronisation
	unsigned long long *word = nullptr;
	{
		std::lock_guard<std::mutex> lock(ds->scratch_mutex);
		for (LaunchScratch *s : ds->scratch) if (s->stream == stream) { word = s->d_counter + RTK_ERROR_WORD; break; }
	}
	if (!word) {
		RTK_HIP_CHECK(hipStreamSynchronize(stream), RTK_AMD_ERR_HIP);
		return RTK_AMD_OK;
	}
	unsigned long long e = 0;
	RTK_HIP_CHECK(hipMemcpyAsync(&e, word, sizeof(e), hipMemcpyDeviceToHost, stream), RTK_AMD_ERR_HIP);
	RTK_HIP_CHECK(hipStreamSynchronize(stream), RTK_AMD_ERR_HIP);
	if (e) {
		(void)hipMemsetAsync(word, 0, sizeof(e), stream);      // reported once
		rtk_set_error("rtk_dev_trace: traversal stack overflow (corrupted scene)");
		return RTK_AMD_ERR_BAD_SCENE;
	}
	return RTK_AMD_OK;
}

// A stream is going away (the host-pointer calls own one per thread): the scratch sets made for it are released, so that
// threads coming and going do not pile them up and a recycled stream handle never finds an old entry.
void rtk_scene_drop_stream(rtk_dev_scene *ds, hipStream_t stream)
{
	if (!ds) return;
	std::lock_guard<std::mutex> lock(ds->scratch_mutex);
	for (size_t i = 0; i < ds->scratch.size();) {
		if (ds->scratch[i]->stream == stream) { rtk_scratch_free(ds->scratch[i]); ds->scratch.erase(ds->scratch.begin() + (long)i); } else i++;
	}
}

int rtk_launch_expand(const rtk_dev_scene *ds_c, const rtk_hit_record *d_records, size_t n, rtk_hit *d_hits,
	uint8_t *d_mask, hipStream_t stream, unsigned long long *h_status, uint32_t ticket)
{
	rtk_dev_scene *ds = const_cast<rtk_dev_scene *>(ds_c);
	if (!ds || (!d_records && n)) { rtk_set_error("rtk_dev_expand_hits: bad argument"); return RTK_AMD_ERR_BAD_ARG; }
	if (n == 0) return RTK_AMD_OK;
	if (!on_scene_device(ds, "rtk_dev_expand_hits")) return RTK_AMD_ERR_BAD_ARG;
	if (d_hits && rtk_scene_side_arrays(ds, stream) != RTK_AMD_OK) return RTK_AMD_ERR_OOM;
	const unsigned long long *status_word = nullptr;
	if (h_status) {
		// the error word of the launches on this stream (rtk_launch_trace has made the scratch set)
		std::lock_guard<std::mutex> lock(ds->scratch_mutex);
		for (LaunchScratch *s : ds->scratch) if (s->stream == stream) status_word = s->d_counter + RTK_ERROR_WORD;
		if (!status_word) h_status = nullptr;
	}
	const size_t blocks = (n + 255) / 256;
	if (blocks != 1 || !h_status) ticket = 0u;             // the ticket is written by a lone workgroup after its results
	hipLaunchKernelGGL(rtk_expand_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, ds->view, d_records,
		(unsigned long long)n, d_hits, d_mask, status_word, h_status, ticket);
	RTK_HIP_CHECK(hipGetLastError(), RTK_AMD_ERR_HIP);
	return RTK_AMD_OK;
}

// rtk_trace_ray's own launch: ONE ray (read here, on the host: it travels in the kernel argument), one wave, the full rtk_hit and the mask written where the host
// reads them, then the ticket ((ticket << 32) | 0, or | 2 = "not done: take the batch path"). No scratch, no queue, no second launch.
int rtk_launch_trace_one(const rtk_dev_scene *ds, const rtk_ray *d_ray, rtk_hit *d_hit, uint8_t *d_mask, hipStream_t stream,
	unsigned long long *h_status, uint32_t ticket)
{
	if (!ds || !d_ray || !d_hit || !d_mask || !h_status || !ticket) { rtk_set_error("rtk_trace_ray: bad argument"); return RTK_AMD_ERR_BAD_ARG; }
	if (!on_scene_device(ds, "rtk_trace_ray")) return RTK_AMD_ERR_BAD_ARG;
	if (!within_4gib(ds->view)) {
		rtk_set_error("rtk_trace_ray: the one-ray kernel addresses nodes and triangles with 32-bit byte offsets (scene: %u nodes, %u triangles)", ds->view.num_nodes, ds->view.num_tris);
		return RTK_AMD_ERR_UNSUPPORTED;
	}
	if (rtk_scene_side_arrays(ds, stream) != RTK_AMD_OK) return RTK_AMD_ERR_OOM;
	hipLaunchKernelGGL(rtk_trace_one_kernel, dim3(1), dim3(64), 0, stream, ds->view, *d_ray, d_hit, d_mask, h_status, ticket);
	RTK_HIP_CHECK(hipGetLastError(), RTK_AMD_ERR_HIP);
	return RTK_AMD_OK;
}
