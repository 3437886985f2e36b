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
#include "rtk_trace_shared.h"

#include <math.h>

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

// ------------------------------------------------------------------------------------
// host side: the kernel's two doors (rtk_trace_shared.h)
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

} // namespace

int rtk_trace_occupancy(int device, int variant)
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

void rtk_trace_kernel_launch(int variant, const TraceParams &p, unsigned blocks, hipStream_t stream)
{
	hipLaunchKernelGGL(trace_variant(variant), dim3(blocks), dim3(BLOCK_THREADS), 0, stream, p);
}
