// rtk_world.hip -- rtk_dev_world: rays through placed copies of device scenes (rtk_amd.h, "Instanced worlds").
//
// THE OBJECT. A world borrows its scenes and owns three small tables and one ordinary rtk_dev_scene, the TOP TREE:
//   - per scene 24 bytes (DevWorldScene: nodes, triangle records and their counts), copied from the scene's view under its
//     scratch_mutex at create and at every update, with the scene's stack_entries on the host;
//   - per instance 64 bytes (DevWorldInstance: the inverse placement, the scene number, the dead flag) and the placement itself;
//   - per instance one proxy triangle (lo, hi, lo) of nine floats whose box is exactly the instance's padded world box
//     (rtk_world_rule.h). The top tree is rtk_dev_scene_build over that buffer as one mesh with implicit indices, so a proxy's
//     primitive id is the instance number; an update is rtk_dev_scene_refit on the same buffer, a rebuild rtk_dev_scene_rebuild.
//     No second builder: the top tree's memory is in its own ledger, the validator and the quality measure work on it as it is.
//     A world of ONE instance has a top tree of one triangle, which a build decodes on the host: that tree is made from a host
//     copy of the proxy, and made anew by update and rebuild.
// k_world_instances makes record and proxy, one lane per instance.
//
// THE WALK, k_world<ANY, COUNT, FILT>: rtk_sweep.hip's frame -- one ray per lane, a fixed grid of resident workgroups striding
// over the batch, 8-byte stack entries (reference, entry distance), WD_LDS_STACK per lane in LDS as [entry][lane], deeper ones in
// the spill area of the (top tree, stream) scratch set, a push that fits neither dropped and flagged in that set's error word.
//   Top level: the exact 128-byte nodes of the top tree, the reference's slab test with every box grown by the ray's margin e
// (rtk_world_margin), children near to far, a child entered behind the best t skipped (again at the pop). A top leaf is a run of
// proxy records: lo from v0, hi from v1, the instance from prim. A proxy whose grown box is entered and whose instance is live
// and passes the filter ENTERS THE INSTANCE: a sentinel entry (WD_REF_TOP, the next proxy slot of the leaf or none) is pushed,
// the ray is transformed by rtk_world_ray, the per-ray constants of the watertight test are made again (dominant axis, shear,
// reciprocal direction) and the instance's scene is walked from its root on the same stack. Popping the sentinel restores the
// world ray and goes on with the leaf.
//   Bottom level: the node step and the leaf rule of rtk_allhits.hip / rtk_trace_kernel, operation for operation: the exact-node
// slab test without a margin in the reference's operand order, far bound = the best t so far; strict min_t < t < max_t; groups of
// four, a partial last group in double, a full group scanned for an exact zero and then evaluated, in double if it has one. A
// candidate of an instance therefore has the bits rtk_dev_trace_rays gives for the transformed ray on that scene. Inside one
// instance the lowest primitive id wins among bit-equal t (rtk_trace_kernel's rule); ACROSS instances a candidate must be strictly
// closer, so of several instances that attain the same bits of t the one the walk meets first is kept.
//   Scene base pointers differ per lane: nodes and records are addressed by 64-bit per-lane pointers (plain loads; the seven
// 16-byte pieces of a node are requested back to back).
//
// FLOATING POINT: compiled with -ffp-contract=off like every traversal; the operation order of the triangle test is normative.
// Compiler's resource report (gfx950, -O3, kernel-resource-usage): WD_RESOURCES below.
#include "rtk_world_internal.h"    // struct rtk_dev_world, DevWorldScene, the WD_ constants, WD_PUSH, rtk_world_launch
#include "rtk_trace_shared.h"      // sse_min, sse_max
#include "rtk_world_rule.h"

#include <atomic>

// WD_RESOURCES (closest / any / closest FILT / any FILT / counting): VGPRs 95 / 89 / 97 / 90 / 102, scratch 0 and no VGPR spills in
// every form (48 to 70 SGPRs spill into VGPR lanes), LDS 32 768 B per workgroup: LDS places five workgroups of four waves on a CU,
// 5 waves per SIMD, and the registers allow 5 (up to 96 VGPRs) or 4. k_world_instances: 60 VGPRs, no LDS, no scratch.

namespace {

struct InstParams {
	DevWorldInstance *inst;
	const rtk_placement *place;
	float *proxy;
	const DevWorldScene *scenes;
	unsigned long long *dead;
	uint32_t num_instances, num_scenes;
};

// One lane per instance: the inverse, the padded world box of the scene's root, the proxy triangle
__global__ void __launch_bounds__(256) k_world_instances(InstParams p)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= p.num_instances) return;
	const uint32_t scene = p.inst[i].scene;
	float m[12], inv[12];
#pragma unroll
	for (int k = 0; k < 12; k++) m[k] = p.place[i].m[k];
	bool live = rtk_world_inverse(m, inv);
	float lo[3] = { 0.0f, 0.0f, 0.0f }, hi[3] = { 0.0f, 0.0f, 0.0f };
	bool any = false;
	if (live && scene < p.num_scenes) {
		const DevWorldScene sc = p.scenes[scene];
		if (sc.num_nodes != 0u && sc.num_tris != 0u) {
			// the root box: the union of node 0's non-empty child boxes
			const DevNode root = sc.nodes[0];
			float rlo[3] = { 0.0f, 0.0f, 0.0f }, rhi[3] = { 0.0f, 0.0f, 0.0f };
			for (int k = 0; k < 4; k++) {
				if (root.child[k] == RTK_REF_NONE) continue;
				const float l[3] = { root.bx[0][k], root.by[0][k], root.bz[0][k] }, h[3] = { root.bx[1][k], root.by[1][k], root.bz[1][k] };
				for (int a = 0; a < 3; a++) {
					rlo[a] = !any || l[a] < rlo[a] ? l[a] : rlo[a];
					rhi[a] = !any || h[a] > rhi[a] ? h[a] : rhi[a];
				}
				any = true;
			}
			if (any) any = rtk_world_box(rlo, rhi, m, lo, hi);
		}
	}
	live = live && any;
	if (!live) {
		// a point box at the placement's translation, at the origin if that is not finite; the walk never enters it
		const bool at = rtk_world_finite(m[3]) && rtk_world_finite(m[7]) && rtk_world_finite(m[11]);
		for (int a = 0; a < 3; a++) lo[a] = hi[a] = at ? m[4 * a + 3] : 0.0f;
		for (int k = 0; k < 12; k++) inv[k] = 0.0f;
		atomicAdd(p.dead, 1ull);
	}
	DevWorldInstance r;
	for (int k = 0; k < 12; k++) r.inv[k] = inv[k];
	r.scene = scene; r.flags = live ? 0u : WD_DEAD; r.pad[0] = r.pad[1] = 0u;
	p.inst[i] = r;
	float *q = p.proxy + (size_t)i * 9u;
	for (int a = 0; a < 3; a++) { q[a] = lo[a]; q[3 + a] = hi[a]; q[6 + a] = lo[a]; }
}

struct WorldParams {
	const DevNode *top_nodes;
	const DevTri *top_tris;
	uint32_t top_num_nodes, top_num_tris;
	const DevWorldInstance *inst;
	const DevWorldScene *scenes;
	uint32_t num_instances, num_scenes;
	float bound;                           // the largest |plane| of the top tree
	uint32_t n;
	const rtk_ray *rays;
	const unsigned long long *ids;         // or NULL: 0, 1, 2, ...
	const unsigned long long *count;       // or NULL: n
	rtk_hit_record *records;               // the closest form
	uint32_t *instances;                   // or NULL
	uint8_t *blocked;                      // the any-hit form
	const uint32_t *mask;                  // or NULL: bit i set = instance i is walked
	uint32_t mask_bits;
	const uint32_t *ignore_instance;       // or NULL: per ray slot
	unsigned long long *counter;           // the stream's counter words: [RTK_ERROR_WORD] is set by a dropped push
	uint2 *spill;                          // [entry][lane of the launch]
	uint32_t spill_stride;
	uint32_t spill_cap;                    // entries per lane
};

typedef float wd_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t wd_u32x4 __attribute__((ext_vector_type(4)));

// ascending by key; the reference travels with it
__device__ __forceinline__ void wd_cswap(float &ka, uint32_t &ra, float &kb, uint32_t &rb)
{
	const bool swap = kb < ka;
	const float k0 = swap ? kb : ka, k1 = swap ? ka : kb;
	const uint32_t r0 = swap ? rb : ra, r1 = swap ? ra : rb;
	ka = k0; kb = k1; ra = r0; rb = r1;
}

// The per-ray constants of the slab test and of the watertight test (rtk.c:550-566, 410), made for the world ray and again for
// every instance a ray enters
struct WdRay {
	float ox, oy, oz, rdx, rdy, rdz;
	float sox, soy, soz, shx, shy, shz;
	bool kz0, kz1, ngx, ngy, ngz;
};

__device__ __forceinline__ void wd_setup(float ox, float oy, float oz, float dx, float dy, float dz, WdRay &s)
{
	s.ox = ox; s.oy = oy; s.oz = oz;
	const float ax = fabsf(dx), ay = fabsf(dy), az = fabsf(dz);
	const float m = sse_max(sse_max(ax, ay), az);
	s.kz0 = ax == m;
	s.kz1 = !s.kz0 && ay == m;
	const float dkx = s.kz0 ? dy : (s.kz1 ? dz : dx);
	const float dky = s.kz0 ? dz : (s.kz1 ? dx : dy);
	const float dkz = s.kz0 ? dx : (s.kz1 ? dy : dz);
	s.shx = -dkx / dkz;
	s.shy = -dky / dkz;
	s.sox = s.kz0 ? oy : (s.kz1 ? oz : ox);
	s.soy = s.kz0 ? oz : (s.kz1 ? ox : oy);
	s.soz = s.kz0 ? ox : (s.kz1 ? oy : oz);
	s.rdx = 1.0f / dx; s.rdy = 1.0f / dy; s.rdz = 1.0f / dz;      // rtk.c:410: true divides
	s.shz = s.kz0 ? s.rdx : (s.kz1 ? s.rdy : s.rdz);
	// near and far plane by the direction's sign BIT (rtk.c:152-154, 458-463)
	s.ngx = (__float_as_uint(dx) >> 31) != 0u; s.ngy = (__float_as_uint(dy) >> 31) != 0u; s.ngz = (__float_as_uint(dz) >> 31) != 0u;
}

// ANY: one byte per ray, retired at the first candidate. COUNT: the visit counts of rtk_dev_world_trace_rays_counted. FILT: the
// instance mask and the per-ray ignored instance
template <bool ANY, bool COUNT, bool FILT>
__global__ void __launch_bounds__(WD_THREADS) k_world(WorldParams p)
{
	__shared__ uint2 s_stack[WD_WAVES][WD_LDS_STACK][64];

	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint2 (*stk)[64] = s_stack[wave];
	const uint32_t glane = blockIdx.x * WD_THREADS + threadIdx.x;
	uint32_t m = p.n;
	if (p.count) { const unsigned long long listed = *p.count; m = listed < p.n ? (uint32_t)listed : p.n; }
	const unsigned long long step = (unsigned long long)gridDim.x * WD_THREADS;
	uint32_t c_rays = 0, c_nodes = 0, c_leaves = 0, c_tris = 0, c_hits = 0, c_spills = 0;

	for (unsigned long long qi = glane; qi < m; qi += step) {
		const uint32_t r = p.ids ? (uint32_t)p.ids[qi] : (uint32_t)qi;
		if (r >= p.n) continue;                                   // (the caller's error; nothing is read or written out of range)
		// (the ray as scalars: kept as an array, the selects of the dominant axis become indexed reads of a copy in scratch memory)
		const wd_f32x4 *src = reinterpret_cast<const wd_f32x4 *>(p.rays + r);
		const wd_f32x4 r0 = __builtin_nontemporal_load(src), r1 = __builtin_nontemporal_load(src + 1);
		const float wox = r0.x, woy = r0.y, woz = r0.z, wdx = r0.w, wdy = r1.x, wdz = r1.y;
		const float tmin_ray = r1.z, tmax_ray = r1.w;
		float e;
		{ const float org[3] = { wox, woy, woz }; e = rtk_world_margin(org, p.bound); }
		const uint32_t skip_inst = (FILT && p.ignore_instance) ? p.ignore_instance[r] : RTK_PRIM_NONE;
		WdRay s;
		wd_setup(wox, woy, woz, wdx, wdy, wdz, s);
		float best_t = tmax_ray, best_u = 0.0f, best_v = 0.0f;
		uint32_t best_prim = RTK_PRIM_NONE, best_inst = RTK_PRIM_NONE;
		// where the walk is: the top tree (in_inst false), or the scene of instance cur_inst
		bool in_inst = false;
		uint32_t cur_inst = RTK_PRIM_NONE;
		const char *nodes = reinterpret_cast<const char *>(p.top_nodes), *tris = reinterpret_cast<const char *>(p.top_tris);
		uint32_t num_nodes = p.top_num_nodes, num_tris = p.top_num_tris;
		uint32_t top = (p.top_num_nodes != 0u && p.top_num_tris != 0u) ? 0u : RTK_REF_NONE;
		uint32_t sp = 0;
		if (COUNT) c_rays++;

		while (top != RTK_REF_NONE) {
			if ((int32_t)top >= 0) {
				// ------------------------------------------------------------ node, of the top tree or of a scene
				if (top < num_nodes) {
					const wd_f32x4 *nd = reinterpret_cast<const wd_f32x4 *>(nodes + (size_t)top * 128u);
					const wd_f32x4 xl = nd[0], xh = nd[1], yl = nd[2], yh = nd[3], zl = nd[4], zh = nd[5];
					const wd_u32x4 ch = *reinterpret_cast<const wd_u32x4 *>(nd + 6);
					if (COUNT) c_nodes++;
					// the top tree's boxes are grown by e on every side; a scene's are taken as they are
					const float g = in_inst ? 0.0f : e;
					float key[4];
					uint32_t ref[4];
#pragma unroll
					for (int k = 0; k < 4; k++) {
						const float nx = s.ngx ? xh[k] : xl[k], fx = s.ngx ? xl[k] : xh[k];
						const float ny = s.ngy ? yh[k] : yl[k], fy = s.ngy ? yl[k] : yh[k];
						const float nz = s.ngz ? zh[k] : zl[k], fz = s.ngz ? zl[k] : zh[k];
						bool enter;
						float tn;
						if (in_inst) {
							// rtk.c:458-465 with the operand order of _mm_max_ps / _mm_min_ps (decides what a NaN from 0 * inf does)
							const float ax = (nx - s.ox) * s.rdx, bx = (fx - s.ox) * s.rdx;
							const float ay = (ny - s.oy) * s.rdy, by = (fy - s.oy) * s.rdy;
							const float az = (nz - s.oz) * s.rdz, bz = (fz - s.oz) * s.rdz;
							tn = sse_max(sse_max(ax, ay), sse_max(az, tmin_ray));
							const float tf = sse_min(sse_min(bx, by), sse_min(bz, best_t));
							enter = tn <= tf;
						} else {
							// the near plane moves away from the box by g, the far plane too; a NaN product drops out of fmaxf / fminf: the
							// axis then decides nothing, which can only admit more
							const float ax = ((nx + (s.ngx ? g : -g)) - s.ox) * s.rdx, bx = ((fx + (s.ngx ? -g : g)) - s.ox) * s.rdx;
							const float ay = ((ny + (s.ngy ? g : -g)) - s.oy) * s.rdy, by = ((fy + (s.ngy ? -g : g)) - s.oy) * s.rdy;
							const float az = ((nz + (s.ngz ? g : -g)) - s.oz) * s.rdz, bz = ((fz + (s.ngz ? -g : g)) - s.oz) * s.rdz;
							tn = fmaxf(fmaxf(fmaxf(ax, ay), az), tmin_ray);
							const float tf = fminf(fminf(fminf(bx, by), bz), best_t);
							enter = tn <= tf;
						}
						enter = enter && ch[k] != RTK_REF_NONE;
						key[k] = enter ? (tn == tn ? tn : -INFINITY) : INFINITY;
						ref[k] = enter ? ch[k] : RTK_REF_NONE;
					}
					wd_cswap(key[0], ref[0], key[1], ref[1]);
					wd_cswap(key[2], ref[2], key[3], ref[3]);
					wd_cswap(key[0], ref[0], key[2], ref[2]);
					wd_cswap(key[1], ref[1], key[3], ref[3]);
					wd_cswap(key[1], ref[1], key[2], ref[2]);
					top = ref[0];
					// the others far to near. A push that fits neither LDS nor the spill area is dropped WITHOUT advancing sp and flagged
#pragma unroll
					for (int k = 3; k >= 1; k--) {
						if (ref[k] == RTK_REF_NONE) continue;
						const uint2 en = make_uint2(ref[k], __float_as_uint(key[k]));
						WD_PUSH(en);
					}
				} else top = RTK_REF_NONE;                            // (a child word beyond the array: not a tree; nothing is read)
			} else if (!in_inst) {
				// ------------------------------------------------------------ a leaf of the top tree: proxies up to RTK_TRI_LAST
				uint32_t slot = top & 0x7fffffffu;
				if (COUNT) c_leaves++;
				top = RTK_REF_NONE;
				while (slot < num_tris) {
					const wd_f32x4 *t = reinterpret_cast<const wd_f32x4 *>(tris + (size_t)slot * RTK_TRI_STRIDE);
					const wd_f32x4 A = t[0], B = t[1];
					const uint32_t inst = __float_as_uint(A.w), flags = __float_as_uint(B.w);
					const bool last = (flags & RTK_TRI_LAST) != 0u;
					if (COUNT) c_tris++;
					bool wanted = inst < p.num_instances;
					if (FILT) {
						wanted = wanted && inst != skip_inst;
						if (p.mask) wanted = wanted && inst < p.mask_bits && ((p.mask[inst >> 5] >> (inst & 31u)) & 1u);
					}
					if (wanted) {
						// lo is v0, hi is v1: the grown box against the world ray, as a node's slot
						const float ax = (((s.ngx ? B.x + e : A.x - e)) - s.ox) * s.rdx, bx = (((s.ngx ? A.x - e : B.x + e)) - s.ox) * s.rdx;
						const float ay = (((s.ngy ? B.y + e : A.y - e)) - s.oy) * s.rdy, by = (((s.ngy ? A.y - e : B.y + e)) - s.oy) * s.rdy;
						const float az = (((s.ngz ? B.z + e : A.z - e)) - s.oz) * s.rdz, bz = (((s.ngz ? A.z - e : B.z + e)) - s.oz) * s.rdz;
						const float tn = fmaxf(fmaxf(fmaxf(ax, ay), az), tmin_ray);
						const float tf = fminf(fminf(fminf(bx, by), bz), best_t);
						wanted = tn <= tf;
					}
					if (wanted) {
						const wd_u32x4 *ir = reinterpret_cast<const wd_u32x4 *>(p.inst + inst);
						const wd_u32x4 i3 = ir[3];
						wanted = (i3.y & WD_DEAD) == 0u && i3.x < p.num_scenes;
						if (wanted) {
							const DevWorldScene sc = p.scenes[i3.x];
							wanted = sc.num_nodes != 0u && sc.num_tris != 0u;
							if (wanted) {
								// ENTER: the sentinel remembers where the leaf goes on; the ray of this instance; its scene from the root
								const wd_f32x4 i0 = *reinterpret_cast<const wd_f32x4 *>(ir), i1 = *reinterpret_cast<const wd_f32x4 *>(ir + 1),
									i2 = *reinterpret_cast<const wd_f32x4 *>(ir + 2);
								const float inv[12] = { i0.x, i0.y, i0.z, i0.w, i1.x, i1.y, i1.z, i1.w, i2.x, i2.y, i2.z, i2.w };
								const uint2 en = make_uint2(WD_REF_TOP, last ? RTK_REF_NONE : slot + 1u);
								const uint32_t sp_before = sp;
								WD_PUSH(en);
								if (sp != sp_before) {                        // (a dropped sentinel: the instance is not entered, the error word says so)
									const float w[8] = { wox, woy, woz, wdx, wdy, wdz, tmin_ray, tmax_ray };
									float o[8];
									rtk_world_ray(inv, w, o);
									wd_setup(o[0], o[1], o[2], o[3], o[4], o[5], s);
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
				// ------------------------------------------------------------ a leaf of a scene: rtk.c's groups of four (rtk.c:212, 302-336)
				// as rtk_allhits_kernel takes them: a partial last group in double; a full group scanned for an exact zero, then evaluated
				const uint32_t slot0 = top & 0x7fffffffu;
				if (COUNT) c_leaves++;
				uint32_t i = 0, n = 1;
				bool force = false, scan = false, scanned = false, zero_in_group = false;
				while (i < n && slot0 + i < num_tris) {
					const wd_f32x4 *t = reinterpret_cast<const wd_f32x4 *>(tris + (size_t)(slot0 + i) * RTK_TRI_STRIDE);
					const wd_f32x4 A = t[0], B = t[1], C = t[2];
					if (i == 0u) n = __float_as_uint(C.w);          // leaf size rides in the first record
					if ((i & 3u) == 0u) {
						if (scanned) scanned = false;                      // second pass over the group: `force` is decided
						else { force = (n - i) < 4u; scan = !force; zero_in_group = false; }
					}
					// permute to (kx,ky,kz) and move the origin (rtk.c:232-280)
					const float v0x = (s.kz0 ? A.y : (s.kz1 ? A.z : A.x)) - s.sox;
					const float v0y = (s.kz0 ? A.z : (s.kz1 ? A.x : A.y)) - s.soy;
					const float v0z = (s.kz0 ? A.x : (s.kz1 ? A.y : A.z)) - s.soz;
					const float v1x = (s.kz0 ? B.y : (s.kz1 ? B.z : B.x)) - s.sox;
					const float v1y = (s.kz0 ? B.z : (s.kz1 ? B.x : B.y)) - s.soy;
					const float v1z = (s.kz0 ? B.x : (s.kz1 ? B.y : B.z)) - s.soz;
					const float v2x = (s.kz0 ? C.y : (s.kz1 ? C.z : C.x)) - s.sox;
					const float v2y = (s.kz0 ? C.z : (s.kz1 ? C.x : C.y)) - s.soy;
					const float v2z = (s.kz0 ? C.x : (s.kz1 ? C.y : C.z)) - s.soz;
					// shear (rtk.c:284-292)
					const float x0 = v0x + s.shx * v0z, y0 = v0y + s.shy * v0z, z0 = s.shz * v0z;
					const float x1 = v1x + s.shx * v1z, y1 = v1y + s.shy * v1z, z1 = s.shz * v1z;
					const float x2 = v2x + s.shx * v2z, y2 = v2y + s.shy * v2z, z2 = s.shz * v2z;
					// edge functions (rtk.c:298-300)
					float u, v, ww;
					if (scan) {
						u = x1 * y2 - y1 * x2;
						v = x2 * y0 - y2 * x0;
						ww = x0 * y1 - y0 * x1;
						zero_in_group = zero_in_group || u == 0.0f || v == 0.0f || ww == 0.0f;
						if ((i & 3u) == 3u) { scan = false; scanned = true; force = zero_in_group; i &= ~3u; }   // rtk.c:306
						else i++;
						continue;
					}
					if (COUNT) c_tris++;
					if (!force) {
						u = x1 * y2 - y1 * x2;
						v = x2 * y0 - y2 * x0;
						ww = x0 * y1 - y0 * x1;
					} else {
						const double xd0 = x0, yd0 = y0, xd1 = x1, yd1 = y1, xd2 = x2, yd2 = y2;
						u = (float)(xd1 * yd2 - yd1 * xd2);
						v = (float)(xd2 * yd0 - yd2 * xd0);
						ww = (float)(xd0 * yd1 - yd0 * xd1);
					}
					// rtk.c:340-342
					const bool neg = sse_min(sse_min(u, v), ww) < 0.0f;
					const bool pos = sse_max(sse_max(u, v), ww) > 0.0f;
					// rtk.c:346-353
					const float det = (u + v) + ww;
					const float rcp = 1.0f / det;
					float zz = u * z0;
					zz = zz + v * z1;
					zz = zz + ww * z2;
					const float tt = zz * rcp;
					const uint32_t prim = __float_as_uint(A.w);
					const bool in_range = !(neg && pos) && tt > tmin_ray && tt < tmax_ray;   // rtk.c:354
					if (ANY) {
						if (in_range) { best_prim = prim; best_inst = cur_inst; break; }
					} else if (in_range && (tt < best_t || (tt == best_t && best_inst == cur_inst && prim < best_prim))) {
						// rtk.c:371; inside one instance the lowest primitive id among bit-equal t, across instances strictly closer
						best_t = tt; best_u = u * rcp; best_v = v * rcp; best_prim = prim; best_inst = cur_inst;
					}
					i++;
				}
				top = RTK_REF_NONE;
				if (ANY && best_prim != RTK_PRIM_NONE) break;
			}
			// ---------------------------------------------------------------- pop: the entry distance again, best_t has shrunk since the push
			while (top == RTK_REF_NONE && sp != 0u) {
				--sp;
				const uint2 en = sp < WD_LDS_STACK ? stk[sp][lane] : p.spill[(size_t)(sp - WD_LDS_STACK) * p.spill_stride + glane];
				if (en.x == WD_REF_TOP) {
					// back in the top tree: the world ray's constants, and the rest of the leaf the instance was entered from
					wd_setup(wox, woy, woz, wdx, wdy, wdz, s);
					in_inst = false; cur_inst = RTK_PRIM_NONE;
					nodes = reinterpret_cast<const char *>(p.top_nodes); tris = reinterpret_cast<const char *>(p.top_tris);
					num_nodes = p.top_num_nodes; num_tris = p.top_num_tris;
					if (en.y != RTK_REF_NONE) top = RTK_REF_LEAF | en.y;
				} else if (ANY || !(__uint_as_float(en.y) > best_t)) top = en.x;
			}
		}

		const bool hit = best_prim != RTK_PRIM_NONE;
		if (COUNT && hit) c_hits++;
		if (ANY) { p.blocked[r] = hit ? 1 : 0; continue; }
		// a miss: max_t as given, u = v = 0, RTK_PRIM_NONE
		wd_u32x4 out;
		out.x = __float_as_uint(best_t); out.y = __float_as_uint(best_u); out.z = __float_as_uint(best_v); out.w = best_prim;
		__builtin_nontemporal_store(out, reinterpret_cast<wd_u32x4 *>(p.records + r));
		if (p.instances) p.instances[r] = best_inst;
	}
	if (COUNT) {
		// (the words rtk_trace_kernel's counting build uses)
		atomicAdd(p.counter + 1, (unsigned long long)c_rays);
		atomicAdd(p.counter + 2, (unsigned long long)c_nodes);
		atomicAdd(p.counter + 3, (unsigned long long)c_leaves);
		atomicAdd(p.counter + 4, (unsigned long long)c_tris);
		atomicAdd(p.counter + 5, (unsigned long long)c_hits);
		atomicAdd(p.counter + 6, (unsigned long long)c_spills);
	}
}

typedef void (*world_kernel_fn)(WorldParams);

// form: any | filtered << 1; 4: the counting closest form (filters included)
world_kernel_fn world_form(int form)
{
	switch (form) {
	case 0: return k_world<false, false, false>;
	case 1: return k_world<true, false, false>;
	case 2: return k_world<false, false, true>;
	case 3: return k_world<true, false, true>;
	default: return k_world<false, true, true>;
	}
}

// workgroups of k_world a CU holds, asked once per device
int world_blocks_per_cu(int device)
{
	static std::atomic<int> known[RTK_MAX_DEVICES];
	if (device < 0 || device >= RTK_MAX_DEVICES) return 2;
	int b = known[device].load(std::memory_order_relaxed);
	if (b == 0) {
		if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, k_world<false, false, true>, (int)WD_THREADS, 0) != hipSuccess || b < 1) b = 2;
		known[device].store(b, std::memory_order_relaxed);
	}
	return b;
}

// the scenes' tables and depths as they are now, each read under its scene's scratch_mutex (what a rebuild replaces them under)
void read_scenes(rtk_dev_world *w)
{
	w->deepest = 0;
	for (size_t k = 0; k < w->scenes.size(); k++) {
		rtk_dev_scene *ds = w->scenes[k];
		std::lock_guard<std::mutex> lock(ds->scratch_mutex);
		w->scene_table[k] = DevWorldScene{ ds->view.nodes, ds->view.tris, ds->view.num_nodes, ds->view.num_tris };
		const uint32_t entries = ds->tree.stack_entries();
		if (entries > w->deepest) w->deepest = entries;
	}
}

// the description of the top tree's one mesh: the proxy buffer (or a host copy of it) with implicit indices
void proxy_desc(const rtk_dev_world *w, const float *positions, rtk_mesh *mesh, rtk_scene_desc *desc)
{
	*mesh = rtk_mesh();
	mesh->num_triangles = w->num_instances;
	mesh->position.data = positions;
	mesh->position.stride = 0;
	mesh->position.type = RTK_TYPE_F32;
	*desc = rtk_scene_desc();
	desc->meshes = mesh;
	desc->num_meshes = 1;
}

// tables -> records and proxies -> the dead count, on `stream`; synchronises it
int make_instances(rtk_dev_world *w, hipStream_t stream, const char *who)
{
	RTK_HIP_CHECK(hipMemcpyAsync(w->d_scenes, w->scene_table.data(), w->scene_table.size() * sizeof(DevWorldScene), hipMemcpyHostToDevice, stream), RTK_AMD_ERR_HIP);
	RTK_HIP_CHECK(hipMemsetAsync(w->d_dead, 0, sizeof(unsigned long long), stream), RTK_AMD_ERR_HIP);
	InstParams p = { w->d_inst, w->d_place, w->d_proxy, w->d_scenes, w->d_dead, w->num_instances, (uint32_t)w->scenes.size() };
	hipLaunchKernelGGL(k_world_instances, dim3((w->num_instances + 255u) / 256u), dim3(256), 0, stream, p);
	RTK_HIP_CHECK(hipGetLastError(), RTK_AMD_ERR_HIP);
	unsigned long long dead = 0;
	RTK_HIP_CHECK(hipMemcpyAsync(&dead, w->d_dead, sizeof(dead), hipMemcpyDeviceToHost, stream), RTK_AMD_ERR_HIP);
	RTK_HIP_CHECK(hipStreamSynchronize(stream), RTK_AMD_ERR_HIP);
	w->dead = dead;
	(void)who;
	return RTK_AMD_OK;
}

// the top tree of a world of one instance: one triangle, which a build decodes on the host, so from a host copy of the proxy
rtk_dev_scene *build_top_of_one(rtk_dev_world *w)
{
	float proxy[9];
	if (hipMemcpy(proxy, w->d_proxy, sizeof(proxy), hipMemcpyDeviceToHost) != hipSuccess) { rtk_set_error("rtk_dev_world: copy of the proxy failed"); return nullptr; }
	rtk_mesh mesh;
	rtk_scene_desc desc;
	proxy_desc(w, proxy, &mesh, &desc);
	return rtk_dev_scene_build(&desc);
}

double ms_since(std::chrono::steady_clock::time_point t0)
{
	return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

} // namespace

extern "C" uint32_t rtk_amd_world_stack_entries(void) { return WD_LDS_STACK; }

extern "C" rtk_dev_world *rtk_dev_world_create(rtk_dev_scene *const *scenes, size_t num_scenes, const uint32_t *instance_scene,
	const rtk_placement *placements, size_t num_instances)
{
	const auto t0 = std::chrono::steady_clock::now();
	// everything the host can see is refused here, before any HIP call
	if (!scenes || !instance_scene || !placements || num_scenes == 0) { rtk_set_error("rtk_dev_world_create: NULL scenes, instance_scene or placements, or no scene"); return nullptr; }
	if (num_instances == 0 || num_instances >= ((size_t)1 << 31)) { rtk_set_error("rtk_dev_world_create: %zu instances: a world holds 1 .. 2^31 - 1", num_instances); return nullptr; }
	if (num_scenes >= ((size_t)1 << 31)) { rtk_set_error("rtk_dev_world_create: %zu scenes: a world names fewer than 2^31", num_scenes); return nullptr; }
	for (size_t k = 0; k < num_scenes; k++) {
		if (!scenes[k]) { rtk_set_error("rtk_dev_world_create: scene %zu is NULL", k); return nullptr; }
		if (scenes[k]->device != scenes[0]->device) {
			rtk_set_error("rtk_dev_world_create: scene %zu lives on device %d, scene 0 on device %d: a world is on one device", k, scenes[k]->device, scenes[0]->device);
			return nullptr;
		}
	}
	for (size_t i = 0; i < num_instances; i++) {
		if (instance_scene[i] >= num_scenes) { rtk_set_error("rtk_dev_world_create: instance %zu names scene %u of %zu", i, instance_scene[i], num_scenes); return nullptr; }
	}
	if (!rtk_on_scene_device(scenes[0], "rtk_dev_world_create")) return nullptr;

	rtk_dev_world *w = new rtk_dev_world();
	w->device = scenes[0]->device;
	w->scenes.assign(scenes, scenes + num_scenes);
	w->scene_table.resize(num_scenes);
	w->num_instances = (uint32_t)num_instances;
	w->d_inst = static_cast<DevWorldInstance *>(w->mem.own(num_instances * sizeof(DevWorldInstance), num_instances * sizeof(DevWorldInstance)));
	w->d_place = static_cast<rtk_placement *>(w->mem.own(num_instances * sizeof(rtk_placement), num_instances * sizeof(rtk_placement)));
	w->d_proxy = static_cast<float *>(w->mem.own(num_instances * 36u, num_instances * 36u));
	w->d_scenes = static_cast<DevWorldScene *>(w->mem.own(num_scenes * sizeof(DevWorldScene), num_scenes * sizeof(DevWorldScene)));
	w->d_dead = static_cast<unsigned long long *>(w->mem.own(sizeof(unsigned long long), sizeof(unsigned long long)));
	if (!w->d_inst || !w->d_place || !w->d_proxy || !w->d_scenes || !w->d_dead) {
		rtk_set_error("rtk_dev_world_create: out of device memory (%zu instances, %zu scenes)", num_instances, num_scenes);
		rtk_dev_world_free(w);
		return nullptr;
	}
	// the records start as their scene numbers; k_world_instances fills the rest
	std::vector<DevWorldInstance> recs(num_instances);
	for (size_t i = 0; i < num_instances; i++) { recs[i] = DevWorldInstance(); recs[i].scene = instance_scene[i]; }
	bool ok = hipMemcpy(w->d_inst, recs.data(), num_instances * sizeof(DevWorldInstance), hipMemcpyHostToDevice) == hipSuccess &&
		hipMemcpy(w->d_place, placements, num_instances * sizeof(rtk_placement), hipMemcpyDefault) == hipSuccess;
	if (!ok) rtk_set_error("rtk_dev_world_create: copy of the instances failed: %s", hipGetErrorString(hipGetLastError()));
	read_scenes(w);
	ok = ok && make_instances(w, nullptr, "rtk_dev_world_create") == RTK_AMD_OK;
	if (ok) {
		if (num_instances < 2) w->top = build_top_of_one(w);
		else {
			rtk_mesh mesh;
			rtk_scene_desc desc;
			proxy_desc(w, w->d_proxy, &mesh, &desc);
			w->top = rtk_dev_scene_build(&desc);
		}
		ok = w->top != nullptr;
	}
	if (!ok) { rtk_dev_world_free(w); return nullptr; }
	w->build_ms = ms_since(t0);
	return w;
}

extern "C" void rtk_dev_world_free(rtk_dev_world *w)
{
	if (!w) return;
	if (w->top) rtk_dev_scene_free(w->top);
	w->mem.release_all();
	delete w;
}

extern "C" int rtk_dev_world_update(rtk_dev_world *w, const rtk_placement *placements, void *stream_)
{
	const auto t0 = std::chrono::steady_clock::now();
	if (!w) { rtk_set_error("rtk_dev_world_update: NULL world"); return RTK_AMD_ERR_BAD_ARG; }
	if (!rtk_on_scene_device(w->top, "rtk_dev_world_update")) return RTK_AMD_ERR_BAD_ARG;
	const hipStream_t stream = (hipStream_t)stream_;
	std::lock_guard<std::mutex> lock(w->mutex);
	if (placements) RTK_HIP_CHECK(hipMemcpyAsync(w->d_place, placements, (size_t)w->num_instances * sizeof(rtk_placement), hipMemcpyDefault, stream), RTK_AMD_ERR_HIP);
	read_scenes(w);
	int rc = make_instances(w, stream, "rtk_dev_world_update");
	if (rc != RTK_AMD_OK) return rc;
	if (w->num_instances < 2) {
		rtk_dev_scene *top = build_top_of_one(w);
		if (!top) return RTK_AMD_ERR_HIP;
		rtk_dev_scene_free(w->top);
		w->top = top;
	} else {
		rtk_mesh mesh;
		rtk_scene_desc desc;
		proxy_desc(w, w->d_proxy, &mesh, &desc);
		rc = rtk_dev_scene_refit(w->top, &desc, stream);
		if (rc != RTK_AMD_OK) return rc;
	}
	w->update_ms = ms_since(t0);
	return RTK_AMD_OK;
}

extern "C" int rtk_dev_world_rebuild(rtk_dev_world *w, void *stream)
{
	if (!w) { rtk_set_error("rtk_dev_world_rebuild: NULL world"); return RTK_AMD_ERR_BAD_ARG; }
	if (!rtk_on_scene_device(w->top, "rtk_dev_world_rebuild")) return RTK_AMD_ERR_BAD_ARG;
	std::lock_guard<std::mutex> lock(w->mutex);
	if (w->num_instances < 2) return RTK_AMD_OK;           // (one proxy under one root: there is nothing to build again)
	return rtk_dev_scene_rebuild(w->top, nullptr, stream);
}

extern "C" int rtk_dev_world_get_info(const rtk_dev_world *w_c, rtk_dev_world_info *out)
{
	if (!w_c || !out) { rtk_set_error("rtk_dev_world_get_info: NULL argument"); return RTK_AMD_ERR_BAD_ARG; }
	rtk_dev_world *w = const_cast<rtk_dev_world *>(w_c);
	std::lock_guard<std::mutex> lock(w->mutex);
	*out = rtk_dev_world_info();
	out->num_scenes = w->scenes.size();
	out->num_instances = w->num_instances;
	out->dead_instances = w->dead;
	out->top_nodes = w->top->view.num_nodes;
	out->total_device_bytes = w->top->mem.counted() + w->mem.counted();
	out->top_max_depth = w->top->tree.max_depth;
	out->stack_entries = w->top->tree.stack_entries() + 1u + w->deepest;
	out->build_ms = w->build_ms;
	out->update_ms = w->update_ms;
	return RTK_AMD_OK;
}

extern "C" const rtk_dev_scene *rtk_dev_world_top_scene(const rtk_dev_world *w)
{
	if (!w) { rtk_set_error("rtk_dev_world_top_scene: NULL world"); return nullptr; }
	return w->top;
}

extern "C" int rtk_dev_world_trace_status(const rtk_dev_world *w, void *stream)
{
	if (!w) { rtk_set_error("rtk_dev_world_trace_status: NULL world"); return RTK_AMD_ERR_BAD_ARG; }
	return rtk_dev_trace_status(w->top, stream);
}

int rtk_launch_world(const rtk_dev_world *w_c, const rtk_ray *d_rays, size_t n, const rtk_ray_list *list, const rtk_world_filter *filter,
	rtk_hit_record *d_records, uint32_t *d_instances, uint8_t *d_blocked, bool any_hit, hipStream_t stream, rtk_trace_counters *counted)
{
	rtk_dev_world *w = const_cast<rtk_dev_world *>(w_c);
	const char *who = any_hit ? "rtk_dev_world_trace_rays_any" : counted ? "rtk_dev_world_trace_rays_counted" : "rtk_dev_world_trace_rays";
	// everything the host can see is refused here, before any HIP call
	const int refused = rtk_world_refuse(who, "rays", w, n, d_rays && (any_hit ? d_blocked != nullptr : d_records != nullptr), list, filter);
	if (refused != RTK_AMD_OK) return refused;
	if (counted) *counted = rtk_trace_counters();
	if (n == 0) return RTK_AMD_OK;
	if (!rtk_on_scene_device(w->top, who)) return RTK_AMD_ERR_BAD_ARG;

	WorldParams p = {};
	p.rays = d_rays;
	p.n = (uint32_t)n;
	p.ids = list ? reinterpret_cast<const unsigned long long *>(list->d_ids) : nullptr;
	p.count = list ? reinterpret_cast<const unsigned long long *>(list->d_count) : nullptr;
	p.records = d_records;
	p.instances = d_instances;
	p.blocked = d_blocked;
	const bool filtered = filter && (filter->d_instance_mask || filter->d_ignore_instance);
	if (filtered) { p.mask = filter->d_instance_mask; p.mask_bits = filter->instance_mask_bits; p.ignore_instance = filter->d_ignore_instance; }
	// (the largest |plane| of the top tree: read under the lock a rebuild replaces it under)
	return rtk_world_launch(w, n, stream, world_blocks_per_cu(w->device), world_form((any_hit ? 1 : 0) | (filtered ? 2 : 0)), world_form(4), p,
		[](const rtk_dev_scene *top, WorldParams &q) { q.bound = top->tree.bound_raw; }, counted, "rtk_dev_world_trace_rays_counted");
}
