// rtk_sign.hip -- rtk_dev_signed_distances: the closest-point walk as it is (rtk_launch_closest) and an epilogue that gives each
// answer its sign by the rule of rtk_sign_rule.h, from a per-primitive table of edge and vertex pseudonormals that is made on the
// device on first use. Table and sign are functions of the scene's triangle records alone (DESIGN.md "Signed distance").
//
// MAKING THE TABLE (rtk_scene_pseudonormals). Corners are welded by place, so equal places have to be found: a sort.
//   terms    one lane per triangle record: the three corner positions, the unit normal and the three terms angle * unit, written
//            at 3 * prim + k -- scattered by the record's PRIMITIVE ID, not by its slot, so that the input order of the sort, and
//            with it the order of every sum, is by (prim, corner) whatever the tree. The sort key of z with them.
//   sort     the 96-bit place does not fit the sort's 64-bit key: two stable passes of rtk_sort_pairs_async, by z (32 bits), then
//            by (x, y) (64 bits) with the keys gathered again in between. -0 and +0 share a key (rtk_sign_key). A corner with a
//            NaN coordinate needs no key of its own: it sorts wherever its bits put it, outside every run of equal numbers,
//            and the comparison that marks the heads below is never true for it.
//   heads    position j of the sorted corners begins a run iff j == 0 or its place differs from the one before (float ==).
//   vertex   one lane per sorted position; the HEAD of a run walks it once to add the terms in order and once more to write the
//            sum to every member's row and the run's bounds to every member. The other lanes idle: a wave of 64 positions holds
//            about ten heads on a closed mesh (valence six), each of which walks six entries. The alternative, every member
//            walking its run, keeps all lanes busy but reads valence times as much and needs the bounds first; neither shares
//            data between lanes, and a segmented wave scan would change the order of the additions, which the rule fixes.
//            (Read from the code, not measured against the alternative.)
//   edges    one lane per (prim, edge): the run of one end is walked and the records that also have a corner at the other end are
//            kept: the sum of their unit normals in ascending prim order, and the counts of rtk_dev_sign_info from the same walk.
//            A vertex that v triangles meet at costs v walks of v entries: valence squared (DESIGN.md says what that means
//            for a pole).
// Temporaries come from the device's workspace (WorkspaceLoan), the table is one entry of the scene's ledger.
#include "rtk_dev.h"
#include "rtk_sign_rule.h"

#include <chrono>
#include <mutex>

#define SG_THREADS 256u

namespace {

typedef float sg_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t sg_u32x4 __attribute__((ext_vector_type(4)));

enum { SG_BOUNDARY, SG_NONMANIFOLD, SG_INCONSISTENT, SG_DEGENERATE, SG_PLACES, SG_COUNTS };

// the temporaries of one making, all in the workspace; m = 3 * num_prims corners
struct SignWork {
	sg_f32x4 *pos;                     // [m] by corner id 3 * prim + k: the corner's position (w: 0)
	sg_f32x4 *term;                    // [m] by corner id: angle * unit normal; w != 0: the triangle has a normal
	sg_f32x4 *unit;                    // [n] by prim: the unit normal; w != 0: the triangle has one
	uint2 *run;                        // [m] by corner id: [begin, end) of its place's run of sorted positions
	uint32_t *head;                    // [m] by sorted position: 1 = first of its run
	unsigned long long *counts;        // SG_COUNTS words
	uint32_t num_prims, num_corners;
};

__global__ void __launch_bounds__(SG_THREADS) k_sign_terms(const DevTri *tris, uint32_t num_tris, SignWork w, unsigned long long *keys, uint32_t *vals)
{
	const uint32_t slot = blockIdx.x * SG_THREADS + threadIdx.x;
	if (slot >= num_tris) return;
	const sg_f32x4 *t = reinterpret_cast<const sg_f32x4 *>(reinterpret_cast<const char *>(tris) + (size_t)slot * RTK_TRI_STRIDE);
	const sg_f32x4 A = t[0], B = t[1], C = t[2];
	const uint32_t prim = __float_as_uint(A.w);
	if (prim >= w.num_prims) return;                                  // (not one record per primitive: refused on the host; nothing out of range)
	const float a[3] = { A.x, A.y, A.z }, b[3] = { B.x, B.y, B.z }, c[3] = { C.x, C.y, C.z };
	float n[3], unit[3], term[9];
	const bool has = rtk_sign_unit_normal(a, b, c, n, unit);
	if (has) rtk_sign_corner_terms(a, b, c, unit, term);
	else { for (int i = 0; i < 9; i++) term[i] = 0.0f; unit[0] = unit[1] = unit[2] = 0.0f; atomicAdd(w.counts + SG_DEGENERATE, 1ull); }
	const float flag = has ? 1.0f : 0.0f;
	sg_f32x4 u4; u4.x = unit[0]; u4.y = unit[1]; u4.z = unit[2]; u4.w = flag;
	w.unit[prim] = u4;
	const float *v[3] = { a, b, c };
	for (int k = 0; k < 3; k++) {
		const uint32_t corner = 3u * prim + (uint32_t)k;
		sg_f32x4 p4; p4.x = v[k][0]; p4.y = v[k][1]; p4.z = v[k][2]; p4.w = 0.0f;
		sg_f32x4 t4; t4.x = term[3 * k]; t4.y = term[3 * k + 1]; t4.z = term[3 * k + 2]; t4.w = flag;
		w.pos[corner] = p4;
		w.term[corner] = t4;
		keys[corner] = (unsigned long long)rtk_sign_key(__float_as_uint(v[k][2]));
		vals[corner] = corner;
	}
}

// the keys of the second pass, gathered through the order the first one left
__global__ void __launch_bounds__(SG_THREADS) k_sign_rekey(const uint32_t *vals, SignWork w, unsigned long long *keys)
{
	const uint32_t j = blockIdx.x * SG_THREADS + threadIdx.x;
	if (j >= w.num_corners) return;
	const uint32_t corner = vals[j];
	if (corner >= w.num_corners) { keys[j] = 0ull; return; }
	const sg_f32x4 p = w.pos[corner];
	keys[j] = (unsigned long long)rtk_sign_key(__float_as_uint(p.x)) << 32 | rtk_sign_key(__float_as_uint(p.y));
}

__global__ void __launch_bounds__(SG_THREADS) k_sign_heads(const uint32_t *order, SignWork w)
{
	const uint32_t j = blockIdx.x * SG_THREADS + threadIdx.x;
	bool head = false;
	if (j < w.num_corners) {
		head = true;
		if (j != 0u) {
			const sg_f32x4 p = w.pos[order[j]], q = w.pos[order[j - 1u]];
			const float x[3] = { p.x, p.y, p.z }, y[3] = { q.x, q.y, q.z };
			head = !rtk_sign_same_place(x, y);
		}
		w.head[j] = head ? 1u : 0u;
	}
	const unsigned long long heads = __ballot(head);
	if ((threadIdx.x & 63u) == 0u && heads) atomicAdd(w.counts + SG_PLACES, (unsigned long long)__popcll(heads));
}

__global__ void __launch_bounds__(SG_THREADS) k_sign_vertex(const uint32_t *order, SignWork w, float *table)
{
	const uint32_t j = blockIdx.x * SG_THREADS + threadIdx.x;
	if (j >= w.num_corners || w.head[j] == 0u) return;
	uint32_t end = j + 1u;
	float sum[3] = { 0.0f, 0.0f, 0.0f };
	bool first = true;
	for (uint32_t i = j; i < w.num_corners && (i == j || w.head[i] == 0u); i++) {
		end = i + 1u;
		const sg_f32x4 t = w.term[order[i]];
		if (t.w == 0.0f) continue;
		if (first) { sum[0] = t.x; sum[1] = t.y; sum[2] = t.z; first = false; }
		else { sum[0] = RTK_CL_ADD(sum[0], t.x); sum[1] = RTK_CL_ADD(sum[1], t.y); sum[2] = RTK_CL_ADD(sum[2], t.z); }
	}
	for (uint32_t i = j; i < end; i++) {
		const uint32_t corner = order[i], prim = corner / 3u, k = corner - 3u * prim;
		float *dst = table + (size_t)prim * 18u + 9u + 3u * k;
		dst[0] = sum[0]; dst[1] = sum[1]; dst[2] = sum[2];
		w.run[corner] = make_uint2(j, end);
	}
}

__global__ void __launch_bounds__(SG_THREADS) k_sign_edges(const uint32_t *order, SignWork w, float *table)
{
	const uint32_t idx = blockIdx.x * SG_THREADS + threadIdx.x;
	if (idx >= w.num_corners) return;
	const uint32_t prim = idx / 3u, e = idx - 3u * prim;
	const int ki = e == 2u ? 1 : 0, kj = e == 0u ? 1 : 2;            // ab: (0, 1)  ac: (0, 2)  bc: (1, 2)
	const uint2 rp = w.run[3u * prim + (uint32_t)ki], rq = w.run[3u * prim + (uint32_t)kj];
	float *dst = table + (size_t)prim * 18u + 3u * e;
	if (rp.x == rq.x) {
		// both ends at one place: the vertex pseudonormal of that place (k_sign_vertex has written it)
		const float *src = table + (size_t)prim * 18u + 9u + 3u * (uint32_t)ki;
		dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
		return;
	}
	float sum[3] = { 0.0f, 0.0f, 0.0f };
	bool first = true, other_forward = false;
	uint32_t others = 0, last = 0xffffffffu;
	for (uint32_t i = rp.x; i < rp.y; i++) {
		const uint32_t corner = order[i], t = corner / 3u;
		if (t == last) continue;                                      // (a record's corners are neighbours in a run: it counts once)
		last = t;
		const int kp = (int)(corner - 3u * t);                        // its lowest corner at P
		int kq = -1;
		for (int k = 2; k >= 0; k--) if (w.run[3u * t + (uint32_t)k].x == rq.x) kq = k;
		if (kq < 0) continue;
		const sg_f32x4 u = w.unit[t];
		if (u.w != 0.0f) {
			if (first) { sum[0] = u.x; sum[1] = u.y; sum[2] = u.z; first = false; }
			else { sum[0] = RTK_CL_ADD(sum[0], u.x); sum[1] = RTK_CL_ADD(sum[1], u.y); sum[2] = RTK_CL_ADD(sum[2], u.z); }
		}
		if (t != prim) { others++; other_forward = rtk_sign_runs_forward(kp, kq); }
	}
	dst[0] = sum[0]; dst[1] = sum[1]; dst[2] = sum[2];
	if (others == 0u) atomicAdd(w.counts + SG_BOUNDARY, 1ull);
	else if (others >= 2u) atomicAdd(w.counts + SG_NONMANIFOLD, 1ull);
	else if (other_forward == rtk_sign_runs_forward(ki, kj)) atomicAdd(w.counts + SG_INCONSISTENT, 1ull);
}

struct SignedParams {
	const DevTri *tris;
	const uint32_t *prim_slot;
	const float *table;
	uint32_t num_tris, num_prims;
	const rtk_point_query *queries;
	const unsigned long long *ids;     // or NULL: 0, 1, 2, ...
	const unsigned long long *count;   // or NULL: n
	const rtk_closest_record *records;
	float *out;
	uint32_t n;
};

// the epilogue: one lane per answered query. The record of the answer's primitive goes through the rule once more
__global__ void __launch_bounds__(SG_THREADS) k_signed(SignedParams p)
{
	uint32_t m = p.n;
	if (p.count) { const unsigned long long listed = *p.count; m = listed < p.n ? (uint32_t)listed : p.n; }
	const unsigned long long step = (unsigned long long)gridDim.x * SG_THREADS;
	for (unsigned long long i = (unsigned long long)blockIdx.x * SG_THREADS + threadIdx.x; i < m; i += step) {
		const unsigned long long id = p.ids ? p.ids[i] : i;
		if (id >= p.n) continue;                                      // (the caller's error; nothing is read or written out of range)
		const uint32_t r = (uint32_t)id;
		const uint32_t prim = p.records[r].prim;
		float out = RTK_SIGN_INF;
		const uint32_t slot = prim < p.num_prims ? p.prim_slot[prim] : 0xffffffffu;
		if (slot < p.num_tris) {
			const sg_f32x4 *t = reinterpret_cast<const sg_f32x4 *>(reinterpret_cast<const char *>(p.tris) + (size_t)slot * RTK_TRI_STRIDE);
			const sg_f32x4 A = t[0], B = t[1], C = t[2];
			const sg_u32x4 qw = *reinterpret_cast<const sg_u32x4 *>(p.queries + r);
			const float P[3] = { __uint_as_float(qw.x), __uint_as_float(qw.y), __uint_as_float(qw.z) };
			const float a[3] = { A.x, A.y, A.z }, b[3] = { B.x, B.y, B.z }, c[3] = { C.x, C.y, C.z };
			float q[3];
			int region;
			out = rtk_sign_signed(P, a, b, c, p.table + (size_t)prim * 18u, q, region);
		}
		p.out[r] = out;
	}
}

int sign_refusals(const char *who, const rtk_dev_scene *ds)
{
	if (!ds->records_once || ds->view.num_tris != ds->view.num_prims) {
		rtk_set_error("%s: the scene does not hold exactly one triangle record per primitive (%u records, %u primitives)", who, ds->view.num_tris, ds->view.num_prims);
		return RTK_AMD_ERR_UNSUPPORTED;
	}
	if ((uint64_t)ds->view.num_prims * 3u >= ((uint64_t)1 << 32)) { rtk_set_error("%s: more than 2^32 triangle corners", who); return RTK_AMD_ERR_UNSUPPORTED; }
	return RTK_AMD_OK;
}

} // namespace

// Makes the table if it is not there. The calling thread waits for `stream` that one time: the workspace goes back when this
// returns, and launches on any other stream may use the table as soon as it does.
int rtk_scene_pseudonormals(const rtk_dev_scene *ds_c, hipStream_t stream)
{
	rtk_dev_scene *ds = const_cast<rtk_dev_scene *>(ds_c);
	if (!ds) return RTK_AMD_ERR_BAD_ARG;
	std::lock_guard<std::mutex> lock(ds->sign_mutex);
	if (ds->sign.d_table) return RTK_AMD_OK;
	int rc = sign_refusals("rtk_scene_pseudonormals", ds);
	if (rc != RTK_AMD_OK) return rc;
	const auto t_begin = std::chrono::steady_clock::now();
	const DevTri *tris;
	uint32_t num_tris, n;
	{
		std::lock_guard<std::mutex> view_lock(ds->scratch_mutex);     // (the view is read under the lock a rebuild replaces it under)
		tris = ds->view.tris; num_tris = ds->view.num_tris; n = ds->view.num_prims;
	}
	const uint32_t m = 3u * n;
	const size_t table_bytes = (size_t)n * 18u * sizeof(float);
	float *table = (float *)ds->mem.own(table_bytes ? table_bytes : 72u, table_bytes);
	if (!table) { rtk_set_error("rtk_scene_pseudonormals: out of device memory (%zu bytes)", table_bytes); return RTK_AMD_ERR_OOM; }
	rtk_dev_sign_info info = {};
	info.table_bytes = table_bytes;
	if (n != 0u) {
		Carve c;
		const size_t o_pos = c.take((size_t)m * 16u), o_term = c.take((size_t)m * 16u), o_unit = c.take((size_t)n * 16u), o_run = c.take((size_t)m * 8u),
			o_head = c.take((size_t)m * 4u), o_counts = c.take(SG_COUNTS * 8u), o_ka = c.take((size_t)m * 8u), o_kb = c.take((size_t)m * 8u),
			o_va = c.take((size_t)m * 4u), o_vb = c.take((size_t)m * 4u), o_sort = c.take(rtk_sort_scratch_words(m) * 4u);
		WorkspaceLoan loan;
		if (!loan.take(ds->device, c.bytes)) { ds->mem.release(table); return RTK_AMD_ERR_OOM; }
		SignWork w;
		w.pos = (sg_f32x4 *)(loan.base + o_pos); w.term = (sg_f32x4 *)(loan.base + o_term); w.unit = (sg_f32x4 *)(loan.base + o_unit);
		w.run = (uint2 *)(loan.base + o_run); w.head = (uint32_t *)(loan.base + o_head); w.counts = (unsigned long long *)(loan.base + o_counts);
		w.num_prims = n; w.num_corners = m;
		unsigned long long *keys_a = (unsigned long long *)(loan.base + o_ka), *keys_b = (unsigned long long *)(loan.base + o_kb);
		uint32_t *vals_a = (uint32_t *)(loan.base + o_va), *vals_b = (uint32_t *)(loan.base + o_vb), *sort_scratch = (uint32_t *)(loan.base + o_sort);
		const dim3 block(SG_THREADS), grid_tris((num_tris + SG_THREADS - 1u) / SG_THREADS), grid_corners((m + SG_THREADS - 1u) / SG_THREADS);
		unsigned long long counts[SG_COUNTS] = {};
		hipError_t e = hipMemsetAsync(w.counts, 0, SG_COUNTS * 8u, stream);
		// (every corner is written by exactly one record; cleared all the same, so that no word of the sort's input is ever undefined)
		if (e == hipSuccess) e = hipMemsetAsync(keys_a, 0, (size_t)m * 8u, stream);
		if (e == hipSuccess) e = hipMemsetAsync(vals_a, 0, (size_t)m * 4u, stream);
		if (e == hipSuccess) e = hipMemsetAsync(w.pos, 0, (size_t)m * 16u, stream);
		if (e == hipSuccess) e = hipMemsetAsync(w.term, 0, (size_t)m * 16u, stream);
		if (e == hipSuccess) e = hipMemsetAsync(w.unit, 0, (size_t)n * 16u, stream);
		if (e == hipSuccess) e = hipMemsetAsync(w.run, 0, (size_t)m * 8u, stream);
		if (e == hipSuccess) {
			hipLaunchKernelGGL(k_sign_terms, grid_tris, block, 0, stream, tris, num_tris, w, keys_a, vals_a);
			// by z, then by (x, y): stable, so that corners at one place stay in (prim, corner) order
			const bool in_b = rtk_sort_pairs_async(keys_a, keys_b, vals_a, vals_b, m, 32u, sort_scratch, stream);
			unsigned long long *k1 = in_b ? keys_a : keys_b, *k2 = in_b ? keys_b : keys_a;      // (k1: free now, takes the new keys)
			uint32_t *v1 = in_b ? vals_b : vals_a, *v2 = in_b ? vals_a : vals_b;                // (v1: the order by z)
			hipLaunchKernelGGL(k_sign_rekey, grid_corners, block, 0, stream, v1, w, k1);
			const bool in_2 = rtk_sort_pairs_async(k1, k2, v1, v2, m, 64u, sort_scratch, stream);
			const uint32_t *order = in_2 ? v2 : v1;
			hipLaunchKernelGGL(k_sign_heads, grid_corners, block, 0, stream, order, w);
			hipLaunchKernelGGL(k_sign_vertex, grid_corners, block, 0, stream, order, w, table);
			hipLaunchKernelGGL(k_sign_edges, grid_corners, block, 0, stream, order, w, table);
			e = hipGetLastError();
		}
		if (e == hipSuccess) e = hipMemcpyAsync(counts, w.counts, sizeof(counts), hipMemcpyDeviceToHost, stream);
		// (also on a failure: whatever was enqueued on the workspace is over before the loan ends)
		const hipError_t e_sync = hipStreamSynchronize(stream);
		if (e == hipSuccess) e = e_sync;
		if (e != hipSuccess) {
			rtk_set_error("rtk_scene_pseudonormals: %s", hipGetErrorString(e));
			ds->mem.release(table);
			return e == hipErrorOutOfMemory ? RTK_AMD_ERR_OOM : RTK_AMD_ERR_HIP;
		}
		info.boundary_sides = counts[SG_BOUNDARY]; info.nonmanifold_sides = counts[SG_NONMANIFOLD]; info.inconsistent_sides = counts[SG_INCONSISTENT];
		info.degenerate_triangles = counts[SG_DEGENERATE]; info.places = counts[SG_PLACES];
	}
	info.table_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
	ds->sign.info = info;
	ds->sign.d_table = table;
	return RTK_AMD_OK;
}

int rtk_launch_signed(const rtk_dev_scene *ds_c, const rtk_point_query *d_queries, size_t num_queries, const rtk_ray_list *list,
	rtk_closest_record *d_records, float *d_points, float *d_signed, hipStream_t stream)
{
	rtk_dev_scene *ds = const_cast<rtk_dev_scene *>(ds_c);
	// everything the host can see is refused here, before any HIP call (rtk_launch_closest's own list, and d_signed)
	if (!ds || (num_queries && (!d_queries || !d_signed))) { rtk_set_error("rtk_dev_signed_distances: NULL scene, queries or d_signed"); return RTK_AMD_ERR_BAD_ARG; }
	if (list && (list->struct_size < sizeof(rtk_ray_list) || list->flags != 0u || !list->d_count)) {
		rtk_set_error("rtk_dev_signed_distances: bad list (struct_size %u, flags %#x, d_count %p)", list->struct_size, list->flags, (const void *)list->d_count);
		return RTK_AMD_ERR_BAD_ARG;
	}
	if (num_queries >= ((size_t)1 << 32)) { rtk_set_error("rtk_dev_signed_distances: %zu queries: a batch holds fewer than 2^32", num_queries); return RTK_AMD_ERR_BAD_ARG; }
	if (num_queries == 0) return RTK_AMD_OK;
	int rc = sign_refusals("rtk_dev_signed_distances", ds);
	if (rc != RTK_AMD_OK) return rc;
	if (!rtk_on_scene_device(ds, "rtk_dev_signed_distances")) return RTK_AMD_ERR_BAD_ARG;
	if ((rc = rtk_scene_pseudonormals(ds, stream)) != RTK_AMD_OK) return rc;
	if ((rc = rtk_scene_side_arrays(ds, stream)) != RTK_AMD_OK) return rc;          // (prim_slot: a device build makes it on first use)
	if (!d_records) {
		// the walk's records in the scratch set of (scene, stream): grown on demand, never a fresh allocation per call
		std::lock_guard<std::mutex> lock(ds->scratch_mutex);
		LaunchScratch *sc = ds->scratch.get(stream);
		if (!sc) return RTK_AMD_ERR_OOM;
		if ((rc = sc->grow(sc->signed_records, num_queries, num_queries * sizeof(rtk_closest_record))) != RTK_AMD_OK) return rc;
		d_records = sc->signed_records.as<rtk_closest_record>();
	}
	if ((rc = rtk_launch_closest(ds, d_queries, num_queries, list, d_records, d_points, stream)) != RTK_AMD_OK) return rc;

	SignedParams p = {};
	p.queries = d_queries;
	p.ids = list ? reinterpret_cast<const unsigned long long *>(list->d_ids) : nullptr;
	p.count = list ? reinterpret_cast<const unsigned long long *>(list->d_count) : nullptr;
	p.records = d_records;
	p.out = d_signed;
	p.n = (uint32_t)num_queries;
	size_t grid = (num_queries + SG_THREADS - 1u) / SG_THREADS;
	const size_t grid_max = (size_t)(ds->num_cus > 0 ? ds->num_cus : 1) * 8u;
	if (grid > grid_max) grid = grid_max;
	std::lock_guard<std::mutex> sign_lock(ds->sign_mutex);
	std::lock_guard<std::mutex> lock(ds->scratch_mutex);
	p.tris = ds->view.tris; p.prim_slot = ds->view.prim_slot; p.num_tris = ds->view.num_tris; p.num_prims = ds->view.num_prims;
	p.table = ds->sign.d_table;
	if (!p.table || !p.prim_slot) { rtk_set_error("rtk_dev_signed_distances: the scene was refitted or rebuilt while the call ran"); return RTK_AMD_ERR_BAD_ARG; }
	hipLaunchKernelGGL(k_signed, dim3((unsigned)grid), dim3(SG_THREADS), 0, stream, p);
	RTK_HIP_CHECK(hipGetLastError(), RTK_AMD_ERR_HIP);
	return RTK_AMD_OK;
}

extern "C" int rtk_dev_scene_prepare_signs(const rtk_dev_scene *ds_c, rtk_dev_sign_info *out, void *stream)
{
	rtk_dev_scene *ds = const_cast<rtk_dev_scene *>(ds_c);
	if (!ds) { rtk_set_error("rtk_dev_scene_prepare_signs: NULL scene"); return RTK_AMD_ERR_BAD_ARG; }
	int rc = sign_refusals("rtk_dev_scene_prepare_signs", ds);
	if (rc != RTK_AMD_OK) return rc;
	bool made;
	{
		std::lock_guard<std::mutex> lock(ds->sign_mutex);
		made = ds->sign.d_table != nullptr;
	}
	if (!made) {
		if (!rtk_on_scene_device(ds, "rtk_dev_scene_prepare_signs")) return RTK_AMD_ERR_BAD_ARG;
		if ((rc = rtk_scene_pseudonormals(ds, (hipStream_t)stream)) != RTK_AMD_OK) return rc;
	}
	if (out) {
		std::lock_guard<std::mutex> lock(ds->sign_mutex);
		*out = ds->sign.info;
		if (made) out->table_ms = 0.0;
	}
	return RTK_AMD_OK;
}

extern "C" int rtk_dev_scene_pseudonormals(const rtk_dev_scene *ds_c, float *d_out, void *stream)
{
	rtk_dev_scene *ds = const_cast<rtk_dev_scene *>(ds_c);
	if (!ds || !d_out) { rtk_set_error("rtk_dev_scene_pseudonormals: NULL scene or d_out"); return RTK_AMD_ERR_BAD_ARG; }
	int rc = sign_refusals("rtk_dev_scene_pseudonormals", ds);
	if (rc != RTK_AMD_OK) return rc;
	if (!rtk_on_scene_device(ds, "rtk_dev_scene_pseudonormals")) return RTK_AMD_ERR_BAD_ARG;
	if ((rc = rtk_scene_pseudonormals(ds, (hipStream_t)stream)) != RTK_AMD_OK) return rc;
	std::lock_guard<std::mutex> lock(ds->sign_mutex);
	if (!ds->sign.d_table) { rtk_set_error("rtk_dev_scene_pseudonormals: the scene was refitted while the call ran"); return RTK_AMD_ERR_BAD_ARG; }
	if (ds->sign.info.table_bytes)
		RTK_HIP_CHECK(hipMemcpyAsync(d_out, ds->sign.d_table, ds->sign.info.table_bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream), RTK_AMD_ERR_HIP);
	return RTK_AMD_OK;
}

extern "C" int rtk_dev_signed_distances(const rtk_dev_scene *ds, const rtk_point_query *d_queries, size_t num_queries, const rtk_ray_list *list,
	rtk_closest_record *d_records, float *d_points, float *d_signed, void *stream)
{
	return rtk_launch_signed(ds, d_queries, num_queries, list, d_records, d_points, d_signed, (hipStream_t)stream);
}
