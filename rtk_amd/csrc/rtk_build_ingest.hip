// rtk_build_ingest.hip -- the device build's first stages (rtk_build_internal.h has the map): every mesh of a description, or the
// records of a live scene, decoded into staged triangles, doubled centroids and their bounds; then the Morton keys and their sort.
#include "rtk_build_internal.h"
#include "rtk_place_rule.h"

#include <math.h>
#include <string.h>

#include <algorithm>

using namespace rtk_bld;

namespace {

// ---------------------------------------------------------------------------------- 1 ingest

__device__ __forceinline__ uint32_t f2ord(float f)
{
	const uint32_t b = __float_as_uint(f);
	return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float ord2f(uint32_t u)
{
	return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// IDX: 0 implicit (3i,3i+1,3i+2), 1 u16, 2 u32 (rtk.c:1028-1070). F64: positions are doubles (rtk.c:1098, B20).
// Compile-time variants: the index and position formats are per mesh, so each launch is one straight-line path.
// (A run-time form of this kernel, k_ingest(pos, stride, int pos_type, idx, stride, int idx_type, ...), faulted once in
// round 1 -- HSA_STATUS_ERROR_MEMORY_APERTURE_VIOLATION on the f64 + u16 mesh of test_edge_scene_indexed_multi_mesh,
// gpurun_out/pytest_dbg.log. That source was never committed, so the cause cannot be settled from the repository; what the
// recorded dispatch is consistent with is a type code reaching the kernel that selected the 32-bit read of the 16-bit index
// buffer: garbage indices times a 24-byte stride leave the legal address range. Nothing run-time is left to get wrong: the
// host validates both type codes -- positions {DEFAULT, REAL, F32, F64}, indices {DEFAULT, U16, U32}, anything else is an
// error as in rtk.c:1080-1113 -- and picks the variant from the validated codes; every arm is covered by tests/test_gpu_build.py.)
// The bounds of the triangle centroids (x2, see k_bounds) are taken in the same pass: one 1024-thread workgroup per CU at
// most, so the six result words see a few hundred atomics, not tens of thousands.
#define INGEST_BLOCK 1024
// DIRECT (implicit indices, float positions): nothing is staged -- k_emit_tris gathers the three vertices of a sorted triangle
// straight from the caller's (or the uploaded) position buffer. Every form writes the doubled centroid (12 B: all k_morton
// needs; it used to read the whole 48-byte staged record for it) and, if the scene keeps them (vidx_in: some mesh is indexed),
// the original vertex indices in input order.
// PLACED (rtk_dev_scene_build_placed): every vertex goes through the mesh's placement (rtk_place_rule.h) as soon as it is a
// float, so the staged record, the centroid and the bounds are those of the placed mesh. Never together with DIRECT: the emit
// would have to place the vertices a second time, so a placed mesh is always staged.
template <int IDX, bool F64, bool DIRECT, bool PLACED>
__global__ void __launch_bounds__(INGEST_BLOCK) k_ingest(const char *pos, unsigned long long pos_stride, const char *idx,
	unsigned long long idx_stride, uint32_t ntris, uint32_t base, InTri *in_tris, float *cent, uint32_t *vidx_in, uint32_t *bounds, rtk_placement place)
{
	static_assert(!(DIRECT && PLACED), "a placed mesh is staged");
	__shared__ float s_mn[3][INGEST_BLOCK / 64], s_mx[3][INGEST_BLOCK / 64];
	float mn[3] = { INFINITY, INFINITY, INFINITY }, mx[3] = { -INFINITY, -INFINITY, -INFINITY };
	for (uint32_t i = blockIdx.x * INGEST_BLOCK + threadIdx.x; i < ntris; i += gridDim.x * INGEST_BLOCK) {
		uint32_t v0, v1, v2;
		if (IDX == 0) {
			v0 = 3u * i; v1 = 3u * i + 1u; v2 = 3u * i + 2u;
		} else if (IDX == 1) {
			const uint16_t *p = reinterpret_cast<const uint16_t *>(idx + (size_t)i * idx_stride);
			v0 = p[0]; v1 = p[1]; v2 = p[2];
		} else {
			const uint32_t *p = reinterpret_cast<const uint32_t *>(idx + (size_t)i * idx_stride);
			v0 = p[0]; v1 = p[1]; v2 = p[2];
		}
		const uint32_t vi[3] = { v0, v1, v2 };
		const size_t g = (size_t)base + (size_t)i;
		InTri rec;
#pragma unroll
		for (int c = 0; c < 3; c++) {
			float x, y, z;
			if (F64) {
				const double *p = reinterpret_cast<const double *>(pos + (size_t)vi[c] * pos_stride);
				x = (float)p[0]; y = (float)p[1]; z = (float)p[2];
			} else {
				const float *p = reinterpret_cast<const float *>(pos + (size_t)vi[c] * pos_stride);
				x = p[0]; y = p[1]; z = p[2];
			}
			if (PLACED) rtk_place_vertex(place.m, x, y, z);
			rec.p[3 * c + 0] = x;
			rec.p[3 * c + 1] = y;
			rec.p[3 * c + 2] = z;
			rec.vi[c] = vi[c];
		}
		if (!DIRECT) {
			float4 *out = reinterpret_cast<float4 *>(in_tris + g);
			const float4 *src = reinterpret_cast<const float4 *>(&rec);
			out[0] = src[0]; out[1] = src[1]; out[2] = src[2];
		}
		if (vidx_in) { vidx_in[3 * g + 0] = vi[0]; vidx_in[3 * g + 1] = vi[1]; vidx_in[3 * g + 2] = vi[2]; }
#pragma unroll
		for (int a = 0; a < 3; a++) {
			const float lo = fminf(fminf(rec.p[a], rec.p[3 + a]), rec.p[6 + a]);
			const float hi = fmaxf(fmaxf(rec.p[a], rec.p[3 + a]), rec.p[6 + a]);
			const float c2 = lo + hi;
			cent[3 * g + a] = c2;
			mn[a] = fminf(mn[a], c2);
			mx[a] = fmaxf(mx[a], c2);
		}
	}
#pragma unroll
	for (int a = 0; a < 3; a++) {
		for (int o = 32; o > 0; o >>= 1) {
			mn[a] = fminf(mn[a], __shfl_xor(mn[a], o));
			mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], o));
		}
		if ((threadIdx.x & 63u) == 0) { s_mn[a][threadIdx.x >> 6] = mn[a]; s_mx[a][threadIdx.x >> 6] = mx[a]; }
	}
	__syncthreads();
	if (threadIdx.x < 3) {
		const int a = threadIdx.x;
		float lo = s_mn[a][0], hi = s_mx[a][0];
		for (int w = 1; w < INGEST_BLOCK / 64; w++) { lo = fminf(lo, s_mn[a][w]); hi = fmaxf(hi, s_mx[a][w]); }
		atomicMin(&bounds[a], f2ord(lo));
		atomicMax(&bounds[3 + a], f2ord(hi));
	}
}

// place: the mesh's placement, or NULL (never with `direct`)
template <int IDX>
void launch_ingest(bool f64, bool direct, const rtk_placement *place, unsigned blocks, const char *pos, unsigned long long pstride, const char *idx,
	unsigned long long istride, uint32_t nt, uint32_t base, InTri *in_tris, float *cent, uint32_t *vidx_in, uint32_t *bounds, hipStream_t stream)
{
	const rtk_placement pl = place ? *place : rtk_placement{};
#define INGEST_LAUNCH(...) hipLaunchKernelGGL((k_ingest<__VA_ARGS__>), dim3(blocks), dim3(INGEST_BLOCK), 0, stream, pos, pstride, idx, istride, nt, base, in_tris, cent, vidx_in, bounds, pl)
	if (place && f64) INGEST_LAUNCH(IDX, true, false, true);
	else if (place) INGEST_LAUNCH(IDX, false, false, true);
	else if (direct) INGEST_LAUNCH(0, false, true, false);
	else if (f64) INGEST_LAUNCH(IDX, true, false, false);
	else INGEST_LAUNCH(IDX, false, false, false);
#undef INGEST_LAUNCH
}

// ---------------------------------------------------------------------------------- 2 bounds

// bounds[0..2] = min of centroid*2 (ordered uint), bounds[3..5] = max. One 1024-thread workgroup per CU: the six result
// words take ~300 atomics/us between them, and 2048 workgroups x 6 atomics cost four times the data pass at 1M triangles.
#define BOUNDS_BLOCK 1024
// (the staged records [first, first + n) of one host-decoded mesh: their doubled centroids, vertex indices and bounds)
__global__ void __launch_bounds__(BOUNDS_BLOCK) k_bounds(const InTri *in_tris, uint32_t first, uint32_t n, uint32_t *bounds, float *cent, uint32_t *vidx_in)
{
	__shared__ float s_mn[3][BOUNDS_BLOCK / 64], s_mx[3][BOUNDS_BLOCK / 64];
	float mn[3] = { INFINITY, INFINITY, INFINITY }, mx[3] = { -INFINITY, -INFINITY, -INFINITY };
	for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (size_t)gridDim.x * blockDim.x) {
		const size_t i = (size_t)first + k;
		const float *p = in_tris[i].p;
#pragma unroll
		for (int a = 0; a < 3; a++) {
			const float lo = fminf(fminf(p[a], p[3 + a]), p[6 + a]);
			const float hi = fmaxf(fmaxf(p[a], p[3 + a]), p[6 + a]);
			const float c2 = lo + hi;
			cent[3 * i + a] = c2;
			if (vidx_in) vidx_in[3 * i + a] = in_tris[i].vi[a];
			mn[a] = fminf(mn[a], c2);
			mx[a] = fmaxf(mx[a], c2);
		}
	}
#pragma unroll
	for (int a = 0; a < 3; a++) {
		for (int o = 32; o > 0; o >>= 1) {
			mn[a] = fminf(mn[a], __shfl_xor(mn[a], o));
			mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], o));
		}
		if ((threadIdx.x & 63u) == 0) { s_mn[a][threadIdx.x >> 6] = mn[a]; s_mx[a][threadIdx.x >> 6] = mx[a]; }
	}
	__syncthreads();
	if (threadIdx.x < 3) {
		const int a = threadIdx.x;
		float lo = s_mn[a][0], hi = s_mx[a][0];
		for (int w = 1; w < BOUNDS_BLOCK / 64; w++) { lo = fminf(lo, s_mn[a][w]); hi = fmaxf(hi, s_mx[a][w]); }
		atomicMin(&bounds[a], f2ord(lo));
		atomicMax(&bounds[3 + a], f2ord(hi));
	}
}

// ---------------------------------------------------------------------------------- 1b staging from a scene (rebuild)

// rtk_dev_scene_rebuild's ingest: the triangles come from the finished records of a scene, not from a description. One thread per
// slot reads its 48-byte record (a wave reads 3 KB in a row) and writes, under the record's primitive id g -- the number k_morton
// and the sort know the triangle by, so ties between equal codes break as in a build from a description --, the doubled centroid
// in k_ingest's arithmetic and the slot the record lies in (k_refit_tile's make_tri gathers old_tris[slot_of[g]]). The bounds
// of the centroids are taken as k_ingest takes them. vidx_out (a scene that arrived as a blob: its vertex indices exist only
// by slot): the original vertex indices in primitive order, which the scene owns from then on.
// slot_of starts out as all ones: with as many slots as primitives an id that is met twice leaves another one unmet, so the
// words k_stage_check still finds at all ones, plus the ids beyond the range counted here, say whether every primitive has
// exactly one record.
#define STAGE_BLOCK 1024
#define STAGE_BAD_WORD 8          // of the sixteen bounds words: records whose primitive id cannot be staged
__global__ void __launch_bounds__(STAGE_BLOCK) k_stage_scene(const DevTri *old_tris, uint32_t n, const uint32_t *vertex_index, float *cent, uint32_t *slot_of,
	uint32_t *vidx_out, uint32_t *bounds)
{
	__shared__ float s_mn[3][STAGE_BLOCK / 64], s_mx[3][STAGE_BLOCK / 64];
	float mn[3] = { INFINITY, INFINITY, INFINITY }, mx[3] = { -INFINITY, -INFINITY, -INFINITY };
	uint32_t bad = 0;
	for (uint32_t s = blockIdx.x * STAGE_BLOCK + threadIdx.x; s < n; s += gridDim.x * STAGE_BLOCK) {
		const float4 *rec = reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(old_tris) + (size_t)s * RTK_TRI_STRIDE);
		const float4 a = rec[0], b = rec[1], c = rec[2];      // v0 prim | v1 flags | v2 spare
		const uint32_t g = __float_as_uint(a.w);
		if (g >= n) { bad++; continue; }
		const float p[9] = { a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z };
		slot_of[g] = s;
		if (vidx_out) { vidx_out[3 * (size_t)g + 0] = vertex_index[3 * (size_t)s + 0]; vidx_out[3 * (size_t)g + 1] = vertex_index[3 * (size_t)s + 1]; vidx_out[3 * (size_t)g + 2] = vertex_index[3 * (size_t)s + 2]; }
#pragma unroll
		for (int ax = 0; ax < 3; ax++) {
			const float lo = fminf(fminf(p[ax], p[3 + ax]), p[6 + ax]);
			const float hi = fmaxf(fmaxf(p[ax], p[3 + ax]), p[6 + ax]);
			const float c2 = lo + hi;
			cent[3 * (size_t)g + ax] = c2;
			mn[ax] = fminf(mn[ax], c2);
			mx[ax] = fmaxf(mx[ax], c2);
		}
	}
#pragma unroll
	for (int a = 0; a < 3; a++) {
		for (int o = 32; o > 0; o >>= 1) {
			mn[a] = fminf(mn[a], __shfl_xor(mn[a], o));
			mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], o));
		}
		if ((threadIdx.x & 63u) == 0) { s_mn[a][threadIdx.x >> 6] = mn[a]; s_mx[a][threadIdx.x >> 6] = mx[a]; }
	}
	for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o);
	if ((threadIdx.x & 63u) == 0 && bad) atomicAdd(&bounds[STAGE_BAD_WORD], bad);
	__syncthreads();
	if (threadIdx.x < 3) {
		const int a = threadIdx.x;
		float lo = s_mn[a][0], hi = s_mx[a][0];
		for (int w = 1; w < STAGE_BLOCK / 64; w++) { lo = fminf(lo, s_mn[a][w]); hi = fmaxf(hi, s_mx[a][w]); }
		atomicMin(&bounds[a], f2ord(lo));
		atomicMax(&bounds[3 + a], f2ord(hi));
	}
}

// primitives no record names (see above), added to the count of ids out of range
__global__ void __launch_bounds__(256) k_stage_check(const uint32_t *slot_of, uint32_t n, uint32_t *bounds)
{
	const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
	const unsigned long long unmet = __ballot(g < n && slot_of[g] == 0xffffffffu);
	if ((threadIdx.x & 63u) == 0 && unmet) atomicAdd(&bounds[STAGE_BAD_WORD], (uint32_t)__popcll(unmet));
}

// ---------------------------------------------------------------------------------- 3 morton

__device__ __forceinline__ unsigned long long spread21(uint32_t v)
{
	unsigned long long x = v & 0x1fffffu;
	x = (x | (x << 32)) & 0x1f00000000ffffull;
	x = (x | (x << 16)) & 0x1f0000ff0000ffull;
	x = (x | (x << 8)) & 0x100f00f00f00f00full;
	x = (x | (x << 4)) & 0x10c30c30c30c30c3ull;
	x = (x | (x << 2)) & 0x1249249249249249ull;
	return x;
}

__global__ void k_morton(const float *cent, uint32_t n, const uint32_t *bounds, unsigned long long *keys, uint32_t *vals, uint32_t drop_bits)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	uint32_t q[3];
#pragma unroll
	for (int a = 0; a < 3; a++) {
		const float lo = ord2f(bounds[a]), hi = ord2f(bounds[3 + a]);
		const float c2 = cent[3 * (size_t)i + a];            // min + max of the triangle's three coordinates, as the ingest pass left it
		const float ext = hi - lo;
		float t = ext > 0.0f ? (c2 - lo) / ext : 0.0f;
		t = fminf(fmaxf(t, 0.0f), 1.0f);
		uint32_t v = (uint32_t)(t * 2097152.0f);
		q[a] = v > 2097151u ? 2097151u : v;
	}
	const unsigned long long code = (spread21(q[0]) << 2) | (spread21(q[1]) << 1) | spread21(q[2]);
	if (vals) {
		keys[i] = code >> drop_bits;                               // most significant bits only
		vals[i] = i;
	} else {
		// fewer than 2^24 triangles: the top `63 - drop_bits` (24 ... 40, a multiple of 8) bits of the code above the triangle's
		// own number. One 8-byte word per triangle goes through three to five sort passes instead of a 12-byte pair through six.
		keys[i] = ((code >> drop_bits) << 24) | (unsigned long long)i;
	}
}

// ---------------------------------------------------------------------------------- host side

// Host decode of a mesh that uses callbacks (rtk.c:1030-1033, 1074-1077), 128 triangles per call.
void decode_mesh_on_host(const rtk_mesh *m, float *pos9, uint32_t *vidx3)
{
	size_t offset = 0, left = m->num_triangles;
	while (left) {
		const size_t chunk = left > 128 ? 128 : left;
		uint32_t indices[128 * 3];
		rtk_vec3 verts[128 * 3 + 1];
		if (m->index_cb) m->index_cb(m->index_cb_user, m, indices, offset, chunk);
		else if (m->index.data) {
			const size_t stride = m->index.stride ? m->index.stride : (m->index.type == RTK_TYPE_U16 ? 6 : 12);
			for (size_t i = 0; i < chunk; i++) {
				const char *p = (const char *)m->index.data + (offset + i) * stride;
				for (int c = 0; c < 3; c++)
					indices[3 * i + c] = m->index.type == RTK_TYPE_U16 ? ((const uint16_t *)p)[c] : ((const uint32_t *)p)[c];
			}
		} else {
			for (size_t i = 0; i < chunk; i++) for (int c = 0; c < 3; c++) indices[3 * i + c] = (uint32_t)(offset + i) * 3u + c;
		}
		if (m->position_cb) m->position_cb(m->position_cb_user, m, verts, indices, chunk);
		else {
			const bool f64 = m->position.type == RTK_TYPE_F64;
			const size_t stride = m->position.stride ? m->position.stride : (f64 ? 24 : 12);
			for (size_t i = 0; i < 3 * chunk; i++) {
				const char *p = (const char *)m->position.data + (size_t)indices[i] * stride;
				if (f64) { verts[i].x = (float)((const double *)p)[0]; verts[i].y = (float)((const double *)p)[1]; verts[i].z = (float)((const double *)p)[2]; }
				else { verts[i].x = ((const float *)p)[0]; verts[i].y = ((const float *)p)[1]; verts[i].z = ((const float *)p)[2]; }
			}
		}
		for (size_t i = 0; i < 3 * chunk; i++) {
			pos9[3 * (3 * offset + i) + 0] = verts[i].x;
			pos9[3 * (3 * offset + i) + 1] = verts[i].y;
			pos9[3 * (3 * offset + i) + 2] = verts[i].z;
			vidx3[3 * offset + i] = indices[i];
		}
		offset += chunk;
		left -= chunk;
	}
}

// Host memory -> device. A plain hipMemcpy (the runtime's own pinned staging) measured faster on the
// GPU box than a hand-rolled double-buffered copy (19 vs 25 ms per 10M-triangle build, steady state).
// (on the build's stream: a plain hipMemcpy from pageable memory is ordered with the NULL stream only, and may return before its
// DMA has landed -- kernels on another stream would not wait for it. The caller's buffers outlive the build.)
hipError_t upload_staged(void *dst, const void *src, size_t bytes, hipStream_t stream)
{
	return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream);
}

// the decoded corners of a mesh (pos9: 9 floats per triangle) under its placement: the host's side of rtk_place_rule.h
void place_on_host(const rtk_placement &pl, float *pos9, size_t num_triangles)
{
	for (size_t v = 0; v < 3 * num_triangles; v++) rtk_place_vertex(pl.m, pos9[3 * v], pos9[3 * v + 1], pos9[3 * v + 2]);
}

} // namespace

namespace rtk_bld {

// ---- fewer than two triangles: no radix tree to build, no workspace; one root node, at most one leaf ----
rtk_dev_scene *build_tiny(const rtk_scene_desc *desc, const std::vector<uint64_t> &mesh_base, const rtk_placement *placements)
{
	std::vector<float> pos;
	std::vector<uint32_t> vidx;
	for (size_t mi = 0; mi < desc->num_meshes; mi++) {
		const rtk_mesh *m = &desc->meshes[mi];
		if (m->num_triangles == 0) continue;
		pos.resize(9 * m->num_triangles);
		vidx.resize(3 * m->num_triangles);
		decode_mesh_on_host(m, pos.data(), vidx.data());
		if (placements) place_on_host(placements[mi], pos.data(), m->num_triangles);
	}
	HostBvh h;
	h.mesh_base = mesh_base;
	h.max_depth = 1;
	DevNode root;
	memset(&root, 0, sizeof(root));
	for (int k = 0; k < 4; k++) {
		root.bx[0][k] = root.by[0][k] = root.bz[0][k] = +1.0f;
		root.bx[1][k] = root.by[1][k] = root.bz[1][k] = -1.0f;
		root.child[k] = RTK_REF_NONE;
	}
	const size_t n = pos.size() / 9;
	if (n == 1) {
		DevTri t;
		memset(&t, 0, sizeof(t));
		for (int a = 0; a < 3; a++) { t.v0[a] = pos[a]; t.v1[a] = pos[3 + a]; t.v2[a] = pos[6 + a]; }
		t.prim = 0; t.spare = 1;
		h.tris.push_back(t);
		for (int c = 0; c < 3; c++) h.vertex_index.push_back(vidx[c]);
		uint32_t mesh = 0;
		while (mesh + 1 < mesh_base.size() - 1 && mesh_base[mesh + 1] == 0) mesh++;
		t.flags = RTK_TRI_LAST | (mesh << 8);
		h.tris.back() = t;
		h.slot_mesh.push_back(mesh);
		h.slot_tri.push_back(0);
		float mn[3], mx[3];
		for (int a = 0; a < 3; a++) { mn[a] = std::min(std::min(t.v0[a], t.v1[a]), t.v2[a]); mx[a] = std::max(std::max(t.v0[a], t.v1[a]), t.v2[a]); }
		root.bx[0][0] = mn[0]; root.bx[1][0] = mx[0];
		root.by[0][0] = mn[1]; root.by[1][0] = mx[1];
		root.bz[0][0] = mn[2]; root.bz[1][0] = mx[2];
		root.child[0] = RTK_REF_LEAF | 0u;
	}
	h.nodes.push_back(root);
	rtk_dev_scene *ds = rtk_dev_scene_from_host_bvh(h);
	if (ds) ds->tree.boxes_exact = true;       // (as finish() says of every device build)
	return ds;
}

// ---- 1 ingest: the scene object; every mesh decoded into staged triangles, doubled centroids and their bounds ----
bool ingest(Build &b)
{
	const rtk_scene_desc *desc = b.desc;
	const hipStream_t bs = b.bs;
	// the scene keeps the original vertex indices in input order (for rtk_hit.vertex[].index: rtk_scene_side_arrays) only if some
	// mesh HAS indices; with implicit indices everywhere they are 3 * triangle + corner
	bool any_indexed = false;
	for (size_t mi = 0; mi < desc->num_meshes; mi++) any_indexed = any_indexed || (desc->meshes[mi].num_triangles && (b.plans[mi].on_host_decode || b.plans[mi].idx_kind != 0));
	rtk_dev_scene *ds = b.ds = new rtk_dev_scene();
	ds->device = b.device;
	ds->num_cus = b.num_cus;
	ds->mesh_base = b.mesh_base;
	ds->side_ready = false;
	uint32_t *d_vidx_in = nullptr;
	if (any_indexed) {
		d_vidx_in = (uint32_t *)b.dev_alloc(3 * (size_t)b.n * 4);
		if (!d_vidx_in) { (void)hipGetLastError(); rtk_set_error("device build: out of device memory (vertex indices)"); return b.give_up(); }
		ds->tree.d_vidx_in = d_vidx_in;
	}
	b.mesh_src.assign(desc->num_meshes + 1, MeshSrc{ nullptr, 0ull });
	// centroid bounds: min words start at all ones, max words at zero (ordered-uint encoding): two fills, nothing the host
	// waits for. The decode kernels below take them in passing.
	if (hipMemsetAsync(b.d_bounds, 0xff, 12, bs) != hipSuccess || hipMemsetAsync(b.d_bounds + 3, 0, 12, bs) != hipSuccess) return b.fail("memset");
	for (size_t mi = 0; mi < desc->num_meshes; mi++) {
		const rtk_mesh *m = &desc->meshes[mi];
		const MeshPlan &pl = b.plans[mi];
		const size_t nt = m->num_triangles;
		if (nt == 0) continue;
		const uint32_t base = (uint32_t)b.mesh_base[mi];
		if (pl.on_host_decode) {
			std::vector<float> pos9(9 * nt);
			std::vector<uint32_t> vidx3(3 * nt);
			decode_mesh_on_host(m, pos9.data(), vidx3.data());
			if (b.placements) place_on_host(b.placements[mi], pos9.data(), nt);
			std::vector<InTri> recs(nt);
			for (size_t t = 0; t < nt; t++) {
				for (int c = 0; c < 9; c++) recs[t].p[c] = pos9[9 * t + c];
				for (int c = 0; c < 3; c++) recs[t].vi[c] = vidx3[3 * t + c];
			}
			if (hipMemcpyAsync(b.in_tris + base, recs.data(), recs.size() * sizeof(InTri), hipMemcpyHostToDevice, bs) != hipSuccess) return b.fail("copy of host-decoded triangles");
			// centroids, vertex indices and centroid bounds of these records (the decode kernels below do this in passing)
			const unsigned bblocks = (unsigned)std::min<size_t>((nt + BOUNDS_BLOCK - 1) / BOUNDS_BLOCK, (size_t)b.num_cus);
			hipLaunchKernelGGL(k_bounds, dim3(bblocks), dim3(BOUNDS_BLOCK), 0, bs, b.in_tris, base, (uint32_t)nt, b.d_bounds, b.d_cent, d_vidx_in);
			if (hipStreamSynchronize(bs) != hipSuccess) return b.fail("host-decoded mesh");      // (recs goes out of scope)
			continue;
		}
		// raw buffers go to the device as they are; the decode runs there
		const char *idx_ptr = pl.idx_src, *pos_ptr = pl.pos_src;
		if (pl.ibytes) {
			char *d = b.at<char>(b.L.mesh_idx[mi]);
			if (upload_staged(d, pl.idx_src, pl.ibytes, bs) != hipSuccess) return b.fail("upload of indices");
			idx_ptr = d;
		}
		if (pl.pbytes) {
			char *d = b.at<char>(b.L.mesh_pos[mi]);
			if (upload_staged(d, pl.pos_src, pl.pbytes, bs) != hipSuccess) return b.fail("upload of positions");
			pos_ptr = d;
		}
		// implicit indices and float positions whose three components can be read as floats in place: gathered in place by k_emit_tris
		// (not a placed mesh: its vertices are placed once, here, and staged)
		const rtk_placement *place = b.placements ? &b.placements[mi] : nullptr;
		const bool direct = !place && b.knobs.direct && pl.idx_kind == 0 && !pl.f64 && (pl.pstride % 4u) == 0u && ((uintptr_t)pos_ptr % 4u) == 0u;
		if (direct) b.mesh_src[mi] = MeshSrc{ pos_ptr, (unsigned long long)pl.pstride };
		const unsigned iblocks = (unsigned)std::min<size_t>((nt + INGEST_BLOCK - 1) / INGEST_BLOCK, (size_t)b.num_cus);
		if (pl.idx_kind == 0) launch_ingest<0>(pl.f64, direct, place, iblocks, pos_ptr, pl.pstride, idx_ptr, pl.istride, (uint32_t)nt, base, b.in_tris, b.d_cent, d_vidx_in, b.d_bounds, bs);
		else if (pl.idx_kind == 1) launch_ingest<1>(pl.f64, false, place, iblocks, pos_ptr, pl.pstride, idx_ptr, pl.istride, (uint32_t)nt, base, b.in_tris, b.d_cent, d_vidx_in, b.d_bounds, bs);
		else launch_ingest<2>(pl.f64, false, place, iblocks, pos_ptr, pl.pstride, idx_ptr, pl.istride, (uint32_t)nt, base, b.in_tris, b.d_cent, d_vidx_in, b.d_bounds, bs);
		if (hipGetLastError() != hipSuccess) return b.fail("ingest launch");
	}
	b.stage("ingest");
	return true;
}

// ---- 1b the other ingest: the records of a live scene (rtk_dev_scene_rebuild). The new scene object; centroids, their bounds and
// [primitive] -> slot from the old records (k_stage_scene); the one refusal that needs the device ----
bool ingest_scene(Build &b)
{
	const rtk_dev_scene *from = b.from;
	const hipStream_t bs = b.bs;
	rtk_dev_scene *ds = b.ds = new rtk_dev_scene();
	ds->device = b.device;
	ds->num_cus = b.num_cus;
	ds->mesh_base = b.mesh_base;
	ds->side_ready = false;
	// The vertex indices in input order. A scene the device built has them, or needs none (implicit indices everywhere): either
	// way they are in input order already and stay where they are. A scene that arrived as a blob (no mesh table on the device:
	// only a build makes one) has them by slot alone, in its side arrays: they are staged by primitive here.
	const bool from_blob = !from->tree.d_mesh_base && !from->tree.d_vidx_in;
	uint32_t *vidx_out = nullptr;
	if (from_blob) {
		if (!from->view.vertex_index) { b.rc = RTK_AMD_ERR_BAD_SCENE; rtk_set_error("rtk_dev_scene_rebuild: the scene has no vertex indices"); return b.give_up(); }
		vidx_out = (uint32_t *)b.dev_alloc(3 * (size_t)b.n * 4);
		if (!vidx_out) { (void)hipGetLastError(); b.rc = RTK_AMD_ERR_OOM; rtk_set_error("device build: out of device memory (vertex indices)"); return b.give_up(); }
		ds->tree.d_vidx_in = vidx_out;
	} else ds->tree.d_vidx_in = from->tree.d_vidx_in;        // (an entry of the live scene's ledger, not of this one's: it survives either outcome)
	b.mesh_src.assign(b.num_meshes + 1, MeshSrc{ nullptr, 0ull });
	uint32_t *slot_of = reinterpret_cast<uint32_t *>(b.in_tris);      // (nothing is staged as InTri: the region holds [primitive] -> slot)
	if (hipMemsetAsync(b.d_bounds, 0xff, 12, bs) != hipSuccess || hipMemsetAsync(b.d_bounds + 3, 0, 12, bs) != hipSuccess ||
		hipMemsetAsync(b.d_bounds + STAGE_BAD_WORD, 0, 4, bs) != hipSuccess || hipMemsetAsync(slot_of, 0xff, (size_t)b.n * 4, bs) != hipSuccess) return b.fail("memset");
	const unsigned blocks = (unsigned)std::min<size_t>(((size_t)b.n + STAGE_BLOCK - 1) / STAGE_BLOCK, (size_t)b.num_cus);
	hipLaunchKernelGGL(k_stage_scene, dim3(blocks), dim3(STAGE_BLOCK), 0, bs, from->view.tris, b.n, from->view.vertex_index, b.d_cent, slot_of, vidx_out, b.d_bounds);
	hipLaunchKernelGGL(k_stage_check, dim3((b.n + 255u) / 256u), dim3(256), 0, bs, slot_of, b.n, b.d_bounds);
	if (hipGetLastError() != hipSuccess) return b.fail("staging launch");
	// (the one wait a build from a description does not have: the emit gathers through slot_of, which must be whole before it is trusted)
	b.results->pad = 0u;
	if (hipMemcpyAsync(&b.results->pad, b.d_bounds + STAGE_BAD_WORD, 4, hipMemcpyDeviceToHost, bs) != hipSuccess || hipStreamSynchronize(bs) != hipSuccess) return b.fail("staging");
	if (b.results->pad != 0u) {
		b.rc = RTK_AMD_ERR_UNSUPPORTED;
		rtk_set_error("rtk_dev_scene_rebuild: %u of %u primitives do not have exactly one triangle record", b.results->pad, b.n);
		return b.give_up();
	}
	b.old_tris = from->view.tris;
	b.slot_of = slot_of;
	b.stage("ingest");
	return true;
}

// ---- 2 bounds, 3 morton, 4 sort: no allocation, no host synchronisation ----
// 63-bit Morton keys resolve 2^-21 of the scene per axis; for < 2^24 triangles the low bits never decide a
// split that matters (lab: identical visit counts down to 30 bits at 1M triangles), so the top 40 bits are kept
// and share one 64-bit word with the triangle's number: 5 radix passes over 8-byte words (see k_morton) instead of
// 8 over 12-byte pairs.
bool keys_and_sort(Build &b)
{
	const uint32_t n = b.n;
	unsigned long long *keys_a = b.at<unsigned long long>(b.L.keys_a), *keys_b = b.at<unsigned long long>(b.L.keys_b);
	uint32_t *vals_a = b.at<uint32_t>(b.L.vals_a), *vals_b = b.at<uint32_t>(b.L.vals_b);       // (NULL when packed)
	uint32_t *sort_scratch = b.at<uint32_t>(b.L.sort_scratch);
	hipLaunchKernelGGL(k_morton, dim3((n + 255u) / 256u), dim3(256), 0, b.bs, b.d_cent, n, b.d_bounds, keys_a, vals_a, 63u - (b.plan.packed ? b.plan.packed_bits : BUILD_KEY_BITS));
	if (hipGetLastError() != hipSuccess) return b.fail("morton launch");
	b.stage("morton");
	const bool in_b = b.plan.packed ? rtk_sort_words_async(keys_a, keys_b, n, 24u, 24u + b.plan.packed_bits, sort_scratch, b.bs)
	                           : rtk_sort_pairs_async(keys_a, keys_b, vals_a, vals_b, n, BUILD_KEY_BITS, sort_scratch, b.bs);
	b.keys = in_b ? keys_b : keys_a;
	b.vals = b.plan.packed ? nullptr : (in_b ? vals_b : vals_a);
	if (hipGetLastError() != hipSuccess) return b.fail("sort launch");
	b.stage("sort");
	return true;
}

} // namespace rtk_bld
