// rtk_build.hip -- scene construction on the GPU (gfx950): Morton-code LBVH, bottom-up
// refit with a surface-area leaf/treelet decision, greedy collapse to 4-wide nodes.
//
// Stands in for the reference's CPU builder (rtk.c:1362-1622: triangle setup tasks,
// binned-SAH node tasks, finalize, linearize). The reference's topology is not part of
// the parity contract -- only the hits are -- so the construction is re-designed for the
// GPU; what IS kept from the reference: triangle identity (mesh_index, per-mesh
// triangle_index, rtk.c:1168-1169), index/position decoding rules (rtk.c:1028-1114),
// <= 63 triangles per leaf (rtk.c:188), and the blob format on export.
//
// Stages (all device kernels; the host only sequences launches):
//   1 ingest     decode indices + positions of every mesh into 48-B staged triangles; centroid bounds in passing
//   2 bounds     (separate pass only for host-decoded meshes)
//   3 morton     63-bit Morton code per triangle; below 2^24 triangles its top 40 bits over the triangle's number
//   4 sort       LSD radix sort, 8-bit digits, per-wave LDS histograms and counters (rtk_sort.hip)
//   5 emit       triangles gathered into Morton order = final 48 B leaf records
//   6 + 7 refit  binary radix tree built bottom-up together with its AABBs and the SAH leaf decision: tile-local in
//                LDS, then the nodes that cross tile borders with memory-side atomics
//   8 collapse   breadth-first, level by level: binary tree -> 128 B 4-wide nodes
#include "rtk_dev.h"
#include "rtk_build_layout.h"
#include "rtk_node_finish.h"
#include "rtk_place_rule.h"

#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <mutex>

void rtk_cache_adopt(const rtk_scene *scene, rtk_dev_scene *ds);

namespace {

struct BinNode {                  // 32 B, written by refit
	float mn[3];
	uint32_t cnt_flag;            // bits 0..30 triangles below, bit 31 = collapses to ONE leaf
	float mx[3];
	float cost;
};
static_assert(sizeof(BinNode) == 32, "BinNode");

struct BuildParams {
	float cost_tri;               // per triangle tested
	float cost_node;              // per binary inner node
	uint32_t max_leaf;
};

// ---------------------------------------------------------------------------------- 1 ingest

// One decoded triangle in input order: 48 B = three 16-B pieces, so that the gather by sorted order in k_emit_tris
// is three loads from (on average) 1.4 lines instead of twelve from two arrays.
struct InTri {
	float p[9];          // v0.xyz, v1.xyz, v2.xyz
	uint32_t vi[3];      // original vertex indices (rtk_vertex.index)
};
static_assert(sizeof(InTri) == 48, "InTri");

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

// ---------------------------------------------------------------------------------- 5 emit

// where the positions of a mesh's triangles are read from: its own buffer (implicit indices, float positions: vertex 3 i + c of
// triangle i at pos + (3 i + c) * stride), or the staged records (pos == NULL)
struct MeshSrc { const char *pos; unsigned long long stride; };

struct EmitSrc {
	const InTri *in_tris;                 // staged records (meshes that are not read in place)
	const MeshSrc *src;                   // per mesh: where its positions are read from
	const uint32_t *vals;                 // sorted order: triangle numbers (pairs), or NULL:
	const unsigned long long *words;      // packed sort words, the number in their low 24 bits
	const unsigned long long *mesh_base;
	uint32_t num_meshes;
	const DevTri *old_tris;               // a rebuild: the scene's records as they lie (NULL: a build from a description), and ...
	const uint32_t *slot_of;              // ... [primitive] -> the slot of its record
};

// the record of sorted triangle s: its positions gathered from the caller's position buffer (implicit float meshes), the staged records,
// or the records of the scene that is being rebuilt
__device__ __forceinline__ DevTri make_tri(const EmitSrc &e, uint32_t s)
{
	const uint32_t g = e.vals ? e.vals[s] : (uint32_t)(e.words[s] & 0xffffffull);     // packed sort words carry the index in their low 24 bits
	// mesh of global primitive g: last m with mesh_base[m] <= g
	uint32_t lo = 0, hi = e.num_meshes;
	while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (e.mesh_base[mid] <= g) lo = mid; else hi = mid; }
	const MeshSrc ms = e.old_tris ? MeshSrc{ nullptr, 0ull } : e.src[lo];
	DevTri t;
	if (e.old_tris) {
		const float4 *rec = reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(e.old_tris) + (size_t)e.slot_of[g] * RTK_TRI_STRIDE);
		const float4 a = rec[0], b = rec[1], c = rec[2];      // v0 prim | v1 flags | v2 spare
		t.v0[0] = a.x; t.v0[1] = a.y; t.v0[2] = a.z;
		t.v1[0] = b.x; t.v1[1] = b.y; t.v1[2] = b.z;
		t.v2[0] = c.x; t.v2[1] = c.y; t.v2[2] = c.z;
	} else if (ms.pos) {
		const size_t first = 3u * (size_t)(g - (uint32_t)e.mesh_base[lo]);
		const float *p0 = reinterpret_cast<const float *>(ms.pos + first * ms.stride);
		const float *p1 = reinterpret_cast<const float *>(ms.pos + (first + 1u) * ms.stride);
		const float *p2 = reinterpret_cast<const float *>(ms.pos + (first + 2u) * ms.stride);
		t.v0[0] = p0[0]; t.v0[1] = p0[1]; t.v0[2] = p0[2];
		t.v1[0] = p1[0]; t.v1[1] = p1[1]; t.v1[2] = p1[2];
		t.v2[0] = p2[0]; t.v2[1] = p2[1]; t.v2[2] = p2[2];
	} else {
		const float4 *rec = reinterpret_cast<const float4 *>(e.in_tris + g);
		const float4 a = rec[0], b = rec[1], c = rec[2];      // p0 p1 p2 p3 | p4 p5 p6 p7 | p8 vi0 vi1 vi2
		t.v0[0] = a.x; t.v0[1] = a.y; t.v0[2] = a.z;
		t.v1[0] = a.w; t.v1[1] = b.x; t.v1[2] = b.y;
		t.v2[0] = b.z; t.v2[1] = b.w; t.v2[2] = c.x;
	}
	// every record starts out as a leaf of its own (count 1, last of its leaf); the collapse rewrites only the
	// members of multi-triangle leaves
	t.prim = g;
	t.flags = (lo << 8) | RTK_TRI_LAST;   // mesh index above the flag bits (RTK_TRI_MESH_SHIFT)
	t.spare = 1u;
#if RTK_TRI_STRIDE == 64
	t.pad[0] = t.pad[1] = t.pad[2] = t.pad[3] = 0u;
#endif
	return t;
}

// stores the records of one wave (lane l: sorted triangle s_own, record t; n triangles in all). Every lane of the wave takes part.
__device__ __forceinline__ void store_tris(DevTri *tris, uint32_t s_own, uint32_t n, const DevTri &t)
{
#if RTK_TRI_STRIDE == 64
	if (s_own < n) tris[s_own] = t;
#else
	// The wave's 64 records are 192 16-byte pieces in a row: store k writes pieces 64 k + lane, 1 KB without a gap (a record per
	// lane is three stores of 16 bytes at a stride of 48: 64 partial lines each). Piece w of the record of lane r is number
	// 3 r + w: it goes to lane (3 r + w) mod 64 -- one to one, 3 and 64 have no common factor -- which receives one piece for
	// each of its three stores: the one of store k has w = (lane + k) mod 3 (64 = 1 mod 3).
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t piece[3][4] = {
		{ __float_as_uint(t.v0[0]), __float_as_uint(t.v0[1]), __float_as_uint(t.v0[2]), t.prim },
		{ __float_as_uint(t.v1[0]), __float_as_uint(t.v1[1]), __float_as_uint(t.v1[2]), t.flags },
		{ __float_as_uint(t.v2[0]), __float_as_uint(t.v2[1]), __float_as_uint(t.v2[2]), t.spare } };
	uint32_t got[3][4];
#pragma unroll
	for (uint32_t w = 0; w < 3u; w++) {
		const int to = (int)(((3u * lane + w) & 63u) << 2);
#pragma unroll
		for (int c = 0; c < 4; c++) got[w][c] = (uint32_t)__builtin_amdgcn_ds_permute(to, (int)piece[w][c]);
	}
	if (s_own - lane >= n) return;
	uint4 *out = reinterpret_cast<uint4 *>(tris + (s_own - lane));
	const uint32_t left = n - (s_own - lane);                               // records of this wave that exist
	const uint32_t w0 = lane % 3u;
#pragma unroll
	for (uint32_t k = 0; k < 3u; k++) {
		const uint32_t w = (w0 + k) % 3u, m = 64u * k + lane;
		uint4 v;
		const uint32_t a0 = got[0][0], a1 = got[1][0], a2 = got[2][0], b0 = got[0][1], b1 = got[1][1], b2 = got[2][1];
		const uint32_t c0 = got[0][2], c1 = got[1][2], c2 = got[2][2], d0 = got[0][3], d1 = got[1][3], d2 = got[2][3];
		v.x = w == 0u ? a0 : (w == 1u ? a1 : a2);
		v.y = w == 0u ? b0 : (w == 1u ? b1 : b2);
		v.z = w == 0u ? c0 : (w == 1u ? c1 : c2);
		v.w = w == 0u ? d0 : (w == 1u ? d1 : d2);
		if (m / 3u < left) out[m] = v;
	}
#endif
}

// (A/B only, RTK_AMD_FUSED_EMIT=0: the records are normally made inside k_refit_tile, which needs them next)
__global__ void k_emit_tris(EmitSrc e, uint32_t n, DevTri *tris)
{
	const uint32_t s_own = blockIdx.x * blockDim.x + threadIdx.x;
	if ((s_own & ~63u) >= n) return;                                            // (whole waves only: the stores are shared by the wave)
	const uint32_t s = s_own < n ? s_own : n - 1u;                              // (lanes behind the last triangle make a copy of it that is not written)
	store_tris(tris, s_own, n, make_tri(e, s));
	// (the side arrays -- original vertex indices, primitive -> slot, slot -> mesh / triangle -- were written here, 52 bytes per
	// triangle with one scattered word: rtk_scene_side_arrays makes them when something asks for a full rtk_hit, a validation or
	// an export, not in every build)
}

// The view's side arrays from the finished triangle records (DevTri carries the primitive id and the mesh index), once per scene.
__global__ void k_side_arrays(const DevTri *tris, uint32_t n, const unsigned long long *mesh_base, const uint32_t *vidx_in,
	uint32_t *vertex_index, uint32_t *prim_slot, uint32_t *slot_mesh, uint32_t *slot_tri)
{
	const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= n) return;
	const uint32_t *w = reinterpret_cast<const uint32_t *>(reinterpret_cast<const char *>(tris) + (size_t)s * RTK_TRI_STRIDE);
	const uint32_t g = w[3], mesh = w[7] >> 8;
	const uint32_t tri = g - (uint32_t)mesh_base[mesh];
	for (uint32_t c = 0; c < 3u; c++) vertex_index[3 * (size_t)s + c] = vidx_in ? vidx_in[3 * (size_t)g + c] : 3u * tri + c;
	prim_slot[g] = s;
	slot_mesh[s] = mesh;
	slot_tri[s] = tri;
}

// ---------------------------------------------------------------------------------- 6 tree topology
// The binary radix tree over the sorted keys (Karras 2012 defines it) is not built by a pass of its own any more: the
// refit pass below builds it bottom-up while it merges boxes (Apetrei 2014). A finished subtree over the sorted range
// [L, R] looks at the two keys on either side of its borders: it is the LEFT child of node R if its right neighbour is
// the more similar one (longer common prefix), else the RIGHT child of node L-1 -- an inner node is numbered by its split
// position (node m separates sorted triangles m and m+1). Two subtrees meet at every node; the second to arrive merges
// and climbs on. Same tree as the top-down search gives, without the search (0.33 ms at 10M triangles) and without the
// parent arrays.
//
// similarity of sorted keys i and i+1: length of their common prefix; equal keys (only on the (key, index) pair path) are
// told apart by their positions, as if the position were appended to the key. -1 outside the array.
__device__ __forceinline__ int key_delta(const unsigned long long *keys, int n, int i)
{
	if (i < 0 || i >= n - 1) return -1;
	const unsigned long long a = keys[i], b = keys[i + 1];
	if (a == b) return 64 + __clz((unsigned)(i ^ (i + 1)));
	return __clzll((long long)(a ^ b));
}

// ---------------------------------------------------------------------------------- 7 refit + SAH

__device__ __forceinline__ float half_area(const float mn[3], const float mx[3])
{
	const float x = mx[0] - mn[0], y = mx[1] - mn[1], z = mx[2] - mn[2];
	return x * y + y * z + z * x;
}

__device__ __forceinline__ void tri_box(const DevTri *tris, uint32_t s, float mn[3], float mx[3])
{
	const DevTri &t = tris[s];
#pragma unroll
	for (int a = 0; a < 3; a++) {
		mn[a] = fminf(fminf(t.v0[a], t.v1[a]), t.v2[a]);
		mx[a] = fmaxf(fmaxf(t.v0[a], t.v1[a]), t.v2[a]);
	}
}

// Record of a single sorted triangle seen as a subtree.
__device__ __forceinline__ BinNode leaf_record(const DevTri *tris, uint32_t s, const BuildParams &bp)
{
	BinNode b;
	tri_box(tris, s, b.mn, b.mx);
	b.cnt_flag = 1u;
	b.cost = bp.cost_tri * half_area(b.mn, b.mx);
	return b;
}

__device__ __forceinline__ BinNode leaf_record_of(const DevTri &t, const BuildParams &bp)
{
	BinNode b;
#pragma unroll
	for (int a = 0; a < 3; a++) {
		b.mn[a] = fminf(fminf(t.v0[a], t.v1[a]), t.v2[a]);
		b.mx[a] = fmaxf(fmaxf(t.v0[a], t.v1[a]), t.v2[a]);
	}
	b.cnt_flag = 1u;
	b.cost = bp.cost_tri * half_area(b.mn, b.mx);
	return b;
}

// Record of an inner node from the records of its two children: box union, triangle count and the SAH
// decision "one leaf of cnt triangles" vs "split" (cost model of rtk.c:931-949 with working constants,
// SURVEY.md appendix B9). min/max/+ are commutative, so the result does not depend on which child is a.
__device__ __forceinline__ BinNode combine_records(const BinNode &a, const BinNode &b, const BuildParams &bp)
{
	BinNode out;
#pragma unroll
	for (int k = 0; k < 3; k++) { out.mn[k] = fminf(a.mn[k], b.mn[k]); out.mx[k] = fmaxf(a.mx[k], b.mx[k]); }
	const uint32_t cnt = (a.cnt_flag & 0x7fffffffu) + (b.cnt_flag & 0x7fffffffu);
	const float cost = a.cost + b.cost;
	const float area = half_area(out.mn, out.mx);
	const float split = bp.cost_node * area + cost;
	// (the size limit is tested by itself: with an infinite or NaN area -- non-finite vertices -- "INFINITY <= split" would
	// be true and the whole scene one leaf)
	const bool may_be_leaf = cnt <= bp.max_leaf;
	const float leaf = may_be_leaf ? bp.cost_tri * (float)cnt * area : INFINITY;
	out.cnt_flag = cnt | ((may_be_leaf && leaf <= split) ? 0x80000000u : 0u);
	out.cost = fminf(leaf, split);
	return out;
}

#define REFIT_TILE 1024
#define REFIT_BLOCK 1024        // one thread per triangle: every global load of the tile is in flight at once

// ---- tile-local collapse (binary -> 4-wide) shared by the counting tail of k_refit_tile and by k_collapse_tile ----
// A binary node whose sorted range lies inside one tile (a node pass 1 finishes) is never opened INSIDE a wide node that
// lies above the tile: the maximal such subtrees ("tile roots") always become wide nodes of their own, so everything
// below them can be collapsed by the tile's workgroup alone, out of LDS, while the few nodes above (the ones pass 2
// finishes) go through the level-by-level collapse. Costs ~1 % more node visits than the unconstrained greedy collapse
// (scripts/bvh_lab.cpp -ft 1024) and replaces a dozen launches of dependent random reads over the whole tree.
//
// Chooses the (up to four) children of wide-node job b, a tile-contained binary node: its two children, then twice the
// largest-area child that is still an openable inner node -- the rule of collapse_open below, on LDS copies of the
// tile's child links and areas (lr_, area_ indexed by node - lo; open_area).
__device__ __forceinline__ int tile_open(int b, int lo, const int2 *lr_, const float *area_, int c[4])
{
	const int2 ch = lr_[b - lo];
	c[0] = ch.x; c[1] = ch.y; c[2] = 0; c[3] = 0;
	int nc = 2;
#pragma unroll
	for (int round = 0; round < 2; round++) {
		int best = -1;
		float best_area = 0.0f;
#pragma unroll
		for (int k = 0; k < 4; k++) {
			if (k >= nc || c[k] < 0) continue;
			const float a = area_[c[k] - lo];                              // <= 0: one leaf, not opened
			if (a > best_area) { best_area = a; best = k; }
		}
		if (best >= 0) {
			int bref = 0;
#pragma unroll
			for (int k = 0; k < 4; k++) if (k == best) bref = c[k];
			const int2 o = lr_[bref - lo];
#pragma unroll
			for (int k = 0; k < 4; k++) {
				if (k == best) c[k] = o.x;
				if (k == nc) c[k] = o.y;
			}
			nc++;
		}
	}
	return nc;
}

// what tile_open ranks openable children by: the half area of the node's box, never zero (a box flat on two axes must stay
// openable); negative for a subtree the SAH rule turned into one leaf
__device__ __forceinline__ float open_area(const BinNode &r)
{
	return (r.cnt_flag & 0x80000000u) ? -1.0f : fmaxf(half_area(r.mn, r.mx), 1e-37f);
}

// exclusive prefix sum of `v` over the threads of the workgroup (at most 1024; s_w: 16 words of LDS); *total = the sum
__device__ __forceinline__ uint32_t block_exclusive_scan_1024(uint32_t v, uint32_t *s_w, uint32_t *total)
{
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
	uint32_t inc = v;
	for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(inc, o); if (lane >= (uint32_t)o) inc += t; }
	__syncthreads();                                   // s_w may still be read from the previous use
	if (lane == 63u) s_w[wave] = inc;
	__syncthreads();
	uint32_t off = 0, tot = 0;
	for (uint32_t w = 0; w < waves; w++) { if (w < wave) off += s_w[w]; tot += s_w[w]; }
	*total = tot;
	return off + inc - v;
}

// Pass 1, tile-local. The sorted triangles are cut into tiles of REFIT_TILE; one 1024-thread workgroup owns a tile and
// builds every inner node whose two children lie inside it (split positions lo .. hi-1 with ranges inside [lo, hi]):
// similarities, child links, range ends, arrival counters and the 32-B node records of the tile live in LDS, so a climb
// waits for no global memory, and the hand-off between the two subtrees that meet at a node never leaves the CU (the
// all-global version of round 1 cost ~14 memory-side atomics per node, 3.8 ms at 10M triangles). Finished nodes are
// written out once, coalesced. A subtree whose parent lies across the tile border is left for pass 2 as a "climber":
// (subtree, L, R), stored at the leaf that carried it.

struct Climb { int cur_ref; int l; int r; };      // cur_ref: >= 0 inner node, < 0 leaf ~slot; INT_MIN: none

// meet[node]: 0 until the first of the node's two subtrees has arrived, then (its reference << 32 | the range end it brings) + 1
// (never 0: a range end is below 2^32 - 1). Which side it is the second arriver knows: the other one.
__device__ __forceinline__ unsigned long long meet_word(int ref, int end) { return (((unsigned long long)(uint32_t)ref << 32) | (uint32_t)end) + 1ull; }

// emit.src != NULL: the kernel first MAKES the tile's triangle records (what k_emit_tris does: positions gathered in sorted order) and
// writes them out; each thread keeps its own in registers for the leaf record. A separate pass wrote 48 bytes per triangle that this
// one read straight back, and its gather (bound by the CU's vector memory pipe) ran apart from this kernel's climb (bound by LDS round
// trips): side by side on a CU's two workgroups the two overlap.
__global__ void __launch_bounds__(REFIT_BLOCK) k_refit_tile(DevTri *tris, int n, const unsigned long long *keys, int2 *lr, uint2 *range,
	BinNode *bin, Climb *climbers, unsigned long long *meet, int *climb_idx, uint32_t *tile_nclimb, int *root, BuildParams bp, float *area,
	uint32_t *equal_codes, int *root_list, uint32_t *tile_nroots, EmitSrc emit)
{
	__shared__ uint32_t s_nclimb, s_nroot;
	__shared__ BinNode s_bin[REFIT_TILE];      // 32 KB
	__shared__ uint32_t s_arrive[REFIT_TILE];
	__shared__ int2 s_lr[REFIT_TILE];                            // children of node lo + k (x left, y right)
	__shared__ int s_rl[REFIT_TILE], s_rr[REFIT_TILE];          // its range
	__shared__ int s_delta[REFIT_TILE + 1];                     // [k] = similarity across the border between lo+k-1 and lo+k
	const int lo = (int)blockIdx.x * REFIT_TILE;
	const int hi = (lo + REFIT_TILE < n ? lo + REFIT_TILE : n) - 1;     // last sorted triangle of the tile
	const int t = (int)threadIdx.x;
	DevTri mine = {};
	if (emit.src) {
		const uint32_t s_own = (uint32_t)(lo + t);
		mine = make_tri(emit, s_own < (uint32_t)n ? s_own : (uint32_t)n - 1u);
		store_tris(tris, s_own, (uint32_t)n, mine);      // (visible to the other waves of the workgroup behind the barrier below: the climb reads sibling leaves)
	}
	s_arrive[t] = 0u;
	if (t == 0) { s_nclimb = 0u; s_nroot = 0u; }
	s_lr[t] = make_int2(INT_MIN, INT_MIN);
	int my_delta = -1;
	if (lo + t - 1 <= hi) s_delta[t] = my_delta = key_delta(keys, n, lo + t - 1);
	if (t == 0 && hi - lo + 1 == REFIT_TILE) s_delta[REFIT_TILE] = key_delta(keys, n, hi);
	{
		// how many neighbours in sorted order share their whole Morton code (a common prefix of 40 bits or more: the packed
		// words carry the code above a 24-bit index, equal pair keys count 64+): where that is common the key was too narrow for
		// the scene -- a dense mesh in a corner of the scene box -- and the host builds again with the full 40 bits
		const unsigned long long same = __ballot(t > 0 && my_delta >= 40);
		if ((t & 63) == 0 && same) atomicAdd(equal_codes, (uint32_t)__popcll(same));
	}
	__syncthreads();
	const int i = lo + t;
	Climb left_over;
	left_over.cur_ref = INT_MIN; left_over.l = left_over.r = 0;
	if (i <= hi) {
		BinNode cur = emit.src ? leaf_record_of(mine, bp) : leaf_record(tris, (uint32_t)i, bp);
		int cur_ref = ~i, L = i, R = i;
		for (;;) {
			if (L == 0 && R == n - 1) { *root = cur_ref; break; }          // the whole scene inside one tile
			const int dl = s_delta[L - lo], dr = s_delta[R - lo + 1];
			const bool go_right = L == 0 || (R != n - 1 && dr > dl);        // (never equal for the borders of a real subtree)
			const int parent = go_right ? R : L - 1;
			if (parent < lo || parent >= hi) {                               // its other child lies in a neighbouring tile
				left_over.cur_ref = cur_ref; left_over.l = L; left_over.r = R;
				break;
			}
			const int k = parent - lo;
			if (go_right) { s_lr[k].x = cur_ref; s_rl[k] = L; } else { s_lr[k].y = cur_ref; s_rr[k] = R; }
			// (cur, if it is an inner node, sits in s_bin[cur_ref - lo] already: LDS is in order, the arrival below publishes it)
			const uint32_t old = __hip_atomic_fetch_add(&s_arrive[k], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
			if (old == 0u) break;                                            // first arriver: the sibling's thread carries on
			const int sib = go_right ? s_lr[k].y : s_lr[k].x;
			if (go_right) R = s_rr[k]; else L = s_rl[k];
			const BinNode other = sib < 0 ? leaf_record(tris, (uint32_t)~sib, bp) : s_bin[sib - lo];
			cur = combine_records(cur, other, bp);
			cur_ref = parent;
			s_bin[k] = cur;
		}
		// a climber is stored at the leaf that carried it, and where pass 2 and the tile collapse find the tile's climbers without
		// looking at every triangle: their positions, packed at the start of the tile's stretch of climb_idx (any order: the tree
		// does not depend on who climbs first). (Round 4 wrote all 1024 records of a tile, 12 bytes per triangle, and both
		// collapse kernels read them all back to find the two dozen that are there.)
		if (left_over.cur_ref != INT_MIN) {
			climbers[i] = left_over; climb_idx[lo + (int)atomicAdd(&s_nclimb, 1u)] = i;
			// tile mode: the subtree it carried to the border is one of the tile's roots (below), unless it is one leaf
			if (root_list && left_over.cur_ref >= 0 && open_area(cur) > 0.0f) root_list[lo + (int)atomicAdd(&s_nroot, 1u)] = left_over.cur_ref;
		}
	}
	__syncthreads();
	if (t == 0) tile_nclimb[blockIdx.x] = s_nclimb;
	// the finished records, 16 bytes per thread and store in the order they lie in LDS and in memory (a 32-byte record per
	// thread is two stores of half lines at a stride of 32)
	static_assert(sizeof(BinNode) == 32 && REFIT_BLOCK == REFIT_TILE, "two 16-byte pieces per record, one record per thread");
#pragma unroll
	for (int m = t; m < 2 * REFIT_TILE; m += REFIT_BLOCK) {
		const int rec = m >> 1;
		if (lo + rec < hi && s_arrive[rec] == 2u) reinterpret_cast<uint4 *>(bin + lo)[m] = reinterpret_cast<const uint4 *>(s_bin)[m];
	}
	// The tile's ROOTS (tile mode): the largest subtrees that lie inside the tile -- what its climbers carried to the border
	// (above) and the half that is here of a node whose other child arrives in pass 2 -- are all known now. The tile-local
	// collapse (k_count_tile, k_collapse_tile) reads this list and the records of the nodes that are complete here, nothing
	// that pass 2 writes: it runs beside pass 2 and the collapse of the nodes above the tiles. area < 0: not a node to open
	// (one leaf: open_area; not complete in this pass: -1).
	unsigned long long meet_here = 0ull;
	if (i < hi && s_arrive[t] == 2u) {
		if (area) area[i] = open_area(s_bin[t]);      // what the tile-local collapse ranks children by (4 bytes instead of the 32-byte record)
		lr[i] = s_lr[t];
		range[i] = make_uint2((uint32_t)s_rl[t], (uint32_t)s_rr[t]);
	} else if (i < hi) {
		if (area) area[i] = -1.0f;
		if (s_arrive[t] == 1u) {
			// one child came, the other one's subtree reaches into a neighbouring tile and arrives in pass 2: hand the half that
			// is here over in the form pass 2 uses (plain stores, the kernel boundary publishes them)
			const bool left_here = s_lr[t].x != INT_MIN;
			const int ref = left_here ? s_lr[t].x : s_lr[t].y, end = left_here ? s_rl[t] : s_rr[t];
			meet_here = meet_word(ref, end);
			if (root_list && ref >= 0 && open_area(s_bin[ref - lo]) > 0.0f) root_list[lo + (int)atomicAdd(&s_nroot, 1u)] = ref;
		}
	}
	// (every word of the tile's stretch is written: 0 = nobody has arrived at this node yet -- a memset of the whole array before
	// the kernel was 13 us at 10M triangles)
	if (i <= hi) meet[i] = meet_here;
	__syncthreads();
	if (t == 0 && tile_nroots) tile_nroots[blockIdx.x] = s_nroot;
}

// exclusive prefix sums of the tiles' wide-node counts (one workgroup; a build has at most n / 1024 tiles); out[num] = total
__global__ void __launch_bounds__(1024) k_scan_tiles(const uint32_t *count, uint32_t num, uint32_t *base)
{
	__shared__ uint32_t s_w[16];
	uint32_t carry = 0;
	for (uint32_t at = 0; at < num; at += 1024u) {
		const uint32_t i = at + threadIdx.x;
		const uint32_t v = i < num ? count[i] : 0u;
		uint32_t total = 0;
		const uint32_t ex = block_exclusive_scan_1024(v, s_w, &total);
		if (i < num) base[i] = carry + ex;
		carry += total;
	}
	if (threadIdx.x == 0) base[num] = carry;
}

// Pass 2: the few nodes whose children lie in different tiles (about two per tile plus chains). The hand-off of the
// first arriver's half -- its child reference, its range end and its 32-byte record -- has to cross CUs and XCDs here
// (per-CU L1 and per-XCD L2 are not coherent with each other): everything travels as 8-byte device-scope atomics, which
// execute at the memory side and are therefore coherent everywhere, and the arrival counter stays relaxed. Records
// written by pass 1 are plain stores made visible by the kernel boundary.
__device__ __forceinline__ void bin_store(BinNode *dst, const BinNode &v)
{
	unsigned long long *d = reinterpret_cast<unsigned long long *>(dst);
	const unsigned long long *sv = reinterpret_cast<const unsigned long long *>(&v);
#pragma unroll
	for (int k = 0; k < 4; k++) (void)__hip_atomic_exchange(d + k, sv[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// a real read-modify-write (hipcc folds fetch_add(p, 0) into an sc1 load): compare-and-swap of a value with itself
// returns the memory-side copy and never changes it
__device__ __forceinline__ unsigned long long mem_load64(unsigned long long *p)
{
	unsigned long long expect = ~0ull;
	(void)__hip_atomic_compare_exchange_strong(p, &expect, ~0ull, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	return expect;
}

__device__ __forceinline__ BinNode bin_load(BinNode *src)
{
	BinNode v;
	unsigned long long *d = reinterpret_cast<unsigned long long *>(src);
	unsigned long long *dv = reinterpret_cast<unsigned long long *>(&v);
#pragma unroll
	for (int k = 0; k < 4; k++) dv[k] = mem_load64(d + k);
	return v;
}

// One 64-wide workgroup per tile takes the tile's climbers (a few to a few dozen; climb_idx / tile_nclimb from pass 1) -- the
// launch used to cover every triangle to find them. Two subtrees meet at a node through ONE compare-and-swap on meet[node]:
// the first arriver swaps its (reference, range end) in and is done, the second gets the first one's word back (round 2: an
// exchange, a wait, a counter increment and a load -- three memory-side round trips per level of a chain that is ~20 levels deep).
// never_leaf (tile mode): a node finished here -- one that reaches across a tile border -- is never ONE leaf. Its finished
// children are the roots that k_collapse_tile turns into wide nodes (k_refit_tile counted them before this pass knew the
// node's cost), so the node above them must stay a node: a leaf of two or three triangles straddling a border would
// otherwise swallow a subtree that already has a number. (One such node at 17M triangles; found by the validator.)
__global__ void __launch_bounds__(64) k_refit_top(const DevTri *tris, int n, const unsigned long long *keys, const Climb *climbers, const int *climb_idx,
	const uint32_t *tile_nclimb, unsigned long long *meet, BinNode *bin, int2 *lr, uint2 *range, int *root, BuildParams bp, bool never_leaf)
{
	const int lo = (int)blockIdx.x * REFIT_TILE;
	const uint32_t count = tile_nclimb[blockIdx.x];
	for (uint32_t j = threadIdx.x; j < count; j += blockDim.x) {
		const Climb c = climbers[climb_idx[lo + (int)j]];
		int cur_ref = c.cur_ref, L = c.l, R = c.r;
		BinNode cur = cur_ref < 0 ? leaf_record(tris, (uint32_t)~cur_ref, bp) : bin[cur_ref];      // finished by pass 1: plain load
		for (;;) {
			if (L == 0 && R == n - 1) { *root = cur_ref; break; }
			const int dl = key_delta(keys, n, L - 1), dr = key_delta(keys, n, R);
			const bool go_right = L == 0 || (R != n - 1 && dr > dl);
			const int parent = go_right ? R : L - 1;
			// (an inner node finished in THIS pass has its record at the memory side already: bin_store and the wait below)
			unsigned long long seen = 0ull;
			(void)__hip_atomic_compare_exchange_strong(meet + parent, &seen, meet_word(cur_ref, go_right ? L : R), __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			if (seen == 0ull) break;                                           // first arriver: the sibling's thread carries on
			const unsigned long long theirs = seen - 1ull;
			const int sib = (int)(uint32_t)(theirs >> 32);
			if (go_right) R = (int)(uint32_t)theirs; else L = (int)(uint32_t)theirs;
			const BinNode other = sib < 0 ? leaf_record(tris, (uint32_t)~sib, bp) : bin_load(&bin[sib]);
			cur = combine_records(cur, other, bp);
			if (never_leaf) cur.cnt_flag &= 0x7fffffffu;
			bin_store(&bin[parent], cur);
			// topology of the finished node: read by the collapse only (later launches), plain stores
			lr[parent] = go_right ? make_int2(cur_ref, sib) : make_int2(sib, cur_ref);
			range[parent] = make_uint2((uint32_t)L, (uint32_t)R);
			cur_ref = parent;
			// everything this thread published is complete at the memory side before it announces the node one level up
			asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
		}
	}
}

// ---------------------------------------------------------------------------------- 8 collapse
// Binary tree -> 128 B 4-wide nodes, breadth first. A job is one wide node = one binary node that gets opened:
// its two children, then twice more the largest-area child that is still an inner node (the reference collapses
// exactly two binary levels, rtk.c:1572-1592; the greedy rule costs 2 % fewer node visits on the benchmark
// scene). Wide-node numbers come from prefix sums, not from an atomic counter, so the node array is the same for
// every build of the same input. A node is written in two steps, each in whole 32-B sectors:
//   k_collapse_open    one thread per job of a level: reads the binary records (the dependent-load chain, so it gets
//                      all the parallelism there is), writes the node's boxes (96 B), marks its leaves in the triangle
//                      array, and leaves behind what depends on a prefix sum: the four child words with binary
//                      references in the slots of inner children (dec), which slots those are (info), and per 256
//                      jobs their number
//   k_collapse_number  per job: prefix sum of the inner children -> their node numbers; writes the child words
//                      (32 B) and the next level's job list. A block adds up the block sums before it by itself.
//   k_collapse_small   levels of at most 1024 jobs -- the top six and the last few -- both steps in ONE workgroup,
//                      several levels per launch (also opens the root)
// Level bookkeeping lives in device memory: launch number `step` reads ring entry step and writes entry step+1,
// so nothing a running kernel reads is written by it. The host reads the ring once per round.
#define COLLAPSE_BLOCK 256
#define COLLAPSE_SMALL 1024          // threads of k_collapse_small = children it opens per round
#define COLLAPSE_SMALL_JOBS 64      // largest level it takes: its children (at most four each) are one round
#define COLLAPSE_RING 64

struct LevelState {
	uint32_t count;           // jobs of this level
	uint32_t base;            // wide-node index of its first job
	uint32_t level;
	uint32_t total_nodes;
	uint32_t depth;
	uint32_t pad[3];
};

// What the host needs to know of a build, in pinned host memory: the kernels write it there and the host reads it after the wait for
// the stream it needs anyway. (Five copies into pageable host memory -- level state, node total, depth, equal codes, scene constants --
// cost the host ~20 us each, one after the other, at the end of every build.)
struct BuildResults {
	LevelState level;          // k_collapse_small: the level the round ended at
	uint32_t tiles_total, depth, equal_codes, pad;
	DevSceneConsts consts;
};

__global__ void k_publish(BuildResults *out, const uint32_t *tiles_total, const uint32_t *depth_word, const DevSceneConsts *consts)
{
	out->tiles_total = tiles_total ? *tiles_total : 0u;
	out->depth = depth_word[0];
	out->equal_codes = depth_word[1];
	out->consts = *consts;
}

struct CollapseBufs {
	int *jobs;                // [job] binary node of the job (current level; LDS inside k_collapse_small)
	int4 *dec;                // [job] child words, binary references where info says so
	uint32_t *info;           // [job] inner-children mask << 4 | their number << 8
	uint32_t *sums;           // [job / 256] inner children of those 256 jobs
};

struct Cand {
	int ref;          // binary child: >= 0 inner, < 0 leaf ~slot
	float area;       // > 0 only if the child may still be opened
	float mn[3], mx[3];
	bool tile_job;    // tile mode: an inner node inside one refit tile -- a wide node that k_collapse_tile makes, not opened here
};

// The subtree is left alone by the level-by-level collapse if it lies inside one refit tile (tile mode).
__device__ __forceinline__ bool in_one_tile(const uint2 rg) { return rg.x / REFIT_TILE == rg.y / REFIT_TILE; }

__device__ __forceinline__ Cand make_cand(int ref, const BinNode *bin, const DevTri *tris, const uint2 *range, bool tile_mode)
{
	Cand c;
	c.ref = ref;
	c.area = -1.0f;
	c.tile_job = false;
	if (ref >= 0) {
		const BinNode b = bin[ref];
		c.mn[0] = b.mn[0]; c.mn[1] = b.mn[1]; c.mn[2] = b.mn[2];
		c.mx[0] = b.mx[0]; c.mx[1] = b.mx[1]; c.mx[2] = b.mx[2];
		// An inner node that is not one leaf can always be opened; the area only ranks the candidates. It can be ZERO
		// (a box flat on two axes: triangles in a row, or extents that underflow) -- taking "area > 0" for "may be opened"
		// turned such subtrees into single leaves of any size, which the 6-bit leaf count of the blob cannot even hold.
		if (!(b.cnt_flag & 0x80000000u)) {
			if (tile_mode && in_one_tile(range[ref])) c.tile_job = true;
			else c.area = fmaxf(half_area(b.mn, b.mx), 1e-37f);
		}
	} else tri_box(tris, (uint32_t)~ref, c.mn, c.mx);
	return c;
}

// a subtree the SAH rule turned into one leaf of the sorted triangles [rg.x, rg.y]: the count goes into its first record,
// and only the last one keeps the end mark (every record starts out as a leaf of its own, k_emit_tris)
__device__ __forceinline__ void mark_leaf(DevTri *tris, const uint2 rg)
{
	tris[rg.x].spare = rg.y - rg.x + 1u;
	for (uint32_t t = rg.x; t < rg.y; t++) { tris[t].flags &= ~RTK_TRI_LAST; tris[t + 1u].spare = 0u; }
}

// Opens binary node b as wide node `node_index`: chooses its (up to four) children and writes the node except for the
// numbers of the children that are wide nodes themselves. Returns how many those are.
// aux.tile_refs != NULL: tile mode -- the nodes ABOVE the refit tiles, written to a stretch of the workspace with numbers of
// their own (k_top_finish moves them behind the tiles' nodes, which k_collapse_tile makes at the same time on another stream).
// Children that are tile jobs keep an empty child word; WHICH binary node hangs in the slot goes to aux.tile_refs[node]
// (+ 1; 0: not a tile job) and the node's level to aux.level[node], for k_top_finish.
struct TopAux { uint4 *tile_refs; uint32_t *level; };
__device__ __forceinline__ uint32_t collapse_open(int b, uint32_t node_index, const int2 *lr, const uint2 *range, const BinNode *bin,
	DevTri *tris, DevNode *nodes, uint32_t node_cap, int4 &dec, uint32_t &info, TopAux aux = TopAux{ nullptr, nullptr }, uint32_t level = 0)
{
	const bool tile_mode = aux.tile_refs != nullptr;
	uint32_t tref[4] = { 0u, 0u, 0u, 0u };
	Cand c[4];
	int nc;
	const BinNode self = bin[b];
	if (self.cnt_flag & 0x80000000u) {
		// the whole (sub)tree is one leaf: only the root of a tiny scene
		c[0].ref = b; c[0].area = -1.0f;
		c[0].mn[0] = self.mn[0]; c[0].mn[1] = self.mn[1]; c[0].mn[2] = self.mn[2];
		c[0].mx[0] = self.mx[0]; c[0].mx[1] = self.mx[1]; c[0].mx[2] = self.mx[2];
		c[0].tile_job = false;
		nc = 1;
	} else {
		const int2 ch = lr[b];
		c[0] = make_cand(ch.x, bin, tris, range, tile_mode);
		c[1] = make_cand(ch.y, bin, tris, range, tile_mode);
		nc = 2;
		// (every index into c[] below is a compile-time constant after unrolling: a run-time index would put the 32-dword
		// array into scratch memory, which made this function several times slower)
#pragma unroll
		for (int round = 0; round < 2; round++) {
			int best = -1, best_ref = 0;
			float best_area = 0.0f;
#pragma unroll
			for (int k = 0; k < 4; k++) if (k < nc && c[k].area > best_area) { best_area = c[k].area; best = k; best_ref = c[k].ref; }
			if (best >= 0) {
				const int2 o = lr[best_ref];
				const Cand left = make_cand(o.x, bin, tris, range, tile_mode), right = make_cand(o.y, bin, tris, range, tile_mode);
#pragma unroll
				for (int k = 0; k < 4; k++) {
					if (k == best) c[k] = left;
					if (k == nc) c[k] = right;
				}
				nc++;
			}
		}
	}
	uint32_t mask = 0, n_inner = 0;
	int r[4] = { 0, 0, 0, 0 };
	float4 rows[6];      // bx[0], bx[1], by[0], by[1], bz[0], bz[1]: the first 96 bytes of the node
	float *out = reinterpret_cast<float *>(rows);
#pragma unroll
	for (int k = 0; k < 4; k++) {
		if (k >= nc) {
			out[0 + k] = out[8 + k] = out[16 + k] = +1.0f;        // inverted = never hit (rtk.c:1612-1620)
			out[4 + k] = out[12 + k] = out[20 + k] = -1.0f;
			continue;
		}
		const int ref = c[k].ref;
		if (ref < 0) {
			// a leaf of one triangle: k_emit_tris wrote every record as exactly that (count 1, last-of-leaf set), so
			// there is nothing to mark -- two 4-byte read-modify-writes per leaf here were the bulk of this kernel's time
			r[k] = (int)(RTK_REF_LEAF | (uint32_t)~ref);
		} else if (c[k].area > 0.0f) {
			mask |= 1u << k;
			n_inner++;
			r[k] = ref;                                           // binary reference; becomes a node number when this level is numbered
		} else if (c[k].tile_job) {
			r[k] = (int)RTK_REF_NONE;                             // k_top_finish writes the number of the wide node k_collapse_tile makes of it
#pragma unroll
			for (int q = 0; q < 4; q++) if (q == k) tref[q] = (uint32_t)ref + 1u;
		} else {
			const uint2 rg = range[ref];
			mark_leaf(tris, rg);
			r[k] = (int)(RTK_REF_LEAF | rg.x);
		}
		out[0 + k] = c[k].mn[0]; out[4 + k] = c[k].mx[0];
		out[8 + k] = c[k].mn[1]; out[12 + k] = c[k].mx[1];
		out[16 + k] = c[k].mn[2]; out[20 + k] = c[k].mx[2];
	}
	// the boxes now (96 B = three whole 32-B sectors); the child words follow in ONE 32-B store when this node's level
	// is numbered -- patching single words of a node written earlier made every patch a read-modify-write in memory
	// (node_cap: the collapse writes straight into the scene's node array, sized from an estimate; should a tree have more
	// nodes than that, the writes beyond it are dropped and the host repeats the collapse into the workspace)
	if (node_index < node_cap) {
		float4 *dst = reinterpret_cast<float4 *>(nodes + node_index);
#pragma unroll
		for (int q = 0; q < 6; q++) dst[q] = rows[q];
		if (tile_mode) {
			aux.tile_refs[node_index] = make_uint4(tref[0], tref[1], tref[2], tref[3]);
			aux.level[node_index] = level;
		}
	}
	for (int k = nc; k < 4; k++) r[k] = (int)RTK_REF_NONE;
	dec = make_int4(r[0], r[1], r[2], r[3]);                      // final child words, except the slots in `mask`: binary references
	info = (mask << 4) | (n_inner << 8);
	return n_inner;
}

// Job `node_index`: its inner children get the numbers next_base + off, ...; the child words go out as one sector and
// the children's binary references to next_jobs[off ...].
__device__ __forceinline__ void collapse_number_children(uint32_t node_index, uint32_t next_base, uint32_t off, const int4 d,
	uint32_t inf, DevNode *nodes, uint32_t node_cap, int *next_jobs)
{
	uint32_t ref[4] = { (uint32_t)d.x, (uint32_t)d.y, (uint32_t)d.z, (uint32_t)d.w };
	const uint32_t mask = (inf >> 4) & 15u;
#pragma unroll
	for (int k = 0; k < 4; k++) {
		if (!(mask & (1u << k))) continue;
		next_jobs[off] = (int)ref[k];
		ref[k] = next_base + off;
		off++;
	}
	// child[4] and pad[4]: the last 32 bytes of the node, one sector
	if (node_index >= node_cap) return;
	uint4 *dst = reinterpret_cast<uint4 *>(&nodes[node_index].child[0]);
	dst[0] = make_uint4(ref[0], ref[1], ref[2], ref[3]);
	dst[1] = make_uint4(0u, 0u, 0u, 0u);
}

__device__ __forceinline__ LevelState next_level(const LevelState &L, uint32_t next_count)
{
	LevelState N = L;
	N.count = next_count;
	N.base = L.base + L.count;
	N.level = L.level + 1u;
	if (L.count) { N.total_nodes = L.base + L.count; N.depth = L.level + 1u; }
	return N;
}

__global__ void __launch_bounds__(COLLAPSE_BLOCK) k_collapse_open(CollapseBufs B, const LevelState *ring, uint32_t step, const int2 *lr, const uint2 *range,
	const BinNode *bin, DevTri *tris, DevNode *nodes, uint32_t node_cap, TopAux aux)
{
	__shared__ uint32_t s_w[COLLAPSE_BLOCK / 64];
	const LevelState L = ring[step % COLLAPSE_RING];
	const uint32_t count = L.count;
	for (uint32_t vb = blockIdx.x; vb * COLLAPSE_BLOCK < count; vb += gridDim.x) {
		const uint32_t j = vb * COLLAPSE_BLOCK + threadIdx.x;
		uint32_t n_inner = 0;
		if (j < count) {
			int4 d;
			uint32_t inf;
			n_inner = collapse_open(B.jobs[j], L.base + j, lr, range, bin, tris, nodes, node_cap, d, inf, aux, L.level);
			B.dec[j] = d;
			B.info[j] = inf;
		}
		uint32_t sum = n_inner;
		for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
		if ((threadIdx.x & 63u) == 0u) s_w[threadIdx.x >> 6] = sum;
		__syncthreads();
		if (threadIdx.x == 0) {
			uint32_t t = 0;
			for (int w = 0; w < COLLAPSE_BLOCK / 64; w++) t += s_w[w];
			B.sums[vb] = t;
		}
		__syncthreads();
	}
}

// Sum of a[lo..hi) for the whole workgroup (COLLAPSE_BLOCK threads).
__device__ __forceinline__ uint32_t block_range_sum(const uint32_t *a, uint32_t lo, uint32_t hi, uint32_t *s_w)
{
	uint32_t t = 0;
	for (uint32_t i = lo + threadIdx.x; i < hi; i += COLLAPSE_BLOCK) t += a[i];
	for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
	__syncthreads();                                    // s_w may still be read from the previous use
	if ((threadIdx.x & 63u) == 0u) s_w[threadIdx.x >> 6] = t;
	__syncthreads();
	uint32_t r = 0;
	for (int w = 0; w < COLLAPSE_BLOCK / 64; w++) r += s_w[w];
	return r;
}

__global__ void __launch_bounds__(COLLAPSE_BLOCK) k_collapse_number(CollapseBufs B, LevelState *ring, uint32_t step, DevNode *nodes, uint32_t node_cap)
{
	__shared__ uint32_t s_w[COLLAPSE_BLOCK / 64];
	__shared__ uint32_t s_r[COLLAPSE_BLOCK / 64];
	const LevelState L = ring[step % COLLAPSE_RING];
	const uint32_t count = L.count, base = L.base, next_base = base + count;
	const uint32_t nb = (count + COLLAPSE_BLOCK - 1u) / COLLAPSE_BLOCK;
	// inner children of the jobs before this workgroup's first block of 256
	uint32_t before = block_range_sum(B.sums, 0u, blockIdx.x < nb ? blockIdx.x : nb, s_r);
	for (uint32_t vb = blockIdx.x; vb * COLLAPSE_BLOCK < count; vb += gridDim.x) {
		const uint32_t j = vb * COLLAPSE_BLOCK + threadIdx.x;
		const uint32_t inf = j < count ? B.info[j] : 0u;
		const int4 d = j < count ? B.dec[j] : make_int4(0, 0, 0, 0);
		const uint32_t n_inner = inf >> 8;
		const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
		uint32_t inc = n_inner;
		for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(inc, o); if (lane >= (uint32_t)o) inc += t; }
		if (lane == 63u) s_w[wave] = inc;
		__syncthreads();
		uint32_t off = before;
		for (uint32_t w = 0; w < wave; w++) off += s_w[w];
		off += inc - n_inner;
		__syncthreads();
		// (the job list is written over the one this level was opened from: nothing reads that any more)
		if (j < count) collapse_number_children(base + j, next_base, off, d, inf, nodes, node_cap, B.jobs);
		const uint32_t hi = vb + gridDim.x < nb ? vb + gridDim.x : nb;
		before += block_range_sum(B.sums, vb, hi, s_r);
	}
	// workgroup 0 has walked over every block sum: `before` is the size of the next level
	if (blockIdx.x == 0 && threadIdx.x == 0) ring[(step + 1u) % COLLAPSE_RING] = next_level(L, before);
}

// Up to max_levels levels, as long as a level has at most COLLAPSE_SMALL jobs; one workgroup. It takes over a level
// that is already opened (dec/info valid) and hands over one that is opened too, block sums included. Launch 0 of a
// build opens the root first.
__global__ void __launch_bounds__(COLLAPSE_SMALL) k_collapse_small(CollapseBufs B, LevelState *ring, uint32_t step, uint32_t max_levels,
	const int2 *lr, const uint2 *range, const BinNode *bin, DevTri *tris, DevNode *nodes, uint32_t node_cap, const int *root, TopAux aux, LevelState *host_out)
{
	__shared__ uint32_t s_w[COLLAPSE_SMALL / 64];
	__shared__ int s_ref[COLLAPSE_SMALL * 4];
	__shared__ uint32_t s_sums[COLLAPSE_SMALL * 4 / COLLAPSE_BLOCK];
	LevelState L;
	if (step == 0u) {
		// level 0 is the root job (the binary node the refit pass ended at), wide node 0
		L.count = 1u; L.base = 0u; L.level = 0u; L.total_nodes = 0u; L.depth = 0u; L.pad[0] = L.pad[1] = L.pad[2] = 0u;
		if (threadIdx.x == 0) {
			int4 d;
			uint32_t inf;
			B.sums[0] = collapse_open(*root, 0u, lr, range, bin, tris, nodes, node_cap, d, inf, aux, 0u);
			B.dec[0] = d;
			B.info[0] = inf;
		}
		__syncthreads();           // (workgroup scope is all that is needed: one workgroup, and the kernel boundary does the rest)
	} else L = ring[step % COLLAPSE_RING];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	for (uint32_t it = 0; it < max_levels && L.count != 0u && L.count <= COLLAPSE_SMALL_JOBS; it++) {
		// number this level's jobs ...
		const uint32_t j = threadIdx.x;
		const uint32_t inf = j < L.count ? B.info[j] : 0u;
		const int4 d = j < L.count ? B.dec[j] : make_int4(0, 0, 0, 0);
		const uint32_t n_inner = inf >> 8;
		uint32_t inc = n_inner;
		for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(inc, o); if (lane >= (uint32_t)o) inc += t; }
		if (lane == 63u) s_w[wave] = inc;
		if (threadIdx.x < COLLAPSE_SMALL * 4 / COLLAPSE_BLOCK) s_sums[threadIdx.x] = 0u;
		__syncthreads();
		uint32_t off = 0, total = 0;
		for (uint32_t w = 0; w < COLLAPSE_SMALL / 64; w++) { if (w < wave) off += s_w[w]; total += s_w[w]; }
		off += inc - n_inner;
		if (j < L.count) collapse_number_children(L.base + j, L.base + L.count, off, d, inf, nodes, node_cap, s_ref);
		const LevelState N = next_level(L, total);
		__syncthreads();
		// ... and open the next level's (every dec/info of this level is in registers by now)
		for (uint32_t i = threadIdx.x; i < total; i += COLLAPSE_SMALL) {
			int4 d2;
			uint32_t inf2;
			const uint32_t n2 = collapse_open(s_ref[i], N.base + i, lr, range, bin, tris, nodes, node_cap, d2, inf2, aux, N.level);
			B.dec[i] = d2;
			B.info[i] = inf2;
			if (n2) atomicAdd(&s_sums[i / COLLAPSE_BLOCK], n2);
		}
		__syncthreads();
		if (threadIdx.x < (total + COLLAPSE_BLOCK - 1u) / COLLAPSE_BLOCK) B.sums[threadIdx.x] = s_sums[threadIdx.x];
		L = N;
		// dec/info/sums of the next level are read by other threads of THIS workgroup (the barrier's workgroup-scope fence
		// covers that) or by the next launch (the kernel boundary does). A device-scope __threadfence() here wrote back and
		// invalidated the L2 at every level: ~25 us per level, a fifth of a 1M-triangle build.
		__syncthreads();
	}
	if (threadIdx.x == 0) {
		ring[(step + 1u) % COLLAPSE_RING] = L;
		if (host_out) *host_out = L;              // (pinned host memory: the last launch of a round)
	}
}

// The tile-local collapse: a SMALL workgroup per refit tile turns the tile's forest of finished binary subtrees into
// 4-wide nodes, out of LDS. Small on purpose: what a tile needs is a dozen rounds of a few dependent LDS reads each (which
// binary nodes become wide nodes is marked top-down from the tile roots, one level per round) -- latency, not throughput --
// so the chip is filled with many tiles at once (21 KB of LDS and one wave each: seven or more per CU) rather than with
// many threads per tile (a 1024-thread workgroup per tile left 90 % of its lanes waiting at barriers: 1.5 ms at 10M
// triangles; the level-by-level collapse over the whole tree, which this replaces, took 1.05 + 0.29 ms).
//   k_count_tile     marks, and counts the tile's wide nodes; a prefix sum over the counts (k_scan_tiles) gives every tile
//                    the number of its first node
//   k_collapse_tile  marks again (same code, same result), numbers the tile's wide nodes in pre-order and writes each of
//                    them ONCE and complete: boxes (the records pass 1 wrote), final child numbers, front-to-back order
//                    words and the 64-byte compressed copy (k_quantize would re-read what was just written). Dense: thread
//                    j makes node j of the tile. The roots of the forest are children of nodes the level-by-level collapse
//                    made before: their numbers are written into those nodes' child words.
#define TILE_THREADS 256       // k_collapse_tile: the first wave marks and numbers, all four finish nodes (k_count_tile: one wave)

// loads the tile's child links and areas into LDS and its roots (root_list / nroots: k_refit_tile listed them -- the subtrees
// its climbers carried to the tile's borders and the halves that are in the tile of nodes that reach beyond it; their order does
// not matter: numbers come from the tree alone. Inner nodes with disjoint ranges: at most REFIT_TILE / 2 of them). Nothing
// pass 2 writes is used: the area of a node that pass 1 did not complete is -1, and no root's subtree leads to one.
// (THREADS = the workgroup's size. All of a thread's global loads are issued before the first one is used -- left as a loop the
// compiler waits for each position's loads before it asks for the next: 16 dependent memory round trips per thread in the
// 64-thread counting kernel, 22 us of a tile's 118 in k_collapse_tile.)
template <int THREADS>
__device__ __forceinline__ void tile_load(int lo, int hi, const int2 *lr, const uint2 *range, const float *area, const int *root_list, uint32_t nroots,
	int2 *s_lr, float *s_area, uint16_t *s_start, int *s_roots, uint32_t *s_nroots)
{
	constexpr int ITER = REFIT_TILE / THREADS;
	const int t = (int)threadIdx.x;
	if (t == 0) *s_nroots = nroots;
	int2 v_lr[ITER];
	uint2 v_rg[ITER];
	float v_a[ITER];
#pragma unroll
	for (int q = 0; q < ITER; q++) {
		const int i = lo + t + q * THREADS;
		const int ic = i < hi ? i : (hi > lo ? hi - 1 : lo);       // (a position that exists: the values of positions beyond the tile are not used)
		v_lr[q] = lr[ic]; v_a[q] = area[ic];
		v_rg[q] = s_start ? range[ic] : make_uint2(0u, 0u);
	}
	for (uint32_t j = (uint32_t)t; j < nroots; j += THREADS) s_roots[j] = root_list[lo + (int)j];
#pragma unroll
	for (int q = 0; q < ITER; q++) {
		const int k = t + q * THREADS, i = lo + k;
		// (entries of nodes that are not complete inside the tile are never followed; their ranges may be anything)
		if (i < hi) { s_lr[k] = v_lr[q]; s_area[k] = v_a[q]; }
		else { s_lr[k] = make_int2(INT_MIN, INT_MIN); s_area[k] = -1.0f; }
		if (s_start) s_start[k] = (uint16_t)((i < hi && (int)v_rg[q].x >= lo && (int)v_rg[q].x <= hi) ? (int)v_rg[q].x - lo : 0);
	}
	__syncthreads();
}

// Which binary nodes of the tile become wide nodes ("jobs"): breadth-first from the tile roots, by ONE wave (the first of the
// workgroup; the others wait at the caller's barrier) -- a level is a handful to a few hundred jobs, each a chain of four
// dependent LDS reads, so what counts is not to touch anything but the jobs: s_q[0 .. count) lists them level by level
// (node - lo), appended with the wave's own prefix sums (ballots), no barriers, no scan over the tile's 1024 positions per
// level (that form of this loop took 100 us per tile). Returns count.
//   s_spine / s_lvl / s_cnt may be NULL (counting only). s_spine[k]: how many jobs above node lo + k share its range start;
//   s_cnt (packed 16-bit counters): jobs per range start; with these two the caller numbers the jobs in the PRE-ORDER of
//   the forest (range start ascending, larger range first): every node after its parent, subtrees contiguous, numbers that
//   depend on the tree alone. s_lvl[k]: level of the node below its tile root (the root: 0); s_rootof[k]: which root that is
//   (its place in s_roots); s_rdepth[r]: the deepest level below root r -- where a root hangs in the tree is not known
//   here (the nodes above the tiles are collapsed at the same time, on another stream): k_top_finish adds the two.
__device__ __forceinline__ uint32_t tile_bfs(int lo, const int2 *s_lr, const float *s_area, const uint16_t *s_start, const int *s_roots, uint32_t nroots,
	uint16_t *s_q, uint16_t *s_spine, uint8_t *s_lvl, uint32_t *s_cnt, uint16_t *s_rootof, uint32_t *s_rdepth)
{
	const uint32_t lane = threadIdx.x & 63u;
	for (uint32_t r = lane; r < nroots; r += 64u) {
		const int k = s_roots[r] - lo;
		s_q[r] = (uint16_t)k;
		if (s_spine) {
			s_spine[k] = 0u;
			s_lvl[k] = 0u;
			s_rootof[k] = (uint16_t)r;
			s_rdepth[r] = 0u;
			atomicAdd(s_cnt + ((uint32_t)s_start[k] >> 1), (s_start[k] & 1u) ? 0x10000u : 1u);
		}
	}
	uint32_t begin = 0, end = nroots, tail = nroots;
	while (begin < end) {
		for (uint32_t j0 = begin; j0 < end; j0 += 64u) {
			const uint32_t j = j0 + lane;
			int c[4] = { -1, -1, -1, -1 };
			int nc = 0, t = 0;
			if (j < end) { t = (int)s_q[j]; nc = tile_open(lo + t, lo, s_lr, s_area, c); }
#pragma unroll
			for (int k = 0; k < 4; k++) {
				const bool inner = k < nc && c[k] >= 0 && s_area[c[k] - lo] > 0.0f;
				const unsigned long long m = __builtin_amdgcn_ballot_w64(inner);
				if (inner) {
					const uint32_t pos = tail + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
					const int ck = c[k] - lo;
					s_q[pos] = (uint16_t)ck;
					if (s_spine) {
						s_spine[ck] = s_start[ck] == s_start[t] ? (uint16_t)(s_spine[t] + 1u) : (uint16_t)0u;
						const uint32_t l = s_lvl[t] < 255u ? s_lvl[t] + 1u : 255u;
						s_lvl[ck] = (uint8_t)l;
						s_rootof[ck] = s_rootof[t];
						atomicMax(s_rdepth + s_rootof[t], l);
						atomicAdd(s_cnt + ((uint32_t)s_start[ck] >> 1), (s_start[ck] & 1u) ? 0x10000u : 1u);
					}
				}
				tail += (uint32_t)__builtin_popcountll(m);
			}
		}
		begin = end;
		end = tail;
	}
	return tail;
}

__global__ void __launch_bounds__(64) k_count_tile(int n, const int2 *lr, const float *area, const int *root_list, const uint32_t *tile_nroots, uint32_t *tile_count)
{
	__shared__ int2 s_lr[REFIT_TILE];
	__shared__ float s_area[REFIT_TILE];
	__shared__ uint16_t s_q[REFIT_TILE];
	__shared__ int s_roots[REFIT_TILE / 2];
	__shared__ uint32_t s_nroots;
	const int lo = (int)blockIdx.x * REFIT_TILE;
	const int hi = (lo + REFIT_TILE < n ? lo + REFIT_TILE : n) - 1;
	tile_load<64>(lo, hi, lr, nullptr, area, root_list, tile_nroots[blockIdx.x], s_lr, s_area, nullptr, s_roots, &s_nroots);
	if (threadIdx.x < 64u) {
		const uint32_t count = tile_bfs(lo, s_lr, s_area, nullptr, s_roots, s_nroots, s_q, nullptr, nullptr, nullptr, nullptr, nullptr);
		if (threadIdx.x == 0) tile_count[blockIdx.x] = count;
	}
}

// Transposes the W x W matrix of 16-byte pieces that W neighbouring lanes hold (lane i of the group: pieces p[0 .. W) of ITS
// record) so that lane i ends up with piece i of each of the W records: p[k] = piece i of the record of lane k of the group.
// A store of p[k] then writes the whole record of lane k from W neighbouring lanes -- W * 16 contiguous bytes -- instead of one
// 16-byte piece per lane at the stride of the records (64 partial lines per instruction). All lanes of the wave take part.
template <int W>
__device__ __forceinline__ void transpose_pieces(uint4 (&p)[W])
{
	const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
	for (int s = 1; s < W; s <<= 1) {
		const bool up = (lane & (uint32_t)s) != 0u;
#pragma unroll
		for (int h = 0; h < W / 2; h++) {
			const int a = ((h & ~(s - 1)) << 1) | (h & (s - 1));       // the h-th piece number without bit s
			// (values first, then the select: `up ? p[a] : p[b]` selects between two ADDRESSES, and the array lands in scratch memory)
			uint4 &lo_p = p[a], &hi_p = p[a ^ s];
#define SWAP_PIECE(c_) { const uint32_t l_ = lo_p.c_, h_ = hi_p.c_; const uint32_t send = up ? l_ : h_; const uint32_t recv = (uint32_t)__shfl_xor((int)send, s); lo_p.c_ = up ? recv : l_; hi_p.c_ = up ? h_ : recv; }
			SWAP_PIECE(x) SWAP_PIECE(y) SWAP_PIECE(z) SWAP_PIECE(w)
#undef SWAP_PIECE
		}
	}
}

#ifdef RTK_TILE_PHASES
__device__ unsigned long long g_tile_phase[8];
#define PHASE_MARK(i_) do { if (threadIdx.x == 0) ph[i_] = wall_clock64(); } while (0)
#else
#define PHASE_MARK(i_)
#endif
#ifdef RTK_TILE_WAVES
#define TILE_WAVES_ATTR __attribute__((amdgpu_waves_per_eu(RTK_TILE_WAVES, RTK_TILE_WAVES)))
#else
#define TILE_WAVES_ATTR
#endif
__global__ void __launch_bounds__(TILE_THREADS) TILE_WAVES_ATTR k_collapse_tile(DevTri *tris, int n, const int2 *lr, const uint2 *range, const BinNode *bin, const float *area,
	const int *root_list, const uint32_t *tile_nroots, unsigned long long *root_info, const uint32_t *tile_base, uint32_t node_offset,
	DevNode *nodes, DevNodeQ *qnodes, uint32_t node_cap, DevSceneConsts *consts)
{
	__shared__ int2 s_lr[REFIT_TILE];          //  8 KB
	__shared__ float s_area[REFIT_TILE];       //  4 KB
	__shared__ uint16_t s_start[REFIT_TILE];   //  2 KB: first sorted triangle of node lo + k's range, minus lo
	__shared__ uint16_t s_base[REFIT_TILE];    //  2 KB: jobs whose range starts at lo + k, then their exclusive prefix sums
	__shared__ uint16_t s_round[REFIT_TILE], s_spine[REFIT_TILE], s_map[REFIT_TILE];   // the jobs in breadth-first order; ...; number -> node
	__shared__ uint8_t s_lvl[REFIT_TILE];
	__shared__ uint16_t s_rootof[REFIT_TILE];  //  2 KB: the tile root above node lo + k (its place in s_roots)
	__shared__ uint32_t s_rdepth[REFIT_TILE / 2];   //  2 KB: deepest level below each root
	__shared__ int s_roots[REFIT_TILE / 2];    //  2 KB: the tile roots
	__shared__ uint32_t s_nroots, s_count;
	const int lo = (int)blockIdx.x * REFIT_TILE;
	const int hi = (lo + REFIT_TILE < n ? lo + REFIT_TILE : n) - 1;
	const int t = (int)threadIdx.x;
#ifdef RTK_TILE_PHASES
	unsigned long long ph[6];
#endif
	PHASE_MARK(0);
	tile_load<TILE_THREADS>(lo, hi, lr, range, area, root_list, tile_nroots[blockIdx.x], s_lr, s_area, s_start, s_roots, &s_nroots);
	for (int k = t; k < REFIT_TILE; k += TILE_THREADS) s_base[k] = 0u;
	__syncthreads();
	PHASE_MARK(1);
	if (t < 64) {
		const uint32_t cnt = tile_bfs(lo, s_lr, s_area, s_start, s_roots, s_nroots, s_round, s_spine, s_lvl, reinterpret_cast<uint32_t *>(s_base), s_rootof, s_rdepth);
		// pre-order numbers: jobs that start further left (prefix sums over the per-start counters, 16 per lane) + jobs above
		// with the same start
		uint32_t sum = 0;
		uint32_t v[16];
#pragma unroll
		for (int q = 0; q < 16; q++) { v[q] = s_base[16 * t + q]; sum += v[q]; }
		uint32_t inc = sum;
		for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(inc, o); if (t >= o) inc += u; }
		uint32_t run = inc - sum;
#pragma unroll
		for (int q = 0; q < 16; q++) { s_base[16 * t + q] = (uint16_t)run; run += v[q]; }
		if (t == 0) s_count = cnt;
	}
	__syncthreads();
	PHASE_MARK(2);
	const uint32_t count = s_count;
	const uint32_t base = node_offset + tile_base[blockIdx.x];
#define TILE_LOCAL(k_) ((uint32_t)s_base[s_start[k_]] + (uint32_t)s_spine[k_])
	// the number of each root's node and the levels of its subtree, for the node above the tiles that it hangs in (k_top_finish)
	for (uint32_t r = (uint32_t)t; r < s_nroots; r += TILE_THREADS)
		root_info[s_roots[r]] = ((unsigned long long)(s_rdepth[r] + 1u) << 32) | (unsigned long long)(base + TILE_LOCAL(s_roots[r] - lo));
	// number -> binary node (s_map), then the nodes themselves, dense: thread j makes wide nodes j, j + blockDim, ... of the tile
	for (uint32_t j = (uint32_t)t; j < count; j += TILE_THREADS) { const uint32_t k = s_round[j]; s_map[TILE_LOCAL(k)] = (uint16_t)k; }
	__syncthreads();
	PHASE_MARK(3);
	bool misfit = false;
	// (every lane of a wave goes through the loop as long as one of them has a node to make: the stores below are shared)
	for (uint32_t j = (uint32_t)t; (j & ~63u) < count; j += TILE_THREADS) {
		const bool made = j < count;
		const int bk = made ? (int)s_map[j] : (int)s_map[0];
		int ch4[4];
		const int nc = tile_open(lo + bk, lo, s_lr, s_area, ch4);
		DevNode nd;
		// the boxes of the (up to four) children: a 32-byte binary record or a 48-byte triangle each. All twelve 16-byte loads
		// are issued before the first one is used (one memory round trip per node instead of one per child: the finishing loop
		// was 74 us of a tile's 118)
		float4 r0[4], r1[4], r2[4];
#pragma unroll
		for (int k = 0; k < 4; k++) {
			const bool leaf = k < nc && ch4[k] < 0;
			const float4 *src = leaf ? reinterpret_cast<const float4 *>(tris + (uint32_t)~ch4[k]) : reinterpret_cast<const float4 *>(bin + (k < nc ? ch4[k] : lo));
			r0[k] = src[0]; r1[k] = src[1];
			r2[k] = leaf ? src[2] : r1[k];
		}
#pragma unroll
		for (int k = 0; k < 4; k++) {
			float mn[3], mx[3];
			uint32_t ref;
			if (k >= nc) {
				mn[0] = mn[1] = mn[2] = 1.0f; mx[0] = mx[1] = mx[2] = -1.0f;      // inverted = never hit (rtk.c:1612-1620)
				ref = RTK_REF_NONE;
			} else if (ch4[k] < 0) {
				// a leaf of one triangle (marked as such by k_emit_tris): v0 | v1 | v2 in the first three floats of its rows (tri_box)
				mn[0] = fminf(fminf(r0[k].x, r1[k].x), r2[k].x); mx[0] = fmaxf(fmaxf(r0[k].x, r1[k].x), r2[k].x);
				mn[1] = fminf(fminf(r0[k].y, r1[k].y), r2[k].y); mx[1] = fmaxf(fmaxf(r0[k].y, r1[k].y), r2[k].y);
				mn[2] = fminf(fminf(r0[k].z, r1[k].z), r2[k].z); mx[2] = fmaxf(fmaxf(r0[k].z, r1[k].z), r2[k].z);
				ref = RTK_REF_LEAF | (uint32_t)~ch4[k];
			} else {
				const float4 b0 = r0[k], b1 = r1[k];                              // mn.xyz cnt_flag | mx.xyz cost
				mn[0] = b0.x; mn[1] = b0.y; mn[2] = b0.z; mx[0] = b1.x; mx[1] = b1.y; mx[2] = b1.z;
				if (s_area[ch4[k] - lo] > 0.0f) ref = base + TILE_LOCAL(ch4[k] - lo);
				else {
					const uint2 lf = range[ch4[k]];                                // a subtree the SAH rule turned into one leaf
					if (made) mark_leaf(tris, lf);
					ref = RTK_REF_LEAF | lf.x;
				}
			}
			nd.bx[0][k] = mn[0]; nd.bx[1][k] = mx[0];
			nd.by[0][k] = mn[1]; nd.by[1][k] = mx[1];
			nd.bz[0][k] = mn[2]; nd.bz[1][k] = mx[2];
			nd.child[k] = ref;
		}
		child_order(nd, nd.order);
		DevNodeQ q;
		if (!quantize_node(nd, q) && made) misfit = true;
		// (a tree with more nodes than the scene's arrays were sized for drops the writes beyond them; the host repeats)
		// the stores: eight neighbouring lanes write one node (its eight 16-byte rows), four its compressed copy
		{
			uint4 p[8], pq[4];
#define ROW_F(a_) make_uint4(__float_as_uint((a_)[0]), __float_as_uint((a_)[1]), __float_as_uint((a_)[2]), __float_as_uint((a_)[3]))
#define ROW_U(a_) make_uint4((a_)[0], (a_)[1], (a_)[2], (a_)[3])
			p[0] = ROW_F(nd.bx[0]); p[1] = ROW_F(nd.bx[1]); p[2] = ROW_F(nd.by[0]); p[3] = ROW_F(nd.by[1]);
			p[4] = ROW_F(nd.bz[0]); p[5] = ROW_F(nd.bz[1]); p[6] = ROW_U(nd.child); p[7] = ROW_U(nd.order);
			pq[0] = make_uint4(__float_as_uint(q.org[0]), __float_as_uint(q.org[1]), __float_as_uint(q.org[2]), __float_as_uint(q.scale[0]));
			pq[1] = make_uint4(__float_as_uint(q.scale[1]), __float_as_uint(q.scale[2]), q.q[0][0], q.q[0][1]);
			pq[2] = make_uint4(q.q[1][0], q.q[1][1], q.q[2][0], q.q[2][1]);
			pq[3] = ROW_U(q.child);
#undef ROW_F
#undef ROW_U
			transpose_pieces<8>(p);
			transpose_pieces<4>(pq);
			const uint32_t lane = (uint32_t)t & 63u, j0 = j - lane;
#pragma unroll
			for (uint32_t k = 0; k < 8u; k++) {
				const uint32_t jn = j0 + (lane & ~7u) + k;                                           // the node of lane k of this group of eight
				if (jn < count && base + jn < node_cap) reinterpret_cast<uint4 *>(nodes + base + jn)[lane & 7u] = p[k];
			}
#pragma unroll
			for (uint32_t k = 0; k < 4u; k++) {
				const uint32_t jn = j0 + (lane & ~3u) + k;
				if (jn < count && base + jn < node_cap) reinterpret_cast<uint4 *>(qnodes + base + jn)[lane & 3u] = pq[k];
			}
		}
	}
#undef TILE_LOCAL
	if (misfit) atomicAdd(&consts->qnode_misfits, 1u);
#ifdef RTK_TILE_PHASES
	__syncthreads();
	PHASE_MARK(4);
	if (threadIdx.x == 0) {
		for (int i = 0; i < 4; i++) atomicAdd(&g_tile_phase[i], ph[i + 1] - ph[i]);
		atomicAdd(&g_tile_phase[4], 1ull);
		atomicAdd(&g_tile_phase[5], (unsigned long long)count);
		atomicMax(&g_tile_phase[6], ((ph[4] - ph[0]) << 32) | blockIdx.x);
		atomicMax(&g_tile_phase[7], ((ph[4] - ph[3]) << 32) | count);
	}
#endif
}

// The nodes above the tiles, from the workspace to their places in the scene's arrays, complete: node 0 stays the root, the
// others go BEHIND the tiles' nodes ([1, 1 + *tiles_total): k_collapse_tile, which ran beside the collapse of these) -- so
// neither of the two collapses has to wait for the other one's node count. Child words: a node above the tiles moves with
// the rest, a tile root gets the number k_collapse_tile gave it (root_info), leaves stay. Order words, compressed copy, scene
// bound (node 0) as k_quantize does them; the depth of the tree = the deepest (level of a node here + levels of a tile subtree).
__global__ void __launch_bounds__(256) k_top_finish(const DevNode *top, const uint4 *tile_refs, const uint32_t *level, uint32_t count, const uint32_t *tiles_total,
	const unsigned long long *root_info, DevNode *nodes, DevNodeQ *qnodes, uint32_t node_cap, DevSceneConsts *consts, uint32_t *depth_word)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	uint32_t deepest = 0u;
	bool misfit = false;
	if (i < count) {
		const uint32_t shift = *tiles_total;
		DevNode nd = top[i];
		const uint4 tr4 = tile_refs[i];
		const uint32_t tr[4] = { tr4.x, tr4.y, tr4.z, tr4.w };
		const uint32_t lvl = level[i];
		deepest = lvl + 1u;                                                       // (the scene's depth counts levels from 1)
#pragma unroll
		for (int k = 0; k < 4; k++) {
			if (tr[k]) {
				const unsigned long long info = root_info[tr[k] - 1u];
				nd.child[k] = (uint32_t)info;
				const uint32_t d = lvl + 1u + (uint32_t)(info >> 32);
				deepest = deepest > d ? deepest : d;
			} else if (nd.child[k] != RTK_REF_NONE && !(nd.child[k] & RTK_REF_LEAF)) nd.child[k] += shift;   // (never the root)
		}
		child_order(nd, nd.order);
		if (i == 0u) {
			const float b = root_bound(nd, 0.0f);
			consts->bound_raw = b;
			consts->bound_abs = fmaxf(b, 1.0f);
		}
		DevNodeQ q;
		misfit = !quantize_node(nd, q);
		const uint32_t at = i ? i + shift : 0u;
		if (at < node_cap) { nodes[at] = nd; qnodes[at] = q; }
	}
	if (misfit) atomicAdd(&consts->qnode_misfits, 1u);
	for (int o = 32; o > 0; o >>= 1) { const uint32_t u = __shfl_xor(deepest, o); deepest = deepest > u ? deepest : u; }
	if ((threadIdx.x & 63u) == 0u && deepest) atomicMax(depth_word, deepest);
}

// ---------------------------------------------------------------------------------- host side

float env_float(const char *name, float def)
{
	const char *s = getenv(name);
	return s && *s ? (float)atof(s) : def;
}

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

} // namespace

// =====================================================================================
// rtk_dev_scene_build
// =====================================================================================

namespace {

// All temporaries of a build come out of ONE device allocation per device that is kept between builds
// (grown on demand, released by rtk_amd_release_workspace): the 25 hipMalloc/hipFree pairs of the first
// version cost more than the kernels of a 1M-triangle build. Builds on one device are serialised by the
// mutex, and so is a pass that borrows the workspace (WorkspaceLoan); whoever holds the mutex touches the memory in
// stream order on a stream of its own (ws.stream for a build) and has waited for that stream before letting go.
struct Workspace {
	std::mutex mutex;
	char *base = nullptr;
	size_t cap = 0;
	hipStream_t stream = nullptr;     // builds of this device run on a stream of their own (not the NULL stream, which would serialise
	                                  // them with every blocking stream of the host), one at a time (the mutex: they share the workspace)
	hipStream_t side = nullptr;       // tile mode: the per-tile node counts and their prefix sums run here, beside the collapse of the
	hipEvent_t fork = nullptr, join = nullptr;      // nodes above the tiles (a string of small launches that leaves the GPU mostly idle)
	struct BuildResults *h_results = nullptr;       // pinned: what a build brings home (kernels write it; the host reads it after its one wait)
};
Workspace g_workspace[RTK_MAX_DEVICES];

// The workspace (its mutex held) grown to at least `bytes`: asks for bytes + bytes / slack_div (0: no slack), and once more for
// exactly `bytes` if that much cannot be had. False: out of device memory, the workspace is empty.
bool workspace_grow(Workspace &w, size_t bytes, unsigned slack_div)
{
	if (w.base && w.cap >= bytes) return true;
	if (w.base) (void)hipFree(w.base);
	w.base = nullptr;
	w.cap = 0;
	const size_t want = bytes + (slack_div ? bytes / slack_div : 0);
	for (const size_t ask : { want, bytes }) {
		if (hipMalloc(&w.base, ask) == hipSuccess) { w.cap = ask; return true; }
		(void)hipGetLastError();
		w.base = nullptr;
		if (want == bytes) break;
	}
	return false;
}

// How one mesh reaches the ingest kernel.
struct MeshPlan {
	bool on_host_decode = false;    // callbacks: decoded on the host, copied as plain positions
	bool f64 = false;
	int idx_kind = 0;               // 0 implicit, 1 u16, 2 u32
	size_t pstride = 0, istride = 0;
	size_t pbytes = 0, ibytes = 0;  // bytes to upload (0: already device memory / nothing)
	const char *pos_src = nullptr, *idx_src = nullptr;
	bool pos_on_device = false, idx_on_device = false;
};

int cached_cu_count(int device)
{
	static std::mutex m;
	static int cus[RTK_MAX_DEVICES];
	std::lock_guard<std::mutex> lock(m);
	if (device < 0 || device >= RTK_MAX_DEVICES) return 256;
	if (cus[device] == 0) {
		int v = 0;
		if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || v <= 0) v = 256;
		cus[device] = v;
	}
	return cus[device];
}

} // namespace

extern "C" void rtk_amd_release_workspace(void)
{
	for (int d = 0; d < RTK_MAX_DEVICES; d++) {
		Workspace &w = g_workspace[d];
		std::lock_guard<std::mutex> lock(w.mutex);
		if (!w.base) continue;
		int cur = 0;
		(void)hipGetDevice(&cur);
		(void)hipSetDevice(d);
		(void)hipFree(w.base);
		(void)hipSetDevice(cur);
		w.base = nullptr;
		w.cap = 0;
	}
}

void rtk_sah_costs(float *cost_node, float *cost_tri)
{
	*cost_tri = env_float("RTK_AMD_SAH_CT", 1.0f);
	*cost_node = env_float("RTK_AMD_SAH_CN", 0.5f);     // sweeps on MI355X: small leaves win (profiles/r01_sweep_sah2.log)
}

// Caller memory that is already device memory (hipMalloc) is read in place (the ingest kernel, a refit's gather).
bool rtk_is_device_ptr(const void *p)
{
	hipPointerAttribute_t attr;
	if (hipPointerGetAttributes(&attr, p) != hipSuccess) { (void)hipGetLastError(); return false; }
	return attr.type == hipMemoryTypeDevice;
}

// WorkspaceLoan (rtk_dev.h): the workspace of a device, grown to `bytes` if need be, under its mutex
bool WorkspaceLoan::take(int dev, size_t bytes)
{
	if (device >= 0) { rtk_set_error("workspace: already borrowed"); return false; }
	if (dev < 0 || dev >= RTK_MAX_DEVICES) { rtk_set_error("workspace: device %d out of range", dev); return false; }
	Workspace &w = g_workspace[dev];
	w.mutex.lock();
	const size_t want = bytes ? bytes : 256;
	if (!workspace_grow(w, want, 0)) {
		w.mutex.unlock();
		rtk_set_error("workspace: out of device memory (%zu bytes)", want);
		return false;
	}
	device = dev;
	base = w.base;
	return true;
}

void WorkspaceLoan::release()
{
	if (device < 0) return;
	g_workspace[device].mutex.unlock();
	device = -1;
	base = nullptr;
}

namespace {

// ---- knobs: every environment variable the build reads, read in one place at the top of a build ----

// "set it to 0 to turn it off": true unless the variable is there and reads as 0
bool env_unless_zero(const char *name)
{
	const char *s = getenv(name);
	return !(s && atoi(s) == 0);
}

struct BuildKnobs {
	bool timing;             // RTK_AMD_BUILD_TIMING (set at all): the device time of every stage, with a device synchronisation after each
	bool host_time;          // RTK_AMD_BUILD_HOSTTIME=1: where the HOST is when (no synchronisation: how far ahead of the GPU the enqueueing thread runs)
	uint32_t max_leaf;       // RTK_AMD_MAX_LEAF, 1 .. 63
	bool sort_packed;        // RTK_AMD_SORT_PACKED=0: the >= 2^24-triangle path (key, index pairs), for tests on small scenes
	uint32_t key_bits;       // RTK_AMD_KEY_BITS: 8 .. 40 in steps of 8, the width of the Morton code in the packed sort words (0: from the number of triangles)
	bool direct;             // RTK_AMD_BUILD_DIRECT=0: every mesh is staged, none gathered in place by the emit. Read once per process.
	bool fused_emit;         // RTK_AMD_FUSED_EMIT=0: the triangle records are made by a pass of their own, not inside k_refit_tile (A/B)
	uint64_t tile_min;       // RTK_AMD_TILE_COLLAPSE_MIN: triangles from which the tile collapse is used (see below)
	uint32_t top_cap;        // RTK_AMD_TOP_CAP: at most so many nodes above the tiles, to drive the way back to the level-by-level collapse from tests
	int est_div;             // RTK_AMD_NODE_ESTIMATE_DIV: node arrays of n / div + 16 nodes at first, to drive the repeat path from tests (0: the usual estimate)
	bool keep_workspace;     // RTK_AMD_KEEP_WORKSPACE=0: the workspace is freed after every build
	bool key_rebuild;        // RTK_AMD_KEY_REBUILD=0: a scene whose narrow keys collide too often is not built again with wide ones
};

} // namespace

// RTK_AMD_MAX_LEAF, 1 .. 63, default 3: the device builder's leaf limit, and what rtk_dev_scene_split_leaves takes for max_leaf 0
uint32_t rtk_build_max_leaf()
{
	uint32_t max_leaf = (uint32_t)env_float("RTK_AMD_MAX_LEAF", 3.0f);
	if (max_leaf < 1) max_leaf = 1;
	if (max_leaf > 63) max_leaf = 63;         // 6-bit count in the blob's leaf header (rtk.c:188)
	return max_leaf;
}

namespace {

BuildKnobs read_build_knobs()
{
	BuildKnobs k;
	k.timing = getenv("RTK_AMD_BUILD_TIMING") != nullptr;
	k.host_time = getenv("RTK_AMD_BUILD_HOSTTIME") && atoi(getenv("RTK_AMD_BUILD_HOSTTIME")) != 0;
	// leaves of at most three triangles: a leaf of fewer than four is one partial group for the reference's group-of-four rule
	// (rtk.c:302-336: double-precision edge functions, no redo), which is all the hand-written packet kernel implements; with
	// cn = 0.5 the SAH rule made 1.008 triangles per leaf at a limit of 8, so nothing of substance changes
	k.max_leaf = rtk_build_max_leaf();
	k.sort_packed = env_unless_zero("RTK_AMD_SORT_PACKED");
	k.key_bits = 0;
	if (getenv("RTK_AMD_KEY_BITS")) { const int kb = atoi(getenv("RTK_AMD_KEY_BITS")); if (kb >= 8 && kb <= 40 && kb % 8 == 0) k.key_bits = (uint32_t)kb; }
	static const bool allow_direct = env_unless_zero("RTK_AMD_BUILD_DIRECT");
	k.direct = allow_direct;
	k.fused_emit = env_unless_zero("RTK_AMD_FUSED_EMIT");
	// Tile mode (the subtrees inside a refit tile collapsed by k_collapse_tile), measured on MI355X (profiles/r05_build_timing.log, level
	// by level / tile mode): 0.47 / 0.46 ms at 0.5M triangles, 0.555 / 0.540 at 1M, 0.785 / 0.748 at 2M, 1.005 / 0.935 at 3M -- since the
	// tiles' kernels run beside pass 2 and the top collapse, tile mode is never slower; its trees have ~2 % more nodes (tile roots are never
	// opened from above: ~1 % more node visits per ray), so it starts where the build time it saves is worth more than that: 1.5M
	// triangles. RTK_AMD_TILE_COLLAPSE_MIN (triangles; read per build) moves that: 0 = whenever there are two tiles, a huge value =
	// never (everything level by level: A/B).
	const char *tile_env = getenv("RTK_AMD_TILE_COLLAPSE_MIN");
	k.tile_min = tile_env ? (uint64_t)atoll(tile_env) : (3ull << 19);
	k.top_cap = getenv("RTK_AMD_TOP_CAP") ? (uint32_t)atoi(getenv("RTK_AMD_TOP_CAP")) : 0xffffffffu;
	k.est_div = getenv("RTK_AMD_NODE_ESTIMATE_DIV") ? atoi(getenv("RTK_AMD_NODE_ESTIMATE_DIV")) : 0;
	k.keep_workspace = env_unless_zero("RTK_AMD_KEEP_WORKSPACE");
	k.key_rebuild = env_unless_zero("RTK_AMD_KEY_REBUILD");
	return k;
}

static_assert(sizeof(InTri) == RTK_BUILD_SIZEOF_INTRI && sizeof(BinNode) == RTK_BUILD_SIZEOF_BINNODE && sizeof(Climb) == RTK_BUILD_SIZEOF_CLIMB &&
	sizeof(LevelState) == RTK_BUILD_SIZEOF_LEVELSTATE && sizeof(MeshSrc) == RTK_BUILD_SIZEOF_MESHSRC && sizeof(DevNode) == RTK_BUILD_SIZEOF_DEVNODE,
	"rtk_build_layout.h sizes the workspace by these");
static_assert(REFIT_TILE == RTK_BUILD_REFIT_TILE && COLLAPSE_BLOCK == RTK_BUILD_COLLAPSE_BLOCK && COLLAPSE_RING == RTK_BUILD_COLLAPSE_RING, "rtk_build_layout.h");

// ---- one build: what its stages share ----
struct Build {
	// where the triangles come from: a description (rtk_dev_scene_build), or the records of a live scene (rtk_dev_scene_rebuild).
	// Only plan_meshes and the two ingests look at it; from there on a build knows the number of meshes and mesh_base.
	const rtk_scene_desc *desc = nullptr;
	const rtk_placement *placements = nullptr;   // rtk_dev_scene_build_placed: one per mesh of desc (host memory), else NULL
	const rtk_dev_scene *from = nullptr;
	size_t num_meshes = 0;
	int rc = RTK_AMD_ERR_HIP;         // what a failed build reports where a code is wanted (the rebuild): set by whoever returns false
	uint32_t n = 0;
	int device = 0, num_cus = 0;
	BuildKnobs knobs;
	BuildParams bp;
	std::vector<uint64_t> mesh_base;
	std::vector<MeshPlan> plans;
	// what n and the knobs decide
	bool packed = false;              // the triangle's number fits under a 40-bit code in one sort word
	uint32_t packed_bits = 40u;       // the width of that code
	uint32_t num_tiles = 0;
	bool tile_mode = false;           // more than one refit tile, and enough triangles: the subtrees inside a tile are collapsed by k_collapse_tile,
	                                  // only the nodes above them go through the level-by-level collapse
	uint32_t top_cap = 0;             // nodes above the tiles that the workspace holds
	// the workspace (its mutex is held by build_impl), the two streams, the scene under construction
	Workspace *ws = nullptr;
	hipStream_t bs = nullptr;         // the build's stream
	hipStream_t cs = nullptr;         // where the tiles' own kernels run: ws->side once it has forked off, else bs
	bool forked = false;
	bool side_busy = false;           // kernels on ws->side may still be reading the workspace
	BuildResults *results = nullptr;
	rtk_dev_scene *ds = nullptr;
	// the layout (byte offsets) and its pointers; what else the stages hand on
	BuildLayout L;
	InTri *in_tris = nullptr;
	float *d_cent = nullptr, *d_area = nullptr;
	uint32_t *d_bounds = nullptr, *d_vidx_in = nullptr, *d_tile_count = nullptr, *d_tile_base = nullptr, *d_depth_word = nullptr, *d_tile_nclimb = nullptr, *d_tile_nroots = nullptr, *d_top_level = nullptr;
	int2 *d_lr = nullptr;
	uint2 *d_range = nullptr;
	Climb *d_climbers = nullptr;
	unsigned long long *d_half = nullptr, *d_root_info = nullptr, *d_mesh_base = nullptr;
	int *d_climb_idx = nullptr, *d_root = nullptr, *d_root_list = nullptr;
	BinNode *d_bin = nullptr;
	DevNode *d_nodes_tmp = nullptr;
	uint4 *d_top_refs = nullptr;
	MeshSrc *d_mesh_src = nullptr;
	LevelState *d_ring = nullptr;
	CollapseBufs cb = {};
	TopAux top_aux = { nullptr, nullptr };
	std::vector<MeshSrc> mesh_src;            // sources of async copies: they live until the final wait
	std::vector<unsigned long long> mb;
	const unsigned long long *keys = nullptr; // sorted. packed: all different (the index is part of the word), in ascending order
	const uint32_t *vals = nullptr;
	DevTri *d_tris = nullptr;
	EmitSrc emit_src = {};
	const DevTri *old_tris = nullptr; // a rebuild: what make_tri gathers from (ingest_scene)
	const uint32_t *slot_of = nullptr;
	// the collapse
	void *node_mem = nullptr;         // [DevNode x node_cap | DevNodeQ x node_cap], owned by the scene (Build::node_alloc)
	size_t node_cap = 0;
	LevelState h_state = {};
	bool tiles_done = false;
	uint32_t total_nodes = 0, depth = 0;
	uint32_t equal_codes = 0;         // sorted neighbours with one and the same Morton code (counted by k_refit_tile)
	std::chrono::steady_clock::time_point t_begin, t_last;

	template <typename T> T *at(size_t offset) const { return offset == RTK_BUILD_NO_BUFFER ? nullptr : reinterpret_cast<T *>(ws->base + offset); }

	void stage(const char *name)
	{
		if (knobs.host_time) fprintf(stderr, "rtk_amd build host: %-10s at %8.3f ms\n", name, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count());
		if (!knobs.timing) return;
		(void)hipDeviceSynchronize();
		const auto now = std::chrono::steady_clock::now();
		fprintf(stderr, "rtk_amd build: %-10s %8.3f ms\n", name, std::chrono::duration<double, std::milli>(now - t_last).count());
		t_last = now;
	}

	// The one way out of a failed build; every stage returns what these return (false). Before the scene exists nothing has been
	// enqueued and there is nothing to free. From then on kernels already enqueued may still read or write the persistent
	// workspace (the next build on this device reuses it as soon as build_impl lets go of the workspace mutex) and the scene's
	// own allocations (freed here): BOTH streams are joined first, the side stream if anything was enqueued on it.
	bool give_up()
	{
		if (!ds) return false;
		(void)hipStreamSynchronize(bs);
		if (side_busy) (void)hipStreamSynchronize(ws->side);
		rtk_dev_scene_free(ds);
		ds = nullptr;
		return false;
	}
	// (the error text is made before the streams are joined: the wait may change the last error)
	bool fail(const char *what)
	{
		const hipError_t e = hipGetLastError();
		rc = e == hipErrorOutOfMemory ? RTK_AMD_ERR_OOM : RTK_AMD_ERR_HIP;
		rtk_set_error("device build: %s: %s", what, hipGetErrorString(e));
		return give_up();
	}
	// a device allocation the scene owns
	char *dev_alloc(size_t bytes) { return (char *)ds->mem.own(bytes ? bytes : 16, bytes); }
	// the scene's node block for node_cap nodes, instead of the one there is (error paths free it with the scene)
	bool node_alloc()
	{
		ds->mem.release(node_mem);
		const size_t bytes = node_cap * (sizeof(DevNode) + sizeof(DevNodeQ));
		node_mem = ds->mem.own(bytes, bytes);
		return node_mem != nullptr;
	}
};

// ---- plan the meshes: host only; everything that can be wrong with the description is found here ----
bool plan_meshes(Build &b)
{
	const rtk_scene_desc *desc = b.desc;
	b.plans.assign(desc->num_meshes, MeshPlan());
	for (size_t mi = 0; mi < desc->num_meshes; mi++) {
		const rtk_mesh *m = &desc->meshes[mi];
		MeshPlan &pl = b.plans[mi];
		const size_t nt = m->num_triangles;
		if (nt == 0) continue;
		if (!m->position_cb && m->position.type != RTK_TYPE_DEFAULT && m->position.type != RTK_TYPE_REAL && m->position.type != RTK_TYPE_F32 &&
			m->position.type != RTK_TYPE_F64) { rtk_set_error("rtk_dev_scene_build: mesh %zu: bad position type %d", mi, (int)m->position.type); return false; }
		// RTK_TYPE_DEFAULT on an index buffer means 32-bit indices (the reference's default index type, rtk.c:1049-1059)
		if (!m->index_cb && m->index.data && m->index.type != RTK_TYPE_DEFAULT && m->index.type != RTK_TYPE_U16 && m->index.type != RTK_TYPE_U32) {
			rtk_set_error("rtk_dev_scene_build: mesh %zu: bad index type %d", mi, (int)m->index.type); return false; }
		if (b.placements && m->position_cb) { b.rc = RTK_AMD_ERR_UNSUPPORTED; rtk_set_error("rtk_dev_scene_build_placed: mesh %zu: a position callback gives world positions, it takes no placement", mi); return false; }
		if (m->position_cb || m->index_cb || b.n < 2) { pl.on_host_decode = true; continue; }
		if (!m->position.data) { rtk_set_error("rtk_dev_scene_build: mesh %zu has no positions", mi); return false; }
		pl.f64 = m->position.type == RTK_TYPE_F64;
		pl.pstride = m->position.stride ? m->position.stride : (pl.f64 ? 24 : 12);
		pl.pos_src = (const char *)m->position.data;
		pl.pos_on_device = rtk_is_device_ptr(m->position.data);
		uint64_t max_vertex = 3ull * nt - 1;
		if (m->index.data) {
			const bool u16 = m->index.type == RTK_TYPE_U16;
			pl.idx_kind = u16 ? 1 : 2;
			pl.istride = m->index.stride ? m->index.stride : (u16 ? 6 : 12);
			pl.idx_src = (const char *)m->index.data;
			pl.idx_on_device = rtk_is_device_ptr(m->index.data);
			if (pl.idx_on_device && !pl.pos_on_device) { rtk_set_error("rtk_dev_scene_build: mesh %zu has device indices but host positions", mi); return false; }
			if (!pl.idx_on_device) {
				if (!pl.pos_on_device) {
					// the position buffer's extent is only known through the largest index used
					max_vertex = 0;
					for (size_t i = 0; i < nt; i++) {
						const char *p = pl.idx_src + i * pl.istride;
						for (int c = 0; c < 3; c++) {
							const uint64_t v = u16 ? ((const uint16_t *)p)[c] : ((const uint32_t *)p)[c];
							if (v > max_vertex) max_vertex = v;
						}
					}
				}
				pl.ibytes = (nt - 1) * pl.istride + (u16 ? 6 : 12);
			}
		}
		if (!pl.pos_on_device) pl.pbytes = (size_t)max_vertex * pl.pstride + (pl.f64 ? 24 : 12);
	}
	return true;
}

// ---- what n and the knobs decide before anything is placed: sort words, key width, tile mode ----
void plan_build(Build &b, uint32_t force_bits)
{
	const uint32_t n = b.n;
	// index fits under a 40-bit code in one word
	b.packed = n < (1u << 24) && b.knobs.sort_packed;
	// Key width from n: ceil(log2 n) + 8 bits of the code, rounded up to whole 8-bit passes -- every triangle still gets hundreds
	// of cells of its own on average, the splits below that are decided by the triangle's number (words are all different). The lab
	// found identical trees down to 30 bits at 1M triangles, and the 10M-triangle build has the same 4 709 302 nodes at 32 bits as at
	// 40 (profiles/r04_build_ab.log): 32 bits = FOUR passes wherever the index fits the word (n < 2^24), three below 64 k triangles.
	uint32_t lg = 0;
	while ((1ull << lg) < (unsigned long long)n) lg++;
	b.packed_bits = ((lg + 8u + 7u) / 8u) * 8u;
	if (b.packed_bits < 24u) b.packed_bits = 24u;
	if (b.packed_bits > 40u) b.packed_bits = 40u;
	if (force_bits) b.packed_bits = force_bits;
	if (b.knobs.key_bits) b.packed_bits = b.knobs.key_bits;
	b.num_tiles = (n + REFIT_TILE - 1u) / REFIT_TILE;
	b.tile_mode = b.num_tiles > 1u && (uint64_t)n >= b.knobs.tile_min;
	b.top_cap = std::min<uint32_t>(n / 2u, b.knobs.top_cap);
	rtk_sah_costs(&b.bp.cost_node, &b.bp.cost_tri);
	b.bp.max_leaf = b.knobs.max_leaf;
}

// ---- the workspace: sized and placed by the one carve of rtk_build_layout.h; the build's stream and pinned results ----
bool prepare_workspace(Build &b)
{
	Workspace &ws = *b.ws;
	std::vector<BuildUpload> uploads(b.plans.size());
	for (size_t mi = 0; mi < b.plans.size(); mi++) uploads[mi] = BuildUpload{ b.plans[mi].ibytes, b.plans[mi].pbytes };
	BuildLayout &L = b.L;
	if (!rtk_build_layout(b.n, uploads, b.packed, b.tile_mode, b.top_cap, rtk_sort_scratch_words(b.n), &L)) { rtk_set_error("device build: workspace too small (internal error)"); return false; }
	if (!workspace_grow(ws, L.bytes, 8) || L.bytes > ws.cap) { b.rc = RTK_AMD_ERR_OOM; rtk_set_error("device build: out of device memory (%zu bytes of workspace)", L.bytes); return false; }
	if (!ws.stream && hipStreamCreateWithFlags(&ws.stream, hipStreamNonBlocking) != hipSuccess) { ws.stream = nullptr; rtk_set_error("device build: hipStreamCreate failed"); return false; }
	if (!ws.h_results && hipHostMalloc(reinterpret_cast<void **>(&ws.h_results), sizeof(BuildResults), hipHostMallocDefault) != hipSuccess) {
		(void)hipGetLastError();
		ws.h_results = nullptr;
		b.rc = RTK_AMD_ERR_OOM;
		rtk_set_error("device build: no pinned host memory for the build's results");
		return false;
	}
	b.results = ws.h_results;
	b.bs = b.cs = ws.stream;
	b.in_tris = b.at<InTri>(L.in_tris); b.d_cent = b.at<float>(L.cent); b.d_bounds = b.at<uint32_t>(L.bounds); b.d_mesh_src = b.at<MeshSrc>(L.mesh_src);
	b.d_lr = b.at<int2>(L.lr); b.d_range = b.at<uint2>(L.range); b.d_climbers = b.at<Climb>(L.climbers); b.d_root = b.at<int>(L.root); b.d_bin = b.at<BinNode>(L.bin);
	b.d_half = b.at<unsigned long long>(L.half);      // two subtrees meet through the first n words
	b.d_climb_idx = b.at<int>(L.arrive);              // pass 2 finds its climbers through their positions, packed per tile, and d_tile_nclimb
	b.d_tile_count = b.at<uint32_t>(L.tile_count); b.d_tile_base = b.at<uint32_t>(L.tile_base); b.d_tile_nclimb = b.at<uint32_t>(L.tile_nclimb); b.d_tile_nroots = b.at<uint32_t>(L.tile_nroots);
	b.d_depth_word = b.at<uint32_t>(L.depth_word); b.d_area = b.at<float>(L.area); b.d_nodes_tmp = b.at<DevNode>(L.nodes_tmp);
	b.d_top_refs = b.at<uint4>(L.top_refs); b.d_top_level = b.at<uint32_t>(L.top_level); b.d_root_info = b.at<unsigned long long>(L.root_info); b.d_root_list = b.at<int>(L.root_list);
	b.cb = CollapseBufs{ b.at<int>(L.jobs), b.at<int4>(L.dec), b.at<uint32_t>(L.info), b.at<uint32_t>(L.sums) };
	b.d_ring = b.at<LevelState>(L.ring);
	b.top_aux = TopAux{ b.d_top_refs, b.d_top_level };
	// a mesh that already lives in device memory was written by the caller's own work, possibly still in flight on the NULL
	// stream or a blocking stream: that work is waited for here (a build stream of our own does not order itself behind it)
	bool device_mesh = false;
	for (const MeshPlan &pl : b.plans) device_mesh = device_mesh || pl.pos_on_device || pl.idx_on_device;
	if (device_mesh && hipStreamSynchronize(0) != hipSuccess) return b.fail("hipStreamSynchronize(0)");
	b.stage("workspace");
	return true;
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
	if (any_indexed) {
		b.d_vidx_in = (uint32_t *)b.dev_alloc(3 * (size_t)b.n * 4);
		if (!b.d_vidx_in) { (void)hipGetLastError(); rtk_set_error("device build: out of device memory (vertex indices)"); return b.give_up(); }
		ds->tree.d_vidx_in = b.d_vidx_in;
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
			hipLaunchKernelGGL(k_bounds, dim3(bblocks), dim3(BOUNDS_BLOCK), 0, bs, b.in_tris, base, (uint32_t)nt, b.d_bounds, b.d_cent, b.d_vidx_in);
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
		if (pl.idx_kind == 0) launch_ingest<0>(pl.f64, direct, place, iblocks, pos_ptr, pl.pstride, idx_ptr, pl.istride, (uint32_t)nt, base, b.in_tris, b.d_cent, b.d_vidx_in, b.d_bounds, bs);
		else if (pl.idx_kind == 1) launch_ingest<1>(pl.f64, false, place, iblocks, pos_ptr, pl.pstride, idx_ptr, pl.istride, (uint32_t)nt, base, b.in_tris, b.d_cent, b.d_vidx_in, b.d_bounds, bs);
		else launch_ingest<2>(pl.f64, false, place, iblocks, pos_ptr, pl.pstride, idx_ptr, pl.istride, (uint32_t)nt, base, b.in_tris, b.d_cent, b.d_vidx_in, b.d_bounds, bs);
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
constexpr uint32_t BUILD_KEY_BITS = 63u;
bool keys_and_sort(Build &b)
{
	const uint32_t n = b.n;
	unsigned long long *keys_a = b.at<unsigned long long>(b.L.keys_a), *keys_b = b.at<unsigned long long>(b.L.keys_b);
	uint32_t *vals_a = b.at<uint32_t>(b.L.vals_a), *vals_b = b.at<uint32_t>(b.L.vals_b);       // (NULL when packed)
	uint32_t *sort_scratch = b.at<uint32_t>(b.L.sort_scratch);
	hipLaunchKernelGGL(k_morton, dim3((n + 255u) / 256u), dim3(256), 0, b.bs, b.d_cent, n, b.d_bounds, keys_a, vals_a, 63u - (b.packed ? b.packed_bits : BUILD_KEY_BITS));
	if (hipGetLastError() != hipSuccess) return b.fail("morton launch");
	b.stage("morton");
	const bool in_b = b.packed ? rtk_sort_words_async(keys_a, keys_b, n, 24u, 24u + b.packed_bits, sort_scratch, b.bs)
	                           : rtk_sort_pairs_async(keys_a, keys_b, vals_a, vals_b, n, BUILD_KEY_BITS, sort_scratch, b.bs);
	b.keys = in_b ? keys_b : keys_a;
	b.vals = b.packed ? nullptr : (in_b ? vals_b : vals_a);
	if (hipGetLastError() != hipSuccess) return b.fail("sort launch");
	b.stage("sort");
	return true;
}

// ---- 5 emit: final triangle records in Morton order ----
bool emit(Build &b)
{
	const uint32_t n = b.n;
	b.mb.assign(b.mesh_base.begin(), b.mesh_base.end());
	// the triangle records; the mesh table (a few words the scene keeps: rtk_scene_side_arrays reads it)
	Carve c;
	const size_t o_tris = c.take((size_t)n * sizeof(DevTri)), o_mb = c.take(b.mb.size() * 8);
	char *tri_mem = b.dev_alloc(c.bytes);
	if (!tri_mem) return b.fail("out of device memory");
	b.d_tris = (DevTri *)(tri_mem + o_tris);
	b.d_mesh_base = (unsigned long long *)(tri_mem + o_mb);
	b.ds->tree.d_mesh_base = b.d_mesh_base;
	if (hipMemcpyAsync(b.d_mesh_base, b.mb.data(), b.mb.size() * 8, hipMemcpyHostToDevice, b.bs) != hipSuccess ||
		hipMemcpyAsync(b.d_mesh_src, b.mesh_src.data(), b.mesh_src.size() * sizeof(MeshSrc), hipMemcpyHostToDevice, b.bs) != hipSuccess) return b.fail("copy");
	// the triangle records in sorted order are made by k_refit_tile, which needs them next (RTK_AMD_FUSED_EMIT=0: by a pass of their own, A/B)
	b.emit_src = EmitSrc{ b.in_tris, b.d_mesh_src, b.vals, b.keys, b.d_mesh_base, (uint32_t)b.num_meshes, b.old_tris, b.slot_of };
	if (!b.knobs.fused_emit) {
		hipLaunchKernelGGL(k_emit_tris, dim3((n + 255u) / 256u), dim3(256), 0, b.bs, b.emit_src, n, b.d_tris);
		if (hipGetLastError() != hipSuccess) return b.fail("emit launch");
		b.emit_src.src = nullptr;
	}
	b.stage("emit");
	return true;
}

// ---- 6 + 7 tree topology and refit in one bottom-up pass (no separate tree-building kernel), then the nodes that cross tile borders ----
bool refit(Build &b)
{
	Workspace &ws = *b.ws;
	const hipStream_t bs = b.bs;
	const uint32_t num_tiles = b.num_tiles;
	if (hipMemsetAsync(b.d_depth_word, 0, 16, bs) != hipSuccess) return b.fail("memset");
	// (the scene's constants block: allocated and cleared here, not between the collapse and the last kernel -- a hipMalloc there was 40 us
	// in which the GPU waited; in tile mode also before the second stream forks off. The callee's error text stands.)
	if (rtk_scene_consts(b.ds, bs) != RTK_AMD_OK) return b.give_up();
	hipLaunchKernelGGL(k_refit_tile, dim3(num_tiles), dim3(REFIT_BLOCK), 0, bs, b.d_tris, (int)b.n, b.keys, b.d_lr, b.d_range,
		b.d_bin, b.d_climbers, b.d_half, b.d_climb_idx, b.d_tile_nclimb, b.d_root, b.bp, b.d_area, b.d_depth_word + 1, b.d_root_list,
		b.tile_mode ? b.d_tile_nroots : (uint32_t *)nullptr, b.emit_src);
	if (b.tile_mode) {
		// how many wide nodes every tile makes, and where they start, then (collapse_tiles, once the node arrays are allocated) the tiles' nodes
		// themselves: on a stream of their own, beside pass 2 of the refit and the collapse of the nodes above the tiles -- a chain of
		// latency-bound launches with host round trips between them, 0.3 ms at 10M triangles in which the chip would have next to
		// nothing to do. (The tiles' kernels read what pass 1 wrote and nothing that pass 2 writes: k_refit_tile lists the roots.)
		if (!ws.side && (hipStreamCreateWithFlags(&ws.side, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&ws.fork, hipEventDisableTiming) != hipSuccess ||
				hipEventCreateWithFlags(&ws.join, hipEventDisableTiming) != hipSuccess)) {
			(void)hipGetLastError();
			if (ws.side) (void)hipStreamDestroy(ws.side);
			ws.side = nullptr;                       // (events created so far are kept for the next attempt: a handful of bytes)
		}
		b.forked = ws.side && hipEventRecord(ws.fork, bs) == hipSuccess && hipStreamWaitEvent(ws.side, ws.fork, 0) == hipSuccess;
		b.cs = b.forked ? ws.side : bs;
		hipLaunchKernelGGL(k_count_tile, dim3(num_tiles), dim3(64), 0, b.cs, (int)b.n, b.d_lr, b.d_area, b.d_root_list, b.d_tile_nroots, b.d_tile_count);
		hipLaunchKernelGGL(k_scan_tiles, dim3(1), dim3(1024), 0, b.cs, b.d_tile_count, num_tiles, b.d_tile_base);
		if (b.forked) b.side_busy = true;
	}
	hipLaunchKernelGGL(k_refit_top, dim3(num_tiles), dim3(64), 0, bs, b.d_tris, (int)b.n, b.keys, b.d_climbers, b.d_climb_idx, b.d_tile_nclimb, b.d_half, b.d_bin, b.d_lr, b.d_range,
		b.d_root, b.bp, b.tile_mode);
	if (hipGetLastError() != hipSuccess) return b.fail("refit");
	b.stage("refit");
	return true;
}

// ---- 8 collapse ----
// The node arrays of the scene, [DevNode x node_cap | DevNodeQ x node_cap], are allocated before the collapse -- the GPU is still
// busy with the refit -- at the size 4-wide trees over n triangles usually have (0.47 n on the benchmark scenes), and the
// collapse writes its nodes straight into them. A tree with more nodes than that drops the writes beyond the capacity
// (the kernels check) and is collapsed once more: into an exact allocation (tile mode) or into the workspace.
// (no node memory afterwards: the estimate could not be allocated -- a dry round gives the exact size)
void alloc_node_estimate(Build &b)
{
	b.node_cap = b.knobs.est_div > 0 ? (size_t)b.n / (size_t)b.knobs.est_div + 16 : (size_t)b.n / 2 + 4096;
	if (!b.node_alloc()) { (void)hipGetLastError(); b.node_cap = 0; }
}

// The level-by-level collapse into `target` (room for `cap` nodes; more are counted but not written). False: a launch or the
// wait failed (nothing is cleaned up here). b.h_state: the last level, with the number of nodes.
bool run_collapse(Build &b, DevNode *target, uint32_t cap, uint64_t jobs_hint)
{
	const hipStream_t bs = b.bs;
	const unsigned big_blocks = (unsigned)std::min<uint64_t>((jobs_hint + COLLAPSE_BLOCK - 1) / COLLAPSE_BLOCK, (uint64_t)b.num_cus * 16);
	// levels with more than COLLAPSE_SMALL jobs in a balanced 4-wide tree over jobs_hint leaves, plus slack; a tree that is
	// deeper than that takes further rounds
	unsigned big_levels = 2;
	for (uint64_t c = COLLAPSE_SMALL_JOBS; c < jobs_hint; c *= 4) big_levels++;
	uint32_t step = 0;
	for (unsigned round = 0;; round++) {
		hipLaunchKernelGGL(k_collapse_small, dim3(1), dim3(COLLAPSE_SMALL), 0, bs, b.cb, b.d_ring, step++, 16u, b.d_lr, b.d_range, b.d_bin, b.d_tris, target, cap, b.d_root, b.top_aux, (LevelState *)nullptr);
		for (unsigned k = 0; k < big_levels; k++) {
			// number the level of ring entry `step` (-> entry step + 1: the next level, not opened yet), then open that
			hipLaunchKernelGGL(k_collapse_number, dim3(big_blocks), dim3(COLLAPSE_BLOCK), 0, bs, b.cb, b.d_ring, step, target, cap);
			step++;
			hipLaunchKernelGGL(k_collapse_open, dim3(big_blocks), dim3(COLLAPSE_BLOCK), 0, bs, b.cb, b.d_ring, step, b.d_lr, b.d_range, b.d_bin, b.d_tris, target, cap, b.top_aux);
		}
		// (the level the round ends at goes straight into pinned host memory)
		hipLaunchKernelGGL(k_collapse_small, dim3(1), dim3(COLLAPSE_SMALL), 0, bs, b.cb, b.d_ring, step++, 16u, b.d_lr, b.d_range, b.d_bin, b.d_tris, target, cap, b.d_root, b.top_aux, &b.results->level);
		if (hipGetLastError() != hipSuccess || hipStreamSynchronize(bs) != hipSuccess) return false;
		memcpy(&b.h_state, const_cast<const LevelState *>(&b.results->level), sizeof(b.h_state));
		if (b.h_state.count == 0) return true;
		if (round > 4096) return false;
		big_levels = 4;
	}
}

// Tile mode: the tiles' nodes by k_collapse_tile beside the level-by-level collapse of the nodes above them (into the workspace),
// then k_top_finish moves those behind the tiles' nodes. Once more into an exact allocation if the estimate was too small.
// b.tiles_done stays false if there are more nodes above the tiles than the workspace holds: collapse_levels does everything then.
bool collapse_tiles(Build &b)
{
	Workspace &ws = *b.ws;
	const hipStream_t bs = b.bs;
	const uint32_t num_tiles = b.num_tiles;
	BuildResults *const results = b.results;
	DevSceneConsts *consts = const_cast<DevSceneConsts *>(b.ds->view.consts);
	uint32_t top_nodes = 0;
	for (int attempt = 0;; attempt++) {
		DevNode *d_nodes_ = (DevNode *)b.node_mem;
		DevNodeQ *d_qnodes_ = (DevNodeQ *)(d_nodes_ + b.node_cap);
		// the tiles' nodes, numbers 1 ... (0 is the root): beside the collapse of the nodes above them the first time
		const hipStream_t ts = attempt == 0 ? b.cs : bs;
		hipLaunchKernelGGL(k_collapse_tile, dim3(num_tiles), dim3(TILE_THREADS), 0, ts, b.d_tris, (int)b.n, b.d_lr, b.d_range, b.d_bin, b.d_area, b.d_root_list, b.d_tile_nroots, b.d_root_info,
			b.d_tile_base, 1u, d_nodes_, d_qnodes_, (uint32_t)b.node_cap, consts);
		if (hipGetLastError() != hipSuccess) return b.fail("tile collapse launch");
		if (attempt == 0) {
			if (b.forked && hipEventRecord(ws.join, ws.side) != hipSuccess) return b.fail("event record");
			// the nodes above the tiles (~4 per tile; ~15 tile roots per tile hang below them), into the workspace
			if (!run_collapse(b, b.d_nodes_tmp, b.top_cap, (uint64_t)num_tiles * 16u)) return b.fail("collapse");
			top_nodes = b.h_state.total_nodes;
			if (b.forked && hipStreamWaitEvent(bs, ws.join, 0) != hipSuccess) return b.fail("stream wait");
			if (top_nodes > b.top_cap) break;           // (more of them than the workspace holds: everything level by level)
		}
		hipLaunchKernelGGL(k_top_finish, dim3((top_nodes + 255u) / 256u), dim3(256), 0, bs, b.d_nodes_tmp, b.d_top_refs, b.d_top_level, top_nodes, b.d_tile_base + num_tiles, b.d_root_info,
			d_nodes_, d_qnodes_, (uint32_t)b.node_cap, consts, b.d_depth_word);
		hipLaunchKernelGGL(k_publish, dim3(1), dim3(1), 0, bs, results, b.d_tile_base + num_tiles, b.d_depth_word, consts);
		if (hipGetLastError() != hipSuccess || hipStreamSynchronize(bs) != hipSuccess) return b.fail("tile collapse");
		const uint32_t tile_nodes = results->tiles_total;      // wide nodes of all tiles
		b.depth = results->depth;
		b.equal_codes = results->equal_codes;
		b.ds->tree.consts_readback = results->consts;
#ifdef RTK_TILE_PHASES
		{
			unsigned long long h[8] = {}, z[8] = {};
			(void)hipMemcpyFromSymbol(h, HIP_SYMBOL(g_tile_phase), sizeof(h));
			(void)hipMemcpyToSymbol(HIP_SYMBOL(g_tile_phase), z, sizeof(z));
			if (h[4]) fprintf(stderr, "rtk_amd tile phases (10 ns ticks per tile): load %.0f bfs %.0f number %.0f finish %.0f; tiles %llu jobs/tile %.0f\n",
				(double)h[0] / h[4], (double)h[1] / h[4], (double)h[2] / h[4], (double)h[3] / h[4], h[4], (double)h[5] / h[4]);
			fprintf(stderr, "rtk_amd tile phases: slowest tile %llu ticks (tile %llu); slowest finish %llu ticks (%llu jobs)\n", h[6] >> 32, h[6] & 0xffffffffull, h[7] >> 32, h[7] & 0xffffffffull);
		}
#endif
		if (b.knobs.timing) {
			std::vector<uint32_t> hc(num_tiles + 1), hb(num_tiles + 1);
			(void)hipMemcpy(hc.data(), b.d_tile_count, (num_tiles) * 4, hipMemcpyDeviceToHost);
			(void)hipMemcpy(hb.data(), b.d_tile_base, (num_tiles + 1) * 4, hipMemcpyDeviceToHost);
			fprintf(stderr, "rtk_amd build: top %u tiles %u tail %u depth %u cap %zu counts %u %u %u bases %u %u %u\n", top_nodes, num_tiles, tile_nodes, b.depth, b.node_cap,
				hc[0], hc[1], hc[num_tiles - 1], hb[0], hb[1], hb[num_tiles]);
		}
		b.total_nodes = top_nodes + tile_nodes;
		if (b.total_nodes <= b.node_cap) {
			b.ds->view.nodes = d_nodes_;
			b.ds->view.qnodes = d_qnodes_;
			b.ds->view.num_nodes = b.total_nodes;
			b.ds->tree.first_top = 1u + tile_nodes;
			b.tiles_done = true;
			break;
		}
		if (attempt > 0) return b.fail("collapse (internal error: node count changed between two runs)");
		// the estimate was too small: an exact allocation, and the tiles and the move once more (the nodes above the tiles stay
		// where they are in the workspace; every pass is deterministic)
		b.node_cap = b.total_nodes;
		if (!b.node_alloc()) return b.fail("out of device memory");
		if (hipMemsetAsync(consts, 0, sizeof(DevSceneConsts), bs) != hipSuccess || hipMemsetAsync(b.d_depth_word, 0, 4, bs) != hipSuccess) return b.fail("memset");
	}
	if (b.tiles_done) b.stage("collapse");
	else {
		// (the other way needs the level-by-level kernels without their tile-mode arguments, and clean counters)
		b.top_aux = TopAux{ nullptr, nullptr };
		if (hipMemsetAsync(b.d_depth_word, 0, 4, bs) != hipSuccess) return b.fail("memset");
	}
	return true;
}

// Every node level by level, straight into the scene's node array; through the workspace and then into an exact allocation if
// the estimate was too small (or could not be had). The compressed nodes follow (rtk_quantize_nodes).
bool collapse_levels(Build &b)
{
	const hipStream_t bs = b.bs;
	bool in_place = b.node_mem != nullptr;
	if (!run_collapse(b, in_place ? (DevNode *)b.node_mem : b.d_nodes_tmp, in_place ? (uint32_t)b.node_cap : b.n, b.n)) return b.fail("collapse");
	if (in_place && b.h_state.total_nodes > b.node_cap) {
		// the estimate was too small: once more, into the workspace; then an exact allocation
		b.ds->mem.release(b.node_mem);
		b.node_mem = nullptr;
		in_place = false;
		if (!run_collapse(b, b.d_nodes_tmp, b.n, b.n)) return b.fail("collapse");
	}
	b.total_nodes = b.h_state.total_nodes;
	b.depth = b.h_state.depth;
	b.stage("collapse");
	if (!b.node_mem) {
		b.node_cap = b.total_nodes ? b.total_nodes : 1;
		if (!b.node_alloc()) return b.fail("out of device memory");
	}
	DevNode *d_nodes_ = (DevNode *)b.node_mem;
	b.ds->view.nodes = d_nodes_;
	b.ds->view.num_nodes = b.total_nodes;
	// compressed nodes beside the exact ones (and, if the collapse had to go through the workspace, the exact ones out of it)
	DevSceneConsts *consts = const_cast<DevSceneConsts *>(b.ds->view.consts);
	if (b.tile_mode && hipMemsetAsync(consts, 0, sizeof(DevSceneConsts), bs) != hipSuccess) return b.fail("memset");     // (the way back from tile mode: its kernels have counted in there)
	if (rtk_quantize_nodes(b.ds, bs, in_place ? nullptr : b.d_nodes_tmp, (DevNodeQ *)(d_nodes_ + b.node_cap), 0.0f, 0xffffffffu, true, false) != RTK_AMD_OK) return b.give_up();
	hipLaunchKernelGGL(k_publish, dim3(1), dim3(1), 0, bs, b.results, (const uint32_t *)nullptr, b.d_depth_word, consts);
	if (hipGetLastError() != hipSuccess) return b.fail("publish launch");
	return true;
}

// ---- finish: the one wait for both streams (the workspace is handed back when build_impl returns), the scene's view ----
bool finish(Build &b)
{
	rtk_dev_scene *ds = b.ds;
	if (hipStreamSynchronize(b.bs) != hipSuccess || (b.side_busy && hipStreamSynchronize(b.ws->side) != hipSuccess)) return b.fail("sync");
	if (!b.tiles_done) {
		b.equal_codes = b.results->equal_codes;
		ds->tree.consts_readback = b.results->consts;
	}
	rtk_quantize_finish(ds);
	ds->view.tris = b.d_tris;
	ds->view.vertex_index = ds->view.prim_slot = ds->view.slot_mesh = ds->view.slot_tri = nullptr;      // (the four side arrays: rtk_scene_side_arrays, on first use)
	ds->view.num_nodes = b.total_nodes;
	ds->view.num_tris = b.n;
	ds->view.num_prims = b.n;
	ds->tree.max_depth = b.depth;
	ds->tree.boxes_exact = true;               // (every box the union of what is below it: what a refit of some meshes relies on)
	b.stage("finish");
	ds->build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - b.t_begin).count();
	return true;
}

// Everything behind the planning of the source, for either ingest. force_bits: 0 = key width from the number of triangles; else
// the width of the Morton code in the packed sort words. *narrow_key: the build was made with fewer than 40 bits and more than an
// eighth of the sorted neighbours share their code. NULL: the build failed (b.rc says how), nothing is left allocated or enqueued.
rtk_dev_scene *run_stages(Build &b, uint32_t force_bits, bool *narrow_key)
{
	plan_build(b, force_bits);
	b.ws = &g_workspace[b.device];
	std::lock_guard<std::mutex> ws_lock(b.ws->mutex);      // held to the end: every exit below has waited for what it enqueued (Build::give_up, finish)
	if (!prepare_workspace(b) || !(b.from ? ingest_scene(b) : ingest(b)) || !keys_and_sort(b) || !emit(b) || !refit(b)) return nullptr;
	alloc_node_estimate(b);
	if (b.tile_mode && !collapse_tiles(b)) return nullptr;
	if (!b.tiles_done && !collapse_levels(b)) return nullptr;
	if (!finish(b)) return nullptr;

	*narrow_key = b.packed && b.packed_bits < 40u && (uint64_t)b.equal_codes * 8u > (uint64_t)b.n;
	if (b.knobs.timing) fprintf(stderr, "rtk_amd build: %u key bits, %u of %u sorted neighbours share a code%s\n", b.packed ? b.packed_bits : BUILD_KEY_BITS, b.equal_codes, b.n,
		*narrow_key ? " -> key too narrow for this scene" : "");
	if (!b.knobs.keep_workspace) {
		(void)hipFree(b.ws->base);
		b.ws->base = nullptr;
		b.ws->cap = 0;
	}
	return b.ds;
}

rtk_dev_scene *build_impl(const rtk_scene_desc *desc, const rtk_placement *placements, const BuildKnobs &knobs, uint32_t force_bits, bool *narrow_key)
{
	*narrow_key = false;
	if (!desc || (!desc->meshes && desc->num_meshes)) { rtk_set_error("rtk_dev_scene_build: NULL scene description"); return nullptr; }
	Build b;
	b.desc = desc;
	b.placements = placements;
	b.num_meshes = desc->num_meshes;
	b.knobs = knobs;
	b.mesh_base.assign(desc->num_meshes + 1, 0);
	for (size_t m = 0; m < desc->num_meshes; m++) b.mesh_base[m + 1] = b.mesh_base[m] + desc->meshes[m].num_triangles;
	const uint64_t n64 = b.mesh_base.back();
	if (n64 >= 0x3ffffff0ull) { rtk_set_error("rtk_dev_scene_build: more than 2^30 triangles"); return nullptr; }
	b.n = (uint32_t)n64;
	if (desc->log_fn) desc->log_fn(desc->log_user, nullptr, "rtk_amd: device LBVH build");
	b.t_begin = b.t_last = std::chrono::steady_clock::now();
	if (hipGetDevice(&b.device) != hipSuccess) { b.fail("hipGetDevice"); return nullptr; }
	if (b.device < 0 || b.device >= RTK_MAX_DEVICES) { rtk_set_error("rtk_dev_scene_build: device %d out of range", b.device); return nullptr; }
	b.num_cus = cached_cu_count(b.device);
	if (!plan_meshes(b)) return nullptr;
	if (b.n < 2) return build_tiny(desc, b.mesh_base, placements);
	return run_stages(b, force_bits, narrow_key);
}

// One build over the records of `from` (at least two, one per primitive as far as the host can tell), into a scene object of its
// own: `from` is read and not written. *key_bits: the width of the Morton code it sorted by.
rtk_dev_scene *rebuild_impl(const rtk_dev_scene *from, const BuildKnobs &knobs, uint32_t force_bits, bool *narrow_key, uint32_t *key_bits, int *rc)
{
	*narrow_key = false;
	Build b;
	b.from = from;
	b.num_meshes = from->mesh_base.empty() ? 0 : from->mesh_base.size() - 1;
	b.knobs = knobs;
	b.mesh_base = from->mesh_base;
	b.plans.assign(b.num_meshes, MeshPlan());              // (nothing is uploaded: the layout is asked with all-zero uploads)
	b.n = from->view.num_tris;
	b.t_begin = b.t_last = std::chrono::steady_clock::now();
	b.device = from->device;
	b.num_cus = cached_cu_count(b.device);
	rtk_dev_scene *ds = run_stages(b, force_bits, narrow_key);
	*key_bits = b.packed ? b.packed_bits : BUILD_KEY_BITS;
	*rc = ds ? RTK_AMD_OK : b.rc;
	return ds;
}

} // namespace

// The key width follows the NUMBER of triangles (ceil(log2 n) + 8 bits of the 63-bit code: four radix passes up to 2^24
// triangles), which assumes they are spread over the scene box. Where they are not -- a dense mesh in 1 % of the box --
// hundreds of triangles share a cell, their order inside it is the order of their numbers, and the SAH decisions of the refit
// cannot repair that topology. k_refit_tile counts the sorted neighbours with equal codes while it builds the
// tree; if more than an eighth of them are equal the scene is built once more with the full 40 bits: twice the time for such a
// scene, the same tree quality as before the narrow keys, nothing for scenes that do not need it.
// placements: NULL (rtk_dev_scene_build), or one per mesh (rtk_dev_scene_build_placed)
static rtk_dev_scene *build_with_key_rule(const rtk_scene_desc *desc, const rtk_placement *placements)
{
	const BuildKnobs knobs = read_build_knobs();
	bool narrow = false;
	rtk_dev_scene *ds = build_impl(desc, placements, knobs, 0u, &narrow);
	if (!ds || !narrow || !knobs.key_rebuild) return ds;
	const double first_ms = ds->build_ms;
	rtk_dev_scene_free(ds);
	ds = build_impl(desc, placements, knobs, 40u, &narrow);
	if (ds) ds->build_ms += first_ms;
	return ds;
}

extern "C" rtk_dev_scene *rtk_dev_scene_build(const rtk_scene_desc *desc)
{
	return build_with_key_rule(desc, nullptr);
}

// The same build over placed meshes (rtk_amd.h has the contract, DESIGN.md 3.4e the reasons): the placement is applied where a
// vertex is first read -- k_ingest, or the host's decode of an index_cb mesh and of a scene of fewer than two triangles -- and
// nothing behind the ingest knows of it.
extern "C" rtk_dev_scene *rtk_dev_scene_build_placed(const rtk_scene_desc *desc, const rtk_placement *placements)
{
	if (!placements) { rtk_set_error("rtk_dev_scene_build_placed: NULL placements"); return nullptr; }
	return build_with_key_rule(desc, placements);
}

// rtk_dev_scene_rebuild: the device builder's tree over the triangles a scene holds now, adopted by the live handle
// (rtk_amd.h has the contract, DESIGN.md 3.4d the reasons). The build runs as rtk_dev_scene_build runs it -- same knobs, same
// plan, same narrow-key rule -- from the scene's own records (ingest_scene) into a scene object of its own; the live scene is
// read until the build's last wait is over and written only by the swap below, which cannot fail.
extern "C" int rtk_dev_scene_rebuild(rtk_dev_scene *ds, rtk_dev_rebuild_info *out, void *stream)
{
	// ---- refused before HIP is touched
	if (!ds) { rtk_set_error("rtk_dev_scene_rebuild: NULL scene"); return RTK_AMD_ERR_BAD_ARG; }
	if (out && out->struct_size < sizeof(rtk_dev_rebuild_info)) {
		rtk_set_error("rtk_dev_scene_rebuild: struct_size %u, rtk_dev_rebuild_info has %zu bytes", out->struct_size, sizeof(rtk_dev_rebuild_info));
		return RTK_AMD_ERR_BAD_ARG;
	}
	ScenePass pass(ds, stream);                                    // never beside a refit, a measurement or a split
	rtk_dev_rebuild_info info = {};
	info.struct_size = out ? out->struct_size : (uint32_t)sizeof(info);
	info.nodes_before = info.nodes_after = ds->view.num_nodes;
	info.max_depth_before = info.max_depth_after = ds->tree.max_depth;
	if (ds->view.num_tris != ds->view.num_prims) {
		rtk_set_error("rtk_dev_scene_rebuild: %u triangle records for %u primitives", ds->view.num_tris, ds->view.num_prims);
		return RTK_AMD_ERR_UNSUPPORTED;
	}
	if (ds->view.num_tris >= 0x3ffffff0u) { rtk_set_error("rtk_dev_scene_rebuild: more than 2^30 triangles"); return RTK_AMD_ERR_UNSUPPORTED; }
	if (ds->view.num_tris < 2u) { if (out) *out = info; return RTK_AMD_OK; }      // (a tree of one node: there is nothing to build better)
	if (!pass.on_device()) return RTK_AMD_ERR_NO_DEVICE;
	// the build runs on a stream of its own: what the caller queued on `stream` (a refit's kernels, say) is over first
	RTK_PASS_CHECK("rtk_dev_scene_rebuild", hipStreamSynchronize(pass.stream));
	const BuildKnobs knobs = read_build_knobs();
	bool narrow = false;
	int rc = RTK_AMD_OK;
	const auto t_build = std::chrono::steady_clock::now();
	rtk_dev_scene *ns = rebuild_impl(ds, knobs, 0u, &narrow, &info.key_bits, &rc);
	if (ns && narrow && knobs.key_rebuild) {
		rtk_dev_scene_free(ns);
		ns = rebuild_impl(ds, knobs, 40u, &narrow, &info.key_bits, &rc);
	}
	if (!ns) return pass.end(rc);
	const auto t_swap = std::chrono::steady_clock::now();

	// ---- the swap: host work only, after the build's last wait. The old arrays go, the new scene's allocations change ledgers.
	{
		std::lock_guard<std::mutex> side_lock(ds->side_mutex);
		std::lock_guard<std::mutex> scratch_lock(ds->scratch_mutex);      // (the trace path reads these fields under it)
		rtk_scene_forget_derived(ds, RTK_FORGET_TREE | RTK_FORGET_SLOTS);
		ds->mem.release(ds->view.nodes);               // (an upload owns its arrays one by one, a device build its compressed nodes
		ds->mem.release(ds->tree.qnodes_mem);          // behind the exact ones and its mesh table behind the records: no entries of their own)
		ds->mem.release(ds->view.tris);
		ds->mem.release(ds->view.consts);
		ds->mem.adopt_all(ns->mem);
		// view and record as wholes (SceneTree's rule, rtk_dev.h): a fresh build's first_split is 0, its boxes are exact, its side
		// arrays are not made -- as RTK_FORGET_SLOTS has just left this scene's
		ds->view = ns->view;
		ds->tree = ns->tree;
		ds->quality.refitted = false;                  // the one deviation: a new tree, never refitted, so the next measurement is its cost at build
	}
	rtk_dev_scene_free(ns);                            // (the shell: its ledger is empty, it never had launch scratch)
	info.nodes_after = ds->view.num_nodes;
	info.max_depth_after = ds->tree.max_depth;
	info.rebuild_ms = pass.ms();
	if (knobs.timing) fprintf(stderr, "rtk_amd rebuild: wait for the stream %.3f ms, build %.3f ms, swap (the old arrays released) %.3f ms\n",
		std::chrono::duration<double, std::milli>(t_build - pass.t_begin).count(), std::chrono::duration<double, std::milli>(t_swap - t_build).count(),
		std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_swap).count());
	if (out) *out = info;
	return RTK_AMD_OK;
}

// The four side arrays of a device-built scene, made when something first needs them (the expansion of hit records into rtk_hit,
// rtk_trace_ray's one-ray kernel, the validator, the exporter). One kernel over the triangle records; the calling thread waits
// for it that one time, so that launches on any other stream may use the arrays as soon as this returns.
int rtk_scene_side_arrays(const rtk_dev_scene *ds_c, hipStream_t stream)
{
	rtk_dev_scene *ds = const_cast<rtk_dev_scene *>(ds_c);
	if (!ds) return RTK_AMD_ERR_BAD_ARG;
	std::lock_guard<std::mutex> lock(ds->side_mutex);
	if (ds->side_ready) return RTK_AMD_OK;
	const size_t n = ds->view.num_tris, np = ds->view.num_prims;
	Carve c;
	const size_t o_vidx = c.take(3 * n * 4), o_pslot = c.take(np * 4), o_smesh = c.take(n * 4), o_stri = c.take(n * 4);
	char *base = (char *)ds->mem.own(c.bytes, c.bytes);
	if (!base) { rtk_set_error("rtk_scene_side_arrays: %s", hipGetErrorString(hipGetLastError())); return RTK_AMD_ERR_OOM; }
	uint32_t *vertex_index = (uint32_t *)(base + o_vidx), *prim_slot = (uint32_t *)(base + o_pslot), *slot_mesh = (uint32_t *)(base + o_smesh), *slot_tri = (uint32_t *)(base + o_stri);
	if (n) {
		hipLaunchKernelGGL(k_side_arrays, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, ds->view.tris, (uint32_t)n, ds->tree.d_mesh_base, ds->tree.d_vidx_in,
			vertex_index, prim_slot, slot_mesh, slot_tri);
		if (hipGetLastError() != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) {
			rtk_set_error("rtk_scene_side_arrays: %s", hipGetErrorString(hipGetLastError()));
			ds->mem.release(base);
			return RTK_AMD_ERR_HIP;
		}
	}
	ds->view.vertex_index = vertex_index;
	ds->view.prim_slot = prim_slot;
	ds->view.slot_mesh = slot_mesh;
	ds->view.slot_tri = slot_tri;
	ds->side_ready = true;
	return RTK_AMD_OK;
}

// =====================================================================================
// rtk.h build API (reference rtk.h:119-127) on top of the device build
// =====================================================================================
//
// The reference hands the caller a graph of CPU tasks to schedule (rtk.c:1362-1507). Here the
// parallelism is inside the GPU, so the graph has exactly one task: running it performs the
// whole device build. Callers that loop "while tasks remain: rtk_run_task" work unchanged.

// -- the CPU task-graph builder (rtk_cpu_build.cpp), selected explicitly by the host --
struct rtk_cpu_build;
void rtk_cpu_task_start(const rtk_task *, rtk_task_ctx *);
rtk_cpu_build *rtk_cpu_build_start(const rtk_scene_desc *desc, void *owner, rtk_task *first_task, rtk_task_fn *runner);
size_t rtk_cpu_build_run(rtk_cpu_build *b, const rtk_task *task, bool start, rtk_task *queue, size_t queue_size);
bool rtk_cpu_build_done(const rtk_cpu_build *b);
size_t rtk_cpu_build_size(rtk_cpu_build *b);
bool rtk_cpu_build_write(rtk_cpu_build *b, void *buffer, size_t size);
void rtk_cpu_build_free(rtk_cpu_build *b);

struct rtk_build {
	rtk_scene_desc desc;
	rtk_dev_scene *scene;      // device builder: the built scene
	bool done;
	rtk_cpu_build *cpu;        // CPU task-graph builder, or NULL
};

static std::atomic<int> g_builder{ -1 };

extern "C" int rtk_amd_set_builder(int builder)
{
	if (builder != RTK_AMD_BUILDER_DEVICE && builder != RTK_AMD_BUILDER_CPU_TASKS) { rtk_set_error("rtk_amd_set_builder: unknown builder %d", builder); return RTK_AMD_ERR_BAD_ARG; }
	g_builder.store(builder);
	return RTK_AMD_OK;
}

extern "C" int rtk_amd_get_builder(void)
{
	int b = g_builder.load();
	if (b < 0) {
		const char *e = getenv("RTK_AMD_BUILDER");
		b = (e && (!strcmp(e, "cpu") || !strcmp(e, "cpu-tasks"))) ? RTK_AMD_BUILDER_CPU_TASKS : RTK_AMD_BUILDER_DEVICE;
		g_builder.store(b);
	}
	return b;
}

static void build_task_fn(const rtk_task *task, rtk_task_ctx *)
{
	rtk_build *b = task->build;
	if (b->done) return;
	b->scene = rtk_dev_scene_build(&b->desc);
	b->done = true;
}

extern "C" rtk_build *rtk_start_build(const rtk_scene_desc *desc, rtk_task *first_task)
{
	if (!desc) { rtk_set_error("rtk_start_build: NULL description"); return nullptr; }
	rtk_build *b = new rtk_build();
	b->desc = *desc;              // by value; meshes stay borrowed (rtk.c:1661)
	b->scene = nullptr;
	b->done = false;
	b->cpu = nullptr;
	if (rtk_amd_get_builder() == RTK_AMD_BUILDER_CPU_TASKS) {
		// the reference's caller-scheduled task graph (rtk.c:1362-1507)
		rtk_task first;
		memset(&first, 0, sizeof(first));
		b->cpu = rtk_cpu_build_start(desc, b, first_task ? first_task : &first, nullptr);
		if (!b->cpu) { delete b; return nullptr; }
		if (!first_task) {
			// the inline path the reference leaves as a TODO (rtk.c:1682-1688, B8): a serial scheduler
			std::vector<rtk_task> queue(1, first), spawned(256);
			while (!queue.empty()) {
				const rtk_task t = queue.back();
				queue.pop_back();
				const size_t n = rtk_run_task(&t, spawned.data(), spawned.size());
				queue.insert(queue.end(), spawned.begin(), spawned.begin() + n);
			}
			if (!rtk_cpu_build_done(b->cpu)) { rtk_set_error("rtk_start_build: task graph did not complete"); rtk_cpu_build_free(b->cpu); delete b; return nullptr; }
		}
		return b;
	}
	if (first_task) {
		first_task->build = b;    // rtk.c:1679-1681
		first_task->fn = &build_task_fn;
		first_task->cost = 0.0;
		first_task->index = 0;
		first_task->arg = 0;
	} else {
		rtk_task t;
		memset(&t, 0, sizeof(t));
		t.build = b;
		t.fn = &build_task_fn;
		build_task_fn(&t, nullptr);   // the inline path the reference leaves as a TODO (rtk.c:1682-1688, B8)
		if (!b->scene) { delete b; return nullptr; }
	}
	return b;
}

extern "C" size_t rtk_run_task(const rtk_task *task, rtk_task *queue, size_t queue_size)
{
	if (!task || !task->fn) return 0;
	if (task->build && task->build->cpu)
		return rtk_cpu_build_run(task->build->cpu, task, task->fn == &rtk_cpu_task_start, queue, queue ? queue_size : 0);
	task->fn(task, nullptr);      // device builder: one task does the whole build, nothing follows
	return 0;
}

extern "C" size_t rtk_get_build_size(const rtk_build *build)
{
	if (build && build->cpu) return rtk_cpu_build_size(build->cpu);
	if (!build || !build->scene) { rtk_set_error("rtk_get_build_size: build has not run (or failed)"); return 0; }
	return rtk_dev_scene_export_size(build->scene);
}

extern "C" rtk_scene *rtk_finish_build_to(rtk_build *build, void *buffer, size_t size)
{
	if (build && build->cpu) {
		if (!buffer || !rtk_cpu_build_write(build->cpu, buffer, size)) return nullptr;      // too small: the build stays alive (rtk.c:1735)
		rtk_cpu_build_free(build->cpu);
		delete build;                                                                        // rtk.c:1771
		rtk_amd_forget_scene((rtk_scene *)buffer);      // whatever blob lived at this address before has no device copy any more
		return (rtk_scene *)buffer;
	}
	if (!build || !build->scene || !buffer) { rtk_set_error("rtk_finish_build_to: build has not run (or failed)"); return nullptr; }
	const size_t need = rtk_dev_scene_export_size(build->scene);
	if (need == 0 || size < need) return nullptr;             // build stays alive (rtk.c:1735)
	rtk_scene *s = rtk_dev_scene_export(build->scene, buffer, size);
	if (!s) return nullptr;
	rtk_cache_adopt(s, build->scene);                         // the device copy stays resident for rtk_trace_rays
	delete build;                                             // rtk.c:1771
	return s;
}

extern "C" rtk_scene *rtk_finish_build(rtk_build *build)
{
	if (!build) return nullptr;
	const size_t need = rtk_get_build_size(build);
	void *buffer = need ? aligned_alloc(128, (need + 127) & ~(size_t)127) : nullptr;
	if (!buffer) {                                            // rtk.c:1779-1783: free the build, return NULL
		if (build->scene) rtk_dev_scene_free(build->scene);
		if (build->cpu) rtk_cpu_build_free(build->cpu);
		delete build;
		return nullptr;
	}
	rtk_dev_scene *scene = build->scene;
	rtk_cpu_build *cpu = build->cpu;
	rtk_scene *s = rtk_finish_build_to(build, buffer, need);
	if (!s) { free(buffer); if (scene) rtk_dev_scene_free(scene); if (cpu) rtk_cpu_build_free(cpu); delete build; }
	return s;
}

extern "C" rtk_scene *rtk_build_scene(const rtk_scene_desc *desc)
{
	rtk_build *b = rtk_start_build(desc, nullptr);            // rtk.c:1788-1792
	return b ? rtk_finish_build(b) : nullptr;
}

extern "C" void rtk_free_scene(rtk_scene *scene)
{
	if (!scene) return;
	rtk_amd_forget_scene(scene);                              // drops the resident device copy
	free(scene);                                              // rtk.c:1794-1797
}
