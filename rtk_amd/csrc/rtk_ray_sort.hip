// rtk_ray_sort.hip -- the ray-reordering pre-pass of the per-lane kernels (RTK_TRACE_SORT_RAYS): 16-bit key = 4 bits of origin cell
// per axis inside the batch's origin bounds + direction octant; rays of one key start close together and head the same way,
// so the 64 rays a wave pulls from the sorted order share nodes (L1/L2 hits instead of fabric traffic).
// The key kernels, and rtk_ray_sort_launch: their only door.
#include "rtk_dev.h"
#include "rtk_trace_shared.h"

#include <math.h>

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

// *perm = the order to trace the rays in. sc->sort holds [words_a | words_b] 8 B each, bounds 6 words + sort scratch (rtk_ray_sort_bytes).
size_t rtk_ray_sort_bytes(size_t n) { return n * 16 + (rtk_sort_scratch_words((uint32_t)n) + 16) * 4; }

int rtk_ray_sort_launch(const rtk_dev_scene *ds, LaunchScratch *sc, const rtk_ray *d_rays, size_t n, const TraceKnobs &knobs, hipStream_t stream, const unsigned long long **perm)
{
	const uint32_t n32 = (uint32_t)n;
	unsigned long long *keys_a = sc->sort.as<unsigned long long>(), *keys_b = keys_a + sc->sort.capacity;
	uint32_t *bounds = (uint32_t *)(keys_b + sc->sort.capacity), *scratch = bounds + 16;
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
