// rtk_select.hip -- rtk_dev_select_rays: the list of the rays whose hit record (or occlusion byte) matches, made on the device
// from a trace's output, in input order, with its length beside it -- what the listed traces (rtk_dev_trace_rays*_listed) take.
//
// A stable stream compaction of fixed shape: count, scan, scatter. A decoupled look-back (one pass, every workgroup waiting for
// its predecessor's running sum) cost 40 us per tile on this machine for its memory-side atomics on one word;
// like the builder's level scans this one is count-then-scan, with no atomic and no host read anywhere:
//   k_select_count    one workgroup per SELECT_BLOCK_ITEMS entries of the input list: the keep flag of every entry, one ballot per
//                     wave -> one 64-bit mask per 64 entries (all the later kernels need of the source: ONE BIT per entry instead
//                     of its 16-byte record a second time), their popcounts summed -> one count per workgroup;
//   k_select_scan     one workgroup per SELECT_SCAN_COUNTS counts: exclusive scan in LDS, written over the counts, the sum of the
//                     group beside it (a list of up to SELECT_SCAN_ITEMS entries is one group: the sum is the list's length);
//   k_select_top      more than one group (at most 4096 of them below 2^32 entries): one workgroup scans the groups' sums;
//   k_select_scatter  one workgroup per SELECT_BLOCK_ITEMS entries again: where its kept entries begin = group base + its scanned
//                     count; inside it the masks' popcounts (a scan of 16 numbers in LDS) and mbcnt of the entry's own mask.
// The number of entries, min(*in->d_count, num_rays), is known on the device only: the grids are sized by num_rays and an entry
// beyond the list counts as not kept.
// Reads 16 B (records) or 1 B (bytes) per entry once, and with an input list its 8-byte ids twice; writes 8 bytes per kept entry.
// Lanes of a wave take consecutive entries, so that a wave reads 1 KB of consecutive records or 512 B of consecutive ids and
// writes its kept ids to consecutive words.
#include "rtk_dev.h"

#include <mutex>

#define SELECT_THREADS 256u
#define SELECT_CHUNKS 16u                                    // 64-entry chunks per workgroup: four per wave
#define SELECT_BLOCK_ITEMS (64u * SELECT_CHUNKS)             // 1024 entries per workgroup of the count and scatter kernels
#define SELECT_SCAN_PER_THREAD 4u
#define SELECT_SCAN_COUNTS (SELECT_THREADS * SELECT_SCAN_PER_THREAD)   // 1024 workgroup counts per workgroup of the scan level ...
#define SELECT_SCAN_ITEMS (SELECT_SCAN_COUNTS * SELECT_BLOCK_ITEMS)    // ... which is 2^20 entries
#define SELECT_TOP_PER_THREAD 16u                            // 256 x 16 = 4096 groups: 2^32 entries

namespace {

struct SelectParams {
	const void *src;               // rtk_hit_record[num_rays] or uint8_t[num_rays]
	const uint64_t *in_ids;        // or NULL: 0, 1, 2, ...
	const uint64_t *in_count;      // or NULL: num_rays
	uint64_t *out_ids;
	uint64_t *out_count;
	unsigned long long *masks;     // [blocks * SELECT_CHUNKS] keep flags of 64 entries each
	uint32_t *counts;              // [blocks] kept entries per workgroup; after the scan: kept entries before it in its group
	uint32_t *groups;              // [groups] kept entries per group; after the top scan: kept entries before it
	uint32_t num_rays;
	uint32_t blocks;
	uint32_t num_groups;
	uint32_t kind;
};

__device__ __forceinline__ uint32_t list_length(const SelectParams &p)
{
	if (!p.in_count) return p.num_rays;
	const unsigned long long c = *p.in_count;
	return c < p.num_rays ? (uint32_t)c : p.num_rays;
}

// inclusive scan of one number per thread over the workgroup (256 threads), in LDS; s[255] is the sum afterwards
__device__ __forceinline__ uint32_t block_scan_inclusive(uint32_t v, uint32_t *s)
{
	const uint32_t t = threadIdx.x;
	s[t] = v;
	__syncthreads();
	for (uint32_t d = 1u; d < SELECT_THREADS; d <<= 1) {
		const uint32_t add = t >= d ? s[t - d] : 0u;
		__syncthreads();
		s[t] += add;
		__syncthreads();
	}
	return s[t];
}

__global__ void __launch_bounds__(SELECT_THREADS) k_select_count(SelectParams p)
{
	__shared__ uint32_t s_pop[SELECT_CHUNKS];
	const uint32_t m = list_length(p);
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const bool want = (p.kind & 1u) == 0u;                    // HIT / NONZERO
	for (uint32_t k = 0; k < SELECT_CHUNKS / 4u; k++) {
		const uint32_t chunk = k * 4u + wave;
		const unsigned long long i = (unsigned long long)blockIdx.x * SELECT_BLOCK_ITEMS + chunk * 64u + lane;
		bool keep = false;
		if (i < m) {
			const uint32_t r = p.in_ids ? (uint32_t)p.in_ids[i] : (uint32_t)i;
			if (r < p.num_rays) {
				const bool set = p.kind < 2u ? reinterpret_cast<const rtk_hit_record *>(p.src)[r].prim != RTK_PRIM_NONE
					: reinterpret_cast<const uint8_t *>(p.src)[r] != 0;
				keep = set == want;
			}
		}
		const unsigned long long mask = __builtin_amdgcn_ballot_w64(keep);
		if (lane == 0) {
			p.masks[(size_t)blockIdx.x * SELECT_CHUNKS + chunk] = mask;
			s_pop[chunk] = (uint32_t)__popcll(mask);
		}
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		uint32_t sum = 0;
		for (uint32_t c = 0; c < SELECT_CHUNKS; c++) sum += s_pop[c];
		p.counts[blockIdx.x] = sum;
	}
}

__global__ void __launch_bounds__(SELECT_THREADS) k_select_scan(SelectParams p)
{
	__shared__ uint32_t s_scan[SELECT_THREADS];
	const uint32_t first = blockIdx.x * SELECT_SCAN_COUNTS + threadIdx.x * SELECT_SCAN_PER_THREAD;
	uint32_t c[SELECT_SCAN_PER_THREAD], mine = 0;
	for (uint32_t j = 0; j < SELECT_SCAN_PER_THREAD; j++) {
		c[j] = first + j < p.blocks ? p.counts[first + j] : 0u;
		mine += c[j];
	}
	uint32_t before = block_scan_inclusive(mine, s_scan) - mine;
	for (uint32_t j = 0; j < SELECT_SCAN_PER_THREAD; j++) {
		if (first + j < p.blocks) p.counts[first + j] = before;
		before += c[j];
	}
	if (threadIdx.x == SELECT_THREADS - 1u) {
		if (p.num_groups == 1u) { p.groups[0] = 0u; *p.out_count = before; }      // (one group: its sum is the answer, no top level)
		else p.groups[blockIdx.x] = before;
	}
}

__global__ void __launch_bounds__(SELECT_THREADS) k_select_top(SelectParams p)
{
	__shared__ uint32_t s_scan[SELECT_THREADS];
	const uint32_t first = threadIdx.x * SELECT_TOP_PER_THREAD;
	uint32_t c[SELECT_TOP_PER_THREAD], mine = 0;
	for (uint32_t j = 0; j < SELECT_TOP_PER_THREAD; j++) {
		c[j] = first + j < p.num_groups ? p.groups[first + j] : 0u;
		mine += c[j];
	}
	uint32_t before = block_scan_inclusive(mine, s_scan) - mine;
	for (uint32_t j = 0; j < SELECT_TOP_PER_THREAD; j++) {
		if (first + j < p.num_groups) p.groups[first + j] = before;
		before += c[j];
	}
	if (threadIdx.x == SELECT_THREADS - 1u) *p.out_count = before;
}

__global__ void __launch_bounds__(SELECT_THREADS) k_select_scatter(SelectParams p)
{
	__shared__ uint32_t s_before[SELECT_CHUNKS];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const unsigned long long *masks = p.masks + (size_t)blockIdx.x * SELECT_CHUNKS;
	if (threadIdx.x == 0) {
		uint32_t sum = 0;
		for (uint32_t c = 0; c < SELECT_CHUNKS; c++) { s_before[c] = sum; sum += (uint32_t)__popcll(masks[c]); }
	}
	__syncthreads();
	const uint32_t base = p.groups[blockIdx.x / SELECT_SCAN_COUNTS] + p.counts[blockIdx.x];
	for (uint32_t k = 0; k < SELECT_CHUNKS / 4u; k++) {
		const uint32_t chunk = k * 4u + wave;
		const unsigned long long mask = masks[chunk];
		if (!((mask >> lane) & 1ull)) continue;
		// (a kept entry lies inside the list and the arrays: k_select_count looked)
		const unsigned long long i = (unsigned long long)blockIdx.x * SELECT_BLOCK_ITEMS + chunk * 64u + lane;
		const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
		p.out_ids[(size_t)base + s_before[chunk] + rank] = p.in_ids ? (uint64_t)(uint32_t)p.in_ids[i] : (uint64_t)i;
	}
}

} // namespace

extern "C" uint32_t rtk_amd_select_block_items(void) { return SELECT_BLOCK_ITEMS; }
extern "C" uint32_t rtk_amd_select_scan_items(void) { return SELECT_SCAN_ITEMS; }

int rtk_launch_select(rtk_dev_scene *ds, const void *d_src, uint32_t kind, size_t num_rays, const rtk_ray_list *in, uint64_t *d_out_ids,
	uint64_t *d_out_count, hipStream_t stream)
{
	if (!ds || !d_out_count || (num_rays && (!d_src || !d_out_ids))) { rtk_set_error("rtk_dev_select_rays: NULL scene, source or output"); return RTK_AMD_ERR_BAD_ARG; }
	if (kind > RTK_SELECT_BYTE_ZERO) { rtk_set_error("rtk_dev_select_rays: unknown kind %u", kind); return RTK_AMD_ERR_BAD_ARG; }
	if (in && (in->struct_size < sizeof(rtk_ray_list) || in->flags != 0u || !in->d_count)) {
		rtk_set_error("rtk_dev_select_rays: bad input list (struct_size %u, flags %#x, d_count %p)", in->struct_size, in->flags, (const void *)in->d_count);
		return RTK_AMD_ERR_BAD_ARG;
	}
	if (num_rays >= ((size_t)1 << 32)) { rtk_set_error("rtk_dev_select_rays: %zu rays: a list holds fewer than 2^32", num_rays); return RTK_AMD_ERR_BAD_ARG; }
	if (!rtk_on_scene_device(ds, "rtk_dev_select_rays")) return RTK_AMD_ERR_BAD_ARG;
	if (num_rays == 0) {
		RTK_HIP_CHECK(hipMemsetAsync(d_out_count, 0, sizeof(uint64_t), stream), RTK_AMD_ERR_HIP);
		return RTK_AMD_OK;
	}
	SelectParams p = {};
	p.src = d_src;
	p.in_ids = in ? in->d_ids : nullptr;
	p.in_count = in ? in->d_count : nullptr;
	p.out_ids = d_out_ids;
	p.out_count = d_out_count;
	p.num_rays = (uint32_t)num_rays;
	p.blocks = (uint32_t)((num_rays + SELECT_BLOCK_ITEMS - 1u) / SELECT_BLOCK_ITEMS);
	p.num_groups = (p.blocks + SELECT_SCAN_COUNTS - 1u) / SELECT_SCAN_COUNTS;
	p.kind = kind;
	const size_t mask_bytes = (size_t)p.blocks * SELECT_CHUNKS * sizeof(unsigned long long);
	const size_t bytes = mask_bytes + ((size_t)p.blocks + p.num_groups) * sizeof(uint32_t);

	// the scratch set of (scene, stream), held until everything is enqueued (rtk_launch_trace does the same)
	std::lock_guard<std::mutex> lock(ds->scratch_mutex);
	LaunchScratch *sc = ds->scratch.get(stream);
	if (!sc) return RTK_AMD_ERR_OOM;
	const int rc = sc->grow(sc->select, bytes, bytes);
	if (rc != RTK_AMD_OK) return rc;
	p.masks = sc->select.as<unsigned long long>();
	p.counts = reinterpret_cast<uint32_t *>(sc->select.as<char>() + mask_bytes);
	p.groups = p.counts + p.blocks;
	hipLaunchKernelGGL(k_select_count, dim3(p.blocks), dim3(SELECT_THREADS), 0, stream, p);
	hipLaunchKernelGGL(k_select_scan, dim3(p.num_groups), dim3(SELECT_THREADS), 0, stream, p);
	if (p.num_groups > 1u) hipLaunchKernelGGL(k_select_top, dim3(1), dim3(SELECT_THREADS), 0, stream, p);
	hipLaunchKernelGGL(k_select_scatter, dim3(p.blocks), dim3(SELECT_THREADS), 0, stream, p);
	RTK_HIP_CHECK(hipGetLastError(), RTK_AMD_ERR_HIP);
	return RTK_AMD_OK;
}
