// rtk_sort.hip -- the LSD radix sort the device build, the refit and the ray reordering share (gfx950): 64-bit keys with or
// without 32-bit values, 8-bit digits, per-wave LDS histograms and counters. Asynchronous: no allocation, no synchronisation.
#include "rtk_dev.h"

#include <stdlib.h>

#include <algorithm>

namespace {

#define SORT_TILE 4096u           // keys handled by one workgroup per pass (4 waves x 16 chunks of 64)
#define SORT_BLOCK 256

// ---------------------------------------------------------------------------------- 4 radix sort
// Unit of work = one workgroup = SORT_TILE consecutive keys (4 waves x 1024). hist is digit-major:
// hist[digit * num_units + unit], so one exclusive scan over the whole array yields, for
// every (digit, unit), the first output position of that unit's keys with that digit.

__global__ void __launch_bounds__(SORT_BLOCK) k_sort_hist(const unsigned long long *keys, uint32_t n, uint32_t shift,
	uint32_t num_units, uint32_t *hist)
{
	__shared__ uint32_t s_h[256];
	const uint32_t unit = blockIdx.x;
	s_h[threadIdx.x] = 0;
	__syncthreads();
	const size_t base = (size_t)unit * SORT_TILE;
	for (uint32_t c = 0; c < SORT_TILE / SORT_BLOCK; c++) {
		const size_t i = base + (size_t)c * SORT_BLOCK + threadIdx.x;     // coalesced 2 KB per step
		if (i < n) atomicAdd(&s_h[(uint32_t)(keys[i] >> shift) & 255u], 1u);
	}
	__syncthreads();
	hist[(size_t)threadIdx.x * num_units + unit] = s_h[threadIdx.x];
}

// exclusive scan of a uint32 array, three launches (block sums -> scan of sums -> add)
#define SCAN_BLOCK 256
#define SCAN_ITEMS 16             // per thread -> 4096 per block

__global__ void __launch_bounds__(SCAN_BLOCK) k_scan_block(uint32_t *data, size_t n, uint32_t *block_sums)
{
	__shared__ uint32_t s_wave[SCAN_BLOCK / 64];
	const size_t base = (size_t)blockIdx.x * (SCAN_BLOCK * SCAN_ITEMS) + (size_t)threadIdx.x * SCAN_ITEMS;
	uint32_t v[SCAN_ITEMS];
	uint32_t sum = 0;
#pragma unroll
	for (int k = 0; k < SCAN_ITEMS; k++) { v[k] = base + k < n ? data[base + k] : 0u; sum += v[k]; }
	// inclusive scan of `sum` across the wave
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint32_t inc = sum;
	for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(inc, o); if (lane >= (uint32_t)o) inc += t; }
	if (lane == 63u) s_wave[wave] = inc;
	__syncthreads();
	uint32_t wave_off = 0;
	for (uint32_t w = 0; w < wave; w++) wave_off += s_wave[w];
	uint32_t run = wave_off + inc - sum;
#pragma unroll
	for (int k = 0; k < SCAN_ITEMS; k++) { if (base + k < n) data[base + k] = run; run += v[k]; }
	if (threadIdx.x == SCAN_BLOCK - 1) block_sums[blockIdx.x] = run;
}

__global__ void __launch_bounds__(1024) k_scan_sums(uint32_t *sums, uint32_t n)
{
	// single block; n block sums, processed in strips of 1024 with a running carry
	__shared__ uint32_t s_wave[16];
	__shared__ uint32_t s_carry;
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	if (threadIdx.x == 0) s_carry = 0;
	__syncthreads();
	for (uint32_t base = 0; base < n; base += 1024u) {
		const uint32_t i = base + threadIdx.x;
		const uint32_t v = i < n ? sums[i] : 0u;
		uint32_t inc = v;
		for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(inc, o); if (lane >= (uint32_t)o) inc += t; }
		if (lane == 63u) s_wave[wave] = inc;
		__syncthreads();
		uint32_t off = s_carry;
		for (uint32_t w = 0; w < wave; w++) off += s_wave[w];
		if (i < n) sums[i] = off + inc - v;
		__syncthreads();
		if (threadIdx.x == 1023u) s_carry = off + inc;
		__syncthreads();
	}
}

__global__ void __launch_bounds__(SCAN_BLOCK) k_scan_add(uint32_t *data, size_t n, const uint32_t *block_sums)
{
	const uint32_t add = block_sums[blockIdx.x];
	const size_t base = (size_t)blockIdx.x * (SCAN_BLOCK * SCAN_ITEMS) + (size_t)threadIdx.x * SCAN_ITEMS;
#pragma unroll
	for (int k = 0; k < SCAN_ITEMS; k++) if (base + k < n) data[base + k] += add;
}

// Scatter pass with an LDS-staged tile. Each wave ranks its 1024 keys in order (16 chunks of 64;
// the rank of a key inside a chunk comes from 8 ballots, the running per-digit counts of the wave
// live in LDS), the four waves' counts are combined into tile-wide digit offsets, the (key, value)
// pairs are written to their SORTED position inside the tile in LDS, and the tile is then streamed
// out in that order: neighbouring threads hold neighbouring keys of the same digit, so the global
// stores form contiguous runs (16 keys on average for random digits) instead of one store per key.
// Stable: tile order = wave order = chunk order = lane order.
// VALS = false: the words carry their payload themselves (sorted field above, index below): no value arrays at all.
template <bool VALS>
__global__ void __launch_bounds__(SORT_BLOCK) k_sort_scatter(const unsigned long long *keys_in, const uint32_t *vals_in, uint32_t n,
	uint32_t shift, uint32_t num_units, const uint32_t *hist, unsigned long long *keys_out, uint32_t *vals_out,
	const uint32_t *scan_sums, uint32_t scan_blocks)
{
	// (LDS: 36.9 KB without values -- 16-bit counts, s_bp inside s_key -- so that four workgroups fit a CU with room to spare; with
	// 39.9 KB the four of them came to 159.8 of the CU's 160 KB. No measurable difference in the pass time either way.)
	__shared__ unsigned long long s_key[SORT_TILE];          // 32 KB
	uint32_t *const s_bp = reinterpret_cast<uint32_t *>(s_key);   // scan_sums != NULL: exclusive prefix of the scan blocks' totals; used before s_key is
	__shared__ uint32_t s_val[SORT_TILE];                    // 16 KB
	__shared__ uint16_t s_cnt[SORT_BLOCK / 64][256];         // per wave: running count (<= 1024), then prefix over earlier waves (<= 4096)
	__shared__ uint32_t s_start[256];                        // first tile position of each digit
	__shared__ uint32_t s_global[256];                       // first output position of this tile's keys of each digit
	__shared__ uint32_t s_wsum[SORT_BLOCK / 64];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const uint32_t unit = blockIdx.x;
	const size_t tile_base = (size_t)unit * SORT_TILE;
	const uint32_t tile_n = (uint32_t)((size_t)n - tile_base < SORT_TILE ? (size_t)n - tile_base : SORT_TILE);

	for (int j = 0; j < 4; j++) s_cnt[wave][lane + 64 * j] = 0;
	if (scan_sums) {
		// hist holds scans local to blocks of SCAN_BLOCK * SCAN_ITEMS entries (k_scan_block); the totals of the blocks
		// before an entry's block are added here (at most SORT_BLOCK of them) instead of by two more launches per pass
		const uint32_t v = threadIdx.x < scan_blocks ? scan_sums[threadIdx.x] : 0u;
		uint32_t inc = v;
		for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(inc, o); if (lane >= (uint32_t)o) inc += t; }
		if (lane == 63u) s_wsum[wave] = inc;
		__syncthreads();
		uint32_t off = 0;
		for (uint32_t w = 0; w < wave; w++) off += s_wsum[w];
		s_bp[threadIdx.x] = off + inc - v;
		__syncthreads();
		const size_t idx = (size_t)threadIdx.x * num_units + unit;
		s_global[threadIdx.x] = hist[idx] + s_bp[idx / ((size_t)SCAN_BLOCK * SCAN_ITEMS)];
	} else s_global[threadIdx.x] = hist[(size_t)threadIdx.x * num_units + unit];
	__syncthreads();

	// ---- phase 1: rank every key among the keys of its digit inside its wave
	constexpr uint32_t CHUNKS = SORT_TILE / SORT_BLOCK;      // 16 chunks of 64 keys per wave
	unsigned long long key[CHUNKS];
	uint32_t val[CHUNKS], rnk[CHUNKS];
	const unsigned long long lt_mask = lane == 0 ? 0ull : (~0ull >> (64u - lane));
	const size_t wave_base = tile_base + (size_t)wave * (SORT_TILE / (SORT_BLOCK / 64));
#pragma unroll
	for (uint32_t c = 0; c < CHUNKS; c++) {
		const size_t i = wave_base + (size_t)c * 64u + lane;
		const bool valid = i < n;
		key[c] = valid ? keys_in[i] : ~0ull;
		val[c] = (VALS && valid) ? vals_in[i] : 0u;
		const uint32_t d = (uint32_t)(key[c] >> shift) & 255u;
		unsigned long long same = __ballot(valid);
#pragma unroll
		for (int b = 0; b < 8; b++) {
			const bool bit = (d >> b) & 1u;
			const unsigned long long vote = __ballot(bit);
			same &= bit ? vote : ~vote;
		}
		rnk[c] = 0;
		if (valid) {
			const uint32_t r = (uint32_t)__popcll(same & lt_mask);
			const uint32_t before = s_cnt[wave][d];            // every lane reads before any leader writes (wave program order)
			rnk[c] = before + r;
			if (r == 0u) s_cnt[wave][d] = (uint16_t)(before + (uint32_t)__popcll(same));
		}
	}
	__syncthreads();

	// ---- phase 2: tile-wide digit offsets. Thread d owns digit d.
	{
		const uint32_t d = threadIdx.x;
		uint32_t run = 0;
		for (uint32_t w = 0; w < SORT_BLOCK / 64; w++) { const uint32_t c = s_cnt[w][d]; s_cnt[w][d] = (uint16_t)run; run += c; }
		// exclusive scan of the 256 digit totals
		uint32_t inc = run;
		for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(inc, o); if (lane >= (uint32_t)o) inc += t; }
		if (lane == 63u) s_wsum[wave] = inc;
		__syncthreads();
		uint32_t off = 0;
		for (uint32_t w = 0; w < wave; w++) off += s_wsum[w];
		s_start[d] = off + inc - run;
	}
	__syncthreads();

	// ---- phase 3: stage the tile in sorted order
#pragma unroll
	for (uint32_t c = 0; c < CHUNKS; c++) {
		const size_t i = wave_base + (size_t)c * 64u + lane;
		if (i < n) {
			const uint32_t d = (uint32_t)(key[c] >> shift) & 255u;
			const uint32_t pos = s_start[d] + s_cnt[wave][d] + rnk[c];
			s_key[pos] = key[c];
			if (VALS) s_val[pos] = val[c];
		}
	}
	__syncthreads();

	// ---- phase 4: stream the tile out; runs of one digit are contiguous in LDS and in HBM
	for (uint32_t i = threadIdx.x; i < tile_n; i += SORT_BLOCK) {
		const unsigned long long k = s_key[i];
		const uint32_t d = (uint32_t)(k >> shift) & 255u;
		const uint32_t dst = s_global[d] + (i - s_start[d]);
		keys_out[dst] = k;
		if (VALS) vals_out[dst] = s_val[i];
	}
}

} // namespace

// Asynchronous radix sort of (64-bit key, 32-bit value) pairs on `stream`, low `key_bits` bits only
// (rounded up to whole 8-bit passes). Ping-pongs between the a/b buffers; returns true if the result
// is in the b buffers. scratch: rtk_sort_scratch_words(n) uint32 words. No allocation, no sync.
size_t rtk_sort_scratch_words(uint32_t n)
{
	const size_t num_units = ((size_t)n + SORT_TILE - 1u) / SORT_TILE;
	const size_t hist = 256 * num_units;
	const size_t sums = (hist + (size_t)SCAN_BLOCK * SCAN_ITEMS - 1) / ((size_t)SCAN_BLOCK * SCAN_ITEMS);
	return hist + sums + 16;
}

// Bits [first_bit, last_bit) of the keys, 8 at a time, least significant digit first. vals_a == NULL: keys only.
static bool sort_async(unsigned long long *keys_a, unsigned long long *keys_b, uint32_t *vals_a, uint32_t *vals_b,
	uint32_t n, uint32_t first_bit, uint32_t last_bit, uint32_t *scratch, hipStream_t stream)
{
	const uint32_t num_units = (n + SORT_TILE - 1u) / SORT_TILE;
	const size_t hist_n = 256 * (size_t)num_units;
	uint32_t *hist = scratch, *sums = scratch + hist_n;
	const size_t scan_blocks = (hist_n + (size_t)SCAN_BLOCK * SCAN_ITEMS - 1) / ((size_t)SCAN_BLOCK * SCAN_ITEMS);
	unsigned long long *kin = keys_a, *kout = keys_b;
	uint32_t *vin = vals_a, *vout = vals_b;
	bool in_b = false;
	for (uint32_t shift = first_bit; shift < last_bit; shift += 8) {
		hipLaunchKernelGGL(k_sort_hist, dim3(num_units), dim3(SORT_BLOCK), 0, stream, kin, n, shift, num_units, hist);
		hipLaunchKernelGGL(k_scan_block, dim3((unsigned)scan_blocks), dim3(SCAN_BLOCK), 0, stream, hist, hist_n, sums);
		// up to 2^24 keys the scatter pass finishes the scan itself (three launches per pass instead of five)
		static const bool allow_fused = !(getenv("RTK_AMD_SORT_FUSED_SCAN") && atoi(getenv("RTK_AMD_SORT_FUSED_SCAN")) == 0);   // 0: test the large-n path on small scenes
		const uint32_t *fused_sums = (allow_fused && scan_blocks <= SORT_BLOCK) ? sums : nullptr;
		if (!fused_sums) {
			hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(1024), 0, stream, sums, (uint32_t)scan_blocks);
			hipLaunchKernelGGL(k_scan_add, dim3((unsigned)scan_blocks), dim3(SCAN_BLOCK), 0, stream, hist, hist_n, sums);
		}
		if (vals_a) hipLaunchKernelGGL((k_sort_scatter<true>), dim3(num_units), dim3(SORT_BLOCK), 0, stream, kin, vin, n, shift, num_units, hist, kout, vout,
			fused_sums, (uint32_t)scan_blocks);
		else hipLaunchKernelGGL((k_sort_scatter<false>), dim3(num_units), dim3(SORT_BLOCK), 0, stream, kin, (const uint32_t *)nullptr, n, shift, num_units, hist,
			kout, (uint32_t *)nullptr, fused_sums, (uint32_t)scan_blocks);
		std::swap(kin, kout);
		std::swap(vin, vout);
		in_b = !in_b;
	}
	return in_b;
}

bool rtk_sort_pairs_async(unsigned long long *keys_a, unsigned long long *keys_b, uint32_t *vals_a, uint32_t *vals_b,
	uint32_t n, uint32_t key_bits, uint32_t *scratch, hipStream_t stream)
{
	return sort_async(keys_a, keys_b, vals_a, vals_b, n, 0u, key_bits, scratch, stream);
}

// 64-bit words sorted by their bits [first_bit, last_bit); the bits below first_bit ride along (an index, a payload).
// Stable, so words that start out in index order stay in index order inside equal fields. True: the result is in keys_b.
bool rtk_sort_words_async(unsigned long long *keys_a, unsigned long long *keys_b, uint32_t n, uint32_t first_bit, uint32_t last_bit,
	uint32_t *scratch, hipStream_t stream)
{
	return sort_async(keys_a, keys_b, nullptr, nullptr, n, first_bit, last_bit, scratch, stream);
}
