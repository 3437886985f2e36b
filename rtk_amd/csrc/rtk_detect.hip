// rtk_detect.hip -- rtk_detect_image: is a batch of device rays a row-major image nobody told us about? The rule is
// rtk_detect_rule.h's (the host applies the same one to host rays, rtk_host_calls.hip); here are its two kernels and their launch.
#include "rtk_dev.h"
#include "rtk_detect_rule.h"

#include <mutex>

namespace {

// the first jump among the first `limit` rays, into *first_jump (RTK_DETECT_NO_JUMP before the launch)
__global__ void k_detect_row(const rtk_ray *rays, uint32_t limit, uint32_t *first_jump)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x + 1u;
	if (i + 1u >= limit) return;
	if (rtk_detect_step_jumps(rays, i)) atomicMin(first_jump, i);
}

// word[0] = first jump (set by k_detect_row). One workgroup, one look per thread;
// the verdict goes straight into host-visible memory (verdict[0] = width or 0, verdict[1] = height): no copy behind the kernel.
__global__ void __launch_bounds__(RTK_DETECT_ROWS) k_detect_check(const rtk_ray *rays, unsigned long long n, const uint32_t *word, uint32_t *verdict)
{
	__shared__ uint32_t s_bad;
	if (threadIdx.x == 0) s_bad = 0u;
	__syncthreads();
	RtkDetectCandidate c;
	const bool candidate = rtk_detect_candidate(word[0], n, &c);
	if (candidate && rtk_detect_row_bad(rays, c, threadIdx.x)) atomicAdd(&s_bad, 1u);
	__syncthreads();
	if (threadIdx.x == 0) {
		const bool ok = candidate && s_bad == 0u;
		verdict[0] = ok ? c.w : 0u;
		verdict[1] = ok ? (uint32_t)c.rows : 0u;
		__threadfence_system();
	}
}

} // namespace

// *w, *h = the image the batch is (row-major, w * h = n), or 0, 0. Two small launches and a wait for `stream`.
int rtk_detect_image(const rtk_dev_scene *ds_c, const rtk_ray *d_rays, size_t n, hipStream_t stream, uint32_t *w_out, uint32_t *h_out)
{
	rtk_dev_scene *ds = const_cast<rtk_dev_scene *>(ds_c);
	*w_out = *h_out = 0u;
	if (!ds || !d_rays || !rtk_detect_sized(n)) return RTK_AMD_OK;
	// (the look uses two words of the (scene, stream) scratch set and its pinned verdict: the scene's scratch mutex is held until the
	// verdict has been read, so that two host threads feeding one stream cannot interleave their looks; ~30 us)
	std::lock_guard<std::mutex> lock(ds->scratch_mutex);
	LaunchScratch *sc0 = ds->scratch.get(stream);
	if (!sc0) return RTK_AMD_ERR_OOM;
	uint32_t *d_word = reinterpret_cast<uint32_t *>(sc0->d_counter + RTK_DETECT_WORD);
	if (!sc0->h_verdict) RTK_HIP_CHECK(hipHostMalloc((void **)&sc0->h_verdict, 64, hipHostMallocDefault), RTK_AMD_ERR_OOM);     // (pinned: the kernel writes the verdict there)
	volatile uint32_t *h_verdict = sc0->h_verdict;
	const uint32_t limit = rtk_detect_limit(n);
	RTK_HIP_CHECK(hipMemsetAsync(d_word, 0xff, 4, stream), RTK_AMD_ERR_HIP);
	hipLaunchKernelGGL(k_detect_row, dim3((limit + 255u) / 256u), dim3(256), 0, stream, d_rays, limit, d_word);
	hipLaunchKernelGGL(k_detect_check, dim3(1), dim3(RTK_DETECT_ROWS), 0, stream, d_rays, (unsigned long long)n, d_word, const_cast<uint32_t *>(h_verdict));
	RTK_HIP_CHECK(hipGetLastError(), RTK_AMD_ERR_HIP);
	RTK_HIP_CHECK(hipStreamSynchronize(stream), RTK_AMD_ERR_HIP);
	*w_out = h_verdict[0];
	*h_out = h_verdict[1];
	return RTK_AMD_OK;
}
