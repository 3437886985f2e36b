// rtk_host_calls.hip -- the calls that take host pointers: rtk_trace_rays, rtk_trace_rays_filter and the two per-ray symbols of
// rtk.h, with what they keep between calls -- the residency cache (which device scene is the copy of which blob: the rule is
// rtk_residency.h's, the upload and its reasons to fail are here) and each thread's stream and staging memory. How a batch is
// cut into pieces, bands and rounds is rtk_host_pieces.h's; here is what a piece does on the GPU. No CPU fallback: every
// batch runs the HIP kernels behind rtk_launch.hip or fails with an error.
#include "rtk_dev.h"
#include "rtk_trace_plan.h"
#include "rtk_detect_rule.h"
#include "rtk_host_pieces.h"
#include "rtk_residency.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <chrono>

// ---------------------------------------------------------------------------- residency cache

namespace {

thread_local bool t_fatal = false;     // the last upload of this thread failed for good (invalid scene / no device)

int current_device()
{
	int d = 0;
	if (hipGetDevice(&d) != hipSuccess) { (void)hipGetLastError(); d = 0; }
	return d;
}

// what kind of failure a NULL is: a blob that does not validate or a machine without a usable GPU will fail the same
// way on every call ("fatal" for rtk_trace_ray, which has no error channel); running out of memory may not
rtk_dev_scene *upload_blob(const rtk_scene *scene)
{
	t_fatal = false;
	HostBvh h;
	if (rtk_blob_to_host_bvh(scene, (size_t)scene->size_in_bytes, &h) != RTK_AMD_OK) { t_fatal = true; return nullptr; }
	int count = 0;
	if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) { (void)hipGetLastError(); t_fatal = true; rtk_set_error("no usable HIP device"); return nullptr; }
	return rtk_dev_scene_from_host_bvh(h);
}

// (of static storage duration, and before the contexts below: it outlives every thread's HostCtx, the main thread's included)
Residency g_cache(upload_blob, rtk_dev_scene_free);

} // namespace

bool rtk_last_failure_is_fatal() { return t_fatal; }

void rtk_cache_adopt(const rtk_scene *scene, rtk_dev_scene *ds) { g_cache.adopt(scene, ds ? ds->device : current_device(), ds); }

extern "C" void rtk_amd_forget_scene(const rtk_scene *scene) { g_cache.forget(scene); }

// ---------------------------------------------------------------------------- host-pointer tracing
//
// Each host thread owns a stream, pinned staging memory and device buffers for one chunk of rays, all
// created on first use and kept: a call allocates nothing in steady state (the first version paid four
// hipMalloc + four hipFree per rtk_trace_ray). Batches larger than a chunk stream through in pieces.

namespace {

struct HostCtx {
	int device = -1;
	hipStream_t stream = nullptr;
	size_t cap = 0;                            // rays
	char *pinned = nullptr, *dev = nullptr;    // one allocation each, laid out alike: h and d
	Staging h, d;                              // h.status: the expand kernel of a zero-copy piece mirrors the launch-error word there
	bool status_mirrored = false;              // ... for the piece in flight
	uint32_t ticket = 0, ticket_in_flight = 0; // pieces of one workgroup (<= 256 rays) are waited for by polling h.status for their ticket
	char *cand_pinned = nullptr, *cand_dev = nullptr;   // candidate lists for host-callback filters, made by the first such call
	CandStaging hc, dc;

	void release()
	{
		if (pinned) (void)hipHostFree(pinned);
		if (dev) (void)hipFree(dev);
		if (cand_pinned) (void)hipHostFree(cand_pinned);
		if (cand_dev) (void)hipFree(cand_dev);
		pinned = dev = cand_pinned = cand_dev = nullptr;
		cap = 0;
	}
	// this thread's stream is going away: every cached scene drops the scratch set it made for it
	void drop_stream()
	{
		if (!stream) return;
		(void)hipStreamSynchronize(stream);
		g_cache.for_each([this](rtk_dev_scene *ds) { rtk_scene_drop_stream(ds, stream); });
		(void)hipStreamDestroy(stream);
		stream = nullptr;
	}
	~HostCtx() { release(); drop_stream(); }
	bool ensure(size_t n)
	{
		int cur = 0;
		if (hipGetDevice(&cur) != hipSuccess) { rtk_set_error("no usable HIP device: %s", hipGetErrorString(hipGetLastError())); return false; }
		if (cur != device) {                   // the thread moved to another GPU
			release();
			drop_stream();
			device = cur;
		}
		if (!stream && hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess) {
			rtk_set_error("hipStreamCreate failed: %s", hipGetErrorString(hipGetLastError()));
			stream = nullptr;
			return false;
		}
		if (n <= cap) return true;
		release();
		const size_t want = staging_capacity(n);
		if (hipHostMalloc((void **)&pinned, Staging::bytes(want), hipHostMallocDefault) != hipSuccess || hipMalloc((void **)&dev, Staging::bytes(want)) != hipSuccess) {
			rtk_set_error("rtk_trace_rays: staging allocation failed (%zu rays): %s", want, hipGetErrorString(hipGetLastError()));
			release();
			return false;
		}
		cap = want;
		h = Staging(pinned, want);
		d = Staging(dev, want);
		*h.status = 0ull;
		return true;
	}
	bool ensure_candidates()
	{
		if (cand_dev) return true;
		if ((!cand_pinned && hipHostMalloc((void **)&cand_pinned, CandStaging::bytes(), hipHostMallocDefault) != hipSuccess) || hipMalloc((void **)&cand_dev, CandStaging::bytes()) != hipSuccess) {
			rtk_set_error("rtk_trace_rays_filter: candidate buffers: %s", hipGetErrorString(hipGetLastError()));
			cand_dev = nullptr;                    // (a pinned half that was had is kept for the next try, or for release())
			return false;
		}
		hc = CandStaging(cand_pinned);
		dc = CandStaging(cand_dev);
		return true;
	}
};

thread_local HostCtx t_ctx;
thread_local HostCtx t_ctx2;                    // second staging set (own stream) for pipelined host-pointer batches

// A lone workgroup signs off with its ticket after its results (release store at system scope): poll for it -- a wait on the
// stream costs the runtime's wake-up latency on top. false: ~2 ms went by without it, the caller falls back to the stream.
bool wait_ticket(const unsigned long long *h_status, uint32_t ticket)
{
	const volatile unsigned long long *w = h_status;
	const auto t0 = std::chrono::steady_clock::now();
	for (uint32_t spin = 0;; spin++) {
		if ((uint32_t)(__atomic_load_n(w, __ATOMIC_ACQUIRE) >> 32) == ticket) return true;
		if ((spin & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) return false;
	}
}

// One piece (n <= chunk capacity), first half: rays up, trace (optionally restricted to candidates after h.after),
// expand, hits and mask on their way down -- everything enqueued on the context's stream, nothing waited for.
bool enqueue_piece(rtk_dev_scene *ds, HostCtx &c, const rtk_ray *rays, size_t n, bool want_hits, bool with_after, const rtk_trace_opts *opts = nullptr)
{
	memcpy(c.h.rays, rays, n * sizeof(rtk_ray));
	// Small pieces skip the copy engines altogether: the pinned staging memory is visible to the device, so the kernels
	// read the rays from it and write hits and mask into it over PCIe themselves -- two launches and one synchronisation
	// instead of those plus four copies (rtk_trace_ray: 74 us -> 50 us; 34 us with the status word and the ticket below, profiles/r02_single_ray_latency.log).
	const bool zero_copy = n <= ZERO_COPY_RAYS && !with_after;
	const rtk_ray *d_rays = zero_copy ? c.h.rays : c.d.rays;
	if (!zero_copy && hipMemcpyAsync(c.d.rays, c.h.rays, n * sizeof(rtk_ray), hipMemcpyHostToDevice, c.stream) != hipSuccess) { rtk_set_error("rtk_trace_rays: H2D copy failed"); return false; }
	rtk_dev_filter f;
	memset(&f, 0, sizeof(f));
	f.struct_size = sizeof(f);
	if (with_after) {
		if (hipMemcpyAsync(c.d.after, c.h.after, n * sizeof(rtk_hit_record), hipMemcpyHostToDevice, c.stream) != hipSuccess) { rtk_set_error("rtk_trace_rays: H2D copy failed"); return false; }
		f.d_after = c.d.after;
	}
	TraceCall call = batch_call(d_rays, n, opts, c.stream);
	call.hits = c.d.rec; call.filter = with_after ? &f : nullptr;
	if (rtk_launch_trace(ds, call) != RTK_AMD_OK) return false;
	c.status_mirrored = false;
	if (zero_copy) {
		c.ticket_in_flight = 0;
		if (n <= 256) c.ticket_in_flight = c.ticket = next_ticket(c.ticket);
		if (rtk_launch_expand(ds, c.d.rec, n, want_hits ? c.h.hits : nullptr, c.h.mask, c.stream, c.h.status, c.ticket_in_flight) != RTK_AMD_OK) return false;
		c.status_mirrored = true;
	} else {
		if (rtk_launch_expand(ds, c.d.rec, n, want_hits ? c.d.hits : nullptr, c.d.mask, c.stream) != RTK_AMD_OK) return false;
		bool ok = hipMemcpyAsync(c.h.mask, c.d.mask, n, hipMemcpyDeviceToHost, c.stream) == hipSuccess;
		if (want_hits) ok = ok && hipMemcpyAsync(c.h.hits, c.d.hits, n * sizeof(rtk_hit), hipMemcpyDeviceToHost, c.stream) == hipSuccess;
		if (!ok) { rtk_set_error("rtk_trace_rays: D2H copy failed: %s", hipGetErrorString(hipGetLastError())); return false; }
	}
	return true;
}

// Second half: wait for the piece, then hand its results to the caller's arrays. Returns the hits, (size_t)-1 on error.
size_t finish_piece(rtk_dev_scene *ds, HostCtx &c, size_t n, rtk_hit *hits, uint8_t *hit_mask)
{
	if (c.status_mirrored) {
		// the error word came down with the results: one synchronisation, no transfer (the slow path below reports and resets it)
		const bool arrived = c.ticket_in_flight && wait_ticket(c.h.status, c.ticket_in_flight);
		if (!arrived && hipStreamSynchronize(c.stream) != hipSuccess) { rtk_set_error("rtk_trace_rays: %s", hipGetErrorString(hipGetLastError())); return (size_t)-1; }
		if ((*c.h.status & 0xffffffffull) != 0ull && rtk_trace_status(ds, c.stream) != RTK_AMD_OK) return (size_t)-1;
	} else if (rtk_trace_status(ds, c.stream) != RTK_AMD_OK) return (size_t)-1;      // synchronises the stream
	size_t count = 0;
	for (size_t i = 0; i < n; i++) {
		if (c.h.mask[i]) { count++; if (hits) hits[i] = c.h.hits[i]; }           // misses stay untouched (rtk.c:571-576)
		if (hit_mask) hit_mask[i] = c.h.mask[i];
	}
	return count;
}

// rtk_trace_ray's own path: one ray, ONE launch (rtk_trace_one_kernel walks the ray's frontier breadth first with a whole wave
// and writes the full rtk_hit, the mask and the ticket into the pinned staging memory itself). Returns the hits (0 / 1),
// (size_t)-1 on error, (size_t)-2 when the kernel reported "not done" (a frontier that does not fit LDS): the caller then takes
// the batch path.
size_t trace_one(rtk_dev_scene *ds, HostCtx &c, const rtk_ray *ray, rtk_hit *hit, uint8_t *hit_mask)
{
	c.h.rays[0] = *ray;
	c.ticket = next_ticket(c.ticket);
	const int launched = rtk_launch_trace_one(ds, c.h.rays, c.h.hits, c.h.mask, c.stream, c.h.status, c.ticket);
	if (launched == RTK_AMD_ERR_UNSUPPORTED) return (size_t)-2;          // (a scene beyond the one-ray kernel's 32-bit offsets: the batch path diagnoses it)
	if (launched != RTK_AMD_OK) return (size_t)-1;
	if (!wait_ticket(c.h.status, c.ticket)) {
		if (hipStreamSynchronize(c.stream) != hipSuccess) { rtk_set_error("rtk_trace_ray: %s", hipGetErrorString(hipGetLastError())); return (size_t)-1; }
		if ((uint32_t)(*c.h.status >> 32) != c.ticket) { rtk_set_error("rtk_trace_ray: the kernel finished without its ticket"); return (size_t)-1; }
	}
	if ((*c.h.status & 0xffffffffull) == 2ull) return (size_t)-2;
	const uint8_t m = c.h.mask[0];
	if (m && hit) *hit = c.h.hits[0];
	if (hit_mask) *hit_mask = m;
	return m ? 1 : 0;
}

std::atomic<int> g_test_fail_calls{0};
// Fault injection for the tests of the per-ray calls' failure reporting. Not in the installed header; a no-op unless the process
// was started with RTK_AMD_TEST_HOOKS=1 (read once): no code of a production host can make its traces fail through it.
extern "C" void rtk_amd_test_fail_next_calls(int calls)
{
	static const bool armed = getenv("RTK_AMD_TEST_HOOKS") && !strcmp(getenv("RTK_AMD_TEST_HOOKS"), "1");
	if (armed) g_test_fail_calls.store(calls > 0 ? calls : 0);
}

bool injected_failure(const char *who)
{
	if (g_test_fail_calls.load(std::memory_order_relaxed) > 0 && g_test_fail_calls.fetch_sub(1) > 0) {
		rtk_set_error("%s: injected failure (rtk_amd_test_fail_next_calls)", who);
		t_fatal = false;
		return true;
	}
	return false;
}

} // namespace

extern "C" size_t rtk_trace_rays(const rtk_scene *scene, const rtk_ray *rays, size_t n, rtk_hit *hits, uint8_t *hit_mask)
{
	if (!scene || (!rays && n)) { rtk_set_error("rtk_trace_rays: NULL argument"); return (size_t)-1; }
	if (n == 0) return 0;
	t_fatal = false;
	if (injected_failure("rtk_trace_rays")) return (size_t)-1;
	rtk_dev_scene *ds = g_cache.lookup(scene, current_device());
	if (!ds) return (size_t)-1;
	if (n < 2 * PIPE_CHUNK_RAYS) {
		HostCtx &c = t_ctx;
		if (!c.ensure(n)) return (size_t)-1;
		static const int one_default = getenv("RTK_AMD_ONE_RAY_KERNEL") ? atoi(getenv("RTK_AMD_ONE_RAY_KERNEL")) : 1;
		if (n == 1 && one_default != 0) {
			const size_t r = trace_one(ds, c, rays, hits, hit_mask);
			if (r != (size_t)-2) return r;
		}
		if (!enqueue_piece(ds, c, rays, n, hits != nullptr, false)) return (size_t)-1;
		return finish_piece(ds, c, n, hits, hit_mask);
	}
	// Pipelined (run_pipeline). An image (recognised by its regular step, as rtk_dev_trace_rays does for device rays:
	// rtk_detect_rule.h) goes in bands: the packet kernels instead of one ray per lane.
	uint32_t iw = 0, ih = 0;
	if (rtk_trace_knobs().detect_image != 0) rtk_detect_host(rays, n, &iw, &ih);
	const size_t band = band_rays(iw, ih);
	rtk_trace_opts band_opts;
	memset(&band_opts, 0, sizeof(band_opts));
	band_opts.struct_size = sizeof(band_opts);
	band_opts.image_width = iw;
	const size_t chunk = band ? band : PIPE_CHUNK_RAYS;
	HostCtx *ctx[2] = { &t_ctx, &t_ctx2 };
	if (!ctx[0]->ensure(chunk) || !ctx[1]->ensure(chunk)) return (size_t)-1;
	return run_pipeline(n, chunk,
		[&](int k, size_t at, size_t m) {
			band_opts.image_height = band ? (uint32_t)(m / iw) : 0u;      // (the last band may be lower; still whole 64-pixel rows)
			return enqueue_piece(ds, *ctx[k], rays + at, m, hits != nullptr, false, band ? &band_opts : nullptr);
		},
		[&](int k, size_t at, size_t m) { return finish_piece(ds, *ctx[k], m, hits ? hits + at : nullptr, hit_mask ? hit_mask + at : nullptr); });
}

// Batch form of rtk_trace_ray_filter (rtk.h:117, 130; a stub in the reference, rtk.c:579-582). Semantics:
// for every ray the closest candidate hit the filter accepts. Candidates of a ray are offered in increasing
// (t, primitive id) order -- every candidate, including several at one and the same t -- until one is
// accepted or none is left. The callback runs on the host, so the batch goes in rounds (run_candidate_rounds): a launch collects
// the k closest candidates of every undecided ray (k = 65536 / rays in the round: 4 for a full round, up to 64
// for a single ray), the callback is asked about them in order, and rays whose k candidates were all rejected
// go into the next round restricted to what comes after the last one. Launches = rounds, not candidates: a
// single ray needs one launch per 64 rejected candidates.
extern "C" size_t rtk_trace_rays_filter(const rtk_scene *scene, const rtk_ray *rays, size_t n, rtk_hit *hits, uint8_t *hit_mask,
	rtk_filter_fn *filter, void *filter_user)
{
	if (!filter) return rtk_trace_rays(scene, rays, n, hits, hit_mask);
	if (!scene || (!rays && n)) { rtk_set_error("rtk_trace_rays_filter: NULL argument"); return (size_t)-1; }
	if (n == 0) return 0;
	t_fatal = false;
	rtk_dev_scene *ds = g_cache.lookup(scene, current_device());
	if (!ds) return (size_t)-1;
	HostCtx &c = t_ctx;
	if (!c.ensure(n < CAND_RAYS ? n : CAND_RAYS) || !c.ensure_candidates()) return (size_t)-1;
	rtk_dev_filter f;
	memset(&f, 0, sizeof(f));
	f.struct_size = sizeof(f);
	f.d_after = c.d.after;
	const CandRound round_failed = { nullptr, nullptr, nullptr };
	auto round = [&](const std::vector<size_t> &todo, const std::vector<rtk_hit_record> &after, size_t k) {
		const size_t r = todo.size();
		for (size_t q = 0; q < r; q++) { c.h.rays[q] = rays[todo[q]]; c.h.after[q] = after[q]; }
		bool ok = hipMemcpyAsync(c.d.rays, c.h.rays, r * sizeof(rtk_ray), hipMemcpyHostToDevice, c.stream) == hipSuccess &&
			hipMemcpyAsync(c.d.after, c.h.after, r * sizeof(rtk_hit_record), hipMemcpyHostToDevice, c.stream) == hipSuccess;
		if (!ok) { rtk_set_error("rtk_trace_rays_filter: H2D copy failed"); return round_failed; }
		// unused list slots stay "no primitive" so that the expand kernel leaves them alone
		if (hipMemsetAsync(c.dc.cand, 0xff, r * k * sizeof(rtk_hit_record), c.stream) != hipSuccess) { rtk_set_error("rtk_trace_rays_filter: memset failed"); return round_failed; }
		TraceCall call = batch_call(c.d.rays, r, nullptr, c.stream);
		call.filter = &f; call.cand = c.dc.cand; call.cand_count = c.dc.count; call.cand_k = (uint32_t)k;
		if (rtk_launch_trace(ds, call) != RTK_AMD_OK) return round_failed;
		if (rtk_launch_expand(ds, c.dc.cand, r * k, c.dc.hits, nullptr, c.stream) != RTK_AMD_OK) return round_failed;
		ok = hipMemcpyAsync(c.hc.cand, c.dc.cand, r * k * sizeof(rtk_hit_record), hipMemcpyDeviceToHost, c.stream) == hipSuccess &&
			hipMemcpyAsync(c.hc.hits, c.dc.hits, r * k * sizeof(rtk_hit), hipMemcpyDeviceToHost, c.stream) == hipSuccess &&
			hipMemcpyAsync(c.hc.count, c.dc.count, r * sizeof(uint32_t), hipMemcpyDeviceToHost, c.stream) == hipSuccess;
		if (!ok) { rtk_set_error("rtk_trace_rays_filter: D2H copy failed: %s", hipGetErrorString(hipGetLastError())); return round_failed; }
		if (rtk_trace_status(ds, c.stream) != RTK_AMD_OK) return round_failed;      // synchronises the stream
		return CandRound{ c.hc.cand, c.hc.hits, c.hc.count };
	};
	return run_candidate_rounds(n, hits, hit_mask, round, [&](size_t i, const rtk_hit *hit) { return filter(filter_user, &rays[i], hit); });
}

// ---------------------------------------------------------------------------- rtk.h: trace

// What a per-ray call does when its batch of one failed. The signatures have no error channel (the reference's entry point
// cannot fail) and `false` means "miss" to a host that only knows rtk.h, so a failure is never silent:
//   * every failure prints one line on stderr (the first 8 of a process, then every 1024th) and sets rtk_amd_last_error();
//   * one that every later call would repeat -- no usable GPU, a scene that does not validate -- or a SECOND failure in a row
//     on the calling thread (a stream error that sticks looks like a transient one the first time) would turn every ray
//     into a wrong "miss": report and stop, unless the host opted into soft failures (RTK_AMD_SOFT_ERRORS: false +
//     rtk_amd_last_error(), still reported on stderr);
//   * a lone failure that may pass (out of memory, an interrupted launch) returns false.
static thread_local unsigned t_per_ray_failures = 0;
static std::atomic<unsigned long long> g_per_ray_failures_reported{0};

static bool per_ray_failure(const char *who)
{
	const unsigned in_a_row = ++t_per_ray_failures;
	const unsigned long long seen = g_per_ray_failures_reported.fetch_add(1);
	const bool fatal = rtk_last_failure_is_fatal() || in_a_row >= 2u;
	const bool soft = getenv("RTK_AMD_SOFT_ERRORS") != nullptr;
	if (seen < 8ull || (seen & 1023ull) == 0ull || (fatal && !soft))
		fprintf(stderr, "%s: FAILED, not a miss (%s)%s: %s\n", who, fatal ? (in_a_row >= 2u ? "second failure in a row" : "permanent") : "transient",
			seen >= 8ull ? " [further reports are rate-limited]" : "", rtk_amd_last_error());
	if (fatal && !soft) abort();
	return false;
}

// The per-ray symbols on the calling thread (rtk_host_trace.cpp): see there why. RTK_AMD_PER_RAY=gpu sends them through the
// GPU again (a batch of one: rtk_trace_one_kernel, one launch + a ticket, ~25 us).
int rtk_host_trace_ray(const rtk_scene *scene, const rtk_ray *ray, rtk_hit *hit, const rtk_hit *after);
int rtk_host_trace_ray_filter(const rtk_scene *scene, const rtk_ray *ray, rtk_hit *hit, rtk_filter_fn *filter, void *user);

static std::atomic<int> g_per_ray_where{-1};           // -1: not decided yet (RTK_AMD_PER_RAY=gpu is read once)

extern "C" int rtk_amd_set_per_ray(int where)
{
	if (where != RTK_AMD_PER_RAY_HOST && where != RTK_AMD_PER_RAY_GPU) { rtk_set_error("rtk_amd_set_per_ray: unknown value %d", where); return RTK_AMD_ERR_BAD_ARG; }
	g_per_ray_where.store(where);
	return RTK_AMD_OK;
}

static bool per_ray_on_gpu()
{
	int w = g_per_ray_where.load(std::memory_order_relaxed);
	if (w < 0) {
		const char *e = getenv("RTK_AMD_PER_RAY");
		w = (e && !strcmp(e, "gpu")) ? RTK_AMD_PER_RAY_GPU : RTK_AMD_PER_RAY_HOST;
		g_per_ray_where.store(w);
	}
	return w == RTK_AMD_PER_RAY_GPU;
}

// one ray, with a filter or without (NULL), where the host chose; the arguments have been checked
static bool per_ray(const char *who, const rtk_scene *scene, const rtk_ray *ray, rtk_hit *hit, rtk_filter_fn *filter, void *filter_user)
{
	if (!per_ray_on_gpu()) {
		if (injected_failure(who)) return per_ray_failure(who);
		const int r = filter ? rtk_host_trace_ray_filter(scene, ray, hit, filter, filter_user) : rtk_host_trace_ray(scene, ray, hit, nullptr);
		if (r < 0) { t_fatal = true; return per_ray_failure(who); }       // a blob that is not a tree stays one
		t_per_ray_failures = 0;
		return r == 1;
	}
	uint8_t m = 0;
	rtk_hit h;
	const size_t r = rtk_trace_rays_filter(scene, ray, 1, &h, &m, filter, filter_user);      // (no filter: rtk_trace_rays)
	if (r == (size_t)-1) return per_ray_failure(who);
	t_per_ray_failures = 0;
	if (m) *hit = h;
	return m != 0;
}

// reference rtk.h:129 / rtk.c:543-577. Re-entrant, any thread, `*hit` untouched on a miss. Served on the calling thread from
// the caller's blob (< 1.5 us; profiles/r05_c_host_latency.log); throughput callers use rtk_trace_rays / rtk_dev_trace_rays,
// which run on the GPU and nowhere else.
extern "C" bool rtk_trace_ray(const rtk_scene *scene, const rtk_ray *ray, rtk_hit *hit)
{
	if (!scene || !ray || !hit) { rtk_set_error("rtk_trace_ray: NULL argument"); return false; }
	return per_ray("rtk_trace_ray", scene, ray, hit, nullptr, nullptr);
}

// reference rtk.h:117,130 (stub at rtk.c:579-582): the closest hit that the filter accepts; see
// rtk_trace_rays_filter for the order in which candidates are offered.
extern "C" bool rtk_trace_ray_filter(const rtk_scene *scene, const rtk_ray *ray, rtk_hit *hit, rtk_filter_fn *filter, void *filter_user)
{
	if (!scene || !ray || !hit) { rtk_set_error("rtk_trace_ray_filter: NULL argument"); return false; }
	return per_ray(filter ? "rtk_trace_ray_filter" : "rtk_trace_ray", scene, ray, hit, filter, filter_user);
}
