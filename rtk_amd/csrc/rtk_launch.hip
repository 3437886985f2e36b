// rtk_launch.hip -- the host side of a trace launch: what is asked (TraceCall, rtk_dev.h) is checked, planned (rtk_trace_plan.h),
// given the scratch set of its (scene, stream) (rtk_launch_scratch.h) and enqueued through the doors of the kernel files:
// rtk_trace.hip, rtk_trace_packet.hip, rtk_ray_sort.hip, rtk_detect.hip and the hand-written code objects (AsmModule). Also the
// environment defaults, the launch-error word and its report, and the debug entry lists. No kernel lives here.
#include "rtk_dev.h"

#include <algorithm>
#include "rtk_trace_shared.h"

#include <stdio.h>
#include <stdlib.h>

#include <mutex>

// ---- the hand-written kernels' code objects (AsmModule, rtk_trace_shared.h). The per-lane ones (rtk_lane_hot.S) belong to this file.
#include "rtk_lane_hot_image.h"

const TraceKnobs &rtk_trace_knobs()
{
	static const TraceKnobs knobs = [] {
		const auto env = [](const char *name, int value) { const char *v = getenv(name); return v ? atoi(v) : value; };
		TraceKnobs k;
		k.detect_image = env("RTK_AMD_DETECT_IMAGE", k.detect_image);
		k.tile_blocks = env("RTK_AMD_TILE_BLOCKS", k.tile_blocks);
		k.any_packets = env("RTK_AMD_ANY_PACKETS", k.any_packets);
		k.qnodes = env("RTK_AMD_QNODES", k.qnodes);
		k.packet_asm = env("RTK_AMD_PACKET_ASM", k.packet_asm);
		// (a number below 0 is the C++ kernel, one above 2 is 2: the counting and any-hit forms are not for choosing)
		const int wanted = env("RTK_AMD_PACKET_BEAM", (int)k.packet_beam);
		k.packet_beam = wanted < 0 ? PacketKernel::Cpp : wanted > (int)PacketKernel::Beam2 ? PacketKernel::Beam2 : (PacketKernel)wanted;
		k.log_path = getenv("RTK_AMD_LOG_PATH") != nullptr;
		k.lane_asm = env("RTK_AMD_LANE_ASM", k.lane_asm);
		k.lane_lds = (size_t)env("RTK_AMD_LANE_LDS", (int)k.lane_lds);
		k.sort_cell_bits = (uint32_t)env("RTK_AMD_SORT_CELL_BITS", (int)k.sort_cell_bits);
		k.sort_octant = (uint32_t)env("RTK_AMD_SORT_OCTANT", (int)k.sort_octant);
		k.sort_key = env("RTK_AMD_SORT_KEY", k.sort_key);
		k.packet_entries = env("RTK_AMD_PACKET_ENTRIES", k.packet_entries);
		k.entry_target = (unsigned)env("RTK_AMD_ENTRY_TARGET", (int)k.entry_target);
		k.entry_levels = (unsigned)env("RTK_AMD_ENTRY_LEVELS", (int)k.entry_levels);
		k.hot_blocks_per_cu = env("RTK_AMD_HOT_BLOCKS_PER_CU", k.hot_blocks_per_cu);
		k.lane_stats = env("RTK_AMD_LANE_STATS", k.lane_stats);
		k.lane_blocks = env("RTK_AMD_LANE_BLOCKS", k.lane_blocks);
		return k;
	}();
	return knobs;
}

AsmModule &rtk_lane_module()
{
	// 80 VGPRs, 30 KB of LDS per workgroup: five workgroups per CU; the any-hit kernel is launched on the same figure
	static const AsmKernel table[4] = { { "rtk_lane_hot_closest", rtk_trace_knobs().lane_blocks }, { "rtk_lane_hot_any", 0 },
		{ "rtk_lane_hot_closest_listed", 0 }, { "rtk_lane_hot_any_listed", 0 } };
	static AsmModule m(rtk_lane_hot_image, table, 4, "rtk_dev_trace: the assembly per-lane kernels are not loaded");
	return m;
}

const AsmModule::Loaded *AsmModule::on(int device)
{
	if (device < 0 || device >= RTK_MAX_DEVICES) return nullptr;
	std::lock_guard<std::mutex> lock(mutex);
	Loaded &h = slot[device];
	if (!h.tried) {
		int cur = -1;
		if (hipGetDevice(&cur) != hipSuccess || cur != device) return nullptr;
		h.tried = true;
		if (hipModuleLoadData(&h.mod, image) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
		for (int k = 0; k < count; k++) {
			if (hipModuleGetFunction(&h.fn[k], h.mod, table[k].name) != hipSuccess) { (void)hipGetLastError(); h.fn[k] = nullptr; continue; }
			if (table[k].cap == 0) continue;
			int nb = 0;
			if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&nb, h.fn[k], TRACE_BLOCK_THREADS, 0) != hipSuccess || nb < 1) nb = 1;
			h.blocks_per_cu[k] = nb > table[k].cap ? table[k].cap : nb;
		}
	}
	return h.fn[0] ? &h : nullptr;
}

int AsmModule::launch(int device, int kernel, void *params, size_t size, unsigned blocks, hipStream_t stream)
{
	const Loaded *h = on(device);
	if (!h || kernel < 0 || kernel >= count || !h->fn[kernel]) { rtk_set_error("%s", not_loaded); return RTK_AMD_ERR_HIP; }
	void *config[] = { HIP_LAUNCH_PARAM_BUFFER_POINTER, params, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END };
	RTK_HIP_CHECK(hipModuleLaunchKernel(h->fn[kernel], blocks, 1, 1, TRACE_BLOCK_THREADS, 1, 1, 0, stream, nullptr, config), RTK_AMD_ERR_HIP);
	return RTK_AMD_OK;
}

// ---- the scratch sets' allocator (rtk_launch_scratch.h)
namespace {

void *scratch_alloc(size_t bytes)
{
	void *p = nullptr;
	const hipError_t e = hipMalloc(&p, bytes);
	if (e != hipSuccess) { rtk_set_error("hipMalloc(ptr, bytes) failed: %s (launch scratch)", hipGetErrorString(e)); return nullptr; }
	return p;
}

void scratch_free(void *p) { (void)hipFree(p); }
void scratch_free_pinned(void *p) { (void)hipHostFree(p); }

int scratch_wait(void *on)
{
	const hipStream_t stream = (hipStream_t)on;
	RTK_HIP_CHECK(hipStreamSynchronize(stream), RTK_AMD_ERR_HIP);
	return RTK_AMD_OK;
}

unsigned long long *scratch_counter(void *stream)
{
	const size_t bytes = (RTK_COUNTER_WORDS + 1 + RTK_DETECT_WORDS) * sizeof(unsigned long long);
	unsigned long long *d_counter = nullptr;
	// (cleared ON THE LAUNCH STREAM: a hipMemset goes to the NULL stream, which non-blocking streams do not wait for -- behind
	// another thread's device build there it ran milliseconds late, and a first launch read a stale error word: an intermittent
	// "traversal stack overflow" in test_builds_and_traces_from_several_threads_at_once)
	if (hipMalloc(&d_counter, bytes) != hipSuccess || hipMemsetAsync(d_counter, 0, bytes, (hipStream_t)stream) != hipSuccess) {
		rtk_set_error("rtk_dev_trace: out of device memory (launch scratch)");
		if (d_counter) (void)hipFree(d_counter);
		return nullptr;
	}
	return d_counter;
}

} // namespace

const ScratchHooks &rtk_scratch_hooks()
{
	static const ScratchHooks hooks = { scratch_alloc, scratch_free, scratch_wait, scratch_counter, scratch_free_pinned };
	return hooks;
}

bool rtk_on_scene_device(const rtk_dev_scene *ds, const char *caller)
{
	int cur = -1;
	if (hipGetDevice(&cur) == hipSuccess && cur == ds->device) return true;
	rtk_set_error("%s: the scene lives on device %d, the calling thread's current device is %d", caller, ds->device, cur);
	return false;
}

unsigned long long *rtk_error_word(rtk_dev_scene *ds, hipStream_t stream)
{
	std::lock_guard<std::mutex> lock(ds->scratch_mutex);
	const LaunchScratch *s = ds->scratch.find(stream);
	return s ? s->d_counter + RTK_ERROR_WORD : nullptr;
}

namespace {

DeviceKernels device_kernels(int device)
{
	DeviceKernels dk;
	if (const AsmModule::Loaded *h = rtk_packet_module().on(device)) {
		for (int k = 0; k < NUM_PACKET_KERNELS; k++) {
			dk.packet[k] = h->fn[k] != nullptr;
			dk.packet_blocks_per_cu[k] = h->blocks_per_cu[k > (int)PacketKernel::Beam2 ? (int)PacketKernel::Beam2 : k];
		}
	}
	if (const AsmModule::Loaded *h = rtk_lane_module().on(device)) {
		dk.lane = h->fn[0] && h->fn[1];
		dk.lane_listed = h->fn[2] && h->fn[3];
		dk.lane_blocks_per_cu = h->blocks_per_cu[0];
	}
	return dk;
}

// Which combinations of a call's fields are legal.
int check_call(const rtk_dev_scene *ds, const TraceCall &c)
{
	const bool collect = c.cand != nullptr;
	if (c.pk_counted && (c.counted || c.any_hit || c.filter || collect)) { rtk_set_error("rtk_dev_trace_rays_packet_counted: closest-hit batches only"); return RTK_AMD_ERR_BAD_ARG; }
	if (c.pk_counted) *c.pk_counted = rtk_packet_counters();
	if (collect && (!c.cand_count || c.cand_k == 0 || c.any_hit || c.counted)) { rtk_set_error("rtk_dev_trace: bad collect arguments"); return RTK_AMD_ERR_BAD_ARG; }
	if (!ds || (!c.rays && c.n) || (!collect && (c.any_hit ? !c.occluded : !c.hits) && c.n)) { rtk_set_error("rtk_dev_trace: bad argument"); return RTK_AMD_ERR_BAD_ARG; }
	if (c.list && (c.counted || c.pk_counted || collect)) { rtk_set_error("rtk_dev_trace: a ray list with a counted or collecting launch"); return RTK_AMD_ERR_BAD_ARG; }
	return RTK_AMD_OK;
}

// ... and what the plan reads of it (the filter has been checked).
TraceRequest request_of(const TraceCall &c)
{
	TraceRequest rq;
	rq.n = c.n; rq.any_hit = c.any_hit; rq.counted = c.counted != nullptr; rq.pk_counted = c.pk_counted != nullptr; rq.collect = c.cand != nullptr;
	rq.has_filter = c.filter != nullptr;
	rq.filtered = c.filter && (c.filter->d_mesh_mask || c.filter->d_ignore_prim || c.filter->d_after);
	rq.listed = c.list != nullptr;
	return rq;
}

SceneFacts facts_of(const rtk_dev_scene *ds)
{
	SceneFacts facts;
	facts.num_nodes = ds->view.num_nodes; facts.num_tris = ds->view.num_tris; facts.has_qnodes = ds->view.qnodes != nullptr;
	facts.stack_entries = ds->tree.stack_entries(); facts.bound_abs = ds->tree.bound_abs; facts.big_leaf_fraction = ds->tree.big_leaf_fraction;
	facts.num_cus = ds->num_cus; facts.tri_stride = RTK_TRI_STRIDE;
	return facts;
}

int grow_scratch(LaunchScratch *sc, const TracePlan &plan, size_t n)
{
	int rc = RTK_AMD_OK;
	if (plan.spill_cap) rc = sc->grow_spill(plan.spill_lanes, plan.spill_cap, sizeof(uint2));
	if (rc == RTK_AMD_OK && plan.sort_rays) rc = sc->grow(sc->sort, n, rtk_ray_sort_bytes(n));
	if (rc == RTK_AMD_OK && plan.entries) {
		const size_t nblk = (size_t)(plan.image_w >> 6) * (plan.image_h >> 6);
		rc = sc->grow(sc->entries, nblk, nblk * sizeof(PkBlockEntries));
	}
	// one list serves both hand-overs: tile numbers (4 bytes each) or one 8-byte word per left-over ray
	const size_t left_bytes = plan.hot ? (n >> 6) * sizeof(uint32_t) : plan.lane_hot ? n * sizeof(unsigned long long) : 0;
	if (rc == RTK_AMD_OK) rc = sc->grow(sc->leftover, left_bytes, left_bytes);
	return rc;
}

// The four ways a batch is traced. `p` is complete; each enqueues on `stream` and leaves launch errors to the caller's hipGetLastError.

// a hand-written packet kernel, then the C++ kernel on the tiles it handed back (mixed signs or axes, untame rays, a big leaf, a deep stack)
int enqueue_packet_hot(const rtk_dev_scene *ds, LaunchScratch *sc, TraceParams &p, const TracePlan &plan, bool any_hit, bool pk_counted, hipStream_t stream)
{
	const size_t tiles = (size_t)p.n >> 6;
	PkHotParams hp = {};
	hp.nodes = p.sc.nodes; hp.tris = p.sc.tris; hp.rays = p.rays; hp.hits = any_hit ? reinterpret_cast<rtk_hit_record *>(p.occluded) : p.hits; hp.counter = p.counter; hp.leftover = sc->leftover.as<uint32_t>();
	hp.num_blocks = (uint32_t)(tiles >> 6);
	hp.image_w = p.image_w;
	hp.blocks_per_row = p.image_w >> 6;
	hp.bpr_magic = (uint32_t)((0x100000000ull + hp.blocks_per_row - 1u) / hp.blocks_per_row);
	hp.bound_abs = ds->tree.bound_floor1();
	hp.entries = p.entries;
	const int rc = rtk_packet_module().launch(ds->device, (int)plan.kernel, &hp, sizeof(hp), (unsigned)plan.hot_grid, stream);
	if (rc != RTK_AMD_OK) return rc;
	// (a small grid: the list is empty for most batches, and a launch that only finds that out should cost next to nothing)
	p.tile_list = hp.leftover;
	const size_t left_blocks = std::min<size_t>(plan.grid, (size_t)ds->num_cus * 2u);
	rtk_packet_launch(p, (unsigned)left_blocks, stream, pk_counted);      // (counting: the handed-back tiles' steps are counted too)
	return RTK_AMD_OK;
}

// a hand-written per-lane kernel, then rtk_trace_kernel on the rays it left over
int enqueue_lane_hot(const rtk_dev_scene *ds, LaunchScratch *sc, const TraceParams &p, const TracePlan &plan, bool any_hit, bool refill_given,
	const TraceKnobs &knobs, hipStream_t stream)
{
	LnHotListedParams lhp = {};
	LnHotParams &hp = lhp.hot;
	hp.qnodes = p.sc.qnodes; hp.tris = p.sc.tris; hp.rays = p.rays;
	hp.out = any_hit ? (void *)p.occluded : (void *)p.hits;
	hp.counter = p.counter;
	hp.leftover = sc->leftover.as<unsigned long long>();
	hp.perm = p.perm;
	hp.n = (uint32_t)p.n;
	// (re-swept for these kernels: refill at 16 idle lanes instead of 8 is +1 % / +2 %, profiles/r04_lane_sweep.log)
	hp.refill_min = refill_given ? p.refill_min : 16u;
	hp.node_exit = p.node_exit;
	hp.bound_abs = ds->tree.bound_raw;             // (no floor of 1: these kernels test child words, not inverted boxes)
	hp.spill = p.spill;
	hp.spill_stride = p.spill_stride;
	hp.spill_cap = p.spill_cap;
	// (a listed batch: the kernel reads how many entries of `perm` -- or how many of the rays themselves -- it traces)
	lhp.count = p.n_indirect;
	const int rc = p.n_indirect ? rtk_lane_module().launch(ds->device, any_hit ? 3 : 2, &lhp, sizeof(lhp), (unsigned)plan.lane_grid, stream)
		: rtk_lane_module().launch(ds->device, any_hit ? 1 : 0, &hp, sizeof(hp), (unsigned)plan.lane_grid, stream);
	if (rc != RTK_AMD_OK) return rc;
	if (knobs.lane_stats) {           // (diagnostics: how many rays the assembly kernel handed back; synchronises the stream)
		unsigned long long left = 0;
		(void)hipMemcpyAsync(&left, p.counter + RTK_LANE_LEFTOVER_WORD, sizeof(left), hipMemcpyDeviceToHost, stream);
		(void)hipStreamSynchronize(stream);
		fprintf(stderr, "rtk_lane_hot: %llu of %zu rays handed back (%.3f %%)\n", left, (size_t)p.n, 100.0 * (double)left / (double)p.n);
	}
	// (none in most batches: a small grid that finds an empty list costs next to nothing)
	TraceParams lp = p;
	lp.perm = hp.leftover;
	lp.n_indirect = p.counter + RTK_LANE_LEFTOVER_WORD;      // (never more than the p.n it is clamped to: a ray is handed back once)
	const size_t left_blocks = std::min<size_t>(plan.grid, (size_t)ds->num_cus);
	rtk_trace_kernel_launch(plan.variant, lp, (unsigned)left_blocks, stream);
	return RTK_AMD_OK;
}

int read_packet_counters(LaunchScratch *sc, size_t n, hipStream_t stream, rtk_packet_counters *out)
{
	unsigned long long c[16];
	RTK_HIP_CHECK(hipMemcpyAsync(c, sc->d_counter, sizeof(c), hipMemcpyDeviceToHost, stream), RTK_AMD_ERR_HIP);
	RTK_HIP_CHECK(hipStreamSynchronize(stream), RTK_AMD_ERR_HIP);
	out->pairs = c[11]; out->node_steps = c[12]; out->triangles_fetched = c[13]; out->triangle_group_tests = c[14];
	out->tiles_handed_back = c[RTK_LEFTOVER_COUNT_WORD];
	out->handed_back_node_steps = c[7]; out->handed_back_triangle_steps = c[8];
	out->tiles = n >> 6;
	return RTK_AMD_OK;
}

int read_counters(LaunchScratch *sc, hipStream_t stream, rtk_trace_counters *out)
{
	unsigned long long c[16], err = 0;
	RTK_HIP_CHECK(hipMemcpyAsync(c, sc->d_counter, sizeof(c), hipMemcpyDeviceToHost, stream), RTK_AMD_ERR_HIP);
	RTK_HIP_CHECK(hipMemcpyAsync(&err, sc->d_counter + RTK_ERROR_WORD, sizeof(err), hipMemcpyDeviceToHost, stream), RTK_AMD_ERR_HIP);
	RTK_HIP_CHECK(hipStreamSynchronize(stream), RTK_AMD_ERR_HIP);
	out->rays = c[1]; out->nodes = c[2]; out->leaves = c[3];
	out->triangles = c[4]; out->hits = c[5]; out->stack_spills = c[6];
	out->wave_node_steps = c[7]; out->wave_triangle_steps = c[8]; out->wave_rays = c[9];
	if (err) {
		(void)hipMemsetAsync(sc->d_counter + RTK_ERROR_WORD, 0, sizeof(err), stream);
		rtk_set_error("rtk_dev_trace: traversal stack overflow (corrupted scene)");
		return RTK_AMD_ERR_BAD_SCENE;
	}
	return RTK_AMD_OK;
}

} // namespace

int rtk_launch_trace(const rtk_dev_scene *ds_c, const TraceCall &c)
{
	rtk_dev_scene *ds = const_cast<rtk_dev_scene *>(ds_c);
	int rc = check_call(ds, c);
	if (rc != RTK_AMD_OK) return rc;
	const size_t n = c.n;
	const hipStream_t stream = c.stream;
	if (n == 0) { if (c.counted) *c.counted = rtk_trace_counters(); return RTK_AMD_OK; }
	if (!rtk_on_scene_device(ds, "rtk_dev_trace")) return RTK_AMD_ERR_BAD_ARG;
	if (!rtk_within_4gib(ds->view)) {
		rtk_set_error("rtk_dev_trace: scene exceeds 4 GiB of nodes or triangles (%u nodes, %u triangles)", ds->view.num_nodes, ds->view.num_tris);
		return RTK_AMD_ERR_UNSUPPORTED;
	}
	TraceParams p = {};
	p.sc = ds->view;
	p.rays = c.rays;
	p.hits = c.hits;
	p.occluded = c.occluded;
	p.cand = c.cand;
	p.cand_count = c.cand_count;
	p.cand_k = c.cand_k;
	p.n = n;
	if (c.list) { p.perm = reinterpret_cast<const unsigned long long *>(c.list->d_ids); p.n_indirect = reinterpret_cast<const unsigned long long *>(c.list->d_count); }
	if (c.filter) {
		if (c.filter->struct_size < sizeof(rtk_dev_filter)) { rtk_set_error("rtk_dev_trace: rtk_dev_filter.struct_size is too small"); return RTK_AMD_ERR_BAD_ARG; }
		if (c.filter->d_mesh_mask && c.filter->mesh_mask_bits == 0) { rtk_set_error("rtk_dev_trace: mesh mask without mesh_mask_bits"); return RTK_AMD_ERR_BAD_ARG; }
		p.mesh_mask = c.filter->d_mesh_mask;
		p.mesh_mask_bits = c.filter->mesh_mask_bits;
		p.ignore_prim = c.filter->d_ignore_prim;
		p.after = c.filter->d_after;
	}

	// what is asked, of which scene, on which device: the plan (rtk_trace_plan.h)
	const TraceKnobs &knobs = rtk_trace_knobs();
	const TraceOpts o = decode_opts(c.opts);
	const TraceRequest rq = request_of(c);
	const SceneFacts facts = facts_of(ds);
	uint32_t look_w = 0, look_h = 0;
	if (wants_image_look(rq, o, facts, knobs) && (rc = rtk_detect_image(ds, c.rays, n, stream, &look_w, &look_h)) != RTK_AMD_OK) return rc;
	const DeviceKernels kernels = device_kernels(ds->device);
	const int occ = rtk_trace_occupancy(ds->device, variant_of(rq, o, look_w, look_h, facts, kernels, knobs));
	const TracePlan plan = plan_trace(rq, o, look_w, look_h, facts, kernels, knobs, occ);
	if (plan.error != RTK_AMD_OK) { rtk_set_error("%s", plan.message); return plan.error; }
	if (knobs.log_path) fprintf(stderr, "rtk_dev_trace: n %zu image %u x %u packet %d hot %d beam %d opts %p flags %x\n", n, plan.image_w, plan.image_h, (int)plan.packet, (int)plan.hot, (int)plan.kernel, (const void *)c.opts, o.flags);
	p.dynamic = plan.dynamic;
	p.refill_min = plan.refill_min;
	p.node_exit = plan.node_exit;
	p.image_w = plan.image_w;
	p.image_h = plan.image_h;
	p.tile_blocks = plan.tile_blocks;

	// From here on the launch uses the scratch set of (scene, stream); the mutex is held until everything is
	// enqueued, so that two host threads feeding one stream cannot interleave "reset queue heads" and "launch".
	std::lock_guard<std::mutex> lock(ds->scratch_mutex);
	LaunchScratch *sc = ds->scratch.get(stream);
	if (!sc) return RTK_AMD_ERR_OOM;
	if ((rc = grow_scratch(sc, plan, n)) != RTK_AMD_OK) return rc;
	p.spill = sc->spill.as<uint2>();
	p.spill_stride = (uint32_t)(plan.spill_cap ? sc->spill.capacity : 0);
	p.spill_cap = (uint32_t)plan.spill_cap;
	p.counter = sc->d_counter;
	if (plan.sort_rays && (rc = rtk_ray_sort_launch(ds, sc, c.rays, n, knobs, stream, &p.perm)) != RTK_AMD_OK) return rc;
	// queue heads and visit counters start from zero; a one-block static launch uses neither. (With entry lists the pre-pass
	// kernel clears them itself: a 4.6 us fill kernel and its launch gap less per frame.)
	if ((plan.dynamic || plan.packet || c.counted) && !plan.entries) RTK_HIP_CHECK(hipMemsetAsync(sc->d_counter, 0, RTK_COUNTER_WORDS * sizeof(unsigned long long), stream), RTK_AMD_ERR_HIP);
	if (plan.entries) {
		rtk_packet_entries_launch(p, sc->entries.as<PkBlockEntries>(), ds->tree.bound_floor1(), knobs.entry_target, knobs.entry_levels, stream);
		p.entries = sc->entries.as<PkBlockEntries>();
	}
	if (plan.hot) rc = enqueue_packet_hot(ds, sc, p, plan, c.any_hit, c.pk_counted != nullptr, stream);
	else if (plan.packet) rtk_packet_launch(p, (unsigned)plan.grid, stream, c.counted != nullptr);
	else if (plan.lane_hot) rc = enqueue_lane_hot(ds, sc, p, plan, c.any_hit, o.refill_given, knobs, stream);
	else rtk_trace_kernel_launch(plan.variant, p, (unsigned)plan.grid, stream);
	if (rc != RTK_AMD_OK) return rc;
	RTK_HIP_CHECK(hipGetLastError(), RTK_AMD_ERR_HIP);
	if (c.pk_counted && (rc = read_packet_counters(sc, n, stream, c.pk_counted)) != RTK_AMD_OK) return rc;
	if (c.counted) return read_counters(sc, stream, c.counted);
	return RTK_AMD_OK;
}

// rtk_dev_trace_rays_count / rtk_dev_trace_rays_all: every candidate of a ray (rtk_allhits.hip). No plan: one kernel family on the
// exact nodes, no packets, no reordering; of the options blocks_per_cu, refill_min and node_exit apply.
int rtk_launch_allhits(const rtk_dev_scene *ds_c, const rtk_ray *d_rays, size_t n, uint32_t *d_counts, const uint64_t *d_offsets,
	rtk_hit_record *d_records, uint32_t *d_written, bool fill, const rtk_dev_filter *filter, const rtk_trace_opts *opts, hipStream_t stream)
{
	rtk_dev_scene *ds = const_cast<rtk_dev_scene *>(ds_c);
	const char *const who = fill ? "rtk_dev_trace_rays_all" : "rtk_dev_trace_rays_count";
	// everything the host can see is refused here, before any HIP call
	if (!ds) { rtk_set_error("%s: NULL scene", who); return RTK_AMD_ERR_BAD_ARG; }
	if (n && (!d_rays || (fill ? (!d_offsets || !d_records) : !d_counts))) { rtk_set_error("%s: NULL rays or output", who); return RTK_AMD_ERR_BAD_ARG; }
	if (filter && filter->struct_size < sizeof(rtk_dev_filter)) { rtk_set_error("%s: rtk_dev_filter.struct_size is too small", who); return RTK_AMD_ERR_BAD_ARG; }
	if (filter && filter->d_mesh_mask && filter->mesh_mask_bits == 0) { rtk_set_error("%s: mesh mask without mesh_mask_bits", who); return RTK_AMD_ERR_BAD_ARG; }
	if (n >= ((size_t)1 << 32)) { rtk_set_error("%s: %zu rays: a batch holds fewer than 2^32", who, n); return RTK_AMD_ERR_BAD_ARG; }
	if (n == 0) return RTK_AMD_OK;
	if (!rtk_on_scene_device(ds, who)) return RTK_AMD_ERR_BAD_ARG;

	AllHitsParams p = {};
	p.rays = d_rays;
	p.n = (uint32_t)n;
	p.counts = d_counts;
	p.offsets = reinterpret_cast<const unsigned long long *>(d_offsets);
	p.records = d_records;
	p.written = d_written;
	bool filtered = false;
	if (filter) {
		p.mesh_mask = filter->d_mesh_mask;
		p.mesh_mask_bits = filter->mesh_mask_bits;
		p.ignore_prim = filter->d_ignore_prim;
		p.after = filter->d_after;
		filtered = filter->d_mesh_mask || filter->d_ignore_prim || filter->d_after;
	}
	const int form = (fill ? 1 : 0) | (filtered ? 2 : 0);
	const TraceOpts o = decode_opts(opts);
	p.refill_min = o.refill_min ? o.refill_min : 8u;
	p.node_exit = o.node_exit ? o.node_exit : 32u;
	// a batch that fits one workgroup needs no work queue (and no counter reset)
	p.dynamic = n > TRACE_BLOCK_THREADS ? 1u : 0u;
	const uint32_t occ = (uint32_t)rtk_allhits_occupancy(ds->device, form);
	const uint32_t blocks_per_cu = (o.blocks_per_cu == 0 || o.blocks_per_cu > occ) ? occ : o.blocks_per_cu;
	const size_t blocks_needed = (n + TRACE_BLOCK_THREADS - 1) / TRACE_BLOCK_THREADS;
	const size_t grid = std::min<size_t>(blocks_needed, (size_t)(ds->num_cus > 0 ? ds->num_cus : 1) * blocks_per_cu);

	// the scratch set of (scene, stream), held until the launch is enqueued; the view and the tree record are read under the
	// same lock a rebuild replaces them under
	std::lock_guard<std::mutex> lock(ds->scratch_mutex);
	if (!rtk_within_4gib(ds->view)) {
		rtk_set_error("%s: scene exceeds 4 GiB of nodes or triangles (%u nodes, %u triangles)", who, ds->view.num_nodes, ds->view.num_tris);
		return RTK_AMD_ERR_UNSUPPORTED;
	}
	p.nodes = ds->view.nodes; p.tris = ds->view.tris;
	p.num_nodes = ds->view.num_tris != 0u ? ds->view.num_nodes : 0u;
	const size_t entries = ds->tree.stack_entries();
	const size_t spill_cap = entries > AH_LDS_STACK ? entries - AH_LDS_STACK : 0;
	LaunchScratch *sc = ds->scratch.get(stream);
	if (!sc) return RTK_AMD_ERR_OOM;
	if (spill_cap) {
		// (the area is shared with the kernels whose entries are 8 bytes, and remembered in their unit: two of this walk's entries each)
		const int rc = sc->grow_spill(grid * TRACE_BLOCK_THREADS, (spill_cap + 1u) / 2u, sizeof(uint2));
		if (rc != RTK_AMD_OK) return rc;
	}
	p.spill = sc->spill.as<uint32_t>();
	p.spill_stride = (uint32_t)(spill_cap ? sc->spill.capacity : 0);
	p.spill_cap = (uint32_t)spill_cap;
	p.counter = sc->d_counter;
	if (p.dynamic) RTK_HIP_CHECK(hipMemsetAsync(sc->d_counter, 0, RTK_COUNTER_WORDS * sizeof(unsigned long long), stream), RTK_AMD_ERR_HIP);
	rtk_allhits_kernel_launch(form, p, (unsigned)grid, stream);
	RTK_HIP_CHECK(hipGetLastError(), RTK_AMD_ERR_HIP);
	return RTK_AMD_OK;
}

// rtk_dev_debug_packet_entries: the pre-pass of an image frame alone, on the null stream's scratch set, and its lists copied to the host
int rtk_debug_packet_entries(const rtk_dev_scene *ds_c, const rtk_ray *d_rays, uint32_t image_w, uint32_t image_h, uint32_t target, uint32_t max_levels, void *host_out)
{
	rtk_dev_scene *ds = const_cast<rtk_dev_scene *>(ds_c);
	if (!ds || !d_rays || !host_out) { rtk_set_error("rtk_dev_debug_packet_entries: NULL argument"); return RTK_AMD_ERR_BAD_ARG; }
	if (image_w == 0 || image_h == 0 || (image_w & 63u) || (image_h & 63u) || (unsigned long long)image_w * image_h > 0xffffffffull) {
		rtk_set_error("rtk_dev_debug_packet_entries: %u x %u is not an image of whole 64x64-pixel blocks", image_w, image_h);
		return RTK_AMD_ERR_BAD_ARG;
	}
	if (!rtk_on_scene_device(ds, "rtk_dev_debug_packet_entries")) return RTK_AMD_ERR_BAD_ARG;
	if (ds->view.num_nodes == 0) { rtk_set_error("rtk_dev_debug_packet_entries: the scene has no nodes"); return RTK_AMD_ERR_BAD_ARG; }
	const hipStream_t stream = nullptr;
	std::lock_guard<std::mutex> lock(ds->scratch_mutex);
	LaunchScratch *sc = ds->scratch.get(stream);
	if (!sc) return RTK_AMD_ERR_OOM;
	const size_t nblk = (size_t)(image_w >> 6) * (image_h >> 6);
	const int rc = sc->grow(sc->entries, nblk, nblk * sizeof(PkBlockEntries));
	if (rc != RTK_AMD_OK) return rc;
	TraceParams p = {};
	p.sc = ds->view;
	p.rays = d_rays;
	p.image_w = image_w;
	p.image_h = image_h;
	p.counter = sc->d_counter;
	rtk_packet_entries_launch(p, sc->entries.as<PkBlockEntries>(), ds->tree.bound_floor1(), target, max_levels, stream);
	RTK_HIP_CHECK(hipGetLastError(), RTK_AMD_ERR_HIP);
	RTK_HIP_CHECK(hipMemcpyAsync(host_out, sc->entries.p, nblk * sizeof(PkBlockEntries), hipMemcpyDeviceToHost, stream), RTK_AMD_ERR_HIP);
	RTK_HIP_CHECK(hipStreamSynchronize(stream), RTK_AMD_ERR_HIP);
	return RTK_AMD_OK;
}

// Did any launch of this scene on `stream` since the last call overflow a traversal stack? Synchronises the stream.
int rtk_trace_status(const rtk_dev_scene *ds_c, hipStream_t stream)
{
	rtk_dev_scene *ds = const_cast<rtk_dev_scene *>(ds_c);
	if (!ds) { rtk_set_error("rtk_dev_trace_status: NULL scene"); return RTK_AMD_ERR_BAD_ARG; }
	// the error word's address is looked up under the lock; the wait for the stream happens outside it, so that threads
	// tracing one scene on their own streams do not queue up behind each other's synchronisation
	unsigned long long *word = rtk_error_word(ds, stream);
	if (!word) {
		RTK_HIP_CHECK(hipStreamSynchronize(stream), RTK_AMD_ERR_HIP);
		return RTK_AMD_OK;
	}
	unsigned long long e = 0;
	RTK_HIP_CHECK(hipMemcpyAsync(&e, word, sizeof(e), hipMemcpyDeviceToHost, stream), RTK_AMD_ERR_HIP);
	RTK_HIP_CHECK(hipStreamSynchronize(stream), RTK_AMD_ERR_HIP);
	if (e) {
		(void)hipMemsetAsync(word, 0, sizeof(e), stream);      // reported once
		rtk_set_error("rtk_dev_trace: traversal stack overflow (corrupted scene)");
		return RTK_AMD_ERR_BAD_SCENE;
	}
	return RTK_AMD_OK;
}

// A stream is going away (the host-pointer calls own one per thread): the scratch sets made for it are released, so that
// threads coming and going do not pile them up and a recycled stream handle never finds an old entry.
void rtk_scene_drop_stream(rtk_dev_scene *ds, hipStream_t stream)
{
	if (!ds) return;
	std::lock_guard<std::mutex> lock(ds->scratch_mutex);
	ds->scratch.drop(stream);
}
