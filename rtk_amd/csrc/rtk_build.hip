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
//
// This file: the per-device workspace and its loan to other passes, the sequence of the stages, the three entry points. The
// stages and their kernels: rtk_build_ingest.hip, rtk_build_refit.hip, rtk_build_collapse.hip (rtk_build_internal.h has the map);
// the host's decisions between them: rtk_build_plan.h; the rtk.h task API on top: rtk_build_api.hip.
#include "rtk_build_internal.h"

#include <stdio.h>

#include <chrono>
#include <mutex>

using namespace rtk_bld;

// =====================================================================================
// rtk_dev_scene_build
// =====================================================================================

namespace {

// (struct Workspace, rtk_build_internal.h, says who may touch it when)
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
	build_sah_costs_from_env(cost_node, cost_tri);
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

// (rtk_dev.h)
uint32_t rtk_build_max_leaf()
{
	return build_max_leaf_from_env();
}

namespace {

// ---- the workspace: sized and placed by the one carve of rtk_build_layout.h; the build's stream and pinned results ----
bool prepare_workspace(Build &b)
{
	Workspace &ws = *b.ws;
	std::vector<BuildUpload> uploads(b.plans.size());
	for (size_t mi = 0; mi < b.plans.size(); mi++) uploads[mi] = BuildUpload{ b.plans[mi].ibytes, b.plans[mi].pbytes };
	BuildLayout &L = b.L;
	if (!rtk_build_layout(b.n, uploads, b.plan.packed, b.plan.tile_mode, b.plan.top_cap, rtk_sort_scratch_words(b.n), &L)) { rtk_set_error("device build: workspace too small (internal error)"); return false; }
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
	b.in_tris = b.at<InTri>(L.in_tris); b.d_cent = b.at<float>(L.cent); b.d_bounds = b.at<uint32_t>(L.bounds);
	b.d_lr = b.at<int2>(L.lr); b.d_range = b.at<uint2>(L.range); b.d_root = b.at<int>(L.root); b.d_bin = b.at<BinNode>(L.bin);
	b.d_tile_count = b.at<uint32_t>(L.tile_count); b.d_tile_base = b.at<uint32_t>(L.tile_base); b.d_tile_nroots = b.at<uint32_t>(L.tile_nroots);
	b.d_depth_word = b.at<uint32_t>(L.depth_word); b.d_area = b.at<float>(L.area); b.d_nodes_tmp = b.at<DevNode>(L.nodes_tmp); b.d_root_list = b.at<int>(L.root_list);
	b.top_aux = TopAux{ b.at<uint4>(L.top_refs), b.at<uint32_t>(L.top_level) };
	// a mesh that already lives in device memory was written by the caller's own work, possibly still in flight on the NULL
	// stream or a blocking stream: that work is waited for here (a build stream of our own does not order itself behind it)
	bool device_mesh = false;
	for (const MeshPlan &pl : b.plans) device_mesh = device_mesh || pl.pos_on_device || pl.idx_on_device;
	if (device_mesh && hipStreamSynchronize(0) != hipSuccess) return b.fail("hipStreamSynchronize(0)");
	b.stage("workspace");
	return true;
}

// ---- finish: the one wait for both streams (the workspace is handed back when run_stages returns), the scene's view ----
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
	b.plan = plan_build(b.n, b.knobs, force_bits);
	rtk_sah_costs(&b.bp.cost_node, &b.bp.cost_tri);
	b.bp.max_leaf = b.knobs.max_leaf;
	b.ws = &g_workspace[b.device];
	std::lock_guard<std::mutex> ws_lock(b.ws->mutex);      // held to the end: every exit below has waited for what it enqueued (Build::give_up, finish)
	if (!prepare_workspace(b) || !(b.from ? ingest_scene(b) : ingest(b)) || !keys_and_sort(b) || !emit(b) || !refit(b)) return nullptr;
	alloc_node_estimate(b);
	if (b.plan.tile_mode && !collapse_tiles(b)) return nullptr;
	if (!b.tiles_done && !collapse_levels(b)) return nullptr;
	if (!finish(b)) return nullptr;

	*narrow_key = plan_key_too_narrow(b.plan, b.equal_codes, b.n);
	if (b.knobs.timing) fprintf(stderr, "rtk_amd build: %u key bits, %u of %u sorted neighbours share a code%s\n", b.plan.packed ? b.plan.packed_bits : BUILD_KEY_BITS, b.equal_codes, b.n,
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
	if (!plan_mesh_base(desc, &b.mesh_base)) { rtk_set_error("rtk_dev_scene_build: more than 2^30 triangles"); return nullptr; }
	b.n = (uint32_t)b.mesh_base.back();
	if (desc->log_fn) desc->log_fn(desc->log_user, nullptr, "rtk_amd: device LBVH build");
	b.t_begin = b.t_last = std::chrono::steady_clock::now();
	if (hipGetDevice(&b.device) != hipSuccess) { b.fail("hipGetDevice"); return nullptr; }
	if (b.device < 0 || b.device >= RTK_MAX_DEVICES) { rtk_set_error("rtk_dev_scene_build: device %d out of range", b.device); return nullptr; }
	b.num_cus = cached_cu_count(b.device);
	// (host only; everything that can be wrong with the description is found here)
	MeshPlans planned = plan_meshes(desc, placements, b.n, rtk_is_device_ptr);
	if (!planned.ok) { rtk_set_error("%s", planned.error); return nullptr; }
	b.plans = std::move(planned.plans);
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
	*key_bits = b.plan.packed ? b.plan.packed_bits : BUILD_KEY_BITS;
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
