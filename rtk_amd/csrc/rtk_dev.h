// rtk_dev.h -- internal: device-side BVH layout and the host-side scene object.
//
// Data layout in HBM (DESIGN.md "Device layout"):
//   DevNode  128 B = one L2 cache line: the reference's 4-wide SoA box block verbatim
//            (rtk.c:69-74: bounds_x/y/z[min|max][slot]) followed by four 32-bit child
//            references instead of four 64-bit byte offsets.
//   DevTri   48 B = three float4: the three vertex positions pre-gathered (the reference
//            chases leaf -> u8 index -> 16 B vertex, rtk.c:215-228), with the global
//            primitive id and the end-of-leaf flag riding in the w lanes.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <chrono>
#include <mutex>
#include <optional>
#include <vector>

#include "rtk.h"
#include "rtk_amd.h"
#include "rtk_carve.h"
#include "rtk_node.h"       // DevNode, DevNodeQ, RTK_REF_NONE, RTK_REF_LEAF
#include "rtk_scene_mem.h"
#include "rtk_launch_scratch.h"   // LaunchScratch, ScratchSets

#define RTK_MAX_DEVICES 64       // per-device tables (workspaces, cached properties)
#define RTK_TRI_LAST 1u           // DevTri.flags: last triangle of its leaf
// Per-launch scratch words: [0] ray pool head, [1..9] visit counters, then RTK_QUEUES work-queue
// heads, each on its own 128-byte line (one word serves only ~88 atomics/us on MI355X).
#define RTK_QUEUES 8
#define RTK_QUEUE_WORD(q) (16 + 16 * (q))
#define RTK_COUNTER_WORDS (16 + 16 * RTK_QUEUES)
// non-zero: a traversal stack overflowed (cannot happen for a validated tree). One word past the ones a launch clears: it
// stays set until rtk_trace_status has reported it.
#define RTK_ERROR_WORD RTK_COUNTER_WORDS
// ... and behind it the words of the image look (rtk_detect.hip)
#define RTK_DETECT_WORDS 4
#define RTK_DETECT_WORD (RTK_ERROR_WORD + 1)

// 48 B of payload at a stride of RTK_TRI_STRIDE bytes. At 48 a record straddles two 128-B lines three times in
// eight (and two 64-B scalar-cache lines every other time); at 64 it never does, for 16 B more per triangle.
#ifndef RTK_TRI_STRIDE
#define RTK_TRI_STRIDE 48
#endif
struct DevTri {
	float v0[3]; uint32_t prim;   // global primitive id
	float v1[3]; uint32_t flags;  // RTK_TRI_LAST | mesh index << 8
	float v2[3]; uint32_t spare;  // first record of a leaf: number of triangles in the leaf
#if RTK_TRI_STRIDE == 64
	uint32_t pad[4];
#endif
};
static_assert(sizeof(DevTri) == RTK_TRI_STRIDE, "triangle record stride");

// A few words per scene that kernels read and k_quantize writes (device memory).
struct DevSceneConsts {
	float bound_abs;           // no plane of any node lies farther than this from the origin on its axis (>= 1: empty slots carry +1 / -1)
	uint32_t qnode_misfits;    // nodes whose child boxes do not fit the 8-bit grid (non-finite extents): the scene then keeps to its exact nodes
	float bound_raw;           // the same bound without the floor of 1 (the per-lane assembly kernels' slab margin is relative to it: a scene 1e-6 wide keeps a 1e-12 margin)
	uint32_t reserved;
};

// Everything a kernel needs to know about a scene (passed by value).
struct DevSceneView {
	const DevSceneConsts *consts;
	const DevNode *nodes;
	const DevNodeQ *qnodes;        // same tree, compressed boxes (may be NULL)
	const DevTri *tris;
	const uint32_t *vertex_index;  // [3*slot+k] original vertex index (rtk_vertex.index)
	const uint32_t *prim_slot;     // [prim] -> triangle slot
	const uint32_t *slot_mesh;     // [slot] -> mesh_index
	const uint32_t *slot_tri;      // [slot] -> triangle_index (per mesh)
	uint32_t num_nodes;
	uint32_t num_tris;
	uint32_t num_prims;
};

// What a refit needs besides the scene (rtk_refit.hip): the node numbers grouped by HEIGHT (0: every child is a leaf or
// empty; else 1 + the largest height among the inner children), so that one launch per height finds its children's boxes
// written by an earlier launch. The device arrays are entries of rtk_dev_scene::mem.
struct RefitSchedule {
	bool ready = false;
	uint32_t *d_order = nullptr;               // [num_nodes] node numbers, by height, by number inside a height
	uint32_t *d_level_start = nullptr;         // [heights + 1] where each height begins in d_order
	std::vector<uint32_t> level_start;         // the same on the host
	void *d_meshes = nullptr;                  // [num_meshes] where each mesh's positions are read from (filled per refit)
	bool max_vertex_ready = false;
	std::vector<uint32_t> max_vertex;          // [num_meshes] largest vertex index the mesh's triangles use (made when a mesh first arrives in host memory)
	void reset(SceneMem &mem);                 // gives the device arrays back (rtk_refit.hip); max_vertex holds for any tree over the same triangles and stays
};

// What a refit of SOME meshes needs on top of the schedule (rtk_dev_scene_refit_meshes): who is above a node, which node holds
// a slot's leaf, every mesh's slots, and the memory of the per-call dirty set. Made by the first such call of a scene, one
// entry of rtk_dev_scene::mem; 12 B per node and 8 B per triangle.
#define RTK_DIRTY_BLOCK 1024u                  // entries of d_order one workgroup of the compaction counts and scatters
struct RefitPartial {
	bool ready = false;
	uint32_t *d_parent = nullptr;              // [num_nodes] the node whose child word names this one (RTK_REF_NONE: the root)
	uint32_t *d_slot_node = nullptr;           // [num_tris] the node whose child word is the leaf that holds the slot
	uint32_t *d_mesh_slots = nullptr;          // [num_tris] slot numbers grouped by mesh, ascending inside one; mesh m's begin at mesh_base[m]
	uint32_t *d_dirty = nullptr;               // [num_nodes] == epoch: boxes of this node are remade by the running call
	uint32_t *d_list = nullptr;                // [num_nodes] the dirty nodes in the order of d_order
	uint32_t *d_block = nullptr;               // [blocks + 1] dirty entries per RTK_DIRTY_BLOCK entries of d_order, then their running sums; [blocks] = all
	uint32_t *d_list_start = nullptr;          // [heights + 1] where each height begins in d_list
	void *d_ranges = nullptr;                  // [num_meshes + 1] runs of listed meshes in d_mesh_slots (filled per call)
	uint32_t epoch = 0;                        // of the last call (0: none yet; d_dirty starts cleared)
	void reset(SceneMem &mem);                 // gives the tables back (rtk_refit.hip)
};

// What rtk_dev_scene_quality keeps per scene (rtk_quality.hip): its partial records and result slot on the device, made by the
// first measurement and an entry of rtk_dev_scene::mem, and the cost the scene had before any refit.
struct QualityState {
	void *d_mem = nullptr;                     // QUALITY_BLOCKS records and one result: the size does not follow the tree, so RTK_FORGET_TREE keeps it
	bool refitted = false;                     // a refit of the scene has succeeded (set by the refit, read by the measurement)
	bool baseline_known = false;               // a measurement was made before any refit ...
	double sah_cost_at_build = 0.0;            // ... and gave this cost
};

// The table of pseudonormals behind rtk_dev_signed_distances (rtk_sign.hip, the rule: rtk_sign_rule.h): 18 floats per primitive,
// indexed by the global primitive id, made from the positions of the triangle records on first use, one entry of
// rtk_dev_scene::mem. The diagnostics of its making are kept with it. Under sign_mutex.
struct SignTable {
	float *d_table = nullptr;                  // [18 * num_prims]; NULL: not made (or dropped by RTK_FORGET_BOXES)
	rtk_dev_sign_info info = {};               // as the making left it (table_ms: of that making)
};

// The moments behind rtk_dev_winding_numbers (rtk_winding.hip, the rule: rtk_winding_rule.h): one record per DevNode at the same
// index, so that a node step of the walk reads this one 128-byte line and never the node's boxes. Per child slot the area vector
// N, the centre P and the radius R of everything under it; then a copy of the node's child words.
struct DevWinding {
	float nx[4], ny[4], nz[4];
	float px[4], py[4], pz[4];
	float r[4];
	uint32_t child[4];
};
static_assert(sizeof(DevWinding) == 128, "one record of moments per node, one 128 B line");
// The table: made from positions and from the tree on first use, one entry of rtk_dev_scene::mem. Under winding_mutex.
struct WindingTable {
	DevWinding *d_table = nullptr;             // [num_nodes]; NULL: not made (or dropped by any RTK_FORGET_*)
	rtk_dev_winding_info info = {};            // as the making left it (table_ms: of that making)
};

// One instance of a world (rtk_world.hip, the rules: rtk_world_rule.h): the inverse of its placement row by row, the scene it places
// and its flags (bit 0: dead -- the placement is not invertible, its scene has no triangles or its world box is not finite).
// Half a 128-byte line, read by a ray only when it enters the instance's box.
struct DevWorldInstance {
	float inv[12];
	uint32_t scene, flags;
	uint32_t pad[2];
};

static inline void *rtk_dev_malloc(size_t bytes) { void *p = nullptr; return hipMalloc(&p, bytes) == hipSuccess ? p : nullptr; }
static inline void rtk_dev_free(void *p) { (void)hipFree(p); }

// The tree a scene holds now, as far as the host describes it besides the view. THE RULE: a host field that a rebuild must replace
// is a member of SceneTree, and nowhere else. A build, an upload and a split fill the record; rtk_dev_scene_rebuild replaces view
// and tree as wholes, so a member added here cannot be forgotten there. Whoever writes a member the trace path reads (bound_abs,
// bound_raw, big_leaf_fraction, max_depth, qnodes_mem) does so under scratch_mutex, like the view.
struct SceneTree {
	uint32_t max_depth = 0;
	uint32_t first_top = 0;                // device build, tile collapse: nodes [1, first_top) are the tiles', 0 and [first_top, n) the ones above them (0: one run)
	uint32_t first_split = 0;              // rtk_dev_scene_split_leaves: nodes [first_split, n) were appended by a split, each after its parent (0: none)
	double big_leaf_fraction = 0.0;        // leaves of more than three triangles (uploads; device builds make ~none): the assembly packet kernel hands those tiles back
	DevSceneConsts consts_readback = {};   // filled by the stream that ran k_quantize; read by rtk_quantize_finish after its synchronisation
	float bound_abs = 0.0f, bound_raw = 0.0f;
	const DevNodeQ *qnodes_mem = nullptr;      // the compressed array, also while view.qnodes is NULL (a misfit): the next refit fills it again
	bool boxes_exact = false;                  // every box is known to be the exact union of what is below it (a device build, a full refit; not an upload)
	const uint32_t *d_vidx_in = nullptr;       // [3 * prim + k] original vertex indices in input order; NULL: every mesh has implicit indices
	const unsigned long long *d_mesh_base = nullptr;   // num_meshes + 1, on the device (made by a build or a rebuild; NULL: a blob as it was uploaded)
	uint32_t stack_entries() const { return 3u * max_depth + 1u; }   // traversal stack entries a ray can need: at most three pushes per level of descent
	float bound_floor1() const { return bound_abs > 1.0f ? bound_abs : 1.0f; }   // what the packet kernels' slab margins are relative to (empty slots carry +1 / -1)
};

const ScratchHooks &rtk_scratch_hooks();       // hipMalloc / hipFree / hipStreamSynchronize (rtk_launch.hip)

struct rtk_dev_scene {
	int device = 0;
	DevSceneView view = {};
	SceneTree tree;
	// what describes calls, the input or derived tables, not the tree
	std::vector<uint64_t> mesh_base;  // num_meshes + 1
	double build_ms = 0.0;
	// owned device allocations, and what each adds to total_device_bytes (rtk_scene_mem.h)
	SceneMem mem{ rtk_dev_malloc, rtk_dev_free };
	// per-stream launch scratch, created on first use (rtk_launch_scratch.h); the mutex covers the collection and the enqueue of a launch
	std::mutex scratch_mutex;
	ScratchSets scratch{ rtk_scratch_hooks() };
	int num_cus = 0;
	// Device-built scenes make the four side arrays of the view (vertex_index, prim_slot, slot_mesh, slot_tri: what the expansion of
	// hit records, the validator and the exporter read -- never a traversal) on first use, not in every build: 52 of the 100
	// bytes per triangle the build's emit kernel wrote, one of them scattered (rtk_scene_side_arrays, rtk_build_refit.hip).
	// RTK_FORGET_TREE keeps them: they go by slot and primitive, not by node, and the split kernel moves their entries with the
	// triangle records it reorders (k_split_leaves<true>, under side_mutex). RTK_FORGET_SLOTS drops them (a rebuild: every slot changes).
	std::mutex side_mutex;
	bool side_ready = true;                    // (uploads arrive with the arrays)
	// Refits (rtk_refit.hip). The schedule is made by the first one and kept, like the side arrays; none of it is in the view
	// the traversals copy.
	std::mutex refit_mutex;                    // one pass over a scene at a time (ScenePass); covers the schedule
	RefitSchedule refit;
	double refit_ms = 0.0;                     // wall time inside the last rtk_dev_scene_refit / rtk_dev_scene_refit_meshes
	RefitPartial partial;
	uint64_t refit_nodes = 0;                  // nodes whose boxes the last successful refit remade
	uint32_t partial_readback = 0;             // the dirty count of a partial refit, brought home with the constants
	QualityState quality;                      // under refit_mutex, like the schedule
	// Signed distances (rtk_sign.hip). The table goes by primitive id and is made from positions: RTK_FORGET_BOXES drops it,
	// RTK_FORGET_TREE and RTK_FORGET_SLOTS keep it. records_once: every primitive id is named by exactly one triangle record (a
	// device build and a rebuild always; an upload counts, on the host) -- what the making of the table needs.
	std::mutex sign_mutex;
	SignTable sign;
	bool records_once = true;
	// Winding numbers (rtk_winding.hip). The table goes by node and is made from positions: every RTK_FORGET_* drops it.
	std::mutex winding_mutex;
	WindingTable winding;
};
// makes the side arrays if they are not there yet (synchronises `stream` the one time it has to work)
int rtk_scene_side_arrays(const rtk_dev_scene *ds, hipStream_t stream);
// What was derived from the scene and no longer holds is dropped here, and only here (rtk_capi.hip); whoever needs a table
// again makes it again. A new derived table is added to this function and nowhere else.
#define RTK_FORGET_BOXES 1u       // boxes moved, the topology stayed (a refit): the export plan; a cost measured from now on is not the build's; the table of pseudonormals (vertices moved: it is made from positions)
#define RTK_FORGET_TREE 2u        // nodes or slots were renumbered (a split): the refit schedule, the partial refit's tables, the export plan, the cost at build. Keeps the table of pseudonormals: it goes by primitive id
#define RTK_FORGET_SLOTS 4u       // every record changed its slot (a rebuild): the four side arrays, made again on first use. The caller holds side_mutex. Keeps the table of pseudonormals: records moved, not vertices
// Each of the three also drops the table of winding moments: it is made from positions (BOXES) and goes by node (TREE, SLOTS).
void rtk_scene_forget_derived(rtk_dev_scene *ds, unsigned what);

// -- error plumbing (rtk_capi.hip) --
void rtk_set_error(const char *fmt, ...);
#define RTK_HIP_CHECK(expr, ret)                                                         \
	do {                                                                                 \
		hipError_t e_ = (expr);                                                          \
		if (e_ != hipSuccess) {                                                          \
			rtk_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
			return ret;                                                                  \
		}                                                                                \
	} while (0)

// A pass over a scene that is not a trace (refit, split, measurement) fails like this: OOM is told apart, the rest is HIP's.
#define RTK_PASS_CHECK(who, expr)                                                                    \
	do {                                                                                             \
		hipError_t e_ = (expr);                                                                      \
		if (e_ != hipSuccess) {                                                                      \
			rtk_set_error(who ": %s failed: %s (line %d)", #expr, hipGetErrorString(e_), __LINE__);  \
			return e_ == hipErrorOutOfMemory ? RTK_AMD_ERR_OOM : RTK_AMD_ERR_HIP;                    \
		}                                                                                            \
	} while (0)
// ... and runs with the scene's device current: switched to here, switched back when the scope ends.
struct SceneDeviceScope {
	int before = 0, device; hipError_t err;
	explicit SceneDeviceScope(const rtk_dev_scene *ds) : device(ds->device)
	{
		err = hipGetDevice(&before);
		if (err == hipSuccess && before != device) err = hipSetDevice(device);
		if (err != hipSuccess) { rtk_set_error("scene on device %d: %s", device, hipGetErrorString(err)); before = device; }
	}
	SceneDeviceScope(const SceneDeviceScope &) = delete;
	~SceneDeviceScope() { if (before != device) (void)hipSetDevice(before); }
	bool ok() const { return err == hipSuccess; }      // false: rtk_set_error has been called, nothing was switched
};
// The frame of such a pass: from its construction the clock runs and refit_mutex is held, to the end of the scope. The scene's
// device becomes current when the entry point asks for it (on_device), not with the lock: what a call refuses or answers from
// the host fields alone touches no HIP. end() is the way out once work may be enqueued: a failed pass leaves nothing running on
// the caller's stream, which may still read the call's tables.
struct ScenePass {
	const std::chrono::steady_clock::time_point t_begin = std::chrono::steady_clock::now();
	std::lock_guard<std::mutex> lock;
	rtk_dev_scene *const ds; const hipStream_t stream;       // (the caller's)
	std::optional<SceneDeviceScope> scope;
	ScenePass(rtk_dev_scene *ds, void *stream) : lock(ds->refit_mutex), ds(ds), stream((hipStream_t)stream) {}
	bool on_device() { scope.emplace(ds); return scope->ok(); }      // false: the call returns RTK_AMD_ERR_NO_DEVICE
	int end(int rc) { if (rc != RTK_AMD_OK && scope && scope->ok()) (void)hipStreamSynchronize(stream); return rc; }
	double ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count(); }
};

// -- upload (rtk_upload.hip) --
struct HostBvh {
	std::vector<DevNode> nodes;
	std::vector<DevTri> tris;
	std::vector<uint32_t> vertex_index;
	std::vector<uint32_t> slot_mesh, slot_tri;
	std::vector<uint64_t> mesh_base;
	uint32_t max_depth = 0;
};
int rtk_blob_to_host_bvh(const rtk_scene *scene, size_t avail, HostBvh *out);
rtk_dev_scene *rtk_dev_scene_from_host_bvh(const HostBvh &h);

// -- compressed node array (rtk_quant.hip): fills ds->view.qnodes from ds->view.nodes on `stream` --
// src: read the exact nodes from there and store them to ds->view.nodes as well; dst: compressed array the caller allocated
// Also writes every node's child order words and the scene constants (DevSceneConsts, allocated here). bound_hint: a bound of
// |plane| over all nodes the caller already knows (uploads: computed on the host, boxes of a blob need not nest); the root's
// own planes are always taken in.
// only_first: finish just the first so many nodes (the device build's tile collapse has finished the others itself);
// keep_consts: the constants block is already set up (rtk_scene_consts) and holds counts that must survive.
int rtk_quantize_nodes(rtk_dev_scene *ds, hipStream_t stream, const DevNode *src = nullptr, DevNodeQ *dst = nullptr, float bound_hint = 0.0f,
	uint32_t only_first = 0xffffffffu, bool keep_consts = false, bool readback = true);   // (bound_hint: 0 = none; the floor of 1 is applied inside; readback: enqueue the copy of the constants to the host -- the device build brings them home with its other results)
int rtk_scene_consts(rtk_dev_scene *ds, hipStream_t stream);
// The same finish for the nodes list[0 .. *d_count) only (a refit of some meshes): compressed node and order words of each, the
// constants' bounds if the root is among them, misfits among them counted. The constants block is cleared first; the copy of
// the constants to the host is enqueued. The compressed array is ds->tree.qnodes_mem.
int rtk_quantize_node_list(rtk_dev_scene *ds, hipStream_t stream, const uint32_t *list, const uint32_t *d_count);
void rtk_quantize_finish(rtk_dev_scene *ds);   // after that stream has been synchronised

// -- the build workspace lent to another pass, helpers shared with the build (rtk_build.hip; its stages: rtk_build_internal.h) --
// The workspace of a device, at least `bytes` large, lent to a pass that is not a build (rtk_refit.hip: the temporaries of the
// schedule, host-resident positions staged as a build stages them). Builds on the device wait while it is out; whatever the
// borrower enqueued on the memory must have completed before release() (the destructor).
struct WorkspaceLoan {
	int device = -1;
	char *base = nullptr;
	WorkspaceLoan() = default;
	WorkspaceLoan(const WorkspaceLoan &) = delete;
	WorkspaceLoan &operator=(const WorkspaceLoan &) = delete;
	~WorkspaceLoan() { release(); }
	bool take(int device, size_t bytes);       // false: nothing is held (out of device memory; rtk_set_error says so)
	void release();
};
bool rtk_is_device_ptr(const void *p);         // hipMalloc'ed memory?
void rtk_export_forget(const rtk_dev_scene *ds);   // the scene's cached export plan, if any (rtk_export.hip)
// the two constants of the surface area heuristic, for the builder that splits by them and for rtk_dev_scene_quality that
// measures by them: 0.5 per node visited, 1.0 per triangle tested, RTK_AMD_SAH_CN / RTK_AMD_SAH_CT override (rtk_build.hip; the
// defaults and the environment: rtk_build_plan.h)
void rtk_sah_costs(float *cost_node, float *cost_tri);
// RTK_AMD_MAX_LEAF, 1 .. 63, default 3: the device builder's leaf limit, and what rtk_dev_scene_split_leaves takes for max_leaf 0
uint32_t rtk_build_max_leaf();
// a blob that rtk_finish_build_to exported from `ds` takes the scene over as its resident device copy (rtk_host_calls.hip)
void rtk_cache_adopt(const rtk_scene *scene, rtk_dev_scene *ds);

// -- radix sort shared with the builder (rtk_sort.hip) --
size_t rtk_sort_scratch_words(uint32_t n);
bool rtk_sort_pairs_async(unsigned long long *keys_a, unsigned long long *keys_b, uint32_t *vals_a, uint32_t *vals_b,
	uint32_t n, uint32_t key_bits, uint32_t *scratch, hipStream_t stream);
bool rtk_sort_words_async(unsigned long long *keys_a, unsigned long long *keys_b, uint32_t n, uint32_t first_bit, uint32_t last_bit,
	uint32_t *scratch, hipStream_t stream);

// -- trace launches (rtk_launch.hip) --
// One launch: every field starts as "not given", a caller sets the ones it means.
struct TraceCall {
	const rtk_ray *rays = nullptr;
	size_t n = 0;
	rtk_hit_record *hits = nullptr;            // closest hit: one record per ray
	uint8_t *occluded = nullptr;               // any hit: one byte per ray
	const rtk_trace_opts *opts = nullptr;
	hipStream_t stream = nullptr;
	bool any_hit = false;
	rtk_trace_counters *counted = nullptr;     // rtk_dev_trace_rays*_counted (synchronises the stream)
	const rtk_dev_filter *filter = nullptr;
	rtk_hit_record *cand = nullptr;            // collect the cand_k closest candidates per ray (host-callback filters) ...
	uint32_t *cand_count = nullptr;            // ... and how many of them are valid
	uint32_t cand_k = 0;
	rtk_packet_counters *pk_counted = nullptr; // rtk_dev_trace_rays_packet_counted (synchronises the stream)
	const rtk_ray_list *list = nullptr;        // rtk_dev_trace_rays*_listed have checked it; n is the size of the arrays, below 2^32
};
// what every batch call says; the rest of a TraceCall stays "not given" unless the entry point means it
inline TraceCall batch_call(const rtk_ray *d_rays, size_t n, const rtk_trace_opts *opts, void *stream)
{
	TraceCall c;
	c.rays = d_rays; c.n = n; c.opts = opts; c.stream = (hipStream_t)stream;
	return c;
}
int rtk_launch_trace(const rtk_dev_scene *ds, const TraceCall &call);
// the scene's memory, its scratch and the stream must all belong to the device this thread has current: a launch from a
// thread on another GPU would read the scene across devices (a fault without peer access). false: rtk_set_error has said so
bool rtk_on_scene_device(const rtk_dev_scene *ds, const char *caller);
// the launch-error word of (scene, stream), or NULL: nothing was launched there yet. Takes scratch_mutex.
unsigned long long *rtk_error_word(rtk_dev_scene *ds, hipStream_t stream);
// the entry-list pre-pass of a w x h frame alone; host_out receives (w / 64) * (h / 64) PkBlockEntries records (rtk_trace_shared.h). Synchronous.
int rtk_debug_packet_entries(const rtk_dev_scene *ds, const rtk_ray *d_rays, uint32_t image_w, uint32_t image_h, uint32_t target, uint32_t max_levels, void *host_out);
int rtk_trace_status(const rtk_dev_scene *ds, hipStream_t stream);
void rtk_scene_drop_stream(rtk_dev_scene *ds, hipStream_t stream);   // the stream is about to be destroyed (and has been synchronised)
// -- rtk_dev_trace_rays_count / rtk_dev_trace_rays_all (rtk_launch.hip; the kernel: rtk_allhits.hip) --
// counts: the count form; else the fill form (offsets, records, written or NULL)
int rtk_launch_allhits(const rtk_dev_scene *ds, const rtk_ray *d_rays, size_t n, uint32_t *d_counts, const uint64_t *d_offsets,
	rtk_hit_record *d_records, uint32_t *d_written, bool fill, const rtk_dev_filter *filter, const rtk_trace_opts *opts, hipStream_t stream);
// -- rtk_dev_select_rays (rtk_select.hip) --
int rtk_launch_select(rtk_dev_scene *ds, const void *d_src, uint32_t kind, size_t num_rays, const rtk_ray_list *in, uint64_t *d_out_ids,
	uint64_t *d_out_count, hipStream_t stream);
// -- rtk_dev_closest_points (rtk_closest.hip) --
int rtk_launch_closest(const rtk_dev_scene *ds, const rtk_point_query *d_queries, size_t num_queries, const rtk_ray_list *list,
	rtk_closest_record *d_records, float *d_points, hipStream_t stream, rtk_trace_counters *counted = nullptr);   // counted: synchronises the stream
// -- rtk_dev_signed_distances (rtk_sign.hip) --
// the table of pseudonormals, made if it is not there (synchronises `stream` the one time it has to work); ds->sign.d_table after RTK_AMD_OK
int rtk_scene_pseudonormals(const rtk_dev_scene *ds, hipStream_t stream);
// rtk_launch_closest as it is, then the epilogue that writes d_signed on the same stream
int rtk_launch_signed(const rtk_dev_scene *ds, const rtk_point_query *d_queries, size_t num_queries, const rtk_ray_list *list,
	rtk_closest_record *d_records, float *d_points, float *d_signed, hipStream_t stream);
// -- rtk_dev_winding_numbers (rtk_winding.hip) --
// the table of moments, made if it is not there (synchronises `stream` the one time it has to work); ds->winding.d_table after RTK_AMD_OK
int rtk_scene_winding_table(const rtk_dev_scene *ds, hipStream_t stream);
// counted: synchronises the stream
int rtk_launch_winding(const rtk_dev_scene *ds, const rtk_point_query *d_queries, size_t num_queries, const rtk_ray_list *list,
	const rtk_winding_opts *opts, float *d_winding, hipStream_t stream, rtk_trace_counters *counted = nullptr);
// -- rtk_dev_triangles_within_count / rtk_dev_triangles_within_all (rtk_within.hip) --
// fill: offsets, records, points or NULL, d_counts the written numbers or NULL; else d_counts the counts. counted: synchronises the stream
int rtk_launch_within(const rtk_dev_scene *ds, const rtk_point_query *d_queries, size_t num_queries, const rtk_ray_list *list,
	uint32_t *d_counts, const uint64_t *d_offsets, rtk_closest_record *d_records, float *d_points, bool fill, hipStream_t stream,
	rtk_trace_counters *counted = nullptr);
// -- rtk_dev_triangles_in_box_count / rtk_dev_triangles_in_box_all (rtk_box.hip) --
// fill: offsets, prims, d_counts the written numbers or NULL; else d_counts the counts. counted: synchronises the stream
int rtk_launch_box(const rtk_dev_scene *ds, const rtk_box_query *d_boxes, size_t num_queries, const rtk_ray_list *list,
	uint32_t *d_counts, const uint64_t *d_offsets, uint32_t *d_prims, bool fill, hipStream_t stream, rtk_trace_counters *counted = nullptr);
// -- rtk_dev_triangles_in_obb_count / rtk_dev_triangles_in_obb_all (rtk_obb.hip) --
// as rtk_launch_box, every query with axes of its own
int rtk_launch_obb(const rtk_dev_scene *ds, const rtk_obb_query *d_obbs, size_t num_queries, const rtk_ray_list *list,
	uint32_t *d_counts, const uint64_t *d_offsets, uint32_t *d_prims, bool fill, hipStream_t stream, rtk_trace_counters *counted = nullptr);
// -- rtk_dev_triangles_touching_count / rtk_dev_triangles_touching_all (rtk_touch.hip) --
// as rtk_launch_box, with the filter (or NULL)
int rtk_launch_touch(const rtk_dev_scene *ds, const rtk_tri_query *d_tris, size_t num_queries, const rtk_ray_list *list,
	const rtk_touch_filter *filter, uint32_t *d_counts, const uint64_t *d_offsets, uint32_t *d_prims, bool fill, hipStream_t stream,
	rtk_trace_counters *counted = nullptr);
// -- rtk_dev_closest_triangles (rtk_pair.hip) --
// counted: synchronises the stream
int rtk_launch_pair(const rtk_dev_scene *ds, const rtk_tri_query *d_tris, size_t num_queries, const rtk_ray_list *list,
	const rtk_touch_filter *filter, const float *d_max_dist2, rtk_closest_record *d_records, float *d_points_query, float *d_points_scene,
	hipStream_t stream, rtk_trace_counters *counted = nullptr);
// -- rtk_dev_triangles_near_count / rtk_dev_triangles_near_all (rtk_near.hip) --
// as rtk_launch_within, with the filter (or NULL), the limits (or NULL) and two point arrays (each or NULL)
int rtk_launch_near(const rtk_dev_scene *ds, const rtk_tri_query *d_tris, size_t num_queries, const rtk_ray_list *list,
	const rtk_touch_filter *filter, const float *d_max_dist2, uint32_t *d_counts, const uint64_t *d_offsets, rtk_closest_record *d_records,
	float *d_points_query, float *d_points_scene, bool fill, hipStream_t stream, rtk_trace_counters *counted = nullptr);
// -- rtk_dev_sweep_spheres / rtk_dev_sweep_spheres_any (rtk_sweep.hip) --
// the closest form writes d_records (d_points, d_centres: each or NULL), the any-hit form d_blocked; a non-null `counted` makes
// it the counting form of the closest one
int rtk_launch_sweep(const rtk_dev_scene *ds, const rtk_sphere_sweep *d_sweeps, size_t num_sweeps, const rtk_ray_list *list,
	rtk_hit_record *d_records, float *d_points, float *d_centres, uint8_t *d_blocked, bool any_hit, const rtk_dev_filter *filter,
	hipStream_t stream, rtk_trace_counters *counted = nullptr);
// -- rtk_dev_sweep_boxes / rtk_dev_sweep_boxes_any (rtk_boxsweep.hip) --
// as rtk_launch_sweep, with centres and normals (each or NULL) as the closest form's arrays
int rtk_launch_boxsweep(const rtk_dev_scene *ds, const rtk_box_sweep *d_sweeps, size_t num_sweeps, const rtk_ray_list *list,
	rtk_hit_record *d_records, float *d_centres, float *d_normals, uint8_t *d_blocked, bool any_hit, const rtk_dev_filter *filter,
	hipStream_t stream, rtk_trace_counters *counted = nullptr);
// -- rtk_dev_sweep_capsules / rtk_dev_sweep_capsules_any (rtk_capsule.hip) --
// as rtk_launch_sweep, with the points on the triangle and on the capsule's axis (each or NULL) as the closest form's arrays
int rtk_launch_capsule(const rtk_dev_scene *ds, const rtk_capsule_sweep *d_sweeps, size_t num_sweeps, const rtk_ray_list *list,
	rtk_hit_record *d_records, float *d_points, float *d_axis_points, uint8_t *d_blocked, bool any_hit, const rtk_dev_filter *filter,
	hipStream_t stream, rtk_trace_counters *counted = nullptr);
// -- rtk_dev_sweep_obbs / rtk_dev_sweep_obbs_any (rtk_obbsweep.hip) --
// as rtk_launch_boxsweep, every query with axes of its own
int rtk_launch_obbsweep(const rtk_dev_scene *ds, const rtk_obb_sweep *d_sweeps, size_t num_sweeps, const rtk_ray_list *list,
	rtk_hit_record *d_records, float *d_centres, float *d_normals, uint8_t *d_blocked, bool any_hit, const rtk_dev_filter *filter,
	hipStream_t stream, rtk_trace_counters *counted = nullptr);
// -- rtk_dev_world_trace_rays / _any / _counted (rtk_world.hip) --
// the closest form writes d_records (d_instances or NULL), the any-hit form d_blocked; a non-null `counted` makes it the counting
// form of the closest one (synchronises the stream)
int rtk_launch_world(const rtk_dev_world *w, const rtk_ray *d_rays, size_t n, const rtk_ray_list *list, const rtk_world_filter *filter,
	rtk_hit_record *d_records, uint32_t *d_instances, uint8_t *d_blocked, bool any_hit, hipStream_t stream, rtk_trace_counters *counted = nullptr);
// -- rtk_dev_world_closest_points / _counted (rtk_world_closest.hip) --
// d_instances, d_points: each or NULL; a non-null `counted` makes it the counting form (synchronises the stream)
int rtk_launch_world_closest(const rtk_dev_world *w, const rtk_point_query *d_queries, size_t n, const rtk_ray_list *list,
	const rtk_world_filter *filter, rtk_closest_record *d_records, uint32_t *d_instances, float *d_points, hipStream_t stream,
	rtk_trace_counters *counted = nullptr);
// -- rtk_dev_world_triangles_in_box_* / _in_obb_* / _touching_* (rtk_world_overlap.hip) --
// fill: offsets, 64-bit entries, d_counts the written numbers or NULL; else d_counts the counts. counted: synchronises the stream
int rtk_launch_world_box(const rtk_dev_world *w, const rtk_box_query *d_boxes, size_t n, const rtk_ray_list *list, const rtk_world_filter *filter,
	uint32_t *d_counts, const uint64_t *d_offsets, uint64_t *d_entries, bool fill, hipStream_t stream, rtk_trace_counters *counted = nullptr);
int rtk_launch_world_obb(const rtk_dev_world *w, const rtk_obb_query *d_obbs, size_t n, const rtk_ray_list *list, const rtk_world_filter *filter,
	uint32_t *d_counts, const uint64_t *d_offsets, uint64_t *d_entries, bool fill, hipStream_t stream, rtk_trace_counters *counted = nullptr);
int rtk_launch_world_touch(const rtk_dev_world *w, const rtk_tri_query *d_tris, size_t n, const rtk_ray_list *list, const rtk_world_filter *filter,
	uint32_t touch_flags, uint32_t *d_counts, const uint64_t *d_offsets, uint64_t *d_entries, bool fill, hipStream_t stream,
	rtk_trace_counters *counted = nullptr);
// -- the look for an image nobody announced (rtk_detect.hip) --
int rtk_detect_image(const rtk_dev_scene *ds, const rtk_ray *d_rays, size_t n, hipStream_t stream, uint32_t *w_out, uint32_t *h_out);
// -- hit records to full hits, and rtk_trace_ray's one-ray launch (rtk_expand.hip) --
// h_status (host-visible): also receives the stream's launch-error word (see rtk_trace_status), or is left alone if the stream has none.
// ticket != 0 and n <= 256: the word becomes (ticket << 32 | error) once every result of the launch is visible to the host.
int rtk_launch_trace_one(const rtk_dev_scene *ds, const rtk_ray *d_ray, rtk_hit *d_hit, uint8_t *d_mask, hipStream_t stream,
	unsigned long long *h_status, uint32_t ticket);
int rtk_launch_expand(const rtk_dev_scene *ds, const rtk_hit_record *d_records, size_t n, rtk_hit *d_hits,
	uint8_t *d_mask, hipStream_t stream, unsigned long long *h_status = nullptr, uint32_t ticket = 0);
