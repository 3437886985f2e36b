// rtk_build_internal.h -- what the files of the device build share, and nothing else includes: the records the kernels hand to
// one another through the workspace, the block sizes, the workspace, `struct Build` (the one thing handed from stage to stage),
// the stage prototypes and the few device helpers that more than one file's kernels use. A kernel lives in the file of the stage
// that launches it (anonymous namespace); the stage function is the only door to it.
//
//   rtk_build.hip           the workspace, prepare_workspace, finish, run_stages, the three entry points
//   rtk_build_ingest.hip    1 ingest (from a description or from a live scene), 2 bounds, 3 morton, 4 sort
//   rtk_build_refit.hip     5 emit, 6 + 7 refit, the side arrays
//   rtk_build_collapse.hip  8 collapse (level by level, and tile-local: the tiles' node counts too, which the refit forks off)
#pragma once

#include "rtk_dev.h"
#include "rtk_build_layout.h"
#include "rtk_build_plan.h"

#include <limits.h>
#include <stdio.h>

#include <chrono>
#include <mutex>
#include <vector>

// (hidden: the stage functions cross translation units, not the library's border)
namespace rtk_bld __attribute__((visibility("hidden"))) {

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

// One decoded triangle in input order: 48 B = three 16-B pieces, so that the gather by sorted order in k_emit_tris
// is three loads from (on average) 1.4 lines instead of twelve from two arrays.
struct InTri {
	float p[9];          // v0.xyz, v1.xyz, v2.xyz
	uint32_t vi[3];      // original vertex indices (rtk_vertex.index)
};
static_assert(sizeof(InTri) == 48, "InTri");

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

#define REFIT_TILE 1024
#define REFIT_BLOCK 1024        // one thread per triangle: every global load of the tile is in flight at once

struct Climb { int cur_ref; int l; int r; };      // cur_ref: >= 0 inner node, < 0 leaf ~slot; INT_MIN: none

#define COLLAPSE_BLOCK 256
#define COLLAPSE_SMALL 1024          // threads of k_collapse_small = children it opens per round
#define COLLAPSE_SMALL_JOBS 64      // largest level it takes: its children (at most four each) are one round
#define COLLAPSE_RING 64
constexpr uint32_t BUILD_KEY_BITS = 63u;     // the Morton code of the (key, index) pair path, whole

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

struct CollapseBufs {
	int *jobs;                // [job] binary node of the job (current level; LDS inside k_collapse_small)
	int4 *dec;                // [job] child words, binary references where info says so
	uint32_t *info;           // [job] inner-children mask << 4 | their number << 8
	uint32_t *sums;           // [job / 256] inner children of those 256 jobs
};

// tile mode (see collapse_open, rtk_build_collapse.hip): per node above the tiles, which tile roots hang in its slots, and its level
struct TopAux { uint4 *tile_refs; uint32_t *level; };

static_assert(sizeof(InTri) == RTK_BUILD_SIZEOF_INTRI && sizeof(BinNode) == RTK_BUILD_SIZEOF_BINNODE && sizeof(Climb) == RTK_BUILD_SIZEOF_CLIMB &&
	sizeof(LevelState) == RTK_BUILD_SIZEOF_LEVELSTATE && sizeof(MeshSrc) == RTK_BUILD_SIZEOF_MESHSRC && sizeof(DevNode) == RTK_BUILD_SIZEOF_DEVNODE,
	"rtk_build_layout.h sizes the workspace by these");
static_assert(REFIT_TILE == RTK_BUILD_REFIT_TILE && COLLAPSE_BLOCK == RTK_BUILD_COLLAPSE_BLOCK && COLLAPSE_RING == RTK_BUILD_COLLAPSE_RING, "rtk_build_layout.h");

static_assert(COLLAPSE_SMALL_JOBS == RTK_BUILD_COLLAPSE_SMALL_JOBS, "rtk_build_layout.h");

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

// ---- one build: what its stages share ----
struct Build {
	// where the triangles come from: a description (rtk_dev_scene_build), or the records of a live scene (rtk_dev_scene_rebuild).
	// Only the planning of the meshes and the two ingests look at it; from there on a build knows the number of meshes and mesh_base.
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
	BuildPlan plan;                   // what n and the knobs decide (rtk_build_plan.h)
	// the workspace (its mutex is held by run_stages), the two streams, the scene under construction
	Workspace *ws = nullptr;
	hipStream_t bs = nullptr;         // the build's stream
	hipStream_t cs = nullptr;         // where the tiles' own kernels run: ws->side once it has forked off, else bs
	bool forked = false;
	bool side_busy = false;           // kernels on ws->side may still be reading the workspace
	BuildResults *results = nullptr;
	rtk_dev_scene *ds = nullptr;
	// the layout (byte offsets) and the pointers into it that more than one stage uses (a stage takes the others with at<T>(L.x)
	// where it launches); what else the stages hand on
	BuildLayout L;
	InTri *in_tris = nullptr;
	float *d_cent = nullptr, *d_area = nullptr;
	uint32_t *d_bounds = nullptr, *d_tile_count = nullptr, *d_tile_base = nullptr, *d_depth_word = nullptr, *d_tile_nroots = nullptr;
	int2 *d_lr = nullptr;
	uint2 *d_range = nullptr;
	int *d_root = nullptr, *d_root_list = nullptr;
	BinNode *d_bin = nullptr;
	DevNode *d_nodes_tmp = nullptr;
	TopAux top_aux = { nullptr, nullptr };    // tile mode: the tile-root and level words of the nodes above the tiles (else NULL)
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
	// workspace (the next build on this device reuses it as soon as run_stages lets go of the workspace mutex) and the scene's
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

// ---- the stages, in the order run_stages calls them; each returns what Build::fail returns (false) when it gives up ----
bool ingest(Build &b);                      // rtk_build_ingest.hip
bool ingest_scene(Build &b);
bool keys_and_sort(Build &b);
bool emit(Build &b);                        // rtk_build_refit.hip
bool refit(Build &b);
void count_tiles(Build &b);                 // rtk_build_collapse.hip (tile mode; called by refit between its two passes)
void alloc_node_estimate(Build &b);
bool collapse_tiles(Build &b);
bool collapse_levels(Build &b);
// a scene of fewer than two triangles, on the host (rtk_build_ingest.hip)
rtk_dev_scene *build_tiny(const rtk_scene_desc *desc, const std::vector<uint64_t> &mesh_base, const rtk_placement *placements);

// ---- device helpers of more than one file ----
// (static: internal to each file that includes them, as the kernels that use them are)

static __device__ __forceinline__ float half_area(const float mn[3], const float mx[3])
{
	const float x = mx[0] - mn[0], y = mx[1] - mn[1], z = mx[2] - mn[2];
	return x * y + y * z + z * x;
}

static __device__ __forceinline__ void tri_box(const DevTri *tris, uint32_t s, float mn[3], float mx[3])
{
	const DevTri &t = tris[s];
#pragma unroll
	for (int a = 0; a < 3; a++) {
		mn[a] = fminf(fminf(t.v0[a], t.v1[a]), t.v2[a]);
		mx[a] = fmaxf(fmaxf(t.v0[a], t.v1[a]), t.v2[a]);
	}
}

} // namespace rtk_bld
