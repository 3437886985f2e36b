// rtk_trace_shared.h -- pieces shared by the two traversal kernels (rtk_trace.hip: one ray
// per lane; rtk_trace_packet.hip: one 8x8 tile per wave) and the launch code that feeds them (rtk_launch.hip).
#pragma once

#include "rtk_dev.h"
#include "rtk_trace_plan.h"

#include <stddef.h>
#include <mutex>

#define WAVES_PER_BLOCK TRACE_WAVES_PER_BLOCK
#define BLOCK_THREADS TRACE_BLOCK_THREADS

struct TraceParams {
	DevSceneView sc;
	const rtk_ray *rays;
	rtk_hit_record *hits;
	uint8_t *occluded;
	unsigned long long *counter;   // [0] pool head, [1..6] visit counters
	uint2 *spill;
	unsigned long long n;
	uint32_t spill_stride;         // lanes in the launch
	uint32_t spill_cap;            // entries per lane in spill
	uint32_t image_w, image_h;     // 0 = no tiling
	uint32_t refill_min;
	uint32_t dynamic;
	uint32_t node_exit;            // leave the node loop when fewer lanes than this still need node steps and a leaf is waiting
	const unsigned long long *perm; // optional: trace rays in this order (sorted words of the ray reordering, ray number in the low 32 bits); results go to the ray's own slot
	// built-in candidate filters (rtk_dev_filter, FILT kernels only); all optional
	const rtk_hit_record *after;   // per ray: only candidates that come after (t, prim) in (t, prim) order
	const uint32_t *ignore_prim;   // per ray: global primitive id that is never a candidate
	const uint32_t *mesh_mask;     // bit m set = triangles of mesh m are candidates
	uint32_t mesh_mask_bits;       // meshes covered by mesh_mask; meshes beyond it are not candidates
	rtk_hit_record *cand;          // MODE 2: cand_k records per ray, the closest candidates in (t, prim) order
	uint32_t *cand_count;          // MODE 2: how many of them are valid
	uint32_t cand_k;
	uint32_t tile_blocks;          // image batches: tiles are numbered block by block (8x8 tiles = 64x64 pixels), not row by row
	const unsigned long long *n_indirect;   // rtk_trace_kernel: if set, the number of rays is read from here when the kernel starts and clamped to n: the list the
	                                        // assembly per-lane kernel left over (`perm` then points at it, its length is counter[RTK_LANE_LEFTOVER_WORD]),
	                                        // or the caller's own (rtk_ray_list: `perm` = d_ids or NULL, n = the size of the arrays)
	const struct PkBlockEntries *entries;   // packet kernels only: per 64x64-pixel block the entry points of its rays (or NULL: every tile starts at the root)
	const uint32_t *tile_list;     // packet kernel only: trace the tiles listed here (counter[RTK_LEFTOVER_COUNT_WORD] of them, dealt through
	                               // counter[RTK_LEFTOVER_HEAD_WORD]) instead of all tiles: what the assembly kernel handed back
};

// Scratch counter words of the hand-over from the assembly packet kernel (rtk_packet_hot.S) to the C++ one; cleared with the rest
#define RTK_LEFTOVER_COUNT_WORD 10
#define RTK_LEFTOVER_HEAD_WORD 11
// ... and from the assembly per-lane kernels (rtk_lane_hot.S) to rtk_trace_kernel: how many rays they left over
#define RTK_LANE_LEFTOVER_WORD 12

// Entry points shared by the 64 tiles of a 64x64-pixel block (rtk_packet_entries_kernel, rtk_trace_packet.hip): the block's
// rays are bounded by a box of origins and a box of reciprocal directions (one sign per axis), that BEAM is walked down the
// top of the tree by the interval form of the slab test, and the nodes it reaches at the cut are listed front to back by a
// lower bound of their entry distance. A tile whose rays lie inside the beam starts at these instead of at the root
// (config 2: 26.7 wave node steps per tile instead of 34.3) and stops at the first entry that lies behind every lane's hit.
// Every entry is an INNER node: a node with a leaf child is listed itself and not opened -- a listed leaf would cost every
// tile of the block a triangle test whether or not any of its rays enters the leaf's box (measured: +25 % triangle tests).
// (Listed in the order a traversal from the root reaches them, with the smallest bound of the rest for the early exit, tiles
// visited more nodes and were slower than from the root: profiles/r04_packet_entries.log.)
#define PK_MAX_ENTRIES 56
struct PkBlockEntries {
	float olo[3], ohi[3];          //  0  the beam: origins ...
	float rlo[3], rhi[3];          // 24  ... and reciprocal directions of the block's rays
	uint32_t count;                // 48  entries; 0 = none (rays of mixed signs, not tame, too many entries): tiles start at the root
	uint32_t pad[3];
	struct { uint32_t ref; float tlo; } e[PK_MAX_ENTRIES];   // 64  node reference, lower bound of the entry distance (ascending)
};
static_assert(sizeof(PkBlockEntries) == 512 && offsetof(PkBlockEntries, count) == 48 && offsetof(PkBlockEntries, e) == 64, "rtk_packet_hot.S reads this layout");

// Kernel argument of rtk_packet_hot (rtk_packet_hot.S reads these offsets)
struct PkHotParams {
	const void *nodes;             //  0
	const void *tris;              //  8
	const rtk_ray *rays;           // 16
	rtk_hit_record *hits;          // 24
	unsigned long long *counter;   // 32
	uint32_t *leftover;            // 40  tile numbers handed to the C++ kernel
	uint32_t num_blocks;           // 48  64x64-pixel blocks of the image
	uint32_t image_w;              // 52
	uint32_t blocks_per_row;       // 56
	uint32_t bpr_magic;            // 60  ceil(2^32 / blocks_per_row): block / blocks_per_row = mul_hi(block, magic)
	float bound_abs;               // 64  max(largest |plane| of the scene, 1)
	uint32_t pad;
	const PkBlockEntries *entries; // 72  per block (numbered like the tiles' blocks), or NULL
};
static_assert(sizeof(PkHotParams) == 80 && offsetof(PkHotParams, num_blocks) == 48 && offsetof(PkHotParams, bound_abs) == 64 && offsetof(PkHotParams, entries) == 72,
	"rtk_packet_hot.S reads this layout");

// Kernel argument of rtk_lane_hot_closest / rtk_lane_hot_any (rtk_lane_hot.S reads these offsets)
struct LnHotParams {
	const void *qnodes;            //  0  64-byte compressed nodes
	const void *tris;              //  8
	const rtk_ray *rays;           // 16
	void *out;                     // 24  closest: rtk_hit_record per ray; any-hit: one byte per ray
	unsigned long long *counter;   // 32
	unsigned long long *leftover;  // 40  ray numbers handed to rtk_trace_kernel (8-byte words, the number in the low half)
	const unsigned long long *perm;// 48  optional ray order (sort words, ray number in the low half)
	uint32_t n;                    // 56
	uint32_t refill_min;           // 60
	uint32_t node_exit;            // 64
	float bound_abs;               // 68  largest |plane| of the scene (DevSceneConsts::bound_raw)
	uint2 *spill;                  // 72  stack entries beyond a lane's LDS column: [entry][lane of the launch]
	uint32_t spill_stride;         // 80  lanes of the launch (>= lanes of this kernel's grid)
	uint32_t spill_cap;            // 84  entries per lane
};
static_assert(sizeof(LnHotParams) == 88 && offsetof(LnHotParams, n) == 56 && offsetof(LnHotParams, bound_abs) == 68 && offsetof(LnHotParams, spill) == 72 &&
	offsetof(LnHotParams, spill_cap) == 84, "rtk_lane_hot.S reads this layout");
// ... and of their listed forms, rtk_lane_hot_closest_listed / rtk_lane_hot_any_listed: n = min(*count, hot.n), read by the kernel
struct LnHotListedParams {
	LnHotParams hot;
	const unsigned long long *count;   // 88
};
static_assert(sizeof(LnHotListedParams) == 96 && offsetof(LnHotListedParams, count) == 88, "rtk_lane_hot.S reads this layout");

// Kernel argument of rtk_allhits_kernel (rtk_allhits.hip): every candidate of a ray, counted or written to the ray's segment
#define AH_LDS_STACK 30u           // 4-byte stack entries per lane held in LDS: 30 KB per workgroup, five workgroups share a CU's 160 KB
struct AllHitsParams {
	const DevNode *nodes;
	const DevTri *tris;
	uint32_t num_nodes;
	uint32_t n;                    // rays, below 2^32
	const rtk_ray *rays;
	uint32_t *counts;              // count form: one word per ray
	const unsigned long long *offsets;   // fill form: n + 1 entries; ray i owns records[offsets[i] .. offsets[i + 1])
	rtk_hit_record *records;
	uint32_t *written;             // fill form, optional: records kept per ray
	unsigned long long *counter;   // the stream's counter words: queue heads, [RTK_ERROR_WORD] is set by a dropped push
	uint32_t *spill;               // stack entries beyond a lane's LDS column: [entry][lane of the launch]
	uint32_t spill_stride;         // lanes
	uint32_t spill_cap;            // entries per lane
	uint32_t refill_min, node_exit, dynamic;
	// built-in candidate filters (rtk_dev_filter, FILT forms only); all optional
	uint32_t mesh_mask_bits;
	const uint32_t *mesh_mask;
	const uint32_t *ignore_prim;
	const rtk_hit_record *after;
};

// DevTri.flags: bit 0 = last triangle of its leaf, bits 8.. = mesh index (for the mesh-mask filter)
#define RTK_TRI_MESH_SHIFT 8

// _mm_min_ps/_mm_max_ps semantics (second operand when the compare is false, NaN included)
__device__ __forceinline__ float sse_min(float a, float b) { return a < b ? a : b; }
__device__ __forceinline__ float sse_max(float a, float b) { return a > b ? a : b; }


// Row-major image -> 8x8 pixel tiles, so that the 64 lanes of a wave share BVH nodes.
// With `blocks` the tiles themselves are numbered block by block (64 consecutive tiles = one 64x64 pixel block), so that
// the tiles a work queue hands out one after the other -- to waves that run at the same time on one XCD -- are
// neighbours in the image and walk the same part of the tree (L2 / scalar cache hits instead of fabric traffic).
__device__ __forceinline__ unsigned long long map_index(unsigned long long i, uint32_t w, uint32_t h, uint32_t blocks = 0)
{
	if (w == 0) return i;
	const unsigned long long tile = i >> 6;
	const uint32_t in = (uint32_t)i & 63u;
	const uint32_t tiles_per_row = w >> 3;
	unsigned long long ty;
	uint32_t tx;
	if (blocks) {
		const unsigned long long blk = tile >> 6;
		const uint32_t b = (uint32_t)tile & 63u, blocks_per_row = w >> 6;
		const unsigned long long by = blk / blocks_per_row;
		tx = (uint32_t)(blk - by * blocks_per_row) * 8u + (b & 7u);
		ty = by * 8u + (b >> 3);
	} else {
		ty = tile / tiles_per_row;
		tx = (uint32_t)(tile - ty * tiles_per_row);
	}
	const unsigned long long x = (unsigned long long)tx * 8u + (in & 7u);
	const unsigned long long y = ty * 8u + (in >> 3);
	return y * w + x;
}


// the kernels address nodes and triangles as SGPR base + 32-bit byte offset
inline bool rtk_within_4gib(const DevSceneView &v)
{
	return (uint64_t)v.num_nodes * 128u <= 0xffffff00ull && (uint64_t)v.num_tris * RTK_TRI_STRIDE <= 0xffffff00ull;
}

// The doors of the kernel files: each holds one kernel family, and these launch it.
// rtk_trace.hip: rtk_trace_kernel's variant (rtk_trace_plan.h). The occupancy query also answers for the C++ packet kernel's variants; cached per device
int rtk_trace_occupancy(int device, int variant);
void rtk_trace_kernel_launch(int variant, const TraceParams &p, unsigned blocks, hipStream_t stream);
// rtk_allhits.hip: rtk_allhits_kernel's form (fill | filtered << 1); resident workgroups per CU, cached per device
int rtk_allhits_occupancy(int device, int form);
void rtk_allhits_kernel_launch(int form, const AllHitsParams &p, unsigned blocks, hipStream_t stream);
// rtk_ray_sort.hip: the ray-reordering pre-pass; sc->sort holds rtk_ray_sort_bytes(n) for a capacity of n rays
size_t rtk_ray_sort_bytes(size_t n);
int rtk_ray_sort_launch(const rtk_dev_scene *ds, LaunchScratch *sc, const rtk_ray *d_rays, size_t n, const TraceKnobs &knobs, hipStream_t stream, const unsigned long long **perm);
// rtk_trace_packet.hip
int rtk_packet_occupancy(bool counted);
void rtk_packet_launch(const TraceParams &p, unsigned blocks, hipStream_t stream, bool counted);
// the blocks' entry lists (p.image_w / image_h, 64x64-pixel blocks numbered row by row) into `out`, one wave per block
void rtk_packet_entries_launch(const TraceParams &p, PkBlockEntries *out, float bound_abs, unsigned target, unsigned max_levels, hipStream_t stream);

// The hand-written kernels: a code object assembled by the Makefile, carried in this library as a byte array and loaded once per
// device, by a thread that has this device current. One object per .S family, its kernels named by a table; all of them run
// TRACE_BLOCK_THREADS lanes per workgroup and take their arguments as one parameter block.
struct AsmKernel {
	const char *name;
	int cap;                       // most workgroups per CU, whatever the occupancy query says; 0: launched on another kernel's figure, not asked
};
struct AsmModule {
	enum { MAX_KERNELS = NUM_PACKET_KERNELS };
	struct Loaded { hipModule_t mod = nullptr; hipFunction_t fn[MAX_KERNELS] = {}; int blocks_per_cu[MAX_KERNELS] = {}; bool tried = false; };
	const void *image;
	const AsmKernel *table;        // [count]; the object counts as loaded if table[0] is found
	int count;
	const char *not_loaded;        // the error of a launch without the kernel
	std::mutex mutex;
	Loaded slot[RTK_MAX_DEVICES];
	AsmModule(const void *image_, const AsmKernel *table_, int count_, const char *not_loaded_) : image(image_), table(table_), count(count_), not_loaded(not_loaded_) {}
	// the device's kernels, or NULL: the object does not load, or this thread has another device current (asked again later)
	const Loaded *on(int device);
	int launch(int device, int kernel, void *params, size_t size, unsigned blocks, hipStream_t stream);
};
AsmModule &rtk_lane_module();      // rtk_lane_hot.S: 0 rtk_lane_hot_closest, 1 rtk_lane_hot_any, 2 and 3 their listed forms (rtk_launch.hip)
AsmModule &rtk_packet_module();    // rtk_packet_hot.S, rtk_packet_beam2.S: kernels numbered by PacketKernel (rtk_trace_packet.hip)
