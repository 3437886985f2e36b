// rtk_trace_plan.h -- which kernels a trace launch runs, decided by a pure function of the batch, the options, the scene, the
// kernels this device has loaded and the environment defaults. Plain C++17, no HIP: the host compiler builds it alone
// (tests/test_trace_plan_cpu.py does). rtk_launch_trace (rtk_launch.hip) gathers the inputs and carries the plan out.
#pragma once

#include "rtk_amd.h"

#include <stddef.h>
#include <stdint.h>

#ifndef LDS_STACK
#define LDS_STACK 15           // entries per lane held in LDS: 30 KB per workgroup, so that FIVE workgroups share a CU's 160 KB (with 16
                               // entries = 32 KB only four are placed: -5 % on incoherent rays, -4 % on shadow rays; 14 and 13 spill more)
#endif
#define TRACE_WAVES_PER_BLOCK 4
#define TRACE_BLOCK_THREADS (64 * TRACE_WAVES_PER_BLOCK)

// rtk_trace_kernel's variant index: any_hit | counted << 1 | filtered << 2 | compressed nodes << 3; then the collecting pair
// (exact, compressed nodes) and the C++ packet kernel (plain, counted)
enum { VARIANT_COLLECT = 16, VARIANT_PACKET = 18, VARIANT_PACKET_COUNTED = 19, NUM_VARIANTS = 20 };

// The packet kernel of a launch. Cpp: rtk_trace_packet_kernel takes every tile. The others are hand-written (rtk_packet_hot.S,
// rtk_packet_beam2.S), take every tile they can and hand the rest to the C++ kernel:
// Hot: rtk_packet_hot, per-lane slab tests; Beam: rtk_packet_beam, the node test is the interval test of the tile's own beam (one
// child plane per lane); Beam2: rtk_packet_beam2, two adjacent tiles per wave (the two halves of the wave test a node for the two
// tiles' beams); Count2: rtk_packet_count2, the counting form of Beam2 (the same source assembled with -DRTK_COUNT); Any2:
// rtk_packet_any2, its any-hit form (-DRTK_ANY: one flag per ray, a ray retired at its first hit).
// (The numbers are what RTK_AMD_PACKET_BEAM takes and what the RTK_AMD_LOG_PATH line prints as "beam".)
enum class PacketKernel { Cpp = -1, Hot, Beam, Beam2, Count2, Any2 };
enum { NUM_PACKET_KERNELS = 5 };

// Environment defaults of the launch path, RTK_AMD_<NAME> each; read once per process by rtk_trace_knobs (rtk_launch.hip).
struct TraceKnobs {
	int detect_image = 1;          // DETECT_IMAGE=0: batches without an image hint are not looked at
	int tile_blocks = 1;           // TILE_BLOCKS=0: image batches number their 8x8 tiles row by row, not by 64x64-pixel blocks
	int any_packets = 1;           // ANY_PACKETS=0: any-hit images stay on the per-lane kernel
	int qnodes = 1;                // QNODES=0: per-lane kernels read the 128 B exact nodes, not the 64 B compressed ones (A/B, and tests that compare the two)
	int packet_asm = 1;            // PACKET_ASM=0: the C++ packet kernel for every tile
	PacketKernel packet_beam = PacketKernel::Beam2;   // PACKET_BEAM (default 2): 2 = rtk_packet_beam2 (two tiles per wave), 1 = rtk_packet_beam,
	                               // 0 = rtk_packet_hot (the per-lane slab tests); A/B and tests
	bool log_path = false;         // LOG_PATH set: every launch prints the path it took to stderr
	int lane_asm = 1;              // LANE_ASM=0: rtk_trace_kernel instead of rtk_lane_hot.S
	size_t lane_lds = LDS_STACK;   // LANE_LDS: A/B builds of rtk_lane_hot.S with fewer LDS entries
	// RTK_TRACE_SORT_RAYS
	uint32_t sort_cell_bits = 7u;  // 2^7 cells per axis: 3.44 against 3.32 Grays/s at 2^5 on the shadow batch (profiles/r03_ab_sort_cells.log)
	uint32_t sort_octant = 0u;     // append the direction octant to the key
	int sort_key = 1;              // 0: origin cell in the batch's origin bounds (1: entry point into the scene bounds)
	// entry points shared by the tiles of a 64x64-pixel block
	int packet_entries = 1;        // PACKET_ENTRIES=0: every tile starts at the root
	unsigned entry_target = 26u;   // list size at which the walk stops: 20 / 24 / 28 / 32 / 36 -> 17.7 / 18.0 / 18.0 / 17.9 / 17.85 Grays/s on config 2, profiles/r04_packet_entries.log
	unsigned entry_levels = 8u;    // depth cap of the walk
	int hot_blocks_per_cu = 0;     // HOT_BLOCKS_PER_CU: fewer resident workgroups, to tell a latency-bound kernel from a throughput-bound one (0: as many as fit)
	int lane_stats = 0;            // LANE_STATS=1: print how many rays rtk_lane_hot.S handed back (synchronises the stream)
	int lane_blocks = 5;           // LANE_BLOCKS: cap of rtk_lane_hot.S's workgroups per CU (80 VGPRs, 30 KB of LDS per workgroup: five)
};

const TraceKnobs &rtk_trace_knobs();   // (the one function here that is not pure, and not in this file)

// rtk_trace_opts decoded; 0 = not given, for every field.
struct TraceOpts {
	uint32_t flags = 0;            // RTK_TRACE_*
	uint32_t image_w = 0, image_h = 0;   // as the caller wrote them (plan_trace checks them against the batch)
	uint32_t refill_min = 0;       // <= 64
	uint32_t blocks_per_cu = 0;
	uint32_t node_exit = 0;        // <= 64
	bool refill_given = false;
};

// The only place that looks at struct_size: a block shorter than a field counts as not having it (a block shorter than 16 bytes,
// or none: no flags and no image).
inline TraceOpts decode_opts(const rtk_trace_opts *opts)
{
	TraceOpts o;
	if (!opts || opts->struct_size < 16) return o;
	o.flags = opts->flags;
	o.image_w = opts->image_width;
	o.image_h = opts->image_height;
	if (opts->struct_size >= 24) {
		o.refill_min = opts->refill_min > 64 ? 64 : opts->refill_min;
		o.refill_given = opts->refill_min != 0;
		o.blocks_per_cu = opts->blocks_per_cu;
	}
	if (opts->struct_size >= 28) o.node_exit = opts->node_exit > 64 ? 64 : opts->node_exit;
	return o;
}

// What the decision reads of a scene ...
struct SceneFacts {
	uint32_t num_nodes = 0, num_tris = 0;
	bool has_qnodes = false;       // the compressed node array is there
	uint32_t stack_entries = 0;    // traversal stack entries a ray can need
	float bound_abs = 0.0f;        // largest |plane| of the scene
	double big_leaf_fraction = 0.0;   // leaves of more than three triangles
	int num_cus = 0;
	uint32_t tri_stride = 48;      // bytes per triangle record (RTK_TRI_STRIDE)
};

// ... of the device: the hand-written kernels that loaded, and how many workgroups of each fit a CU ...
struct DeviceKernels {
	bool packet[NUM_PACKET_KERNELS] = {};
	int packet_blocks_per_cu[NUM_PACKET_KERNELS] = {};
	bool lane = false;             // rtk_lane_hot_closest and rtk_lane_hot_any
	bool lane_listed = false;      // rtk_lane_hot_closest_listed and rtk_lane_hot_any_listed (the count of the batch read on the device)
	int lane_blocks_per_cu = 0;
	bool has(PacketKernel k) const { return k >= PacketKernel::Hot && packet[(int)k]; }
};

// ... and of the call.
struct TraceRequest {
	size_t n = 0;
	bool any_hit = false;
	bool counted = false;          // rtk_dev_trace_rays*_counted
	bool pk_counted = false;       // rtk_dev_trace_rays_packet_counted
	bool collect = false;          // the k closest candidates per ray (host-callback filters)
	bool filtered = false;         // a built-in filter is set (mesh mask, ignored primitive, "after")
	bool has_filter = false;       // a rtk_dev_filter came with the call, set or not
	bool listed = false;           // rtk_dev_trace_rays*_listed: n is the size of the arrays, how many rays are traced is read on the device
};

struct TracePlan {
	int error = RTK_AMD_OK;        // a refusal: nothing is launched, `message` says why
	const char *message = nullptr;
	uint32_t dynamic = 0;          // persistent workgroups that pull rays from a queue
	uint32_t image_w = 0, image_h = 0;   // 0: not an image
	uint32_t tile_blocks = 0;      // tiles are numbered block by block
	uint32_t refill_min = 8, node_exit = 32;
	bool qn = false;               // per-lane kernels read the compressed nodes
	int variant = 0;               // of rtk_trace_kernel / the C++ packet kernel
	bool packet = false;           // the packet kernels take the batch ...
	PacketKernel kernel = PacketKernel::Cpp;   // ... this one ...
	bool hot = false;              // ... which is hand-written: it runs first, the C++ kernel takes the tiles it hands back
	bool lane_hot = false;         // rtk_lane_hot.S runs first, rtk_trace_kernel takes the rays it hands back
	bool entries = false;          // the entry-list pre-pass runs
	bool sort_rays = false;        // the ray-reordering pre-pass runs
	size_t grid = 0, hot_grid = 0, lane_grid = 0;   // workgroups: of the C++ kernel, of the assembly packet kernel, of the assembly per-lane kernel
	size_t lds_entries = LDS_STACK;   // stack entries per lane that the first kernel keeps in LDS
	size_t spill_cap = 0;          // stack entries per lane beyond them: the spill area's depth ...
	size_t spill_lanes = 0;        // ... and width (one area serves the assembly kernel and the C++ pass behind it)
};

// an image of whole 64x64-pixel blocks
inline bool whole_blocks(uint32_t w, uint32_t h) { return (w % 64u) == 0u && (h % 64u) == 0u; }

// the image the caller announced, if it is one of this batch: rows of 8x8-pixel tiles
inline bool hinted_image(const TraceRequest &rq, const TraceOpts &o)
{
	return o.image_w && o.image_h && (size_t)o.image_w * o.image_h == rq.n && (o.image_w % 8u) == 0 && (o.image_h % 8u) == 0;
}

// A listed batch (rtk_ray_list) is no image, is not re-ordered and is always dealt from the queues (the host does not know how
// many of its rays are traced): the options as such a batch reads them, the image hint and the two flags taken out.
inline TraceOpts listed_opts(TraceOpts o)
{
	o.image_w = o.image_h = 0;
	o.flags &= ~(uint32_t)(RTK_TRACE_SORT_RAYS | RTK_TRACE_STATIC);
	return o;
}

// a batch that fits one workgroup needs no work queue (and no counter reset)
inline bool dynamic_launch(const TraceRequest &rq, const TraceOpts &o) { return rq.n > TRACE_BLOCK_THREADS && !(o.flags & RTK_TRACE_STATIC); }

// No image hint: is the batch an image anyway? Only worth asking where the packet kernels would take it (a closest-hit or any-hit
// batch without filters, whole 64x64-pixel blocks); costs two small launches and one wait for the stream (~20 us; the wait also
// stands between this batch and the host's next enqueue: a caller that knows its image says so in the options).
inline bool wants_image_look(const TraceRequest &rq, const TraceOpts &o, const SceneFacts &f, const TraceKnobs &k)
{
	return !rq.listed && k.detect_image != 0 && !hinted_image(rq, o) && !rq.has_filter && !rq.collect && !rq.counted && !rq.pk_counted &&
		rq.n >= 16384u && (rq.n % 4096u) == 0u && rq.n <= 0x40000000ull && dynamic_launch(rq, o) && f.stack_entries <= 64 &&
		!(o.flags & (RTK_TRACE_NO_DETECT | RTK_TRACE_NO_PACKET | RTK_TRACE_SORT_RAYS | RTK_TRACE_STATIC));
}

// Everything of the plan that needs no occupancy figure. look_w x look_h: what the image look found (0 x 0: nothing, or not asked).
inline TracePlan plan_kernels(const TraceRequest &rq, const TraceOpts &o_given, uint32_t look_w, uint32_t look_h, const SceneFacts &f,
	const DeviceKernels &dk, const TraceKnobs &k)
{
	TracePlan pl;
	const TraceOpts o = rq.listed ? listed_opts(o_given) : o_given;
	if (rq.listed) look_w = look_h = 0u;
	// (the assembly per-lane kernels take the batches a queue-fed launch of the plain call takes: more than one workgroup of rays)
	const bool many = dynamic_launch(rq, o);
	pl.dynamic = (many || rq.listed) ? 1u : 0u;
	// Defaults from sweeps on MI355X (profiles/r01_sweep_opts*.log, r02_ab_r2o/p.log): leave the node
	// loop once fewer than 32 lanes still descend (24 for image-shaped batches); image-shaped (tiled, coherent)
	// batches refill a wave only when it is empty, everything else as soon as 8 lanes are idle.
	const bool hinted = hinted_image(rq, o);
	if (hinted) { pl.image_w = o.image_w; pl.image_h = o.image_h; pl.refill_min = 64; pl.node_exit = 24; }
	if (o.refill_min) pl.refill_min = o.refill_min;
	if (o.node_exit) pl.node_exit = o.node_exit;
	// (an image that was found, not announced: at least two blocks per row, and the image's defaults whatever the options say)
	if (!hinted && look_w >= 128u && whole_blocks(look_w, look_h)) { pl.image_w = look_w; pl.image_h = look_h; pl.refill_min = 64; pl.node_exit = 24; }
	pl.tile_blocks = (k.tile_blocks && pl.image_w && whole_blocks(pl.image_w, pl.image_h)) ? 1u : 0u;

	// image-shaped closest-hit batches go to the wave-packet kernels (rtk_trace_packet.hip). So do image-shaped ANY-HIT batches of
	// whole 64x64-pixel blocks: "is there a hit in (min_t, max_t)" is what a closest-hit traversal answers, at several times the rate of
	// a ray per lane where the rays run side by side (coherent shadow / visibility rays); rtk_packet_any2 retires a ray at its first
	// hit and writes the flags, the C++ kernel (the tiles handed back) writes "the closest hit exists".
	const bool any_packet = rq.any_hit && k.any_packets != 0 && !rq.counted && pl.image_w >= 128u && whole_blocks(pl.image_w, pl.image_h) &&
		!(o.flags & (RTK_TRACE_SORT_RAYS | RTK_TRACE_STATIC));
	pl.packet = (!rq.any_hit || any_packet) && !rq.filtered && !rq.collect && pl.image_w != 0 && f.stack_entries <= 64 && !(o.flags & RTK_TRACE_NO_PACKET);
	pl.qn = f.has_qnodes && k.qnodes != 0 && !(o.flags & RTK_TRACE_EXACT_NODES);
	pl.variant = pl.packet ? (rq.counted ? VARIANT_PACKET_COUNTED : VARIANT_PACKET) : rq.collect ? VARIANT_COLLECT + (pl.qn ? 1 : 0)
		: ((rq.any_hit ? 1 : 0) | (rq.counted ? 2 : 0) | (rq.filtered ? 4 : 0) | (pl.qn ? 8 : 0));

	// ... and of those, a hand-written kernel takes every tile it can and hands the rest to the C++ kernel: whole 64x64-pixel
	// blocks, at least two per row, a scene whose planes bound the slab margins and whose leaves are small
	PacketKernel kernel = (o.flags & RTK_TRACE_NO_BEAM) ? PacketKernel::Hot : k.packet_beam;
	if ((o.flags & RTK_TRACE_ONE_TILE_BEAM) && kernel == PacketKernel::Beam2) kernel = PacketKernel::Beam;
	while (kernel > PacketKernel::Hot && !dk.has(kernel)) kernel = (PacketKernel)((int)kernel - 1);
	// (the any-hit form exists of rtk_packet_beam2 only)
	if (rq.any_hit && pl.packet) kernel = (kernel == PacketKernel::Beam2 && dk.has(PacketKernel::Any2)) ? PacketKernel::Any2 : PacketKernel::Cpp;
	// the counting form of the kernel that is timed: only where that kernel runs
	if (rq.pk_counted) {
		if (kernel != PacketKernel::Beam2 || !dk.has(PacketKernel::Count2)) {
			pl.error = RTK_AMD_ERR_UNSUPPORTED;
			pl.message = "rtk_dev_trace_rays_packet_counted: rtk_packet_beam2 is not the kernel of this launch";
			return pl;
		}
		kernel = PacketKernel::Count2;
	}
	pl.kernel = kernel;
	// (rtk_packet_beam2 has the group rule for leaves of four and more triangles; the one-tile kernels hand such tiles back)
	pl.hot = pl.packet && kernel != PacketKernel::Cpp && !rq.counted && k.packet_asm != 0 && pl.tile_blocks && pl.image_w >= 128u && pl.image_w <= 65536u &&
		rq.n <= 0x40000000ull && f.bound_abs < 0x1p19f && (kernel >= PacketKernel::Beam2 || f.big_leaf_fraction <= 0.02) && !(o.flags & RTK_TRACE_NO_ASM) &&
		dk.has(kernel);
	if (rq.pk_counted && !pl.hot) {
		pl.error = RTK_AMD_ERR_UNSUPPORTED;
		pl.message = "rtk_dev_trace_rays_packet_counted: this batch does not run on the assembly packet kernel (image hint, whole 64x64-pixel blocks, small leaves)";
		return pl;
	}
	// Plain closest-hit / any-hit batches on compressed nodes go to the hand-written per-lane kernels (rtk_lane_hot.S); the rays
	// they hand back (not tame, a leaf of four or more triangles, a stack deeper than the LDS column) follow in rtk_trace_kernel.
	// Byte offsets into nodes, triangles, rays and the ray order are 32-bit and kept below 2^31 there.
	pl.lane_hot = !pl.packet && !rq.collect && !rq.counted && !rq.filtered && pl.qn && many && pl.image_w == 0 && k.lane_asm != 0 &&
		f.tri_stride == 48 && rq.n <= ((size_t)1 << 26) && (uint64_t)f.num_nodes * 64u < 0x80000000ull &&
		(uint64_t)f.num_tris * f.tri_stride < 0x80000000ull && f.bound_abs < 0x1p60f && (!rq.any_hit || f.big_leaf_fraction <= 0.02) &&
		!(o.flags & (RTK_TRACE_NO_ASM | RTK_TRACE_STATIC)) && f.stack_entries < 512u && (rq.listed ? dk.lane_listed : dk.lane);
	// entry points shared by the tiles of a 64x64-pixel block (rtk_packet_entries_kernel, one small launch ahead of the traversal)
	pl.entries = pl.packet && pl.tile_blocks && k.packet_entries != 0 && f.bound_abs < 0x1p19f && f.num_nodes != 0u && !(o.flags & RTK_TRACE_NO_ENTRIES);
	// optional ray reordering pre-pass (per-lane kernels only)
	pl.sort_rays = !pl.packet && (o.flags & RTK_TRACE_SORT_RAYS) && rq.n < 0x7fffffffu;
	return pl;
}

// The kernel variant whose occupancy plan_trace wants to know.
inline int variant_of(const TraceRequest &rq, const TraceOpts &o, uint32_t look_w, uint32_t look_h, const SceneFacts &f, const DeviceKernels &dk,
	const TraceKnobs &k)
{
	return plan_kernels(rq, o, look_w, look_h, f, dk, k).variant;
}

// The whole plan. occ: resident workgroups per CU of rtk_trace_kernel's / the C++ packet kernel's variant_of(the same arguments).
inline TracePlan plan_trace(const TraceRequest &rq, const TraceOpts &o, uint32_t look_w, uint32_t look_h, const SceneFacts &f, const DeviceKernels &dk,
	const TraceKnobs &k, int occ)
{
	TracePlan pl = plan_kernels(rq, o, look_w, look_h, f, dk, k);
	if (pl.error != RTK_AMD_OK) return pl;
	uint32_t blocks_per_cu = o.blocks_per_cu;
	if (blocks_per_cu == 0 || blocks_per_cu > (uint32_t)occ) blocks_per_cu = (uint32_t)occ;
	const size_t blocks_needed = (rq.n + TRACE_BLOCK_THREADS - 1) / TRACE_BLOCK_THREADS;
	pl.grid = (pl.dynamic || pl.packet) ? (size_t)f.num_cus * blocks_per_cu : blocks_needed;
	if (pl.grid > blocks_needed) pl.grid = blocks_needed;
	if (pl.grid > 0x7fffffffu) {
		pl.error = RTK_AMD_ERR_BAD_ARG;
		pl.message = "rtk_dev_trace: batch too large for one launch";
		return pl;
	}
	if (pl.hot) {
		const int fit = dk.packet_blocks_per_cu[(int)pl.kernel];
		pl.hot_grid = (size_t)f.num_cus * (size_t)(k.hot_blocks_per_cu > 0 && k.hot_blocks_per_cu < fit ? k.hot_blocks_per_cu : fit);
		if (pl.hot_grid > blocks_needed) pl.hot_grid = blocks_needed;
	}
	if (pl.lane_hot) {
		pl.lane_grid = (size_t)f.num_cus * (size_t)dk.lane_blocks_per_cu;
		if (pl.lane_grid > blocks_needed) pl.lane_grid = blocks_needed;
	}
	// spill area for rays whose stack outgrows LDS (16: PK_LDS_STACK in rtk_trace_packet.hip)
	pl.spill_lanes = (pl.lane_grid > pl.grid ? pl.lane_grid : pl.grid) * TRACE_BLOCK_THREADS;
	pl.lds_entries = pl.packet ? 16 : (pl.lane_hot && k.lane_lds < LDS_STACK) ? k.lane_lds : LDS_STACK;
	pl.spill_cap = f.stack_entries > pl.lds_entries ? f.stack_entries - pl.lds_entries : 0;
	return pl;
}
