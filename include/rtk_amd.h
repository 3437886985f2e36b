/*
 * rtk_amd.h -- additive batch / device entry points of librtk_amd.so (MI355X, gfx950).
 *
 * The reference's trace call is per ray and synchronous (reference rtk.h:129-130,
 * rtk.c:543-577); a GPU needs whole batches and device residency. Everything here is
 * NEW surface next to the nine unchanged rtk.h symbols. All functions are plain C:
 * pointers + sizes, no C++ or torch types. `stream` arguments are a hipStream_t passed
 * as void* (NULL = the default stream); "d_" pointers are DEVICE memory.
 *
 * Which reference interface each entry point stands in for:
 *   rtk_dev_scene_upload   : the hand-over of a built scene blob to the tracer. In the
 *                            reference that is just the rtk_scene* itself (rtk.c:546);
 *                            here the blob (format: SURVEY.md appendix A, reader
 *                            rtk.c:181-193, 457-465) is validated and re-laid-out in HBM.
 *   rtk_dev_scene_build    : rtk_build_scene / rtk_start_build..rtk_finish_build
 *                            (rtk.h:119-126; rtk.c:1625-1792) with the result left
 *                            device-resident (LBVH on the GPU instead of binned SAH tasks).
 *   rtk_dev_scene_export   : rtk_finish_build_to (rtk.h:123; rtk.c:1732-1774): emits the
 *                            device BVH as a reference-format blob.
 *   rtk_dev_trace_rays     : a loop of rtk_trace_ray over a ray array (rtk.h:129).
 *   rtk_dev_trace_rays_any : a loop of rtk_trace_ray_filter with a filter that accepts
 *                            the first candidate (rtk.h:117, 130; stub at rtk.c:579-582).
 *   rtk_dev_expand_hits    : the *hit = rt.hit copy-out of rtk.c:571-573 (full rtk_hit).
 *   rtk_trace_rays         : host-pointer convenience over the three above.
 */
#ifndef RTK_AMD_H
#define RTK_AMD_H

#include "rtk.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Status codes (0 = success). rtk_amd_last_error() describes the last failure on the
 * calling thread. */
enum {
	RTK_AMD_OK = 0,
	RTK_AMD_ERR_NO_DEVICE = -1,   /* no HIP device / driver */
	RTK_AMD_ERR_BAD_ARG = -2,
	RTK_AMD_ERR_OOM = -3,
	RTK_AMD_ERR_HIP = -4,         /* a HIP runtime call failed */
	RTK_AMD_ERR_BAD_SCENE = -5,   /* blob failed validation */
	RTK_AMD_ERR_UNSUPPORTED = -6,
};

const char *rtk_amd_last_error(void);
int rtk_amd_device_count(void);
int rtk_amd_set_device(int device);

/* Device-resident scene. */
typedef struct rtk_dev_scene rtk_dev_scene;

/* Compact hit record, 16 bytes. prim is the GLOBAL primitive id: the triangle's position
 * in concatenated mesh order (mesh_base[mesh_index] + triangle_index, cf. rtk.c:1131-1178);
 * RTK_PRIM_NONE on a miss (then t = ray.max_t, u = v = 0). u, v as in rtk_hit. */
typedef struct rtk_hit_record {
	float t, u, v;
	uint32_t prim;
} rtk_hit_record;
#define RTK_PRIM_NONE 0xffffffffu

typedef struct rtk_dev_scene_info {
	uint64_t num_triangles;
	uint64_t num_meshes;
	uint64_t num_nodes;        /* 4-wide nodes, 128 B each */
	uint64_t node_bytes;
	uint64_t triangle_bytes;   /* 48 B per triangle */
	uint64_t total_device_bytes;
	uint32_t max_depth;        /* deepest 4-wide node level (root = 1) */
	uint32_t stack_entries;    /* traversal stack entries a ray can need */
	double build_ms;           /* wall time inside rtk_dev_scene_build (0 for uploads) */
} rtk_dev_scene_info;

/* Trace options; pass NULL for defaults. */
typedef struct rtk_trace_opts {
	uint32_t struct_size;      /* sizeof(rtk_trace_opts) */
	uint32_t flags;            /* RTK_TRACE_* */
	uint32_t image_width;      /* if both non-zero and width*height == n: rays are a   */
	uint32_t image_height;     /* row-major image; lanes are mapped to 8x8 pixel tiles. Without it (or with NULL options) a closest-hit batch of whole
	                              64x64-pixel blocks is LOOKED AT: a regular step from ray to ray that jumps at the same distance every time is an image */
	uint32_t refill_min;       /* 0 = default; idle lanes needed before a wave refills  */
	uint32_t blocks_per_cu;    /* 0 = default; persistent grid size                     */
	uint32_t node_exit;        /* 0 = default; see DESIGN.md 3.1 (divergence control)   */
} rtk_trace_opts;
#define RTK_TRACE_STATIC    1u   /* one fixed ray per lane, no persistent refill (A/B only) */
#define RTK_TRACE_NO_PACKET 2u   /* image-shaped batch, but use the per-lane kernel (A/B only) */
#define RTK_TRACE_EXACT_NODES 8u  /* per-lane kernels: read the 128 B exact nodes instead of the 64 B compressed ones (A/B only) */
#define RTK_TRACE_NO_ASM 16u      /* C++ kernels only, not the hand-written ones (rtk_packet_hot.S, rtk_lane_hot.S) (A/B only) */
#define RTK_TRACE_NO_ENTRIES 32u  /* image-shaped batch: every tile starts at the root, no per-block entry lists (A/B only) */
#define RTK_TRACE_NO_BEAM 64u     /* image-shaped batch: rtk_packet_hot (per-lane slab tests) instead of the beam kernels (A/B only) */
#define RTK_TRACE_ONE_TILE_BEAM 128u /* image-shaped batch: rtk_packet_beam (one tile per wave) instead of rtk_packet_beam2 (A/B only) */
#define RTK_TRACE_NO_DETECT 256u   /* no image hint given: do not look whether the batch is a row-major image anyway (A/B; saves the two small launches
                                     and the wait of the look when the caller knows its rays are not an image) */
#define RTK_TRACE_SORT_RAYS 4u   /* reorder the batch by (origin cell, direction octant) before tracing; hits
                                    still land in input order. Pays off for large incoherent batches. */

/* Visit counters of the counting build (algorithmic-bytes model). */
typedef struct rtk_trace_counters {
	uint64_t rays;
	uint64_t nodes;            /* 128 B node records fetched by rays  */
	uint64_t leaves;
	uint64_t triangles;        /* 48 B triangle records fetched       */
	uint64_t hits;
	uint64_t stack_spills;     /* pushes that went past the LDS stack */
	uint64_t wave_node_steps;      /* wave-level node-loop trips (divergence diagnostics) */
	uint64_t wave_triangle_steps;  /* wave-level triangle-loop trips */
	uint64_t wave_rays;            /* reserved */
} rtk_trace_counters;

/* -- scenes -- */
/* Validates the blob (every offset range-checked without wrap-around; it must be a tree: a node or leaf
 * reached twice is refused; an empty child slot is the inverted box +1 / -1 on all three axes that every writer gives it,
 * and a slot that is inverted or NaN on some axis without being exactly that box is refused, not taken for empty) and
 * lays it out in HBM. rtk_dev_scene_upload trusts scene->size_in_bytes to be
 * readable, as the reference's bare rtk_scene* forces it to; a loader of untrusted files uses
 * rtk_dev_scene_upload_buffer, which also checks the header against the buffer size. */
rtk_dev_scene *rtk_dev_scene_upload(const rtk_scene *scene);
rtk_dev_scene *rtk_dev_scene_upload_buffer(const void *blob, size_t blob_bytes);
rtk_dev_scene *rtk_dev_scene_build(const rtk_scene_desc *desc);
void rtk_dev_scene_free(rtk_dev_scene *ds);
int rtk_dev_scene_get_info(const rtk_dev_scene *ds, rtk_dev_scene_info *info);
/* mesh_base[0..num_meshes] (prefix sums of per-mesh triangle counts) */
int rtk_dev_scene_mesh_base(const rtk_dev_scene *ds, uint64_t *out, size_t capacity);
/* out[slot] = global primitive id of the triangle stored at that slot (device order: leaf by leaf;
 * Morton order for device-built scenes). capacity in elements; returns the triangle count or < 0. */
long long rtk_dev_scene_primitive_order(const rtk_dev_scene *ds, uint32_t *out, size_t capacity);
size_t rtk_dev_scene_export_size(const rtk_dev_scene *ds);
rtk_scene *rtk_dev_scene_export(const rtk_dev_scene *ds, void *buffer, size_t size);

/* New positions for the SAME triangles, in place: desc must describe the meshes the scene was made from -- the same
 * num_meshes, the same num_triangles per mesh. Only mesh.position (data, stride, type; host or device memory, F32 or
 * F64, as rtk_dev_scene_build accepts) is read; the triangles keep the vertex indices the scene recorded when it was
 * built or uploaded (rtk_vertex.index), so mesh.index / index_cb are ignored. Afterwards the scene is what a build would
 * have produced for this topology: every child box is the exact union of what is below it (also for an uploaded blob,
 * whose boxes need not be), compressed nodes, child order words and constants are remade. Slots, primitive ids
 * (rtk_dev_scene_primitive_order), node numbers, max_depth, stack_entries and every handle to the scene stay.
 *   - A refit WRITES the scene. "A scene is never modified by a launch" stays true for traces; the caller must not have
 *     a trace of this scene in flight on another stream or thread while a refit runs. Work queued earlier on `stream`
 *     is ordered before it by the stream.
 *   - Synchronous: the call returns after the refit has completed on `stream`; the scene may then be traced from any
 *     stream. The first refit of a scene also makes its schedule (and, for a device-built scene, its side arrays).
 *   - RTK_AMD_ERR_BAD_ARG: a NULL argument, a mesh count or a per-mesh triangle count that differs from the scene's, an
 *     unknown position type, a mesh without positions. RTK_AMD_ERR_UNSUPPORTED: a mesh with position_cb set (callbacks
 *     are out of scope for a refit). These are decided before anything is launched: the scene is untouched.
 *   - The tree's QUALITY is the topology's: after a large deformation the scene traces correctly, but slower than a
 *     rebuild of the new positions would. rtk_dev_scene_quality (below) measures that; the host decides when to rebuild.
 * rtk_dev_scene_last_refit_ms: wall time inside the last successful refit of the scene (0 if there was none). */
int rtk_dev_scene_refit(rtk_dev_scene *ds, const rtk_scene_desc *desc, void *stream);
double rtk_dev_scene_last_refit_ms(const rtk_dev_scene *ds);

/* The same for SOME meshes, at a cost that follows what moved. desc describes the scene as for rtk_dev_scene_refit (same
 * num_meshes, same num_triangles per mesh: both checked for every mesh), but only the meshes listed in mesh_ids are READ:
 * a mesh that is not listed may have position.data == NULL, a callback, anything; its triangles keep the positions they
 * have. Listed meshes obey the rules above (F32 / F64 / REAL / DEFAULT, stride, host or device memory; position_cb ->
 * RTK_AMD_ERR_UNSUPPORTED; no positions -> RTK_AMD_ERR_BAD_ARG). mesh_ids is host memory; an id may repeat (counted
 * once); a listed mesh may have zero triangles.
 *   - The result is BIT-IDENTICAL to the full refit: every node word, triangle record, compressed node, order word and
 *     constant, and the choice between exact and compressed nodes, are what rtk_dev_scene_refit would have left, had it
 *     been given the listed meshes' new positions and, for every other mesh, the positions the scene holds now.
 *     Everything said above holds word for word: slots, ids, node numbers, depth and handles stay; the scene is WRITTEN,
 *     so no trace of it may be in flight; synchronous; work queued earlier on `stream` is ordered before it.
 *   - Work: the listed meshes' triangles, and the nodes above their leaves (boxes, compressed node, order words). The
 *     first such call of a scene makes its tables (12 B per node, 8 B per triangle, counted in total_device_bytes). Two
 *     cases run the full box and finish passes instead, with the same result: the listed meshes hold more than a
 *     quarter of the scene's triangles (the full passes are cheaper then), or the scene is an uploaded blob that has not
 *     had a refit yet (its boxes need not be exact unions, and the ones left alone would stay loose).
 *   - num_ids == 0, or no triangle in the listed meshes: success, no bit changes, nothing is launched.
 *   - RTK_AMD_ERR_BAD_ARG also for an id >= num_meshes and for mesh_ids == NULL with num_ids != 0. As above every
 *     refusal is decided before anything is launched and leaves the scene alone.
 * rtk_dev_scene_last_refit_nodes: how many nodes the last successful refit of the scene (either call) remade the boxes
 * of: num_nodes after a full refit, 0 if there was none or it had nothing to do. rtk_dev_scene_last_refit_ms covers both
 * calls (0 after a call that had nothing to do). */
int rtk_dev_scene_refit_meshes(rtk_dev_scene *ds, const rtk_scene_desc *desc, const uint32_t *mesh_ids, size_t num_ids, void *stream);
uint64_t rtk_dev_scene_last_refit_nodes(const rtk_dev_scene *ds);

/* PLACED meshes: the description holds every mesh in its rest pose, and a 3 x 4 matrix per mesh says where it stands. What a
 * host of rigid bodies has (one vertex buffer per mesh, one matrix per mesh and frame), and what an instance is: two meshes
 * may name the same position and index buffers with different placements. rtk_mesh has the reference's 96 bytes and no room
 * for a matrix, so the placements come in beside the description: host memory, desc->num_meshes entries, indexed by mesh
 * number; rtk_dev_scene_refit_meshes_placed reads only the listed entries.
 *   - THE RULE: m[0..11] row by row; the vertex is made float as an unplaced call makes it ((float) of a double), then
 *         x' = ((m0*x + m1*y) + m2*z) + m3,  y' = ((m4*x + m5*y) + m6*z) + m7,  z' = ((m8*x + m9*y) + m10*z) + m11
 *     with every product and every sum rounded to float on its own, in this order, never fused: numpy float32 arithmetic.
 *     Denormals are kept. The identity is not a bit-for-bit no-op (-0 becomes +0, 0 * inf is NaN); of a NaN result only
 *     that it is one is promised. rtk_amd/csrc/rtk_place_rule.h is the rule, for the host and the device.
 *   - RESULT: each call leaves the scene bit for bit as its unplaced sibling (rtk_dev_scene_build, _refit, _refit_meshes)
 *     would, given a twin description in which every mesh has tightly packed F32 positions equal to the rule applied to
 *     every vertex of that mesh, with the same index buffers and triangle counts: content_hash,
 *     rtk_dev_scene_primitive_order, the exported blob, every field of rtk_dev_scene_info except build_ms (so
 *     total_device_bytes too), last_refit_nodes, the choice between exact and compressed nodes and the narrow-key rule of
 *     the build are the twin's.
 *   - INPUTS: whatever the sibling accepts for positions and indices: F32 / F64 / REAL / DEFAULT positions, strides, host
 *     or device memory, u16 / u32 / implicit indices, index_cb where the build accepts it. Host-resident positions are
 *     staged as they are and placed on the device.
 *   - rtk_hit.mesh_index, triangle_index and vertex[].index are those of the mesh ENTRY (of the instance, not of whoever
 *     else shares its buffers); vertex[].position is the placed position the scene holds.
 *   - NOTHING IS REMEMBERED: the scene keeps no placement. A later rtk_dev_scene_refit takes its positions as given;
 *     rtk_dev_scene_rebuild, _export, _quality, _split_leaves and _validate work on the records as always. The unplaced
 *     calls allocate and count what they always did.
 *   - RTK_AMD_ERR_BAD_ARG (the build: NULL) for placements == NULL and for everything the sibling refuses;
 *     RTK_AMD_ERR_UNSUPPORTED (the build: NULL) for a mesh that is read and has position_cb set: a callback produces world
 *     positions already. Every refusal is decided before anything is launched and leaves the scene alone.
 *   - rtk_dev_scene_refit_meshes_placed keeps the quarter crossover, the rule for an uploaded blob's first refit and the
 *     num_ids == 0 no-op of rtk_dev_scene_refit_meshes. Locks, synchrony, rtk_dev_scene_last_refit_ms and
 *     rtk_dev_scene_last_refit_nodes are the siblings'. */
typedef struct rtk_placement { float m[12]; } rtk_placement;
rtk_dev_scene *rtk_dev_scene_build_placed(const rtk_scene_desc *desc, const rtk_placement *placements);
int rtk_dev_scene_refit_placed(rtk_dev_scene *ds, const rtk_scene_desc *desc, const rtk_placement *placements, void *stream);
int rtk_dev_scene_refit_meshes_placed(rtk_dev_scene *ds, const rtk_scene_desc *desc, const rtk_placement *placements,
                                      const uint32_t *mesh_ids, size_t num_ids, void *stream);

/* How good the tree is NOW: the surface-area-heuristic cost of the scene's exact child boxes, measured on the device. What
 * a host that refits every frame asks to learn that a rebuild pays: measure once after rtk_dev_scene_build (or an upload),
 * refit, measure again every frame or every few, and rebuild when sah_cost has grown past a ratio of the host's choosing.
 *   - Area of a box: 2 * (dx*dy + dy*dz + dz*dx) with dx = (double)max - (double)min, in this order. A child slot counts by
 *     its child word: empty slots are skipped whatever their planes hold; a leaf child's triangle count is the one its first
 *     triangle record carries. A child box whose area is not finite (NaN or inf positions) is counted in nonfinite_boxes and
 *     left out of every sum (it still counts as an inner or a leaf child).
 *   - cost_node and cost_tri are the builder's own constants (0.5 and 1.0; environment RTK_AMD_SAH_CN / RTK_AMD_SAH_CT
 *     override both the builder and this call).
 *   - A root_area that is 0 or not finite gives node_visits = triangle_tests = sah_cost = 0; the sums are still reported
 *     and the call succeeds. A scene without triangles gives all zeros.
 *   - sah_cost_at_build: the sah_cost of the first successful call made while the scene had never had a successful refit
 *     (either refit call); the scene keeps it and every later call reports it. If the first call comes after a refit the
 *     field stays 0 (not known) for good: a host that wants sah_cost / sah_cost_at_build calls once right after the build
 *     or the upload. A refit measures nothing by itself.
 *   - DETERMINISTIC: two calls on a scene with the same bits return the same bits (measure_ms apart), so a scene and its
 *     replicas on other GPUs of the same kind agree, and a refit back to the build's positions gives the build's cost.
 *   - Reads only: no bit of the scene changes (rtk_dev_scene_validate's content_hash stays); safe beside traces of the
 *     scene on other streams and threads. It must not overlap a refit of the scene: the two take the same lock, and a
 *     measurement beside a refit on another thread waits for it. Synchronous: the call returns with the result in *out;
 *     work queued earlier on `stream` is ordered before it. The first call of a scene allocates 64 KB of device memory
 *     (counted in total_device_bytes); later calls allocate nothing.
 *   - RTK_AMD_ERR_BAD_ARG: ds or out NULL, or out->struct_size < sizeof(rtk_dev_scene_quality_info); decided before any
 *     HIP call. Works unchanged on the replicas of a multi-GPU context, rtk_mgpu_scene(m, i). */
typedef struct rtk_dev_scene_quality_info {
	uint32_t struct_size;        /* sizeof(rtk_dev_scene_quality_info), set by the caller */
	uint32_t nonfinite_boxes;    /* child boxes whose area is not finite: counted, left out of every sum */
	uint64_t inner_children;     /* child slots that name a node */
	uint64_t leaf_children;      /* child slots that name a leaf */
	double root_area;            /* surface area of the union of the root node's non-empty child boxes */
	double inner_area;           /* sum of the areas of all inner child boxes */
	double leaf_area;            /* sum of the areas of all leaf child boxes */
	double leaf_area_triangles;  /* sum over leaf children of area * triangles in the leaf */
	double node_visits;          /* 1 + inner_area / root_area */
	double triangle_tests;       /* leaf_area_triangles / root_area */
	double sah_cost;             /* cost_node * node_visits + cost_tri * triangle_tests */
	double sah_cost_at_build;    /* see above; 0 = not known */
	double measure_ms;           /* wall time inside this call */
} rtk_dev_scene_quality_info;
int rtk_dev_scene_quality(const rtk_dev_scene *ds, rtk_dev_scene_quality_info *out, void *stream);

/* Big leaves of a scene split in place: every leaf that holds more than max_leaf triangles is replaced by a small subtree of
 * 4-wide nodes whose leaves hold at most max_leaf. What a scene that arrived as a blob needs before it is traced many times:
 * the reference's builder, the CPU task builder and every file on disk make leaves of 4 to 63 triangles, the device builder
 * leaves of at most 3, and the hand-written packet kernels are made for those (a scene with more than 2 % bigger leaves is
 * kept off some of them and pays for every triangle of a leaf a beam touches). The top of the tree, which a binned-SAH
 * builder made well, stays as it is. max_leaf == 0: the device builder's own limit (RTK_AMD_MAX_LEAF, default 3); 1 .. 63 are
 * taken as given.
 *   - STAYS: primitive ids, the set of triangles, mesh_base, every handle. Every existing node's number and boxes: loose
 *     boxes of an upload stay loose (a refit makes them exact as before). The slot range of every former leaf: its K
 *     triangles are permuted inside [first, first + K) and nowhere else, so rtk_dev_scene_primitive_order changes there and
 *     stays a permutation.
 *   - CHANGES: a child word that named a split leaf names a new node. New nodes are appended at [old num_nodes, new
 *     num_nodes): subtree after subtree in the order of their former leaf's first slot, breadth-first inside a subtree, so a
 *     child always comes after its parent. Every box of a new node is the exact union of the triangles below it. The
 *     end-of-leaf flags and leaf sizes of the permuted records, and the entries of the four side arrays (vertex indices,
 *     primitive -> slot, slot -> mesh, slot -> triangle) where the scene has made them, follow the permutation. Compressed
 *     nodes, child order words and the scene's constants are made again over the whole new tree. num_nodes, node_bytes,
 *     total_device_bytes, max_depth, stack_entries (3 * max_depth + 1) and the share of big leaves that picks the kernels
 *     are recomputed; launch scratch grows by itself at the next launch.
 *   - FORGOTTEN, and made again on next use: the refit schedule, the tables of rtk_dev_scene_refit_meshes, the cached export
 *     plan. sah_cost_at_build is forgotten too: the next rtk_dev_scene_quality call sets it anew if the scene has never had
 *     a refit (after a refit it stays 0, as before).
 *   - DEPTH: the subtree that replaces a leaf of K triangles is at most 2 * ceil(log4(K / max_leaf)) node levels deep (a
 *     four-way median split needs ceil(log4(K / max_leaf)); the rest is the room the surface-area choice of the cuts gets),
 *     whatever the triangles are: equal, on a line, not finite. Every set of at most max_leaf triangles is a leaf; every
 *     new node has two to four children, none of them empty.
 *   - DETERMINISTIC: the result is a pure function of the scene's bits and max_leaf. Two scenes with equal content_hash
 *     have equal content_hash afterwards; the replicas of a multi-GPU context agree.
 *   - The call WRITES the scene and MOVES its node arrays: no trace, refit or measurement of the scene may be in flight on
 *     another stream or thread. It takes the lock of the refits and is synchronous; work queued earlier on `stream` is
 *     ordered before it.
 *   - Nothing to split (a device-built scene, a second call with the same limit, a scene without triangles): success,
 *     leaves_split == 0, no bit changes, nothing is kept allocated, nothing is forgotten.
 *   - RTK_AMD_ERR_BAD_ARG: ds NULL, max_leaf > 63, out->struct_size < sizeof(rtk_dev_split_info); decided before any HIP
 *     call. RTK_AMD_ERR_OOM is decided before the scene is written: everything is allocated first. While the call runs the
 *     scene needs its new node arrays beside the old ones (192 bytes per node) and 4 bytes per triangle and node.
 * rtk_mgpu_split_leaves does the same on every GPU of the context; rtk_mgpu_scene handles stay valid. */
typedef struct rtk_dev_split_info {
	uint32_t struct_size;        /* sizeof(rtk_dev_split_info), set by the caller */
	uint32_t max_leaf;           /* the limit that was applied (after resolving 0) */
	uint64_t leaves_split;       /* leaves that held more than max_leaf triangles */
	uint64_t nodes_added;        /* num_nodes after - num_nodes before */
	uint32_t largest_leaf_before, largest_leaf_after;
	uint32_t max_depth_before, max_depth_after;
	double split_ms;             /* wall time inside the call */
} rtk_dev_split_info;
int rtk_dev_scene_split_leaves(rtk_dev_scene *ds, uint32_t max_leaf, rtk_dev_split_info *out /* may be NULL */, void *stream);

/* The last step of the loop for animated scenes: when rtk_dev_scene_quality says the tree has degraded (or for a blob, which
 * has no description to build from), the device builder builds the tree again over the triangles the scene holds NOW, and the
 * live handle adopts it.
 *   - RESULT: the scene becomes what rtk_dev_scene_build returns for a description of the same meshes (same num_meshes, the
 *     same triangles per mesh in the same order) that holds the positions the scene holds now: nodes, triangle records,
 *     compressed nodes, order words and constants, num_nodes, max_depth, stack_entries, the slot order. content_hash of
 *     rtk_dev_scene_validate and rtk_dev_scene_primitive_order equal that fresh build's.
 *   - HOW: the builder runs over the triangles in primitive-id order (the id breaks ties between equal Morton codes, as the
 *     triangle's number does in a build), with the knobs, the plan and the narrow-key rule of rtk_dev_scene_build: if more
 *     than an eighth of the sorted neighbours share a code the build runs once more with 40 bits (rebuild_ms covers both).
 *     The leaf limit is the builder's own (RTK_AMD_MAX_LEAF).
 *   - STAYS: the handle, mesh_base, primitive ids, every primitive's rtk_vertex.index triple, the positions bit for bit, the
 *     per-stream launch scratch (it grows by itself at the next launch, as after a split), rtk_dev_scene_info.build_ms.
 *   - CHANGES: slots (rtk_dev_scene_primitive_order becomes another permutation), node numbers, num_nodes, node_bytes,
 *     total_device_bytes, max_depth, stack_entries; the share of big leaves that picks the kernels is the new tree's; no
 *     node counts as appended by a split any more; every box is an exact union again (what a refit of some meshes relies
 *     on). A scene that arrived as a blob keeps, from its first rebuild on, its vertex indices by primitive (12 bytes per
 *     triangle, counted in total_device_bytes).
 *   - FORGOTTEN, and made again on next use: the refit schedule, the tables of rtk_dev_scene_refit_meshes, the cached export
 *     plan, the four side arrays (they go by slot). The scene counts as NEVER REFITTED again: the next
 *     rtk_dev_scene_quality call sets sah_cost_at_build anew, so a host's ratio starts from the new tree.
 *   - ALL OR NOTHING: the new records and nodes are built in fresh allocations beside the old ones; the host swaps them in
 *     after the build's last wait and then releases the old ones. RTK_AMD_ERR_OOM and RTK_AMD_ERR_HIP release what was
 *     allocated and leave every bit of the scene as it was. While the call runs the scene needs its new records (48 bytes per
 *     triangle) and node block (about 96 bytes per triangle) beside the old ones, plus the build workspace.
 *   - The call WRITES the scene and MOVES its arrays: no trace, refit, measurement or split of the scene may be in flight on
 *     another stream or thread. It takes the locks the split takes, in the same order, and is synchronous; work queued
 *     earlier on `stream` is ordered before it.
 *   - Fewer than two triangles: success, no bit changes, nothing is launched.
 *   - RTK_AMD_ERR_BAD_ARG: ds NULL, out->struct_size < sizeof(rtk_dev_rebuild_info); decided before any HIP call.
 *     RTK_AMD_ERR_UNSUPPORTED: the scene does not hold exactly one triangle record per primitive (an uploaded blob may
 *     name an id twice or never, which rtk_dev_scene_validate reports as primitive_id_errors); decided before the scene is written, which stays as it was.
 * rtk_mgpu_rebuild does the same on every GPU of the context; rtk_mgpu_scene handles stay valid. */
typedef struct rtk_dev_rebuild_info {
	uint32_t struct_size;            /* sizeof(rtk_dev_rebuild_info), set by the caller */
	uint32_t key_bits;               /* width of the Morton code the final build used */
	uint64_t nodes_before, nodes_after;
	uint32_t max_depth_before, max_depth_after;
	double rebuild_ms;               /* wall time inside the call */
} rtk_dev_rebuild_info;
int rtk_dev_scene_rebuild(rtk_dev_scene *ds, rtk_dev_rebuild_info *out /* may be NULL */, void *stream);

/* Structural check of a device scene, run on the device (the loader/validator the reference lacks,
 * SURVEY.md section 5; blob-level checks happen in rtk_dev_scene_upload). Every child box must contain
 * what is below it, every triangle slot must sit in exactly one leaf, every node but the root must be
 * referenced exactly once by an earlier node, leaf headers must be well formed (1..63 triangles,
 * rtk.c:188). Returns RTK_AMD_OK when all error counts are zero, RTK_AMD_ERR_BAD_SCENE otherwise;
 * `loose_boxes` (a box that contains its contents without being their exact union) is legal and only
 * reported. content_hash covers nodes and triangle records: equal for two builds of the same input. */
typedef struct rtk_dev_scene_check {
	uint64_t nodes_checked, leaves_checked, triangles_checked;
	uint64_t box_violations;        /* child box does not contain its subtree / empty slot can be hit */
	uint64_t loose_boxes;
	uint64_t bad_references;        /* child index out of range or not after its parent */
	uint64_t leaf_format_errors;
	uint64_t triangles_missing, triangles_duplicated;
	uint64_t nodes_unreachable, nodes_shared;
	uint64_t primitive_id_errors;   /* id out of range, repeated, never used (uploaded blobs too: a mesh has largest triangle index + 1 primitives), or prim -> slot table inconsistent */
	uint64_t compressed_node_errors; /* a 64 B compressed node whose decoded child box does not contain the exact one */
	uint64_t first_bad_index;       /* smallest node / slot index that raised an error, ~0 if none */
	uint64_t content_hash;
} rtk_dev_scene_check;
int rtk_dev_scene_validate(const rtk_dev_scene *ds, rtk_dev_scene_check *out);

/* Which builder rtk_start_build / rtk_build_scene use (rtk.h:119-126). Default: the device LBVH build, a graph of
 * ONE task. RTK_AMD_BUILDER_CPU_TASKS selects the reference's caller-scheduled task graph on the CPU (rtk.c:1362-1507:
 * <= 128 triangle-setup tasks, one binned-SAH task per node, vertex-group finalisation), so a host's own scheduler
 * keeps driving a real graph from any number of threads; it needs no GPU to BUILD (tracing the blob still does).
 * Never selected implicitly. Environment RTK_AMD_BUILDER=cpu is read once if this was never called. */
enum { RTK_AMD_BUILDER_DEVICE = 0, RTK_AMD_BUILDER_CPU_TASKS = 1 };
int rtk_amd_set_builder(int builder);
/* Where the two PER-RAY symbols of rtk.h (rtk_trace_ray, rtk_trace_ray_filter; reference rtk.h:129-130) run. HOST (default): on
 * the calling thread, from the caller's blob -- a synchronous call for one ray cannot drive a GPU (a launch and its completion
 * are ~7 us before any work; the reference's call is under 1 us), SURVEY.md 8b serves this one symbol on the CPU. GPU: a batch
 * of one through the one-ray kernel (~25 us). Both return the same bytes. Batch entry points are not affected by this and have
 * no host form. Environment RTK_AMD_PER_RAY=gpu is read once if this was never called. */
enum { RTK_AMD_PER_RAY_HOST = 0, RTK_AMD_PER_RAY_GPU = 1 };
int rtk_amd_set_per_ray(int where);
int rtk_amd_get_builder(void);

/* Device builds draw their temporaries from one workspace per device that is kept between builds
 * (about 330 bytes per triangle); this releases it. */
void rtk_amd_release_workspace(void);

/* -- batches; asynchronous on `stream` --
 * Thread-safe: a scene is never modified by a launch. What a launch writes besides its outputs (work-queue
 * heads, the global part of the traversal stacks) lives in a scratch set per (scene, stream), so launches on
 * different streams or from different host threads never share state; launches on one stream are ordered by
 * the stream (reference: rtk_trace_ray is a pure function of a const scene, rtk.c:543-577). */
int rtk_dev_trace_rays(const rtk_dev_scene *ds, const rtk_ray *d_rays, size_t n,
	rtk_hit_record *d_hits, const rtk_trace_opts *opts, void *stream);
/* (any-hit with an image hint of whole 64x64-pixel blocks, image_width >= 128: traced by the packet kernels in their any-hit form
 * -- a ray is retired at its first hit -- the same flags at about three times the per-lane rate on rays that run side by side;
 * other shapes ignore the hint) */
int rtk_dev_trace_rays_any(const rtk_dev_scene *ds, const rtk_ray *d_rays, size_t n,
	uint8_t *d_occluded, const rtk_trace_opts *opts, void *stream);
int rtk_dev_expand_hits(const rtk_dev_scene *ds, const rtk_hit_record *d_records, size_t n,
	rtk_hit *d_hits, uint8_t *d_mask, void *stream);
/* Built-in candidate filters evaluated on the device (reference rtk.h:117,130: rtk_filter_fn /
 * rtk_trace_ray_filter, a stub at rtk.c:579-582; arbitrary C callbacks cannot run on the GPU, these cover
 * the common ones). A candidate hit is considered only if EVERY filter that is set accepts it; the result is
 * the closest accepted candidate (closest-hit call) or "is there an accepted candidate" (any-hit call).
 *   d_mesh_mask    bit m (word m/32, bit m%32) set = triangles of mesh m are visible; meshes >= mesh_mask_bits are not
 *   d_ignore_prim  one per ray: global primitive id that is never a candidate (self-intersection); RTK_PRIM_NONE = none
 *   d_after        one per ray: only candidates that come AFTER (t, prim) in lexicographic (t, prim) order are
 *                  considered; prim = RTK_PRIM_NONE switches it off for that ray. Feeding a ray's previous result
 *                  back enumerates ALL candidates of the ray in order, equal-t ones included -- the device half of
 *                  rtk_trace_rays_filter's host-callback loop.
 * All pointers are device memory and optional (NULL). */
typedef struct rtk_dev_filter {
	uint32_t struct_size;               /* sizeof(rtk_dev_filter) */
	uint32_t mesh_mask_bits;
	const uint32_t *d_mesh_mask;
	const uint32_t *d_ignore_prim;
	const rtk_hit_record *d_after;
} rtk_dev_filter;
int rtk_dev_trace_rays_filtered(const rtk_dev_scene *ds, const rtk_ray *d_rays, size_t n,
	rtk_hit_record *d_hits, const rtk_dev_filter *filter, const rtk_trace_opts *opts, void *stream);
int rtk_dev_trace_rays_any_filtered(const rtk_dev_scene *ds, const rtk_ray *d_rays, size_t n,
	uint8_t *d_occluded, const rtk_dev_filter *filter, const rtk_trace_opts *opts, void *stream);

/* ---- Ray lists: which rays of a batch are traced is decided on the device ----
 * After a trace a caller keeps some rays (the ones that hit, the ones that are not occluded); how many and which is known
 * on the device only. A rtk_ray_list names them there, rtk_dev_select_rays makes one from a trace's output, and the listed
 * traces take one: bounce after bounce is enqueued on one stream without a host wait in between.
 *
 * Listed traces. m = min(*d_count, num_rays) entries are traced. num_rays is the size of d_rays, of d_hits / d_occluded
 * and of the per-ray filter arrays (d_ignore_prim, d_after), as the host knows it; d_ids holds at least m entries. The
 * result for ray r goes to slot r of the output -- the rule the per-ray filter arrays follow --, and A SLOT THAT IS NOT
 * LISTED IS NOT WRITTEN. A listed slot holds bit for bit what rtk_dev_trace_rays[_any][_filtered] writes there for the same
 * ray array. An id may repeat: the ray is traced twice and written twice with the same bytes. An id >= num_rays is the
 * caller's error and, like a bad ray pointer, is NOT CHECKED (the ray is read and the result written out of range).
 * *d_count == 0 writes nothing and is not an error. The calls are asynchronous on `stream` and read nothing back: no host
 * wait anywhere. A count or a list that earlier work on the same stream wrote (a select, a kernel of the caller's) is
 * seen. They use the per-(scene, stream) scratch set like every other launch: the thread-safety rules above hold unchanged.
 * Listed batches never go to the packet kernels (a listed subset is not an image): image_width, image_height,
 * RTK_TRACE_SORT_RAYS and RTK_TRACE_STATIC of `opts` are IGNORED (they are speed hints); refill_min, node_exit,
 * blocks_per_cu, RTK_TRACE_NO_ASM and RTK_TRACE_EXACT_NODES apply as always.
 * Refused before anything is launched, RTK_AMD_ERR_BAD_ARG: list == NULL, d_count == NULL, a struct_size that is too small,
 * flags != 0, a missing output, num_rays >= 2^32; scene and device refusals are those of rtk_dev_trace_rays.
 * num_rays == 0 is RTK_AMD_OK with nothing launched. `filter` may be NULL. */
typedef struct rtk_ray_list {
	uint32_t struct_size;        /* sizeof(rtk_ray_list) */
	uint32_t flags;              /* 0 */
	const uint64_t *d_ids;       /* device; optional. Entry i names ray (uint32_t)d_ids[i]; only the low 32 bits are read,
	                                so a torch int64 index tensor is a list as it stands. NULL: the list is 0, 1, 2, ... */
	const uint64_t *d_count;     /* device; required. Read when the work reaches it on `stream`, never by the host. */
} rtk_ray_list;
int rtk_dev_trace_rays_listed(const rtk_dev_scene *ds, const rtk_ray *d_rays, size_t num_rays, const rtk_ray_list *list,
	rtk_hit_record *d_hits, const rtk_dev_filter *filter, const rtk_trace_opts *opts, void *stream);
int rtk_dev_trace_rays_any_listed(const rtk_dev_scene *ds, const rtk_ray *d_rays, size_t num_rays, const rtk_ray_list *list,
	uint8_t *d_occluded, const rtk_dev_filter *filter, const rtk_trace_opts *opts, void *stream);

/* Select: the list of the rays whose source element matches `kind`. The input list is gone through in order -- `in` == NULL:
 * 0 .. num_rays - 1; else the first min(*in->d_count, num_rays) entries of `in` -- and the ids r are kept whose element r of
 * d_src matches: d_src as rtk_hit_record[num_rays], prim != RTK_PRIM_NONE is a hit (RTK_SELECT_RECORD_HIT) and prim ==
 * RTK_PRIM_NONE a miss (RTK_SELECT_RECORD_MISS); d_src as uint8_t[num_rays], non-zero (RTK_SELECT_BYTE_NONZERO) or zero
 * (RTK_SELECT_BYTE_ZERO). The output is STABLE: kept ids appear in input order, packed from d_out_ids[0] (8 bytes each, the
 * upper half zero), and *d_out_count is their number; entries of d_out_ids at and beyond *d_out_count are not written. The
 * result is deterministic: the same inputs give the same bytes. Asynchronous on `stream`, no host wait. d_out_ids has room
 * for num_rays entries and MAY NOT ALIAS in->d_ids, nor d_out_count in->d_count (both are read after the outputs are begun).
 * As in the listed traces an input id >= num_rays is the caller's error. Scratch (one bit per ray and a few words per 1024)
 * comes from the scene's scratch set of the stream and grows like the rest: that is why `ds` is a parameter, and the
 * thread-safety rules above hold. RTK_AMD_ERR_BAD_ARG: an unknown kind, a NULL scene, source or output, a bad `in` (as for
 * the listed traces), num_rays >= 2^32. num_rays == 0: *d_out_count = 0. */
enum { RTK_SELECT_RECORD_HIT = 0, RTK_SELECT_RECORD_MISS = 1, RTK_SELECT_BYTE_NONZERO = 2, RTK_SELECT_BYTE_ZERO = 3 };
int rtk_dev_select_rays(const rtk_dev_scene *ds, const void *d_src, uint32_t kind, size_t num_rays,
	const rtk_ray_list *in, uint64_t *d_out_ids, uint64_t *d_out_count, void *stream);
/* (what one workgroup of the select's count / scatter kernels and one workgroup of its scan level cover, in rays: the sizes at
 * which the kernels take another path, for tests) */
uint32_t rtk_amd_select_block_items(void);
uint32_t rtk_amd_select_scan_items(void);

/* ---- Closest points: which triangle of the scene is nearest to a point, how far, and where on it ----
 * The second question the tree answers (signed-distance baking, proximity and collision checks, projection, snapping, ICP). It
 * reads the scene as it stands -- a device build, an uploaded blob, after any refit, split or rebuild -- and changes no bit of it.
 *
 * THE RESULT DOES NOT DEPEND ON THE TREE. It is a function of the scene's triangle records and the query alone, stated in float
 * arithmetic (rtk_amd/csrc/rtk_closest_rule.h; INTEGRATION.md "Closest points"): every triangle has a squared distance dist2,
 * barycentrics and a closest point q by Ericson's region walk, every operation rounded on its own, q clamped to the triangle's
 * own box; the answer to (p, max_dist2) is the triangle with the smallest dist2 < max_dist2, THE LOWEST PRIMITIVE ID AMONG EQUAL
 * dist2, or a miss. Leaf sizes, loose boxes and the node format only decide how many triangles are never looked at.
 *   hit    dist2, u (weight of vertex 0), v (weight of vertex 1) and the global primitive id; d_points[3 i ..] = q
 *   miss   dist2 = max_dist2 as given, u = v = 0, prim = RTK_PRIM_NONE; d_points[3 i ..] = the query point as given
 * The record has the shape of rtk_hit_record with dist2 in the place of t, and its miss is that record's miss: rtk_dev_select_rays
 * (RTK_SELECT_RECORD_HIT / _MISS) and rtk_dev_expand_hits take these records as they are. A max_dist2 that is NaN, zero or
 * negative is a miss, and so is a query with a non-finite coordinate; RTK_INF means no limit. A scene without triangles
 * answers every query with a miss.
 * `list` may be NULL: all num_queries queries are answered. Otherwise the words of the listed traces hold: m = min(*d_count,
 * num_queries) entries are answered, the result of query r goes to slot r of d_records (and d_points), A SLOT THAT IS NOT LISTED
 * IS NOT WRITTEN, an id may repeat, and the count is read when the work reaches it on `stream`. d_points may be NULL.
 * Asynchronous on `stream`: no host wait, nothing read back. The scene is only read, so the thread-safety rules of the batches
 * hold; the part of the walk's stack that does not fit on chip lives in the per-(scene, stream) scratch set, and a dropped push
 * (impossible for a tree) is reported by rtk_dev_trace_status like a trace's. Nothing it allocates counts toward the scene.
 * Refused before anything is launched, RTK_AMD_ERR_BAD_ARG: a NULL scene; NULL d_queries or d_records with num_queries != 0; a
 * bad list (as for the listed traces); num_queries >= 2^32; a calling thread whose current device is not the scene's.
 * num_queries == 0 is RTK_AMD_OK with nothing launched. Works as it is on rtk_mgpu_scene(m, i).
 * A scene with non-finite vertex coordinates: the call terminates and writes only inside its outputs; NOTHING ELSE IS PROMISED
 * about its results. */
typedef struct rtk_point_query { float x, y, z, max_dist2; } rtk_point_query;
typedef struct rtk_closest_record { float dist2, u, v; uint32_t prim; } rtk_closest_record;
int rtk_dev_closest_points(const rtk_dev_scene *ds, const rtk_point_query *d_queries, size_t num_queries,
	const rtk_ray_list *list, rtk_closest_record *d_records, float *d_points, void *stream);
/* Same result as rtk_dev_closest_points without a list, plus visit counts: rays = queries answered, nodes = 128 B node records
 * fetched, leaves, triangles = 48 B triangle records fetched, hits = queries that found a triangle, stack_spills = pushes that
 * went past the on-chip part of the stack (the wave_ fields stay 0). Null stream, synchronous; not for timing. */
int rtk_dev_closest_points_counted(const rtk_dev_scene *ds, const rtk_point_query *d_queries, size_t num_queries,
	rtk_closest_record *d_records, float *d_points, rtk_trace_counters *out);
/* (entries per lane the walk keeps on chip before it uses the spill area, for tests) */
uint32_t rtk_amd_closest_stack_entries(void);

/* ---- Signed distance: how far a point is from the surface, and on which side of it ----
 * What a closest-point query is asked next (sampling a signed distance field for implicit and neural shapes, voxelising a solid,
 * "is this particle inside the body", pushing a point out of a body). rtk_dev_signed_distances answers every query as
 * rtk_dev_closest_points does -- the same walk, the same records and points, byte for byte -- and then gives the distance a sign.
 *
 * THE RULE (rtk_amd/csrc/rtk_sign_rule.h; INTEGRATION.md "Signed distance") is Baerentzen and Aanaes's angle-weighted
 * pseudonormal. The closest point q of the answer's triangle lies on a feature of it: the face, one of its three edges or one of
 * its three vertices (the region 1 .. 7 of the closest rule, evaluated again on that record). The feature has a normal N: the
 * face's own cross product; for an edge the sum of the unit normals of every triangle on that edge; for a vertex the sum of
 * angle * unit normal over every triangle corner at that vertex. s = dot(p - q, N); the point is INSIDE iff s < 0 (a zero or a
 * NaN s is outside) and signed = inside ? -sqrt(dist2) : sqrt(dist2). The face normal alone, dot(p - q, n), is wrong at every
 * concave or saddle edge and vertex; the sums are right there. Corners are WELDED BY PLACE: two corners are the same vertex iff
 * their three coordinates compare equal as numbers (-0 equals +0, a NaN equals nothing). Vertex indices and mesh numbers play no
 * part, so a seam with duplicated vertices and two meshes that meet are one surface; a placed mesh's records are world positions.
 * Every operation is one float operation rounded on its own, sums are taken in ascending (primitive, corner) order, the angle
 * is a polynomial arctangent written in the header (no libm): THE TABLE AND THE SIGN DO NOT DEPEND ON THE TREE, on slots or on
 * the way the scene was made, and a numpy float32 restatement gives the same bits (tests/sign_ref.py).
 *   hit    d_signed[i] = +-sqrt(dist2); d_records[i] and d_points[3 i ..] as rtk_dev_closest_points writes them
 *   miss   d_signed[i] = RTK_INF: no triangle within max_dist2, the side is not known; record and point are that call's miss.
 *          A query that call answers with a miss without a walk (a NaN, zero or negative limit, a non-finite coordinate) is one.
 * What the method promises: on a CLOSED, CONSISTENTLY WOUND, NON-SELF-INTERSECTING surface the sign is the true one, up to the
 * float rounding of a dot product that is near zero only for points near the surface's tangent planes. On an open or
 * inconsistently wound mesh the call still terminates and is deterministic; the sign near the defects means nothing. The
 * diagnostics say which case a scene is in:
 *     closed = boundary_sides == 0 && nonmanifold_sides == 0 && inconsistent_sides == 0
 * is the "is the sign meaningful" test (degenerate_triangles only says how many records gave no normal to their neighbours).
 *
 * The table (18 floats per primitive: the edge normals of ab, ac, bc, then the vertex normals of a, b, c) is made on the device
 * on first use -- by rtk_dev_scene_prepare_signs or by the first rtk_dev_signed_distances / rtk_dev_scene_pseudonormals -- which
 * synchronises `stream` that one time; it counts 72 bytes per primitive toward total_device_bytes. A refit of any kind (vertices
 * moved) drops it and the next call makes it again; rtk_dev_scene_split_leaves and rtk_dev_scene_rebuild keep it. The call reads
 * a record through the scene's side arrays, which a device-built scene makes on first use as rtk_dev_expand_hits does.
 * `list`, d_points == NULL, asynchrony, the scratch set and rtk_dev_trace_status: as for rtk_dev_closest_points; A SLOT THAT IS
 * NOT LISTED IS NOT WRITTEN in d_signed either. d_records may be NULL: the walk's records then live in the per-(scene, stream)
 * scratch set.
 * Refused before any HIP call: RTK_AMD_ERR_BAD_ARG for everything rtk_dev_closest_points refuses and for a NULL d_signed with
 * num_queries != 0 (rtk_dev_scene_pseudonormals: a NULL d_out); RTK_AMD_ERR_UNSUPPORTED for a scene that does not hold exactly
 * one triangle record per primitive (an uploaded blob may name an id twice): nothing is allocated or written.
 * num_queries == 0 is RTK_AMD_OK and does not make the table. Works as it is on rtk_mgpu_scene(m, i). */
typedef struct rtk_dev_sign_info {
	uint64_t boundary_sides;        /* (prim, edge) pairs whose edge no other triangle shares */
	uint64_t nonmanifold_sides;     /* ... whose edge three or more triangles share */
	uint64_t inconsistent_sides;    /* ... shared with exactly one other triangle that runs it in the same direction */
	uint64_t degenerate_triangles;  /* records without a unit normal in float */
	uint64_t places;                /* distinct vertex places after welding */
	uint64_t table_bytes;
	double   table_ms;              /* wall time of the last making of the table; 0 if this call found it made */
} rtk_dev_sign_info;
/* makes the table now if it is not there (synchronises `stream` the one time it has to work), reports the diagnostics (kept with the table) */
int rtk_dev_scene_prepare_signs(const rtk_dev_scene *ds, rtk_dev_sign_info *out /* may be NULL */, void *stream);
/* copies the table to d_out[18 * num_prims] on `stream` (for tests and for users who want smooth feature normals) */
int rtk_dev_scene_pseudonormals(const rtk_dev_scene *ds, float *d_out, void *stream);
int rtk_dev_signed_distances(const rtk_dev_scene *ds, const rtk_point_query *d_queries, size_t num_queries, const rtk_ray_list *list,
	rtk_closest_record *d_records /* may be NULL */, float *d_points /* may be NULL */, float *d_signed, void *stream);

/* ---- Winding numbers: how many times the surface wraps round a point, also where the surface has holes ----
 * The inside test for the meshes the two others fail on: a scan, a game asset, a CAD export with a hole, a crack or a duplicated
 * shell, where pseudonormals (rtk_dev_signed_distances) and crossing parity mean nothing near the defect. The generalized
 * winding number (Jacobson et al. 2013) of a point is the sum of the signed solid angles of all triangles seen from it, over
 * 4 pi: 1 inside and 0 outside a closed surface wound outwards, k inside k nested shells, -1 inside a shell wound inwards, a
 * smooth fraction near a hole. w > 0.5 is an inside test that degrades gracefully.
 *
 * THE RULE (rtk_amd/csrc/rtk_winding_rule.h; INTEGRATION.md "Winding numbers"). The sum is taken over the scene's tree (Barill et
 * al. 2018, first order): each child slot of a node has MOMENTS -- the area vector N = sum of 0.5 * cross(b - a, c - a), the
 * area-weighted centre P and a radius R that every corner under the slot lies within of P (from the slot's box) --, and a child
 * is answered by the one far term dot(N, P - p) / |P - p|^3 / (4 pi) iff |P - p|^2 > (beta * R)^2; otherwise it is descended,
 * and a leaf's triangles are summed by van Oosterom and Strackee's solid angle with the polynomial atan2 of rtk_sign_rule.h.
 * One float operation at a time, no libm. beta = 2 is the default; a larger beta descends more and is more exact;
 * RTK_WINDING_EXACT takes no far term at all: every triangle is summed, O(n) per query, the form the fast one is measured against.
 *   d_winding[i] = w of (x, y, z) of d_queries[i]. max_dist2 of an rtk_point_query IS NOT READ.
 *   A query with a non-finite coordinate is answered without a walk, with the quiet NaN 0x7fc00000.
 * THE SUM'S ORDER FOLLOWS THE TREE, so -- unlike a signed distance -- the result is NOT promised bit for bit across trees (a
 * split, a rebuild, another builder): it is promised within a tolerance. Measured for points not within 5 % of the shape's size
 * of the surface (profiles/winding_accuracy.log, asserted by tests/test_gpu_winding.py): the exact form within 1e-3 of the
 * float64 sum, and the fast form on the side of 0.5 the float64 sum is on. The same scene object gives the same bits every call.
 *
 * The table of moments (one 128-byte record per node: Nx Ny Nz Px Py Pz R of the four child slots, four floats each, then a copy
 * of the node's four child words: 32 words, so a node step of the walk reads that one line and never the boxes) is made on the
 * device on first use -- by rtk_dev_scene_prepare_winding or by the first rtk_dev_winding_numbers / rtk_dev_scene_winding_moments
 * --, which synchronises `stream` that one time; it counts 128 bytes per node toward total_device_bytes and is released with the
 * scene. It depends on positions AND on the tree: every refit (rtk_dev_scene_refit, _refit_meshes, the _placed forms),
 * rtk_dev_scene_split_leaves and rtk_dev_scene_rebuild drop it, and the next call makes it again.
 * `list`, asynchrony on `stream`, the scratch set and rtk_dev_trace_status: as for rtk_dev_closest_points; A SLOT THAT IS NOT
 * LISTED IS NOT WRITTEN. _counted: rays = queries, nodes = table records fetched, leaves and triangles as for the closest call,
 * hits = far terms taken, stack_spills = pushes past the on-chip part.
 * Refused before any HIP call: RTK_AMD_ERR_BAD_ARG for everything rtk_dev_closest_points refuses, for a NULL d_winding with
 * num_queries != 0, and for opts with a wrong struct_size, an unknown flag, a negative or a NaN beta (beta == 0: the default, 2);
 * RTK_AMD_ERR_UNSUPPORTED for a scene that does not hold exactly one triangle record per primitive (a triangle named twice
 * would be counted twice): nothing is allocated or written. num_queries == 0 is RTK_AMD_OK and does not make the table.
 * Works as it is on rtk_mgpu_scene(m, i). */
typedef struct rtk_winding_opts { uint32_t struct_size; uint32_t flags; float beta; } rtk_winding_opts;
#define RTK_WINDING_EXACT 1u   /* never accept a far term: every triangle is summed (the reference the fast form is measured against) */
typedef struct rtk_dev_winding_info {
	uint64_t nodes;                 /* records of the table: the scene's nodes when it was made */
	uint64_t table_bytes;           /* 128 * nodes */
	double   table_ms;              /* wall time of the last making of the table; 0 if this call found it made */
	double   total_area_vector[3];  /* the sum of N over the root's child slots: near 0 for a closed surface */
	double   total_area;            /* the sum of the triangles' areas, as the table's float sums give it */
} rtk_dev_winding_info;
/* makes the table now if it is not there (synchronises `stream` only when it has to work) */
int rtk_dev_scene_prepare_winding(const rtk_dev_scene *ds, rtk_dev_winding_info *out /* may be NULL */, void *stream);
/* copies the table to d_out[32 * nodes] on `stream` (for tests) */
int rtk_dev_scene_winding_moments(const rtk_dev_scene *ds, float *d_out, void *stream);
int rtk_dev_winding_numbers(const rtk_dev_scene *ds, const rtk_point_query *d_queries, size_t num_queries,
	const rtk_ray_list *list, const rtk_winding_opts *opts /* NULL: beta 2, flags 0 */, float *d_winding, void *stream);
int rtk_dev_winding_numbers_counted(const rtk_dev_scene *ds, const rtk_point_query *d_queries, size_t num_queries,
	const rtk_winding_opts *opts, float *d_winding, rtk_trace_counters *out);
/* (entries per lane the walk keeps on chip before it uses the spill area, for tests) */
uint32_t rtk_amd_winding_stack_entries(void);

/* ---- Triangles within a distance: how many triangles lie within r of a point, and all of them (or the k nearest) ----
 * The question asked in the same breath as "which triangle is nearest": contact generation needs every triangle a sphere
 * touches, robust normals and ICP with outlier rejection the k nearest, photon and sample gathering a radius query. Closest
 * points has no "after": one call per answer cannot even be written. These calls are to closest points what "Every hit along
 * a ray" is to the closest-hit trace, and they read the scene the same way: as it stands, changing no bit of it.
 *
 * THE RULE (rtk_amd/csrc/rtk_within_rule.h on top of rtk_closest_rule.h; INTEGRATION.md "Triangles within a distance"). dist2,
 * u, v and the point q of a triangle are those of closest points, bit for bit. A triangle is a CANDIDATE of the query
 * (p, max_dist2) iff dist2 < max_dist2 -- strictly; a NaN dist2 is never one. A query whose max_dist2 is NaN, zero or negative,
 * or that has a non-finite coordinate, has no candidates; neither has any query of a scene without triangles; RTK_INF means no
 * limit. The LIST of a query is its candidates in ascending (dist2, prim) order, THE LOWEST PRIMITIVE ID FIRST AMONG EQUAL dist2;
 * its first entry is word for word what rtk_dev_closest_points writes for the query. THE RESULT DOES NOT DEPEND ON THE TREE OR
 * ON THE ORDER OF THE WALK: a subtree is left out only if the bound b of its box has b >= max_dist2, or if the query's segment
 * is full and b > worst.dist2 (the last kept entry; strictly, an equal bound can hide a lower id), and the box bound never
 * exceeds the dist2 of a triangle inside the box, without a margin. Only the exact 128-byte nodes are used.
 *
 * rtk_dev_triangles_within_count: d_counts[i] = the number of candidates of query i, written for EVERY answered query (0 for a
 *   query without any); nothing else is written.
 * rtk_dev_triangles_within_all: query i owns d_records[d_offsets[i] .. d_offsets[i + 1]), and d_points[3 j ..] (d_points may be
 *   NULL) belongs to record j; d_offsets has num_queries + 1 entries, indexed by query slot; r = d_offsets[i + 1] - d_offsets[i]
 *   is its room and may be 0. Written are the first min(count_i, r) entries of the query's list, each the rtk_closest_record and
 *   the point closest points would write for that triangle; d_written[i] (d_written may be NULL) is that number. Entries of the
 *   segment beyond it ARE NOT WRITTEN, entries outside every segment are not written. A query whose offsets decrease has no
 *   room and nothing is written for it (d_written[i] = 0). One call serves two uses:
 *     every triangle within r   count, an inclusive prefix sum into uint64 offsets on the same stream (torch.cumsum into an int64
 *                               tensor is one as it stands), then fill;
 *     the k nearest             d_offsets[i] = i * k, no count pass; max_dist2 = RTK_INF if there is no limit. The walk is culled
 *                               by the k-th best distance so far, as closest points culls by the best.
 * `list` may be NULL: all num_queries queries are answered. Otherwise the words of closest points hold: m = min(*d_count,
 * num_queries) entries are answered, the results of query r go to slot r of d_counts / d_written and to segment r, A SLOT THAT
 * IS NOT LISTED IS NOT WRITTEN, an id may repeat (the query is answered once), the count is read when the work reaches it on
 * `stream`, and an id >= num_queries is the caller's error.
 * DETERMINISTIC: the same inputs give the same bytes. Asynchronous on `stream`: no host wait, nothing read back. The scene is
 * only read, as it stands: built, uploaded, refitted, split or rebuilt, and rtk_mgpu_scene(m, i) as it is; the thread-safety
 * rules of the batches hold. The part of the walk's stack that does not fit on chip (and one bit per query for a list with ids)
 * lives in the per-(scene, stream) scratch set, and a dropped push (impossible for a tree) is reported by rtk_dev_trace_status
 * like a trace's. Nothing they allocate counts toward the scene.
 * Refused before anything is launched and before any HIP call, RTK_AMD_ERR_BAD_ARG, with a message that names the function: a
 * NULL scene; NULL d_queries or d_counts, NULL d_offsets or d_records with num_queries != 0; a bad list (as for the listed
 * traces); num_queries >= 2^32; a calling thread whose current device is not the scene's. num_queries == 0 is RTK_AMD_OK with
 * nothing launched. Offsets that run past the caller's buffer are the caller's error and are NOT CHECKED.
 * A scene with non-finite vertex coordinates: the calls terminate and write only inside their outputs; NOTHING ELSE IS PROMISED
 * about their results. */
int rtk_dev_triangles_within_count(const rtk_dev_scene *ds, const rtk_point_query *d_queries, size_t num_queries,
	const rtk_ray_list *list, uint32_t *d_counts, void *stream);
int rtk_dev_triangles_within_all(const rtk_dev_scene *ds, const rtk_point_query *d_queries, size_t num_queries,
	const rtk_ray_list *list, const uint64_t *d_offsets, rtk_closest_record *d_records, float *d_points /* may be NULL */,
	uint32_t *d_written /* may be NULL */, void *stream);
/* The same results without a list, plus visit counts in the fields of rtk_dev_closest_points_counted (hits = queries with at least
 * one candidate counted or kept). d_offsets == NULL: the count form, d_counts_or_written receives the counts (required);
 * otherwise the fill form, d_points and d_counts_or_written may be NULL. Null stream, synchronous; not for timing. */
int rtk_dev_triangles_within_counted(const rtk_dev_scene *ds, const rtk_point_query *d_queries, size_t num_queries,
	const uint64_t *d_offsets, rtk_closest_record *d_records, float *d_points, uint32_t *d_counts_or_written,
	rtk_trace_counters *out);
/* (entries per lane the walk keeps on chip before it uses the spill area, for tests) */
uint32_t rtk_amd_within_stack_entries(void);

/* ---- Triangles that touch a box: how many triangles touch an axis-aligned box, and which ----
 * The region question of the family: voxelisation and occupancy grids, broad-phase collision against a body's bounds, "select
 * everything in this region", tiling a scene for out-of-core work. A sphere around the box's centre through
 * rtk_dev_triangles_within_* over-reports by up to the corner distance, pays a closest-point evaluation with a division per
 * triangle and still leaves the caller to run a box test of their own. This walk is the cheapest the tree offers: box against
 * box, comparisons only, no arithmetic in the skip. The calls read the scene as it stands, changing no bit of it.
 *
 * THE RULE (rtk_amd/csrc/rtk_box_rule.h; INTEGRATION.md "Triangles that touch a box"). All arithmetic is float32, every
 * operation rounded on its own, no FMA. A query is LIVE iff its six numbers are finite and lo[a] <= hi[a] on every axis; lo == hi
 * on one, two or three axes is legal (a rectangle, a segment, a point). A query that is not live has no candidates; neither has
 * any query of a scene without triangles. A triangle is a CANDIDATE of a live query iff its own box (componentwise min / max of
 * its vertices) has tlo[a] <= hi[a] && thi[a] >= lo[a] on all three axes -- CLOSED: touching counts -- and none of the other
 * ten axes of Akenine-Moller's test (the nine unit_i x e_j and the triangle's plane, about the box's centre (lo + hi) * 0.5f with
 * the half extent (hi - lo) * 0.5f) separates the two; a comparison with a NaN never separates. It is a FLOAT RULE and the
 * candidate set is DEFINED BY IT; on inputs whose intermediates are exact it is the exact answer. The LIST of a query is its
 * candidates in ASCENDING PRIMITIVE ID. THE RESULT DOES NOT DEPEND ON THE TREE OR ON THE ORDER OF THE WALK: a child box [clo, chi]
 * is left out only if clo[a] > hi[a] || chi[a] < lo[a] on some axis, exact without a margin because every box above a triangle
 * contains the triangle's own box. Only the exact 128-byte nodes are used.
 *
 * rtk_dev_triangles_in_box_count: d_counts[i] = the number of candidates of query i, written for EVERY answered query (0 for a
 *   query without any); nothing else is written.
 * rtk_dev_triangles_in_box_all: query i owns d_prims[d_offsets[i] .. d_offsets[i + 1]); d_offsets has num_queries + 1 entries,
 *   indexed by query slot; r = d_offsets[i + 1] - d_offsets[i] is its room and may be 0. Written are the first min(count_i, r)
 *   entries of the query's list, each one global primitive id; d_written[i] (d_written may be NULL) is that number. Entries of
 *   the segment beyond it ARE NOT WRITTEN, entries outside every segment are not written. A query whose offsets decrease has
 *   no room and nothing is written for it (d_written[i] = 0). One call serves two uses:
 *     every triangle in the box   count, an inclusive prefix sum into uint64 offsets on the same stream (torch.cumsum into an
 *                                 int64 tensor is one as it stands), then fill;
 *     at most k, deterministic    d_offsets[i] = i * k, no count pass: the k LOWEST ids among the candidates. THAT WALK CANNOT BE
 *                                 CULLED BY WHAT IT HAS KEPT, since the tree is not ordered by id: it visits what the count
 *                                 visits, and a candidate that does not get in costs no memory access.
 * `list` may be NULL: all num_queries queries are answered. Otherwise the words of closest points hold: m = min(*d_count,
 * num_queries) entries are answered, the results of query r go to slot r of d_counts / d_written and to segment r, A SLOT THAT
 * IS NOT LISTED IS NOT WRITTEN, an id may repeat (the query is answered once), the count is read when the work reaches it on
 * `stream`, and an id >= num_queries is the caller's error.
 * DETERMINISTIC: the same inputs give the same bytes. Asynchronous on `stream`: no host wait, nothing read back. The scene is
 * only read, as it stands: built, uploaded, refitted, split or rebuilt, and rtk_mgpu_scene(m, i) as it is; the thread-safety
 * rules of the batches hold. The part of the walk's stack that does not fit on chip (and one bit per query for a list with ids)
 * lives in the per-(scene, stream) scratch set, and a dropped push (impossible for a tree) is reported by rtk_dev_trace_status
 * like a trace's. Nothing they allocate counts toward the scene.
 * Refused before anything is launched and before any HIP call, RTK_AMD_ERR_BAD_ARG, with a message that names the function: a
 * NULL scene; NULL d_boxes or d_counts, NULL d_offsets or d_prims with num_queries != 0; a bad list (as for the listed
 * traces); num_queries >= 2^32; a calling thread whose current device is not the scene's. num_queries == 0 is RTK_AMD_OK with
 * nothing launched. Offsets that run past the caller's buffer are the caller's error and are NOT CHECKED.
 * A scene with non-finite vertex coordinates: the calls terminate and write only inside their outputs; NOTHING ELSE IS PROMISED
 * about their results. */
typedef struct rtk_box_query { float lo[3], hi[3]; } rtk_box_query;      /* 24 bytes; a torch float32 [n, 6] tensor is one */
int rtk_dev_triangles_in_box_count(const rtk_dev_scene *ds, const rtk_box_query *d_boxes, size_t num_queries,
	const rtk_ray_list *list, uint32_t *d_counts, void *stream);
int rtk_dev_triangles_in_box_all(const rtk_dev_scene *ds, const rtk_box_query *d_boxes, size_t num_queries,
	const rtk_ray_list *list, const uint64_t *d_offsets, uint32_t *d_prims, uint32_t *d_written /* may be NULL */, void *stream);
/* The same results without a list, plus visit counts in the fields of rtk_dev_closest_points_counted (hits = queries with at least
 * one candidate counted or kept). d_offsets == NULL: the count form, d_counts_or_written receives the counts (required);
 * otherwise the fill form, d_counts_or_written may be NULL. Null stream, synchronous; not for timing. */
int rtk_dev_triangles_in_box_counted(const rtk_dev_scene *ds, const rtk_box_query *d_boxes, size_t num_queries,
	const uint64_t *d_offsets, uint32_t *d_prims, uint32_t *d_counts_or_written, rtk_trace_counters *out);
/* (entries per lane the walk keeps on chip before it uses the spill area, for tests) */
uint32_t rtk_amd_box_stack_entries(void);

/* ---- Triangles that touch an oriented box: how many triangles touch a box with axes of its own, and which ----
 * The region question for a shape that does not follow the scene's axes: a rigid body's hull, a vehicle chassis, a tilted
 * selection volume; the start test of an oriented sweep and of a depenetration step; voxelising a scene in a body's own frame.
 * rtk_dev_triangles_in_box_* on the hull's world bounds over-reports by everything in the bounds but not in the hull -- a cube
 * turned by 45 degrees about two axes has bounds of several times its volume -- and leaves the caller to filter;
 * rtk_dev_sweep_obbs with a tiny path answers one triangle, not the set. The walk is the axis-aligned one's, box against box on
 * the turned box's bounds, comparisons only; the box's own axes are paid per triangle. The calls read the scene as it stands,
 * changing no bit of it.
 *
 * A query is a rtk_obb_query: `axes` holds three rows u0, u1, u2, the box's own axes in scene coordinates (the rows of a rotation
 * matrix whose rows are those axes); the box is { centre + a0 * u0 + a1 * u1 + a2 * u2 : |aj| <= half[j] }.
 *
 * THE RULE (rtk_amd/csrc/rtk_obb_rule.h; INTEGRATION.md "Triangles that touch an oriented box"). All arithmetic is float32, every
 * operation rounded on its own, no FMA. A query is LIVE iff its fifteen numbers are finite, every half[j] >= 0 and the axes are
 * orthonormal to within 2^-10 (the gate of rtk_dev_sweep_obbs: a gate against garbage, not an accuracy claim; a left-handed
 * triple is a box as well); half == 0 on one, two or three axes is legal (a rectangle, a segment, a point). A query that is not
 * live has no candidates; neither has any query of a scene without triangles. With g[k] = (|u0[k]| * half[0] + |u1[k]| * half[1])
 * + |u2[k]| * half[2] the box's reach along scene axis k, qlo = centre - g and qhi = centre + g, a triangle is a CANDIDATE of a
 * live query iff its own box (componentwise min / max of its vertices) has tlo[a] <= qhi[a] && thi[a] >= qlo[a] on all three
 * axes -- CLOSED: touching counts -- and, with its vertices taken into the box's frame (w = v - centre, then the three dots with
 * u0, u1, u2), none of the thirteen axes separates the two: the box's own three (all three coordinates > half[j] or all
 * < -half[j]) and the ten of Akenine-Moller's test as "Triangles that touch a box" states them, about the origin of the frame
 * with the half extent `half`; a comparison with a NaN never separates. It is a FLOAT RULE and the candidate set is DEFINED BY IT;
 * on inputs whose intermediates are exact it is the exact answer. Identity axes give the answer of rtk_dev_triangles_in_box_* on
 * [centre - half, centre + half] up to rounding only, not bit for bit. The LIST of a query is its candidates in ASCENDING PRIMITIVE
 * ID. THE RESULT DOES NOT DEPEND ON THE TREE OR ON THE ORDER OF THE WALK: a child box [clo, chi] is left out only if
 * clo[a] > qhi[a] || chi[a] < qlo[a] on some axis, exact without a margin because every box above a triangle contains the
 * triangle's own box and the test of the triangle's box against [qlo, qhi] is part of the rule. Only the exact 128-byte nodes
 * are used.
 *
 * rtk_dev_triangles_in_obb_count: d_counts[i] = the number of candidates of query i, written for EVERY answered query (0 for a
 *   query without any); nothing else is written.
 * rtk_dev_triangles_in_obb_all: query i owns d_prims[d_offsets[i] .. d_offsets[i + 1]); d_offsets has num_queries + 1 entries,
 *   indexed by query slot; r = d_offsets[i + 1] - d_offsets[i] is its room and may be 0. Written are the first min(count_i, r)
 *   entries of the query's list, each one global primitive id; d_written[i] (d_written may be NULL) is that number. Entries of
 *   the segment beyond it ARE NOT WRITTEN, entries outside every segment are not written. A query whose offsets decrease has
 *   no room and nothing is written for it (d_written[i] = 0). One call serves two uses:
 *     every triangle in the box   count, an inclusive prefix sum into uint64 offsets on the same stream (torch.cumsum into an
 *                                 int64 tensor is one as it stands), then fill;
 *     at most k, deterministic    d_offsets[i] = i * k, no count pass: the k LOWEST ids among the candidates. THAT WALK CANNOT BE
 *                                 CULLED BY WHAT IT HAS KEPT, since the tree is not ordered by id: it visits what the count
 *                                 visits, and a candidate that does not get in costs no memory access.
 * `list` may be NULL: all num_queries queries are answered. Otherwise the words of closest points hold: m = min(*d_count,
 * num_queries) entries are answered, the results of query r go to slot r of d_counts / d_written and to segment r, A SLOT THAT
 * IS NOT LISTED IS NOT WRITTEN, an id may repeat (the query is answered once), the count is read when the work reaches it on
 * `stream`, and an id >= num_queries is the caller's error.
 * DETERMINISTIC: the same inputs give the same bytes. Asynchronous on `stream`: no host wait, nothing read back. The scene is
 * only read, as it stands: built, uploaded, refitted, split or rebuilt, and rtk_mgpu_scene(m, i) as it is; the thread-safety
 * rules of the batches hold. The part of the walk's stack that does not fit on chip (and one bit per query for a list with ids)
 * lives in the per-(scene, stream) scratch set, and a dropped push (impossible for a tree) is reported by rtk_dev_trace_status
 * like a trace's. Nothing they allocate counts toward the scene.
 * Refused before anything is launched and before any HIP call, RTK_AMD_ERR_BAD_ARG, with a message that names the function: a
 * NULL scene; NULL d_obbs or d_counts, NULL d_offsets or d_prims with num_queries != 0; a bad list (as for the listed
 * traces); num_queries >= 2^32; a calling thread whose current device is not the scene's. num_queries == 0 is RTK_AMD_OK with
 * nothing launched. Offsets that run past the caller's buffer are the caller's error and are NOT CHECKED.
 * A scene with non-finite vertex coordinates: the calls terminate and write only inside their outputs; NOTHING ELSE IS PROMISED
 * about their results. */
typedef struct rtk_obb_query { float centre[3], half[3], axes[9]; } rtk_obb_query;   /* 60 bytes; a float32 [n, 15] tensor */
int rtk_dev_triangles_in_obb_count(const rtk_dev_scene *ds, const rtk_obb_query *d_obbs, size_t num_queries,
	const rtk_ray_list *list, uint32_t *d_counts, void *stream);
int rtk_dev_triangles_in_obb_all(const rtk_dev_scene *ds, const rtk_obb_query *d_obbs, size_t num_queries,
	const rtk_ray_list *list, const uint64_t *d_offsets, uint32_t *d_prims, uint32_t *d_written /* may be NULL */, void *stream);
/* The same results without a list, plus visit counts in the fields of rtk_dev_closest_points_counted (hits = queries with at least
 * one candidate counted or kept). d_offsets == NULL: the count form, d_counts_or_written receives the counts (required);
 * otherwise the fill form, d_counts_or_written may be NULL. Null stream, synchronous; not for timing. */
int rtk_dev_triangles_in_obb_counted(const rtk_dev_scene *ds, const rtk_obb_query *d_obbs, size_t num_queries,
	const uint64_t *d_offsets, uint32_t *d_prims, uint32_t *d_counts_or_written, rtk_trace_counters *out);
/* (entries per lane the walk keeps on chip before it uses the spill area, for tests) */
uint32_t rtk_amd_obb_stack_entries(void);

/* ---- Triangles that touch a triangle: which triangles of the scene a given triangle meets ----
 * The narrow phase that the box query (a body's bounds) and the distance query (contact generation) lead up to: mesh-against-mesh
 * collision, one body's triangles against another body's scene; self-intersection checks of a deforming mesh after a refit;
 * cutting and boolean pre-passes; "does this swept quad hit anything". A box query over-reports by everything that lies in the
 * triangle's box but not on the triangle, and a ray or a distance query cannot put the question at all. The calls read the scene
 * as it stands, changing no bit of it.
 *
 * THE RULE (rtk_amd/csrc/rtk_touch_rule.h; INTEGRATION.md "Triangles that touch a triangle"). All arithmetic is float32, every
 * operation rounded on its own, no FMA. The query A = (v0, v1, v2) is LIVE iff its nine numbers are finite; a query without area
 * (a segment, a point) is live. A query that is not live has no candidates; neither has any query of a scene without triangles.
 * A record B of the scene is a CANDIDATE of a live query iff B's own box (componentwise min / max of its vertices) and A's have
 * tlo[a] <= ahi[a] && thi[a] >= alo[a] on all three axes -- CLOSED: touching counts --, none of the SEVENTEEN AXES separates the
 * two -- the two normals, the nine cross products of an edge of A with an edge of B, and the six in-plane edge normals nA x ea_i,
 * nB x eb_j, all always evaluated; an axis separates iff every projection of B is above every projection of A or every one
 * below, and a comparison with a NaN never separates --, and the filter lets it through. It is a FLOAT RULE and the candidate
 * set is DEFINED BY IT. A separating axis proves disjointness in exact arithmetic, so on inputs whose intermediates are exact
 * the rule never loses a pair that meets, and for two triangles of non-zero area it is then the exact answer; if A or B has no
 * area it may keep a pair that does not meet (a segment in B's plane that passes beside B). The LIST of a query is its
 * candidates in ASCENDING PRIMITIVE ID. THE RESULT DOES NOT DEPEND ON THE TREE OR ON THE ORDER OF THE WALK: a child box is left
 * out only if it is disjoint from A's box by comparison, exact without a margin because every box above a triangle contains the
 * triangle's own box. Only the exact 128-byte nodes are used.
 *
 * THE FILTER is part of the rule and is applied to the record's global primitive id and stored positions. filter == NULL: none.
 *   d_first_prim (may be NULL)      indexed by query slot, like the per-ray filter arrays: a candidate of query i has
 *                                   prim >= d_first_prim[i].
 *   RTK_TOUCH_SKIP_SHARED_VERTEX    a record is not a candidate if one of its vertices equals one of the query's on all three
 *                                   coordinates by float ==. Neighbours in a mesh share positions bit for bit, and a triangle
 *                                   shares them with itself: the flag plus d_first_prim[i] = (the query's own id) + 1 gives each
 *                                   self-intersecting pair of a scene once.
 *
 * rtk_dev_triangles_touching_count: d_counts[i] = the number of candidates of query i, written for EVERY answered query (0 for
 *   a query without any); nothing else is written.
 * rtk_dev_triangles_touching_all: query i owns d_prims[d_offsets[i] .. d_offsets[i + 1]); d_offsets has num_queries + 1 entries,
 *   indexed by query slot; r = d_offsets[i + 1] - d_offsets[i] is its room and may be 0. Written are the first min(count_i, r)
 *   entries of the query's list, each one global primitive id; d_written[i] (d_written may be NULL) is that number. Entries of
 *   the segment beyond it ARE NOT WRITTEN, entries outside every segment are not written. A query whose offsets decrease has
 *   no room and nothing is written for it (d_written[i] = 0). One call serves two uses:
 *     every triangle it meets     count, an inclusive prefix sum into uint64 offsets on the same stream (torch.cumsum into an
 *                                 int64 tensor is one as it stands), then fill;
 *     at most k, deterministic    d_offsets[i] = i * k, no count pass: the k LOWEST ids among the candidates. THAT WALK CANNOT BE
 *                                 CULLED BY WHAT IT HAS KEPT, since the tree is not ordered by id: it visits what the count
 *                                 visits, and a candidate that does not get in costs no memory access.
 * `list` may be NULL: all num_queries queries are answered. Otherwise the words of closest points hold: m = min(*d_count,
 * num_queries) entries are answered, the results of query r go to slot r of d_counts / d_written and to segment r, A SLOT THAT
 * IS NOT LISTED IS NOT WRITTEN, an id may repeat (the query is answered once), the count is read when the work reaches it on
 * `stream`, and an id >= num_queries is the caller's error.
 * DETERMINISTIC: the same inputs give the same bytes. Asynchronous on `stream`: no host wait, nothing read back. The scene is
 * only read, as it stands: built, uploaded, refitted, split or rebuilt, and rtk_mgpu_scene(m, i) as it is; the thread-safety
 * rules of the batches hold. The part of the walk's stack that does not fit on chip (and one bit per query for a list with ids)
 * lives in the per-(scene, stream) scratch set, and a dropped push (impossible for a tree) is reported by rtk_dev_trace_status
 * like a trace's. Nothing they allocate counts toward the scene.
 * Refused before anything is launched and before any HIP call, RTK_AMD_ERR_BAD_ARG, with a message that names the function: a
 * NULL scene; NULL d_tris or d_counts, NULL d_offsets or d_prims with num_queries != 0; a bad list (as for the listed
 * traces); a filter whose struct_size is too small or whose flags hold an unknown bit; num_queries >= 2^32; a calling thread
 * whose current device is not the scene's. num_queries == 0 is RTK_AMD_OK with nothing launched. Offsets that run past the
 * caller's buffer are the caller's error and are NOT CHECKED.
 * A scene with non-finite vertex coordinates: the calls terminate and write only inside their outputs; NOTHING ELSE IS PROMISED
 * about their results. */
typedef struct rtk_tri_query { float v0[3], v1[3], v2[3]; } rtk_tri_query;     /* 36 bytes; a torch float32 [n, 9] tensor is one */
enum { RTK_TOUCH_SKIP_SHARED_VERTEX = 1u };
typedef struct rtk_touch_filter { uint32_t struct_size; uint32_t flags; const uint32_t *d_first_prim; /* device, per query slot; may be NULL */ } rtk_touch_filter;
int rtk_dev_triangles_touching_count(const rtk_dev_scene *ds, const rtk_tri_query *d_tris, size_t num_queries,
	const rtk_ray_list *list, const rtk_touch_filter *filter, uint32_t *d_counts, void *stream);
int rtk_dev_triangles_touching_all(const rtk_dev_scene *ds, const rtk_tri_query *d_tris, size_t num_queries,
	const rtk_ray_list *list, const rtk_touch_filter *filter, const uint64_t *d_offsets, uint32_t *d_prims,
	uint32_t *d_written /* may be NULL */, void *stream);
/* The same results without a list, plus visit counts in the fields of rtk_dev_closest_points_counted (hits = queries with at least
 * one candidate counted or kept). d_offsets == NULL: the count form, d_counts_or_written receives the counts (required);
 * otherwise the fill form, d_counts_or_written may be NULL. Null stream, synchronous; not for timing. */
int rtk_dev_triangles_touching_counted(const rtk_dev_scene *ds, const rtk_tri_query *d_tris, size_t num_queries,
	const rtk_touch_filter *filter, const uint64_t *d_offsets, uint32_t *d_prims, uint32_t *d_counts_or_written, rtk_trace_counters *out);
/* (entries per lane the walk keeps on chip before it uses the spill area, for tests) */
uint32_t rtk_amd_touch_stack_entries(void);

/* ---- Closest triangles: how far a triangle (or a segment, or a point) is from the scene, and where the two nearest points are ----
 * The distance query that stands next to "collide": clearance and minimum separation between two meshes, the distance term of
 * contact models (which need edge-edge as well as point-triangle distances), thickness and self-proximity of a deforming mesh
 * after a refit, safe step sizes. Sampling points for rtk_dev_closest_points misses every edge-edge closest pair, and
 * rtk_dev_triangles_touching_* says "0 or not 0" and nothing more. The call reads the scene as it stands, changing no bit of it.
 *
 * THE RULE (rtk_amd/csrc/rtk_pair_rule.h; INTEGRATION.md "Closest triangles"). All arithmetic is float32, every operation
 * rounded on its own, no FMA. The query A = (v0, v1, v2) is LIVE iff its nine numbers are finite; a query without area (a segment,
 * a point) is live and is a supported use. For a record B of the scene, FIFTEEN FEATURE PAIRS in a fixed order -- A's three
 * vertices against B and B's three against A through the point rule of closest points as it is, then the nine pairs of an edge
 * of A with an edge of B by a segment-segment routine whose parallel and zero-length cases are selects, never 0 / 0, without an
 * epsilon -- each give a point qa on A and a point qb on B; qa IS CLAMPED TO A'S OWN BOX AND qb TO B'S OWN BOX, and dist2 is the
 * squared difference of the two clamped points. The pair's result is the feature with the smallest dist2, the first in the order
 * among equal ones; a NaN never wins. PIERCING: if the two triangles' own boxes touch (closed) and an edge of one goes through the
 * other -- its end points strictly on opposite sides of the plane, the three scalar triple products of one sign, zero as either
 * sign but not all three zero --, dist2 = 0 and qa = qb = the crossing point, clamped to the boxes' intersection; the first of
 * the six edges in the order decides. The seventeen axes of the touching calls are not used: a segment beside a triangle gets its
 * true distance. It is a FLOAT RULE and the result is DEFINED BY IT. The answer to (A, max_dist2) is, over all records that the
 * filter lets through and whose dist2 < max_dist2 -- strictly --, the smallest dist2, THE LOWEST PRIMITIVE ID AMONG EQUAL dist2,
 * or a miss. THE RESULT DOES NOT DEPEND ON THE TREE OR ON THE ORDER OF THE WALK: a subtree is left out only if the bound b of its
 * box against A's box (per axis the gap max(lo - ahi, alo - hi, 0), squared and summed in dist2's order) has b > best dist2 so
 * far -- strictly, an equal bound can hide a lower id -- or b >= max_dist2, and that bound never exceeds the dist2 of a record
 * inside the box, without a margin, because qa lies in A's box and qb in a box inside the node's. Only the exact 128-byte nodes
 * are used.
 *   hit    dist2, u and v (the weights of B's vertex 0 and vertex 1 at qb) and the global primitive id;
 *          d_points_query[3 i ..] = qa, d_points_scene[3 i ..] = qb
 *   miss   dist2 = max_dist2 as given (RTK_INF with a NULL array), u = v = 0, prim = RTK_PRIM_NONE; both points = the query's
 *          vertex 0 as given
 * The record is rtk_closest_record: rtk_dev_select_rays (RTK_SELECT_RECORD_HIT / _MISS) and rtk_dev_expand_hits take it as it
 * is. A query that is not live is a miss; so is one whose max_dist2 is NaN, zero or negative, and any query of a scene without
 * triangles. d_max_dist2 is indexed by query slot; NULL means RTK_INF, no limit, for every query.
 *
 * THE FILTER is part of the rule: rtk_touch_filter as for the touching calls (d_first_prim indexed by query slot, and
 * RTK_TOUCH_SKIP_SHARED_VERTEX), applied to the record's global primitive id and stored positions. The flag together with
 * d_first_prim[i] = (the query's own id) + 1 gives each triangle of a mesh its nearest non-adjacent triangle of a higher id:
 * the minimum over the mesh is its self-clearance.
 *
 * `list` may be NULL: all num_queries queries are answered. Otherwise the words of closest points hold: m = min(*d_count,
 * num_queries) entries are answered, the result of query r goes to slot r of d_records (and of the point arrays), A SLOT THAT IS
 * NOT LISTED IS NOT WRITTEN, an id may repeat, the count is read when the work reaches it on `stream`, and an id >= num_queries
 * is the caller's error. d_points_query and d_points_scene may each be NULL.
 * DETERMINISTIC: the same inputs give the same bytes. Asynchronous on `stream`: no host wait, nothing read back. The scene is
 * only read, as it stands: built, uploaded, refitted, split or rebuilt, and rtk_mgpu_scene(m, i) as it is; the thread-safety
 * rules of the batches hold. The part of the walk's stack that does not fit on chip lives in the per-(scene, stream) scratch
 * set, and a dropped push (impossible for a tree) is reported by rtk_dev_trace_status like a trace's. Nothing it allocates
 * counts toward the scene.
 * Refused before anything is launched and before any HIP call, RTK_AMD_ERR_BAD_ARG, with a message that names the function: a
 * NULL scene; NULL d_tris or d_records with num_queries != 0; a bad list (as for the listed traces); a filter whose struct_size
 * is too small or whose flags hold an unknown bit; num_queries >= 2^32; a calling thread whose current device is not the
 * scene's. num_queries == 0 is RTK_AMD_OK with nothing launched.
 * A scene with non-finite vertex coordinates: the call terminates and writes only inside its outputs; NOTHING ELSE IS PROMISED
 * about its results. */
int rtk_dev_closest_triangles(const rtk_dev_scene *ds, const rtk_tri_query *d_tris, size_t num_queries,
	const rtk_ray_list *list, const rtk_touch_filter *filter, const float *d_max_dist2 /* per query slot; NULL = RTK_INF */,
	rtk_closest_record *d_records, float *d_points_query /* may be NULL */, float *d_points_scene /* may be NULL */, void *stream);
/* The same results without a list, plus visit counts in the fields of rtk_dev_closest_points_counted (triangles = records
 * fetched, of which those that their own box rules out are not evaluated). Null stream, synchronous; not for timing. */
int rtk_dev_closest_triangles_counted(const rtk_dev_scene *ds, const rtk_tri_query *d_tris, size_t num_queries,
	const rtk_touch_filter *filter, const float *d_max_dist2, rtk_closest_record *d_records, float *d_points_query,
	float *d_points_scene, rtk_trace_counters *out);
/* (entries per lane the walk keeps on chip before it uses the spill area, for tests) */
uint32_t rtk_amd_pair_stack_entries(void);

/* ---- Triangles near a triangle: how many triangles lie within a distance of a triangle, and all of them (or the k nearest) ----
 * The last cell of the proximity family: mesh-against-mesh contact generation needs EVERY scene triangle within a contact margin
 * of a body's triangle, with the two nearest points of each pair. rtk_dev_closest_triangles returns one pair per query and has
 * no "after" -- one call per answer cannot be written --, rtk_dev_triangles_touching_* says "0 or not 0" and gives no points,
 * and sampling points for rtk_dev_triangles_within_* misses every edge-edge pair. These calls are to closest triangles what
 * "Triangles within a distance" is to closest points, and they read the scene the same way: as it stands, changing no bit of it.
 *
 * THE RULE (rtk_amd/csrc/rtk_near_rule.h on top of rtk_pair_rule.h; INTEGRATION.md "Triangles near a triangle"). dist2, u, v and
 * the two points qa, qb of a (query, record) pair are those of closest triangles, bit for bit (rtk_pair_evaluate): the fifteen
 * feature pairs, PIERCING (dist2 = 0, qa = qb) and both box clamps included. THE FILTER is rtk_touch_filter as for the touching
 * calls (d_first_prim indexed by query slot, and RTK_TOUCH_SKIP_SHARED_VERTEX), applied to the record's global primitive id and
 * stored positions. A record is a CANDIDATE of the query (A, max_dist2) iff the query is live (its nine numbers finite; a segment
 * or a point is live), max_dist2 > 0, the filter passes and dist2 < max_dist2 -- strictly; a NaN dist2 is never one. A query
 * that is not live or whose max_dist2 is NaN, zero or negative has no candidates; neither has any query of a scene without
 * triangles. d_max_dist2 is indexed by query slot; NULL means RTK_INF, no limit, for every query. The LIST of a query is its
 * candidates in ascending (dist2, prim) order, THE LOWEST PRIMITIVE ID FIRST AMONG EQUAL dist2: pierced pairs all have dist2 = 0
 * and come first, by id. Its first entry, with its two points, is word for word what rtk_dev_closest_triangles writes for the
 * query. THE RESULT DOES NOT DEPEND ON THE TREE OR ON THE ORDER OF THE WALK: a subtree -- or a record, by its own box -- is left
 * out only if the bound b of its box against A's box has b >= max_dist2, or if the query's segment is full and b > worst.dist2
 * (the last kept entry; strictly, an equal bound can hide a lower id), and that bound never exceeds the dist2 of a record inside
 * the box, without a margin. Only the exact 128-byte nodes are used.
 *
 * rtk_dev_triangles_near_count: d_counts[i] = the number of candidates of query i, written for EVERY answered query (0 for a
 *   query without any); nothing else is written.
 * rtk_dev_triangles_near_all: query i owns d_records[d_offsets[i] .. d_offsets[i + 1]), and d_points_query[3 j ..] and
 *   d_points_scene[3 j ..] (each may be NULL) belong to record j; d_offsets has num_queries + 1 entries, indexed by query slot;
 *   r = d_offsets[i + 1] - d_offsets[i] is its room and may be 0. Written are the first min(count_i, r) entries of the query's
 *   list, each the rtk_closest_record and the points qa (on the query) and qb (on the scene) closest triangles would write for
 *   that record; d_written[i] (d_written may be NULL) is that number. Entries of the segment beyond it ARE NOT WRITTEN, entries
 *   outside every segment are not written. A query whose offsets decrease has no room and nothing is written for it
 *   (d_written[i] = 0). One call serves two uses:
 *     every triangle within r   count, an inclusive prefix sum into uint64 offsets on the same stream (torch.cumsum into an int64
 *                               tensor is one as it stands), then fill with the same limits and filter;
 *     the k nearest             d_offsets[i] = i * k, no count pass; d_max_dist2 = NULL if there is no limit. The walk is culled
 *                               by the k-th best distance so far, as closest triangles culls by the best.
 * `list` may be NULL: all num_queries queries are answered. Otherwise the words of the within calls hold: m = min(*d_count,
 * num_queries) entries are answered, the results of query r go to slot r of d_counts / d_written and to segment r, A SLOT THAT
 * IS NOT LISTED IS NOT WRITTEN, an id may repeat (the query is answered once), the count is read when the work reaches it on
 * `stream`, and an id >= num_queries is the caller's error.
 * DETERMINISTIC: the same inputs give the same bytes. Asynchronous on `stream`: no host wait, nothing read back. The scene is
 * only read, as it stands: built, uploaded, refitted, split or rebuilt, and rtk_mgpu_scene(m, i) as it is; the thread-safety
 * rules of the batches hold. The part of the walk's stack that does not fit on chip (and one bit per query for a list with ids)
 * lives in the per-(scene, stream) scratch set, and a dropped push (impossible for a tree) is reported by rtk_dev_trace_status
 * like a trace's. Nothing they allocate counts toward the scene.
 * Refused before anything is launched and before any HIP call, RTK_AMD_ERR_BAD_ARG, with a message that names the function: a
 * NULL scene; NULL d_tris or d_counts, NULL d_offsets or d_records with num_queries != 0; a bad list (as for the listed
 * traces); a filter whose struct_size is too small or whose flags hold an unknown bit; num_queries >= 2^32; a calling thread
 * whose current device is not the scene's. num_queries == 0 is RTK_AMD_OK with nothing launched. Offsets that run past the
 * caller's buffer are the caller's error and are NOT CHECKED.
 * The weakness of the pair rule holds here as well: two triangles in one plane up to rounding whose boxes touch can be called
 * pierced by rounding errors. A scene with non-finite vertex coordinates: the calls terminate and write only inside their
 * outputs; NOTHING ELSE IS PROMISED about their results. */
int rtk_dev_triangles_near_count(const rtk_dev_scene *ds, const rtk_tri_query *d_tris, size_t num_queries,
	const rtk_ray_list *list, const rtk_touch_filter *filter, const float *d_max_dist2 /* per query slot; NULL = RTK_INF */,
	uint32_t *d_counts, void *stream);
int rtk_dev_triangles_near_all(const rtk_dev_scene *ds, const rtk_tri_query *d_tris, size_t num_queries,
	const rtk_ray_list *list, const rtk_touch_filter *filter, const float *d_max_dist2, const uint64_t *d_offsets,
	rtk_closest_record *d_records, float *d_points_query /* may be NULL */, float *d_points_scene /* may be NULL */,
	uint32_t *d_written /* may be NULL */, void *stream);
/* The same results without a list, plus visit counts in the fields of rtk_dev_closest_points_counted (triangles = records
 * fetched, of which those that the filter or their own box rules out are not evaluated; hits = queries with at least one
 * candidate counted or kept). d_offsets == NULL: the count form, d_counts_or_written receives the counts (required); otherwise
 * the fill form, the point arrays and d_counts_or_written may be NULL. Null stream, synchronous; not for timing. */
int rtk_dev_triangles_near_counted(const rtk_dev_scene *ds, const rtk_tri_query *d_tris, size_t num_queries,
	const rtk_touch_filter *filter, const float *d_max_dist2, const uint64_t *d_offsets, rtk_closest_record *d_records,
	float *d_points_query, float *d_points_scene, uint32_t *d_counts_or_written, rtk_trace_counters *out);
/* (entries per lane the walk keeps on chip before it uses the spill area, for tests) */
uint32_t rtk_amd_near_stack_entries(void);

/* ---- Sphere sweeps: how far a ball can move along a direction before it first touches the scene, and where it touches ----
 * The third question of a collision layer beside raycast and overlap: character and camera controllers, continuous collision of
 * small fast bodies (which tunnel through a discrete "within" check), thick-ray visibility and line of sight with clearance,
 * probe placement. A ray misses everything a ball of radius r grazes, and marching the "within" calls along the path costs one
 * walk per step and only brackets the answer. The scene is read as it stands -- a device build, an uploaded blob, after any
 * refit, split or rebuild -- and no bit of it changes.
 *
 * A query is a rtk_sphere_sweep: the ball's centre is c(t) = origin + direction * t, t in units of `direction` (which need not
 * be normalised) over the CLOSED interval [min_t, max_t] -- not a ray's open one: a ball that already touches at the start is a
 * hit at the start (min_t, or the float above it: the rule's 2. (ii)), and no time outside [min_t, max_t] is ever reported. A
 * torch float32 [n, 9] tensor is an array of them.
 *
 * THE RULE (rtk_amd/csrc/rtk_sweep_rule.h; INTEGRATION.md "Sphere sweeps"): THE RESULT DOES NOT DEPEND ON THE TREE. It is a
 * function of the scene's triangle records, the filter and the query alone, stated in float arithmetic, every operation rounded
 * on its own. Every triangle has a time or none: none if the path misses the triangle's own box grown by the radius; the start if the
 * ball at min_t is within the radius of it (touching counts); otherwise the smallest time at which the ball reaches the
 * face, one of the three edges or one of the three vertices, the maximum of that time and the entry time of the grown box, and none if that exceeds max_t. The
 * answer is the smallest time, THE LOWEST PRIMITIVE ID AMONG EQUAL TIMES, or a miss. Leaf sizes, loose boxes and the node
 * format only decide how many triangles are never looked at.
 *   hit    t, u (weight of vertex 0), v (weight of vertex 1) and the global primitive id: a rtk_hit_record, which
 *          rtk_dev_select_rays and rtk_dev_expand_hits take as it is; d_points[3 i ..] = the contact point on the triangle,
 *          d_centres[3 i ..] = c(t) as the rule computed it; u, v and the contact point are those of the point of the triangle
 *          nearest to c(t) (one rtk_closest_rule.h evaluation)
 *   miss   t = max_t as given, u = v = 0, prim = RTK_PRIM_NONE; d_points[3 i ..] = d_centres[3 i ..] = the origin as given
 * A query is live iff origin, direction, min_t, max_t and radius are finite (RTK_INF is a finite number: "no limit"), the
 * direction is not all zeros, radius >= 0 and min_t <= max_t; a query that is not live is a miss, and so is every query of a
 * scene without triangles. radius == 0 is legal and is this rule on a point: it is NOT rtk's watertight ray test, and its
 * results are not bit-equal to a trace's.
 * THE FILTER is part of the rule: of a rtk_dev_filter, d_mesh_mask (with mesh_mask_bits) and d_ignore_prim (read per query slot)
 * say which triangles are candidates, as for the filtered traces; a non-NULL d_after is refused. `filter` may be NULL.
 * rtk_dev_sweep_spheres_any answers "is the path blocked": d_blocked[i] = 1 if query i has a candidate with a time, else 0 --
 * exactly prim != RTK_PRIM_NONE of rtk_dev_sweep_spheres; its walk ends at the first one it meets.
 * `list` may be NULL: all num_sweeps queries are answered. Otherwise the words of the listed traces hold: m = min(*d_count,
 * num_sweeps) entries are answered, the result of query r goes to slot r of the outputs, d_ignore_prim is read at slot r, A SLOT
 * THAT IS NOT LISTED IS NOT WRITTEN, an id may repeat, and the count is read when the work reaches it on `stream`. d_points and
 * d_centres may each be NULL.
 * Asynchronous on `stream`: no host wait, nothing read back. The scene is only read, so the thread-safety rules of the batches
 * hold; the part of the walk's stack that does not fit on chip lives in the per-(scene, stream) scratch set, and a dropped push
 * (impossible for a tree) is reported by rtk_dev_trace_status like a trace's. Nothing it allocates counts toward the scene.
 * Refused before anything is launched, RTK_AMD_ERR_BAD_ARG: a NULL scene; NULL d_sweeps or a NULL d_records / d_blocked with
 * num_sweeps != 0; a bad list (as for the listed traces); a filter whose struct_size is too small, whose d_after is set or whose
 * mesh mask has no bits; num_sweeps >= 2^32; a calling thread whose current device is not the scene's. num_sweeps == 0 is
 * RTK_AMD_OK with nothing launched. Works as it is on rtk_mgpu_scene(m, i).
 * A scene with non-finite vertex coordinates: the call terminates and writes only inside its outputs; NOTHING ELSE IS PROMISED
 * about its results. */
typedef struct rtk_sphere_sweep { float origin[3], direction[3], min_t, max_t, radius; } rtk_sphere_sweep;   /* 36 bytes */
int rtk_dev_sweep_spheres(const rtk_dev_scene *ds, const rtk_sphere_sweep *d_sweeps, size_t num_sweeps, const rtk_ray_list *list,
	rtk_hit_record *d_records, float *d_points /* may be NULL */, float *d_centres /* may be NULL */,
	const rtk_dev_filter *filter /* may be NULL */, void *stream);
int rtk_dev_sweep_spheres_any(const rtk_dev_scene *ds, const rtk_sphere_sweep *d_sweeps, size_t num_sweeps, const rtk_ray_list *list,
	uint8_t *d_blocked, const rtk_dev_filter *filter, void *stream);
/* Same result as rtk_dev_sweep_spheres without a list, plus visit counts in the fields of rtk_dev_closest_points_counted (rays =
 * queries answered; triangles = records fetched, of which those the filter rules out are not evaluated; hits = queries that
 * found a triangle). Null stream, synchronous; not for timing. */
int rtk_dev_sweep_spheres_counted(const rtk_dev_scene *ds, const rtk_sphere_sweep *d_sweeps, size_t num_sweeps,
	rtk_hit_record *d_records, float *d_points, float *d_centres, const rtk_dev_filter *filter, rtk_trace_counters *out);
/* (entries per lane the walk keeps on chip before it uses the spill area, for tests) */
uint32_t rtk_amd_sweep_stack_entries(void);

/* ---- Box sweeps: how far an axis-aligned box can move along a direction before it first touches the scene ----
 * The sweep engines use for bodies: character and vehicle hulls, camera collision, continuous collision of a body's bounds,
 * conservative advancement of a rigid body by its box, "does this voxel, tile or crate fit along this path". A ball is a poor
 * stand-in: the inscribed one tunnels at the corners, the circumscribed one gets stuck in doorways the hull fits through; and
 * marching rtk_dev_triangles_in_box_count along the path costs one walk per step and only brackets the time. The scene is read
 * as it stands -- a device build, an uploaded blob, after any refit, split or rebuild -- and no bit of it changes.
 *
 * A query is a rtk_box_sweep: the box at time t is [c(t) - half, c(t) + half] with the centre c(t) = origin + direction * t, t
 * in units of `direction` (which need not be normalised) over the CLOSED interval [min_t, max_t] -- not a ray's open one: a box
 * that already overlaps a triangle at min_t is a hit at the start, and no time outside [min_t, max_t] is ever reported. A torch
 * float32 [n, 11] tensor is an array of them. The box keeps the scene's axes: a box with axes of its own is
 * rtk_dev_sweep_obbs, "Oriented box sweeps" below.
 *
 * THE RULE (rtk_amd/csrc/rtk_boxsweep_rule.h; INTEGRATION.md "Box sweeps"): THE RESULT DOES NOT DEPEND ON THE TREE. It is a
 * function of the scene's triangle records, the filter and the query alone, stated in float arithmetic, every operation rounded
 * on its own. Every triangle has a time or none, by swept separating axes: none if the path of the centre misses the triangle's
 * own box grown by the half extents; otherwise the other ten axes -- the triangle's normal and the nine cross products of an
 * edge and a box axis --, measured from the centre at the entry into that grown box, each give an interval of times at which
 * they do not separate the two; the time is the start of the intersection of all of them, none if it is empty, never earlier
 * than the entry into the grown box, and none if it exceeds max_t. The answer is the smallest time, THE LOWEST PRIMITIVE ID
 * AMONG EQUAL TIMES, or a miss. Leaf sizes, loose boxes and the node format only decide how many triangles are never looked at.
 *   hit    t, u (weight of vertex 0), v (weight of vertex 1) and the global primitive id: a rtk_hit_record, which
 *          rtk_dev_select_rays and rtk_dev_expand_hits take as it is. u and v are those of the point of the triangle nearest to
 *          the centre c(t) (one rtk_closest_rule.h evaluation): A WITNESS ON THE TRIANGLE, NOT NECESSARILY A POINT OF CONTACT
 *          (a box touches with a corner, an edge or a face, and the nearest point to its centre may be elsewhere on the
 *          triangle). d_centres[3 i ..] = c(t) as the rule computed it; d_normals[3 i ..] = the unit separating axis that gave
 *          the entry time, turned against the motion (dot(normal, direction) < 0): the contact normal a controller slides
 *          along. It is all zeros where the box already overlaps at the start, or where the axis has no length in float; it
 *          is never a NaN for a live query and a finite scene.
 *   miss   t = max_t as given, u = v = 0, prim = RTK_PRIM_NONE; d_centres[3 i ..] = the origin as given, d_normals[3 i ..] = 0
 * A query is live iff all eleven floats are finite (RTK_INF is a finite number: "no limit"), the direction is not all zeros,
 * every half[k] >= 0 and min_t <= max_t; a query that is not live is a miss, and so is every query of a scene without
 * triangles. half == 0 on one, two or all three axes is legal: a rectangle, a segment and a point are boxes; on a point the rule
 * is NOT rtk's watertight ray test, and its results are not bit-equal to a trace's.
 * THE FILTER is part of the rule: of a rtk_dev_filter, d_mesh_mask (with mesh_mask_bits) and d_ignore_prim (read per query slot)
 * say which triangles are candidates, as for the filtered traces; a non-NULL d_after is refused. `filter` may be NULL.
 * rtk_dev_sweep_boxes_any answers "is the path blocked": d_blocked[i] = 1 if query i has a candidate with a time, else 0 --
 * exactly prim != RTK_PRIM_NONE of rtk_dev_sweep_boxes; its walk ends at the first one it meets.
 * `list` may be NULL: all num_sweeps queries are answered. Otherwise the words of the listed traces hold: m = min(*d_count,
 * num_sweeps) entries are answered, the result of query r goes to slot r of the outputs, d_ignore_prim is read at slot r, A SLOT
 * THAT IS NOT LISTED IS NOT WRITTEN, an id may repeat, and the count is read when the work reaches it on `stream`. d_centres and
 * d_normals may each be NULL.
 * Asynchronous on `stream`: no host wait, nothing read back. The scene is only read, so the thread-safety rules of the batches
 * hold; the part of the walk's stack that does not fit on chip lives in the per-(scene, stream) scratch set, and a dropped push
 * (impossible for a tree) is reported by rtk_dev_trace_status like a trace's. Nothing it allocates counts toward the scene.
 * Refused before anything is launched, RTK_AMD_ERR_BAD_ARG: a NULL scene; NULL d_sweeps or a NULL d_records / d_blocked with
 * num_sweeps != 0; a bad list (as for the listed traces); a filter whose struct_size is too small, whose d_after is set or whose
 * mesh mask has no bits; num_sweeps >= 2^32; a calling thread whose current device is not the scene's. num_sweeps == 0 is
 * RTK_AMD_OK with nothing launched. Works as it is on rtk_mgpu_scene(m, i).
 * A scene with non-finite vertex coordinates: the call terminates and writes only inside its outputs; NOTHING ELSE IS PROMISED
 * about its results. */
typedef struct rtk_box_sweep { float origin[3], direction[3], min_t, max_t, half[3]; } rtk_box_sweep;   /* 44 bytes; a float32 [n, 11] tensor */
int rtk_dev_sweep_boxes(const rtk_dev_scene *ds, const rtk_box_sweep *d_sweeps, size_t num_sweeps, const rtk_ray_list *list,
	rtk_hit_record *d_records, float *d_centres /* may be NULL */, float *d_normals /* may be NULL */,
	const rtk_dev_filter *filter /* may be NULL */, void *stream);
int rtk_dev_sweep_boxes_any(const rtk_dev_scene *ds, const rtk_box_sweep *d_sweeps, size_t num_sweeps, const rtk_ray_list *list,
	uint8_t *d_blocked, const rtk_dev_filter *filter, void *stream);
/* Same result as rtk_dev_sweep_boxes without a list, plus visit counts in the fields of rtk_dev_closest_points_counted (rays =
 * queries answered; triangles = records fetched, of which those the filter rules out are not evaluated; hits = queries that
 * found a triangle). Null stream, synchronous; not for timing. */
int rtk_dev_sweep_boxes_counted(const rtk_dev_scene *ds, const rtk_box_sweep *d_sweeps, size_t num_sweeps,
	rtk_hit_record *d_records, float *d_centres, float *d_normals, const rtk_dev_filter *filter, rtk_trace_counters *out);
/* (entries per lane the walk keeps on chip before it uses the spill area, for tests) */
uint32_t rtk_amd_boxsweep_stack_entries(void);

/* ---- Capsule sweeps: how far a capsule (a segment with a radius) can move along a direction before it first touches the scene ----
 * The shape a character or camera controller sweeps, a thick limb, a cable segment, a tool shaft. Neither other sweep stands in
 * for it: a ball of the capsule's radius tunnels with the body's ends, a ball that encloses it gets stuck in every doorway, and
 * the axis-aligned box cannot lean; marching rtk_dev_triangles_near_count along the path costs one walk per step and only
 * brackets the time. The scene is read as it stands -- a device build, an uploaded blob, after any refit, split or rebuild --
 * and no bit of it changes.
 *
 * A query is a rtk_capsule_sweep: the capsule at time t is every point within `radius` of the segment from c(t) - half_axis to
 * c(t) + half_axis, with the centre c(t) = origin + direction * t, t in units of `direction` (which need not be normalised)
 * over the CLOSED interval [min_t, max_t] -- not a ray's open one: a capsule that already touches a triangle at min_t is a hit
 * at the start, and no time outside [min_t, max_t] is ever reported. The capsule does not rotate; its axis may point anywhere.
 * A torch float32 [n, 12] tensor is an array of them.
 *
 * THE RULE (rtk_amd/csrc/rtk_capsule_rule.h; INTEGRATION.md "Capsule sweeps"): THE RESULT DOES NOT DEPEND ON THE TREE. It is a
 * function of the scene's triangle records, the filter and the query alone, stated in float arithmetic, every operation rounded
 * on its own. Every triangle has a time or none: none if the path of the centre misses the triangle's own box grown by
 * radius + |half_axis[k]| on axis k; the entry into that box if the capsule at the start is within `radius` of the triangle
 * (its axis going through the triangle, or the smallest of five distances: the axis's two ends against the triangle and the
 * axis against the three edges); otherwise the smallest valid entry time of a ball of that radius into the 26 features of the
 * prism the triangle sweeps out along +-half_axis -- eight faces, twelve edges, six vertices, the first in the rule's order
 * among equal times --, measured from the centre at the entry into the grown box, never earlier than that entry, and none if
 * it exceeds max_t. The answer is the smallest time, THE LOWEST PRIMITIVE ID AMONG EQUAL TIMES, or a miss. Leaf sizes, loose
 * boxes and the node format only decide how many triangles are never looked at.
 *   hit    t, u (weight of vertex 0), v (weight of vertex 1) and the global primitive id: a rtk_hit_record, which
 *          rtk_dev_select_rays and rtk_dev_expand_hits take as it is. ONE evaluation of the rule's distance walk at c(t) on the
 *          answer's triangle gives u, v and both points: d_points[3 i ..] = the point of the triangle nearest the capsule's
 *          segment at that time, d_axis_points[3 i ..] = the point of the capsule's segment nearest the triangle. A
 *          controller's contact normal is their difference (of length `radius` up to rounding at a first contact; zero where
 *          the axis itself goes through the triangle, where both are the point of crossing).
 *   miss   t = max_t as given, u = v = 0, prim = RTK_PRIM_NONE; d_points[3 i ..] = d_axis_points[3 i ..] = the origin as given
 * A query is live iff all twelve floats are finite (RTK_INF is a finite number: "no limit"), the direction is not all zeros,
 * radius >= 0 and min_t <= max_t; a query that is not live is a miss, and so is every query of a scene without triangles.
 * half_axis == 0 is legal and is a ball; radius == 0 is legal and is a moving segment; both at once is a point, on which the
 * rule is NOT rtk's watertight ray test, and its results are not bit-equal to a trace's. half_axis == 0 IS NOT PROMISED
 * BIT-EQUAL TO rtk_dev_sweep_spheres: the start test is a different float expression (the times from features are the same).
 * THE FILTER is part of the rule: of a rtk_dev_filter, d_mesh_mask (with mesh_mask_bits) and d_ignore_prim (read per query slot)
 * say which triangles are candidates, as for the filtered traces; a non-NULL d_after is refused. `filter` may be NULL.
 * rtk_dev_sweep_capsules_any answers "is the path blocked": d_blocked[i] = 1 if query i has a candidate with a time, else 0 --
 * exactly prim != RTK_PRIM_NONE of rtk_dev_sweep_capsules; its walk ends at the first one it meets.
 * `list` may be NULL: all num_sweeps queries are answered. Otherwise the words of the listed traces hold: m = min(*d_count,
 * num_sweeps) entries are answered, the result of query r goes to slot r of the outputs, d_ignore_prim is read at slot r, A SLOT
 * THAT IS NOT LISTED IS NOT WRITTEN, an id may repeat, and the count is read when the work reaches it on `stream`. d_points and
 * d_axis_points may each be NULL.
 * Asynchronous on `stream`: no host wait, nothing read back. The scene is only read, so the thread-safety rules of the batches
 * hold; the part of the walk's stack that does not fit on chip lives in the per-(scene, stream) scratch set, and a dropped push
 * (impossible for a tree) is reported by rtk_dev_trace_status like a trace's. Nothing it allocates counts toward the scene.
 * Refused before anything is launched, RTK_AMD_ERR_BAD_ARG: a NULL scene; NULL d_sweeps or a NULL d_records / d_blocked with
 * num_sweeps != 0; a bad list (as for the listed traces); a filter whose struct_size is too small, whose d_after is set or whose
 * mesh mask has no bits; num_sweeps >= 2^32; a calling thread whose current device is not the scene's. num_sweeps == 0 is
 * RTK_AMD_OK with nothing launched. Works as it is on rtk_mgpu_scene(m, i).
 * A scene with non-finite vertex coordinates: the call terminates and writes only inside its outputs; NOTHING ELSE IS PROMISED
 * about its results. */
typedef struct rtk_capsule_sweep { float origin[3], direction[3], min_t, max_t, radius, half_axis[3]; } rtk_capsule_sweep;   /* 48 bytes; a float32 [n, 12] tensor */
int rtk_dev_sweep_capsules(const rtk_dev_scene *ds, const rtk_capsule_sweep *d_sweeps, size_t num_sweeps, const rtk_ray_list *list,
	rtk_hit_record *d_records, float *d_points /* may be NULL */, float *d_axis_points /* may be NULL */,
	const rtk_dev_filter *filter /* may be NULL */, void *stream);
int rtk_dev_sweep_capsules_any(const rtk_dev_scene *ds, const rtk_capsule_sweep *d_sweeps, size_t num_sweeps, const rtk_ray_list *list,
	uint8_t *d_blocked, const rtk_dev_filter *filter, void *stream);
/* Same result as rtk_dev_sweep_capsules without a list, plus visit counts in the fields of rtk_dev_closest_points_counted (rays =
 * queries answered; triangles = records fetched, of which those the filter rules out are not evaluated; hits = queries that
 * found a triangle). Null stream, synchronous; not for timing. */
int rtk_dev_sweep_capsules_counted(const rtk_dev_scene *ds, const rtk_capsule_sweep *d_sweeps, size_t num_sweeps,
	rtk_hit_record *d_records, float *d_points, float *d_axis_points, const rtk_dev_filter *filter, rtk_trace_counters *out);
/* (entries per lane the walk keeps on chip before it uses the spill area, for tests) */
uint32_t rtk_amd_capsule_stack_entries(void);

/* ---- Oriented box sweeps: how far a box with axes of its own can move along a direction before it first touches the scene ----
 * A rigid body's hull, a vehicle chassis, a crate on a ramp, a rotated camera volume: a box that does not keep the scene's axes.
 * rtk_dev_sweep_boxes cannot lean, and turning the scene instead (placed meshes and a refit) costs one pass over the whole scene
 * per orientation; here every query of a batch carries its own rotation. The box does not turn while it moves. The scene is
 * read as it stands -- a device build, an uploaded blob, after any refit, split or rebuild -- and no bit of it changes.
 *
 * A query is a rtk_obb_sweep: `axes` holds three rows u0, u1, u2, the box's own axes in scene coordinates (the rows of a rotation
 * matrix that takes scene coordinates to the box's), and the box at time t is { c(t) + a0 * u0 + a1 * u1 + a2 * u2 :
 * |aj| <= half[j] } with the centre c(t) = origin + direction * t, t in units of `direction` (which need not be normalised) over
 * the CLOSED interval [min_t, max_t] -- not a ray's open one: a box that already overlaps a triangle at min_t is a hit at the
 * start, and no time outside [min_t, max_t] is ever reported. A torch float32 [n, 20] tensor is an array of them.
 *
 * THE RULE (rtk_amd/csrc/rtk_obbsweep_rule.h; INTEGRATION.md "Oriented box sweeps"): THE RESULT DOES NOT DEPEND ON THE TREE. It is
 * a function of the scene's triangle records, the filter and the query alone, stated in float arithmetic, every operation
 * rounded on its own. Every triangle has a time or none, by swept separating axes: none if the path of the centre misses the
 * triangle's own box grown on scene axis k by the box's reach along it, |u0[k]| * half[0] + |u1[k]| * half[1] + |u2[k]| * half[2];
 * otherwise the triangle is measured from the centre at the entry into that grown box and taken into the box's frame (three
 * dots per vertex), where the box is axis-aligned, and thirteen axes -- the box's three, the triangle's normal and the nine
 * cross products of an edge and a box axis -- each give an interval of times at which they do not separate the two; the time
 * is the start of the intersection of all of them, none if it is empty, never earlier than the entry into the grown box, and
 * none if it exceeds max_t. The answer is the smallest time, THE LOWEST PRIMITIVE ID AMONG EQUAL TIMES, or a miss. Leaf sizes,
 * loose boxes and the node format only decide how many triangles are never looked at. With the unit vectors as axes the
 * answers are rtk_dev_sweep_boxes' UP TO ROUNDING, NOT BIT FOR BIT.
 *   hit    t, u (weight of vertex 0), v (weight of vertex 1) and the global primitive id: a rtk_hit_record, which
 *          rtk_dev_select_rays and rtk_dev_expand_hits take as it is. u and v are those of the point of the triangle nearest to
 *          the centre c(t) (one rtk_closest_rule.h evaluation): A WITNESS ON THE TRIANGLE, NOT NECESSARILY A POINT OF CONTACT.
 *          d_centres[3 i ..] = c(t) as the rule computed it; d_normals[3 i ..] = the unit separating axis that gave the time, in
 *          scene coordinates, turned against the motion (dot(normal, direction) < 0): the contact normal a controller slides
 *          along. It is all zeros where the box already overlaps at the start (t == min_t), or where the axis has no length in
 *          float; it is never a NaN for a live query and a finite scene.
 *   miss   t = max_t as given, u = v = 0, prim = RTK_PRIM_NONE; d_centres[3 i ..] = the origin as given, d_normals[3 i ..] = 0
 * A query is live iff all twenty floats are finite (RTK_INF is a finite number: "no limit"), the direction is not all zeros,
 * every half[j] >= 0, min_t <= max_t and THE AXES ARE ORTHONORMAL TO WITHIN 2^-10: |dot(uj, uj) - 1| <= 2^-10 for each axis and
 * |dot(ui, uj)| <= 2^-10 for each pair, in float. That gate keeps garbage out and is no accuracy claim: rows rounded from a
 * float64 rotation or made from a float32 unit quaternion pass with room to spare; scaled, sheared or zero axes do not. Within
 * the gate the axes are used as given. A query that is not live is a miss, and so is every query of a scene without triangles.
 * half == 0 on one, two or all three axes is legal: a rectangle, a segment and a point are boxes; on a point the rule is NOT
 * rtk's watertight ray test, and its results are not bit-equal to a trace's.
 * THE FILTER is part of the rule: of a rtk_dev_filter, d_mesh_mask (with mesh_mask_bits) and d_ignore_prim (read per query slot)
 * say which triangles are candidates, as for the filtered traces; a non-NULL d_after is refused. `filter` may be NULL.
 * rtk_dev_sweep_obbs_any answers "is the path blocked": d_blocked[i] = 1 if query i has a candidate with a time, else 0 --
 * exactly prim != RTK_PRIM_NONE of rtk_dev_sweep_obbs; its walk ends at the first one it meets.
 * `list` may be NULL: all num_sweeps queries are answered. Otherwise the words of the listed traces hold: m = min(*d_count,
 * num_sweeps) entries are answered, the result of query r goes to slot r of the outputs, d_ignore_prim is read at slot r, A SLOT
 * THAT IS NOT LISTED IS NOT WRITTEN, an id may repeat, and the count is read when the work reaches it on `stream`. d_centres and
 * d_normals may each be NULL.
 * Asynchronous on `stream`: no host wait, nothing read back. The scene is only read, so the thread-safety rules of the batches
 * hold; the part of the walk's stack that does not fit on chip lives in the per-(scene, stream) scratch set, and a dropped push
 * (impossible for a tree) is reported by rtk_dev_trace_status like a trace's. Nothing it allocates counts toward the scene.
 * Refused before anything is launched, RTK_AMD_ERR_BAD_ARG: a NULL scene; NULL d_sweeps or a NULL d_records / d_blocked with
 * num_sweeps != 0; a bad list (as for the listed traces); a filter whose struct_size is too small, whose d_after is set or whose
 * mesh mask has no bits; num_sweeps >= 2^32; a calling thread whose current device is not the scene's. num_sweeps == 0 is
 * RTK_AMD_OK with nothing launched. Works as it is on rtk_mgpu_scene(m, i).
 * A scene with non-finite vertex coordinates: the call terminates and writes only inside its outputs; NOTHING ELSE IS PROMISED
 * about its results. */
typedef struct rtk_obb_sweep { float origin[3], direction[3], min_t, max_t, half[3], axes[9]; } rtk_obb_sweep;   /* 80 bytes; a float32 [n, 20] tensor */
int rtk_dev_sweep_obbs(const rtk_dev_scene *ds, const rtk_obb_sweep *d_sweeps, size_t num_sweeps, const rtk_ray_list *list,
	rtk_hit_record *d_records, float *d_centres /* may be NULL */, float *d_normals /* may be NULL */,
	const rtk_dev_filter *filter /* may be NULL */, void *stream);
int rtk_dev_sweep_obbs_any(const rtk_dev_scene *ds, const rtk_obb_sweep *d_sweeps, size_t num_sweeps, const rtk_ray_list *list,
	uint8_t *d_blocked, const rtk_dev_filter *filter, void *stream);
/* Same result as rtk_dev_sweep_obbs without a list, plus visit counts in the fields of rtk_dev_closest_points_counted (rays =
 * queries answered; triangles = records fetched, of which those the filter rules out are not evaluated; hits = queries that
 * found a triangle). Null stream, synchronous; not for timing. */
int rtk_dev_sweep_obbs_counted(const rtk_dev_scene *ds, const rtk_obb_sweep *d_sweeps, size_t num_sweeps,
	rtk_hit_record *d_records, float *d_centres, float *d_normals, const rtk_dev_filter *filter, rtk_trace_counters *out);
/* (entries per lane the walk keeps on chip before it uses the spill area, for tests) */
uint32_t rtk_amd_obbsweep_stack_entries(void);

/* ---- Every hit along a ray: how many triangles a ray crosses, and all of them (or the k closest) in one walk ----
 * What transparency and alpha compositing, thickness and x-ray depth, visibility through several occluders and point-in-mesh by
 * crossing parity ask. Until now the only route was the d_after loop of rtk_dev_trace_rays_filtered: one complete closest-hit
 * walk per candidate per ray and a read-back per round.
 *
 * THE RULE. A CANDIDATE of a ray is a triangle that
 *   - lies in a leaf that the walk enters,
 *   - rtk's watertight test accepts: !(neg && pos) && t > min_t && t < max_t, with rtk's operation order and rtk's group-of-four
 *     double-precision rule (rtk.c:302-336): a partial last group of a leaf is always evaluated in double; a full group is
 *     scanned for an exactly-zero edge function first and then evaluated, in double if it has one (what is counted or written
 *     is never undone),
 *   - and every filter that is set lets through: d_mesh_mask, d_ignore_prim and d_after mean exactly what they mean in
 *     rtk_dev_trace_rays_filtered (d_after makes paging possible: the candidates after a given (t, prim)).
 * The walk ENTERS a child if its slot is not empty and the slab test of the exact 128-byte node passes WITH THE FAR BOUND FIXED
 * AT THE RAY'S max_t: (plane - origin) * (1 / direction) per axis, near and far plane picked by the direction's sign bit,
 * max(near.., min_t) <= min(far.., max_t), the arithmetic of the closest-hit kernels' exact-node branch (for a ray whose
 * products can be NaN, with the reference's SSE operand order of min and max). The candidate set is therefore a FUNCTION OF THE
 * SCENE'S BITS AND THE RAY: it does not depend on the order of the walk, and it is exactly what a rtk_filter_fn that rejects
 * everything is offered, once each, by the reference's traversal (the oracle's ora_trace_rays_filter) on the exported blob.
 * ONLY THE EXACT NODES are used, never the 64-byte compressed ones: those admit a superset of boxes, and the set would depend
 * on the node format. RTK_TRACE_EXACT_NODES is implied.
 *
 * rtk_dev_trace_rays_count: d_counts[i] = the number of candidates of ray i, written for EVERY ray (0 for a ray without any);
 *   nothing else is written.
 * rtk_dev_trace_rays_all: ray i owns d_records[d_offsets[i] .. d_offsets[i + 1]); d_offsets has n + 1 entries, non-decreasing;
 *   r = d_offsets[i + 1] - d_offsets[i] is its room and may be 0. Written are the min(count_i, r) CLOSEST candidates in ascending
 *   (t, prim) order, each the rtk_hit_record the closest-hit call would write for that triangle (t, u * rcp, v * rcp, global
 *   prim); d_written[i] (d_written may be NULL) is that number. Entries of the segment beyond it ARE NOT WRITTEN, entries
 *   outside every segment are not written. The far bound of the walk stays at max_t also when a segment is full (a shrunk
 *   bound would let the rounding of a box's entry distance against a triangle's t decide which of two near-equal candidates is
 *   kept): the kept records are EXACTLY the first min(count_i, r) of the ray's full list. So one call serves two uses:
 *     every hit      count, an inclusive prefix sum into uint64 offsets on the same stream (torch.cumsum into an int64 tensor is
 *                    one as it stands, like rtk_ray_list.d_ids), then fill;
 *     the k closest  d_offsets[i] = i * k, no count pass.
 * DETERMINISTIC: the same inputs give the same bytes.
 * Both calls are asynchronous on `stream`, need no host wait and read nothing back. The scene is only read, as it stands: built,
 * uploaded, refitted, split or rebuilt, and rtk_mgpu_scene(m, i) as it is. They use the per-(scene, stream) scratch set like
 * every other launch (queue heads; the part of the walk's stack that does not fit on chip), so the thread-safety rules of the
 * batches hold unchanged; a dropped push (impossible for a tree) is reported by rtk_dev_trace_status.
 * `opts` may be NULL; blocks_per_cu, refill_min and node_exit apply; image hints, RTK_TRACE_SORT_RAYS and every other flag are
 * IGNORED: there is no packet form. `filter` may be NULL.
 * Refused before anything is launched and before any HIP call, RTK_AMD_ERR_BAD_ARG: a NULL scene; NULL d_rays or d_counts, NULL
 * d_offsets or d_records with n != 0; a filter whose struct_size is too small (or a mesh mask without mesh_mask_bits);
 * n >= 2^32. The scene and device refusals are those of rtk_dev_trace_rays. n == 0 is RTK_AMD_OK with nothing launched.
 * Offsets that run past the caller's buffer are the caller's error and, like a listed trace's ids, are NOT CHECKED (records
 * are written out of range); a ray whose offsets decrease has no room and nothing is written for it. */
int rtk_dev_trace_rays_count(const rtk_dev_scene *ds, const rtk_ray *d_rays, size_t n,
	uint32_t *d_counts, const rtk_dev_filter *filter, const rtk_trace_opts *opts, void *stream);
int rtk_dev_trace_rays_all(const rtk_dev_scene *ds, const rtk_ray *d_rays, size_t n,
	const uint64_t *d_offsets, rtk_hit_record *d_records, uint32_t *d_written /* may be NULL */,
	const rtk_dev_filter *filter, const rtk_trace_opts *opts, void *stream);
/* (4-byte stack entries per lane the walk keeps on chip before it uses the spill area, for tests) */
uint32_t rtk_amd_allhits_stack_entries(void);

/* ---- Instanced worlds: rays through placed copies of device scenes ----
 * Every other call takes ONE rtk_dev_scene: one tree over one flat set of triangles; rtk_dev_scene_build_placed flattens its
 * placed meshes into such a set, so memory and build time grow with instances x triangles and moving one body refits that
 * body's triangles. A rtk_dev_world is the second level: a small TOP TREE over the world boxes of INSTANCES, each a
 * (scene, rtk_placement) pair; a scene is held once however often it is placed, and moving an instance costs a 64-byte
 * record and a refit of the top tree. A world answers rays (closest hit and any hit), closest points
 * (rtk_dev_world_closest_points, below) and the three overlap queries (rtk_dev_world_triangles_in_box_* / _in_obb_* /
 * _touching_*, below); signed distance, winding, within, pairs and sweeps still take one rtk_dev_scene.
 *
 * THE OBJECT. rtk_dev_world_create(scenes, num_scenes, instance_scene, placements, num_instances): instance i places scene
 * scenes[instance_scene[i]] by placements[i] (host memory, both arrays; the rule of rtk_dev_scene_build_placed maps the
 * scene's coordinates to the world's). Synchronous. NULL on failure.
 *   - THE WORLD BORROWS ITS SCENES and does not own them: FREEING A SCENE THAT A LIVE WORLD NAMES IS THE CALLER'S ERROR.
 *     The world keeps a small device table per scene (nodes, triangle records, their counts) and the scene's stack_entries,
 *     copied at create and at every rtk_dev_world_update. A SCENE THAT WAS REFITTED, SPLIT OR REBUILT MUST BE FOLLOWED BY
 *     rtk_dev_world_update BEFORE THE NEXT TRACE of the world (placements == NULL re-reads the scenes and keeps the placements).
 *   - Per instance the world holds one 64-byte record (the inverse placement, the scene number, flags), the placement and one
 *     proxy triangle whose box is the instance's padded world box. The top tree is an ordinary rtk_dev_scene over the proxies,
 *     which the world owns: rtk_dev_world_top_scene lends it for rtk_dev_scene_get_info, _validate and _quality, nothing else.
 *   - A DEAD instance is never hit: its placement is not invertible in float (determinant 0 or not finite, an inverse that
 *     overflows), its scene has no triangles, or its world box is not finite. It keeps its number and a point box.
 *   - rtk_dev_world_update(w, placements, stream): new placements for the same instances (host or device memory,
 *     num_instances entries; NULL: keep them), the scenes' tables read again, the top tree refitted. Synchronous, like
 *     rtk_dev_scene_refit, and like it WRITES the world: no trace of the world may be in flight. rtk_dev_world_rebuild builds
 *     the top tree again from the current boxes (rtk_dev_scene_rebuild) when instances have moved far; answers do not change.
 *   - rtk_dev_world_info: dead_instances as of the last create or update; total_device_bytes is the world's own memory (the
 *     top tree's ledger, the instance records, placements and proxies, the scene table, one counter), not the scenes';
 *     stack_entries = the top tree's + 1 + the deepest scene's.
 *
 * THE RULES (rtk_amd/csrc/rtk_world_rule.h, for the host and the device). The inverse placement is made in double in a stated
 * order and rounded to float once. An instance's scene is walked with the ray (inv * origin + translation, inv * direction),
 * every product and sum rounded to float on its own; min_t and max_t are copied and THE DIRECTION IS NOT RENORMALISED: an affine
 * map keeps the ray parameter, so t is comparable across instances and is the world ray's t.
 *
 * THE ANSWER. rtk_dev_world_trace_rays: per ray the rtk_hit_record of the closest candidate over all live instances the filter
 * lets through, prim the GLOBAL PRIMITIVE ID IN THE INSTANCE'S SCENE, and (d_instances may be NULL) the instance number;
 * a miss is t = max_t, u = v = 0, RTK_PRIM_NONE in both. A candidate of an instance has bit for bit the t, u, v, prim that
 * rtk_dev_trace_rays gives for the transformed ray on that instance's scene (exact nodes, rtk's leaf rule; inside one
 * instance the lowest primitive id wins among bit-equal t). TIES: t is the minimum over all instances; WHEN SEVERAL
 * INSTANCES ATTAIN BIT-EQUAL t THE RECORD IS THAT OF ONE OF THEM, which one is not promised.
 * rtk_dev_world_trace_rays_any: one byte per ray, 1 if some instance has a candidate. _counted: the closest form with visit
 * counts (nodes and leaves of the top tree and of the scenes together, triangles = proxies and triangle records); synchronises.
 * `list` as for the listed traces (a slot that is not listed is not written; an id >= n is skipped). rtk_world_filter:
 * d_instance_mask (bit i set = instance i is walked; instances at and beyond instance_mask_bits are not) and d_ignore_instance
 * (per ray slot, an instance that ray never enters: the instance a bounce starts on); both device memory, both optional.
 * Asynchronous on `stream`, nothing is read back; the scratch set and the launch-error word are the top tree's for that stream
 * (rtk_dev_world_trace_status waits and reports it). The top tree never culls an instance the walk of its scene would hit
 * as long as every placement's 3 x 3 part has a condition number of at most 100 (DESIGN.md 3.23 derives the padding of the
 * boxes and the margin of the top tree's slab test); beyond that nothing is promised but no fault and no access out of range.
 *
 * Refused before any HIP call (create: NULL; else RTK_AMD_ERR_BAD_ARG): NULL arguments, a struct_size that is too small,
 * flags != 0, num_instances == 0 or >= 2^31, instance_scene[i] >= num_scenes, scenes on different devices, a mask without
 * bits, n >= 2^32, a bad list; then a device other than the calling thread's current one, as for every launch. */
typedef struct rtk_dev_world rtk_dev_world;
typedef struct rtk_dev_world_info {
	uint64_t num_scenes, num_instances, dead_instances;   /* dead: placement not invertible, or its scene has no triangles */
	uint64_t top_nodes, total_device_bytes;               /* the world's own memory, not the scenes' */
	uint32_t top_max_depth, stack_entries;                /* entries a ray can need: top + 1 + the deepest scene's */
	double build_ms, update_ms;
} rtk_dev_world_info;
rtk_dev_world *rtk_dev_world_create(rtk_dev_scene *const *scenes, size_t num_scenes,
	const uint32_t *instance_scene, const rtk_placement *placements, size_t num_instances);
int rtk_dev_world_update(rtk_dev_world *w, const rtk_placement *placements, void *stream);  /* host or device pointer; NULL: keep the placements, re-read the scenes */
int rtk_dev_world_rebuild(rtk_dev_world *w, void *stream);   /* the top tree built again from the current boxes */
int rtk_dev_world_get_info(const rtk_dev_world *w, rtk_dev_world_info *out);
void rtk_dev_world_free(rtk_dev_world *w);
const rtk_dev_scene *rtk_dev_world_top_scene(const rtk_dev_world *w);   /* borrowed; replaced by an update of a one-instance world */
int rtk_dev_world_trace_status(const rtk_dev_world *w, void *stream);   /* rtk_dev_trace_status of the top tree */
typedef struct rtk_world_filter { uint32_t struct_size, flags; const uint32_t *d_instance_mask; uint32_t instance_mask_bits;
                                  const uint32_t *d_ignore_instance; /* per ray slot */ } rtk_world_filter;
int rtk_dev_world_trace_rays(const rtk_dev_world *w, const rtk_ray *d_rays, size_t n, const rtk_ray_list *list,
	const rtk_world_filter *filter, rtk_hit_record *d_records, uint32_t *d_instances, void *stream);
int rtk_dev_world_trace_rays_any(const rtk_dev_world *w, const rtk_ray *d_rays, size_t n, const rtk_ray_list *list,
	const rtk_world_filter *filter, uint8_t *d_blocked, void *stream);
int rtk_dev_world_trace_rays_counted(const rtk_dev_world *w, const rtk_ray *d_rays, size_t n, const rtk_world_filter *filter,
	rtk_hit_record *d_records, uint32_t *d_instances, rtk_trace_counters *out);
/* (8-byte stack entries per lane the walk keeps on chip before it uses the spill area, for tests) */
uint32_t rtk_amd_world_stack_entries(void);

/* CLOSEST POINTS ON A WORLD. rtk_dev_world_closest_points: per query the rtk_closest_record of the nearest triangle over all
 * live instances the filter lets through, prim the GLOBAL PRIMITIVE ID IN THE INSTANCE'S SCENE as for rtk_dev_world_trace_rays,
 * (d_instances may be NULL) the instance number and (d_points may be NULL, 3 floats per query) the point on the triangle in
 * world coordinates. The rule (rtk_amd/csrc/rtk_world_closest_rule.h): a record's vertices are placed by the instance's
 * FORWARD placement with the rule of rtk_dev_scene_build_placed, then rtk_dev_closest_points's rule answers on the placed
 * vertices. THE RESULT HAS THE BITS rtk_dev_closest_points GIVES ON THE FLAT PLACED TWIN (rtk_dev_scene_build_placed of the same
 * meshes under the same placements), for any affine placement with finite placed vertices: no condition number, no margin.
 * Among candidates with dist2 < max_dist2 the smallest dist2 wins; among equal dist2 THE LOWEST INSTANCE NUMBER, then the
 * lowest primitive id: unlike the world's rays, a tie across instances is decided, and the result depends on neither tree
 * nor on the order of the walk. A dead instance is never answered. Liveness of a query and the miss record are
 * rtk_dev_closest_points's: a non-finite coordinate or a max_dist2 that is NaN, zero or negative is a miss; RTK_INF means no
 * limit; a miss is dist2 = max_dist2 as given, u = v = 0, RTK_PRIM_NONE in prim and in the instance, the point the query's.
 * With placed vertices that are not finite nothing is promised about results; the call terminates and writes only its outputs.
 * The record is a rtk_closest_record: rtk_dev_select_rays and rtk_dev_expand_hits (on the instance's scene) take it.
 * `list` as for the listed traces (a slot that is not listed is not written; an id >= n is skipped; an id may repeat).
 * rtk_world_filter as for rays; d_ignore_instance is read at the query's slot (the body a point belongs to).
 * Asynchronous on `stream`, nothing is read back; the scratch set and the launch-error word are the top tree's for that stream
 * (rtk_dev_world_trace_status). A scene that changed must be followed by rtk_dev_world_update first, as for rays.
 * _counted: with visit counts (nodes and leaves of both levels together, triangles = proxies and triangle records, hits,
 * stack_spills); on the null stream, synchronises. Refusals before any HIP call are those of rtk_dev_world_trace_rays;
 * num_queries == 0 is RTK_AMD_OK with nothing launched. */
int rtk_dev_world_closest_points(const rtk_dev_world *w, const rtk_point_query *d_queries, size_t num_queries,
	const rtk_ray_list *list, const rtk_world_filter *filter,
	rtk_closest_record *d_records, uint32_t *d_instances /* may be NULL */, float *d_points /* may be NULL */, void *stream);
int rtk_dev_world_closest_points_counted(const rtk_dev_world *w, const rtk_point_query *d_queries, size_t num_queries,
	const rtk_world_filter *filter, rtk_closest_record *d_records, uint32_t *d_instances, float *d_points, rtk_trace_counters *out);
/* (8-byte stack entries per lane the walk keeps on chip before it uses the spill area, for tests) */
uint32_t rtk_amd_world_closest_stack_entries(void);

/* OVERLAPS ON A WORLD: which triangles of which instances touch this box, this oriented box, this triangle -- the broad and
 * narrow phase of collision without flattening the world. rtk_dev_world_triangles_in_box_*, _in_obb_* and _touching_* are
 * rtk_dev_triangles_in_box_*, _in_obb_* and _touching_* asked of a world, with the world's filter in place of the scene's.
 * The rule (rtk_amd/csrc/rtk_world_overlap_rule.h): a record's vertices are placed by the instance's FORWARD placement with the
 * rule of rtk_dev_scene_build_placed, then the shape's own candidate rule (rtk_box_rule.h, rtk_obb_rule.h, rtk_touch_rule.h)
 * answers on the placed vertices, unchanged. THE CANDIDATES ARE THOSE THE SCENE CALL GIVES ON THE FLAT PLACED TWIN
 * (rtk_dev_scene_build_placed of the same meshes under the same placements), for any affine placement with finite placed
 * vertices: no condition number, no margin -- a scene's node box is placed exactly and all three skips are comparisons
 * (DESIGN.md 3.23.2). A query's liveness is the shape's own; a dead instance is never answered. The result depends on
 * neither tree nor on the order of the walk.
 * AN ENTRY is one uint64_t: ((uint64_t)instance << 32) | prim, prim the GLOBAL PRIMITIVE ID IN THE INSTANCE'S SCENE as for
 * rtk_dev_world_trace_rays. A query's list is its candidates in ASCENDING ENTRY, that is by instance, then by primitive id;
 * a torch int64 tensor is an entry buffer as it stands (instance = e >> 32, prim = e & 0xffffffff).
 * _count: d_counts[i] = the number of candidates of query i over all live instances the filter lets through, written for
 * EVERY answered query (0 for a query that is not live). _all: query i owns d_entries[d_offsets[i] .. d_offsets[i + 1]);
 * d_offsets has num_queries + 1 entries and is indexed by query slot; the segment receives the first
 * min(count, d_offsets[i + 1] - d_offsets[i]) entries of the list, d_written[i] (d_written may be NULL) that number; ENTRIES
 * BEYOND IT AND OUTSIDE EVERY SEGMENT ARE NOT WRITTEN. Offsets that decrease mean no room: nothing is written into such a
 * segment and d_written[i] = 0. d_offsets[i] = i * k with no count pass gives the k lowest entries of every query. `list` as
 * for the scene calls: A SLOT THAT IS NOT LISTED IS NOT WRITTEN, an id >= num_queries is skipped, an id that repeats is
 * answered once. rtk_world_filter as for rays and closest points; d_ignore_instance is read at the query's slot (the body a
 * query shape belongs to: there is no d_first_prim on a world). touch_flags: RTK_TOUCH_SKIP_SHARED_VERTEX or 0 -- a record
 * whose PLACED vertices share a position with the query's is left out, which is what the flat twin compares; any other bit is
 * refused.
 * Asynchronous on `stream`, nothing is read back; the scratch set and the launch-error word are the top tree's for that stream
 * (rtk_dev_world_trace_status). A scene that changed must be followed by rtk_dev_world_update first, as for rays.
 * _counted: the count form (d_offsets == NULL) or the fill form with visit counts (nodes and leaves of both levels together,
 * triangles = proxies and triangle records, hits = queries with a candidate, stack_spills); on the null stream, synchronises.
 * Refusals before any HIP call (RTK_AMD_ERR_BAD_ARG, the function's name in the text) are those of rtk_dev_world_trace_rays --
 * a NULL world, NULL queries or outputs with num_queries != 0, a bad list, a bad filter, num_queries >= 2^32 -- and an unknown
 * bit of touch_flags; num_queries == 0 is RTK_AMD_OK with nothing launched. */
int rtk_dev_world_triangles_in_box_count(const rtk_dev_world *w, const rtk_box_query *d_boxes, size_t num_queries,
	const rtk_ray_list *list, const rtk_world_filter *filter, uint32_t *d_counts, void *stream);
int rtk_dev_world_triangles_in_box_all(const rtk_dev_world *w, const rtk_box_query *d_boxes, size_t num_queries,
	const rtk_ray_list *list, const rtk_world_filter *filter, const uint64_t *d_offsets, uint64_t *d_entries, uint32_t *d_written /* may be NULL */, void *stream);
int rtk_dev_world_triangles_in_box_counted(const rtk_dev_world *w, const rtk_box_query *d_boxes, size_t num_queries,
	const rtk_world_filter *filter, const uint64_t *d_offsets, uint64_t *d_entries, uint32_t *d_counts_or_written, rtk_trace_counters *out);
int rtk_dev_world_triangles_in_obb_count(const rtk_dev_world *w, const rtk_obb_query *d_obbs, size_t num_queries,
	const rtk_ray_list *list, const rtk_world_filter *filter, uint32_t *d_counts, void *stream);
int rtk_dev_world_triangles_in_obb_all(const rtk_dev_world *w, const rtk_obb_query *d_obbs, size_t num_queries,
	const rtk_ray_list *list, const rtk_world_filter *filter, const uint64_t *d_offsets, uint64_t *d_entries, uint32_t *d_written /* may be NULL */, void *stream);
int rtk_dev_world_triangles_in_obb_counted(const rtk_dev_world *w, const rtk_obb_query *d_obbs, size_t num_queries,
	const rtk_world_filter *filter, const uint64_t *d_offsets, uint64_t *d_entries, uint32_t *d_counts_or_written, rtk_trace_counters *out);
int rtk_dev_world_triangles_touching_count(const rtk_dev_world *w, const rtk_tri_query *d_tris, size_t num_queries,
	const rtk_ray_list *list, const rtk_world_filter *filter, uint32_t touch_flags, uint32_t *d_counts, void *stream);
int rtk_dev_world_triangles_touching_all(const rtk_dev_world *w, const rtk_tri_query *d_tris, size_t num_queries,
	const rtk_ray_list *list, const rtk_world_filter *filter, uint32_t touch_flags, const uint64_t *d_offsets, uint64_t *d_entries,
	uint32_t *d_written /* may be NULL */, void *stream);
int rtk_dev_world_triangles_touching_counted(const rtk_dev_world *w, const rtk_tri_query *d_tris, size_t num_queries,
	const rtk_world_filter *filter, uint32_t touch_flags, const uint64_t *d_offsets, uint64_t *d_entries, uint32_t *d_counts_or_written,
	rtk_trace_counters *out);
/* (8-byte stack entries per lane the walk keeps on chip before it uses the spill area, for tests) */
uint32_t rtk_amd_world_overlap_stack_entries(void);

/* Waits for `stream` and reports whether a launch of this scene on it overflowed a traversal stack
 * (RTK_AMD_ERR_BAD_SCENE; impossible for a validated tree -- the push is dropped, never written out of bounds). */
int rtk_dev_trace_status(const rtk_dev_scene *ds, void *stream);

/* Is the device-resident batch a row-major image (a regular step from ray to ray -- origin and direction -- that jumps at the same
 * distance every time)? *width, *height = its shape, or 0, 0. What rtk_dev_trace_rays does by itself for a closest-hit batch that
 * comes without the image hint (two small launches and a wait for `stream`, ~20 us): a host that traces many frames of one
 * shape asks once and passes the shape in rtk_trace_opts afterwards. A wrong answer can only cost speed, never a hit. */
int rtk_dev_detect_image(const rtk_dev_scene *ds, const rtk_ray *d_rays, size_t n, uint32_t *width, uint32_t *height, void *stream);

/* Same result as rtk_dev_trace_rays, plus visit counts. Synchronous; not for timing. */
int rtk_dev_trace_rays_counted(const rtk_dev_scene *ds, const rtk_ray *d_rays, size_t n,
	rtk_hit_record *d_hits, const rtk_trace_opts *opts, rtk_trace_counters *out);

int rtk_dev_trace_rays_any_counted(const rtk_dev_scene *ds, const rtk_ray *d_rays, size_t n,
	uint8_t *d_occluded, const rtk_trace_opts *opts, rtk_trace_counters *out);

/* Step counts of the hand-written packet kernel ITSELF: the launch runs rtk_packet_count2, which is rtk_packet_beam2.S assembled
 * with three scalar counters per pair of tiles ("visit counts come from a counting build of the same kernel"), and
 * the counting build of the C++ packet kernel on the tiles it hands back. Same records as rtk_dev_trace_rays. Synchronous; not
 * for timing. RTK_AMD_ERR_UNSUPPORTED if the batch would not run on rtk_packet_beam2 (no image hint, big leaves, ...). */
typedef struct rtk_packet_counters {
	uint64_t tiles;                      /* 8x8-pixel tiles of the batch (n / 64) */
	uint64_t pairs;                      /* pairs of tiles walked by a wave (handed-back pairs included, with the steps they took until then) */
	uint64_t node_steps;                 /* 128 B nodes fetched: one per node step of a PAIR */
	uint64_t triangles_fetched;          /* 48 B triangle records fetched: one per triangle of a leaf a pair enters */
	uint64_t triangle_group_tests;       /* triangle tests: one per (triangle, group of 64 rays whose beam reaches the leaf) */
	uint64_t tiles_handed_back;          /* tiles traced again from the start by the C++ packet kernel */
	uint64_t handed_back_node_steps;     /* ... its wave-level node steps (one tile per wave) */
	uint64_t handed_back_triangle_steps; /* ... and triangle steps */
} rtk_packet_counters;
int rtk_dev_trace_rays_packet_counted(const rtk_dev_scene *ds, const rtk_ray *d_rays, size_t n,
	rtk_hit_record *d_hits, const rtk_trace_opts *opts, rtk_packet_counters *out);

/* For tests and tools: the entry-list pre-pass of an image frame alone (what rtk_dev_trace_rays runs ahead of the packet kernel
 * when the image hint is given). image_w and image_h are multiples of 64; d_rays holds image_w * image_h rays, row-major;
 * target and max_levels are the two list knobs (the library's defaults: 26 and 8). host_out receives (image_w / 64) *
 * (image_h / 64) records of 512 bytes, one per 64x64-pixel block, row by row: float olo[3], ohi[3], rlo[3], rhi[3] (the
 * block's beam), uint32 count at byte 48, float min_t at 52, and from byte 64 count pairs { uint32 node, float lower bound of
 * the entry distance }, ascending. count = 0: the block's tiles start at the root. Runs on the NULL stream; synchronous. */
int rtk_dev_debug_packet_entries(const rtk_dev_scene *ds, const rtk_ray *d_rays, uint32_t image_w, uint32_t image_h,
	uint32_t target, uint32_t max_levels, void *host_out);

/* -- several GPUs of one node, one process --
 * Rays shard, nothing else: the scene is replicated (the deterministic build or the upload runs on every GPU),
 * shard r of R owns the contiguous range rtk_amd_shard_range(n, r, R) of the batch, and the only exchange is the
 * gather of the 16-byte records, each GPU copying straight to the final place on its own stream (its own xGMI
 * link into the root), piece by piece while the rest of its shard is still being traced. Synchronous calls. */
typedef struct rtk_mgpu rtk_mgpu;
void rtk_amd_shard_range(size_t n, int rank, int num_shards, size_t *first, size_t *count);
rtk_mgpu *rtk_mgpu_create(const int *devices, int num_devices);   /* NULL / 0: all devices; an id may repeat (virtual shards) */
void rtk_mgpu_destroy(rtk_mgpu *m);
int rtk_mgpu_num_devices(const rtk_mgpu *m);
const rtk_dev_scene *rtk_mgpu_scene(const rtk_mgpu *m, int index);
int rtk_mgpu_build(rtk_mgpu *m, const rtk_scene_desc *desc);      /* rtk_dev_scene_build on every GPU */
int rtk_mgpu_upload(rtk_mgpu *m, const rtk_scene *scene);         /* rtk_dev_scene_upload on every GPU */
int rtk_mgpu_refit(rtk_mgpu *m, const rtk_scene_desc *desc);      /* rtk_dev_scene_refit on every GPU of the context (handles stay valid) */
int rtk_mgpu_refit_meshes(rtk_mgpu *m, const rtk_scene_desc *desc, const uint32_t *mesh_ids, size_t num_ids);   /* rtk_dev_scene_refit_meshes on every GPU */
/* the placed forms (rtk_placement above) on every GPU: the same placements for every replica, which agree afterwards */
int rtk_mgpu_build_placed(rtk_mgpu *m, const rtk_scene_desc *desc, const rtk_placement *placements);
int rtk_mgpu_refit_placed(rtk_mgpu *m, const rtk_scene_desc *desc, const rtk_placement *placements);
int rtk_mgpu_refit_meshes_placed(rtk_mgpu *m, const rtk_scene_desc *desc, const rtk_placement *placements,
                                 const uint32_t *mesh_ids, size_t num_ids);
int rtk_mgpu_split_leaves(rtk_mgpu *m, uint32_t max_leaf);        /* rtk_dev_scene_split_leaves on every GPU of the context (handles stay valid) */
int rtk_mgpu_rebuild(rtk_mgpu *m);   /* on every GPU of the context; rtk_mgpu_scene handles stay valid */
/* host rays in, host records out (records[i] belongs to rays[i]) */
int rtk_mgpu_trace_rays(rtk_mgpu *m, const rtk_ray *rays, size_t n, rtk_hit_record *records, const rtk_trace_opts *opts);
/* device-resident shards: d_rays[r] / d_records[r] (counts[r] elements) live on GPU r of the context; if d_gathered
 * is not NULL it is memory of GPU `root_index` that receives all records, shard after shard. opts applies per shard
 * (an image-shaped shard is traced in bands of whole tile rows by the packet kernel). */
int rtk_mgpu_trace_rays_device(rtk_mgpu *m, const rtk_ray *const *d_rays, const size_t *counts, rtk_hit_record *const *d_records,
	rtk_hit_record *d_gathered, int root_index, const rtk_trace_opts *opts);
/* The same with a STRIPED exchange instead of a gather onto one root (which is bound by that root's links: eight GPUs
 * gathered onto one deliver ~2x one GPU): GPU j ends up with stripe j of EVERY shard in d_striped[j] (memory of GPU j),
 * segments in shard order; stripe j of a shard of c records is rtk_amd_shard_range(c, j, R) of it, and
 * rtk_mgpu_striped_segment(counts, R, shard, stripe, &first, &count) says where it sits in d_striped[stripe]. Every GPU
 * sends 1/R of each piece over each of its links while the rest of its shard is still being traced. */
int rtk_mgpu_trace_rays_device_striped(rtk_mgpu *m, const rtk_ray *const *d_rays, const size_t *counts, rtk_hit_record *const *d_records,
	rtk_hit_record *const *d_striped, const rtk_trace_opts *opts);
void rtk_mgpu_striped_segment(const size_t *counts, int num_shards, int shard, int stripe, size_t *first, size_t *count);

/* -- host-pointer convenience (PCIe-inclusive, synchronous) --
 * Closest hits of n rays against a scene blob. hits[i] is written where the ray hit
 * (left untouched on a miss, like rtk_trace_ray); hit_mask[i] (optional) gets 0/1.
 * Returns the number of hits, or (size_t)-1 on error. The device copy of the blob is cached per (scene pointer,
 * current device) until rtk_free_scene / rtk_amd_forget_scene. Every way this library itself writes a blob to an
 * address (rtk_finish_build, rtk_finish_build_to with either builder) drops what was cached for that address. A
 * caller that overwrites a blob in place by its own means MUST call rtk_amd_forget_scene(address) before tracing it
 * again. As a safety net every lookup re-checks the header, the root node and one 4 KB stripe of the blob (a different
 * one each time, against hashes of all stripes taken at upload): another scene at the same address is noticed at
 * once, a small in-place edit within size / 4 KB lookups -- not immediately. A blob in caller-owned memory keeps its
 * device copy until rtk_amd_forget_scene is called for it. Each calling thread uses its own stream and staging
 * buffers. rtk_trace_ray / rtk_trace_ray_filter (no error channel, and `false` means "miss" to a host that knows only
 * rtk.h): a failure is never silent -- it prints one line on stderr (rate-limited after the first eight) and sets
 * rtk_amd_last_error(). A lone failure that may pass (out of memory, an interrupted launch) then returns false; one
 * that every later call would repeat (no usable GPU, a scene that does not validate), or a SECOND failure in a row on
 * the calling thread (a stream error that sticks), abort()s unless RTK_AMD_SOFT_ERRORS is set in the environment. */
size_t rtk_trace_rays(const rtk_scene *scene, const rtk_ray *rays, size_t n, rtk_hit *hits, uint8_t *hit_mask);
/* Batch form of rtk_trace_ray_filter (rtk.h:130) with a host callback: per ray the closest candidate that
 * `filter` accepts. Every candidate of a ray is offered, in increasing (t, primitive id) order (equal-t ones
 * included), until one is accepted. The batch runs in rounds: one launch collects the k closest candidates of
 * every undecided ray (k = 4 for 16 384 rays ... 64 for a single ray); rays whose k candidates were all rejected
 * continue after the last one in the next round. */
size_t rtk_trace_rays_filter(const rtk_scene *scene, const rtk_ray *rays, size_t n, rtk_hit *hits, uint8_t *hit_mask,
	rtk_filter_fn *filter, void *filter_user);
void rtk_amd_forget_scene(const rtk_scene *scene);

#ifdef __cplusplus
}
#endif
#endif /* RTK_AMD_H */
