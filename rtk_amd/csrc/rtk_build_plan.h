// rtk_build_plan.h -- what the host decides in a device build, between the kernels: the environment knobs, how every mesh
// reaches the ingest kernel and how many of the caller's bytes are copied for it, the sort words and their key width, tile mode,
// the first node capacity, the narrow-key verdict. Plain C++17, no HIP: the host compiler builds it alone
// (tests/test_build_plan_cpu.py does, under the address sanitizer). rtk_build.hip and the stage files carry the plans out.
#pragma once

#include "rtk.h"
#include "rtk_amd.h"
#include "rtk_build_layout.h"

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#pragma GCC visibility push(hidden)      // (nothing here is part of the library's interface, nor what the standard templates make of it)

// ---- knobs: every environment variable the build reads, read in one place at the top of a build ----

static inline float env_float(const char *name, float def)
{
	const char *s = getenv(name);
	return s && *s ? (float)atof(s) : def;
}

// "set it to 0 to turn it off": true unless the variable is there and reads as 0
static inline bool env_unless_zero(const char *name)
{
	const char *s = getenv(name);
	return !(s && atoi(s) == 0);
}

struct BuildKnobs {
	bool timing;             // RTK_AMD_BUILD_TIMING (set at all): the device time of every stage, with a device synchronisation after each
	bool host_time;          // RTK_AMD_BUILD_HOSTTIME=1: where the HOST is when (no synchronisation: how far ahead of the GPU the enqueueing thread runs)
	uint32_t max_leaf;       // RTK_AMD_MAX_LEAF, 1 .. 63
	bool sort_packed;        // RTK_AMD_SORT_PACKED=0: the >= 2^24-triangle path (key, index pairs), for tests on small scenes
	uint32_t key_bits;       // RTK_AMD_KEY_BITS: 8 .. 40 in steps of 8, the width of the Morton code in the packed sort words (0: from the number of triangles)
	bool direct;             // RTK_AMD_BUILD_DIRECT=0: every mesh is staged, none gathered in place by the emit. Read once per process.
	bool fused_emit;         // RTK_AMD_FUSED_EMIT=0: the triangle records are made by a pass of their own, not inside k_refit_tile (A/B)
	uint64_t tile_min;       // RTK_AMD_TILE_COLLAPSE_MIN: triangles from which the tile collapse is used (see below)
	uint32_t top_cap;        // RTK_AMD_TOP_CAP: at most so many nodes above the tiles, to drive the way back to the level-by-level collapse from tests
	int est_div;             // RTK_AMD_NODE_ESTIMATE_DIV: node arrays of n / div + 16 nodes at first, to drive the repeat path from tests (0: the usual estimate)
	bool keep_workspace;     // RTK_AMD_KEEP_WORKSPACE=0: the workspace is freed after every build
	bool key_rebuild;        // RTK_AMD_KEY_REBUILD=0: a scene whose narrow keys collide too often is not built again with wide ones
};

// RTK_AMD_MAX_LEAF, 1 .. 63, default 3 (rtk_build_max_leaf, rtk_dev.h)
static inline uint32_t build_max_leaf_from_env()
{
	uint32_t max_leaf = (uint32_t)env_float("RTK_AMD_MAX_LEAF", 3.0f);
	if (max_leaf < 1) max_leaf = 1;
	if (max_leaf > 63) max_leaf = 63;         // 6-bit count in the blob's leaf header (rtk.c:188)
	return max_leaf;
}

// the two constants of the surface area heuristic (rtk_sah_costs, rtk_dev.h)
static inline void build_sah_costs_from_env(float *cost_node, float *cost_tri)
{
	*cost_tri = env_float("RTK_AMD_SAH_CT", 1.0f);
	*cost_node = env_float("RTK_AMD_SAH_CN", 0.5f);     // sweeps on MI355X: small leaves win (profiles/r01_sweep_sah2.log)
}

static inline BuildKnobs read_build_knobs()
{
	BuildKnobs k;
	k.timing = getenv("RTK_AMD_BUILD_TIMING") != nullptr;
	k.host_time = getenv("RTK_AMD_BUILD_HOSTTIME") && atoi(getenv("RTK_AMD_BUILD_HOSTTIME")) != 0;
	// leaves of at most three triangles: a leaf of fewer than four is one partial group for the reference's group-of-four rule
	// (rtk.c:302-336: double-precision edge functions, no redo), which is all the hand-written packet kernel implements; with
	// cn = 0.5 the SAH rule made 1.008 triangles per leaf at a limit of 8, so nothing of substance changes
	k.max_leaf = build_max_leaf_from_env();
	k.sort_packed = env_unless_zero("RTK_AMD_SORT_PACKED");
	k.key_bits = 0;
	if (getenv("RTK_AMD_KEY_BITS")) { const int kb = atoi(getenv("RTK_AMD_KEY_BITS")); if (kb >= 8 && kb <= 40 && kb % 8 == 0) k.key_bits = (uint32_t)kb; }
	static const bool allow_direct = env_unless_zero("RTK_AMD_BUILD_DIRECT");
	k.direct = allow_direct;
	k.fused_emit = env_unless_zero("RTK_AMD_FUSED_EMIT");
	// Tile mode (the subtrees inside a refit tile collapsed by k_collapse_tile), measured on MI355X (profiles/r05_build_timing.log, level
	// by level / tile mode): 0.47 / 0.46 ms at 0.5M triangles, 0.555 / 0.540 at 1M, 0.785 / 0.748 at 2M, 1.005 / 0.935 at 3M -- since the
	// tiles' kernels run beside pass 2 and the top collapse, tile mode is never slower; its trees have ~2 % more nodes (tile roots are never
	// opened from above: ~1 % more node visits per ray), so it starts where the build time it saves is worth more than that: 1.5M
	// triangles. RTK_AMD_TILE_COLLAPSE_MIN (triangles; read per build) moves that: 0 = whenever there are two tiles, a huge value =
	// never (everything level by level: A/B).
	const char *tile_env = getenv("RTK_AMD_TILE_COLLAPSE_MIN");
	k.tile_min = tile_env ? (uint64_t)atoll(tile_env) : (3ull << 19);
	k.top_cap = getenv("RTK_AMD_TOP_CAP") ? (uint32_t)atoi(getenv("RTK_AMD_TOP_CAP")) : 0xffffffffu;
	k.est_div = getenv("RTK_AMD_NODE_ESTIMATE_DIV") ? atoi(getenv("RTK_AMD_NODE_ESTIMATE_DIV")) : 0;
	k.keep_workspace = env_unless_zero("RTK_AMD_KEEP_WORKSPACE");
	k.key_rebuild = env_unless_zero("RTK_AMD_KEY_REBUILD");
	return k;
}

// ---- the meshes: everything that can be wrong with the description is found here ----

// How one mesh reaches the ingest kernel.
struct MeshPlan {
	bool on_host_decode = false;    // callbacks: decoded on the host, copied as plain positions
	bool f64 = false;
	int idx_kind = 0;               // 0 implicit, 1 u16, 2 u32
	size_t pstride = 0, istride = 0;
	size_t pbytes = 0, ibytes = 0;  // bytes to upload (0: already device memory / nothing)
	const char *pos_src = nullptr, *idx_src = nullptr;
	bool pos_on_device = false, idx_on_device = false;
};

// total triangles in front of every mesh (num_meshes + 1 entries, the last one the scene's). False: 2^30 triangles or more.
static inline bool plan_mesh_base(const rtk_scene_desc *desc, std::vector<uint64_t> *mesh_base)
{
	mesh_base->assign(desc->num_meshes + 1, 0);
	for (size_t m = 0; m < desc->num_meshes; m++) (*mesh_base)[m + 1] = (*mesh_base)[m] + desc->meshes[m].num_triangles;
	return mesh_base->back() < 0x3ffffff0ull;
}

struct MeshPlans {
	std::vector<MeshPlan> plans;    // one per mesh of the description
	bool ok = true;
	int rc = 0;                     // refused with a code of its own (else 0: the build's default stands)
	char error[160] = "";           // refused: what rtk_set_error is given
};

// placements: one per mesh, or NULL; n: the scene's triangles (fewer than two: every mesh is decoded on the host);
// is_device: "is this the caller's device memory" (read in place, nothing is copied and nothing of it is read here)
static inline MeshPlans plan_meshes(const rtk_scene_desc *desc, const rtk_placement *placements, uint32_t n, bool (*is_device)(const void *))
{
	MeshPlans out;
	out.plans.assign(desc->num_meshes, MeshPlan());
#define PLAN_REFUSE(...) do { snprintf(out.error, sizeof(out.error), __VA_ARGS__); out.ok = false; return out; } while (0)
	for (size_t mi = 0; mi < desc->num_meshes; mi++) {
		const rtk_mesh *m = &desc->meshes[mi];
		MeshPlan &pl = out.plans[mi];
		const size_t nt = m->num_triangles;
		if (nt == 0) continue;
		if (!m->position_cb && m->position.type != RTK_TYPE_DEFAULT && m->position.type != RTK_TYPE_REAL && m->position.type != RTK_TYPE_F32 &&
			m->position.type != RTK_TYPE_F64) PLAN_REFUSE("rtk_dev_scene_build: mesh %zu: bad position type %d", mi, (int)m->position.type);
		// RTK_TYPE_DEFAULT on an index buffer means 32-bit indices (the reference's default index type, rtk.c:1049-1059)
		if (!m->index_cb && m->index.data && m->index.type != RTK_TYPE_DEFAULT && m->index.type != RTK_TYPE_U16 && m->index.type != RTK_TYPE_U32)
			PLAN_REFUSE("rtk_dev_scene_build: mesh %zu: bad index type %d", mi, (int)m->index.type);
		if (placements && m->position_cb) { out.rc = RTK_AMD_ERR_UNSUPPORTED; PLAN_REFUSE("rtk_dev_scene_build_placed: mesh %zu: a position callback gives world positions, it takes no placement", mi); }
		if (m->position_cb || m->index_cb || n < 2) { pl.on_host_decode = true; continue; }
		if (!m->position.data) PLAN_REFUSE("rtk_dev_scene_build: mesh %zu has no positions", mi);
		pl.f64 = m->position.type == RTK_TYPE_F64;
		pl.pstride = m->position.stride ? m->position.stride : (pl.f64 ? 24 : 12);
		pl.pos_src = (const char *)m->position.data;
		pl.pos_on_device = is_device(m->position.data);
		uint64_t max_vertex = 3ull * nt - 1;
		if (m->index.data) {
			const bool u16 = m->index.type == RTK_TYPE_U16;
			pl.idx_kind = u16 ? 1 : 2;
			pl.istride = m->index.stride ? m->index.stride : (u16 ? 6 : 12);
			pl.idx_src = (const char *)m->index.data;
			pl.idx_on_device = is_device(m->index.data);
			if (pl.idx_on_device && !pl.pos_on_device) PLAN_REFUSE("rtk_dev_scene_build: mesh %zu has device indices but host positions", mi);
			if (!pl.idx_on_device) {
				if (!pl.pos_on_device) {
					// the position buffer's extent is only known through the largest index used
					max_vertex = 0;
					for (size_t i = 0; i < nt; i++) {
						const char *p = pl.idx_src + i * pl.istride;
						for (int c = 0; c < 3; c++) {
							const uint64_t v = u16 ? ((const uint16_t *)p)[c] : ((const uint32_t *)p)[c];
							if (v > max_vertex) max_vertex = v;
						}
					}
				}
				pl.ibytes = (nt - 1) * pl.istride + (u16 ? 6 : 12);
			}
		}
		if (!pl.pos_on_device) pl.pbytes = (size_t)max_vertex * pl.pstride + (pl.f64 ? 24 : 12);
	}
#undef PLAN_REFUSE
	return out;
}

// ---- what n and the knobs decide before anything is placed: sort words, key width, tile mode ----

struct BuildPlan {
	bool packed = false;              // the triangle's number fits under a 40-bit code in one sort word
	uint32_t packed_bits = 40u;       // the width of that code
	uint32_t num_tiles = 0;
	bool tile_mode = false;           // more than one refit tile, and enough triangles: the subtrees inside a tile are collapsed by k_collapse_tile,
	                                  // only the nodes above them go through the level-by-level collapse
	uint32_t top_cap = 0;             // nodes above the tiles that the workspace holds
};

// force_bits: 0 = key width from the number of triangles; else the width of the Morton code in the packed sort words
static inline BuildPlan plan_build(uint32_t n, const BuildKnobs &knobs, uint32_t force_bits)
{
	BuildPlan p;
	// index fits under a 40-bit code in one word
	p.packed = n < (1u << 24) && knobs.sort_packed;
	// Key width from n: ceil(log2 n) + 8 bits of the code, rounded up to whole 8-bit passes -- every triangle still gets hundreds
	// of cells of its own on average, the splits below that are decided by the triangle's number (words are all different). The lab
	// found identical trees down to 30 bits at 1M triangles, and the 10M-triangle build has the same 4 709 302 nodes at 32 bits as at
	// 40 (profiles/r04_build_ab.log): 32 bits = FOUR passes wherever the index fits the word (n < 2^24), three below 64 k triangles.
	uint32_t lg = 0;
	while ((1ull << lg) < (unsigned long long)n) lg++;
	p.packed_bits = ((lg + 8u + 7u) / 8u) * 8u;
	if (p.packed_bits < 24u) p.packed_bits = 24u;
	if (p.packed_bits > 40u) p.packed_bits = 40u;
	if (force_bits) p.packed_bits = force_bits;
	if (knobs.key_bits) p.packed_bits = knobs.key_bits;
	p.num_tiles = (n + RTK_BUILD_REFIT_TILE - 1u) / RTK_BUILD_REFIT_TILE;
	p.tile_mode = p.num_tiles > 1u && (uint64_t)n >= knobs.tile_min;
	p.top_cap = std::min<uint32_t>(n / 2u, knobs.top_cap);
	return p;
}

// ---- three rules of the stages ----

// nodes the scene's arrays are allocated for before the collapse: what 4-wide trees over n triangles usually have, with room
static inline size_t plan_first_node_capacity(uint32_t n, int est_div)
{
	return est_div > 0 ? (size_t)n / (size_t)est_div + 16 : (size_t)n / 2 + 4096;
}

// the build was made with fewer than 40 bits and more than an eighth of the sorted neighbours share their code
static inline bool plan_key_too_narrow(const BuildPlan &p, uint32_t equal_codes, uint32_t n)
{
	return p.packed && p.packed_bits < 40u && (uint64_t)equal_codes * 8u > (uint64_t)n;
}

// levels with more than RTK_BUILD_COLLAPSE_SMALL_JOBS jobs in a balanced 4-wide tree over jobs_hint leaves, plus slack; a tree
// that is deeper than that takes further rounds
static inline unsigned plan_big_levels(uint64_t jobs_hint)
{
	unsigned big_levels = 2;
	for (uint64_t c = RTK_BUILD_COLLAPSE_SMALL_JOBS; c < jobs_hint; c *= 4) big_levels++;
	return big_levels;
}

#pragma GCC visibility pop
