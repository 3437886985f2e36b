// rtk_refit_plan.h -- what the host decides in a refit, between the kernels: what is refused, where every mesh's positions are
// read from and what is staged for them, the sizes and offsets of the temporaries and of the kept tables, the workspace to
// borrow, the sort widths, the runs of listed meshes, whether the dirty set pays, which heights share a launch. Plain C++17, no
// HIP: the host compiler builds it alone (tests/test_refit_plan_cpu.py does, under the address sanitizer). What needs the device
// arrives as a parameter. rtk_refit.hip carries the plans out.
#pragma once

#include "rtk.h"
#include "rtk_amd.h"
#include "rtk_carve.h"

#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include <vector>

#pragma GCC visibility push(hidden)      // (nothing here is part of the library's interface, nor what the standard templates make of it)

// ---- what the kernels and the host share ----

// (The two records below are kernel parameters, and a kernel's name spells out where its parameter types live: they stay in the
// unnamed namespace rtk_refit.hip had them in, and with them everything here that holds one.)
namespace {

// where one mesh's positions are read from (device memory: the caller's own buffer or its copy in the workspace)
struct RefitMesh {
	const char *pos;
	unsigned long long stride;
	uint32_t f64;
	uint32_t pad;
};
static_assert(sizeof(RefitMesh) == 24, "RefitMesh");

// A run of listed meshes that are neighbours in mesh_slots: its entries from entry_begin on belong to the threads from
// thread_begin on (the last run is followed by one that begins at the thread count).
struct RefitRange { uint32_t entry_begin, thread_begin; };

#define REFIT_SMALL_THREADS 1024                 // k_refit_small: four lanes per node, 256 nodes per trip
#define REFIT_SMALL_LEVEL 1024u                // heights of at most this many nodes go to k_refit_small

// Above this share of the scene's triangles in the listed meshes the dirty-set passes lose against the full box and finish
// passes, which then run instead (the triangles are still regathered for the listed meshes only). Where the two measured
// curves meet, rounded down to a power of two: profiles/refit_meshes_timing.log. RTK_AMD_REFIT_MESHES_SHARE overrides it
// (0: always the full passes, 1: never), for A/B; read at every call, so one process can measure both.
#define REFIT_MESHES_MAX_SHARE 0.25
static inline double partial_max_share()
{
	const char *e = getenv("RTK_AMD_REFIT_MESHES_SHARE");
	return e ? atof(e) : REFIT_MESHES_MAX_SHARE;
}

// ---- refusals: everything that can be refused is refused here, before HIP is touched ----

typedef void (*refit_error_fn)(const char *fmt, ...) __attribute__((format(printf, 1, 2)));      // rtk_set_error

// the rules for the positions of a mesh that is read
static inline int check_mesh_positions(refit_error_fn fail, const char *who, const rtk_mesh *m, size_t mi)
{
	if (m->position_cb) { fail("%s: mesh %zu: position callbacks are not supported by a refit", who, mi); return RTK_AMD_ERR_UNSUPPORTED; }
	if (m->num_triangles == 0) return RTK_AMD_OK;
	if (m->position.type != RTK_TYPE_DEFAULT && m->position.type != RTK_TYPE_REAL && m->position.type != RTK_TYPE_F32 && m->position.type != RTK_TYPE_F64) {
		fail("%s: mesh %zu: bad position type %d", who, mi, (int)m->position.type);
		return RTK_AMD_ERR_BAD_ARG;
	}
	if (!m->position.data) { fail("%s: mesh %zu has no positions", who, mi); return RTK_AMD_ERR_BAD_ARG; }
	return RTK_AMD_OK;
}

// the description against the scene it claims to describe (mesh_base: the scene's, num_meshes + 1 sums, or empty)
static inline int check_desc(refit_error_fn fail, const char *who, const std::vector<uint64_t> &mesh_base, const rtk_scene_desc *desc)
{
	if (!desc->meshes && desc->num_meshes) { fail("%s: NULL meshes", who); return RTK_AMD_ERR_BAD_ARG; }
	const size_t scene_meshes = mesh_base.empty() ? 0 : mesh_base.size() - 1;
	if (desc->num_meshes != scene_meshes) {
		fail("%s: %zu meshes, the scene was made from %zu", who, (size_t)desc->num_meshes, scene_meshes);
		return RTK_AMD_ERR_BAD_ARG;
	}
	for (size_t mi = 0; mi < desc->num_meshes; mi++) {
		const uint64_t have = mesh_base[mi + 1] - mesh_base[mi];
		if ((uint64_t)desc->meshes[mi].num_triangles != have) {
			fail("%s: mesh %zu has %zu triangles, the scene's has %llu", who, mi, (size_t)desc->meshes[mi].num_triangles, (unsigned long long)have);
			return RTK_AMD_ERR_BAD_ARG;
		}
	}
	return RTK_AMD_OK;
}

// What a call comes to once its arguments have been looked at.
struct RefitScope {
	int rc = RTK_AMD_OK;              // not RTK_AMD_OK: refused, `fail` has been told why
	bool nothing = false;             // the listed meshes have no triangle: nothing moves, no bit changes, nothing is launched
	bool full = true;                 // every mesh is read (false: the flagged ones)
	std::vector<uint8_t> flags;       // per-mesh forms: one per mesh (one entry where there is none); an id that repeats counts once
	uint64_t listed_tris = 0;         // triangles in the flagged meshes
	const uint8_t *listed() const { return full ? nullptr : flags.data(); }      // what refit_on_device is given
};

// Both full refits. who: the public function the error texts name; mesh_base: the scene's, NULL without a scene; placed: the
// _placed entry point, which needs placements.
static inline RefitScope check_refit_all(refit_error_fn fail, const char *who, const std::vector<uint64_t> *mesh_base, const rtk_scene_desc *desc,
	const rtk_placement *placements, bool placed)
{
	RefitScope s;
	if (!mesh_base || !desc || (placed && !placements)) { fail("%s: NULL argument", who); s.rc = RTK_AMD_ERR_BAD_ARG; return s; }
	s.rc = check_desc(fail, who, *mesh_base, desc);
	for (size_t mi = 0; s.rc == RTK_AMD_OK && mi < desc->num_meshes; mi++) s.rc = check_mesh_positions(fail, who, &desc->meshes[mi], mi);
	return s;
}

// Both per-mesh refits, likewise: only the listed meshes' positions (and placements) are looked at.
static inline RefitScope check_refit_some(refit_error_fn fail, const char *who, const std::vector<uint64_t> *mesh_base, const rtk_scene_desc *desc,
	const rtk_placement *placements, bool placed, const uint32_t *mesh_ids, size_t num_ids)
{
	RefitScope s;
	s.rc = RTK_AMD_ERR_BAD_ARG;
	if (!mesh_base || !desc || (placed && !placements)) { fail("%s: NULL argument", who); return s; }
	if (!mesh_ids && num_ids) { fail("%s: NULL mesh_ids with %zu ids", who, num_ids); return s; }
	s.rc = check_desc(fail, who, *mesh_base, desc);
	if (s.rc != RTK_AMD_OK) return s;
	s.flags.assign(desc->num_meshes ? desc->num_meshes : 1, 0);
	for (size_t k = 0; k < num_ids; k++) {
		if (mesh_ids[k] >= desc->num_meshes) { fail("%s: mesh id %u, the scene has %zu meshes", who, mesh_ids[k], (size_t)desc->num_meshes); s.rc = RTK_AMD_ERR_BAD_ARG; return s; }
		s.flags[mesh_ids[k]] = 1;
	}
	for (size_t mi = 0; mi < desc->num_meshes; mi++) {
		if (!s.flags[mi]) continue;
		s.rc = check_mesh_positions(fail, who, &desc->meshes[mi], mi);
		if (s.rc != RTK_AMD_OK) return s;
		s.listed_tris += desc->meshes[mi].num_triangles;
	}
	s.nothing = s.listed_tris == 0;
	// every mesh that has a triangle is listed: that IS the full refit (no mesh it would read is one this call may not read)
	s.full = !s.nothing && s.listed_tris == mesh_base->back();
	return s;
}

// ---- where every mesh's positions are read from ----

struct RefitSource {
	bool need_max_vertex = false;     // a mesh that is read lies in host memory and max_vertex was not given: make it, then plan again
	std::vector<RefitMesh> table;     // one per mesh (one entry where there is none); pos NULL: not read. A staged mesh still names the caller's buffer
	std::vector<size_t> staged;       // bytes of the caller's host buffer that are copied (0: device memory, or not read) ...
	std::vector<size_t> staged_at;    // ... to this offset of the workspace, every copy on a 256-byte step
	std::vector<rtk_placement> places;    // placed forms: the placements of the meshes that are read, zeros for the others (one entry where there is no mesh)
	size_t places_at = 0;             // ... copied behind the staged positions
	size_t upload_bytes = 0;          // the workspace all of that takes
	bool any_device = false;          // a mesh is read from the caller's device memory
	int mode = 0;                     // 0: every mesh that is read has float positions, 1: every one doubles, 2: both occur
};

// listed: NULL = every mesh, else one flag per mesh; placements: NULL, or one per mesh (only the entries of meshes that are read
// are looked at); is_device: "is this the caller's device memory" (read in place); max_vertex: the largest vertex index each
// mesh's triangles use, NULL = not made yet (needed, and so made, only when a read mesh is host-resident)
static inline RefitSource plan_source(const rtk_scene_desc *desc, const rtk_placement *placements, const uint8_t *listed, bool (*is_device)(const void *),
	const uint32_t *max_vertex)
{
	RefitSource s;
	const size_t num_meshes = desc->num_meshes;
	s.table.assign(num_meshes ? num_meshes : 1, RefitMesh{ nullptr, 0ull, 0u, 0u });
	s.staged.assign(num_meshes, 0);
	s.staged_at.assign(num_meshes, 0);
	bool any_f32 = false, any_f64 = false;
	for (size_t mi = 0; mi < num_meshes; mi++) {
		const rtk_mesh *m = &desc->meshes[mi];
		if (m->num_triangles == 0 || (listed && !listed[mi])) continue;
		RefitMesh &t = s.table[mi];
		t.f64 = m->position.type == RTK_TYPE_F64 ? 1u : 0u;
		t.stride = m->position.stride ? m->position.stride : (t.f64 ? 24 : 12);
		t.pos = (const char *)m->position.data;
		(t.f64 ? any_f64 : any_f32) = true;
		if (is_device(m->position.data)) { s.any_device = true; continue; }
		if (!max_vertex) { s.need_max_vertex = true; return s; }
		s.staged[mi] = (size_t)max_vertex[mi] * t.stride + (t.f64 ? 24 : 12);
		s.staged_at[mi] = s.upload_bytes;
		s.upload_bytes += rtk_padded(s.staged[mi]);
	}
	// the placements of the meshes that are read go to the device beside the staged positions (entries of other meshes: zeros)
	if (placements) {
		s.places.assign(num_meshes ? num_meshes : 1, rtk_placement{});
		for (size_t mi = 0; mi < num_meshes; mi++) if (s.table[mi].pos) s.places[mi] = placements[mi];
		s.places_at = s.upload_bytes;
		s.upload_bytes += rtk_padded(s.places.size() * sizeof(rtk_placement));
	}
	s.mode = any_f64 && any_f32 ? 2 : any_f64 ? 1 : 0;
	return s;
}

// ---- sizes and offsets (sort_words: rtk_sort_scratch_words of the same count) ----

// temporaries of the schedule: heights, the changed word, two key arrays, the sort's scratch, level starts
struct ScheduleTmp { size_t o_height, o_changed, o_ka, o_kb, o_sort, o_ls, bytes; };
static inline ScheduleTmp schedule_tmp(uint32_t n, size_t sort_words)
{
	Carve c;       // (a braced list is evaluated left to right: the pieces in the order of the members, then their sum)
	return ScheduleTmp{ c.take((size_t)n * 4), c.take(4), c.take((size_t)n * 8), c.take((size_t)n * 8), c.take(sort_words * 4), c.take(((size_t)n + 2) * 4), c.bytes };
}

// temporaries of the per-mesh tables: two key arrays over the slots and the sort's scratch
struct TablesTmp { size_t o_ka, o_kb, o_sort, bytes; };
static inline TablesTmp tables_tmp(uint32_t num_tris, size_t sort_words)
{
	Carve c;
	return TablesTmp{ c.take((size_t)num_tris * 8), c.take((size_t)num_tris * 8), c.take(sort_words * 4), c.bytes };
}

// The level starts and the mesh table share one small allocation. The table lies behind the carve: the last piece, not padded,
// with room for one record even where there is no mesh, which the ledger does not count.
struct ScheduleSmall { size_t o_meshes, bytes, counted; };
static inline ScheduleSmall schedule_small(size_t heights, size_t num_meshes)
{
	Carve c;
	c.take((heights + 1) * 4);
	return ScheduleSmall{ c.bytes, c.bytes + (num_meshes ? num_meshes : 1) * sizeof(RefitMesh), c.counted + num_meshes * sizeof(RefitMesh) };
}

// the tables of the per-mesh refit, one allocation (RefitPartial, rtk_dev.h); dirty_blocks: workgroups of the compaction
struct PartialTables { size_t o_parent, o_slot_node, o_mesh_slots, o_dirty, o_list, o_block, o_list_start, o_ranges, bytes, counted; };
static inline PartialTables partial_tables(uint32_t n, uint32_t num_tris, size_t num_meshes, size_t heights, uint32_t dirty_blocks)
{
	Carve c;
	return PartialTables{ c.take((size_t)n * 4), c.take((size_t)num_tris * 4), c.take((size_t)num_tris * 4), c.take((size_t)n * 4), c.take((size_t)n * 4),
		c.take(((size_t)dirty_blocks + 1) * 4), c.take((heights + 1) * 4), c.take((num_meshes + 1) * sizeof(RefitRange)), c.bytes, c.counted };
}

// The workspace a call borrows: first the temporaries of the schedule (the first refit of a scene; over when the schedule is
// made), then those of the per-mesh tables (the first refit of some meshes), then the staged positions and placements. 0: no loan.
static inline size_t plan_borrow(bool schedule_ready, const ScheduleTmp &schedule, bool tables_needed, const TablesTmp &tables, size_t upload_bytes)
{
	const size_t schedule_bytes = schedule_ready ? 0 : schedule.bytes;
	const size_t tables_bytes = tables_needed ? tables.bytes : 0;
	size_t borrow = schedule_bytes > upload_bytes ? schedule_bytes : upload_bytes;
	if (tables_bytes > borrow) borrow = tables_bytes;
	return borrow;
}

// ---- rules of the schedule and the tables ----

// heights are below n: that many bits of the upper word, in whole 8-bit passes; stable, so numbers stay in order
static inline uint32_t height_sort_bits(uint32_t n)
{
	uint32_t bits = 1;
	while (bits < 32u && (1ull << bits) <= (unsigned long long)n) bits++;
	return bits;
}

// mesh numbers are below num_meshes: that many bits of the upper word (0: one mesh, no sort); stable, so the slots of a mesh stay ascending
static inline uint32_t mesh_sort_bits(size_t num_meshes)
{
	uint32_t bits = 0;
	while (bits < 32u && (1ull << bits) < (unsigned long long)num_meshes) bits++;
	return bits;
}

// A tree has no cycle and its heights are below max_depth, so max_depth sweeps settle them; one more, which must change
// nothing, is the proof. Should a scene's max_depth be too small the rounds go on, eight sweeps at a time ...
static inline uint32_t sweep_round(bool first, uint32_t max_depth) { return !first ? 8u : max_depth < 4096u ? max_depth + 1u : 4096u; }
// ... until no tree of n nodes could still be changing
static inline bool sweeps_exhausted(uint32_t sweeps, uint32_t n) { return sweeps > n + 8u; }

// every height up to the largest occurs, so the starts rise strictly from 0 to n
static inline bool level_starts_sane(const std::vector<uint32_t> &level_start, uint32_t n)
{
	bool sane = !level_start.empty() && level_start.front() == 0u && level_start.back() == n;
	for (size_t h = 0; h + 1 < level_start.size(); h++) sane = sane && level_start[h] < level_start[h + 1];
	return sane;
}

// ---- per call: the listed meshes' threads, the dirty set, the launches of the box pass ----

// runs of listed meshes that are neighbours in mesh_slots, one thread per slot (mesh_base: the scene's)
struct RefitRuns { std::vector<RefitRange> ranges; uint64_t threads = 0; };
static inline RefitRuns plan_runs(const uint8_t *listed, const std::vector<uint64_t> &mesh_base, size_t num_meshes)
{
	RefitRuns r;
	uint64_t run_end = 0;
	for (size_t mi = 0; mi < num_meshes; mi++) {
		if (!listed[mi] || mesh_base[mi + 1] == mesh_base[mi]) continue;
		if (r.ranges.empty() || run_end != mesh_base[mi]) r.ranges.push_back(RefitRange{ (uint32_t)mesh_base[mi], (uint32_t)r.threads });
		r.threads += mesh_base[mi + 1] - mesh_base[mi];
		run_end = mesh_base[mi + 1];
	}
	return r;
}

// the dirty set pays while the listed meshes are a small part of the scene and the other boxes can be trusted
static inline bool plan_dirty_set(bool listed, bool were_exact, uint64_t listed_tris, uint32_t num_tris, double max_share)
{
	return listed && were_exact && (double)listed_tris <= max_share * (double)num_tris;
}

// the mark of this call in the dirty flags; clear: every 2^32 calls the flags start over
struct EpochStep { uint32_t epoch; bool clear; };
static inline EpochStep next_epoch(uint32_t epoch)
{
	return epoch + 1u == 0u ? EpochStep{ 1u, true } : EpochStep{ epoch + 1u, false };
}

// One launch of the box pass: a height of more than REFIT_SMALL_LEVEL nodes alone (entries [begin, end) of the schedule, four
// lanes per node in `blocks` workgroups of 256), or a run of small heights [h, h1) in one workgroup. Which heights get a launch
// of their own is the full schedule's decision also where only the dirty nodes are remade (the host does not know their
// counts): a height that is small there is small here.
struct LevelStep { bool small; uint32_t h, h1, begin, end; size_t blocks; };
static inline std::vector<LevelStep> plan_levels(const std::vector<uint32_t> &level_start)
{
	std::vector<LevelStep> steps;
	const uint32_t heights = level_start.empty() ? 0u : (uint32_t)level_start.size() - 1u;
	steps.reserve(heights);
	for (uint32_t h = 0; h < heights;) {
		const uint32_t begin = level_start[h], end = level_start[h + 1];
		uint32_t h1 = h + 1;
		const bool small = end - begin <= REFIT_SMALL_LEVEL;
		while (small && h1 < heights && level_start[h1 + 1] - level_start[h1] <= REFIT_SMALL_LEVEL) h1++;
		steps.push_back(LevelStep{ small, h, h1, begin, small ? level_start[h1] : end, small ? 1 : ((size_t)(end - begin) * 4 + 255) / 256 });
		h = h1;
	}
	return steps;
}

} // namespace

#pragma GCC visibility pop
