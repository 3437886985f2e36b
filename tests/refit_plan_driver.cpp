// Driver of tests/test_refit_plan_cpu.py: built by the host compiler against rtk_amd/csrc/rtk_refit_plan.h alone (no HIP), with
// -fsanitize=address,undefined. Every line of standard input is one command; the answer is one line. Whatever a plan reads --
// position buffers, mesh_ids, mesh_base, level_start -- is a heap block of exactly the bytes the TEST expects it to need.
//
//   check <who> <scene> <desc> <placed> <placements> <some> <ids> <num_ids> id... <S> sum*(S) <M> <meshes> then per mesh: nt ptype cb data
//       scene / desc / placements / ids / meshes / data: 0 = the pointer is NULL; S: entries of the scene's mesh_base (0: empty);
//       some: the per-mesh form   -> rc nothing full listed_tris flags(one word, "-" for none) | error text
//   source <placed> <listed> <have_mv> <M> then per mesh: nt ptype pstride where flag mv alloc
//       where 0: host memory of `alloc` bytes, 1: device memory (one byte nobody may read); flag: listed[mi]; mv: max_vertex[mi]
//       -> need_mv any_device mode upload_bytes places_at places, then per mesh: read stride f64 staged staged_at placed
//       (placed: the mesh's entry of the placement copy is the caller's, not zeros). [0, staged) of every buffer is then read.
//   tmp <n> <sort_words> | tables <nt> <sort_words> | small <heights> <meshes> | partial <n> <nt> <meshes> <heights> <blocks>   -> the record's fields
//   borrow <ready> <schedule_bytes> <needed> <tables_bytes> <upload>   -> bytes
//   hbits <n> | mbits <meshes> | sweep <first> <max_depth> | exhausted <sweeps> <n> | epoch <e> | share
//   sane <n> <k> v*(k) | levels <k> v*(k) | runs <M> flag*(M) sum*(M + 1) | dirty <listed> <exact> <listed_tris> <num_tris>
//   setenv <NAME> [VALUE]
#include "rtk_refit_plan.h"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <iostream>
#include <memory>
#include <set>
#include <sstream>
#include <string>

static char g_error[512];
__attribute__((format(printf, 1, 2))) static void fail(const char *fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_error, sizeof(g_error), fmt, ap);
	va_end(ap);
}
static std::set<const void *> g_device;
static bool is_device(const void *p) { return g_device.count(p) != 0; }
static void position_cb(void *, const rtk_mesh *, rtk_vec3 *, const uint32_t *, size_t) {}

// k numbers in a heap block of exactly k entries
template <class T> static bool read_exact(std::istringstream &in, size_t k, std::vector<T> *out)
{
	out->clear();
	out->reserve(k);
	for (size_t i = 0; i < k; i++) { unsigned long long v; if (!(in >> v)) return false; out->push_back((T)v); }
	return true;
}

static int check_command(std::istringstream &in)
{
	std::string who;
	int scene, have_desc, placed, have_placements, some, have_ids, have_meshes;
	size_t num_ids, S, M;
	std::vector<uint32_t> ids;
	std::vector<uint64_t> base;
	if (!(in >> who >> scene >> have_desc >> placed >> have_placements >> some >> have_ids >> num_ids) || !read_exact(in, have_ids ? num_ids : 0, &ids)) return 2;
	if (!(in >> S) || !read_exact(in, S, &base) || !(in >> M >> have_meshes)) return 2;
	std::unique_ptr<rtk_mesh[]> meshes(new rtk_mesh[M]);
	static char some_positions[1];
	for (size_t mi = 0; mi < M; mi++) {
		unsigned long long nt; int ptype, cb, data;
		if (!(in >> nt >> ptype >> cb >> data)) return 2;
		rtk_mesh &m = meshes[mi];
		memset(&m, 0, sizeof(m));
		m.num_triangles = (size_t)nt;
		m.position.type = (rtk_type)ptype;
		if (cb) m.position_cb = position_cb;
		if (data) m.position.data = some_positions;
	}
	rtk_scene_desc desc;
	memset(&desc, 0, sizeof(desc));
	desc.meshes = have_meshes ? meshes.get() : nullptr;
	desc.num_meshes = M;
	const std::unique_ptr<rtk_placement[]> placements(new rtk_placement[M]);
	g_error[0] = 0;
	const rtk_scene_desc *d = have_desc ? &desc : nullptr;
	const rtk_placement *p = have_placements ? placements.get() : nullptr;
	const RefitScope s = some ? check_refit_some(fail, who.c_str(), scene ? &base : nullptr, d, p, placed != 0, have_ids ? ids.data() : nullptr, num_ids)
	                          : check_refit_all(fail, who.c_str(), scene ? &base : nullptr, d, p, placed != 0);
	std::string flags;
	for (uint8_t f : s.flags) flags += f ? '1' : '0';
	const bool listed_ok = s.rc != RTK_AMD_OK || s.nothing || (s.listed() == nullptr) == s.full;
	std::cout << s.rc << ' ' << s.nothing << ' ' << s.full << ' ' << s.listed_tris << ' ' << (flags.empty() ? "-" : flags) << (listed_ok ? "" : " LISTED?") << " | " << g_error << "\n";
	return 0;
}

static int source_command(std::istringstream &in)
{
	int placed, have_listed, have_mv;
	size_t M;
	if (!(in >> placed >> have_listed >> have_mv >> M)) return 2;
	std::unique_ptr<rtk_mesh[]> meshes(new rtk_mesh[M]);
	std::vector<std::unique_ptr<char[]>> buffers;
	std::vector<uint8_t> listed;
	std::vector<uint32_t> mv;
	std::vector<rtk_placement> placements;
	listed.reserve(M); mv.reserve(M); placements.reserve(M ? M : 1);      // (no mesh: still a pointer that is not NULL)
	g_device.clear();
	for (size_t mi = 0; mi < M; mi++) {
		unsigned long long nt, pstride, flag, v, alloc; int ptype, where;
		if (!(in >> nt >> ptype >> pstride >> where >> flag >> v >> alloc)) return 2;
		rtk_mesh &m = meshes[mi];
		memset(&m, 0, sizeof(m));
		m.num_triangles = (size_t)nt;
		m.position.type = (rtk_type)ptype;
		m.position.stride = (size_t)pstride;
		buffers.emplace_back(new char[where ? 1 : (size_t)alloc]());
		if (where) g_device.insert(buffers.back().get());
		m.position.data = buffers.back().get();
		listed.push_back((uint8_t)flag);
		mv.push_back((uint32_t)v);
		rtk_placement pl;
		for (int k = 0; k < 12; k++) pl.m[k] = (float)(mi + 1);
		placements.push_back(pl);
	}
	rtk_scene_desc desc;
	memset(&desc, 0, sizeof(desc));
	desc.meshes = meshes.get();
	desc.num_meshes = M;
	const RefitSource s = plan_source(&desc, placed ? placements.data() : nullptr, have_listed ? listed.data() : nullptr, is_device, have_mv ? mv.data() : nullptr);
	std::cout << s.need_max_vertex << ' ' << s.any_device << ' ' << s.mode << ' ' << s.upload_bytes << ' ' << s.places_at << ' ' << s.places.size();
	unsigned long long sum = 0;
	for (size_t mi = 0; !s.need_max_vertex && mi < M; mi++) {
		const RefitMesh &t = s.table[mi];
		const bool mine = t.pos == nullptr || t.pos == (const char *)meshes[mi].position.data;
		const bool put = !s.places.empty() && s.places[mi].m[0] == (float)(mi + 1) && s.places[mi].m[11] == (float)(mi + 1);
		const bool zero = !s.places.empty() && s.places[mi].m[0] == 0.0f && s.places[mi].m[11] == 0.0f;
		std::cout << ' ' << (t.pos != nullptr) << ' ' << t.stride << ' ' << t.f64 << ' ' << s.staged[mi] << ' ' << s.staged_at[mi] << ' ' << (put ? 1 : zero ? 0 : -1)
		          << (mine && t.pad == 0u ? "" : " SOURCE?");
		// what the staging copy does with the plan: every byte of the extent is read
		for (size_t k = 0; k < s.staged[mi]; k++) sum += (unsigned char)t.pos[k];
	}
	std::cout << (sum == ~0ull ? " " : "") << "\n";
	return 0;
}

int main()
{
	std::string line;
	while (std::getline(std::cin, line)) {
		std::istringstream in(line);
		std::string cmd;
		in >> cmd;
		unsigned long long a = 0, b = 0, c = 0, d = 0, e = 0;
		int bad = 0;
		if (cmd == "check") bad = check_command(in);
		else if (cmd == "source") bad = source_command(in);
		else if (cmd == "tmp") {
			in >> a >> b;
			const ScheduleTmp T = schedule_tmp((uint32_t)a, (size_t)b);
			std::cout << T.o_height << ' ' << T.o_changed << ' ' << T.o_ka << ' ' << T.o_kb << ' ' << T.o_sort << ' ' << T.o_ls << ' ' << T.bytes << "\n";
		} else if (cmd == "tables") {
			in >> a >> b;
			const TablesTmp T = tables_tmp((uint32_t)a, (size_t)b);
			std::cout << T.o_ka << ' ' << T.o_kb << ' ' << T.o_sort << ' ' << T.bytes << "\n";
		} else if (cmd == "small") {
			in >> a >> b;
			const ScheduleSmall s = schedule_small((size_t)a, (size_t)b);
			std::cout << s.o_meshes << ' ' << s.bytes << ' ' << s.counted << "\n";
		} else if (cmd == "partial") {
			in >> a >> b >> c >> d >> e;
			const PartialTables P = partial_tables((uint32_t)a, (uint32_t)b, (size_t)c, (size_t)d, (uint32_t)e);
			std::cout << P.o_parent << ' ' << P.o_slot_node << ' ' << P.o_mesh_slots << ' ' << P.o_dirty << ' ' << P.o_list << ' ' << P.o_block << ' ' << P.o_list_start << ' '
			          << P.o_ranges << ' ' << P.bytes << ' ' << P.counted << "\n";
		} else if (cmd == "borrow") {
			in >> a >> b >> c >> d >> e;
			ScheduleTmp st = {}; TablesTmp tt = {};
			st.bytes = (size_t)b; tt.bytes = (size_t)d;
			std::cout << plan_borrow(a != 0, st, c != 0, tt, (size_t)e) << "\n";
		} else if (cmd == "hbits") { in >> a; std::cout << height_sort_bits((uint32_t)a) << "\n"; }
		else if (cmd == "mbits") { in >> a; std::cout << mesh_sort_bits((size_t)a) << "\n"; }
		else if (cmd == "sweep") { in >> a >> b; std::cout << sweep_round(a != 0, (uint32_t)b) << "\n"; }
		else if (cmd == "exhausted") { in >> a >> b; std::cout << sweeps_exhausted((uint32_t)a, (uint32_t)b) << "\n"; }
		else if (cmd == "epoch") { in >> a; const EpochStep s = next_epoch((uint32_t)a); std::cout << s.epoch << ' ' << s.clear << "\n"; }
		else if (cmd == "share") std::cout << partial_max_share() << "\n";
		else if (cmd == "dirty") { in >> a >> b >> c >> d; std::cout << plan_dirty_set(a != 0, b != 0, c, (uint32_t)d, partial_max_share()) << "\n"; }
		else if (cmd == "sane") {
			std::vector<uint32_t> ls;
			in >> a >> b;
			if (!read_exact(in, (size_t)b, &ls)) bad = 2; else std::cout << level_starts_sane(ls, (uint32_t)a) << "\n";
		} else if (cmd == "levels") {
			std::vector<uint32_t> ls;
			in >> a;
			if (!read_exact(in, (size_t)a, &ls)) bad = 2;
			else {
				const std::vector<LevelStep> steps = plan_levels(ls);
				std::cout << steps.size();
				for (const LevelStep &s : steps) std::cout << ' ' << s.small << ' ' << s.h << ' ' << s.h1 << ' ' << s.begin << ' ' << s.end << ' ' << s.blocks;
				std::cout << "\n";
			}
		} else if (cmd == "runs") {
			std::vector<uint8_t> listed;
			std::vector<uint64_t> base;
			in >> a;
			if (!read_exact(in, (size_t)a, &listed) || !read_exact(in, (size_t)a + 1, &base)) bad = 2;
			else {
				const RefitRuns r = plan_runs(listed.data(), base, (size_t)a);
				std::cout << r.threads << ' ' << r.ranges.size();
				for (const RefitRange &g : r.ranges) std::cout << ' ' << g.entry_begin << ' ' << g.thread_begin;
				std::cout << "\n";
			}
		} else if (cmd == "setenv") {
			std::string name, value;
			in >> name >> value;
			setenv(name.c_str(), value.c_str(), 1);
			std::cout << "ok\n";
		} else bad = 2;
		if (bad) { std::cerr << "bad command: " << line << "\n"; return 2; }
	}
	return 0;
}
