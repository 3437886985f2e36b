// Driver of tests/test_build_plan_cpu.py: built by the host compiler against rtk_amd/csrc/rtk_build_plan.h alone (no HIP), with
// -fsanitize=address,undefined. Every line of standard input is one command; the answer is one line.
//
//   meshes <n> <placed> <M> then per mesh: nt ikind itype istride ialloc idev vcount ptype pstride palloc pdev cbs
//       ikind 0: no index buffer, 1: 16-bit values, 2: 32-bit values; itype / ptype: the rtk_type written into the description;
//       ialloc / palloc: bytes the buffer is allocated with -- exactly what the TEST expects the plan to say, so that a plan that
//       says more (or a scan of the indices that reads further) is a heap overflow (palloc -1: no position buffer at all);
//       idev / pdev: the "is this device memory" callable says yes (the buffer is then one byte that nobody may read);
//       index value number k is (7 k) mod vcount; cbs: 1 position callback, 2 index callback.
//       -> ok rc, then per mesh: host f64 idx_kind pstride istride pbytes ibytes pos_dev idx_dev src (src: the plan points at the
//       buffers it was given), then "| error text". Bytes [0, ibytes) and [0, pbytes) are then read as the upload reads them.
//   plan <n> <force_bits> <sort_packed> <key_bits> <tile_min> <top_cap>   -> packed bits tiles tile_mode top_cap
//   estimate <n> <div>   -> nodes;  narrow <packed> <bits> <equal> <n>   -> 0 / 1;  levels <jobs_hint>   -> big_levels
//   base <M> <nt>...   -> ok, then the M + 1 sums
//   knobs   -> key=value words;  setenv <NAME> [VALUE]   -> ok
#include "rtk_build_plan.h"

#include <string.h>

#include <iostream>
#include <memory>
#include <set>
#include <sstream>
#include <string>

static std::set<const void *> g_device;
static bool is_device(const void *p) { return g_device.count(p) != 0; }
static void position_cb(void *, const rtk_mesh *, rtk_vec3 *, const uint32_t *, size_t) {}
static void index_cb(void *, const rtk_mesh *, uint32_t *, size_t, size_t) {}

static int meshes_command(std::istringstream &in)
{
	unsigned long long n, placed, count;
	if (!(in >> n >> placed >> count)) return 2;
	std::vector<rtk_mesh> meshes(count);
	std::vector<std::unique_ptr<char[]>> buffers;
	g_device.clear();
	const auto buffer = [&buffers](long long bytes, bool device) {
		buffers.emplace_back(new char[device ? 1 : (size_t)bytes]());
		if (device) g_device.insert(buffers.back().get());
		return buffers.back().get();
	};
	for (rtk_mesh &m : meshes) {
		long long nt, ikind, itype, istride, ialloc, idev, vcount, ptype, pstride, palloc, pdev, cbs;
		if (!(in >> nt >> ikind >> itype >> istride >> ialloc >> idev >> vcount >> ptype >> pstride >> palloc >> pdev >> cbs)) return 2;
		memset(&m, 0, sizeof(m));
		m.num_triangles = (size_t)nt;
		m.position.type = (rtk_type)ptype;
		m.position.stride = (size_t)pstride;
		if (palloc >= 0) m.position.data = buffer(palloc, pdev != 0);
		m.index.type = (rtk_type)itype;
		m.index.stride = (size_t)istride;
		if (ikind) {
			char *data = buffer(ialloc, idev != 0);
			const size_t step = istride ? (size_t)istride : (ikind == 1 ? 6 : 12);
			for (long long k = 0; !idev && k < 3 * nt; k++) {
				const uint32_t v = (uint32_t)((7 * k) % vcount);
				char *at = data + (size_t)(k / 3) * step;
				if (ikind == 1) ((uint16_t *)at)[k % 3] = (uint16_t)v; else ((uint32_t *)at)[k % 3] = v;
			}
			m.index.data = data;
		}
		if (cbs & 1) m.position_cb = position_cb;
		if (cbs & 2) m.index_cb = index_cb;
	}
	rtk_scene_desc desc;
	memset(&desc, 0, sizeof(desc));
	desc.meshes = meshes.data();
	desc.num_meshes = meshes.size();
	const std::vector<rtk_placement> placements(meshes.size());
	const MeshPlans got = plan_meshes(&desc, placed ? placements.data() : nullptr, (uint32_t)n, is_device);
	std::cout << (got.ok ? 1 : 0) << ' ' << got.rc;
	unsigned long long sum = 0;
	for (size_t mi = 0; got.ok && mi < meshes.size(); mi++) {
		const MeshPlan &pl = got.plans[mi];
		const bool src = pl.on_host_decode || meshes[mi].num_triangles == 0 ||
			(pl.pos_src == (const char *)meshes[mi].position.data && pl.idx_src == (const char *)meshes[mi].index.data);
		std::cout << ' ' << pl.on_host_decode << ' ' << pl.f64 << ' ' << pl.idx_kind << ' ' << pl.pstride << ' ' << pl.istride << ' ' << pl.pbytes << ' ' << pl.ibytes
		          << ' ' << pl.pos_on_device << ' ' << pl.idx_on_device << ' ' << src;
		// what the upload does with the plan: every byte of the two extents is read
		for (size_t k = 0; k < pl.ibytes; k++) sum += (unsigned char)pl.idx_src[k];
		for (size_t k = 0; k < pl.pbytes; k++) sum += (unsigned char)pl.pos_src[k];
	}
	std::cout << " | " << got.error << (sum == ~0ull ? " " : "") << "\n";
	return 0;
}

int main()
{
	std::string line;
	while (std::getline(std::cin, line)) {
		std::istringstream in(line);
		std::string cmd;
		in >> cmd;
		if (cmd == "meshes") {
			if (meshes_command(in)) { std::cerr << "bad case: " << line << "\n"; return 2; }
		} else if (cmd == "plan") {
			unsigned long long n, force_bits, sort_packed, key_bits, tile_min, top_cap;
			if (!(in >> n >> force_bits >> sort_packed >> key_bits >> tile_min >> top_cap)) { std::cerr << "bad case: " << line << "\n"; return 2; }
			BuildKnobs k;
			memset(&k, 0, sizeof(k));
			k.sort_packed = sort_packed != 0; k.key_bits = (uint32_t)key_bits; k.tile_min = tile_min; k.top_cap = (uint32_t)top_cap;
			const BuildPlan p = plan_build((uint32_t)n, k, (uint32_t)force_bits);
			std::cout << p.packed << ' ' << p.packed_bits << ' ' << p.num_tiles << ' ' << p.tile_mode << ' ' << p.top_cap << "\n";
		} else if (cmd == "estimate") {
			unsigned long long n; int div;
			in >> n >> div;
			std::cout << plan_first_node_capacity((uint32_t)n, div) << "\n";
		} else if (cmd == "narrow") {
			unsigned long long packed, bits, equal, n;
			in >> packed >> bits >> equal >> n;
			BuildPlan p;
			p.packed = packed != 0; p.packed_bits = (uint32_t)bits;
			std::cout << plan_key_too_narrow(p, (uint32_t)equal, (uint32_t)n) << "\n";
		} else if (cmd == "levels") {
			unsigned long long hint;
			in >> hint;
			std::cout << plan_big_levels(hint) << "\n";
		} else if (cmd == "base") {
			size_t count;
			in >> count;
			std::vector<rtk_mesh> meshes(count);
			for (rtk_mesh &m : meshes) { memset(&m, 0, sizeof(m)); in >> m.num_triangles; }
			rtk_scene_desc desc;
			memset(&desc, 0, sizeof(desc));
			desc.meshes = meshes.data();
			desc.num_meshes = count;
			std::vector<uint64_t> base(3, 77);
			std::cout << plan_mesh_base(&desc, &base);
			for (uint64_t v : base) std::cout << ' ' << v;
			std::cout << "\n";
		} else if (cmd == "knobs") {
			const BuildKnobs k = read_build_knobs();
			float cn = 0.0f, ct = 0.0f;
			build_sah_costs_from_env(&cn, &ct);
			std::cout << "timing=" << k.timing << " host_time=" << k.host_time << " max_leaf=" << k.max_leaf << " sort_packed=" << k.sort_packed << " key_bits=" << k.key_bits
			          << " direct=" << k.direct << " fused_emit=" << k.fused_emit << " tile_min=" << k.tile_min << " top_cap=" << k.top_cap << " est_div=" << k.est_div
			          << " keep_workspace=" << k.keep_workspace << " key_rebuild=" << k.key_rebuild << " max_leaf_fn=" << build_max_leaf_from_env()
			          << " cost_node=" << cn << " cost_tri=" << ct << "\n";
		} else if (cmd == "setenv") {
			std::string name, value;
			in >> name >> value;
			setenv(name.c_str(), value.c_str(), 1);
			std::cout << "ok\n";
		} else { std::cerr << "bad command: " << line << "\n"; return 2; }
	}
	return 0;
}
