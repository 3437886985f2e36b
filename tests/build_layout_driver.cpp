// Driver of tests/test_build_layout_cpu.py: built by the host compiler against rtk_amd/csrc/rtk_build_layout.h alone (no HIP).
// Every line of standard input is one case: n packed tile_mode top_cap sort_words num_meshes, then ibytes pbytes of every mesh.
// The answer is one line of "key=value" words: ok, bytes, and the offset of every buffer (-1: the build has no such buffer;
// per-mesh uploads as idx<m> / pos<m>).
#include "rtk_build_layout.h"

#include <iostream>
#include <sstream>
#include <string>

int main()
{
	std::string line;
	while (std::getline(std::cin, line)) {
		std::istringstream in(line);
		unsigned long long n, packed, tile_mode, top_cap, sort_words, meshes;
		if (!(in >> n >> packed >> tile_mode >> top_cap >> sort_words >> meshes)) { std::cerr << "bad case: " << line << "\n"; return 2; }
		std::vector<BuildUpload> uploads(meshes);
		for (BuildUpload &u : uploads) {
			unsigned long long i, p;
			if (!(in >> i >> p)) { std::cerr << "bad case: " << line << "\n"; return 2; }
			u.ibytes = (size_t)i; u.pbytes = (size_t)p;
		}
		BuildLayout L;
		const bool ok = rtk_build_layout((uint32_t)n, uploads, packed != 0, tile_mode != 0, (uint32_t)top_cap, (size_t)sort_words, &L);
		std::cout << "ok=" << (ok ? 1 : 0);
		if (ok) {
			const auto put = [](const char *name, size_t off) { std::cout << ' ' << name << '=' << (off == RTK_BUILD_NO_BUFFER ? -1ll : (long long)off); };
			put("bytes", L.bytes);
#define PUT(f_) put(#f_, L.f_)
			PUT(in_tris); PUT(cent); PUT(bounds); PUT(keys_a); PUT(keys_b); PUT(vals_a); PUT(vals_b); PUT(sort_scratch); PUT(mesh_src);
			PUT(lr); PUT(range); PUT(climbers); PUT(half); PUT(arrive); PUT(root); PUT(bin); PUT(tile_count); PUT(tile_base); PUT(depth_word);
			PUT(area); PUT(tile_nclimb); PUT(nodes_tmp); PUT(top_refs); PUT(top_level); PUT(root_info); PUT(root_list); PUT(tile_nroots);
			PUT(jobs); PUT(dec); PUT(info); PUT(sums); PUT(ring);
#undef PUT
			for (size_t m = 0; m < uploads.size(); m++) {
				put(("idx" + std::to_string(m)).c_str(), L.mesh_idx[m]);
				put(("pos" + std::to_string(m)).c_str(), L.mesh_pos[m]);
			}
		}
		std::cout << "\n";
	}
	return 0;
}
