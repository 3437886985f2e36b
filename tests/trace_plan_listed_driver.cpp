// Driver of tests/test_trace_plan_listed_cpu.py: tests/trace_plan_driver.cpp with the two inputs that listed batches
// (rtk_dev_trace_rays*_listed) add to the plan -- "listed" (TraceRequest::listed) and "lane_listed_loaded" (the listed forms of the
// assembly per-lane kernels) --, built by the host compiler against rtk_amd/csrc/rtk_trace_plan.h alone (no HIP).
// Every line of standard input is one case, "key=value" words that overwrite the defaults below; the answer is one line of
// "key=value" words: the decoded options, wants_image_look, variant_of and every field of plan_trace.
#include "rtk_trace_plan.h"

#include <iostream>
#include <map>
#include <sstream>
#include <string>

int main()
{
	std::string line;
	while (std::getline(std::cin, line)) {
		std::map<std::string, double> in;
		std::istringstream words(line);
		std::string word;
		while (words >> word) {
			const size_t eq = word.find('=');
			if (eq == std::string::npos) { std::cerr << "bad word: " << word << "\n"; return 2; }
			in[word.substr(0, eq)] = std::stod(word.substr(eq + 1));
		}
		const auto get = [&in](const char *key, double value) { const auto it = in.find(key); if (it == in.end()) return value; const double v = it->second; in.erase(it); return v; };

		TraceRequest rq;
		rq.n = (size_t)get("n", 1000000);
		rq.any_hit = get("any_hit", 0) != 0;
		rq.counted = get("counted", 0) != 0;
		rq.pk_counted = get("pk_counted", 0) != 0;
		rq.collect = get("collect", 0) != 0;
		rq.filtered = get("filtered", 0) != 0;
		rq.has_filter = get("has_filter", rq.filtered ? 1 : 0) != 0;
		if (in.count("listed")) rq.listed = get("listed", 0) != 0;      // (not given: the struct's own default)

		// struct_size = -1: no options block at all
		rtk_trace_opts opts = {};
		const double struct_size = get("struct_size", -1);
		opts.struct_size = struct_size < 0 ? 0u : (uint32_t)struct_size;
		opts.flags = (uint32_t)get("flags", 0);
		opts.image_width = (uint32_t)get("image_width", 0);
		opts.image_height = (uint32_t)get("image_height", 0);
		opts.refill_min = (uint32_t)get("refill_min", 0);
		opts.blocks_per_cu = (uint32_t)get("blocks_per_cu", 0);
		opts.node_exit = (uint32_t)get("node_exit", 0);
		const TraceOpts o = decode_opts(struct_size < 0 ? nullptr : &opts);

		SceneFacts f;
		f.num_nodes = (uint32_t)get("num_nodes", 200000);
		f.num_tris = (uint32_t)get("num_tris", 1000000);
		f.has_qnodes = get("has_qnodes", 1) != 0;
		f.stack_entries = (uint32_t)get("stack_entries", 40);
		f.bound_abs = (float)get("bound_abs", 100.0);
		f.big_leaf_fraction = get("big_leaf_fraction", 0.0);
		f.num_cus = (int)get("num_cus", 256);

		DeviceKernels dk;
		const int loaded = (int)get("loaded", 31);           // bit k: PacketKernel k
		const int fit[NUM_PACKET_KERNELS] = { 7, 8, 7, 7, 7 };
		for (int k = 0; k < NUM_PACKET_KERNELS; k++) { dk.packet[k] = (loaded >> k) & 1; dk.packet_blocks_per_cu[k] = fit[k]; }
		dk.lane = get("lane_loaded", 1) != 0;
		dk.lane_listed = get("lane_listed_loaded", 1) != 0;
		dk.lane_blocks_per_cu = 5;

		TraceKnobs k;
		k.detect_image = (int)get("DETECT_IMAGE", k.detect_image);
		k.tile_blocks = (int)get("TILE_BLOCKS", k.tile_blocks);
		k.any_packets = (int)get("ANY_PACKETS", k.any_packets);
		k.qnodes = (int)get("QNODES", k.qnodes);
		k.packet_asm = (int)get("PACKET_ASM", k.packet_asm);
		k.packet_beam = (PacketKernel)(int)get("PACKET_BEAM", (int)k.packet_beam);
		k.lane_asm = (int)get("LANE_ASM", k.lane_asm);
		k.lane_lds = (size_t)get("LANE_LDS", (double)k.lane_lds);
		k.packet_entries = (int)get("PACKET_ENTRIES", k.packet_entries);
		k.hot_blocks_per_cu = (int)get("HOT_BLOCKS_PER_CU", k.hot_blocks_per_cu);

		const uint32_t look_w = (uint32_t)get("look_w", 0), look_h = (uint32_t)get("look_h", 0);
		const int occ = (int)get("occ", 4);
		if (!in.empty()) { std::cerr << "unknown key: " << in.begin()->first << "\n"; return 2; }

		const TracePlan p = plan_trace(rq, o, look_w, look_h, f, dk, k, occ);
		std::cout << "o_flags=" << o.flags << " o_image_w=" << o.image_w << " o_image_h=" << o.image_h << " o_refill_min=" << o.refill_min
			<< " o_refill_given=" << o.refill_given << " o_blocks_per_cu=" << o.blocks_per_cu << " o_node_exit=" << o.node_exit
			<< " look=" << wants_image_look(rq, o, f, k) << " variant_of=" << variant_of(rq, o, look_w, look_h, f, dk, k)
			<< " error=" << p.error << " dynamic=" << p.dynamic << " image_w=" << p.image_w << " image_h=" << p.image_h
			<< " tile_blocks=" << p.tile_blocks << " refill_min=" << p.refill_min << " node_exit=" << p.node_exit << " qn=" << p.qn
			<< " variant=" << p.variant << " packet=" << p.packet << " kernel=" << (int)p.kernel << " hot=" << p.hot << " lane_hot=" << p.lane_hot
			<< " entries=" << p.entries << " sort_rays=" << p.sort_rays << " grid=" << p.grid << " hot_grid=" << p.hot_grid
			<< " lane_grid=" << p.lane_grid << " lds_entries=" << p.lds_entries << " spill_cap=" << p.spill_cap << " spill_lanes=" << p.spill_lanes
			<< " has_message=" << (p.message != nullptr) << "\n";
	}
	return 0;
}
