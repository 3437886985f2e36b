// Driver of tests/test_scene_mem_cpu.py: built by the host compiler against rtk_amd/csrc/rtk_scene_mem.h alone (no HIP), with
// the address and undefined-behaviour sanitizers; the allocator is malloc / free. Every line of standard input is one command
// on the one ledger there is; pointers are named by the number of the command that made them (0, 1, ...: own, adopt, foreign):
//   new | fail 0/1 (the allocator answers NULL) | own ALLOC COUNTED | adopt ALLOC COUNTED | foreign (memory the ledger never sees)
//   release NUMBER | release null | release_all | counted | leak (16 bytes nobody frees: the run must not end clean)
// The answer to each is one line: ret counted allocs frees (ret: own / adopt / foreign: the pointer's number, -1 = NULL;
// release: 1 / 0; else 0; allocs and frees: calls of the ledger's two functions so far).
#include "rtk_scene_mem.h"

#include <stdlib.h>

#include <iostream>
#include <memory>
#include <sstream>
#include <string>

static bool g_fail = false;
static long g_allocs = 0, g_frees = 0;
static void *counting_alloc(size_t bytes) { g_allocs++; return g_fail ? nullptr : malloc(bytes ? bytes : 1); }
static void counting_free(void *p) { g_frees++; free(p); }

int main()
{
	std::unique_ptr<SceneMem> mem(new SceneMem(counting_alloc, counting_free));
	std::vector<void *> made, foreign;
	std::string line;
	while (std::getline(std::cin, line)) {
		std::istringstream in(line);
		std::string cmd, arg;
		unsigned long long a = 0, c = 0;
		in >> cmd;
		long long ret = 0;
		if (cmd == "new") { mem.reset(new SceneMem(counting_alloc, counting_free)); made.clear(); }
		else if (cmd == "fail") { in >> a; g_fail = a != 0; }
		else if (cmd == "own") { in >> a >> c; void *p = mem->own((size_t)a, (size_t)c); made.push_back(p); ret = p ? (long long)made.size() - 1 : -1; }
		else if (cmd == "adopt") { in >> a >> c; void *p = malloc((size_t)a); mem->adopt(p, (size_t)c); made.push_back(p); ret = (long long)made.size() - 1; }
		else if (cmd == "foreign") { void *p = malloc(16); foreign.push_back(p); made.push_back(p); ret = (long long)made.size() - 1; }
		else if (cmd == "release") { in >> arg; ret = mem->release(arg == "null" ? nullptr : made.at(std::stoul(arg))) ? 1 : 0; }
		else if (cmd == "release_all") mem->release_all();
		else if (cmd == "leak") { void *volatile p = malloc(16); p = nullptr; (void)p; }
		else if (cmd != "counted") { std::cerr << "bad command: " << line << "\n"; return 2; }
		std::cout << ret << ' ' << mem->counted() << ' ' << g_allocs << ' ' << g_frees << "\n";
	}
	for (void *p : foreign) free(p);
	return 0;
}
