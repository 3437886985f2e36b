// Driver of tests/test_launch_scratch_cpu.py: built by the host compiler against rtk_amd/csrc/rtk_launch_scratch.h alone (no HIP), with
// the address and undefined-behaviour sanitizers; the allocator is malloc / free, "wait for the stream" counts. Every line of
// standard input is one command on the one collection there is; streams are small numbers, buffers are named:
//   new (the collection goes away and a fresh one comes) | fail 0/1 (the allocator answers NULL) | get S | find S | drop S
//   grow S sort|entries|leftover|select NEED BYTES | spill S LANES ENTRIES | verdict S (the set gets a pinned verdict)
//   leak (16 bytes nobody frees: the run must not end clean)
// The answer to each is one line: ret nonnull capacity entries events allocs frees waits pinned_frees
//   ret: get / find: the set's number (sets are numbered as they are made), -1 = none; grow / spill: the code; else 0
//   nonnull capacity entries: of the buffer a grow / spill named (entries: the spill's second measure), else 0 0 0
//   events: what the command made the hooks do, in order: w(ait) f(ree) a(lloc) c(ounter) p(inned free); "-" = nothing
#include "rtk_launch_scratch.h"

#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <map>
#include <memory>
#include <sstream>
#include <string>

static bool g_fail = false;
static long g_allocs = 0, g_frees = 0, g_waits = 0, g_pinned_frees = 0;
static std::string g_events;
static void *counting_alloc(size_t bytes)
{
	g_allocs++; g_events += 'a';
	void *p = g_fail ? nullptr : malloc(bytes ? bytes : 1);
	if (p) memset(p, 0xab, bytes);             // (the whole of what was asked for is there)
	return p;
}
static void counting_free(void *p) { g_frees++; g_events += 'f'; free(p); }
static void pinned_free(void *p) { g_pinned_frees++; g_events += 'p'; free(p); }
static int counting_wait(void *) { g_waits++; g_events += 'w'; return RTK_AMD_OK; }
static unsigned long long *counter_words(void *)
{
	g_events += 'c';
	return g_fail ? nullptr : static_cast<unsigned long long *>(malloc(64));
}
static const ScratchHooks g_hooks = { counting_alloc, counting_free, counting_wait, counter_words, pinned_free };

int main()
{
	std::unique_ptr<ScratchSets> sets(new ScratchSets(g_hooks));
	std::map<const LaunchScratch *, long> number;
	long made = 0;
	std::string line;
	while (std::getline(std::cin, line)) {
		std::istringstream in(line);
		std::string cmd, name;
		unsigned long long s = 0, a = 0, b = 0;
		in >> cmd;
		long long ret = 0;
		const ScratchBuf *named = nullptr;
		size_t entries = 0;
		g_events.clear();
		void *const stream = (in >> s, reinterpret_cast<void *>((uintptr_t)s * 8u));
		if (cmd == "new") { sets.reset(); sets.reset(new ScratchSets(g_hooks)); number.clear(); }
		else if (cmd == "fail") g_fail = s != 0;
		else if (cmd == "get") {
			LaunchScratch *sc = sets->get(stream);
			if (sc && !number.count(sc)) number[sc] = made++;
			ret = sc ? number.at(sc) : -1;
		}
		else if (cmd == "find") { const LaunchScratch *sc = sets->find(stream); ret = sc ? number.at(sc) : -1; }
		else if (cmd == "drop") { if (const LaunchScratch *sc = sets->find(stream)) number.erase(sc); sets->drop(stream); }
		else if (cmd == "verdict") { LaunchScratch *sc = sets->find(stream); sc->h_verdict = static_cast<uint32_t *>(malloc(64)); }
		else if (cmd == "grow") {
			in >> name >> a >> b;
			LaunchScratch *sc = sets->find(stream);
			ScratchBuf &buf = name == "sort" ? sc->sort : name == "entries" ? sc->entries : name == "leftover" ? sc->leftover : sc->select;
			if (name != "sort" && name != "entries" && name != "leftover" && name != "select") { std::cerr << "bad buffer: " << line << "\n"; return 2; }
			ret = sc->grow(buf, (size_t)a, (size_t)b);
			named = &buf;
		}
		else if (cmd == "spill") {
			in >> a >> b;
			LaunchScratch *sc = sets->find(stream);
			ret = sc->grow_spill((size_t)a, (size_t)b, 8);
			named = &sc->spill;
			entries = sc->spill_entries_per_lane;
		}
		else if (cmd == "leak") { void *volatile p = malloc(16); p = nullptr; (void)p; }
		else { std::cerr << "bad command: " << line << "\n"; return 2; }
		std::cout << ret << ' ' << (named && named->p ? 1 : 0) << ' ' << (named ? named->capacity : 0) << ' ' << entries << ' '
			<< (g_events.empty() ? "-" : g_events) << ' ' << g_allocs << ' ' << g_frees << ' ' << g_waits << ' ' << g_pinned_frees << "\n";
	}
	return 0;
}
