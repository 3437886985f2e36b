// Driver of tests/test_residency_cpu.py: built by the host compiler against rtk_amd/csrc/rtk_residency.h alone (no HIP), with the
// address and undefined-behaviour sanitizers. "A device copy" is a malloc'ed dummy that carries a number (copies are numbered
// as they are made, from 0); blobs are malloc'ed at exactly their size, so a hash that reads past a blob's end is an error of
// the run. Every line of standard input is one command on the one cache there is; blobs are named by small numbers:
//   blob B SIZE SEED (a blob of SIZE bytes: byte i is (i * 131 + SEED * 31 + (i >> 8)) & 255, then size_in_bytes = SIZE in the header)
//   poke B OFFSET VALUE (one byte) | setsize B SIZE (the header's size_in_bytes alone; SIZE is at most what the blob was made with)
//   lookup B DEVICE | adopt B DEVICE (a new copy is made here and handed over) | forget B | each | fail 0/1 (uploads answer NULL)
//   unblob B (the blob's memory goes; forget it first) | leak (16 bytes nobody frees: the run must not end clean)
// The answer to each is one line: ret made freed events
//   ret: lookup: the copy's number, -1 = none; adopt: the new copy's number; each: how many copies were visited; else 0
//   made, freed: copies made and freed so far
//   events: what the command made the hooks do and (each) saw, in order: u(pload asked) fN (copy N freed) vN (copy N visited); "-" = nothing
#include "rtk_residency.h"

#include <stdlib.h>

#include <iostream>
#include <map>
#include <sstream>
#include <string>

struct rtk_dev_scene { long number; };

static bool g_fail = false;
static long g_made = 0, g_freed = 0;
static std::string g_events;
static rtk_dev_scene *make_copy()
{
	rtk_dev_scene *ds = static_cast<rtk_dev_scene *>(malloc(sizeof(rtk_dev_scene)));
	ds->number = g_made++;
	return ds;
}
static rtk_dev_scene *upload(const rtk_scene *) { g_events += 'u'; return g_fail ? nullptr : make_copy(); }
static void free_copy(rtk_dev_scene *ds) { g_events += 'f' + std::to_string(ds->number); g_freed++; free(ds); }

int main()
{
	Residency cache(upload, free_copy);
	std::map<long, unsigned char *> blobs;
	std::string line;
	while (std::getline(std::cin, line)) {
		std::istringstream in(line);
		std::string cmd;
		long b = 0;
		unsigned long long x = 0, y = 0;
		in >> cmd >> b >> x >> y;
		long long ret = 0;
		g_events.clear();
		rtk_scene *const scene = blobs.count(b) ? reinterpret_cast<rtk_scene *>(blobs[b]) : nullptr;
		if (cmd == "blob") {
			unsigned char *p = static_cast<unsigned char *>(malloc((size_t)x));
			for (size_t i = 0; i < (size_t)x; i++) p[i] = (unsigned char)((i * 131u + y * 31u + (i >> 8)) & 255u);
			blobs[b] = p;
			reinterpret_cast<rtk_scene *>(p)->size_in_bytes = x;
		}
		else if (cmd == "poke") blobs.at(b)[x] = (unsigned char)y;
		else if (cmd == "setsize") scene->size_in_bytes = x;
		else if (cmd == "lookup") { const rtk_dev_scene *ds = cache.lookup(scene, (int)x); ret = ds ? ds->number : -1; }
		else if (cmd == "adopt") { rtk_dev_scene *ds = make_copy(); ret = ds->number; cache.adopt(scene, (int)x, ds); }
		else if (cmd == "forget") cache.forget(scene);
		else if (cmd == "each") cache.for_each([&](rtk_dev_scene *ds) { ret++; g_events += 'v' + std::to_string(ds->number); });
		else if (cmd == "fail") g_fail = b != 0;
		else if (cmd == "unblob") { free(blobs.at(b)); blobs.erase(b); }
		else if (cmd == "leak") { void *volatile p = malloc(16); p = nullptr; (void)p; }
		else { std::cerr << "bad command: " << line << "\n"; return 2; }
		std::cout << ret << ' ' << g_made << ' ' << g_freed << ' ' << (g_events.empty() ? "-" : g_events) << "\n";
	}
	return 0;
}
