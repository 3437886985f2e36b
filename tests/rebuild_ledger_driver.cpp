// Driver of tests/test_rebuild_cpu.py: SceneMem::adopt_all (rtk_amd/csrc/rtk_scene_mem.h), the step by which the allocations of
// a rebuilt tree change from the new scene object's ledger to the live scene's. Built by the host compiler against that
// header alone, with malloc / free as the allocator, and run under the address and undefined-behaviour sanitizers.
#include "rtk_scene_mem.h"

#include <stdio.h>
#include <stdlib.h>

static int g_allocs = 0, g_frees = 0;
static void *count_alloc(size_t bytes) { g_allocs++; return malloc(bytes ? bytes : 1); }
static void count_free(void *p) { g_frees++; free(p); }

#define CHECK(cond) do { if (!(cond)) { printf("FAIL line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main()
{
	{
		SceneMem live(count_alloc, count_free), fresh(count_alloc, count_free);
		void *old_tris = live.own(480, 480), *kept = live.own(120, 120);
		void *new_tris = fresh.own(512, 480), *consts = fresh.own(16, 0), *nodes = fresh.own(1920, 1920);
		CHECK(old_tris && kept && new_tris && consts && nodes);
		CHECK(live.counted() == 600 && fresh.counted() == 2400);
		// the swap of a rebuild: the old array goes, the new scene's entries arrive as they are counted
		CHECK(live.release(old_tris));
		live.adopt_all(fresh);
		CHECK(fresh.counted() == 0 && live.counted() == 120 + 2400);
		CHECK(!fresh.release(new_tris));               // the giver no longer knows them ...
		CHECK(g_frees == 1);
		CHECK(live.release(consts) && live.counted() == 2520);     // ... the receiver does (counted 0: the constants block)
		CHECK(live.release(new_tris) && live.counted() == 2040);
		CHECK(g_frees == 3);
		// from an empty ledger, and into one: nothing happens, nothing is lost
		live.adopt_all(fresh);
		CHECK(live.counted() == 2040);
		SceneMem empty(count_alloc, count_free);
		empty.adopt_all(live);
		CHECK(live.counted() == 0 && empty.counted() == 2040);
		fresh.release_all();
		live.release_all();
		CHECK(g_frees == 3);
		// (what `empty` holds -- kept, nodes -- is freed by its destructor)
	}
	CHECK(g_allocs == 5 && g_frees == 5);
	printf("ok\n");
	return 0;
}
