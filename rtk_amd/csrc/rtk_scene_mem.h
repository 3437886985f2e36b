// rtk_scene_mem.h -- internal, host only (no HIP): the ledger of the device allocations one scene owns.
//
// Every allocation that lives as long as the scene, or until the call that replaces it, is recorded here with the number of
// bytes it adds to rtk_dev_scene_info.total_device_bytes. The two sizes are separate arguments because the sites never agreed
// on what to count, and the reported figure is part of what callers see: it stays as it was, site by site.
//
//   who                                         allocates                             counts
//   upload_vec (rtk_upload.hip), six arrays     max(elements, 1) * sizeof(T)          the same
//   rtk_scene_consts (rtk_quant.hip)            sizeof(DevSceneConsts)                0
//   rtk_quantize_nodes, an upload's qnodes      max(num_nodes, 1) * 64                num_nodes * 64
//   Build::dev_alloc (rtk_build_internal.h)     bytes, 16 if that is 0                bytes
//   the build's node block                      node_cap * (128 + 64)                 the same (the capacity, not num_nodes)
//   rtk_scene_side_arrays (rtk_build_refit.hip) four arrays, one Carve                the same (Carve::bytes: padded)
//   make_schedule (rtk_refit.hip), d_order      num_nodes * 4                         the same
//   make_schedule, level starts + mesh table    padded starts + max(meshes, 1) * 24   starts * 4 + meshes * 24 (unpadded)
//   make_partial_tables (rtk_refit.hip)         eight tables, one Carve               Carve::counted: the tables' unpadded sum
//   make_buffers (rtk_quality.hip)              records + result slot                 the same
//   rtk_dev_scene_split_leaves, node block      new nodes * (128 + 64)                the same
//   rtk_dev_scene_rebuild                       a build's entries (Build::dev_alloc,  the same: they change ledgers as they are
//                                               the node block, the constants)        (adopt_all), the old ones are released
//   rtk_dev_scene_rebuild of a blob, d_vidx_in  num_tris * 12, by Build::dev_alloc    the same
//   rtk_scene_pseudonormals (rtk_sign.hip)      max(num_prims, 1) * 72                num_prims * 72
//   rtk_scene_winding_table (rtk_winding.hip)   max(num_nodes, 1) * 128               num_nodes * 128
//   rtk_dev_world_create (rtk_world.hip), in    instances * (64 + 48 + 36), scenes    the same
//   the WORLD's ledger, not a scene's           * 24, one 8-byte counter
//
// The allocator and its free are the owner's (hipMalloc / hipFree for a scene, malloc / free for tests/scene_mem_driver.cpp).
// One lock of its own: the side arrays arrive under another mutex of the scene than the tables of a refit or a measurement.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <mutex>
#include <vector>

class SceneMem {
public:
	typedef void *(*AllocFn)(size_t bytes);    // NULL: out of memory
	typedef void (*FreeFn)(void *p);
	SceneMem(AllocFn alloc, FreeFn free) : alloc_(alloc), free_(free) {}
	~SceneMem() { release_all(); }             // (not copyable: the lock is not)

	// allocates and records; NULL (and nothing recorded) if the allocator fails
	void *own(size_t alloc_bytes, size_t counted_bytes)
	{
		void *p = alloc_(alloc_bytes);
		if (p) adopt(p, counted_bytes);
		return p;
	}
	// memory of the same allocator that was made elsewhere
	void adopt(void *p, size_t counted_bytes)
	{
		std::lock_guard<std::mutex> lock(mutex_);
		entries_.push_back(Entry{ p, counted_bytes });
	}
	// every entry of `from` (same allocator) becomes an entry of this ledger, counted as it was; `from` is left empty
	void adopt_all(SceneMem &from)
	{
		std::vector<Entry> moved;
		{
			std::lock_guard<std::mutex> lock(from.mutex_);
			moved.swap(from.entries_);
		}
		std::lock_guard<std::mutex> lock(mutex_);
		entries_.insert(entries_.end(), moved.begin(), moved.end());
	}
	// frees and forgets one entry; false (and nothing freed) for NULL or a pointer that is not an entry's
	bool release(const void *p)
	{
		std::lock_guard<std::mutex> lock(mutex_);
		for (size_t i = 0; p && i < entries_.size(); i++) {
			if (entries_[i].p != p) continue;
			free_(entries_[i].p);
			entries_.erase(entries_.begin() + i);
			return true;
		}
		return false;
	}
	void release_all()
	{
		std::lock_guard<std::mutex> lock(mutex_);
		for (const Entry &e : entries_) free_(e.p);
		entries_.clear();
	}
	// what the live entries add to total_device_bytes
	uint64_t counted() const
	{
		std::lock_guard<std::mutex> lock(mutex_);
		uint64_t sum = 0;
		for (const Entry &e : entries_) sum += e.counted;
		return sum;
	}

private:
	struct Entry { void *p; size_t counted; };
	AllocFn alloc_;
	FreeFn free_;
	mutable std::mutex mutex_;
	std::vector<Entry> entries_;
};
