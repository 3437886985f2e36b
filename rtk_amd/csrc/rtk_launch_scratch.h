// rtk_launch_scratch.h -- internal, host only (no HIP): the device memory a launch writes besides its outputs, and who owns it.
//
// One set per (scene, stream): work-queue heads and visit counters, the global part of the traversal stacks, the ray-reordering
// buffers, the packet kernels' entry lists and hand-over list, the masks of rtk_dev_select_rays. Launches on one stream are
// ordered by the stream, launches on different streams (or from different host threads) never share a set, so tracing one scene
// from many threads is safe (the reference's rtk_trace_ray is a pure function of a const scene, rtk.c:543-577).
//
// The allocator, its free and "wait for the stream" are the owner's (hipMalloc / hipFree / hipStreamSynchronize for a scene,
// rtk_launch.hip; malloc / free and a counter for tests/launch_scratch_driver.cpp). No lock of its own: the scene's scratch_mutex
// is held by whoever touches the collection or a set, until everything that uses the set is enqueued.
#pragma once

#include "rtk_amd.h"

#include <stddef.h>
#include <stdint.h>
#include <vector>

struct ScratchHooks {
	void *(*alloc)(size_t bytes);              // NULL: out of memory (the hook has said why)
	void (*free)(void *p);
	int (*wait)(void *stream);                 // RTK_AMD_OK once everything enqueued on the stream has completed, or the error's code
	unsigned long long *(*counter)(void *stream);   // the counter words of a new set, cleared on its stream; NULL: out of memory
	void (*free_pinned)(void *p);              // the verdict (its user makes it)
};

// One buffer, grown on demand. `capacity` is in its user's unit (rays, blocks, bytes); `bytes` is what `need` units take.
struct ScratchBuf {
	void *p = nullptr;
	size_t capacity = 0;
	int grow(size_t need, size_t bytes, void *stream, const ScratchHooks &h)
	{
		if (capacity >= need) return RTK_AMD_OK;
		// an earlier launch on this stream may still be using the old area
		if (p) { const int rc = h.wait(stream); if (rc != RTK_AMD_OK) return rc; h.free(p); }
		capacity = 0;
		p = h.alloc(bytes);
		if (!p) return RTK_AMD_ERR_OOM;
		capacity = need;
		return RTK_AMD_OK;
	}
	template <class T> T *as() const { return static_cast<T *>(p); }
};

struct LaunchScratch {
	enum { SPILL, SORT, ENTRIES, LEFTOVER, SELECT, SIGNED, NUM_BUFFERS };
	void *const stream;
	const ScratchHooks &hooks;
	unsigned long long *d_counter = nullptr;    // RTK_COUNTER_WORDS, the error word, the image look's words (rtk_dev.h)
	volatile uint32_t *h_verdict = nullptr;     // pinned: where k_detect_check leaves (width, height) of an image nobody announced
	ScratchBuf buf[NUM_BUFFERS];                // what free_all() walks: a buffer is a name here and a reference below, nothing else
	ScratchBuf &spill = buf[SPILL];             // uint2 [entry][lane]; capacity: lanes, and spill_entries_per_lane beside it
	ScratchBuf &sort = buf[SORT];               // ray reordering (RTK_TRACE_SORT_RAYS); capacity: rays
	ScratchBuf &entries = buf[ENTRIES];         // packet kernels: entry lists of the image's 64x64-pixel blocks (PkBlockEntries); capacity: blocks
	ScratchBuf &leftover = buf[LEFTOVER];       // tiles the assembly packet kernel hands to the C++ one, or rays the assembly per-lane kernel hands to rtk_trace_kernel; capacity: bytes
	ScratchBuf &select = buf[SELECT];           // rtk_dev_select_rays: keep masks, per-workgroup counts and their sums (rtk_select.hip); capacity: bytes
	ScratchBuf &signed_records = buf[SIGNED];   // rtk_dev_signed_distances without d_records: the closest walk's records (rtk_sign.hip); capacity: queries
	size_t spill_entries_per_lane = 0;

	LaunchScratch(void *stream_, const ScratchHooks &hooks_) : stream(stream_), hooks(hooks_) {}
	LaunchScratch(const LaunchScratch &) = delete;
	~LaunchScratch()
	{
		if (d_counter) hooks.free(d_counter);
		if (h_verdict) hooks.free_pinned((void *)h_verdict);
		for (ScratchBuf &b : buf) if (b.p) hooks.free(b.p);
	}
	int grow(ScratchBuf &b, size_t need, size_t bytes) { return b.grow(need, bytes, stream, hooks); }
	// two measures: made anew when either is short
	int grow_spill(size_t lanes, size_t entries_per_lane, size_t entry_bytes)
	{
		if (spill.capacity >= lanes && spill_entries_per_lane >= entries_per_lane) return RTK_AMD_OK;
		spill.capacity = spill_entries_per_lane = 0;
		const int rc = grow(spill, lanes, lanes * entries_per_lane * entry_bytes);
		if (rc == RTK_AMD_OK) spill_entries_per_lane = entries_per_lane;
		return rc;
	}
};

// The sets of one scene, by stream.
class ScratchSets {
public:
	explicit ScratchSets(const ScratchHooks &hooks) : hooks_(hooks) {}
	ScratchSets(const ScratchSets &) = delete;
	~ScratchSets() { for (LaunchScratch *s : sets_) delete s; }
	LaunchScratch *find(void *stream) const
	{
		for (LaunchScratch *s : sets_) if (s->stream == stream) return s;
		return nullptr;
	}
	// ... made on first use; NULL (and nothing entered) if its counter words cannot be had
	LaunchScratch *get(void *stream)
	{
		if (LaunchScratch *s = find(stream)) return s;
		unsigned long long *counter = hooks_.counter(stream);
		if (!counter) return nullptr;
		LaunchScratch *s = new LaunchScratch(stream, hooks_);
		s->d_counter = counter;
		sets_.push_back(s);
		return s;
	}
	// the stream is going away: a recycled handle must never find the old set
	void drop(void *stream)
	{
		for (size_t i = 0; i < sets_.size();) {
			if (sets_[i]->stream == stream) { delete sets_[i]; sets_.erase(sets_.begin() + (long)i); } else i++;
		}
	}

private:
	const ScratchHooks hooks_;
	std::vector<LaunchScratch *> sets_;
};
