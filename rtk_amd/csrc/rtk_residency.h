// rtk_residency.h -- internal, host only (no HIP): which device scene is the copy of which blob, for the host-pointer calls.
//
// Host-pointer calls (rtk_trace_ray[s], the reference's own signatures) find the device copy of a blob through its
// address and the calling thread's current device. The address alone is not an identity: rtk_finish_build_to writes
// into caller memory that the caller releases with free(), so a different blob can later live at the same address.
//   * Every way this library itself puts a blob at an address (rtk_finish_build[_to] with either builder, rtk_free_scene)
//     drops or replaces the entry.
//   * When a blob is uploaded, EVERY 4 KB stripe of it is hashed (one pass, ~1 ns per 8 bytes). A lookup re-checks the
//     header and the root node (a different scene of another size or shape is caught at once) plus ONE stripe, a
//     different one each time, in rotation: a caller that rewrites a blob in place behind the library's back -- one moved
//     vertex -- is found out within (size / 4 KB) lookups instead of never, at ~0.2 us per call instead of a re-hash of
//     up to 100 MB. rtk_amd_forget_scene is the immediate, documented way (include/rtk_amd.h).
//
// Making a device copy and freeing one are the owner's (an upload with its reasons to fail and rtk_dev_scene_free,
// rtk_host_calls.hip; malloc / free of a counting dummy for tests/residency_driver.cpp). One lock of its own, held over both.
#pragma once

#include "rtk.h"

#include <string.h>

#include <algorithm>
#include <functional>
#include <mutex>
#include <unordered_map>
#include <vector>

struct rtk_dev_scene;

#pragma GCC visibility push(hidden)      // (nothing here is part of the library's interface, nor what the standard templates make of it)

const size_t RESIDENCY_STRIPE = 4096;

inline uint64_t hash_words(const void *data, size_t n, uint64_t h)
{
	const unsigned char *p = static_cast<const unsigned char *>(data);
	size_t i = 0;
	for (; i + 8 <= n; i += 8) { uint64_t w; memcpy(&w, p + i, 8); h = (h ^ w) * 0x9e3779b97f4a7c15ull; h ^= h >> 29; }
	for (; i < n; i++) { h = (h ^ p[i]) * 0x100000001b3ull; }
	return h;
}

// a blob with a root node: one that has stripes (a size beyond 2^48 is no blob's: nothing past the header is read)
inline bool has_root(uint64_t size) { return size >= 256 && size <= ((uint64_t)1 << 48); }

inline uint64_t head_hash(const rtk_scene *scene)
{
	uint64_t h = hash_words(scene, sizeof(rtk_scene), 0xcbf29ce484222325ull);
	if (has_root(scene->size_in_bytes)) h = hash_words(reinterpret_cast<const char *>(scene) + 128, 128, h);   // root node
	return h;
}

// stripe k of a blob of `size` bytes, seeded with where it begins
inline uint64_t stripe_hash(const rtk_scene *scene, uint64_t size, size_t k)
{
	const uint64_t at = (uint64_t)k * RESIDENCY_STRIPE;
	return hash_words(reinterpret_cast<const char *>(scene) + at, (size_t)std::min<uint64_t>(RESIDENCY_STRIPE, size - at), at);
}

struct ResidencyEntry {
	rtk_dev_scene *ds = nullptr;
	uint64_t size = 0, head = 0;
	std::vector<uint64_t> stripes;     // hash of every RESIDENCY_STRIPE bytes of the blob as it was uploaded
	size_t next = 0;                   // the stripe the next lookup re-checks
};
struct ResidencyKey {
	const rtk_scene *scene; int device;
	bool operator==(const ResidencyKey &o) const { return scene == o.scene && device == o.device; }
};
struct ResidencyKeyHash { size_t operator()(const ResidencyKey &k) const { return std::hash<const void *>()(k.scene) ^ ((size_t)k.device * 0x9e3779b97f4a7c15ull); } };

class Residency {
public:
	typedef rtk_dev_scene *(*UploadFn)(const rtk_scene *scene);   // a device copy of the blob on the calling thread's device; NULL: the hook has said why
	typedef void (*FreeFn)(rtk_dev_scene *ds);
	Residency(UploadFn upload, FreeFn free) : upload_(upload), free_(free) {}

	// the device copy of the blob at `scene` on `device`, uploaded if there is none or another blob lives at this address now
	rtk_dev_scene *lookup(const rtk_scene *scene, int device)
	{
		const ResidencyKey key = { scene, device };
		std::lock_guard<std::mutex> lock(mutex_);
		auto it = map_.find(key);
		if (it != map_.end()) {
			ResidencyEntry &e = it->second;
			bool same = e.size == scene->size_in_bytes && e.head == head_hash(scene);
			if (same && !e.stripes.empty()) {
				const size_t k = e.next;
				e.next = (k + 1) % e.stripes.size();
				same = stripe_hash(scene, e.size, k) == e.stripes[k];
			}
			if (same) return e.ds;
			free_(e.ds);
			map_.erase(it);
		}
		rtk_dev_scene *ds = upload_(scene);
		if (ds) fill(map_[key], scene, ds);
		return ds;
	}
	// `ds` was made from the blob elsewhere: nothing that lived at this address before is valid any more, on any device
	void adopt(const rtk_scene *scene, int device, rtk_dev_scene *ds)
	{
		std::lock_guard<std::mutex> lock(mutex_);
		drop_address(scene);
		fill(map_[ResidencyKey{ scene, device }], scene, ds);
	}
	void forget(const rtk_scene *scene) { std::lock_guard<std::mutex> lock(mutex_); drop_address(scene); }
	// fn(ds) of every device copy there is, under the lock
	template <class Fn> void for_each(Fn fn) { std::lock_guard<std::mutex> lock(mutex_); for (auto &kv : map_) fn(kv.second.ds); }

private:
	void drop_address(const rtk_scene *scene)
	{
		for (auto it = map_.begin(); it != map_.end();) {
			if (it->first.scene == scene) { free_(it->second.ds); it = map_.erase(it); } else ++it;
		}
	}
	static void fill(ResidencyEntry &e, const rtk_scene *scene, rtk_dev_scene *ds)
	{
		e.ds = ds;
		e.size = scene->size_in_bytes;
		e.head = head_hash(scene);
		e.next = 0;
		e.stripes.clear();
		if (has_root(e.size)) for (size_t k = 0; (uint64_t)k * RESIDENCY_STRIPE < e.size; k++) e.stripes.push_back(stripe_hash(scene, e.size, k));
	}
	const UploadFn upload_;
	const FreeFn free_;
	std::mutex mutex_;
	std::unordered_map<ResidencyKey, ResidencyEntry, ResidencyKeyHash> map_;
};

#pragma GCC visibility pop
