// rtk_world_internal.h -- internal: the world object and what every walk of a world shares (rtk_world.hip: rays;
// rtk_world_closest.hip: closest points; rtk_world_overlap.hip: the three overlap queries): the stack frame's constants, the refusals the host can see, and the launch on the
// (top tree, stream) scratch set.
#pragma once

#include "rtk_dev.h"

#include <mutex>
#include <vector>

#define WD_THREADS 256u
#define WD_WAVES (WD_THREADS / 64u)
#define WD_LDS_STACK 16u           // entries per lane held in LDS: 32 KB per workgroup
#define WD_REF_TOP 0xfffffffeu     // the sentinel: back to the top tree (never a leaf reference: a scene holds fewer than 2^30 slots)
#define WD_DEAD 1u                 // DevWorldInstance.flags

struct DevWorldScene {
	const DevNode *nodes;
	const DevTri *tris;
	uint32_t num_nodes, num_tris;
};
static_assert(sizeof(DevWorldScene) == 24, "one scene of a world's table");

struct rtk_dev_world {
	int device = 0;
	std::mutex mutex;                              // create, update, rebuild and info; a trace reads what they leave
	std::vector<rtk_dev_scene *> scenes;           // borrowed
	std::vector<DevWorldScene> scene_table;        // what d_scenes holds
	uint32_t deepest = 0;                          // the largest stack_entries among the scenes, as of the last update
	uint32_t num_instances = 0;
	rtk_dev_scene *top = nullptr;                  // owned
	SceneMem mem{ rtk_dev_malloc, rtk_dev_free };  // the four tables and the counter
	DevWorldInstance *d_inst = nullptr;            // [num_instances]
	rtk_placement *d_place = nullptr;              // [num_instances] as last given
	float *d_proxy = nullptr;                      // [9 * num_instances]
	DevWorldScene *d_scenes = nullptr;             // [num_scenes]
	unsigned long long *d_dead = nullptr;          // dead instances, counted by k_world_instances
	uint64_t dead = 0;
	double build_ms = 0.0, update_ms = 0.0;
};

// a push of the 8-byte entry e_ by a lane whose stack is stk / sp, with the kernel's parameters in p: LDS first, then the spill
// area; a push that fits neither is dropped WITHOUT advancing sp and flagged
#define WD_PUSH(e_)                                                                                                        \
	do {                                                                                                                   \
		if (sp < WD_LDS_STACK) { stk[sp][lane] = (e_); sp++; }                                                             \
		else if (sp - WD_LDS_STACK < p.spill_cap) { p.spill[(size_t)(sp - WD_LDS_STACK) * p.spill_stride + glane] = (e_); sp++; if (COUNT) c_spills++; } \
		else p.counter[RTK_ERROR_WORD] = 1ull;                                                                             \
	} while (0)

// everything about a query call on a world that the host can see, refused before any HIP call; have_io: neither the queries
// nor the output the form writes is NULL
static inline int rtk_world_refuse(const char *who, const char *what, const rtk_dev_world *w, size_t n, bool have_io, const rtk_ray_list *list,
	const rtk_world_filter *filter)
{
	if (!w || (n && !have_io)) { rtk_set_error("%s: NULL world, %s or output", who, what); return RTK_AMD_ERR_BAD_ARG; }
	if (list && (list->struct_size < sizeof(rtk_ray_list) || list->flags != 0u || !list->d_count)) {
		rtk_set_error("%s: bad list (struct_size %u, flags %#x, d_count %p)", who, list->struct_size, list->flags, (const void *)list->d_count);
		return RTK_AMD_ERR_BAD_ARG;
	}
	if (filter && (filter->struct_size < sizeof(rtk_world_filter) || filter->flags != 0u)) { rtk_set_error("%s: bad rtk_world_filter (struct_size %u, flags %#x)", who, filter->struct_size, filter->flags); return RTK_AMD_ERR_BAD_ARG; }
	if (filter && filter->d_instance_mask && filter->instance_mask_bits == 0) { rtk_set_error("%s: instance mask without instance_mask_bits", who); return RTK_AMD_ERR_BAD_ARG; }
	if (n >= ((size_t)1 << 32)) { rtk_set_error("%s: %zu %s: a batch holds fewer than 2^32", who, n, what); return RTK_AMD_ERR_BAD_ARG; }
	return RTK_AMD_OK;
}

// The launch of one walk of a world: `p` has the batch's own fields set; this fills what every walk takes from the world and from
// the scratch set of (top tree, stream) -- top_nodes .. top_num_tris, inst, scenes, num_instances, num_scenes, counter, spill,
// spill_stride, spill_cap -- lets `extra(top, p)` add what only that walk reads under the top tree's lock, and enqueues `kernel`
// on a resident grid, or, with `counted`, `counting` between a clear and a read of the visit counters (synchronises the stream).
// `from_scratch(sc, stream, p)` is the hook of a walk that needs more of the scratch set than the spill area and the counter (the
// overlap walk's claim bits): it runs once the set is fetched and the spill area is sized, under both locks, ahead of the launch
// on the same stream, and a result other than RTK_AMD_OK ends the call with it. The form without it is the one rays and closest
// points call.
template <class Params, class Extra, class FromScratch>
int rtk_world_launch(rtk_dev_world *w, size_t n, hipStream_t stream, int blocks_per_cu, void (*kernel)(Params), void (*counting)(Params), Params &p,
	Extra extra, FromScratch from_scratch, rtk_trace_counters *counted, const char *who)
{
	std::lock_guard<std::mutex> wlock(w->mutex);
	rtk_dev_scene *top = w->top;
	p.inst = w->d_inst; p.scenes = w->d_scenes;
	p.num_instances = w->num_instances; p.num_scenes = (uint32_t)w->scenes.size();
	const size_t blocks_needed = (n + WD_THREADS - 1u) / WD_THREADS;
	size_t grid = (size_t)(top->num_cus > 0 ? top->num_cus : 1) * (size_t)blocks_per_cu;
	if (grid > blocks_needed) grid = blocks_needed;

	// the scratch set of (top tree, stream), held until the launch is enqueued; the top tree's view and tree record are read under
	// the lock a rebuild replaces them under
	std::lock_guard<std::mutex> lock(top->scratch_mutex);
	p.top_nodes = top->view.nodes; p.top_tris = top->view.tris; p.top_num_nodes = top->view.num_nodes; p.top_num_tris = top->view.num_tris;
	extra(top, p);
	const size_t entries = (size_t)top->tree.stack_entries() + 1u + w->deepest;
	const size_t spill_cap = entries > WD_LDS_STACK ? entries - WD_LDS_STACK : 0;
	LaunchScratch *sc = top->scratch.get(stream);
	if (!sc) return RTK_AMD_ERR_OOM;
	if (spill_cap) {
		const int rc = sc->grow_spill(grid * WD_THREADS, spill_cap, sizeof(uint2));
		if (rc != RTK_AMD_OK) return rc;
	}
	p.spill = sc->spill.as<uint2>();
	p.spill_stride = (uint32_t)(spill_cap ? sc->spill.capacity : 0);
	p.spill_cap = (uint32_t)spill_cap;
	p.counter = sc->d_counter;
	{
		const int rc = from_scratch(sc, stream, p);
		if (rc != RTK_AMD_OK) return rc;
	}
	if (!counted) {
		hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(WD_THREADS), 0, stream, p);
		RTK_HIP_CHECK(hipGetLastError(), RTK_AMD_ERR_HIP);
		return RTK_AMD_OK;
	}
	// the counting form: the visit counters start from zero, are brought home and the stream is waited for
	unsigned long long c[8], err = 0;
	RTK_HIP_CHECK(hipMemsetAsync(sc->d_counter, 0, RTK_COUNTER_WORDS * sizeof(unsigned long long), stream), RTK_AMD_ERR_HIP);
	hipLaunchKernelGGL(counting, dim3((unsigned)grid), dim3(WD_THREADS), 0, stream, p);
	RTK_HIP_CHECK(hipGetLastError(), RTK_AMD_ERR_HIP);
	RTK_HIP_CHECK(hipMemcpyAsync(c, sc->d_counter, sizeof(c), hipMemcpyDeviceToHost, stream), RTK_AMD_ERR_HIP);
	RTK_HIP_CHECK(hipMemcpyAsync(&err, sc->d_counter + RTK_ERROR_WORD, sizeof(err), hipMemcpyDeviceToHost, stream), RTK_AMD_ERR_HIP);
	RTK_HIP_CHECK(hipStreamSynchronize(stream), RTK_AMD_ERR_HIP);
	counted->rays = c[1]; counted->nodes = c[2]; counted->leaves = c[3]; counted->triangles = c[4]; counted->hits = c[5]; counted->stack_spills = c[6];
	if (err) {
		(void)hipMemsetAsync(sc->d_counter + RTK_ERROR_WORD, 0, sizeof(err), stream);
		rtk_set_error("%s: traversal stack overflow (corrupted scene)", who);
		return RTK_AMD_ERR_BAD_SCENE;
	}
	return RTK_AMD_OK;
}

// ... without a hook: the spill area and the counter are all the walk takes from the scratch set
template <class Params, class Extra>
int rtk_world_launch(rtk_dev_world *w, size_t n, hipStream_t stream, int blocks_per_cu, void (*kernel)(Params), void (*counting)(Params), Params &p,
	Extra extra, rtk_trace_counters *counted, const char *who)
{
	return rtk_world_launch(w, n, stream, blocks_per_cu, kernel, counting, p, extra, [](LaunchScratch *, hipStream_t, Params &) { return (int)RTK_AMD_OK; }, counted, who);
}
