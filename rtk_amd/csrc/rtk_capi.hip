// rtk_capi.hip -- the thin part of librtk_amd.so's C ABI: errors and device selection, a device scene's upload, release and
// figures, and the rtk_dev_* batch calls of rtk_amd.h, which are argument checks and a TraceCall. The calls that take host
// pointers (rtk_trace_ray[s], the residency cache) are rtk_host_calls.hip, the build's rtk_build_api.hip. No intersection
// arithmetic lives here and there is no CPU fallback: every trace call runs the HIP kernels behind rtk_launch.hip or fails
// with an error.
#include "rtk_dev.h"
#include "rtk_layout_check.h"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

// ---------------------------------------------------------------------------- errors

static thread_local char g_error[512] = "";

void rtk_set_error(const char *fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_error, sizeof(g_error), fmt, ap);
	va_end(ap);
}

extern "C" const char *rtk_amd_last_error(void) { return g_error; }


extern "C" int rtk_amd_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) { rtk_set_error("hipGetDeviceCount failed: no HIP device or driver"); return 0; }
	return n;
}

extern "C" int rtk_amd_set_device(int device)
{
	RTK_HIP_CHECK(hipSetDevice(device), RTK_AMD_ERR_NO_DEVICE);
	return RTK_AMD_OK;
}

// ---------------------------------------------------------------------------- scenes

extern "C" rtk_dev_scene *rtk_dev_scene_upload(const rtk_scene *scene)
{
	HostBvh h;
	if (rtk_blob_to_host_bvh(scene, scene ? (size_t)scene->size_in_bytes : 0, &h) != RTK_AMD_OK) return nullptr;
	return rtk_dev_scene_from_host_bvh(h);
}

extern "C" rtk_dev_scene *rtk_dev_scene_upload_buffer(const void *blob, size_t blob_bytes)
{
	HostBvh h;
	if (!blob || blob_bytes < sizeof(rtk_scene)) { rtk_set_error("scene blob: buffer smaller than the header"); return nullptr; }
	if (rtk_blob_to_host_bvh(static_cast<const rtk_scene *>(blob), blob_bytes, &h) != RTK_AMD_OK) return nullptr;
	return rtk_dev_scene_from_host_bvh(h);
}

void rtk_scene_forget_derived(rtk_dev_scene *ds, unsigned what)
{
	rtk_export_forget(ds);
	if (what & (RTK_FORGET_BOXES | RTK_FORGET_TREE | RTK_FORGET_SLOTS)) {
		// (the winding moments are made from positions and go by node: whatever moved or was renumbered, the next winding query
		// makes them again. A rebuild is here with scratch_mutex held: that lock comes before this one everywhere, rtk_winding.hip)
		std::lock_guard<std::mutex> lock(ds->winding_mutex);
		ds->mem.release(ds->winding.d_table);
		ds->winding = WindingTable();
	}
	if (what & RTK_FORGET_BOXES) {
		ds->quality.refitted = true;
		// (vertices moved: the pseudonormals are made from positions; the next signed query makes them again)
		std::lock_guard<std::mutex> lock(ds->sign_mutex);
		ds->mem.release(ds->sign.d_table);
		ds->sign = SignTable();
	}
	if (what & RTK_FORGET_TREE) {
		ds->refit.reset(ds->mem);
		ds->partial.reset(ds->mem);
		ds->quality.baseline_known = false;
		ds->quality.sah_cost_at_build = 0.0;
	}
	if (what & RTK_FORGET_SLOTS) {
		// (a device build made the four as one allocation that begins with the vertex indices, an upload one by one)
		ds->mem.release(ds->view.vertex_index);
		ds->mem.release(ds->view.prim_slot);
		ds->mem.release(ds->view.slot_mesh);
		ds->mem.release(ds->view.slot_tri);
		ds->view.vertex_index = ds->view.prim_slot = ds->view.slot_mesh = ds->view.slot_tri = nullptr;
		ds->side_ready = false;
	}
}

extern "C" void rtk_dev_scene_free(rtk_dev_scene *ds)
{
	if (!ds) return;
	rtk_scene_forget_derived(ds, RTK_FORGET_BOXES | RTK_FORGET_TREE);
	ds->mem.release_all();
	delete ds;                         // (with its launch scratch: ScratchSets)
}

extern "C" int rtk_dev_scene_get_info(const rtk_dev_scene *ds, rtk_dev_scene_info *info)
{
	if (!ds || !info) { rtk_set_error("rtk_dev_scene_get_info: NULL argument"); return RTK_AMD_ERR_BAD_ARG; }
	info->num_triangles = ds->view.num_tris;
	info->num_meshes = ds->mesh_base.empty() ? 0 : ds->mesh_base.size() - 1;
	info->num_nodes = ds->view.num_nodes;
	info->node_bytes = (uint64_t)ds->view.num_nodes * sizeof(DevNode);
	info->triangle_bytes = (uint64_t)ds->view.num_tris * sizeof(DevTri);
	info->total_device_bytes = ds->mem.counted();
	info->max_depth = ds->tree.max_depth;
	info->stack_entries = ds->tree.stack_entries();
	info->build_ms = ds->build_ms;
	return RTK_AMD_OK;
}

extern "C" int rtk_dev_scene_mesh_base(const rtk_dev_scene *ds, uint64_t *out, size_t capacity)
{
	if (!ds || !out || capacity < ds->mesh_base.size()) { rtk_set_error("rtk_dev_scene_mesh_base: bad argument"); return RTK_AMD_ERR_BAD_ARG; }
	memcpy(out, ds->mesh_base.data(), ds->mesh_base.size() * sizeof(uint64_t));
	return (int)ds->mesh_base.size();
}

extern "C" long long rtk_dev_scene_primitive_order(const rtk_dev_scene *ds, uint32_t *out, size_t capacity)
{
	if (!ds || !out || capacity < ds->view.num_tris) { rtk_set_error("rtk_dev_scene_primitive_order: bad argument"); return RTK_AMD_ERR_BAD_ARG; }
	if (ds->view.num_tris == 0) return 0;
	// DevTri.prim is the 4th dword of each 48-byte record
	if (hipMemcpy2D(out, 4, reinterpret_cast<const char *>(ds->view.tris) + 12, sizeof(DevTri), 4, ds->view.num_tris, hipMemcpyDeviceToHost) != hipSuccess) {
		rtk_set_error("rtk_dev_scene_primitive_order: copy failed: %s", hipGetErrorString(hipGetLastError()));
		return RTK_AMD_ERR_HIP;
	}
	return (long long)ds->view.num_tris;
}

// ---------------------------------------------------------------------------- batches

extern "C" int rtk_dev_trace_rays(const rtk_dev_scene *ds, const rtk_ray *d_rays, size_t n,
	rtk_hit_record *d_hits, const rtk_trace_opts *opts, void *stream)
{
	TraceCall c = batch_call(d_rays, n, opts, stream);
	c.hits = d_hits;
	return rtk_launch_trace(ds, c);
}

extern "C" int rtk_dev_trace_rays_any(const rtk_dev_scene *ds, const rtk_ray *d_rays, size_t n,
	uint8_t *d_occluded, const rtk_trace_opts *opts, void *stream)
{
	TraceCall c = batch_call(d_rays, n, opts, stream);
	c.occluded = d_occluded; c.any_hit = true;
	return rtk_launch_trace(ds, c);
}

extern "C" int rtk_dev_trace_rays_filtered(const rtk_dev_scene *ds, const rtk_ray *d_rays, size_t n,
	rtk_hit_record *d_hits, const rtk_dev_filter *filter, const rtk_trace_opts *opts, void *stream)
{
	TraceCall c = batch_call(d_rays, n, opts, stream);
	c.hits = d_hits; c.filter = filter;
	return rtk_launch_trace(ds, c);
}

extern "C" int rtk_dev_trace_rays_any_filtered(const rtk_dev_scene *ds, const rtk_ray *d_rays, size_t n,
	uint8_t *d_occluded, const rtk_dev_filter *filter, const rtk_trace_opts *opts, void *stream)
{
	TraceCall c = batch_call(d_rays, n, opts, stream);
	c.occluded = d_occluded; c.any_hit = true; c.filter = filter;
	return rtk_launch_trace(ds, c);
}

// Rays through a world (rtk_world.hip): the three doors of one launch
extern "C" int rtk_dev_world_trace_rays(const rtk_dev_world *w, const rtk_ray *d_rays, size_t n, const rtk_ray_list *list,
	const rtk_world_filter *filter, rtk_hit_record *d_records, uint32_t *d_instances, void *stream)
{
	return rtk_launch_world(w, d_rays, n, list, filter, d_records, d_instances, nullptr, false, (hipStream_t)stream);
}

extern "C" int rtk_dev_world_trace_rays_any(const rtk_dev_world *w, const rtk_ray *d_rays, size_t n, const rtk_ray_list *list,
	const rtk_world_filter *filter, uint8_t *d_blocked, void *stream)
{
	return rtk_launch_world(w, d_rays, n, list, filter, nullptr, nullptr, d_blocked, true, (hipStream_t)stream);
}

extern "C" int rtk_dev_world_trace_rays_counted(const rtk_dev_world *w, const rtk_ray *d_rays, size_t n, const rtk_world_filter *filter,
	rtk_hit_record *d_records, uint32_t *d_instances, rtk_trace_counters *out)
{
	if (!out) { rtk_set_error("rtk_dev_world_trace_rays_counted: NULL counters"); return RTK_AMD_ERR_BAD_ARG; }
	return rtk_launch_world(w, d_rays, n, nullptr, filter, d_records, d_instances, nullptr, false, nullptr, out);
}

// Closest points on a world (rtk_world_closest.hip): the two doors of one launch
extern "C" int rtk_dev_world_closest_points(const rtk_dev_world *w, const rtk_point_query *d_queries, size_t num_queries,
	const rtk_ray_list *list, const rtk_world_filter *filter, rtk_closest_record *d_records, uint32_t *d_instances, float *d_points, void *stream)
{
	return rtk_launch_world_closest(w, d_queries, num_queries, list, filter, d_records, d_instances, d_points, (hipStream_t)stream);
}

extern "C" int rtk_dev_world_closest_points_counted(const rtk_dev_world *w, const rtk_point_query *d_queries, size_t num_queries,
	const rtk_world_filter *filter, rtk_closest_record *d_records, uint32_t *d_instances, float *d_points, rtk_trace_counters *out)
{
	if (!out) { rtk_set_error("rtk_dev_world_closest_points_counted: NULL counters"); return RTK_AMD_ERR_BAD_ARG; }
	return rtk_launch_world_closest(w, d_queries, num_queries, nullptr, filter, d_records, d_instances, d_points, nullptr, out);
}

// Overlaps on a world (rtk_world_overlap.hip): per shape the three doors of one launch
extern "C" int rtk_dev_world_triangles_in_box_count(const rtk_dev_world *w, const rtk_box_query *d_boxes, size_t num_queries,
	const rtk_ray_list *list, const rtk_world_filter *filter, uint32_t *d_counts, void *stream)
{
	return rtk_launch_world_box(w, d_boxes, num_queries, list, filter, d_counts, nullptr, nullptr, false, (hipStream_t)stream);
}

extern "C" int rtk_dev_world_triangles_in_box_all(const rtk_dev_world *w, const rtk_box_query *d_boxes, size_t num_queries,
	const rtk_ray_list *list, const rtk_world_filter *filter, const uint64_t *d_offsets, uint64_t *d_entries, uint32_t *d_written, void *stream)
{
	return rtk_launch_world_box(w, d_boxes, num_queries, list, filter, d_written, d_offsets, d_entries, true, (hipStream_t)stream);
}

extern "C" int rtk_dev_world_triangles_in_box_counted(const rtk_dev_world *w, const rtk_box_query *d_boxes, size_t num_queries,
	const rtk_world_filter *filter, const uint64_t *d_offsets, uint64_t *d_entries, uint32_t *d_counts_or_written, rtk_trace_counters *out)
{
	if (!out) { rtk_set_error("rtk_dev_world_triangles_in_box_counted: NULL counters"); return RTK_AMD_ERR_BAD_ARG; }
	return rtk_launch_world_box(w, d_boxes, num_queries, nullptr, filter, d_counts_or_written, d_offsets, d_entries, d_offsets != nullptr, nullptr, out);
}

extern "C" int rtk_dev_world_triangles_in_obb_count(const rtk_dev_world *w, const rtk_obb_query *d_obbs, size_t num_queries,
	const rtk_ray_list *list, const rtk_world_filter *filter, uint32_t *d_counts, void *stream)
{
	return rtk_launch_world_obb(w, d_obbs, num_queries, list, filter, d_counts, nullptr, nullptr, false, (hipStream_t)stream);
}

extern "C" int rtk_dev_world_triangles_in_obb_all(const rtk_dev_world *w, const rtk_obb_query *d_obbs, size_t num_queries,
	const rtk_ray_list *list, const rtk_world_filter *filter, const uint64_t *d_offsets, uint64_t *d_entries, uint32_t *d_written, void *stream)
{
	return rtk_launch_world_obb(w, d_obbs, num_queries, list, filter, d_written, d_offsets, d_entries, true, (hipStream_t)stream);
}

extern "C" int rtk_dev_world_triangles_in_obb_counted(const rtk_dev_world *w, const rtk_obb_query *d_obbs, size_t num_queries,
	const rtk_world_filter *filter, const uint64_t *d_offsets, uint64_t *d_entries, uint32_t *d_counts_or_written, rtk_trace_counters *out)
{
	if (!out) { rtk_set_error("rtk_dev_world_triangles_in_obb_counted: NULL counters"); return RTK_AMD_ERR_BAD_ARG; }
	return rtk_launch_world_obb(w, d_obbs, num_queries, nullptr, filter, d_counts_or_written, d_offsets, d_entries, d_offsets != nullptr, nullptr, out);
}

extern "C" int rtk_dev_world_triangles_touching_count(const rtk_dev_world *w, const rtk_tri_query *d_tris, size_t num_queries,
	const rtk_ray_list *list, const rtk_world_filter *filter, uint32_t touch_flags, uint32_t *d_counts, void *stream)
{
	return rtk_launch_world_touch(w, d_tris, num_queries, list, filter, touch_flags, d_counts, nullptr, nullptr, false, (hipStream_t)stream);
}

extern "C" int rtk_dev_world_triangles_touching_all(const rtk_dev_world *w, const rtk_tri_query *d_tris, size_t num_queries,
	const rtk_ray_list *list, const rtk_world_filter *filter, uint32_t touch_flags, const uint64_t *d_offsets, uint64_t *d_entries, uint32_t *d_written,
	void *stream)
{
	return rtk_launch_world_touch(w, d_tris, num_queries, list, filter, touch_flags, d_written, d_offsets, d_entries, true, (hipStream_t)stream);
}

extern "C" int rtk_dev_world_triangles_touching_counted(const rtk_dev_world *w, const rtk_tri_query *d_tris, size_t num_queries,
	const rtk_world_filter *filter, uint32_t touch_flags, const uint64_t *d_offsets, uint64_t *d_entries, uint32_t *d_counts_or_written,
	rtk_trace_counters *out)
{
	if (!out) { rtk_set_error("rtk_dev_world_triangles_touching_counted: NULL counters"); return RTK_AMD_ERR_BAD_ARG; }
	return rtk_launch_world_touch(w, d_tris, num_queries, nullptr, filter, touch_flags, d_counts_or_written, d_offsets, d_entries, d_offsets != nullptr,
		nullptr, out);
}

// Listed batches (rtk_ray_list): everything about the list that the host can see is refused here, before anything is launched
static int listed_trace(const char *who, const rtk_dev_scene *ds, const rtk_ray *d_rays, size_t num_rays, const rtk_ray_list *list,
	rtk_hit_record *d_hits, uint8_t *d_occluded, bool any_hit, const rtk_dev_filter *filter, const rtk_trace_opts *opts, void *stream)
{
	if (!list) { rtk_set_error("%s: NULL list", who); return RTK_AMD_ERR_BAD_ARG; }
	if (list->struct_size < sizeof(rtk_ray_list)) { rtk_set_error("%s: rtk_ray_list.struct_size is too small", who); return RTK_AMD_ERR_BAD_ARG; }
	if (list->flags != 0u) { rtk_set_error("%s: rtk_ray_list.flags must be 0", who); return RTK_AMD_ERR_BAD_ARG; }
	if (!list->d_count) { rtk_set_error("%s: rtk_ray_list.d_count is NULL", who); return RTK_AMD_ERR_BAD_ARG; }
	if (any_hit ? !d_occluded : !d_hits) { rtk_set_error("%s: NULL output", who); return RTK_AMD_ERR_BAD_ARG; }
	if (num_rays >= ((size_t)1 << 32)) { rtk_set_error("%s: %zu rays: a listed batch holds fewer than 2^32", who, num_rays); return RTK_AMD_ERR_BAD_ARG; }
	TraceCall c = batch_call(d_rays, num_rays, opts, stream);
	c.hits = d_hits; c.occluded = d_occluded; c.any_hit = any_hit; c.filter = filter; c.list = list;
	return rtk_launch_trace(ds, c);
}

extern "C" int rtk_dev_trace_rays_listed(const rtk_dev_scene *ds, const rtk_ray *d_rays, size_t num_rays, const rtk_ray_list *list,
	rtk_hit_record *d_hits, const rtk_dev_filter *filter, const rtk_trace_opts *opts, void *stream)
{
	return listed_trace("rtk_dev_trace_rays_listed", ds, d_rays, num_rays, list, d_hits, nullptr, false, filter, opts, stream);
}

extern "C" int rtk_dev_trace_rays_any_listed(const rtk_dev_scene *ds, const rtk_ray *d_rays, size_t num_rays, const rtk_ray_list *list,
	uint8_t *d_occluded, const rtk_dev_filter *filter, const rtk_trace_opts *opts, void *stream)
{
	return listed_trace("rtk_dev_trace_rays_any_listed", ds, d_rays, num_rays, list, nullptr, d_occluded, true, filter, opts, stream);
}

extern "C" int rtk_dev_select_rays(const rtk_dev_scene *ds, const void *d_src, uint32_t kind, size_t num_rays,
	const rtk_ray_list *in, uint64_t *d_out_ids, uint64_t *d_out_count, void *stream)
{
	return rtk_launch_select(const_cast<rtk_dev_scene *>(ds), d_src, kind, num_rays, in, d_out_ids, d_out_count, (hipStream_t)stream);
}

extern "C" int rtk_dev_closest_points(const rtk_dev_scene *ds, const rtk_point_query *d_queries, size_t num_queries,
	const rtk_ray_list *list, rtk_closest_record *d_records, float *d_points, void *stream)
{
	return rtk_launch_closest(ds, d_queries, num_queries, list, d_records, d_points, (hipStream_t)stream);
}

extern "C" int rtk_dev_closest_points_counted(const rtk_dev_scene *ds, const rtk_point_query *d_queries, size_t num_queries,
	rtk_closest_record *d_records, float *d_points, rtk_trace_counters *out)
{
	if (!out) { rtk_set_error("rtk_dev_closest_points_counted: NULL counters"); return RTK_AMD_ERR_BAD_ARG; }
	return rtk_launch_closest(ds, d_queries, num_queries, nullptr, d_records, d_points, nullptr, out);
}

extern "C" int rtk_dev_triangles_within_count(const rtk_dev_scene *ds, const rtk_point_query *d_queries, size_t num_queries,
	const rtk_ray_list *list, uint32_t *d_counts, void *stream)
{
	return rtk_launch_within(ds, d_queries, num_queries, list, d_counts, nullptr, nullptr, nullptr, false, (hipStream_t)stream);
}

extern "C" int rtk_dev_triangles_within_all(const rtk_dev_scene *ds, const rtk_point_query *d_queries, size_t num_queries,
	const rtk_ray_list *list, const uint64_t *d_offsets, rtk_closest_record *d_records, float *d_points, uint32_t *d_written, void *stream)
{
	return rtk_launch_within(ds, d_queries, num_queries, list, d_written, d_offsets, d_records, d_points, true, (hipStream_t)stream);
}

extern "C" int rtk_dev_triangles_within_counted(const rtk_dev_scene *ds, const rtk_point_query *d_queries, size_t num_queries,
	const uint64_t *d_offsets, rtk_closest_record *d_records, float *d_points, uint32_t *d_counts_or_written, rtk_trace_counters *out)
{
	if (!out) { rtk_set_error("rtk_dev_triangles_within_counted: NULL counters"); return RTK_AMD_ERR_BAD_ARG; }
	return rtk_launch_within(ds, d_queries, num_queries, nullptr, d_counts_or_written, d_offsets, d_records, d_points, d_offsets != nullptr, nullptr, out);
}

extern "C" int rtk_dev_triangles_in_box_count(const rtk_dev_scene *ds, const rtk_box_query *d_boxes, size_t num_queries,
	const rtk_ray_list *list, uint32_t *d_counts, void *stream)
{
	return rtk_launch_box(ds, d_boxes, num_queries, list, d_counts, nullptr, nullptr, false, (hipStream_t)stream);
}

extern "C" int rtk_dev_triangles_in_box_all(const rtk_dev_scene *ds, const rtk_box_query *d_boxes, size_t num_queries,
	const rtk_ray_list *list, const uint64_t *d_offsets, uint32_t *d_prims, uint32_t *d_written, void *stream)
{
	return rtk_launch_box(ds, d_boxes, num_queries, list, d_written, d_offsets, d_prims, true, (hipStream_t)stream);
}

extern "C" int rtk_dev_triangles_in_box_counted(const rtk_dev_scene *ds, const rtk_box_query *d_boxes, size_t num_queries,
	const uint64_t *d_offsets, uint32_t *d_prims, uint32_t *d_counts_or_written, rtk_trace_counters *out)
{
	if (!out) { rtk_set_error("rtk_dev_triangles_in_box_counted: NULL counters"); return RTK_AMD_ERR_BAD_ARG; }
	return rtk_launch_box(ds, d_boxes, num_queries, nullptr, d_counts_or_written, d_offsets, d_prims, d_offsets != nullptr, nullptr, out);
}

extern "C" int rtk_dev_triangles_in_obb_count(const rtk_dev_scene *ds, const rtk_obb_query *d_obbs, size_t num_queries,
	const rtk_ray_list *list, uint32_t *d_counts, void *stream)
{
	return rtk_launch_obb(ds, d_obbs, num_queries, list, d_counts, nullptr, nullptr, false, (hipStream_t)stream);
}

extern "C" int rtk_dev_triangles_in_obb_all(const rtk_dev_scene *ds, const rtk_obb_query *d_obbs, size_t num_queries,
	const rtk_ray_list *list, const uint64_t *d_offsets, uint32_t *d_prims, uint32_t *d_written, void *stream)
{
	return rtk_launch_obb(ds, d_obbs, num_queries, list, d_written, d_offsets, d_prims, true, (hipStream_t)stream);
}

extern "C" int rtk_dev_triangles_in_obb_counted(const rtk_dev_scene *ds, const rtk_obb_query *d_obbs, size_t num_queries,
	const uint64_t *d_offsets, uint32_t *d_prims, uint32_t *d_counts_or_written, rtk_trace_counters *out)
{
	if (!out) { rtk_set_error("rtk_dev_triangles_in_obb_counted: NULL counters"); return RTK_AMD_ERR_BAD_ARG; }
	return rtk_launch_obb(ds, d_obbs, num_queries, nullptr, d_counts_or_written, d_offsets, d_prims, d_offsets != nullptr, nullptr, out);
}

extern "C" int rtk_dev_triangles_touching_count(const rtk_dev_scene *ds, const rtk_tri_query *d_tris, size_t num_queries,
	const rtk_ray_list *list, const rtk_touch_filter *filter, uint32_t *d_counts, void *stream)
{
	return rtk_launch_touch(ds, d_tris, num_queries, list, filter, d_counts, nullptr, nullptr, false, (hipStream_t)stream);
}

extern "C" int rtk_dev_triangles_touching_all(const rtk_dev_scene *ds, const rtk_tri_query *d_tris, size_t num_queries,
	const rtk_ray_list *list, const rtk_touch_filter *filter, const uint64_t *d_offsets, uint32_t *d_prims, uint32_t *d_written, void *stream)
{
	return rtk_launch_touch(ds, d_tris, num_queries, list, filter, d_written, d_offsets, d_prims, true, (hipStream_t)stream);
}

extern "C" int rtk_dev_triangles_touching_counted(const rtk_dev_scene *ds, const rtk_tri_query *d_tris, size_t num_queries,
	const rtk_touch_filter *filter, const uint64_t *d_offsets, uint32_t *d_prims, uint32_t *d_counts_or_written, rtk_trace_counters *out)
{
	if (!out) { rtk_set_error("rtk_dev_triangles_touching_counted: NULL counters"); return RTK_AMD_ERR_BAD_ARG; }
	return rtk_launch_touch(ds, d_tris, num_queries, nullptr, filter, d_counts_or_written, d_offsets, d_prims, d_offsets != nullptr, nullptr, out);
}

extern "C" int rtk_dev_closest_triangles(const rtk_dev_scene *ds, const rtk_tri_query *d_tris, size_t num_queries,
	const rtk_ray_list *list, const rtk_touch_filter *filter, const float *d_max_dist2, rtk_closest_record *d_records,
	float *d_points_query, float *d_points_scene, void *stream)
{
	return rtk_launch_pair(ds, d_tris, num_queries, list, filter, d_max_dist2, d_records, d_points_query, d_points_scene, (hipStream_t)stream);
}

extern "C" int rtk_dev_closest_triangles_counted(const rtk_dev_scene *ds, const rtk_tri_query *d_tris, size_t num_queries,
	const rtk_touch_filter *filter, const float *d_max_dist2, rtk_closest_record *d_records, float *d_points_query, float *d_points_scene,
	rtk_trace_counters *out)
{
	if (!out) { rtk_set_error("rtk_dev_closest_triangles_counted: NULL counters"); return RTK_AMD_ERR_BAD_ARG; }
	return rtk_launch_pair(ds, d_tris, num_queries, nullptr, filter, d_max_dist2, d_records, d_points_query, d_points_scene, nullptr, out);
}

extern "C" int rtk_dev_triangles_near_count(const rtk_dev_scene *ds, const rtk_tri_query *d_tris, size_t num_queries,
	const rtk_ray_list *list, const rtk_touch_filter *filter, const float *d_max_dist2, uint32_t *d_counts, void *stream)
{
	return rtk_launch_near(ds, d_tris, num_queries, list, filter, d_max_dist2, d_counts, nullptr, nullptr, nullptr, nullptr, false, (hipStream_t)stream);
}

extern "C" int rtk_dev_triangles_near_all(const rtk_dev_scene *ds, const rtk_tri_query *d_tris, size_t num_queries,
	const rtk_ray_list *list, const rtk_touch_filter *filter, const float *d_max_dist2, const uint64_t *d_offsets, rtk_closest_record *d_records,
	float *d_points_query, float *d_points_scene, uint32_t *d_written, void *stream)
{
	return rtk_launch_near(ds, d_tris, num_queries, list, filter, d_max_dist2, d_written, d_offsets, d_records, d_points_query, d_points_scene, true,
		(hipStream_t)stream);
}

extern "C" int rtk_dev_triangles_near_counted(const rtk_dev_scene *ds, const rtk_tri_query *d_tris, size_t num_queries,
	const rtk_touch_filter *filter, const float *d_max_dist2, const uint64_t *d_offsets, rtk_closest_record *d_records, float *d_points_query,
	float *d_points_scene, uint32_t *d_counts_or_written, rtk_trace_counters *out)
{
	if (!out) { rtk_set_error("rtk_dev_triangles_near_counted: NULL counters"); return RTK_AMD_ERR_BAD_ARG; }
	return rtk_launch_near(ds, d_tris, num_queries, nullptr, filter, d_max_dist2, d_counts_or_written, d_offsets, d_records, d_points_query,
		d_points_scene, d_offsets != nullptr, nullptr, out);
}

extern "C" int rtk_dev_sweep_spheres(const rtk_dev_scene *ds, const rtk_sphere_sweep *d_sweeps, size_t num_sweeps, const rtk_ray_list *list,
	rtk_hit_record *d_records, float *d_points, float *d_centres, const rtk_dev_filter *filter, void *stream)
{
	return rtk_launch_sweep(ds, d_sweeps, num_sweeps, list, d_records, d_points, d_centres, nullptr, false, filter, (hipStream_t)stream);
}

extern "C" int rtk_dev_sweep_spheres_any(const rtk_dev_scene *ds, const rtk_sphere_sweep *d_sweeps, size_t num_sweeps, const rtk_ray_list *list,
	uint8_t *d_blocked, const rtk_dev_filter *filter, void *stream)
{
	return rtk_launch_sweep(ds, d_sweeps, num_sweeps, list, nullptr, nullptr, nullptr, d_blocked, true, filter, (hipStream_t)stream);
}

extern "C" int rtk_dev_sweep_spheres_counted(const rtk_dev_scene *ds, const rtk_sphere_sweep *d_sweeps, size_t num_sweeps,
	rtk_hit_record *d_records, float *d_points, float *d_centres, const rtk_dev_filter *filter, rtk_trace_counters *out)
{
	if (!out) { rtk_set_error("rtk_dev_sweep_spheres_counted: NULL counters"); return RTK_AMD_ERR_BAD_ARG; }
	return rtk_launch_sweep(ds, d_sweeps, num_sweeps, nullptr, d_records, d_points, d_centres, nullptr, false, filter, nullptr, out);
}

extern "C" int rtk_dev_sweep_boxes(const rtk_dev_scene *ds, const rtk_box_sweep *d_sweeps, size_t num_sweeps, const rtk_ray_list *list,
	rtk_hit_record *d_records, float *d_centres, float *d_normals, const rtk_dev_filter *filter, void *stream)
{
	return rtk_launch_boxsweep(ds, d_sweeps, num_sweeps, list, d_records, d_centres, d_normals, nullptr, false, filter, (hipStream_t)stream);
}

extern "C" int rtk_dev_sweep_boxes_any(const rtk_dev_scene *ds, const rtk_box_sweep *d_sweeps, size_t num_sweeps, const rtk_ray_list *list,
	uint8_t *d_blocked, const rtk_dev_filter *filter, void *stream)
{
	return rtk_launch_boxsweep(ds, d_sweeps, num_sweeps, list, nullptr, nullptr, nullptr, d_blocked, true, filter, (hipStream_t)stream);
}

extern "C" int rtk_dev_sweep_boxes_counted(const rtk_dev_scene *ds, const rtk_box_sweep *d_sweeps, size_t num_sweeps,
	rtk_hit_record *d_records, float *d_centres, float *d_normals, const rtk_dev_filter *filter, rtk_trace_counters *out)
{
	if (!out) { rtk_set_error("rtk_dev_sweep_boxes_counted: NULL counters"); return RTK_AMD_ERR_BAD_ARG; }
	return rtk_launch_boxsweep(ds, d_sweeps, num_sweeps, nullptr, d_records, d_centres, d_normals, nullptr, false, filter, nullptr, out);
}

extern "C" int rtk_dev_sweep_capsules(const rtk_dev_scene *ds, const rtk_capsule_sweep *d_sweeps, size_t num_sweeps, const rtk_ray_list *list,
	rtk_hit_record *d_records, float *d_points, float *d_axis_points, const rtk_dev_filter *filter, void *stream)
{
	return rtk_launch_capsule(ds, d_sweeps, num_sweeps, list, d_records, d_points, d_axis_points, nullptr, false, filter, (hipStream_t)stream);
}

extern "C" int rtk_dev_sweep_capsules_any(const rtk_dev_scene *ds, const rtk_capsule_sweep *d_sweeps, size_t num_sweeps, const rtk_ray_list *list,
	uint8_t *d_blocked, const rtk_dev_filter *filter, void *stream)
{
	return rtk_launch_capsule(ds, d_sweeps, num_sweeps, list, nullptr, nullptr, nullptr, d_blocked, true, filter, (hipStream_t)stream);
}

extern "C" int rtk_dev_sweep_capsules_counted(const rtk_dev_scene *ds, const rtk_capsule_sweep *d_sweeps, size_t num_sweeps,
	rtk_hit_record *d_records, float *d_points, float *d_axis_points, const rtk_dev_filter *filter, rtk_trace_counters *out)
{
	if (!out) { rtk_set_error("rtk_dev_sweep_capsules_counted: NULL counters"); return RTK_AMD_ERR_BAD_ARG; }
	return rtk_launch_capsule(ds, d_sweeps, num_sweeps, nullptr, d_records, d_points, d_axis_points, nullptr, false, filter, nullptr, out);
}

extern "C" int rtk_dev_sweep_obbs(const rtk_dev_scene *ds, const rtk_obb_sweep *d_sweeps, size_t num_sweeps, const rtk_ray_list *list,
	rtk_hit_record *d_records, float *d_centres, float *d_normals, const rtk_dev_filter *filter, void *stream)
{
	return rtk_launch_obbsweep(ds, d_sweeps, num_sweeps, list, d_records, d_centres, d_normals, nullptr, false, filter, (hipStream_t)stream);
}

extern "C" int rtk_dev_sweep_obbs_any(const rtk_dev_scene *ds, const rtk_obb_sweep *d_sweeps, size_t num_sweeps, const rtk_ray_list *list,
	uint8_t *d_blocked, const rtk_dev_filter *filter, void *stream)
{
	return rtk_launch_obbsweep(ds, d_sweeps, num_sweeps, list, nullptr, nullptr, nullptr, d_blocked, true, filter, (hipStream_t)stream);
}

extern "C" int rtk_dev_sweep_obbs_counted(const rtk_dev_scene *ds, const rtk_obb_sweep *d_sweeps, size_t num_sweeps,
	rtk_hit_record *d_records, float *d_centres, float *d_normals, const rtk_dev_filter *filter, rtk_trace_counters *out)
{
	if (!out) { rtk_set_error("rtk_dev_sweep_obbs_counted: NULL counters"); return RTK_AMD_ERR_BAD_ARG; }
	return rtk_launch_obbsweep(ds, d_sweeps, num_sweeps, nullptr, d_records, d_centres, d_normals, nullptr, false, filter, nullptr, out);
}

extern "C" int rtk_dev_trace_rays_count(const rtk_dev_scene *ds, const rtk_ray *d_rays, size_t n,
	uint32_t *d_counts, const rtk_dev_filter *filter, const rtk_trace_opts *opts, void *stream)
{
	return rtk_launch_allhits(ds, d_rays, n, d_counts, nullptr, nullptr, nullptr, false, filter, opts, (hipStream_t)stream);
}

extern "C" int rtk_dev_trace_rays_all(const rtk_dev_scene *ds, const rtk_ray *d_rays, size_t n,
	const uint64_t *d_offsets, rtk_hit_record *d_records, uint32_t *d_written, const rtk_dev_filter *filter, const rtk_trace_opts *opts, void *stream)
{
	return rtk_launch_allhits(ds, d_rays, n, nullptr, d_offsets, d_records, d_written, true, filter, opts, (hipStream_t)stream);
}

extern "C" int rtk_dev_trace_rays_counted(const rtk_dev_scene *ds, const rtk_ray *d_rays, size_t n,
	rtk_hit_record *d_hits, const rtk_trace_opts *opts, rtk_trace_counters *out)
{
	if (!out) { rtk_set_error("rtk_dev_trace_rays_counted: NULL counters"); return RTK_AMD_ERR_BAD_ARG; }
	TraceCall c = batch_call(d_rays, n, opts, nullptr);
	c.hits = d_hits; c.counted = out;
	return rtk_launch_trace(ds, c);
}

extern "C" int rtk_dev_trace_rays_any_counted(const rtk_dev_scene *ds, const rtk_ray *d_rays, size_t n,
	uint8_t *d_occluded, const rtk_trace_opts *opts, rtk_trace_counters *out)
{
	if (!out) { rtk_set_error("rtk_dev_trace_rays_any_counted: NULL counters"); return RTK_AMD_ERR_BAD_ARG; }
	TraceCall c = batch_call(d_rays, n, opts, nullptr);
	c.occluded = d_occluded; c.any_hit = true; c.counted = out;
	return rtk_launch_trace(ds, c);
}

extern "C" int rtk_dev_trace_rays_packet_counted(const rtk_dev_scene *ds, const rtk_ray *d_rays, size_t n,
	rtk_hit_record *d_hits, const rtk_trace_opts *opts, rtk_packet_counters *out)
{
	if (!out) { rtk_set_error("rtk_dev_trace_rays_packet_counted: NULL counters"); return RTK_AMD_ERR_BAD_ARG; }
	TraceCall c = batch_call(d_rays, n, opts, nullptr);
	c.hits = d_hits; c.pk_counted = out;
	return rtk_launch_trace(ds, c);
}

extern "C" int rtk_dev_debug_packet_entries(const rtk_dev_scene *ds, const rtk_ray *d_rays, uint32_t image_w, uint32_t image_h,
	uint32_t target, uint32_t max_levels, void *host_out)
{
	return rtk_debug_packet_entries(ds, d_rays, image_w, image_h, target, max_levels, host_out);
}

extern "C" int rtk_dev_detect_image(const rtk_dev_scene *ds, const rtk_ray *d_rays, size_t n, uint32_t *width, uint32_t *height, void *stream)
{
	if (!ds || !width || !height || (!d_rays && n)) { rtk_set_error("rtk_dev_detect_image: NULL argument"); return RTK_AMD_ERR_BAD_ARG; }
	return rtk_detect_image(ds, d_rays, n, (hipStream_t)stream, width, height);
}

extern "C" int rtk_dev_trace_status(const rtk_dev_scene *ds, void *stream)
{
	return rtk_trace_status(ds, (hipStream_t)stream);
}

extern "C" int rtk_dev_expand_hits(const rtk_dev_scene *ds, const rtk_hit_record *d_records, size_t n,
	rtk_hit *d_hits, uint8_t *d_mask, void *stream)
{
	return rtk_launch_expand(ds, d_records, n, d_hits, d_mask, (hipStream_t)stream);
}
