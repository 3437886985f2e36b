// rtk_layout_check.h -- compile-time proof that include/rtk.h has the reference's ABI
// (sizes and offsets probed from the reference build).
#pragma once

#include <stddef.h>

#include "rtk.h"
#include "rtk_amd.h"

static_assert(sizeof(rtk_vec3) == 12, "rtk_vec3");
static_assert(sizeof(rtk_vertex) == 16 && offsetof(rtk_vertex, index) == 12, "rtk_vertex");
static_assert(sizeof(rtk_ray) == 32 && offsetof(rtk_ray, direction) == 12 && offsetof(rtk_ray, min_t) == 24, "rtk_ray");
static_assert(sizeof(rtk_hit) == 68 && offsetof(rtk_hit, vertex) == 12 && offsetof(rtk_hit, mesh_index) == 60, "rtk_hit");
static_assert(sizeof(rtk_buffer) == 24, "rtk_buffer");
static_assert(sizeof(rtk_mesh) == 96 && offsetof(rtk_mesh, position) == 16 && offsetof(rtk_mesh, index) == 40 &&
	offsetof(rtk_mesh, position_cb) == 64 && offsetof(rtk_mesh, index_cb) == 80, "rtk_mesh");
static_assert(sizeof(rtk_scene) == 56 && offsetof(rtk_scene, size_in_bytes) == 24 && offsetof(rtk_scene, vertex_offset) == 48, "rtk_scene");
static_assert(sizeof(rtk_scene_desc) == 32, "rtk_scene_desc");
static_assert(sizeof(rtk_task) == 40 && offsetof(rtk_task, cost) == 16 && offsetof(rtk_task, arg) == 32, "rtk_task");
static_assert(sizeof(rtk_hit_record) == 16, "rtk_hit_record");
static_assert(sizeof(rtk_dev_scene_quality_info) == 96 && offsetof(rtk_dev_scene_quality_info, inner_children) == 8 &&
	offsetof(rtk_dev_scene_quality_info, root_area) == 24 && offsetof(rtk_dev_scene_quality_info, measure_ms) == 88, "rtk_dev_scene_quality_info");
static_assert(sizeof(rtk_dev_split_info) == 48 && offsetof(rtk_dev_split_info, leaves_split) == 8 && offsetof(rtk_dev_split_info, largest_leaf_before) == 24 &&
	offsetof(rtk_dev_split_info, max_depth_after) == 36 && offsetof(rtk_dev_split_info, split_ms) == 40, "rtk_dev_split_info");
static_assert(sizeof(rtk_placement) == 48 && offsetof(rtk_placement, m) == 0, "rtk_placement");
static_assert(sizeof(rtk_point_query) == 16 && offsetof(rtk_point_query, max_dist2) == 12, "rtk_point_query");
static_assert(sizeof(rtk_closest_record) == 16 && offsetof(rtk_closest_record, prim) == 12, "rtk_closest_record");
static_assert(sizeof(rtk_sphere_sweep) == 36 && offsetof(rtk_sphere_sweep, direction) == 12 && offsetof(rtk_sphere_sweep, min_t) == 24 &&
	offsetof(rtk_sphere_sweep, radius) == 32, "rtk_sphere_sweep");
static_assert(sizeof(rtk_box_sweep) == 44 && offsetof(rtk_box_sweep, direction) == 12 && offsetof(rtk_box_sweep, min_t) == 24 &&
	offsetof(rtk_box_sweep, half) == 32, "rtk_box_sweep");
static_assert(sizeof(rtk_capsule_sweep) == 48 && offsetof(rtk_capsule_sweep, direction) == 12 && offsetof(rtk_capsule_sweep, min_t) == 24 &&
	offsetof(rtk_capsule_sweep, radius) == 32 && offsetof(rtk_capsule_sweep, half_axis) == 36, "rtk_capsule_sweep");
static_assert(sizeof(rtk_obb_sweep) == 80 && offsetof(rtk_obb_sweep, direction) == 12 && offsetof(rtk_obb_sweep, min_t) == 24 &&
	offsetof(rtk_obb_sweep, half) == 32 && offsetof(rtk_obb_sweep, axes) == 44, "rtk_obb_sweep");
static_assert(sizeof(rtk_obb_query) == 60 && offsetof(rtk_obb_query, half) == 12 && offsetof(rtk_obb_query, axes) == 24, "rtk_obb_query");
static_assert(sizeof(rtk_dev_filter) == 32&& offsetof(rtk_dev_filter, d_ignore_prim) == 16 && offsetof(rtk_dev_filter, d_after) == 24, "rtk_dev_filter");
static_assert(sizeof(rtk_dev_rebuild_info) == 40 && offsetof(rtk_dev_rebuild_info, nodes_before) == 8 && offsetof(rtk_dev_rebuild_info, max_depth_before) == 24 &&
	offsetof(rtk_dev_rebuild_info, rebuild_ms) == 32, "rtk_dev_rebuild_info");
static_assert(sizeof(rtk_dev_sign_info) == 56 && offsetof(rtk_dev_sign_info, places) == 32 && offsetof(rtk_dev_sign_info, table_ms) == 48, "rtk_dev_sign_info");
static_assert(sizeof(rtk_winding_opts) == 12 && offsetof(rtk_winding_opts, beta) == 8, "rtk_winding_opts");
static_assert(sizeof(rtk_dev_winding_info) == 56 && offsetof(rtk_dev_winding_info, table_ms) == 16 && offsetof(rtk_dev_winding_info, total_area) == 48, "rtk_dev_winding_info");
static_assert(sizeof(rtk_world_filter) == 32 && offsetof(rtk_world_filter, d_instance_mask) == 8 && offsetof(rtk_world_filter, d_ignore_instance) == 24, "rtk_world_filter");
static_assert(sizeof(rtk_dev_world_info) == 64 && offsetof(rtk_dev_world_info, top_nodes) == 24 && offsetof(rtk_dev_world_info, top_max_depth) == 40 &&
	offsetof(rtk_dev_world_info, build_ms) == 48, "rtk_dev_world_info");
// (rtk_dev.h, which rtk_capi.hip includes before this file: the record k_world reads as four 16-byte pieces)
static_assert(sizeof(DevWorldInstance) == 64 && offsetof(DevWorldInstance, scene) == 48 && offsetof(DevWorldInstance, flags) == 52, "one 64-byte record per instance of a world");
