"""Python host-side mirror of the rtk interface over librtk_amd.so (ctypes).

Names follow the reference's API (reference rtk.h:119-130): build_scene / free_scene /
trace_ray, plus the additive batch calls of include/rtk_amd.h. Everything goes through
the C-ABI; there is no Python or CPU fallback -- if the HIP library is missing or no GPU
is present the calls raise.

torch is used only as plumbing: device buffers and the current HIP stream.
"""
import collections
import ctypes as C
import os

import numpy as np

from .types import (BOX_QUERY_DTYPE, BOX_SWEEP_DTYPE, CAPSULE_SWEEP_DTYPE, CLOSEST_RECORD_DTYPE, HIT_DTYPE, HIT_RECORD_DTYPE, OBB_QUERY_DTYPE, OBB_SWEEP_DTYPE, POINT_QUERY_DTYPE, RAY_DTYPE, RTK_INF, SPHERE_SWEEP_DTYPE, TRI_QUERY_DTYPE, WORLD_ENTRY_DTYPE, MeshSet, Placement, SceneDesc, SceneHeader,
                    placement_array)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RTK_AMD_LIB") or os.path.join(HERE, "librtk_amd.so")   # RTK_AMD_LIB: kernel A/B builds only

RTK_TRACE_STATIC = 1
RTK_TRACE_NO_PACKET = 2
RTK_TRACE_SORT_RAYS = 4
RTK_TRACE_EXACT_NODES = 8
RTK_TRACE_NO_ASM = 16


class RtkError(RuntimeError):
    pass


class SceneInfo(C.Structure):
    _fields_ = [("num_triangles", C.c_uint64), ("num_meshes", C.c_uint64), ("num_nodes", C.c_uint64),
                ("node_bytes", C.c_uint64), ("triangle_bytes", C.c_uint64), ("total_device_bytes", C.c_uint64),
                ("max_depth", C.c_uint32), ("stack_entries", C.c_uint32), ("build_ms", C.c_double)]

    def as_dict(self):
        return {k: (float(getattr(self, k)) if k == "build_ms" else int(getattr(self, k))) for k, _ in self._fields_}


class SceneCheck(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in (
        "nodes_checked", "leaves_checked", "triangles_checked", "box_violations", "loose_boxes", "bad_references",
        "leaf_format_errors", "triangles_missing", "triangles_duplicated", "nodes_unreachable", "nodes_shared",
        "primitive_id_errors", "compressed_node_errors", "first_bad_index", "content_hash")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class SceneQuality(C.Structure):
    """rtk_dev_scene_quality_info: the SAH cost of a scene's tree as it is now."""
    _fields_ = [("struct_size", C.c_uint32), ("nonfinite_boxes", C.c_uint32), ("inner_children", C.c_uint64),
                ("leaf_children", C.c_uint64), ("root_area", C.c_double), ("inner_area", C.c_double), ("leaf_area", C.c_double),
                ("leaf_area_triangles", C.c_double), ("node_visits", C.c_double), ("triangle_tests", C.c_double),
                ("sah_cost", C.c_double), ("sah_cost_at_build", C.c_double), ("measure_ms", C.c_double)]

    def as_dict(self):
        return {k: (float(getattr(self, k)) if t is C.c_double else int(getattr(self, k))) for k, t in self._fields_}


class SplitInfo(C.Structure):
    """rtk_dev_split_info: what rtk_dev_scene_split_leaves did."""
    _fields_ = [("struct_size", C.c_uint32), ("max_leaf", C.c_uint32), ("leaves_split", C.c_uint64), ("nodes_added", C.c_uint64),
                ("largest_leaf_before", C.c_uint32), ("largest_leaf_after", C.c_uint32), ("max_depth_before", C.c_uint32),
                ("max_depth_after", C.c_uint32), ("split_ms", C.c_double)]

    def as_dict(self):
        return {k: (float(getattr(self, k)) if t is C.c_double else int(getattr(self, k))) for k, t in self._fields_}


class RebuildInfo(C.Structure):
    """rtk_dev_rebuild_info: what rtk_dev_scene_rebuild did."""
    _fields_ = [("struct_size", C.c_uint32), ("key_bits", C.c_uint32), ("nodes_before", C.c_uint64), ("nodes_after", C.c_uint64),
                ("max_depth_before", C.c_uint32), ("max_depth_after", C.c_uint32), ("rebuild_ms", C.c_double)]

    def as_dict(self):
        return {k: (float(getattr(self, k)) if t is C.c_double else int(getattr(self, k))) for k, t in self._fields_}


class SignInfo(C.Structure):
    """rtk_dev_sign_info: what the making of a scene's table of pseudonormals found (rtk_dev_scene_prepare_signs)."""
    _fields_ = [("boundary_sides", C.c_uint64), ("nonmanifold_sides", C.c_uint64), ("inconsistent_sides", C.c_uint64),
                ("degenerate_triangles", C.c_uint64), ("places", C.c_uint64), ("table_bytes", C.c_uint64), ("table_ms", C.c_double)]

    def as_dict(self):
        return {k: (float(getattr(self, k)) if t is C.c_double else int(getattr(self, k))) for k, t in self._fields_}


class WindingInfo(C.Structure):
    """rtk_dev_winding_info: what the making of a scene's table of winding moments found (rtk_dev_scene_prepare_winding)."""
    _fields_ = [("nodes", C.c_uint64), ("table_bytes", C.c_uint64), ("table_ms", C.c_double), ("total_area_vector", C.c_double * 3),
                ("total_area", C.c_double)]

    def as_dict(self):
        return dict(nodes=int(self.nodes), table_bytes=int(self.table_bytes), table_ms=float(self.table_ms),
                    total_area_vector=[float(x) for x in self.total_area_vector], total_area=float(self.total_area))


class WindingOpts(C.Structure):
    """rtk_winding_opts: beta of the accept test (0: the default, 2) and RTK_WINDING_EXACT."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("beta", C.c_float)]


RTK_WINDING_EXACT = 1


def make_winding_opts(beta=2.0, exact=False):
    o = WindingOpts()
    o.struct_size, o.flags, o.beta = C.sizeof(WindingOpts), (RTK_WINDING_EXACT if exact else 0), beta
    return o


class WorldInfo(C.Structure):
    """rtk_dev_world_info: the figures of an instanced world (rtk_dev_world_get_info)."""
    _fields_ = [("num_scenes", C.c_uint64), ("num_instances", C.c_uint64), ("dead_instances", C.c_uint64), ("top_nodes", C.c_uint64),
                ("total_device_bytes", C.c_uint64), ("top_max_depth", C.c_uint32), ("stack_entries", C.c_uint32), ("build_ms", C.c_double),
                ("update_ms", C.c_double)]

    def as_dict(self):
        return {k: (float(getattr(self, k)) if t is C.c_double else int(getattr(self, k))) for k, t in self._fields_}


class WorldFilter(C.Structure):
    """rtk_world_filter: which instances the rays of a world trace may enter."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("d_instance_mask", C.c_void_p), ("instance_mask_bits", C.c_uint32),
                ("d_ignore_instance", C.c_void_p)]


class TraceOpts(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("image_width", C.c_uint32),
                ("image_height", C.c_uint32), ("refill_min", C.c_uint32), ("blocks_per_cu", C.c_uint32),
                ("node_exit", C.c_uint32)]


class DevFilter(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("mesh_mask_bits", C.c_uint32), ("d_mesh_mask", C.c_void_p),
                ("d_ignore_prim", C.c_void_p), ("d_after", C.c_void_p)]


class RayList(C.Structure):
    """rtk_ray_list: the rays of a batch that a listed trace takes, named on the device."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("d_ids", C.c_void_p), ("d_count", C.c_void_p)]


class TouchFilter(C.Structure):
    """rtk_touch_filter: the filter of the touching calls (include/rtk_amd.h, "Triangles that touch a triangle")."""
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("d_first_prim", C.c_void_p)]


TOUCH_SKIP_SHARED_VERTEX = 1


def make_touch_filter(first_prim=None, skip_shared=False):
    """first_prim: a cuda tensor of one 32-bit word per query slot, or None; it must outlive the calls that read it. Returns None
    when there is nothing to filter (the calls then get NULL)."""
    if first_prim is None and not skip_shared:
        return None
    f = TouchFilter()
    f.struct_size = C.sizeof(TouchFilter)
    f.flags = TOUCH_SKIP_SHARED_VERTEX if skip_shared else 0
    f.d_first_prim = first_prim.data_ptr() if first_prim is not None else None
    return f


# rtk_dev_select_rays kinds
SELECT_RECORD_HIT, SELECT_RECORD_MISS, SELECT_BYTE_NONZERO, SELECT_BYTE_ZERO = 0, 1, 2, 3


def make_ray_list(count, ids=None):
    """count: a cuda tensor whose first 8 bytes are the number of entries; ids: a cuda int64 tensor of ray numbers, or None for
    0, 1, 2, ... The tensors must outlive the calls that read them."""
    l = RayList()
    l.struct_size = C.sizeof(RayList)
    l.d_ids = ids.data_ptr() if ids is not None else None
    l.d_count = count.data_ptr() if count is not None else None
    return l


FILTER_FN = C.CFUNCTYPE(C.c_bool, C.c_void_p, C.c_void_p, C.c_void_p)   # rtk_filter_fn (rtk.h:117)


class TraceCounters(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("nodes", C.c_uint64), ("leaves", C.c_uint64),
                ("triangles", C.c_uint64), ("hits", C.c_uint64), ("stack_spills", C.c_uint64),
                ("wave_node_steps", C.c_uint64), ("wave_triangle_steps", C.c_uint64), ("wave_rays", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class PacketCounters(C.Structure):
    """rtk_packet_counters: step counts of rtk_packet_count2 (the counting form of rtk_packet_beam2)."""
    _fields_ = [("tiles", C.c_uint64), ("pairs", C.c_uint64), ("node_steps", C.c_uint64), ("triangles_fetched", C.c_uint64),
                ("triangle_group_tests", C.c_uint64), ("tiles_handed_back", C.c_uint64),
                ("handed_back_node_steps", C.c_uint64), ("handed_back_triangle_steps", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


# one record of rtk_dev_debug_packet_entries (PkBlockEntries, rtk_amd/csrc/rtk_trace_shared.h)
PACKET_ENTRIES_DTYPE = np.dtype([("olo", "<f4", (3,)), ("ohi", "<f4", (3,)), ("rlo", "<f4", (3,)), ("rhi", "<f4", (3,)), ("count", "<u4"), ("tmin", "<f4"),
                                 ("pad", "<u4", (2,)), ("e", [("ref", "<u4"), ("tlo", "<f4")], (56,))])
assert PACKET_ENTRIES_DTYPE.itemsize == 512

# every symbol include/rtk.h and include/rtk_amd.h declare
RTK_H_SYMBOLS = ["rtk_start_build", "rtk_run_task", "rtk_get_build_size", "rtk_finish_build_to",
                 "rtk_finish_build", "rtk_build_scene", "rtk_free_scene", "rtk_trace_ray", "rtk_trace_ray_filter"]
RTK_AMD_H_SYMBOLS = ["rtk_amd_last_error", "rtk_amd_device_count", "rtk_amd_set_device",
                     "rtk_dev_scene_upload", "rtk_dev_scene_build", "rtk_dev_scene_free", "rtk_dev_scene_get_info",
                     "rtk_dev_scene_mesh_base", "rtk_dev_scene_primitive_order", "rtk_dev_scene_export_size", "rtk_dev_scene_export",
                     "rtk_dev_trace_rays", "rtk_dev_trace_rays_any", "rtk_dev_expand_hits",
                     "rtk_dev_trace_rays_counted", "rtk_dev_trace_rays_any_counted", "rtk_dev_trace_rays_packet_counted", "rtk_dev_debug_packet_entries", "rtk_dev_detect_image", "rtk_trace_rays", "rtk_amd_forget_scene",
                     "rtk_dev_scene_validate", "rtk_amd_release_workspace", "rtk_dev_scene_upload_buffer",
                     "rtk_dev_trace_rays_filtered", "rtk_dev_trace_rays_any_filtered", "rtk_dev_trace_status",
                     "rtk_trace_rays_filter", "rtk_amd_shard_range", "rtk_mgpu_create", "rtk_mgpu_destroy", "rtk_mgpu_num_devices",
                     "rtk_mgpu_scene", "rtk_mgpu_build", "rtk_mgpu_upload", "rtk_mgpu_trace_rays", "rtk_mgpu_trace_rays_device",
                     "rtk_amd_set_builder", "rtk_amd_get_builder", "rtk_amd_set_per_ray",
                     "rtk_mgpu_trace_rays_device_striped", "rtk_mgpu_striped_segment",
                     "rtk_dev_scene_refit", "rtk_dev_scene_last_refit_ms", "rtk_mgpu_refit",
                     "rtk_dev_scene_refit_meshes", "rtk_dev_scene_last_refit_nodes", "rtk_mgpu_refit_meshes",
                     "rtk_dev_scene_quality", "rtk_dev_scene_split_leaves", "rtk_mgpu_split_leaves",
                     "rtk_dev_scene_rebuild", "rtk_mgpu_rebuild",
                     "rtk_dev_scene_build_placed", "rtk_dev_scene_refit_placed", "rtk_dev_scene_refit_meshes_placed",
                     "rtk_mgpu_build_placed", "rtk_mgpu_refit_placed", "rtk_mgpu_refit_meshes_placed",
                     "rtk_dev_trace_rays_listed", "rtk_dev_trace_rays_any_listed", "rtk_dev_select_rays",
                     "rtk_amd_select_block_items", "rtk_amd_select_scan_items",
                     "rtk_dev_closest_points", "rtk_dev_closest_points_counted", "rtk_amd_closest_stack_entries",
                     "rtk_dev_scene_prepare_signs", "rtk_dev_scene_pseudonormals", "rtk_dev_signed_distances",
                     "rtk_dev_scene_prepare_winding", "rtk_dev_scene_winding_moments", "rtk_dev_winding_numbers",
                     "rtk_dev_winding_numbers_counted", "rtk_amd_winding_stack_entries",
                     "rtk_dev_world_create", "rtk_dev_world_update", "rtk_dev_world_rebuild", "rtk_dev_world_get_info", "rtk_dev_world_free",
                     "rtk_dev_world_top_scene", "rtk_dev_world_trace_status", "rtk_dev_world_trace_rays", "rtk_dev_world_trace_rays_any",
                     "rtk_dev_world_trace_rays_counted", "rtk_amd_world_stack_entries",
                     "rtk_dev_world_closest_points", "rtk_dev_world_closest_points_counted", "rtk_amd_world_closest_stack_entries",
                     "rtk_dev_world_triangles_in_box_count", "rtk_dev_world_triangles_in_box_all", "rtk_dev_world_triangles_in_box_counted",
                     "rtk_dev_world_triangles_in_obb_count", "rtk_dev_world_triangles_in_obb_all", "rtk_dev_world_triangles_in_obb_counted",
                     "rtk_dev_world_triangles_touching_count", "rtk_dev_world_triangles_touching_all",
                     "rtk_dev_world_triangles_touching_counted", "rtk_amd_world_overlap_stack_entries",
                     "rtk_dev_trace_rays_count", "rtk_dev_trace_rays_all", "rtk_amd_allhits_stack_entries",
                     "rtk_dev_triangles_within_count", "rtk_dev_triangles_within_all", "rtk_dev_triangles_within_counted",
                     "rtk_amd_within_stack_entries",
                     "rtk_dev_triangles_in_box_count", "rtk_dev_triangles_in_box_all", "rtk_dev_triangles_in_box_counted",
                     "rtk_amd_box_stack_entries",
                     "rtk_dev_triangles_in_obb_count", "rtk_dev_triangles_in_obb_all", "rtk_dev_triangles_in_obb_counted",
                     "rtk_amd_obb_stack_entries",
                     "rtk_dev_triangles_touching_count", "rtk_dev_triangles_touching_all", "rtk_dev_triangles_touching_counted",
                     "rtk_amd_touch_stack_entries",
                     "rtk_dev_closest_triangles", "rtk_dev_closest_triangles_counted", "rtk_amd_pair_stack_entries",
                     "rtk_dev_triangles_near_count", "rtk_dev_triangles_near_all", "rtk_dev_triangles_near_counted",
                     "rtk_amd_near_stack_entries",
                     "rtk_dev_sweep_spheres", "rtk_dev_sweep_spheres_any", "rtk_dev_sweep_spheres_counted",
                     "rtk_amd_sweep_stack_entries",
                     "rtk_dev_sweep_boxes", "rtk_dev_sweep_boxes_any", "rtk_dev_sweep_boxes_counted", "rtk_amd_boxsweep_stack_entries",
                     "rtk_dev_sweep_capsules", "rtk_dev_sweep_capsules_any", "rtk_dev_sweep_capsules_counted", "rtk_amd_capsule_stack_entries",
                     "rtk_dev_sweep_obbs", "rtk_dev_sweep_obbs_any", "rtk_dev_sweep_obbs_counted", "rtk_amd_obbsweep_stack_entries"]

# the four swept shapes (one walk, rtk_amd/csrc/rtk_sweep_walk.h): the name in the Python methods, the C symbol stem, the keyword
# names of the two 3-float side arrays, the query record, the symbol that tells the on-chip stack entries
Sweep = collections.namedtuple("Sweep", "name stem sides dtype stack_entries")
SWEEPS = {f.name: f for f in (
    Sweep("spheres", "rtk_dev_sweep_spheres", ("d_points", "d_centres"), SPHERE_SWEEP_DTYPE, "rtk_amd_sweep_stack_entries"),
    Sweep("boxes", "rtk_dev_sweep_boxes", ("d_centres", "d_normals"), BOX_SWEEP_DTYPE, "rtk_amd_boxsweep_stack_entries"),
    Sweep("capsules", "rtk_dev_sweep_capsules", ("d_points", "d_axis_points"), CAPSULE_SWEEP_DTYPE, "rtk_amd_capsule_stack_entries"),
    Sweep("obbs", "rtk_dev_sweep_obbs", ("d_centres", "d_normals"), OBB_SWEEP_DTYPE, "rtk_amd_obbsweep_stack_entries"))}

# the three overlap queries (one walk, rtk_amd/csrc/rtk_overlap_walk.h): the name in the Python methods (count_<name>_device,
# <name>_all_device), the C symbol stem, the symbol that tells the on-chip stack entries, whether the calls take a TouchFilter
Overlap = collections.namedtuple("Overlap", "name stem stack_entries filtered")
OVERLAPS = {f.name: f for f in (
    Overlap("in_boxes", "rtk_dev_triangles_in_box", "rtk_amd_box_stack_entries", False),
    Overlap("in_obbs", "rtk_dev_triangles_in_obb", "rtk_amd_obb_stack_entries", False),
    Overlap("touching", "rtk_dev_triangles_touching", "rtk_amd_touch_stack_entries", True))}

# ... and on a world (rtk_amd/csrc/rtk_world_overlap.hip): the name in DeviceWorld's methods (triangles_<name>_count_device, ...),
# the C symbol stem, the width of a query in floats, whether the calls take touch_flags after the world's filter
WorldOverlap = collections.namedtuple("WorldOverlap", "name stem floats flagged")
WORLD_OVERLAPS = {f.name: f for f in (
    WorldOverlap("in_box", "rtk_dev_world_triangles_in_box", 6, False),
    WorldOverlap("in_obb", "rtk_dev_world_triangles_in_obb", 15, False),
    WorldOverlap("touching", "rtk_dev_world_triangles_touching", 9, True))}

_lib = None


def lib():
    """Load librtk_amd.so (built by rtk_amd/csrc/Makefile). Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RtkError("%s not found: build it with `make -C rtk_amd/csrc` (or __graft_entry__.build()); "
                       "there is no CPU fallback" % LIB_PATH)
    # torch first: both link libamdhip64.so.7 and the process must end up with ONE HIP runtime
    # (the one torch ships); loading ours first leaves torch.cuda unusable.
    import torch  # noqa: F401
    L = C.CDLL(LIB_PATH)
    L.rtk_amd_last_error.restype = C.c_char_p
    L.rtk_amd_device_count.restype = C.c_int
    L.rtk_amd_set_device.argtypes = [C.c_int]
    L.rtk_dev_scene_upload.restype = C.c_void_p
    L.rtk_dev_scene_upload.argtypes = [C.c_void_p]
    L.rtk_dev_scene_build.restype = C.c_void_p
    L.rtk_dev_scene_build.argtypes = [C.POINTER(SceneDesc)]
    L.rtk_dev_scene_free.argtypes = [C.c_void_p]
    L.rtk_dev_scene_get_info.argtypes = [C.c_void_p, C.POINTER(SceneInfo)]
    L.rtk_dev_scene_mesh_base.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.rtk_dev_scene_primitive_order.restype = C.c_longlong
    L.rtk_dev_scene_primitive_order.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.rtk_dev_scene_export_size.restype = C.c_size_t
    L.rtk_dev_scene_export_size.argtypes = [C.c_void_p]
    L.rtk_dev_scene_export.restype = C.c_void_p
    L.rtk_dev_scene_export.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.rtk_dev_trace_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(TraceOpts), C.c_void_p]
    L.rtk_dev_trace_rays_any.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(TraceOpts), C.c_void_p]
    L.rtk_dev_expand_hits.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rtk_dev_trace_rays_packet_counted.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(TraceOpts), C.POINTER(PacketCounters)]
    L.rtk_dev_debug_packet_entries.restype = C.c_int
    L.rtk_dev_debug_packet_entries.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    L.rtk_dev_trace_rays_counted.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(TraceOpts),
                                             C.POINTER(TraceCounters)]
    L.rtk_dev_trace_rays_any_counted.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(TraceOpts),
                                                 C.POINTER(TraceCounters)]
    L.rtk_trace_rays.restype = C.c_size_t
    L.rtk_trace_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.rtk_amd_forget_scene.argtypes = [C.c_void_p]
    L.rtk_dev_scene_validate.argtypes = [C.c_void_p, C.POINTER(SceneCheck)]
    L.rtk_dev_scene_upload_buffer.restype = C.c_void_p
    L.rtk_dev_scene_upload_buffer.argtypes = [C.c_void_p, C.c_size_t]
    L.rtk_dev_trace_rays_filtered.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(DevFilter),
                                              C.POINTER(TraceOpts), C.c_void_p]
    L.rtk_dev_trace_rays_any_filtered.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(DevFilter),
                                                  C.POINTER(TraceOpts), C.c_void_p]
    L.rtk_dev_trace_status.argtypes = [C.c_void_p, C.c_void_p]
    for fn in (L.rtk_dev_trace_rays_listed, L.rtk_dev_trace_rays_any_listed):
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(RayList), C.c_void_p, C.POINTER(DevFilter), C.POINTER(TraceOpts), C.c_void_p]
        fn.restype = C.c_int
    L.rtk_dev_select_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_size_t, C.POINTER(RayList), C.c_void_p, C.c_void_p, C.c_void_p]
    L.rtk_dev_select_rays.restype = C.c_int
    L.rtk_amd_select_block_items.argtypes = []
    L.rtk_amd_select_block_items.restype = C.c_uint32
    L.rtk_amd_select_scan_items.argtypes = []
    L.rtk_amd_select_scan_items.restype = C.c_uint32
    L.rtk_dev_closest_points.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(RayList), C.c_void_p, C.c_void_p, C.c_void_p]
    L.rtk_dev_closest_points.restype = C.c_int
    L.rtk_dev_closest_points_counted.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(TraceCounters)]
    L.rtk_dev_closest_points_counted.restype = C.c_int
    L.rtk_dev_scene_prepare_signs.argtypes = [C.c_void_p, C.POINTER(SignInfo), C.c_void_p]
    L.rtk_dev_scene_prepare_signs.restype = C.c_int
    L.rtk_dev_scene_pseudonormals.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.rtk_dev_scene_pseudonormals.restype = C.c_int
    L.rtk_dev_signed_distances.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(RayList), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rtk_dev_signed_distances.restype = C.c_int
    L.rtk_amd_closest_stack_entries.argtypes = []
    L.rtk_amd_closest_stack_entries.restype = C.c_uint32
    L.rtk_dev_scene_prepare_winding.argtypes = [C.c_void_p, C.POINTER(WindingInfo), C.c_void_p]
    L.rtk_dev_scene_prepare_winding.restype = C.c_int
    L.rtk_dev_scene_winding_moments.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.rtk_dev_scene_winding_moments.restype = C.c_int
    L.rtk_dev_winding_numbers.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(RayList), C.POINTER(WindingOpts), C.c_void_p, C.c_void_p]
    L.rtk_dev_winding_numbers.restype = C.c_int
    L.rtk_dev_winding_numbers_counted.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(WindingOpts), C.c_void_p, C.POINTER(TraceCounters)]
    L.rtk_dev_winding_numbers_counted.restype = C.c_int
    L.rtk_amd_winding_stack_entries.argtypes = []
    L.rtk_amd_winding_stack_entries.restype = C.c_uint32
    L.rtk_dev_world_create.argtypes = [C.POINTER(C.c_void_p), C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(Placement), C.c_size_t]
    L.rtk_dev_world_create.restype = C.c_void_p
    L.rtk_dev_world_update.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.rtk_dev_world_update.restype = C.c_int
    L.rtk_dev_world_rebuild.argtypes = [C.c_void_p, C.c_void_p]
    L.rtk_dev_world_rebuild.restype = C.c_int
    L.rtk_dev_world_get_info.argtypes = [C.c_void_p, C.POINTER(WorldInfo)]
    L.rtk_dev_world_get_info.restype = C.c_int
    L.rtk_dev_world_free.argtypes = [C.c_void_p]
    L.rtk_dev_world_free.restype = None
    L.rtk_dev_world_top_scene.argtypes = [C.c_void_p]
    L.rtk_dev_world_top_scene.restype = C.c_void_p
    L.rtk_dev_world_trace_status.argtypes = [C.c_void_p, C.c_void_p]
    L.rtk_dev_world_trace_status.restype = C.c_int
    L.rtk_dev_world_trace_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(RayList), C.POINTER(WorldFilter), C.c_void_p, C.c_void_p, C.c_void_p]
    L.rtk_dev_world_trace_rays.restype = C.c_int
    L.rtk_dev_world_trace_rays_any.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(RayList), C.POINTER(WorldFilter), C.c_void_p, C.c_void_p]
    L.rtk_dev_world_trace_rays_any.restype = C.c_int
    L.rtk_dev_world_trace_rays_counted.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(WorldFilter), C.c_void_p, C.c_void_p, C.POINTER(TraceCounters)]
    L.rtk_dev_world_trace_rays_counted.restype = C.c_int
    L.rtk_amd_world_stack_entries.argtypes = []
    L.rtk_amd_world_stack_entries.restype = C.c_uint32
    L.rtk_dev_world_closest_points.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(RayList), C.POINTER(WorldFilter), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rtk_dev_world_closest_points.restype = C.c_int
    L.rtk_dev_world_closest_points_counted.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(WorldFilter), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(TraceCounters)]
    L.rtk_dev_world_closest_points_counted.restype = C.c_int
    L.rtk_amd_world_closest_stack_entries.argtypes = []
    L.rtk_amd_world_closest_stack_entries.restype = C.c_uint32
    for fam in WORLD_OVERLAPS.values():
        fn_count, fn_all, fn_counted = (getattr(L, fam.stem + tail) for tail in ("_count", "_all", "_counted"))
        flags = [C.c_uint32] if fam.flagged else []
        fn_count.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(RayList), C.POINTER(WorldFilter)] + flags + [C.c_void_p, C.c_void_p]
        fn_all.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(RayList), C.POINTER(WorldFilter)] + flags + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        fn_counted.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(WorldFilter)] + flags + [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(TraceCounters)]
        fn_count.restype = fn_all.restype = fn_counted.restype = C.c_int
    L.rtk_amd_world_overlap_stack_entries.argtypes = []
    L.rtk_amd_world_overlap_stack_entries.restype = C.c_uint32
    for fam in SWEEPS.values():
        fn, fn_any, fn_counted, entries = (getattr(L, name) for name in (fam.stem, fam.stem + "_any", fam.stem + "_counted", fam.stack_entries))
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(RayList), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(DevFilter), C.c_void_p]
        fn_any.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(RayList), C.c_void_p, C.POINTER(DevFilter), C.c_void_p]
        fn_counted.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(DevFilter), C.POINTER(TraceCounters)]
        fn.restype = fn_any.restype = fn_counted.restype = C.c_int
        entries.argtypes = []
        entries.restype = C.c_uint32
    L.rtk_dev_triangles_within_count.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(RayList), C.c_void_p, C.c_void_p]
    L.rtk_dev_triangles_within_count.restype = C.c_int
    L.rtk_dev_triangles_within_all.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(RayList), C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p]
    L.rtk_dev_triangles_within_all.restype = C.c_int
    L.rtk_dev_triangles_within_counted.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.POINTER(TraceCounters)]
    L.rtk_dev_triangles_within_counted.restype = C.c_int
    L.rtk_amd_within_stack_entries.argtypes = []
    L.rtk_amd_within_stack_entries.restype = C.c_uint32
    for fam in OVERLAPS.values():
        fn_count, fn_all, fn_counted, entries = (getattr(L, name) for name in (fam.stem + "_count", fam.stem + "_all", fam.stem + "_counted", fam.stack_entries))
        filt = [C.POINTER(TouchFilter)] if fam.filtered else []
        fn_count.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(RayList)] + filt + [C.c_void_p, C.c_void_p]
        fn_all.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(RayList)] + filt + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        fn_counted.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t] + filt + [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(TraceCounters)]
        fn_count.restype = fn_all.restype = fn_counted.restype = C.c_int
        entries.argtypes = []
        entries.restype = C.c_uint32
    L.rtk_dev_closest_triangles.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(RayList), C.POINTER(TouchFilter), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rtk_dev_closest_triangles.restype = C.c_int
    L.rtk_dev_closest_triangles_counted.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(TouchFilter), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(TraceCounters)]
    L.rtk_dev_closest_triangles_counted.restype = C.c_int
    L.rtk_amd_pair_stack_entries.argtypes = []
    L.rtk_amd_pair_stack_entries.restype = C.c_uint32
    L.rtk_dev_triangles_near_count.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(RayList), C.POINTER(TouchFilter), C.c_void_p, C.c_void_p, C.c_void_p]
    L.rtk_dev_triangles_near_count.restype = C.c_int
    L.rtk_dev_triangles_near_all.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(RayList), C.POINTER(TouchFilter), C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rtk_dev_triangles_near_all.restype = C.c_int
    L.rtk_dev_triangles_near_counted.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(TouchFilter), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.POINTER(TraceCounters)]
    L.rtk_dev_triangles_near_counted.restype = C.c_int
    L.rtk_amd_near_stack_entries.argtypes = []
    L.rtk_amd_near_stack_entries.restype = C.c_uint32
    L.rtk_dev_trace_rays_count.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(DevFilter), C.POINTER(TraceOpts), C.c_void_p]
    L.rtk_dev_trace_rays_count.restype = C.c_int
    L.rtk_dev_trace_rays_all.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(DevFilter), C.POINTER(TraceOpts), C.c_void_p]
    L.rtk_dev_trace_rays_all.restype = C.c_int
    L.rtk_amd_allhits_stack_entries.argtypes = []
    L.rtk_amd_allhits_stack_entries.restype = C.c_uint32
    L.rtk_trace_rays_filter.restype = C.c_size_t
    L.rtk_trace_rays_filter.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rtk_amd_shard_range.restype = None
    L.rtk_amd_shard_range.argtypes = [C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.rtk_mgpu_create.restype = C.c_void_p
    L.rtk_mgpu_create.argtypes = [C.POINTER(C.c_int), C.c_int]
    L.rtk_mgpu_destroy.restype = None
    L.rtk_mgpu_destroy.argtypes = [C.c_void_p]
    L.rtk_mgpu_num_devices.argtypes = [C.c_void_p]
    L.rtk_mgpu_scene.restype = C.c_void_p
    L.rtk_mgpu_scene.argtypes = [C.c_void_p, C.c_int]
    L.rtk_mgpu_build.argtypes = [C.c_void_p, C.POINTER(SceneDesc)]
    L.rtk_mgpu_upload.argtypes = [C.c_void_p, C.c_void_p]
    L.rtk_mgpu_refit.restype = C.c_int
    L.rtk_mgpu_refit.argtypes = [C.c_void_p, C.POINTER(SceneDesc)]
    L.rtk_dev_scene_refit.restype = C.c_int
    L.rtk_dev_scene_refit.argtypes = [C.c_void_p, C.POINTER(SceneDesc), C.c_void_p]
    L.rtk_dev_scene_last_refit_ms.restype = C.c_double
    L.rtk_dev_scene_last_refit_ms.argtypes = [C.c_void_p]
    L.rtk_dev_scene_refit_meshes.restype = C.c_int
    L.rtk_dev_scene_refit_meshes.argtypes = [C.c_void_p, C.POINTER(SceneDesc), C.POINTER(C.c_uint32), C.c_size_t, C.c_void_p]
    L.rtk_dev_scene_last_refit_nodes.restype = C.c_uint64
    L.rtk_dev_scene_last_refit_nodes.argtypes = [C.c_void_p]
    L.rtk_dev_scene_quality.restype = C.c_int
    L.rtk_dev_scene_quality.argtypes = [C.c_void_p, C.POINTER(SceneQuality), C.c_void_p]
    L.rtk_dev_scene_split_leaves.restype = C.c_int
    L.rtk_dev_scene_split_leaves.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(SplitInfo), C.c_void_p]
    L.rtk_mgpu_split_leaves.restype = C.c_int
    L.rtk_mgpu_split_leaves.argtypes = [C.c_void_p, C.c_uint32]
    L.rtk_dev_scene_rebuild.restype = C.c_int
    L.rtk_dev_scene_rebuild.argtypes = [C.c_void_p, C.POINTER(RebuildInfo), C.c_void_p]
    L.rtk_mgpu_rebuild.restype = C.c_int
    L.rtk_mgpu_rebuild.argtypes = [C.c_void_p]
    L.rtk_mgpu_refit_meshes.restype = C.c_int
    L.rtk_mgpu_refit_meshes.argtypes = [C.c_void_p, C.POINTER(SceneDesc), C.POINTER(C.c_uint32), C.c_size_t]
    L.rtk_dev_scene_build_placed.restype = C.c_void_p
    L.rtk_dev_scene_build_placed.argtypes = [C.POINTER(SceneDesc), C.POINTER(Placement)]
    L.rtk_dev_scene_refit_placed.restype = C.c_int
    L.rtk_dev_scene_refit_placed.argtypes = [C.c_void_p, C.POINTER(SceneDesc), C.POINTER(Placement), C.c_void_p]
    L.rtk_dev_scene_refit_meshes_placed.restype = C.c_int
    L.rtk_dev_scene_refit_meshes_placed.argtypes = [C.c_void_p, C.POINTER(SceneDesc), C.POINTER(Placement), C.POINTER(C.c_uint32), C.c_size_t, C.c_void_p]
    L.rtk_mgpu_build_placed.restype = C.c_int
    L.rtk_mgpu_build_placed.argtypes = [C.c_void_p, C.POINTER(SceneDesc), C.POINTER(Placement)]
    L.rtk_mgpu_refit_placed.restype = C.c_int
    L.rtk_mgpu_refit_placed.argtypes = [C.c_void_p, C.POINTER(SceneDesc), C.POINTER(Placement)]
    L.rtk_mgpu_refit_meshes_placed.restype = C.c_int
    L.rtk_mgpu_refit_meshes_placed.argtypes = [C.c_void_p, C.POINTER(SceneDesc), C.POINTER(Placement), C.POINTER(C.c_uint32), C.c_size_t]
    L.rtk_mgpu_trace_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(TraceOpts)]
    L.rtk_mgpu_trace_rays_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(TraceOpts)]
    L.rtk_mgpu_trace_rays_device_striped.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(TraceOpts)]
    L.rtk_mgpu_striped_segment.restype = None
    L.rtk_mgpu_striped_segment.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.rtk_trace_ray_filter.restype = C.c_bool
    L.rtk_trace_ray_filter.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.rtk_amd_release_workspace.restype = None
    L.rtk_build_scene.restype = C.c_void_p
    L.rtk_build_scene.argtypes = [C.POINTER(SceneDesc)]
    L.rtk_free_scene.argtypes = [C.c_void_p]
    L.rtk_trace_ray.restype = C.c_bool
    L.rtk_trace_ray.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.rtk_start_build.restype = C.c_void_p
    L.rtk_start_build.argtypes = [C.POINTER(SceneDesc), C.c_void_p]
    L.rtk_run_task.restype = C.c_size_t
    L.rtk_run_task.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.rtk_get_build_size.restype = C.c_size_t
    L.rtk_get_build_size.argtypes = [C.c_void_p]
    L.rtk_finish_build_to.restype = C.c_void_p
    L.rtk_finish_build_to.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.rtk_finish_build.restype = C.c_void_p
    L.rtk_finish_build.argtypes = [C.c_void_p]
    _lib = L
    return L


def last_error():
    return lib().rtk_amd_last_error().decode("utf-8", "replace")


def _check(rc, what):
    if rc != 0:
        raise RtkError("%s failed (%d): %s" % (what, rc, last_error()))


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise RtkError("no GPU visible to torch: the rtk_amd trace path has no CPU fallback")
    return torch


def _stream_ptr():
    return C.c_void_p(_torch().cuda.current_stream().cuda_stream)


def to_device(a):
    """numpy structured/plain array -> uint8 cuda tensor holding the same bytes."""
    torch = _torch()
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda()


def make_opts(image=None, static=False, refill_min=0, blocks_per_cu=0, node_exit=0, no_packet=False, sort_rays=False, exact_nodes=False,
              no_asm=False, no_entries=False, no_beam=False, one_tile_beam=False, no_detect=False):
    o = TraceOpts()
    o.struct_size = C.sizeof(TraceOpts)
    o.flags = (RTK_TRACE_STATIC if static else 0) | (RTK_TRACE_NO_PACKET if no_packet else 0) | (RTK_TRACE_SORT_RAYS if sort_rays else 0)
    if exact_nodes:
        o.flags |= RTK_TRACE_EXACT_NODES
    if no_asm:
        o.flags |= RTK_TRACE_NO_ASM
    if no_entries:
        o.flags |= 32      # RTK_TRACE_NO_ENTRIES
    if no_beam:
        o.flags |= 64      # RTK_TRACE_NO_BEAM
    if one_tile_beam:
        o.flags |= 128     # RTK_TRACE_ONE_TILE_BEAM
    if no_detect:
        o.flags |= 256     # RTK_TRACE_NO_DETECT
    if image:
        o.image_width, o.image_height = int(image[0]), int(image[1])
    o.refill_min = refill_min
    o.blocks_per_cu = blocks_per_cu
    o.node_exit = node_exit
    return o


def mesh_set_of_some(meshes, mesh_base):
    """A MeshSet in which the entries of `meshes` that are None describe their mesh by its triangle count alone
    (mesh_base: the scene's prefix sums) and have no positions: what rtk_dev_scene_refit_meshes takes for meshes it is
    not asked to move."""
    empty = np.zeros((0, 3), np.float32)
    ms = MeshSet([m if m is not None else dict(positions=empty) for m in meshes])
    for i, m in enumerate(meshes):
        if m is None and i + 1 < len(mesh_base):
            ms._arr[i].num_triangles = int(mesh_base[i + 1] - mesh_base[i])
            ms._arr[i].position.data = None
    return ms


def placement_ptr(placements, num_meshes):
    """(rtk_placement pointer, the array it points into) for array-like placements of shape (num_meshes, 3, 4) or (num_meshes, 12)."""
    a = placement_array(placements, num_meshes)
    return a.ctypes.data_as(C.POINTER(Placement)), a


class DeviceScene:
    """A device-resident scene (rtk_dev_scene*)."""

    def __init__(self, handle, keepalive=None):
        if not handle:
            raise RtkError("scene creation failed: " + last_error())
        self.handle = C.c_void_p(handle)
        self._keep = keepalive

    @classmethod
    def upload(cls, blob):
        """blob: bytes-like / numpy uint8 / object with .ptr -- a scene blob in rtk format."""
        _torch()
        if hasattr(blob, "ptr"):
            return cls(lib().rtk_dev_scene_upload_buffer(C.c_void_p(blob.ptr), blob.size), blob)
        arr = np.frombuffer(blob, dtype=np.uint8) if not isinstance(blob, np.ndarray) else blob
        arr = np.ascontiguousarray(arr)
        return cls(lib().rtk_dev_scene_upload_buffer(C.c_void_p(arr.ctypes.data), arr.size), arr)

    @classmethod
    def build(cls, meshes, placements=None):
        """Device LBVH build from mesh dicts (see rtk_amd.types.MeshSet). placements: one 3 x 4 matrix per mesh, array-like
        (num_meshes, 3, 4) or (num_meshes, 12) float32 -- the meshes are in their rest pose and every vertex is moved by
        its mesh's matrix as it is read (rtk_dev_scene_build_placed); two meshes may share buffers (instances)."""
        _torch()
        ms = meshes if isinstance(meshes, MeshSet) else MeshSet(meshes)
        if placements is None:
            return cls(lib().rtk_dev_scene_build(C.byref(ms.desc)), ms)
        ptr, _keep = placement_ptr(placements, int(ms.desc.num_meshes))
        return cls(lib().rtk_dev_scene_build_placed(C.byref(ms.desc), ptr), ms)

    def refit(self, meshes, only=None, placements=None):
        """New vertex positions for the same triangles, in place (rtk_dev_scene_refit): meshes as for build(); only the
        positions are read. Synchronous; the scene must not be traced from another stream or thread meanwhile.
        only: a list of mesh indices (rtk_dev_scene_refit_meshes) -- just those meshes are read and moved, at a cost that
        follows them; the entries of `meshes` that are not listed may be None.
        placements: as for build() (rtk_dev_scene_refit_placed / rtk_dev_scene_refit_meshes_placed): one matrix per mesh of
        the scene, of which only those of the meshes that are read count."""
        _torch()
        if only is None:
            ms = meshes if isinstance(meshes, MeshSet) else MeshSet(meshes)
            if placements is None:
                _check(lib().rtk_dev_scene_refit(self.handle, C.byref(ms.desc), _stream_ptr()), "rtk_dev_scene_refit")
                return
            ptr, _keep = placement_ptr(placements, int(ms.desc.num_meshes))
            _check(lib().rtk_dev_scene_refit_placed(self.handle, C.byref(ms.desc), ptr, _stream_ptr()), "rtk_dev_scene_refit_placed")
            return
        ms = meshes if isinstance(meshes, MeshSet) else mesh_set_of_some(meshes, self.mesh_base())
        ids = np.ascontiguousarray(only, np.uint32).reshape(-1)
        id_ptr = ids.ctypes.data_as(C.POINTER(C.c_uint32)) if ids.size else None
        if placements is None:
            _check(lib().rtk_dev_scene_refit_meshes(self.handle, C.byref(ms.desc), id_ptr, ids.size, _stream_ptr()), "rtk_dev_scene_refit_meshes")
            return
        ptr, _keep = placement_ptr(placements, int(ms.desc.num_meshes))
        _check(lib().rtk_dev_scene_refit_meshes_placed(self.handle, C.byref(ms.desc), ptr, id_ptr, ids.size, _stream_ptr()),
               "rtk_dev_scene_refit_meshes_placed")

    def last_refit_ms(self):
        return float(lib().rtk_dev_scene_last_refit_ms(self.handle))

    def last_refit_nodes(self):
        """Nodes whose boxes the last successful refit remade (rtk_dev_scene_last_refit_nodes)."""
        return int(lib().rtk_dev_scene_last_refit_nodes(self.handle))

    def quality(self):
        """The SAH cost of the tree as it is now (rtk_dev_scene_quality), measured on the device on the current stream: the
        fields of rtk_dev_scene_quality_info as a dict, plus ratio = sah_cost / sah_cost_at_build (None while the scene has
        no cost from before its first refit: call once right after build() or upload()). Reads only; deterministic."""
        _torch()
        q = SceneQuality()
        q.struct_size = C.sizeof(SceneQuality)
        _check(lib().rtk_dev_scene_quality(self.handle, C.byref(q), _stream_ptr()), "rtk_dev_scene_quality")
        d = q.as_dict()
        d["ratio"] = d["sah_cost"] / d["sah_cost_at_build"] if d["sah_cost_at_build"] != 0.0 else None
        return d

    def split_leaves(self, max_leaf=0):
        """Every leaf of more than max_leaf triangles becomes a small subtree with leaves of at most max_leaf
        (rtk_dev_scene_split_leaves), in place, on the current stream; 0 = the device builder's limit (3). What an uploaded
        blob wants before it is traced many times. Returns the fields of rtk_dev_split_info as a dict. Synchronous; the
        scene must not be traced from another stream or thread meanwhile."""
        if not 0 <= int(max_leaf) <= 63:
            raise RtkError("split_leaves: max_leaf %r (0 = the device builder's limit, else 1 .. 63)" % (max_leaf,))
        _torch()
        s = SplitInfo()
        s.struct_size = C.sizeof(SplitInfo)
        _check(lib().rtk_dev_scene_split_leaves(self.handle, int(max_leaf), C.byref(s), _stream_ptr()), "rtk_dev_scene_split_leaves")
        return s.as_dict()

    def rebuild(self):
        """The device builder's tree over the triangles the scene holds now (rtk_dev_scene_rebuild), in place: what build()
        of the current positions would return, under the same handle. For a scene whose tree has degraded under refits
        (quality()["ratio"]) and for an uploaded blob, which has no description to build from. Returns the fields of
        rtk_dev_rebuild_info as a dict. Synchronous; the scene must not be traced from another stream or thread meanwhile."""
        _torch()
        r = RebuildInfo()
        r.struct_size = C.sizeof(RebuildInfo)
        _check(lib().rtk_dev_scene_rebuild(self.handle, C.byref(r), _stream_ptr()), "rtk_dev_scene_rebuild")
        return r.as_dict()

    def free(self):
        if self.handle:
            lib().rtk_dev_scene_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def info(self):
        i = SceneInfo()
        _check(lib().rtk_dev_scene_get_info(self.handle, C.byref(i)), "rtk_dev_scene_get_info")
        return i.as_dict()

    def validate(self):
        """Device-side structural check; returns (ok, counts dict)."""
        c = SceneCheck()
        rc = lib().rtk_dev_scene_validate(self.handle, C.byref(c))
        if rc not in (0, -5):
            raise RtkError("rtk_dev_scene_validate failed (%d): %s" % (rc, last_error()))
        return rc == 0, c.as_dict()

    def mesh_base(self):
        n = self.info()["num_meshes"] + 1
        out = np.zeros(n, np.uint64)
        rc = lib().rtk_dev_scene_mesh_base(self.handle, out.ctypes.data, n)
        if rc < 0:
            raise RtkError(last_error())
        return out

    def primitive_order(self):
        n = self.info()["num_triangles"]
        out = np.zeros(max(n, 1), np.uint32)
        rc = lib().rtk_dev_scene_primitive_order(self.handle, out.ctypes.data, out.size)
        if rc < 0:
            raise RtkError(last_error())
        return out[:n]

    def export_blob(self):
        size = lib().rtk_dev_scene_export_size(self.handle)
        if size == 0:
            raise RtkError("rtk_dev_scene_export_size: " + last_error())
        raw = np.zeros(size + 128, np.uint8)
        off = (-raw.ctypes.data) % 128
        buf = raw[off:off + size]
        if not lib().rtk_dev_scene_export(self.handle, buf.ctypes.data, size):
            raise RtkError("rtk_dev_scene_export: " + last_error())
        return buf

    # -- device-pointer batch calls (tensors are uint8 cuda tensors) --

    def trace_device(self, d_rays, n, d_records=None, opts=None):
        torch = _torch()
        if d_records is None:
            d_records = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
        _check(lib().rtk_dev_trace_rays(self.handle, C.c_void_p(d_rays.data_ptr()), n, C.c_void_p(d_records.data_ptr()),
                                        C.byref(opts) if opts is not None else None, _stream_ptr()), "rtk_dev_trace_rays")
        return d_records

    def trace_any_device(self, d_rays, n, d_occluded=None, opts=None):
        torch = _torch()
        if d_occluded is None:
            d_occluded = torch.empty(n, dtype=torch.uint8, device="cuda")
        _check(lib().rtk_dev_trace_rays_any(self.handle, C.c_void_p(d_rays.data_ptr()), n, C.c_void_p(d_occluded.data_ptr()),
                                            C.byref(opts) if opts is not None else None, _stream_ptr()), "rtk_dev_trace_rays_any")
        return d_occluded

    # -- ray lists: which rays are traced is decided on the device (rtk_ray_list); nothing here waits for the stream --

    def trace_listed_device(self, d_rays, num_rays, count, ids=None, d_records=None, filter=None, opts=None):
        """Closest hits of the first min(count[0], num_rays) rays that `ids` names (None: of the rays themselves), written to the
        rays' own slots of d_records; slots that are not listed are not written. count, ids: cuda int64 tensors."""
        torch = _torch()
        if d_records is None:
            d_records = torch.empty(num_rays * 16, dtype=torch.uint8, device="cuda")
        l = make_ray_list(count, ids)
        _check(lib().rtk_dev_trace_rays_listed(self.handle, C.c_void_p(d_rays.data_ptr()), num_rays, C.byref(l), C.c_void_p(d_records.data_ptr()),
                                               C.byref(filter) if filter is not None else None, C.byref(opts) if opts is not None else None,
                                               _stream_ptr()), "rtk_dev_trace_rays_listed")
        return d_records

    def trace_any_listed_device(self, d_rays, num_rays, count, ids=None, d_occluded=None, filter=None, opts=None):
        """The any-hit form of trace_listed_device: one byte per ray, in the rays' own slots."""
        torch = _torch()
        if d_occluded is None:
            d_occluded = torch.empty(num_rays, dtype=torch.uint8, device="cuda")
        l = make_ray_list(count, ids)
        _check(lib().rtk_dev_trace_rays_any_listed(self.handle, C.c_void_p(d_rays.data_ptr()), num_rays, C.byref(l), C.c_void_p(d_occluded.data_ptr()),
                                                   C.byref(filter) if filter is not None else None, C.byref(opts) if opts is not None else None,
                                                   _stream_ptr()), "rtk_dev_trace_rays_any_listed")
        return d_occluded

    def select_rays(self, src, kind, num_rays, in_ids=None, in_count=None):
        """The rays of 0 .. num_rays - 1 (or of the list in_ids / in_count, in its order) whose element of `src` -- hit records for
        SELECT_RECORD_*, bytes for SELECT_BYTE_* -- matches `kind`. Returns (ids, count): cuda int64 tensors of num_rays and 1
        entries; ids beyond count[0] are not written."""
        torch = _torch()
        ids = torch.empty(max(num_rays, 1), dtype=torch.int64, device="cuda")
        count = torch.empty(1, dtype=torch.int64, device="cuda")
        if in_ids is not None and in_count is None:
            raise RtkError("select_rays: in_ids without in_count (a list's length lives on the device)")
        l = make_ray_list(in_count, in_ids) if in_count is not None else None
        _check(lib().rtk_dev_select_rays(self.handle, C.c_void_p(src.data_ptr()), kind, num_rays, C.byref(l) if l is not None else None,
                                         C.c_void_p(ids.data_ptr()), C.c_void_p(count.data_ptr()), _stream_ptr()), "rtk_dev_select_rays")
        return ids, count

    # -- closest points (rtk_dev_closest_points): asynchronous on the current stream, nothing here waits for it --

    def closest_points_device(self, d_queries, n, d_records=None, d_points=None, count=None, ids=None, want_points=True):
        """The nearest triangle to each of n queries (POINT_QUERY_DTYPE bytes on the device): returns (d_records, d_points), uint8
        cuda tensors of CLOSEST_RECORD_DTYPE records and of 3 floats per query. want_points=False: no points are written (the
        call gets NULL for them and None is returned). count / ids: cuda int64 tensors naming the queries to answer, as for trace_listed_device;
        slots that are not listed are not written."""
        torch = _torch()
        if d_records is None:
            d_records = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
        if not want_points:
            d_points = None
        elif d_points is None:
            d_points = torch.empty(n * 12, dtype=torch.uint8, device="cuda")
        if ids is not None and count is None:
            raise RtkError("closest_points_device: ids without count (a list's length lives on the device)")
        l = make_ray_list(count, ids) if count is not None else None
        _check(lib().rtk_dev_closest_points(self.handle, C.c_void_p(d_queries.data_ptr()), n, C.byref(l) if l is not None else None,
                                            C.c_void_p(d_records.data_ptr()), C.c_void_p(d_points.data_ptr()) if d_points is not None else None,
                                            _stream_ptr()), "rtk_dev_closest_points")
        return d_records, d_points

    def closest_points_counted(self, d_queries, n):
        """closest_points_device of all n queries on the null stream, synchronous, with the visit counts of
        rtk_dev_closest_points_counted: returns (d_records, d_points, counts dict)."""
        torch = _torch()
        d_records = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
        d_points = torch.empty(n * 12, dtype=torch.uint8, device="cuda")
        ctr = TraceCounters()
        torch.cuda.synchronize()
        _check(lib().rtk_dev_closest_points_counted(self.handle, C.c_void_p(d_queries.data_ptr()), n, C.c_void_p(d_records.data_ptr()),
                                                    C.c_void_p(d_points.data_ptr()), C.byref(ctr)), "rtk_dev_closest_points_counted")
        return d_records, d_points, ctr.as_dict()

    def closest_points(self, points, max_dist=None):
        """points: array-like (n, 3) float32. max_dist: a distance (scalar or one per point) beyond which a triangle does not
        count, squared in float32; None = no limit (RTK_INF). Returns (records CLOSEST_RECORD_DTYPE, points (n, 3) float32):
        prim == 0xFFFFFFFF is a miss, whose point is the query itself."""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        n = pts.shape[0]
        q = np.zeros(n, POINT_QUERY_DTYPE)
        q["point"] = pts
        if max_dist is None:
            q["max_dist2"] = RTK_INF
        else:
            d = np.broadcast_to(np.asarray(max_dist, np.float32), (n,))
            with np.errstate(over="ignore", invalid="ignore"):
                q["max_dist2"] = d * d
        if n == 0:
            return np.zeros(0, CLOSEST_RECORD_DTYPE), np.zeros((0, 3), np.float32)
        d_rec, d_pts = self.closest_points_device(to_device(q), n)
        _check(lib().rtk_dev_trace_status(self.handle, _stream_ptr()), "rtk_dev_trace_status")
        return d_rec.cpu().numpy().view(CLOSEST_RECORD_DTYPE), d_pts.cpu().numpy().view(np.float32).reshape(n, 3)

    # -- signed distances (rtk_dev_signed_distances): the closest-point call and the side of the surface --

    def prepare_signs(self):
        """Makes the scene's table of pseudonormals now if it is not there (rtk_dev_scene_prepare_signs, on the current stream)
        and returns the fields of rtk_dev_sign_info as a dict, plus closed = no boundary, non-manifold or inconsistent side:
        whether the sign of a distance means anything. table_ms is 0 when the table was found made."""
        _torch()
        s = SignInfo()
        _check(lib().rtk_dev_scene_prepare_signs(self.handle, C.byref(s), _stream_ptr()), "rtk_dev_scene_prepare_signs")
        d = s.as_dict()
        d["closed"] = d["boundary_sides"] == 0 and d["nonmanifold_sides"] == 0 and d["inconsistent_sides"] == 0
        return d

    def pseudonormals(self):
        """The table as a float32 cuda tensor (num_prims, 18): per primitive the edge normals of ab, ac, bc, then the vertex
        normals of a, b, c (rtk_dev_scene_pseudonormals). Made on first use."""
        torch = _torch()
        n = self.info()["num_triangles"]
        out = torch.empty((n, 18), dtype=torch.float32, device="cuda")
        _check(lib().rtk_dev_scene_pseudonormals(self.handle, C.c_void_p(out.data_ptr()), _stream_ptr()), "rtk_dev_scene_pseudonormals")
        return out

    def signed_distances_device(self, d_queries, n, d_records=None, d_points=None, d_signed=None, count=None, ids=None, want_records=True, want_points=True):
        """closest_points_device plus the signed distance of every answered query: returns (d_signed, d_records, d_points) --
        a float32 cuda tensor of n entries, negative inside, RTK_INF for a miss, and the two tensors of closest_points_device
        (None for the one that want_records=False or want_points=False leaves out: the call gets NULL for it). count / ids as
        there; slots that are not listed are not written. Nothing waits for the stream, except the one call that makes the table."""
        torch = _torch()
        if not want_records:
            d_records = None
        elif d_records is None:
            d_records = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
        if not want_points:
            d_points = None
        elif d_points is None:
            d_points = torch.empty(n * 12, dtype=torch.uint8, device="cuda")
        if d_signed is None:
            d_signed = torch.empty(n, dtype=torch.float32, device="cuda")
        if ids is not None and count is None:
            raise RtkError("signed_distances_device: ids without count (a list's length lives on the device)")
        l = make_ray_list(count, ids) if count is not None else None
        _check(lib().rtk_dev_signed_distances(self.handle, C.c_void_p(d_queries.data_ptr()), n, C.byref(l) if l is not None else None,
                                              C.c_void_p(d_records.data_ptr()) if d_records is not None else None,
                                              C.c_void_p(d_points.data_ptr()) if d_points is not None else None,
                                              C.c_void_p(d_signed.data_ptr()), _stream_ptr()), "rtk_dev_signed_distances")
        return d_signed, d_records, d_points

    def signed_distances(self, points, max_dist=None):
        """points: array-like or tensor (n, 3) float32; max_dist as for closest_points. Returns cuda tensors (signed (n,) float32
        -- negative inside, RTK_INF where no triangle is within max_dist --, prim (n,) int64 with -1 for a miss, points (n, 3)
        float32: the closest points)."""
        torch = _torch()
        pts = points.detach().cpu().numpy() if hasattr(points, "detach") else points
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
        n = pts.shape[0]
        q = np.zeros(n, POINT_QUERY_DTYPE)
        q["point"] = pts
        if max_dist is None:
            q["max_dist2"] = RTK_INF
        else:
            d = np.broadcast_to(np.asarray(max_dist, np.float32), (n,))
            with np.errstate(over="ignore", invalid="ignore"):
                q["max_dist2"] = d * d
        if n == 0:
            return (torch.empty(0, dtype=torch.float32, device="cuda"), torch.empty(0, dtype=torch.int64, device="cuda"),
                    torch.empty((0, 3), dtype=torch.float32, device="cuda"))
        d_signed, d_rec, d_pts = self.signed_distances_device(to_device(q), n)
        _check(lib().rtk_dev_trace_status(self.handle, _stream_ptr()), "rtk_dev_trace_status")
        prim = d_rec.view(torch.int32).view(n, 4)[:, 3].to(torch.int64)
        return d_signed, prim, d_pts.view(torch.float32).view(n, 3)

    def contains_signed(self, points):
        """A bool cuda tensor: signed_distances(points)[0] < 0. Meaningful on a closed scene (prepare_signs()["closed"]). (contains()
        is the older crossing-parity route through count_hits and stays as it is; this one does not flip at grazed edges.)"""
        return self.signed_distances(points)[0] < 0

    # -- winding numbers (rtk_dev_winding_numbers): the inside test that survives holes, cracks and duplicated shells --

    def prepare_winding(self):
        """Makes the scene's table of winding moments now if it is not there (rtk_dev_scene_prepare_winding, on the current
        stream) and returns the fields of rtk_dev_winding_info as a dict. table_ms is 0 when the table was found made."""
        _torch()
        s = WindingInfo()
        _check(lib().rtk_dev_scene_prepare_winding(self.handle, C.byref(s), _stream_ptr()), "rtk_dev_scene_prepare_winding")
        return s.as_dict()

    def winding_moments(self):
        """The table as a float32 cuda tensor (nodes, 8, 4): per node the rows Nx Ny Nz Px Py Pz R of its four child slots, then
        the node's four child words (view the last row as int32). Made on first use (rtk_dev_scene_winding_moments)."""
        torch = _torch()
        n = self.prepare_winding()["nodes"]
        out = torch.empty((n, 8, 4), dtype=torch.float32, device="cuda")
        _check(lib().rtk_dev_scene_winding_moments(self.handle, C.c_void_p(out.data_ptr()), _stream_ptr()), "rtk_dev_scene_winding_moments")
        return out

    def winding_numbers_device(self, d_queries, n, d_winding=None, count=None, ids=None, beta=2.0, exact=False):
        """The winding number of each of n queries (POINT_QUERY_DTYPE bytes on the device; max_dist2 is not read): returns
        d_winding, a float32 cuda tensor of n entries. count / ids as for closest_points_device; slots that are not listed are
        not written. exact: RTK_WINDING_EXACT, every triangle is summed. Nothing waits for the stream, except the one call that
        makes the table."""
        torch = _torch()
        if d_winding is None:
            d_winding = torch.empty(n, dtype=torch.float32, device="cuda")
        if ids is not None and count is None:
            raise RtkError("winding_numbers_device: ids without count (a list's length lives on the device)")
        l = make_ray_list(count, ids) if count is not None else None
        o = make_winding_opts(beta, exact)
        _check(lib().rtk_dev_winding_numbers(self.handle, C.c_void_p(d_queries.data_ptr()), n, C.byref(l) if l is not None else None,
                                             C.byref(o), C.c_void_p(d_winding.data_ptr()), _stream_ptr()), "rtk_dev_winding_numbers")
        return d_winding

    def winding_numbers_counted(self, d_queries, n, beta=2.0, exact=False):
        """winding_numbers_device of all n queries on the null stream, synchronous, with the visit counts of
        rtk_dev_winding_numbers_counted (nodes: table records fetched; hits: far terms taken): returns (d_winding, counts dict)."""
        torch = _torch()
        d_winding = torch.empty(n, dtype=torch.float32, device="cuda")
        ctr = TraceCounters()
        o = make_winding_opts(beta, exact)
        torch.cuda.synchronize()
        _check(lib().rtk_dev_winding_numbers_counted(self.handle, C.c_void_p(d_queries.data_ptr()), n, C.byref(o),
                                                     C.c_void_p(d_winding.data_ptr()), C.byref(ctr)), "rtk_dev_winding_numbers_counted")
        return d_winding, ctr.as_dict()

    def winding_numbers(self, points, beta=2.0, exact=False):
        """points: array-like or tensor (n, 3) float32. Returns the generalized winding numbers as a numpy float32 array (n,): 1
        inside and 0 outside a closed surface wound outwards, k inside k nested shells, -1 inside a shell wound inwards, a
        fraction near a hole; NaN for a point with a non-finite coordinate."""
        pts = points.detach().cpu().numpy() if hasattr(points, "detach") else points
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
        n = pts.shape[0]
        if n == 0:
            return np.zeros(0, np.float32)
        q = np.zeros(n, POINT_QUERY_DTYPE)
        q["point"] = pts
        q["max_dist2"] = RTK_INF
        d_w = self.winding_numbers_device(to_device(q), n, beta=beta, exact=exact)
        _check(lib().rtk_dev_trace_status(self.handle, _stream_ptr()), "rtk_dev_trace_status")
        return d_w.cpu().numpy()

    def contains_winding(self, points, beta=2.0):
        """A numpy bool array: winding_numbers(points, beta) > 0.5. A shell wound INWARDS gives -1 inside and is therefore
        "outside"; k nested shells give k and are inside. Prefer this over contains_signed and contains when the mesh may have
        holes, cracks, duplicated or overlapping shells or inconsistent patches (scans, game assets, CAD exports): the winding
        number degrades smoothly there, where the pseudonormal's sign and the crossing parity mean nothing near the defect. On a
        closed, consistently wound mesh contains_signed is cheaper (one nearest-triangle walk, and it gives the distance too)
        and contains needs no table at all."""
        return self.winding_numbers(points, beta=beta) > 0.5

    # -- swept shapes (rtk_dev_sweep_spheres / _boxes / _capsules / _obbs, each with _any and _counted; a row of SWEEPS each):
    # asynchronous on the current stream, nothing here waits for it --

    def _sweep_filter(self, n, mesh_mask, ignore_prim):
        """(DevFilter or None, the tensors it points into). mesh_mask: bools per mesh; ignore_prim: a cuda tensor of n 32-bit
        words (used as it is) or array-like of n ids, one per query slot."""
        if ignore_prim is not None and hasattr(ignore_prim, "data_ptr"):
            f, keep = self._device_filter(n, mesh_mask, None, None)
            if f is None:
                f = DevFilter()
                f.struct_size = C.sizeof(DevFilter)
            f.d_ignore_prim = ignore_prim.data_ptr()
            return f, keep + [ignore_prim]
        return self._device_filter(n, mesh_mask, ignore_prim, None)

    def _sweep_device(self, fam, d_sweeps, n, d_records, d_side0, d_side1, count, ids, mesh_mask, ignore_prim):
        """sweep_<fam.name>_device; the two side arrays are fam.sides, in that order"""
        torch = _torch()
        if d_records is None:
            d_records = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
        if d_side0 is None:
            d_side0 = torch.empty(n * 12, dtype=torch.uint8, device="cuda")
        if d_side1 is None:
            d_side1 = torch.empty(n * 12, dtype=torch.uint8, device="cuda")
        if ids is not None and count is None:
            raise RtkError("sweep_%s_device: ids without count (a list's length lives on the device)" % fam.name)
        l = make_ray_list(count, ids) if count is not None else None
        f, _keep = self._sweep_filter(n, mesh_mask, ignore_prim)
        _check(getattr(lib(), fam.stem)(self.handle, C.c_void_p(d_sweeps.data_ptr()), n, C.byref(l) if l is not None else None,
                                        C.c_void_p(d_records.data_ptr()), C.c_void_p(d_side0.data_ptr()), C.c_void_p(d_side1.data_ptr()),
                                        C.byref(f) if f is not None else None, _stream_ptr()), fam.stem)
        return d_records, d_side0, d_side1

    def _sweep_any_device(self, fam, d_sweeps, n, d_blocked, count, ids, mesh_mask, ignore_prim):
        """sweep_<fam.name>_any_device"""
        torch = _torch()
        if d_blocked is None:
            d_blocked = torch.empty(n, dtype=torch.uint8, device="cuda")
        if ids is not None and count is None:
            raise RtkError("sweep_%s_any_device: ids without count (a list's length lives on the device)" % fam.name)
        l = make_ray_list(count, ids) if count is not None else None
        f, _keep = self._sweep_filter(n, mesh_mask, ignore_prim)
        _check(getattr(lib(), fam.stem + "_any")(self.handle, C.c_void_p(d_sweeps.data_ptr()), n, C.byref(l) if l is not None else None,
                                                 C.c_void_p(d_blocked.data_ptr()), C.byref(f) if f is not None else None, _stream_ptr()),
               fam.stem + "_any")
        return d_blocked

    def _sweep_counted(self, fam, d_sweeps, n, mesh_mask, ignore_prim):
        """sweep_<fam.name>_counted"""
        torch = _torch()
        d_records = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
        d_side0 = torch.empty(n * 12, dtype=torch.uint8, device="cuda")
        d_side1 = torch.empty(n * 12, dtype=torch.uint8, device="cuda")
        ctr = TraceCounters()
        f, _keep = self._sweep_filter(n, mesh_mask, ignore_prim)
        torch.cuda.synchronize()
        _check(getattr(lib(), fam.stem + "_counted")(self.handle, C.c_void_p(d_sweeps.data_ptr()), n, C.c_void_p(d_records.data_ptr()),
                                                     C.c_void_p(d_side0.data_ptr()), C.c_void_p(d_side1.data_ptr()),
                                                     C.byref(f) if f is not None else None, C.byref(ctr)), fam.stem + "_counted")
        return d_records, d_side0, d_side1, ctr.as_dict()

    @staticmethod
    def _sweep_array(fam, origins, directions, max_t, min_t, **fields):
        """fam.dtype records: the path, and every other field (scalars or one per query) by its name"""
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        n = o.shape[0]
        s = np.zeros(n, fam.dtype)
        s["origin"] = o
        s["direction"] = np.broadcast_to(np.asarray(directions, np.float32), (n, 3))
        s["min_t"] = np.broadcast_to(np.asarray(min_t, np.float32), (n,))
        s["max_t"] = RTK_INF if max_t is None else np.broadcast_to(np.asarray(max_t, np.float32), (n,))
        for name, value in fields.items():
            s[name] = np.broadcast_to(np.asarray(value, np.float32), s[name].shape)
        return s

    def _sweep_host(self, fam, s, mesh_mask, ignore_prim):
        """The closest form of host records s: (records, side array 0, side array 1) as numpy arrays"""
        n = s.shape[0]
        if n == 0:
            return np.zeros(0, HIT_RECORD_DTYPE), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32)
        d_rec, d_0, d_1 = self._sweep_device(fam, to_device(s), n, None, None, None, None, None, mesh_mask, ignore_prim)
        _check(lib().rtk_dev_trace_status(self.handle, _stream_ptr()), "rtk_dev_trace_status")
        return (d_rec.cpu().numpy().view(HIT_RECORD_DTYPE), d_0.cpu().numpy().view(np.float32).reshape(n, 3),
                d_1.cpu().numpy().view(np.float32).reshape(n, 3))

    def _sweep_blocked_host(self, fam, s, mesh_mask, ignore_prim):
        """The any-hit form of host records s: a bool array"""
        n = s.shape[0]
        if n == 0:
            return np.zeros(0, bool)
        d_blocked = self._sweep_any_device(fam, to_device(s), n, None, None, None, mesh_mask, ignore_prim)
        _check(lib().rtk_dev_trace_status(self.handle, _stream_ptr()), "rtk_dev_trace_status")
        return d_blocked.cpu().numpy() != 0

    def sweep_spheres_device(self, d_sweeps, n, d_records=None, d_points=None, d_centres=None, count=None, ids=None, mesh_mask=None,
                             ignore_prim=None):
        """The first contact of each of n moving balls (SPHERE_SWEEP_DTYPE bytes on the device; include/rtk_amd.h, "Sphere
        sweeps") with the scene: returns (d_records, d_points, d_centres), uint8 cuda tensors of HIT_RECORD_DTYPE records and of 3
        floats per query each (the contact point on the triangle, the ball's centre at the contact). count / ids: cuda int64
        tensors naming the queries to answer, as for closest_points_device; slots that are not listed are not written. mesh_mask:
        bools per mesh; ignore_prim: one id per query slot (a cuda tensor, or array-like)."""
        return self._sweep_device(SWEEPS["spheres"], d_sweeps, n, d_records, d_points, d_centres, count, ids, mesh_mask, ignore_prim)

    def sweep_spheres_any_device(self, d_sweeps, n, d_blocked=None, count=None, ids=None, mesh_mask=None, ignore_prim=None):
        """The any-hit form of sweep_spheres_device: one byte per query, 1 where the path is blocked, in the queries' own slots."""
        return self._sweep_any_device(SWEEPS["spheres"], d_sweeps, n, d_blocked, count, ids, mesh_mask, ignore_prim)

    def sweep_spheres_counted(self, d_sweeps, n, mesh_mask=None, ignore_prim=None):
        """sweep_spheres_device of all n queries on the null stream, synchronous, with the visit counts of
        rtk_dev_sweep_spheres_counted: returns (d_records, d_points, d_centres, counts dict)."""
        return self._sweep_counted(SWEEPS["spheres"], d_sweeps, n, mesh_mask, ignore_prim)

    def sweep_spheres(self, origins, directions, radius, max_t=None, min_t=0.0, mesh_mask=None, ignore_prim=None):
        """origins: array-like (n, 3) float32; directions (n, 3) or (3,), not necessarily normalised: t is in their units;
        radius, max_t, min_t: scalars or one per query; max_t None = no limit (RTK_INF). Returns (records HIT_RECORD_DTYPE,
        contact points (n, 3) float32, centres at the contact (n, 3) float32): prim == 0xFFFFFFFF is a miss, whose t is max_t and
        whose two points are the origin."""
        fam = SWEEPS["spheres"]
        return self._sweep_host(fam, self._sweep_array(fam, origins, directions, max_t, min_t, radius=radius), mesh_mask, ignore_prim)

    def path_blocked(self, origins, directions, radius, max_t=None, min_t=0.0, mesh_mask=None, ignore_prim=None):
        """The any-hit form of sweep_spheres: a bool array, True where the ball touches the scene somewhere in [min_t, max_t]."""
        fam = SWEEPS["spheres"]
        return self._sweep_blocked_host(fam, self._sweep_array(fam, origins, directions, max_t, min_t, radius=radius), mesh_mask, ignore_prim)

    def sweep_boxes_device(self, d_sweeps, n, d_records=None, d_centres=None, d_normals=None, count=None, ids=None, mesh_mask=None,
                           ignore_prim=None):
        """The first contact of each of n moving axis-aligned boxes (BOX_SWEEP_DTYPE bytes on the device; include/rtk_amd.h, "Box
        sweeps") with the scene: returns (d_records, d_centres, d_normals), uint8 cuda tensors of HIT_RECORD_DTYPE records and of 3
        floats per query each (the box's centre at the contact, the contact normal against the motion). count / ids: cuda int64
        tensors naming the queries to answer, as for closest_points_device; slots that are not listed are not written. mesh_mask:
        bools per mesh; ignore_prim: one id per query slot (a cuda tensor, or array-like)."""
        return self._sweep_device(SWEEPS["boxes"], d_sweeps, n, d_records, d_centres, d_normals, count, ids, mesh_mask, ignore_prim)

    def sweep_boxes_any_device(self, d_sweeps, n, d_blocked=None, count=None, ids=None, mesh_mask=None, ignore_prim=None):
        """The any-hit form of sweep_boxes_device: one byte per query, 1 where the path is blocked, in the queries' own slots."""
        return self._sweep_any_device(SWEEPS["boxes"], d_sweeps, n, d_blocked, count, ids, mesh_mask, ignore_prim)

    def sweep_boxes_counted(self, d_sweeps, n, mesh_mask=None, ignore_prim=None):
        """sweep_boxes_device of all n queries on the null stream, synchronous, with the visit counts of
        rtk_dev_sweep_boxes_counted: returns (d_records, d_centres, d_normals, counts dict)."""
        return self._sweep_counted(SWEEPS["boxes"], d_sweeps, n, mesh_mask, ignore_prim)

    def sweep_boxes(self, origins, directions, half, max_t=None, min_t=0.0, mesh_mask=None, ignore_prim=None):
        """origins: array-like (n, 3) float32; directions (n, 3) or (3,), not necessarily normalised: t is in their units; half:
        the half extents, (n, 3), (3,) or a scalar (a cube); max_t, min_t: scalars or one per query; max_t None = no limit
        (RTK_INF). Returns (records HIT_RECORD_DTYPE, centres at the contact (n, 3) float32, contact normals (n, 3) float32):
        prim == 0xFFFFFFFF is a miss, whose t is max_t, whose centre is the origin and whose normal is zeros."""
        fam = SWEEPS["boxes"]
        return self._sweep_host(fam, self._sweep_array(fam, origins, directions, max_t, min_t, half=half), mesh_mask, ignore_prim)

    def box_path_blocked(self, origins, directions, half, max_t=None, min_t=0.0, mesh_mask=None, ignore_prim=None):
        """The any-hit form of sweep_boxes: a bool array, True where the box touches the scene somewhere in [min_t, max_t]."""
        fam = SWEEPS["boxes"]
        return self._sweep_blocked_host(fam, self._sweep_array(fam, origins, directions, max_t, min_t, half=half), mesh_mask, ignore_prim)

    def sweep_capsules_device(self, d_sweeps, n, d_records=None, d_points=None, d_axis_points=None, count=None, ids=None, mesh_mask=None,
                              ignore_prim=None):
        """The first contact of each of n moving capsules (CAPSULE_SWEEP_DTYPE bytes on the device; include/rtk_amd.h, "Capsule
        sweeps") with the scene: returns (d_records, d_points, d_axis_points), uint8 cuda tensors of HIT_RECORD_DTYPE records and of
        3 floats per query each (the point of the triangle nearest the capsule's segment at the contact, the point of that segment
        nearest the triangle). count / ids: cuda int64 tensors naming the queries to answer, as for closest_points_device; slots
        that are not listed are not written. mesh_mask: bools per mesh; ignore_prim: one id per query slot (a cuda tensor, or
        array-like)."""
        return self._sweep_device(SWEEPS["capsules"], d_sweeps, n, d_records, d_points, d_axis_points, count, ids, mesh_mask, ignore_prim)

    def sweep_capsules_any_device(self, d_sweeps, n, d_blocked=None, count=None, ids=None, mesh_mask=None, ignore_prim=None):
        """The any-hit form of sweep_capsules_device: one byte per query, 1 where the path is blocked, in the queries' own slots."""
        return self._sweep_any_device(SWEEPS["capsules"], d_sweeps, n, d_blocked, count, ids, mesh_mask, ignore_prim)

    def sweep_capsules_counted(self, d_sweeps, n, mesh_mask=None, ignore_prim=None):
        """sweep_capsules_device of all n queries on the null stream, synchronous, with the visit counts of
        rtk_dev_sweep_capsules_counted: returns (d_records, d_points, d_axis_points, counts dict)."""
        return self._sweep_counted(SWEEPS["capsules"], d_sweeps, n, mesh_mask, ignore_prim)

    def sweep_capsules(self, origins, directions, radius, half_axis, max_t=None, min_t=0.0, mesh_mask=None, ignore_prim=None):
        """origins: array-like (n, 3) float32; directions (n, 3) or (3,), not necessarily normalised: t is in their units; radius: a
        scalar or one per query; half_axis: (n, 3) or (3,), from the capsule's centre to one end of its segment; max_t, min_t:
        scalars or one per query; max_t None = no limit (RTK_INF). Returns (records HIT_RECORD_DTYPE, the points of the triangles
        nearest the capsule's segment at the contact (n, 3) float32, the points of that segment nearest the triangle (n, 3)
        float32): prim == 0xFFFFFFFF is a miss, whose t is max_t and whose two points are the origin."""
        fam = SWEEPS["capsules"]
        s = self._sweep_array(fam, origins, directions, max_t, min_t, radius=radius, half_axis=half_axis)
        return self._sweep_host(fam, s, mesh_mask, ignore_prim)

    def capsule_path_blocked(self, origins, directions, radius, half_axis, max_t=None, min_t=0.0, mesh_mask=None, ignore_prim=None):
        """The any-hit form of sweep_capsules: a bool array, True where the capsule touches the scene somewhere in [min_t, max_t]."""
        fam = SWEEPS["capsules"]
        s = self._sweep_array(fam, origins, directions, max_t, min_t, radius=radius, half_axis=half_axis)
        return self._sweep_blocked_host(fam, s, mesh_mask, ignore_prim)

    def sweep_obbs_device(self, d_sweeps, n, d_records=None, d_centres=None, d_normals=None, count=None, ids=None, mesh_mask=None,
                          ignore_prim=None):
        """The first contact of each of n moving oriented boxes (OBB_SWEEP_DTYPE bytes on the device; include/rtk_amd.h, "Oriented
        box sweeps") with the scene: returns (d_records, d_centres, d_normals), uint8 cuda tensors of HIT_RECORD_DTYPE records and
        of 3 floats per query each (the box's centre at the contact, the contact normal against the motion). count / ids: cuda
        int64 tensors naming the queries to answer, as for closest_points_device; slots that are not listed are not written.
        mesh_mask: bools per mesh; ignore_prim: one id per query slot (a cuda tensor, or array-like)."""
        return self._sweep_device(SWEEPS["obbs"], d_sweeps, n, d_records, d_centres, d_normals, count, ids, mesh_mask, ignore_prim)

    def sweep_obbs_any_device(self, d_sweeps, n, d_blocked=None, count=None, ids=None, mesh_mask=None, ignore_prim=None):
        """The any-hit form of sweep_obbs_device: one byte per query, 1 where the path is blocked, in the queries' own slots."""
        return self._sweep_any_device(SWEEPS["obbs"], d_sweeps, n, d_blocked, count, ids, mesh_mask, ignore_prim)

    def sweep_obbs_counted(self, d_sweeps, n, mesh_mask=None, ignore_prim=None):
        """sweep_obbs_device of all n queries on the null stream, synchronous, with the visit counts of
        rtk_dev_sweep_obbs_counted: returns (d_records, d_centres, d_normals, counts dict)."""
        return self._sweep_counted(SWEEPS["obbs"], d_sweeps, n, mesh_mask, ignore_prim)

    @staticmethod
    def _obb_sweep_array(origins, directions, half, rotation, max_t, min_t):
        s = DeviceScene._sweep_array(SWEEPS["obbs"], origins, directions, max_t, min_t, half=half)
        s["axes"] = obb_axes(rotation, s.shape[0])
        return s

    def sweep_obbs(self, origins, directions, half, rotation, max_t=None, min_t=0.0, mesh_mask=None, ignore_prim=None):
        """origins: array-like (n, 3) float32; directions (n, 3) or (3,), not necessarily normalised: t is in their units; half:
        the half extents along the box's own axes, (n, 3), (3,) or a scalar (a cube); rotation: (n, 3, 3) or (3, 3) matrices whose
        ROWS are the box's axes in scene coordinates, or (n, 4) or (4,) quaternions (x, y, z, w) that turn the unit vectors into
        them (see obb_axes); max_t, min_t: scalars or one per query; max_t None = no limit (RTK_INF). Returns (records
        HIT_RECORD_DTYPE, centres at the contact (n, 3) float32, contact normals (n, 3) float32): prim == 0xFFFFFFFF is a miss,
        whose t is max_t, whose centre is the origin and whose normal is zeros. Axes that are not orthonormal to 2^-10 are a miss."""
        s = self._obb_sweep_array(origins, directions, half, rotation, max_t, min_t)
        return self._sweep_host(SWEEPS["obbs"], s, mesh_mask, ignore_prim)

    def obb_path_blocked(self, origins, directions, half, rotation, max_t=None, min_t=0.0, mesh_mask=None, ignore_prim=None):
        """The any-hit form of sweep_obbs: a bool array, True where the box touches the scene somewhere in [min_t, max_t]."""
        s = self._obb_sweep_array(origins, directions, half, rotation, max_t, min_t)
        return self._sweep_blocked_host(SWEEPS["obbs"], s, mesh_mask, ignore_prim)

    # -- triangles within a distance (rtk_dev_triangles_within_count / _all): asynchronous on the current stream --

    def count_within_device(self, d_queries, n, d_counts=None, count=None, ids=None):
        """The number of triangles nearer than its max_dist2 to each of n queries (POINT_QUERY_DTYPE bytes on the device;
        include/rtk_amd.h, "Triangles within a distance"): a cuda tensor of n uint32 words (d_counts: any cuda tensor of at
        least 4 n bytes; None: a new int32 tensor). count / ids: cuda int64 tensors naming the queries to answer, as for
        closest_points_device; slots that are not listed are not written. Nothing waits for the stream."""
        torch = _torch()
        if d_counts is None:
            d_counts = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")[:n]
        if ids is not None and count is None:
            raise RtkError("count_within_device: ids without count (a list's length lives on the device)")
        l = make_ray_list(count, ids) if count is not None else None
        _check(lib().rtk_dev_triangles_within_count(self.handle, C.c_void_p(d_queries.data_ptr()), n, C.byref(l) if l is not None else None,
                                                    C.c_void_p(d_counts.data_ptr()), _stream_ptr()), "rtk_dev_triangles_within_count")
        return d_counts

    def within_all_device(self, d_queries, n, d_offsets, d_records, d_points=None, d_written=None, count=None, ids=None):
        """Query i's nearest triangles within its max_dist2, ascending in (dist2, prim), into records d_offsets[i] ..
        d_offsets[i + 1] of d_records (16-byte CLOSEST_RECORD_DTYPE records) and, if d_points is given, their points into the
        same entries of d_points (3 floats each): as many as the query has or the segment holds. d_offsets: a cuda int64 tensor
        of n + 1 entries. d_written: a cuda tensor of 4 n bytes, or None (the call gets NULL). Records beyond written[i], and
        outside every segment, are not written. count / ids as for count_within_device. Nothing waits for the stream."""
        if ids is not None and count is None:
            raise RtkError("within_all_device: ids without count (a list's length lives on the device)")
        l = make_ray_list(count, ids) if count is not None else None
        _check(lib().rtk_dev_triangles_within_all(self.handle, C.c_void_p(d_queries.data_ptr()), n, C.byref(l) if l is not None else None,
                                                  C.c_void_p(d_offsets.data_ptr()), C.c_void_p(d_records.data_ptr()),
                                                  C.c_void_p(d_points.data_ptr()) if d_points is not None else None,
                                                  C.c_void_p(d_written.data_ptr()) if d_written is not None else None,
                                                  _stream_ptr()), "rtk_dev_triangles_within_all")
        return d_written

    def triangles_within_counted(self, d_queries, n, d_offsets=None, d_records=None, d_points=None, d_counts=None):
        """count_within_device (d_offsets None) or within_all_device of all n queries on the null stream, synchronous, with the
        visit counts of rtk_dev_triangles_within_counted: returns (d_counts -- the counts, or the written numbers --, counts dict)."""
        torch = _torch()
        if d_counts is None:
            d_counts = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")[:n]
        ctr = TraceCounters()
        torch.cuda.synchronize()
        _check(lib().rtk_dev_triangles_within_counted(self.handle, C.c_void_p(d_queries.data_ptr()), n,
                                                      C.c_void_p(d_offsets.data_ptr()) if d_offsets is not None else None,
                                                      C.c_void_p(d_records.data_ptr()) if d_records is not None else None,
                                                      C.c_void_p(d_points.data_ptr()) if d_points is not None else None,
                                                      C.c_void_p(d_counts.data_ptr()), C.byref(ctr)), "rtk_dev_triangles_within_counted")
        return d_counts, ctr.as_dict()

    def _within_queries(self, points, max_dist):
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        q = np.zeros(pts.shape[0], POINT_QUERY_DTYPE)
        q["point"] = pts
        if max_dist is None:
            q["max_dist2"] = RTK_INF
        else:
            d = np.broadcast_to(np.asarray(max_dist, np.float32), (pts.shape[0],))
            with np.errstate(over="ignore", invalid="ignore"):
                q["max_dist2"] = d * d
        return q

    def triangles_within(self, points, max_dist, max_per_point=None):
        """Every triangle nearer than max_dist to each point, or with max_per_point=k the k nearest of them. points: array-like
        (n, 3) float32; max_dist: a distance (scalar or one per point), squared in float32; None = no limit (RTK_INF). Returns
        (offsets int64[n + 1], records CLOSEST_RECORD_DTYPE[offsets[n]], points (offsets[n], 3) float32, written uint32[n]):
        point i's triangles are records[offsets[i] : offsets[i] + written[i]], ascending in (dist2, prim), and points[j] is the
        point on the triangle of records[j]. Without max_per_point: a count, its prefix sum on the device and the fill, enqueued
        without a host wait in between (only the size of the buffers is read back, to allocate them), and written[i] ==
        offsets[i + 1] - offsets[i]. With it: offsets[i] = i * k, no count, and the entries of a segment beyond written[i] are zero."""
        torch = _torch()
        q = self._within_queries(points, max_dist)
        n = q.shape[0]
        if n == 0:
            return np.zeros(1, np.int64), np.zeros(0, CLOSEST_RECORD_DTYPE), np.zeros((0, 3), np.float32), np.zeros(0, np.uint32)
        d_q = to_device(q)
        if max_per_point is None:
            d_counts = self.count_within_device(d_q, n)
            d_offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
            d_offsets[1:] = torch.cumsum(d_counts, 0, dtype=torch.int64)
            total = int(d_offsets[n].item())                 # (the one read-back: how many records to allocate)
        else:
            k = int(max_per_point)
            if k < 0:
                raise RtkError("triangles_within: max_per_point %r" % (max_per_point,))
            d_offsets = torch.arange(n + 1, dtype=torch.int64, device="cuda") * k
            total = n * k
        d_records = torch.zeros(max(total, 1) * 16, dtype=torch.uint8, device="cuda")
        d_points = torch.zeros(max(total, 1) * 12, dtype=torch.uint8, device="cuda")
        d_written = torch.empty(n, dtype=torch.int32, device="cuda")
        self.within_all_device(d_q, n, d_offsets, d_records, d_points, d_written)
        _check(lib().rtk_dev_trace_status(self.handle, _stream_ptr()), "rtk_dev_trace_status")
        return (d_offsets.cpu().numpy(), d_records.cpu().numpy().view(CLOSEST_RECORD_DTYPE)[:total],
                d_points.cpu().numpy().view(np.float32).reshape(-1, 3)[:total], d_written.cpu().numpy().view(np.uint32))

    def nearest_triangles(self, points, k, max_dist=None):
        """The k nearest triangles to each point (nearer than max_dist, if given). Returns (records CLOSEST_RECORD_DTYPE (n, k),
        points (n, k, 3) float32, written uint32[n]): row i holds written[i] entries, ascending in (dist2, prim); the rest of
        the row is zero."""
        k = int(k)
        n = np.ascontiguousarray(points, np.float32).reshape(-1, 3).shape[0]
        _, rec, pts, written = self.triangles_within(points, max_dist, max_per_point=k)
        return rec.reshape(n, k), pts.reshape(n, k, 3), written

    # -- the three overlap queries (triangles that touch a box, an oriented box, a triangle; a row of OVERLAPS each): asynchronous
    # on the current stream, nothing here waits for it. first_prim / skip_shared are the touching calls' alone --

    def _overlap_count_device(self, fam, d_q, n, d_counts, count, ids, first_prim=None, skip_shared=False):
        """count_<fam.name>_device"""
        torch = _torch()
        if d_counts is None:
            d_counts = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")[:n]
        if ids is not None and count is None:
            raise RtkError("count_%s_device: ids without count (a list's length lives on the device)" % fam.name)
        l = make_ray_list(count, ids) if count is not None else None
        f = make_touch_filter(first_prim, skip_shared)
        filt = (C.byref(f) if f is not None else None,) if fam.filtered else ()
        _check(getattr(lib(), fam.stem + "_count")(self.handle, C.c_void_p(d_q.data_ptr()), n, C.byref(l) if l is not None else None, *filt,
                                                   C.c_void_p(d_counts.data_ptr()), _stream_ptr()), fam.stem + "_count")
        return d_counts

    def _overlap_all_device(self, fam, d_q, n, d_offsets, d_prims, d_written, count, ids, first_prim=None, skip_shared=False):
        """<fam.name>_all_device"""
        if ids is not None and count is None:
            raise RtkError("%s_all_device: ids without count (a list's length lives on the device)" % fam.name)
        l = make_ray_list(count, ids) if count is not None else None
        f = make_touch_filter(first_prim, skip_shared)
        filt = (C.byref(f) if f is not None else None,) if fam.filtered else ()
        _check(getattr(lib(), fam.stem + "_all")(self.handle, C.c_void_p(d_q.data_ptr()), n, C.byref(l) if l is not None else None, *filt,
                                                 C.c_void_p(d_offsets.data_ptr()), C.c_void_p(d_prims.data_ptr()),
                                                 C.c_void_p(d_written.data_ptr()) if d_written is not None else None, _stream_ptr()), fam.stem + "_all")
        return d_written

    def _overlap_counted(self, fam, d_q, n, d_offsets, d_prims, d_counts, first_prim=None, skip_shared=False):
        """triangles_<fam.name>_counted: on the null stream, synchronous"""
        torch = _torch()
        if d_counts is None:
            d_counts = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")[:n]
        ctr = TraceCounters()
        f = make_touch_filter(first_prim, skip_shared)
        filt = (C.byref(f) if f is not None else None,) if fam.filtered else ()
        torch.cuda.synchronize()
        _check(getattr(lib(), fam.stem + "_counted")(self.handle, C.c_void_p(d_q.data_ptr()), n, *filt,
                                                     C.c_void_p(d_offsets.data_ptr()) if d_offsets is not None else None,
                                                     C.c_void_p(d_prims.data_ptr()) if d_prims is not None else None,
                                                     C.c_void_p(d_counts.data_ptr()), C.byref(ctr)), fam.stem + "_counted")
        return d_counts, ctr.as_dict()

    def _overlap_lists(self, fam, d_q, n, k, first_prim=None, skip_shared=False):
        """count, prefix sum and fill (or, with k, offsets i * k and the fill) on the current stream -> (d_offsets int64 [n + 1],
        d_prims int32 [max(total, 1)], d_written int32 [n], total). Only the size of the buffer is read back."""
        torch = _torch()
        if k is None:
            d_counts = self._overlap_count_device(fam, d_q, n, None, None, None, first_prim, skip_shared)
            d_offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
            d_offsets[1:] = torch.cumsum(d_counts, 0, dtype=torch.int64)
            total = int(d_offsets[n].item())                 # (the one read-back: how many ids to allocate)
        else:
            d_offsets = torch.arange(n + 1, dtype=torch.int64, device="cuda") * k
            total = n * k
        d_prims = torch.zeros(max(total, 1), dtype=torch.int32, device="cuda")
        d_written = torch.empty(n, dtype=torch.int32, device="cuda")
        self._overlap_all_device(fam, d_q, n, d_offsets, d_prims, d_written, None, None, first_prim, skip_shared)
        _check(lib().rtk_dev_trace_status(self.handle, _stream_ptr()), "rtk_dev_trace_status")
        return d_offsets, d_prims, d_written, total

    def _overlap_lists_host(self, fam, q, max_per_query, who, first_prim=None, skip_shared=False):
        """_overlap_lists of host records q (max_per_query: None or k, refused in `who`'s name if negative) as numpy arrays:
        (offsets int64[n + 1], prims uint32[offsets[n]], written uint32[n])"""
        n = q.shape[0]
        if n == 0:
            return np.zeros(1, np.int64), np.zeros(0, np.uint32), np.zeros(0, np.uint32)
        k = None
        if max_per_query is not None:
            k = int(max_per_query)
            if k < 0:
                raise RtkError("%s %r" % (who, max_per_query))
        d_offsets, d_prims, d_written, total = self._overlap_lists(fam, to_device(q), n, k, first_prim, skip_shared)
        return d_offsets.cpu().numpy(), d_prims.cpu().numpy().view(np.uint32)[:total], d_written.cpu().numpy().view(np.uint32)

    # -- triangles that touch a box (rtk_dev_triangles_in_box_count / _all) --

    def count_in_boxes_device(self, d_boxes, n, d_counts=None, count=None, ids=None):
        """The number of triangles that touch each of n boxes (BOX_QUERY_DTYPE bytes on the device, or a float32 [n, 6] cuda
        tensor of lo, hi; include/rtk_amd.h, "Triangles that touch a box"): a cuda tensor of n uint32 words (d_counts: any
        cuda tensor of at least 4 n bytes; None: a new int32 tensor). count / ids: cuda int64 tensors naming the queries to
        answer, as for closest_points_device; slots that are not listed are not written. Nothing waits for the stream."""
        return self._overlap_count_device(OVERLAPS["in_boxes"], d_boxes, n, d_counts, count, ids)

    def in_boxes_all_device(self, d_boxes, n, d_offsets, d_prims, d_written=None, count=None, ids=None):
        """Box i's triangles, ascending global primitive ids (uint32), into entries d_offsets[i] .. d_offsets[i + 1] of d_prims:
        as many as the box has or the segment holds, the lowest ids first. d_offsets: a cuda int64 tensor of n + 1 entries.
        d_written: a cuda tensor of 4 n bytes, or None (the call gets NULL). Entries beyond written[i], and outside every
        segment, are not written. count / ids as for count_in_boxes_device. Nothing waits for the stream."""
        return self._overlap_all_device(OVERLAPS["in_boxes"], d_boxes, n, d_offsets, d_prims, d_written, count, ids)

    def triangles_in_boxes_counted(self, d_boxes, n, d_offsets=None, d_prims=None, d_counts=None):
        """count_in_boxes_device (d_offsets None) or in_boxes_all_device of all n boxes on the null stream, synchronous, with the
        visit counts of rtk_dev_triangles_in_box_counted: returns (d_counts -- the counts, or the written numbers --, counts dict)."""
        return self._overlap_counted(OVERLAPS["in_boxes"], d_boxes, n, d_offsets, d_prims, d_counts)

    def triangles_in_boxes(self, boxes, max_per_box=None):
        """Every triangle that touches each box, or with max_per_box=k the k lowest ids of them. boxes: array-like (n, 6) float32
        of lo, hi, or BOX_QUERY_DTYPE records. Returns (offsets int64[n + 1], prims uint32[offsets[n]], written uint32[n]): box
        i's triangles are prims[offsets[i] : offsets[i] + written[i]], ascending. Without max_per_box: a count, its prefix sum on
        the device and the fill, enqueued without a host wait in between (only the size of the buffer is read back, to allocate
        it), and written[i] == offsets[i + 1] - offsets[i]. With it: offsets[i] = i * k, no count, and the entries of a segment
        beyond written[i] are zero."""
        boxes = np.asarray(boxes)
        q = np.ascontiguousarray(boxes if boxes.dtype == BOX_QUERY_DTYPE else np.asarray(boxes, np.float32).reshape(-1, 6))
        return self._overlap_lists_host(OVERLAPS["in_boxes"], q, max_per_box, "triangles_in_boxes: max_per_box")

    def occupancy(self, lo, hi, shape):
        """A bool cuda tensor of `shape` (nx, ny, nz): true where at least one triangle touches the voxel. The voxel faces are
        one float32 torch.linspace(lo[a], hi[a], shape[a] + 1) per axis (made on the host, so its bits do not depend on the
        device), so neighbours share their face bits and a triangle that touches a shared face is in both. One count over
        nx * ny * nz boxes on the current stream; the result is not waited for."""
        torch = _torch()
        shape = tuple(int(s) for s in shape)
        if len(shape) != 3 or min(shape) < 1:
            raise RtkError("occupancy: shape %r" % (shape,))
        faces = [torch.linspace(float(lo[a]), float(hi[a]), shape[a] + 1, dtype=torch.float32).cuda() for a in range(3)]
        lows = torch.stack(torch.meshgrid(faces[0][:-1], faces[1][:-1], faces[2][:-1], indexing="ij"), -1)
        highs = torch.stack(torch.meshgrid(faces[0][1:], faces[1][1:], faces[2][1:], indexing="ij"), -1)
        d_boxes = torch.cat([lows, highs], -1).reshape(-1, 6).contiguous()
        n = d_boxes.shape[0]
        d_counts = self.count_in_boxes_device(d_boxes, n)
        return (d_counts != 0).reshape(shape)

    # -- triangles that touch an oriented box (rtk_dev_triangles_in_obb_count / _all): asynchronous on the current stream --

    def count_in_obbs_device(self, d_obbs, n, d_counts=None, count=None, ids=None):
        """The number of triangles that touch each of n oriented boxes (OBB_QUERY_DTYPE bytes on the device, or a float32
        [n, 15] cuda tensor of centre, half, axes; include/rtk_amd.h, "Triangles that touch an oriented box"): a cuda tensor of
        n uint32 words (d_counts: any cuda tensor of at least 4 n bytes; None: a new int32 tensor). count / ids: cuda int64
        tensors naming the queries to answer, as for count_in_boxes_device; slots that are not listed are not written. Nothing
        waits for the stream."""
        return self._overlap_count_device(OVERLAPS["in_obbs"], d_obbs, n, d_counts, count, ids)

    def in_obbs_all_device(self, d_obbs, n, d_offsets, d_prims, d_written=None, count=None, ids=None):
        """Oriented box i's triangles, ascending global primitive ids (uint32), into entries d_offsets[i] .. d_offsets[i + 1] of
        d_prims: as many as the box has or the segment holds, the lowest ids first. d_offsets: a cuda int64 tensor of n + 1
        entries. d_written: a cuda tensor of 4 n bytes, or None (the call gets NULL). Entries beyond written[i], and outside every
        segment, are not written. count / ids as for count_in_obbs_device. Nothing waits for the stream."""
        return self._overlap_all_device(OVERLAPS["in_obbs"], d_obbs, n, d_offsets, d_prims, d_written, count, ids)

    def triangles_in_obbs_counted(self, d_obbs, n, d_offsets=None, d_prims=None, d_counts=None):
        """count_in_obbs_device (d_offsets None) or in_obbs_all_device of all n boxes on the null stream, synchronous, with the
        visit counts of rtk_dev_triangles_in_obb_counted: returns (d_counts -- the counts, or the written numbers --, counts dict)."""
        return self._overlap_counted(OVERLAPS["in_obbs"], d_obbs, n, d_offsets, d_prims, d_counts)

    def triangles_in_obbs(self, centres, half, rotation, max_per_box=None):
        """Every triangle that touches each oriented box, or with max_per_box=k the k lowest ids of them. centres: (n, 3); half:
        the half extents along the box's own axes, (n, 3), (3,) or a scalar (a cube); rotation: (n, 3, 3) or (3, 3) matrices whose
        ROWS are the box's axes in scene coordinates, or (n, 4) or (4,) quaternions (x, y, z, w) (see obb_axes). Returns what
        triangles_in_boxes returns: (offsets int64[n + 1], prims uint32[offsets[n]], written uint32[n])."""
        return self._overlap_lists_host(OVERLAPS["in_obbs"], obb_query_array(centres, half, rotation), max_per_box, "triangles_in_obbs: max_per_box")

    def occupancy_oriented(self, centre, half, rotation, shape):
        """A bool cuda tensor of `shape` (nx, ny, nz): true where at least one triangle touches the cell of the nx x ny x nz grid
        that fills the oriented box (centre, half, rotation as for triangles_in_obbs, one box). The cells' centres and half
        extents are made on the host in numpy float32 (oriented_grid), so their bits do not depend on the device. One count over
        nx * ny * nz oriented boxes on the current stream; the result is not waited for."""
        q = oriented_grid(centre, half, rotation, shape)
        d_counts = self.count_in_obbs_device(to_device(q), q.shape[0])
        return (d_counts != 0).reshape(tuple(int(s) for s in shape))

    # -- triangles that touch a triangle (rtk_dev_triangles_touching_count / _all): asynchronous on the current stream --

    def count_touching_device(self, d_tris, n, d_counts=None, count=None, ids=None, first_prim=None, skip_shared=False):
        """The number of the scene's triangles that each of n query triangles meets (TRI_QUERY_DTYPE bytes on the device, or a
        float32 [n, 9] or [n, 3, 3] cuda tensor; include/rtk_amd.h, "Triangles that touch a triangle"): a cuda tensor of n
        uint32 words (d_counts: any cuda tensor of at least 4 n bytes; None: a new int32 tensor). count / ids: cuda int64
        tensors naming the queries to answer, as for closest_points_device; slots that are not listed are not written.
        first_prim: a cuda tensor of n 32-bit words, query i keeps ids >= first_prim[i]; skip_shared: records that share a
        vertex position with the query are left out. Nothing waits for the stream."""
        return self._overlap_count_device(OVERLAPS["touching"], d_tris, n, d_counts, count, ids, first_prim, skip_shared)

    def touching_all_device(self, d_tris, n, d_offsets, d_prims, d_written=None, count=None, ids=None, first_prim=None, skip_shared=False):
        """Query i's triangles, ascending global primitive ids (uint32), into entries d_offsets[i] .. d_offsets[i + 1] of d_prims:
        as many as it meets or the segment holds, the lowest ids first. d_offsets: a cuda int64 tensor of n + 1 entries.
        d_written: a cuda tensor of 4 n bytes, or None (the call gets NULL). Entries beyond written[i], and outside every
        segment, are not written. The other arguments as for count_touching_device. Nothing waits for the stream."""
        return self._overlap_all_device(OVERLAPS["touching"], d_tris, n, d_offsets, d_prims, d_written, count, ids, first_prim, skip_shared)

    def triangles_touching_counted(self, d_tris, n, d_offsets=None, d_prims=None, d_counts=None, first_prim=None, skip_shared=False):
        """count_touching_device (d_offsets None) or touching_all_device of all n queries on the null stream, synchronous, with the
        visit counts of rtk_dev_triangles_touching_counted: returns (d_counts -- the counts, or the written numbers --, counts dict)."""
        return self._overlap_counted(OVERLAPS["touching"], d_tris, n, d_offsets, d_prims, d_counts, first_prim, skip_shared)

    def _touching_on_device(self, d_q, n, k, d_first, skip_shared):
        """count, prefix sum and fill (or, with k, offsets i * k and the fill) on the current stream -> (d_offsets int64 [n + 1],
        d_prims int32 [max(total, 1)], d_written int32 [n], total). Only the size of the buffer is read back."""
        return self._overlap_lists(OVERLAPS["touching"], d_q, n, k, d_first, skip_shared)

    def triangles_touching(self, tris, max_per_tri=None, first_prim=None, skip_shared=False):
        """Every triangle of the scene that each query triangle meets, or with max_per_tri=k the k lowest ids of them. tris:
        array-like (n, 9) or (n, 3, 3) float32, or TRI_QUERY_DTYPE records; first_prim: array-like of n ids or None. Returns
        (offsets int64[n + 1], prims uint32[offsets[n]], written uint32[n]): query i's triangles are
        prims[offsets[i] : offsets[i] + written[i]], ascending. Without max_per_tri: a count, its prefix sum on the device and
        the fill, enqueued without a host wait in between (only the size of the buffer is read back, to allocate it), and
        written[i] == offsets[i + 1] - offsets[i]. With it: offsets[i] = i * k, no count, and the entries of a segment beyond
        written[i] are zero."""
        torch = _torch()
        tris = np.asarray(tris)
        q = np.ascontiguousarray(tris if tris.dtype == TRI_QUERY_DTYPE else np.asarray(tris, np.float32).reshape(-1, 9))
        n = q.shape[0]
        if n == 0:
            return np.zeros(1, np.int64), np.zeros(0, np.uint32), np.zeros(0, np.uint32)
        k = None
        if max_per_tri is not None:
            k = int(max_per_tri)
            if k < 0:
                raise RtkError("triangles_touching: max_per_tri %r" % (max_per_tri,))
        d_first = None
        if first_prim is not None:
            first = np.ascontiguousarray(first_prim, np.uint32)
            if first.shape != (n,):
                raise RtkError("triangles_touching: first_prim of shape %r for %d queries" % (first.shape, n))
            d_first = torch.from_numpy(first.view(np.int32)).cuda()
        d_offsets, d_prims, d_written, total = self._touching_on_device(to_device(q), n, k, d_first, skip_shared)
        return d_offsets.cpu().numpy(), d_prims.cpu().numpy().view(np.uint32)[:total], d_written.cpu().numpy().view(np.uint32)

    def triangles(self):
        """The scene's current positions by primitive id: a float32 cuda tensor [T, 3, 3], through rtk_dev_expand_hits of one
        made-up record per primitive, on the current stream. A batch of queries as it stands."""
        torch = _torch()
        n = self.info()["num_triangles"]
        if n == 0:
            return torch.zeros((0, 3, 3), dtype=torch.float32, device="cuda")
        rec = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
        rec[:, 3] = torch.arange(n, dtype=torch.int32, device="cuda")
        d_hits, _ = self.expand_device(rec, n)
        # (rtk_hit: t u v, then three vertices of position[3] and index, then mesh and triangle: 17 words)
        return d_hits.view(torch.float32).reshape(n, 17)[:, 3:15].reshape(n, 3, 4)[:, :, :3].contiguous()

    def _pairs(self, d_q, d_first, skip_shared):
        torch = _torch()
        n = d_q.shape[0]
        if n == 0 or self.info()["num_triangles"] == 0:
            return torch.zeros((0, 2), dtype=torch.int64, device="cuda")
        d_offsets, d_prims, d_written, total = self._touching_on_device(d_q, n, None, d_first, skip_shared)
        who = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device="cuda"), d_written.to(torch.int64), output_size=total)
        return torch.stack([who, d_prims[:total].to(torch.int64) & 0xffffffff], 1)

    def intersections(self, other):
        """The pairs (primitive of other, primitive of self) whose triangles meet by the rule, other.triangles() being the
        queries: an int64 cuda tensor [m, 2], ascending in both columns. Count, prefix sum and fill on the current stream."""
        return self._pairs(other.triangles(), None, False)

    def self_intersections(self):
        """The pairs (i, j), i < j, of the scene's own triangles that meet by the rule and share no vertex position (neighbours in
        a mesh share positions bit for bit and always touch): an int64 cuda tensor [m, 2], ascending in both columns. The
        queries are self.triangles(), with skip_shared and first_prim = own id + 1."""
        torch = _torch()
        d_q = self.triangles()
        d_first = torch.arange(1, d_q.shape[0] + 1, dtype=torch.int32, device="cuda")
        return self._pairs(d_q, d_first, True)

    # -- closest triangles (rtk_dev_closest_triangles): asynchronous on the current stream, nothing here waits for it --

    def closest_triangles_device(self, d_tris, n, d_records=None, d_points_query=None, d_points_scene=None, max_dist2=None, count=None, ids=None,
                                 first_prim=None, skip_shared=False):
        """The nearest triangle of the scene to each of n query triangles, segments or points (TRI_QUERY_DTYPE bytes on the
        device, or a float32 [n, 9] or [n, 3, 3] cuda tensor; include/rtk_amd.h, "Closest triangles"): returns (d_records,
        d_points_query, d_points_scene), uint8 cuda tensors of CLOSEST_RECORD_DTYPE records and of 3 floats per query each (any
        cuda tensors of enough bytes may be passed in; None: new ones). max_dist2: a cuda float32 tensor of one squared limit per query slot, or
        None (no limit). count / ids: cuda int64 tensors naming the queries to answer, as for closest_points_device; slots that
        are not listed are not written. first_prim / skip_shared: the filter of count_touching_device."""
        torch = _torch()
        if d_records is None:
            d_records = torch.empty(max(n, 1) * 16, dtype=torch.uint8, device="cuda")[:n * 16]
        if d_points_query is None:
            d_points_query = torch.empty(max(n, 1) * 12, dtype=torch.uint8, device="cuda")[:n * 12]
        if d_points_scene is None:
            d_points_scene = torch.empty(max(n, 1) * 12, dtype=torch.uint8, device="cuda")[:n * 12]
        if ids is not None and count is None:
            raise RtkError("closest_triangles_device: ids without count (a list's length lives on the device)")
        l = make_ray_list(count, ids) if count is not None else None
        f = make_touch_filter(first_prim, skip_shared)
        _check(lib().rtk_dev_closest_triangles(self.handle, C.c_void_p(d_tris.data_ptr()), n, C.byref(l) if l is not None else None,
                                               C.byref(f) if f is not None else None,
                                               C.c_void_p(max_dist2.data_ptr()) if max_dist2 is not None else None, C.c_void_p(d_records.data_ptr()),
                                               C.c_void_p(d_points_query.data_ptr()), C.c_void_p(d_points_scene.data_ptr()),
                                               _stream_ptr()), "rtk_dev_closest_triangles")
        return d_records, d_points_query, d_points_scene

    def closest_triangles_counted(self, d_tris, n, max_dist2=None, first_prim=None, skip_shared=False):
        """closest_triangles_device of all n queries on the null stream, synchronous, with the visit counts of
        rtk_dev_closest_triangles_counted: returns (d_records, d_points_query, d_points_scene, counts dict)."""
        torch = _torch()
        d_records = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
        d_pq = torch.empty(n * 12, dtype=torch.uint8, device="cuda")
        d_ps = torch.empty(n * 12, dtype=torch.uint8, device="cuda")
        ctr = TraceCounters()
        f = make_touch_filter(first_prim, skip_shared)
        torch.cuda.synchronize()
        _check(lib().rtk_dev_closest_triangles_counted(self.handle, C.c_void_p(d_tris.data_ptr()), n, C.byref(f) if f is not None else None,
                                                       C.c_void_p(max_dist2.data_ptr()) if max_dist2 is not None else None,
                                                       C.c_void_p(d_records.data_ptr()), C.c_void_p(d_pq.data_ptr()), C.c_void_p(d_ps.data_ptr()),
                                                       C.byref(ctr)), "rtk_dev_closest_triangles_counted")
        return d_records, d_pq, d_ps, ctr.as_dict()

    def closest_triangles(self, tris, max_dist=None, first_prim=None, skip_shared=False):
        """The nearest triangle of the scene to each query. tris: array-like (n, 9) or (n, 3, 3) float32, or TRI_QUERY_DTYPE
        records (a segment or a point is a triangle with equal vertices); max_dist: a distance (scalar or one per query) at
        or beyond which a triangle does not count, squared in float32, None = no limit; first_prim: array-like of n ids or
        None. Returns (dist float32[n] -- the square root of dist2 --, prim uint32[n], u, v float32[n], points on the query
        (n, 3), points on the scene (n, 3)): prim == 0xFFFFFFFF is a miss, whose points are the query's vertex 0."""
        torch = _torch()
        tris = np.asarray(tris)
        q = np.ascontiguousarray(tris if tris.dtype == TRI_QUERY_DTYPE else np.asarray(tris, np.float32).reshape(-1, 9))
        n = q.shape[0]
        if n == 0:
            z = np.zeros(0, np.float32)
            return z, np.zeros(0, np.uint32), z.copy(), z.copy(), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32)
        d_max = None
        if max_dist is not None:
            d = np.broadcast_to(np.asarray(max_dist, np.float32), (n,))
            with np.errstate(over="ignore", invalid="ignore"):
                d_max = torch.from_numpy(np.ascontiguousarray(d * d)).cuda()
        d_first = None
        if first_prim is not None:
            first = np.ascontiguousarray(first_prim, np.uint32)
            if first.shape != (n,):
                raise RtkError("closest_triangles: first_prim of shape %r for %d queries" % (first.shape, n))
            d_first = torch.from_numpy(first.view(np.int32)).cuda()
        d_rec, d_pq, d_ps = self.closest_triangles_device(to_device(q), n, max_dist2=d_max, first_prim=d_first, skip_shared=skip_shared)
        _check(lib().rtk_dev_trace_status(self.handle, _stream_ptr()), "rtk_dev_trace_status")
        rec = d_rec.cpu().numpy().view(CLOSEST_RECORD_DTYPE)
        with np.errstate(invalid="ignore"):
            dist = np.sqrt(rec["dist2"])
        return (dist, rec["prim"].copy(), rec["u"].copy(), rec["v"].copy(), d_pq.cpu().numpy().view(np.float32).reshape(n, 3),
                d_ps.cpu().numpy().view(np.float32).reshape(n, 3))

    def _nearest_pair(self, d_q, d_first, skip_shared):
        """The smallest (dist2, query index) over the queries d_q [n, 3, 3], reduced on the device: (distance, query index,
        primitive of self, point on the query, point on self), or None if no query found a triangle."""
        torch = _torch()
        n = d_q.shape[0]
        if n == 0 or self.info()["num_triangles"] == 0:
            return None
        d_rec, d_pq, d_ps = self.closest_triangles_device(d_q, n, first_prim=d_first, skip_shared=skip_shared)
        _check(lib().rtk_dev_trace_status(self.handle, _stream_ptr()), "rtk_dev_trace_status")
        rec = d_rec.view(torch.int32).reshape(n, 4)
        hit = rec[:, 3] != -1
        # (dist2 >= +0: its bits order like its value; the query index breaks ties, the lowest first)
        key = torch.where(hit, (rec[:, 0].to(torch.int64) << 32) | torch.arange(n, dtype=torch.int64, device="cuda"),
                          torch.full((n,), 2 ** 63 - 1, dtype=torch.int64, device="cuda"))
        best = int(torch.argmin(key).item())                 # (the one read-back, with the row below)
        row = torch.cat([rec[best].view(torch.float32), d_pq.view(torch.float32).reshape(n, 3)[best], d_ps.view(torch.float32).reshape(n, 3)[best]]).cpu().numpy()
        prim = int(row[3:4].view(np.uint32)[0])
        if prim == 0xFFFFFFFF:
            return None
        return float(np.sqrt(row[0])), best, prim, row[4:7].copy(), row[7:10].copy()

    def distance(self, other):
        """The distance between this scene and `other` by the rule of "Closest triangles", other.triangles() being the
        queries against this scene, reduced on the device to the smallest (dist2, primitive of other): (distance, primitive of
        other, primitive of self, point on other, point on self), or None if either scene has no triangles."""
        return self._nearest_pair(other.triangles(), None, False)

    def self_clearance(self):
        """The smallest distance between two of the scene's own triangles that share no vertex position: the queries are
        self.triangles() with skip_shared and first_prim = own id + 1. Returns (distance, i, j, point on i, point on j), i < j,
        or None if there is no such pair. The rule's known weakness applies (rtk_amd/csrc/rtk_pair_rule.h): two triangles that
        lie in one plane up to rounding and whose boxes touch can be called pierced by rounding errors, so a flat part of a
        mesh that is not axis-aligned can make this return 0 although nothing meets."""
        torch = _torch()
        d_q = self.triangles()
        d_first = torch.arange(1, d_q.shape[0] + 1, dtype=torch.int32, device="cuda")
        return self._nearest_pair(d_q, d_first, True)

    # -- triangles near a triangle (rtk_dev_triangles_near_count / _all): asynchronous on the current stream --

    def count_near_device(self, d_tris, n, d_counts=None, max_dist2=None, count=None, ids=None, first_prim=None, skip_shared=False):
        """The number of the scene's triangles nearer than its limit to each of n query triangles, segments or points
        (TRI_QUERY_DTYPE bytes on the device, or a float32 [n, 9] or [n, 3, 3] cuda tensor; include/rtk_amd.h, "Triangles near a
        triangle"): a cuda tensor of n uint32 words (d_counts: any cuda tensor of at least 4 n bytes; None: a new int32
        tensor). max_dist2: a cuda float32 tensor of one squared limit per query slot, or None (no limit: the whole filtered
        scene). count / ids: cuda int64 tensors naming the queries to answer, as for closest_points_device; slots that are not
        listed are not written. first_prim / skip_shared: the filter of count_touching_device. Nothing waits for the stream."""
        torch = _torch()
        if d_counts is None:
            d_counts = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")[:n]
        if ids is not None and count is None:
            raise RtkError("count_near_device: ids without count (a list's length lives on the device)")
        l = make_ray_list(count, ids) if count is not None else None
        f = make_touch_filter(first_prim, skip_shared)
        _check(lib().rtk_dev_triangles_near_count(self.handle, C.c_void_p(d_tris.data_ptr()), n, C.byref(l) if l is not None else None,
                                                  C.byref(f) if f is not None else None,
                                                  C.c_void_p(max_dist2.data_ptr()) if max_dist2 is not None else None,
                                                  C.c_void_p(d_counts.data_ptr()), _stream_ptr()), "rtk_dev_triangles_near_count")
        return d_counts

    def near_all_device(self, d_tris, n, d_offsets, d_records, d_points_query=None, d_points_scene=None, d_written=None, max_dist2=None,
                        count=None, ids=None, first_prim=None, skip_shared=False):
        """Query i's nearest triangles within its limit, ascending in (dist2, prim), into records d_offsets[i] ..
        d_offsets[i + 1] of d_records (16-byte CLOSEST_RECORD_DTYPE records) and, where given, the nearest point on the query
        and on the scene's triangle into the same entries of d_points_query and d_points_scene (3 floats each): as many as the
        query has or the segment holds. d_offsets: a cuda int64 tensor of n + 1 entries. d_written: a cuda tensor of 4 n bytes,
        or None (the call gets NULL). Records beyond written[i], and outside every segment, are not written. The other
        arguments as for count_near_device. Nothing waits for the stream."""
        if ids is not None and count is None:
            raise RtkError("near_all_device: ids without count (a list's length lives on the device)")
        l = make_ray_list(count, ids) if count is not None else None
        f = make_touch_filter(first_prim, skip_shared)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
        _check(lib().rtk_dev_triangles_near_all(self.handle, ptr(d_tris), n, C.byref(l) if l is not None else None,
                                                C.byref(f) if f is not None else None, ptr(max_dist2), ptr(d_offsets), ptr(d_records),
                                                ptr(d_points_query), ptr(d_points_scene), ptr(d_written), _stream_ptr()),
               "rtk_dev_triangles_near_all")
        return d_written

    def near_counted(self, d_tris, n, d_offsets=None, d_records=None, d_points_query=None, d_points_scene=None, d_counts=None, max_dist2=None,
                     first_prim=None, skip_shared=False):
        """count_near_device (d_offsets None) or near_all_device of all n queries on the null stream, synchronous, with the visit
        counts of rtk_dev_triangles_near_counted: returns (d_counts -- the counts, or the written numbers --, counts dict)."""
        torch = _torch()
        if d_counts is None:
            d_counts = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")[:n]
        ctr = TraceCounters()
        f = make_touch_filter(first_prim, skip_shared)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
        torch.cuda.synchronize()
        _check(lib().rtk_dev_triangles_near_counted(self.handle, ptr(d_tris), n, C.byref(f) if f is not None else None, ptr(max_dist2),
                                                    ptr(d_offsets), ptr(d_records), ptr(d_points_query), ptr(d_points_scene), ptr(d_counts),
                                                    C.byref(ctr)), "rtk_dev_triangles_near_counted")
        return d_counts, ctr.as_dict()

    def _near_on_device(self, d_q, n, k, d_max, d_first, skip_shared):
        """count, prefix sum and fill (or, with k, offsets i * k and the fill) on the current stream -> (d_offsets int64 [n + 1],
        d_records uint8, d_points_query uint8, d_points_scene uint8, d_written int32 [n], total). Only the size of the buffers is
        read back."""
        torch = _torch()
        if k is None:
            d_counts = self.count_near_device(d_q, n, max_dist2=d_max, first_prim=d_first, skip_shared=skip_shared)
            d_offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
            d_offsets[1:] = torch.cumsum(d_counts, 0, dtype=torch.int64)
            total = int(d_offsets[n].item())                 # (the one read-back: how many records to allocate)
        else:
            d_offsets = torch.arange(n + 1, dtype=torch.int64, device="cuda") * k
            total = n * k
        d_records = torch.zeros(max(total, 1) * 16, dtype=torch.uint8, device="cuda")
        d_pq = torch.zeros(max(total, 1) * 12, dtype=torch.uint8, device="cuda")
        d_ps = torch.zeros(max(total, 1) * 12, dtype=torch.uint8, device="cuda")
        d_written = torch.empty(n, dtype=torch.int32, device="cuda")
        self.near_all_device(d_q, n, d_offsets, d_records, d_pq, d_ps, d_written, max_dist2=d_max, first_prim=d_first, skip_shared=skip_shared)
        _check(lib().rtk_dev_trace_status(self.handle, _stream_ptr()), "rtk_dev_trace_status")
        return d_offsets, d_records, d_pq, d_ps, d_written, total

    def triangles_near(self, tris, max_dist, max_per_query=None, first_prim=None, skip_shared=False):
        """Every triangle of the scene nearer than max_dist to each query triangle, or with max_per_query=k the k nearest of
        them. tris: array-like (n, 9) or (n, 3, 3) float32, or TRI_QUERY_DTYPE records (a segment or a point is a triangle
        with equal vertices); max_dist: a distance (scalar or one per query), squared in float32; None = no limit (RTK_INF);
        first_prim: array-like of n ids or None. Returns (offsets int64[n + 1], records CLOSEST_RECORD_DTYPE[offsets[n]],
        points on the query (offsets[n], 3) float32, points on the scene (offsets[n], 3) float32, written uint32[n]): query i's
        triangles are records[offsets[i] : offsets[i] + written[i]], ascending in (dist2, prim). Without max_per_query: a
        count, its prefix sum on the device and the fill, enqueued without a host wait in between (only the size of the buffers
        is read back, to allocate them), and written[i] == offsets[i + 1] - offsets[i]. With it: offsets[i] = i * k, no count,
        and the entries of a segment beyond written[i] are zero."""
        torch = _torch()
        tris = np.asarray(tris)
        q = np.ascontiguousarray(tris if tris.dtype == TRI_QUERY_DTYPE else np.asarray(tris, np.float32).reshape(-1, 9))
        n = q.shape[0]
        if n == 0:
            return (np.zeros(1, np.int64), np.zeros(0, CLOSEST_RECORD_DTYPE), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32),
                    np.zeros(0, np.uint32))
        k = None
        if max_per_query is not None:
            k = int(max_per_query)
            if k < 0:
                raise RtkError("triangles_near: max_per_query %r" % (max_per_query,))
        d_max = None
        if max_dist is not None:
            d = np.broadcast_to(np.asarray(max_dist, np.float32), (n,))
            with np.errstate(over="ignore", invalid="ignore"):
                d_max = torch.from_numpy(np.ascontiguousarray(d * d)).cuda()
        d_first = None
        if first_prim is not None:
            first = np.ascontiguousarray(first_prim, np.uint32)
            if first.shape != (n,):
                raise RtkError("triangles_near: first_prim of shape %r for %d queries" % (first.shape, n))
            d_first = torch.from_numpy(first.view(np.int32)).cuda()
        d_offsets, d_rec, d_pq, d_ps, d_written, total = self._near_on_device(to_device(q), n, k, d_max, d_first, skip_shared)
        return (d_offsets.cpu().numpy(), d_rec.cpu().numpy().view(CLOSEST_RECORD_DTYPE)[:total],
                d_pq.cpu().numpy().view(np.float32).reshape(-1, 3)[:total], d_ps.cpu().numpy().view(np.float32).reshape(-1, 3)[:total],
                d_written.cpu().numpy().view(np.uint32))

    def nearest_triangles_to(self, tris, k, max_dist=None):
        """The k nearest triangles of the scene to each query triangle (nearer than max_dist, if given). Returns (records
        CLOSEST_RECORD_DTYPE (n, k), points on the query (n, k, 3) float32, points on the scene (n, k, 3) float32, written
        uint32[n]): row i holds written[i] entries, ascending in (dist2, prim); the rest of the row is zero."""
        k = int(k)
        _, rec, pq, ps, written = self.triangles_near(tris, max_dist, max_per_query=k)
        n = len(written)
        return rec.reshape(n, k), pq.reshape(n, k, 3), ps.reshape(n, k, 3), written

    def _contacts(self, d_q, margin, d_first, skip_shared):
        torch = _torch()
        n = d_q.shape[0]
        if n == 0 or self.info()["num_triangles"] == 0:
            z = torch.zeros((0, 3), dtype=torch.float32, device="cuda")
            return torch.zeros((0, 2), dtype=torch.int64, device="cuda"), torch.zeros(0, dtype=torch.float32, device="cuda"), z, z.clone()
        m = np.float32(margin)
        with np.errstate(over="ignore", invalid="ignore"):
            d_max = torch.full((n,), float(m * m), dtype=torch.float32, device="cuda")
        d_offsets, d_rec, d_pq, d_ps, d_written, total = self._near_on_device(d_q, n, None, d_max, d_first, skip_shared)
        who = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device="cuda"), d_written.to(torch.int64), output_size=total)
        rec = d_rec.view(torch.int32).reshape(-1, 4)[:total]
        pairs = torch.stack([who, rec[:, 3].to(torch.int64) & 0xffffffff], 1)
        return (pairs, torch.sqrt(rec[:, 0].contiguous().view(torch.float32)), d_pq.view(torch.float32).reshape(-1, 3)[:total],
                d_ps.view(torch.float32).reshape(-1, 3)[:total])

    def contacts(self, other, margin):
        """Every pair (primitive of other, primitive of self) whose triangles are nearer than `margin` by the rule of "Triangles
        near a triangle", other.triangles() being the queries: cuda tensors (pairs int64 [m, 2], distance float32 [m], point on
        other [m, 3], point on self [m, 3]), ascending in the primitive of other, then in (distance, primitive of self). Count,
        prefix sum and fill on the current stream; only the number of pairs is read back."""
        return self._contacts(other.triangles(), margin, None, False)

    def self_contacts(self, margin):
        """The pairs (i, j), i < j, of the scene's own triangles that are nearer than `margin` and share no vertex position, each
        once: the queries are self.triangles() with skip_shared and first_prim = own id + 1. Returns what contacts returns. The
        weakness stated under self_clearance applies."""
        torch = _torch()
        d_q = self.triangles()
        d_first = torch.arange(1, d_q.shape[0] + 1, dtype=torch.int32, device="cuda")
        return self._contacts(d_q, margin, d_first, True)

    # -- every hit along a ray (rtk_dev_trace_rays_count / rtk_dev_trace_rays_all): asynchronous on the current stream --

    def count_hits_device(self, d_rays, n, d_counts=None, filter=None, opts=None):
        """The number of candidates of each of n rays (include/rtk_amd.h, "Every hit along a ray"): a cuda tensor of n uint32
        words (d_counts: any cuda tensor of at least 4 n bytes; None: a new int32 tensor). Nothing waits for the stream."""
        torch = _torch()
        if d_counts is None:
            d_counts = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")[:n]
        _check(lib().rtk_dev_trace_rays_count(self.handle, C.c_void_p(d_rays.data_ptr()), n, C.c_void_p(d_counts.data_ptr()),
                                              C.byref(filter) if filter is not None else None, C.byref(opts) if opts is not None else None,
                                              _stream_ptr()), "rtk_dev_trace_rays_count")
        return d_counts

    def trace_all_device(self, d_rays, n, d_offsets, d_records, d_written=None, filter=None, opts=None):
        """Ray i's closest candidates, in (t, prim) order, into records d_offsets[i] .. d_offsets[i + 1] of d_records (16-byte
        HIT_RECORD_DTYPE records): as many as the ray has or the segment holds. d_offsets: a cuda int64 tensor of n + 1 entries,
        non-decreasing; d_written: None (a new int32 tensor of n entries) or a cuda tensor of 4 n bytes. Records beyond
        written[i], and outside every segment, are not written. Returns d_written. Nothing waits for the stream."""
        torch = _torch()
        if d_written is None:
            d_written = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")[:n]
        _check(lib().rtk_dev_trace_rays_all(self.handle, C.c_void_p(d_rays.data_ptr()), n, C.c_void_p(d_offsets.data_ptr()),
                                            C.c_void_p(d_records.data_ptr()), C.c_void_p(d_written.data_ptr()),
                                            C.byref(filter) if filter is not None else None, C.byref(opts) if opts is not None else None,
                                            _stream_ptr()), "rtk_dev_trace_rays_all")
        return d_written

    def _device_filter(self, n, mesh_mask, ignore_prim, after):
        """(DevFilter or None, the tensors it points into) for the numpy filters of trace_filtered"""
        if mesh_mask is None and ignore_prim is None and after is None:
            return None, []
        f = DevFilter()
        f.struct_size = C.sizeof(DevFilter)
        keep = []
        if mesh_mask is not None:
            bits = np.asarray(mesh_mask, bool)
            words = np.zeros((len(bits) + 31) // 32, np.uint32)
            for m, b in enumerate(bits):
                if b:
                    words[m >> 5] |= np.uint32(1 << (m & 31))
            d = to_device(words); keep.append(d)
            f.d_mesh_mask, f.mesh_mask_bits = d.data_ptr(), len(bits)
        if ignore_prim is not None:
            a = np.ascontiguousarray(ignore_prim, np.uint32)
            assert a.shape[0] == n
            d = to_device(a); keep.append(d)
            f.d_ignore_prim = d.data_ptr()
        if after is not None:
            a = np.ascontiguousarray(after)
            assert a.dtype == HIT_RECORD_DTYPE and a.shape[0] == n
            d = to_device(a); keep.append(d)
            f.d_after = d.data_ptr()
        return f, keep

    def count_hits(self, rays, mesh_mask=None, ignore_prim=None, after=None, opts=None):
        """rays: numpy RAY_DTYPE; filters as for trace_filtered. Returns the candidates per ray, uint32[n]."""
        rays = np.ascontiguousarray(rays)
        assert rays.dtype == RAY_DTYPE
        n = rays.shape[0]
        if n == 0:
            return np.zeros(0, np.uint32)
        f, _keep = self._device_filter(n, mesh_mask, ignore_prim, after)
        d_counts = self.count_hits_device(to_device(rays), n, filter=f, opts=opts)
        _check(lib().rtk_dev_trace_status(self.handle, _stream_ptr()), "rtk_dev_trace_status")
        return d_counts.cpu().numpy().view(np.uint32)

    def trace_all(self, rays, mesh_mask=None, ignore_prim=None, after=None, max_per_ray=None):
        """Every candidate of every ray, or with max_per_ray=k the k closest. rays: numpy RAY_DTYPE; filters as for
        trace_filtered. Returns (offsets int64[n + 1], records HIT_RECORD_DTYPE[offsets[n]], written uint32[n]): ray i's records
        are records[offsets[i] : offsets[i] + written[i]], ascending in (t, prim). Without max_per_ray: a count, its prefix sum on
        the device and the fill, enqueued without a host wait in between (only the size of the record buffer is read back,
        to allocate it), and written[i] == offsets[i + 1] - offsets[i]. With it: offsets[i] = i * k, no count, and the records
        of a segment beyond written[i] are zero."""
        torch = _torch()
        rays = np.ascontiguousarray(rays)
        assert rays.dtype == RAY_DTYPE
        n = rays.shape[0]
        if n == 0:
            return np.zeros(1, np.int64), np.zeros(0, HIT_RECORD_DTYPE), np.zeros(0, np.uint32)
        d_rays = to_device(rays)
        f, _keep = self._device_filter(n, mesh_mask, ignore_prim, after)
        if max_per_ray is None:
            d_counts = self.count_hits_device(d_rays, n, filter=f)
            d_offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
            d_offsets[1:] = torch.cumsum(d_counts, 0, dtype=torch.int64)
            total = int(d_offsets[n].item())                 # (the one read-back: how many records to allocate)
        else:
            k = int(max_per_ray)
            if k < 0:
                raise RtkError("trace_all: max_per_ray %r" % (max_per_ray,))
            d_offsets = torch.arange(n + 1, dtype=torch.int64, device="cuda") * k
            total = n * k
        d_records = torch.zeros(max(total, 1) * 16, dtype=torch.uint8, device="cuda")
        d_written = self.trace_all_device(d_rays, n, d_offsets, d_records, filter=f)
        _check(lib().rtk_dev_trace_status(self.handle, _stream_ptr()), "rtk_dev_trace_status")
        return (d_offsets.cpu().numpy(), d_records.cpu().numpy().view(HIT_RECORD_DTYPE)[:total], d_written.cpu().numpy().view(np.uint32))

    def contains(self, points, direction=(0.5458, 0.3207, 0.7743)):
        """Is each point inside the mesh? The parity (odd = inside) of count_hits for the rays from the points along `direction`
        with min_t = 0 and max_t = RTK_INF. points: array-like (n, 3) float32; returns bool[n]. MEANINGFUL FOR CLOSED MESHES
        ONLY (every ray that enters must leave). UNDEFINED for a point on the surface and for a ray that passes through an edge
        or a vertex: rtk's watertight test accepts an exactly-zero edge function on BOTH sides of a shared edge, so such a
        crossing counts twice (the default direction is generic on purpose: no component ratio is a small fraction)."""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        rays = np.zeros(pts.shape[0], RAY_DTYPE)
        rays["origin"] = pts
        rays["direction"] = np.asarray(direction, np.float32)
        rays["min_t"] = 0.0
        rays["max_t"] = RTK_INF
        return (self.count_hits(rays) & 1).astype(bool)

    def expand_device(self, d_records, n):
        torch = _torch()
        d_hits = torch.empty(n * 68, dtype=torch.uint8, device="cuda")
        d_mask = torch.empty(n, dtype=torch.uint8, device="cuda")
        _check(lib().rtk_dev_expand_hits(self.handle, C.c_void_p(d_records.data_ptr()), n, C.c_void_p(d_hits.data_ptr()),
                                         C.c_void_p(d_mask.data_ptr()), _stream_ptr()), "rtk_dev_expand_hits")
        return d_hits, d_mask

    # -- numpy conveniences used by the tests --

    def trace(self, rays, opts=None, full=True):
        """rays: numpy RAY_DTYPE. Returns (hits HIT_DTYPE, mask bool, records HIT_RECORD_DTYPE)."""
        torch = _torch()
        rays = np.ascontiguousarray(rays)
        assert rays.dtype == RAY_DTYPE
        n = rays.shape[0]
        d_rays = to_device(rays)
        d_rec = self.trace_device(d_rays, n, opts=opts)
        rec = d_rec.cpu().numpy().view(HIT_RECORD_DTYPE)
        if not full:
            torch.cuda.synchronize()
            return rec
        d_hits, d_mask = self.expand_device(d_rec, n)
        hits = d_hits.cpu().numpy().view(HIT_DTYPE)
        mask = d_mask.cpu().numpy().astype(bool)
        return hits, mask, rec

    def trace_filtered(self, rays, mesh_mask=None, ignore_prim=None, after=None, any_hit=False, opts=None):
        """Built-in device filters (rtk_dev_filter). mesh_mask: iterable of bools per mesh; ignore_prim: uint32 per
        ray; after: HIT_RECORD_DTYPE per ray. Returns records (closest) or an occluded bool array (any_hit)."""
        torch = _torch()
        rays = np.ascontiguousarray(rays)
        n = rays.shape[0]
        d_rays = to_device(rays)
        f = DevFilter()
        f.struct_size = C.sizeof(DevFilter)
        keep = []
        if mesh_mask is not None:
            bits = np.asarray(mesh_mask, bool)
            words = np.zeros((len(bits) + 31) // 32, np.uint32)
            for m, b in enumerate(bits):
                if b:
                    words[m >> 5] |= np.uint32(1 << (m & 31))
            d = to_device(words); keep.append(d)
            f.d_mesh_mask, f.mesh_mask_bits = d.data_ptr(), len(bits)
        if ignore_prim is not None:
            d = to_device(np.ascontiguousarray(ignore_prim, np.uint32)); keep.append(d)
            f.d_ignore_prim = d.data_ptr()
        if after is not None:
            a = np.ascontiguousarray(after)
            assert a.dtype == HIT_RECORD_DTYPE and a.shape[0] == n
            d = to_device(a); keep.append(d)
            f.d_after = d.data_ptr()
        if any_hit:
            d_out = torch.empty(n, dtype=torch.uint8, device="cuda")
            _check(lib().rtk_dev_trace_rays_any_filtered(self.handle, C.c_void_p(d_rays.data_ptr()), n, C.c_void_p(d_out.data_ptr()),
                                                         C.byref(f), C.byref(opts) if opts is not None else None, _stream_ptr()),
                   "rtk_dev_trace_rays_any_filtered")
            _check(lib().rtk_dev_trace_status(self.handle, _stream_ptr()), "rtk_dev_trace_status")
            return d_out.cpu().numpy().astype(bool)
        d_out = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
        _check(lib().rtk_dev_trace_rays_filtered(self.handle, C.c_void_p(d_rays.data_ptr()), n, C.c_void_p(d_out.data_ptr()),
                                                 C.byref(f), C.byref(opts) if opts is not None else None, _stream_ptr()),
               "rtk_dev_trace_rays_filtered")
        _check(lib().rtk_dev_trace_status(self.handle, _stream_ptr()), "rtk_dev_trace_status")
        return d_out.cpu().numpy().view(HIT_RECORD_DTYPE)

    def trace_any(self, rays, opts=None):
        rays = np.ascontiguousarray(rays)
        n = rays.shape[0]
        d_rays = to_device(rays)
        return self.trace_any_device(d_rays, n, opts=opts).cpu().numpy().astype(bool)

    def trace_any_counted(self, rays, opts=None):
        torch = _torch()
        if hasattr(rays, "data_ptr"):       # a torch tensor of rays already on the device ([n, 8] float32 or raw bytes)
            d_rays, n = rays, rays.numel() * rays.element_size() // 32
        else:
            rays = np.ascontiguousarray(rays)
            n = rays.shape[0]
            d_rays = to_device(rays)
        d_occ = torch.empty(n, dtype=torch.uint8, device="cuda")
        ctr = TraceCounters()
        torch.cuda.synchronize()
        _check(lib().rtk_dev_trace_rays_any_counted(self.handle, C.c_void_p(d_rays.data_ptr()), n, C.c_void_p(d_occ.data_ptr()),
                                                    C.byref(opts) if opts is not None else None, C.byref(ctr)),
               "rtk_dev_trace_rays_any_counted")
        return d_occ.cpu().numpy().astype(bool), ctr.as_dict()

    def trace_counted(self, rays, opts=None):
        torch = _torch()
        if hasattr(rays, "data_ptr"):
            d_rays, n = rays, rays.numel() * rays.element_size() // 32
        else:
            rays = np.ascontiguousarray(rays)
            n = rays.shape[0]
            d_rays = to_device(rays)
        d_rec = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
        ctr = TraceCounters()
        torch.cuda.synchronize()
        _check(lib().rtk_dev_trace_rays_counted(self.handle, C.c_void_p(d_rays.data_ptr()), n, C.c_void_p(d_rec.data_ptr()),
                                                C.byref(opts) if opts is not None else None, C.byref(ctr)),
               "rtk_dev_trace_rays_counted")
        return d_rec.cpu().numpy().view(HIT_RECORD_DTYPE), ctr.as_dict()


    def detect_image(self, rays):
        """rtk_dev_detect_image: (width, height) of the row-major image the batch is, or (0, 0)."""
        rays = np.ascontiguousarray(rays)
        d_rays = to_device(rays)
        w, h = C.c_uint32(0), C.c_uint32(0)
        _check(lib().rtk_dev_detect_image(self.handle, C.c_void_p(d_rays.data_ptr()), C.c_size_t(rays.shape[0]), C.byref(w), C.byref(h), _stream_ptr()), "rtk_dev_detect_image")
        return int(w.value), int(h.value)

    def debug_packet_entries(self, rays, width, height, target=26, max_levels=8):
        """rtk_dev_debug_packet_entries: the entry-list pre-pass of a width x height frame alone; one 512-byte record per
        64x64-pixel block, row by row (numpy, PACKET_ENTRIES_DTYPE)."""
        torch = _torch()
        d_rays = rays if hasattr(rays, "data_ptr") else to_device(np.ascontiguousarray(rays))
        assert d_rays.numel() * d_rays.element_size() == width * height * 32
        out = np.zeros((width // 64) * (height // 64), dtype=PACKET_ENTRIES_DTYPE)
        torch.cuda.synchronize()
        _check(lib().rtk_dev_debug_packet_entries(self.handle, C.c_void_p(d_rays.data_ptr()), width, height, target, max_levels,
                                                  C.c_void_p(out.ctypes.data)), "rtk_dev_debug_packet_entries")
        return out

    def trace_packet_counted(self, rays, opts):
        """rtk_dev_trace_rays_packet_counted: (records, counters of the hand-written packet kernel itself)."""
        torch = _torch()
        if hasattr(rays, "data_ptr"):
            d_rays, n = rays, rays.numel() * rays.element_size() // 32
        else:
            rays = np.ascontiguousarray(rays)
            n = rays.shape[0]
            d_rays = to_device(rays)
        d_rec = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
        ctr = PacketCounters()
        torch.cuda.synchronize()
        _check(lib().rtk_dev_trace_rays_packet_counted(self.handle, C.c_void_p(d_rays.data_ptr()), n, C.c_void_p(d_rec.data_ptr()),
                                                       C.byref(opts) if opts is not None else None, C.byref(ctr)),
               "rtk_dev_trace_rays_packet_counted")
        return d_rec.cpu().numpy().view(HIT_RECORD_DTYPE), ctr.as_dict()


class DeviceWorld:
    """An instanced world (rtk_dev_world*; include/rtk_amd.h, "Instanced worlds"): placed copies of device scenes under a small
    top tree, for rays, closest points and the three overlap queries. The object keeps its scenes alive; a scene that was refitted, split or rebuilt must be followed by
    update() before the next trace."""

    def __init__(self, handle, scenes):
        if not handle:
            raise RtkError("world creation failed: " + last_error())
        self.handle = C.c_void_p(handle)
        self.scenes = list(scenes)
        self._keep = []

    @classmethod
    def create(cls, scenes, instance_scene, placements):
        """scenes: DeviceScene objects; instance_scene: for every instance the index of its scene; placements: one 3 x 4 matrix
        per instance, array-like (n, 3, 4) or (n, 12) float32, mapping the scene's coordinates to the world's."""
        _torch()
        scenes = list(scenes)
        which = np.ascontiguousarray(instance_scene, np.uint32).reshape(-1)
        ptr, _keep = placement_ptr(placements, which.size)
        handles = (C.c_void_p * max(len(scenes), 1))(*[s.handle for s in scenes])
        return cls(lib().rtk_dev_world_create(handles, len(scenes), which.ctypes.data_as(C.POINTER(C.c_uint32)), ptr, which.size), scenes)

    def update(self, placements=None):
        """New placements for the same instances (array-like as for create, or a float32 cuda tensor of n * 12 values used where
        it is), or None: keep them and read the scenes again. Synchronous; no trace of the world may be in flight."""
        _torch()
        if placements is None:
            p = None
        elif hasattr(placements, "data_ptr"):
            p = C.c_void_p(placements.data_ptr())
        else:
            arr = placement_array(placements, self.info()["num_instances"])
            p = C.c_void_p(arr.ctypes.data)
        _check(lib().rtk_dev_world_update(self.handle, p, _stream_ptr()), "rtk_dev_world_update")

    def rebuild(self):
        """The top tree built again from the instances' current boxes (rtk_dev_world_rebuild); no answer changes."""
        _torch()
        _check(lib().rtk_dev_world_rebuild(self.handle, _stream_ptr()), "rtk_dev_world_rebuild")

    def info(self):
        i = WorldInfo()
        _check(lib().rtk_dev_world_get_info(self.handle, C.byref(i)), "rtk_dev_world_get_info")
        return i.as_dict()

    def top_scene_info(self):
        """rtk_dev_scene_get_info of the top tree (borrowed through rtk_dev_world_top_scene) as a dict."""
        i = SceneInfo()
        _check(lib().rtk_dev_scene_get_info(C.c_void_p(lib().rtk_dev_world_top_scene(self.handle)), C.byref(i)), "rtk_dev_scene_get_info")
        return i.as_dict()

    def status(self):
        """Waits for the current stream and raises if a launch of this world on it overflowed a traversal stack."""
        _check(lib().rtk_dev_world_trace_status(self.handle, _stream_ptr()), "rtk_dev_world_trace_status")

    def free(self):
        if self.handle:
            lib().rtk_dev_world_free(self.handle)
            self.handle = None
        self.scenes = []

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def _filter(self, instance_mask, ignore_instance):
        """(WorldFilter or None, the tensors it points into). instance_mask: bools per instance; ignore_instance: a cuda tensor of
        one 32-bit word per ray slot (used as it is) or array-like."""
        if instance_mask is None and ignore_instance is None:
            return None, []
        torch = _torch()
        f = WorldFilter()
        f.struct_size = C.sizeof(WorldFilter)
        keep = []
        if instance_mask is not None:
            bits = np.ascontiguousarray(instance_mask, bool).reshape(-1)
            words = np.zeros((bits.size + 31) // 32, np.uint32)
            for i in np.flatnonzero(bits):
                words[i >> 5] |= np.uint32(1 << (int(i) & 31))
            d = torch.from_numpy(words.view(np.int32)).cuda()
            f.d_instance_mask, f.instance_mask_bits = d.data_ptr(), bits.size
            keep.append(d)
        if ignore_instance is not None:
            d = ignore_instance if hasattr(ignore_instance, "data_ptr") else torch.from_numpy(np.ascontiguousarray(ignore_instance, np.uint32).view(np.int32)).cuda()
            f.d_ignore_instance = d.data_ptr()
            keep.append(d)
        return f, keep

    def trace_device(self, d_rays, n, d_records=None, d_instances=None, count=None, ids=None, instance_mask=None, ignore_instance=None):
        """Closest hits of n rays (RAY_DTYPE bytes on the device) over all instances: returns (d_records, d_instances), a uint8 cuda
        tensor of HIT_RECORD_DTYPE records (prim: the primitive id in the instance's scene) and an int32 cuda tensor of instance
        numbers (-1 = RTK_PRIM_NONE on a miss). count / ids: cuda int64 tensors naming the rays to trace; slots that are not listed
        are not written. Asynchronous on the current stream."""
        torch = _torch()
        if d_records is None:
            d_records = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
        if d_instances is None:
            d_instances = torch.empty(n, dtype=torch.int32, device="cuda")
        if ids is not None and count is None:
            raise RtkError("DeviceWorld.trace_device: ids without count (a list's length lives on the device)")
        l = make_ray_list(count, ids) if count is not None else None
        f, _keep = self._filter(instance_mask, ignore_instance)
        _check(lib().rtk_dev_world_trace_rays(self.handle, C.c_void_p(d_rays.data_ptr()), n, C.byref(l) if l is not None else None,
                                              C.byref(f) if f is not None else None, C.c_void_p(d_records.data_ptr()),
                                              C.c_void_p(d_instances.data_ptr()), _stream_ptr()), "rtk_dev_world_trace_rays")
        self._keep = _keep
        return d_records, d_instances

    def trace_any_device(self, d_rays, n, d_blocked=None, count=None, ids=None, instance_mask=None, ignore_instance=None):
        """The any-hit form of trace_device: one byte per ray, 1 where some instance has a candidate."""
        torch = _torch()
        if d_blocked is None:
            d_blocked = torch.empty(n, dtype=torch.uint8, device="cuda")
        if ids is not None and count is None:
            raise RtkError("DeviceWorld.trace_any_device: ids without count (a list's length lives on the device)")
        l = make_ray_list(count, ids) if count is not None else None
        f, _keep = self._filter(instance_mask, ignore_instance)
        _check(lib().rtk_dev_world_trace_rays_any(self.handle, C.c_void_p(d_rays.data_ptr()), n, C.byref(l) if l is not None else None,
                                                  C.byref(f) if f is not None else None, C.c_void_p(d_blocked.data_ptr()), _stream_ptr()),
               "rtk_dev_world_trace_rays_any")
        self._keep = _keep
        return d_blocked

    def trace_counted(self, rays, instance_mask=None, ignore_instance=None):
        """trace of all rays on the null stream, synchronous, with the visit counts of rtk_dev_world_trace_rays_counted: returns
        (records, instances, counts dict)."""
        torch = _torch()
        rays = np.ascontiguousarray(rays)
        n = rays.shape[0]
        d_rays = to_device(rays)
        d_rec = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
        d_inst = torch.empty(n, dtype=torch.int32, device="cuda")
        ctr = TraceCounters()
        f, _keep = self._filter(instance_mask, ignore_instance)
        torch.cuda.synchronize()
        _check(lib().rtk_dev_world_trace_rays_counted(self.handle, C.c_void_p(d_rays.data_ptr()), n, C.byref(f) if f is not None else None,
                                                      C.c_void_p(d_rec.data_ptr()), C.c_void_p(d_inst.data_ptr()), C.byref(ctr)),
               "rtk_dev_world_trace_rays_counted")
        return d_rec.cpu().numpy().view(HIT_RECORD_DTYPE), d_inst.cpu().numpy().view(np.uint32), ctr.as_dict()

    def trace(self, rays, instance_mask=None, ignore_instance=None):
        """rays: numpy RAY_DTYPE array. Returns (records, instances): HIT_RECORD_DTYPE records and uint32 instance numbers
        (0xffffffff on a miss). Waits for the stream."""
        rays = np.ascontiguousarray(rays)
        n = rays.shape[0]
        if n == 0:
            return np.zeros(0, HIT_RECORD_DTYPE), np.zeros(0, np.uint32)
        d_rec, d_inst = self.trace_device(to_device(rays), n, instance_mask=instance_mask, ignore_instance=ignore_instance)
        self.status()
        return d_rec.cpu().numpy().view(HIT_RECORD_DTYPE), d_inst.cpu().numpy().view(np.uint32)

    def trace_any(self, rays, instance_mask=None, ignore_instance=None):
        """rays: numpy RAY_DTYPE array. Returns a numpy bool array: the ray is blocked by some instance. Waits for the stream."""
        rays = np.ascontiguousarray(rays)
        n = rays.shape[0]
        if n == 0:
            return np.zeros(0, bool)
        d = self.trace_any_device(to_device(rays), n, instance_mask=instance_mask, ignore_instance=ignore_instance)
        self.status()
        return d.cpu().numpy().astype(bool)


    # -- closest points on the world (rtk_dev_world_closest_points): asynchronous on the current stream --

    def closest_points_device(self, d_queries, n, d_records=None, d_instances=None, d_points=None, count=None, ids=None, instance_mask=None,
                              ignore_instance=None, want_points=True):
        """The nearest triangle over all instances to each of n queries (POINT_QUERY_DTYPE bytes on the device): returns
        (d_records, d_instances, d_points): a uint8 cuda tensor of CLOSEST_RECORD_DTYPE records (prim: the primitive id in the
        instance's scene), an int32 cuda tensor of instance numbers (-1 = RTK_PRIM_NONE on a miss) and a uint8 cuda tensor of 3
        floats per query, world coordinates (want_points=False: NULL is passed and None returned). count / ids: cuda int64 tensors
        naming the queries to answer; slots that are not listed are not written. ignore_instance is read at the query's slot."""
        torch = _torch()
        if d_records is None:
            d_records = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
        if d_instances is None:
            d_instances = torch.empty(n, dtype=torch.int32, device="cuda")
        if not want_points:
            d_points = None
        elif d_points is None:
            d_points = torch.empty(n * 12, dtype=torch.uint8, device="cuda")
        if ids is not None and count is None:
            raise RtkError("DeviceWorld.closest_points_device: ids without count (a list's length lives on the device)")
        l = make_ray_list(count, ids) if count is not None else None
        f, _keep = self._filter(instance_mask, ignore_instance)
        _check(lib().rtk_dev_world_closest_points(self.handle, C.c_void_p(d_queries.data_ptr()), n, C.byref(l) if l is not None else None,
                                                  C.byref(f) if f is not None else None, C.c_void_p(d_records.data_ptr()),
                                                  C.c_void_p(d_instances.data_ptr()), C.c_void_p(d_points.data_ptr()) if d_points is not None else None,
                                                  _stream_ptr()), "rtk_dev_world_closest_points")
        self._keep = _keep
        return d_records, d_instances, d_points

    def closest_points_counted(self, d_queries, n, instance_mask=None, ignore_instance=None):
        """closest_points_device of all n queries on the null stream, synchronous, with the visit counts of
        rtk_dev_world_closest_points_counted: returns (d_records, d_instances, d_points, counts dict)."""
        torch = _torch()
        d_records = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
        d_instances = torch.empty(n, dtype=torch.int32, device="cuda")
        d_points = torch.empty(n * 12, dtype=torch.uint8, device="cuda")
        ctr = TraceCounters()
        f, _keep = self._filter(instance_mask, ignore_instance)
        torch.cuda.synchronize()
        _check(lib().rtk_dev_world_closest_points_counted(self.handle, C.c_void_p(d_queries.data_ptr()), n, C.byref(f) if f is not None else None,
                                                          C.c_void_p(d_records.data_ptr()), C.c_void_p(d_instances.data_ptr()),
                                                          C.c_void_p(d_points.data_ptr()), C.byref(ctr)), "rtk_dev_world_closest_points_counted")
        return d_records, d_instances, d_points, ctr.as_dict()

    def closest_points(self, points, max_dist=None, instance_mask=None, ignore_instance=None):
        """points: array-like (n, 3) float32. max_dist: a distance (scalar or one per point) beyond which a triangle does not
        count, squared in float32; None = no limit (RTK_INF). Returns (records CLOSEST_RECORD_DTYPE, instances uint32, points
        (n, 3) float32): prim == instance == 0xFFFFFFFF is a miss, whose point is the query itself. Waits for the stream."""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        n = pts.shape[0]
        q = np.zeros(n, POINT_QUERY_DTYPE)
        q["point"] = pts
        if max_dist is None:
            q["max_dist2"] = RTK_INF
        else:
            d = np.broadcast_to(np.asarray(max_dist, np.float32), (n,))
            with np.errstate(over="ignore", invalid="ignore"):
                q["max_dist2"] = d * d
        if n == 0:
            return np.zeros(0, CLOSEST_RECORD_DTYPE), np.zeros(0, np.uint32), np.zeros((0, 3), np.float32)
        d_rec, d_inst, d_pts = self.closest_points_device(to_device(q), n, instance_mask=instance_mask, ignore_instance=ignore_instance)
        self.status()
        return (d_rec.cpu().numpy().view(CLOSEST_RECORD_DTYPE), d_inst.cpu().numpy().view(np.uint32),
                d_pts.cpu().numpy().view(np.float32).reshape(n, 3))


    # -- the three overlap queries on the world (rtk_dev_world_triangles_in_box_* / _in_obb_* / _touching_*; a row of
    # WORLD_OVERLAPS each): asynchronous on the current stream. An entry is instance << 32 | prim: an int64 tensor holds them --

    def _overlap_count_device(self, fam, d_q, n, d_counts, count, ids, instance_mask, ignore_instance, skip_shared=False):
        torch = _torch()
        if d_counts is None:
            d_counts = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")[:n]
        if ids is not None and count is None:
            raise RtkError("DeviceWorld.triangles_%s_count_device: ids without count (a list's length lives on the device)" % fam.name)
        l = make_ray_list(count, ids) if count is not None else None
        f, _keep = self._filter(instance_mask, ignore_instance)
        flags = (TOUCH_SKIP_SHARED_VERTEX if skip_shared else 0,) if fam.flagged else ()
        _check(getattr(lib(), fam.stem + "_count")(self.handle, C.c_void_p(d_q.data_ptr()), n, C.byref(l) if l is not None else None,
                                                   C.byref(f) if f is not None else None, *flags, C.c_void_p(d_counts.data_ptr()), _stream_ptr()),
               fam.stem + "_count")
        self._keep = _keep
        return d_counts

    def _overlap_all_device(self, fam, d_q, n, d_offsets, d_entries, d_written, count, ids, instance_mask, ignore_instance, skip_shared=False):
        if ids is not None and count is None:
            raise RtkError("DeviceWorld.triangles_%s_all_device: ids without count (a list's length lives on the device)" % fam.name)
        l = make_ray_list(count, ids) if count is not None else None
        f, _keep = self._filter(instance_mask, ignore_instance)
        flags = (TOUCH_SKIP_SHARED_VERTEX if skip_shared else 0,) if fam.flagged else ()
        _check(getattr(lib(), fam.stem + "_all")(self.handle, C.c_void_p(d_q.data_ptr()), n, C.byref(l) if l is not None else None,
                                                 C.byref(f) if f is not None else None, *flags, C.c_void_p(d_offsets.data_ptr()),
                                                 C.c_void_p(d_entries.data_ptr()), C.c_void_p(d_written.data_ptr()) if d_written is not None else None,
                                                 _stream_ptr()), fam.stem + "_all")
        self._keep = _keep
        return d_written

    def _overlap_counted(self, fam, d_q, n, d_offsets, d_entries, d_counts, instance_mask, ignore_instance, skip_shared=False):
        torch = _torch()
        if d_counts is None:
            d_counts = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")[:n]
        ctr = TraceCounters()
        f, _keep = self._filter(instance_mask, ignore_instance)
        flags = (TOUCH_SKIP_SHARED_VERTEX if skip_shared else 0,) if fam.flagged else ()
        torch.cuda.synchronize()
        _check(getattr(lib(), fam.stem + "_counted")(self.handle, C.c_void_p(d_q.data_ptr()), n, C.byref(f) if f is not None else None, *flags,
                                                     C.c_void_p(d_offsets.data_ptr()) if d_offsets is not None else None,
                                                     C.c_void_p(d_entries.data_ptr()) if d_entries is not None else None,
                                                     C.c_void_p(d_counts.data_ptr()), C.byref(ctr)), fam.stem + "_counted")
        return d_counts, ctr.as_dict()

    def _overlap_host(self, fam, q, instance_mask, ignore_instance, skip_shared=False):
        """count, prefix sum and fill of host records q [n, fam.floats] float32 -> (counts uint32 [n], instances uint32 [total],
        prims uint32 [total]): query i's candidates are the entries sum(counts[:i]) .. + counts[i], by instance, then by primitive id"""
        torch = _torch()
        n = q.shape[0]
        if n == 0:
            return np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint32)
        d_q = to_device(q)
        if ignore_instance is not None and not hasattr(ignore_instance, "data_ptr"):
            ignore_instance = torch.from_numpy(np.ascontiguousarray(ignore_instance, np.uint32).view(np.int32)).cuda()
        d_counts = self._overlap_count_device(fam, d_q, n, None, None, None, instance_mask, ignore_instance, skip_shared)
        d_offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        d_offsets[1:] = torch.cumsum(d_counts, 0, dtype=torch.int64)
        total = int(d_offsets[n].item())                     # (the one read-back: how many entries to allocate)
        d_entries = torch.zeros(max(total, 1), dtype=torch.int64, device="cuda")
        self._overlap_all_device(fam, d_q, n, d_offsets, d_entries, None, None, None, instance_mask, ignore_instance, skip_shared)
        self.status()
        e = d_entries.cpu().numpy()[:total].view(WORLD_ENTRY_DTYPE)
        return d_counts.cpu().numpy().view(np.uint32), e["instance"].copy(), e["prim"].copy()

    def triangles_in_box_count_device(self, d_boxes, n, d_counts=None, count=None, ids=None, instance_mask=None, ignore_instance=None):
        """The number of triangles over all instances that touch each of n boxes (BOX_QUERY_DTYPE bytes on the device, or a float32
        [n, 6] cuda tensor of lo, hi; include/rtk_amd.h, "OVERLAPS ON A WORLD"): a cuda tensor of n uint32 words (d_counts: any cuda
        tensor of at least 4 n bytes; None: a new int32 tensor). count / ids: cuda int64 tensors naming the queries to answer;
        slots that are not listed are not written. instance_mask / ignore_instance as for closest_points_device; ignore_instance
        is read at the query's slot. Nothing waits for the stream."""
        return self._overlap_count_device(WORLD_OVERLAPS["in_box"], d_boxes, n, d_counts, count, ids, instance_mask, ignore_instance)

    def triangles_in_box_all_device(self, d_boxes, n, d_offsets, d_entries, d_written=None, count=None, ids=None, instance_mask=None,
                                    ignore_instance=None):
        """Box i's candidates as entries instance << 32 | prim (prim: the primitive id in the instance's scene), ascending, into
        d_entries[d_offsets[i] .. d_offsets[i + 1]): as many as the box has or the segment holds, the lowest first. d_offsets,
        d_entries: cuda int64 tensors (n + 1 offsets). d_written: a cuda tensor of 4 n bytes, or None (the call gets NULL).
        Entries beyond written[i], and outside every segment, are not written. The rest as for triangles_in_box_count_device."""
        return self._overlap_all_device(WORLD_OVERLAPS["in_box"], d_boxes, n, d_offsets, d_entries, d_written, count, ids, instance_mask, ignore_instance)

    def triangles_in_box_counted(self, d_boxes, n, d_offsets=None, d_entries=None, d_counts=None, instance_mask=None, ignore_instance=None):
        """The count form (d_offsets None) or the fill form of all n boxes on the null stream, synchronous, with the visit counts of
        rtk_dev_world_triangles_in_box_counted: returns (d_counts -- the counts, or the written numbers --, counts dict)."""
        return self._overlap_counted(WORLD_OVERLAPS["in_box"], d_boxes, n, d_offsets, d_entries, d_counts, instance_mask, ignore_instance)

    def triangles_in_box(self, boxes, instance_mask=None, ignore_instance=None):
        """boxes: array-like (n, 6) float32 of lo, hi, or BOX_QUERY_DTYPE records. A count, its prefix sum on the device and the
        fill; returns (counts uint32 [n], instances uint32 [total], prims uint32 [total]): box i's candidates are the entries
        sum(counts[:i]) .. + counts[i], by instance, then by primitive id. Waits for the stream."""
        boxes = np.asarray(boxes)
        q = np.ascontiguousarray(boxes.view(np.float32) if boxes.dtype == BOX_QUERY_DTYPE else np.asarray(boxes, np.float32)).reshape(-1, 6)
        return self._overlap_host(WORLD_OVERLAPS["in_box"], q, instance_mask, ignore_instance)

    def triangles_in_obb_count_device(self, d_obbs, n, d_counts=None, count=None, ids=None, instance_mask=None, ignore_instance=None):
        """triangles_in_box_count_device for n oriented boxes (OBB_QUERY_DTYPE bytes on the device, or a float32 [n, 15] cuda tensor
        of centre, half, axes)."""
        return self._overlap_count_device(WORLD_OVERLAPS["in_obb"], d_obbs, n, d_counts, count, ids, instance_mask, ignore_instance)

    def triangles_in_obb_all_device(self, d_obbs, n, d_offsets, d_entries, d_written=None, count=None, ids=None, instance_mask=None,
                                    ignore_instance=None):
        """triangles_in_box_all_device for n oriented boxes."""
        return self._overlap_all_device(WORLD_OVERLAPS["in_obb"], d_obbs, n, d_offsets, d_entries, d_written, count, ids, instance_mask, ignore_instance)

    def triangles_in_obb_counted(self, d_obbs, n, d_offsets=None, d_entries=None, d_counts=None, instance_mask=None, ignore_instance=None):
        """triangles_in_box_counted for n oriented boxes (rtk_dev_world_triangles_in_obb_counted)."""
        return self._overlap_counted(WORLD_OVERLAPS["in_obb"], d_obbs, n, d_offsets, d_entries, d_counts, instance_mask, ignore_instance)

    def triangles_in_obb(self, centres, half, rotation, instance_mask=None, ignore_instance=None):
        """centres, half, rotation as for DeviceScene.triangles_in_obbs; returns what triangles_in_box returns."""
        q = np.ascontiguousarray(obb_query_array(centres, half, rotation)).view(np.float32).reshape(-1, 15)
        return self._overlap_host(WORLD_OVERLAPS["in_obb"], q, instance_mask, ignore_instance)

    def triangles_touching_count_device(self, d_tris, n, d_counts=None, count=None, ids=None, instance_mask=None, ignore_instance=None,
                                        skip_shared=False):
        """triangles_in_box_count_device for n query triangles (TRI_QUERY_DTYPE bytes on the device, or a float32 [n, 9] cuda
        tensor). skip_shared: records whose placed vertices share a position with the query's are left out
        (RTK_TOUCH_SKIP_SHARED_VERTEX). There is no first_prim on a world: ignore_instance leaves a body's own triangles out."""
        return self._overlap_count_device(WORLD_OVERLAPS["touching"], d_tris, n, d_counts, count, ids, instance_mask, ignore_instance, skip_shared)

    def triangles_touching_all_device(self, d_tris, n, d_offsets, d_entries, d_written=None, count=None, ids=None, instance_mask=None,
                                      ignore_instance=None, skip_shared=False):
        """triangles_in_box_all_device for n query triangles; skip_shared as for triangles_touching_count_device."""
        return self._overlap_all_device(WORLD_OVERLAPS["touching"], d_tris, n, d_offsets, d_entries, d_written, count, ids, instance_mask,
                                        ignore_instance, skip_shared)

    def triangles_touching_counted(self, d_tris, n, d_offsets=None, d_entries=None, d_counts=None, instance_mask=None, ignore_instance=None,
                                   skip_shared=False):
        """triangles_in_box_counted for n query triangles (rtk_dev_world_triangles_touching_counted)."""
        return self._overlap_counted(WORLD_OVERLAPS["touching"], d_tris, n, d_offsets, d_entries, d_counts, instance_mask, ignore_instance, skip_shared)

    def triangles_touching(self, tris, instance_mask=None, ignore_instance=None, skip_shared=False):
        """tris: array-like (n, 9) or (n, 3, 3) float32, or TRI_QUERY_DTYPE records; returns what triangles_in_box returns."""
        tris = np.asarray(tris)
        q = np.ascontiguousarray(tris.view(np.float32) if tris.dtype == TRI_QUERY_DTYPE else np.asarray(tris, np.float32)).reshape(-1, 9)
        return self._overlap_host(WORLD_OVERLAPS["touching"], q, instance_mask, ignore_instance, skip_shared)


# -- the reference's own entry points, host pointers (reference rtk.h:126-130) --

def obb_axes(rotation, n):
    """The `axes` of n rtk_obb_sweep queries, float32 (n, 3, 3), rows = the box's own axes in scene coordinates. rotation: (n, 3, 3) or
    (3, 3) matrices with those rows, or (n, 4) or (4,) quaternions (x, y, z, w): normalised and converted in float64 -- row j is the
    image of unit vector j under the quaternion's rotation -- then rounded once to float32."""
    r = np.asarray(rotation, np.float64)
    if r.shape in ((3, 3), (n, 3, 3)):
        m = r
    elif r.shape in ((4,), (n, 4)):
        q = r.reshape(-1, 4)
        with np.errstate(all="ignore"):
            q = q / np.sqrt((q * q).sum(1, keepdims=True))
        x, y, z, w = q.T
        # (the transpose of the usual rotation matrix: its columns are the images of the unit vectors)
        m = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y + z * w), 2 * (x * z - y * w),
                      2 * (x * y - z * w), 1 - 2 * (x * x + z * z), 2 * (y * z + x * w),
                      2 * (x * z + y * w), 2 * (y * z - x * w), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)
    else:
        raise RtkError("obb_axes: rotation of shape %s: (n, 3, 3), (3, 3), (n, 4) or (4,) with n = %d" % (r.shape, n))
    return np.ascontiguousarray(np.broadcast_to(m.reshape(-1, 3, 3), (n, 3, 3)), np.float32)


def obb_query_array(centres, half, rotation):
    """n rtk_obb_query records (OBB_QUERY_DTYPE). centres: (n, 3); half: (n, 3), (3,) or a scalar; rotation: see obb_axes."""
    c = np.ascontiguousarray(centres, np.float32).reshape(-1, 3)
    n = c.shape[0]
    q = np.zeros(n, OBB_QUERY_DTYPE)
    q["centre"] = c
    h = np.asarray(half, np.float32)
    if h.shape not in ((), (3,), (n, 3)):
        raise RtkError("obb_query_array: half of shape %s: (n, 3), (3,) or a scalar with n = %d" % (h.shape, n))
    q["half"] = h if h.shape != () else np.broadcast_to(h, (n, 3))
    q["axes"] = obb_axes(rotation, n)
    return q


def oriented_grid(centre, half, rotation, shape):
    """The nx * ny * nz cells (OBB_QUERY_DTYPE, x slowest) of the grid that fills one oriented box, all in numpy float32, every
    operation rounded on its own: a cell's half extent is half[j] / n_j, its centre centre + ((a0 * u0 + a1 * u1) + a2 * u2) with
    a_j = (2 i_j + 1 - n_j) * (half[j] / n_j), and its axes are the box's."""
    shape = tuple(int(s) for s in shape)
    if len(shape) != 3 or min(shape) < 1:
        raise RtkError("oriented_grid: shape %r" % (shape,))
    F = np.float32
    box = obb_query_array(np.asarray(centre, F).reshape(1, 3), half, rotation)
    c, h, u = box["centre"][0], box["half"][0], box["axes"][0]
    ch = h / np.array(shape, F)
    a = [((2 * np.arange(shape[j]) + 1 - shape[j]).astype(F) * ch[j]).astype(F) for j in range(3)]
    a0, a1, a2 = (x.reshape(-1, 1) for x in np.meshgrid(a[0], a[1], a[2], indexing="ij"))
    q = np.zeros(shape[0] * shape[1] * shape[2], OBB_QUERY_DTYPE)
    q["centre"] = c[None, :] + ((a0 * u[0][None, :] + a1 * u[1][None, :]) + a2 * u[2][None, :])
    q["half"] = ch
    q["axes"] = u
    return q


def build_scene(meshes):
    """rtk_build_scene: returns (scene pointer, MeshSet keepalive). Release with free_scene."""
    _torch()
    ms = meshes if isinstance(meshes, MeshSet) else MeshSet(meshes)
    p = lib().rtk_build_scene(C.byref(ms.desc))
    if not p:
        raise RtkError("rtk_build_scene failed: " + last_error())
    return p, ms


def free_scene(scene_ptr):
    lib().rtk_free_scene(C.c_void_p(scene_ptr))


def scene_bytes(scene_ptr):
    hdr = SceneHeader.from_address(scene_ptr)
    return np.ctypeslib.as_array((C.c_uint8 * hdr.size_in_bytes).from_address(scene_ptr)).copy()


def trace_ray(scene_ptr, ray):
    """rtk_trace_ray: one ray (RAY_DTYPE scalar). Returns HIT_DTYPE record or None."""
    _torch()
    r = np.ascontiguousarray(ray).reshape(1)
    h = np.zeros(1, HIT_DTYPE)
    ok = lib().rtk_trace_ray(C.c_void_p(scene_ptr), r.ctypes.data, h.ctypes.data)
    return h[0] if ok else None


def trace_rays_filter(scene_ptr, rays, accept):
    """rtk_trace_rays_filter with a Python callback accept(ray_index, hit) -> bool; hit is a HIT_DTYPE record."""
    _torch()
    rays = np.ascontiguousarray(rays)
    n = rays.shape[0]
    hits = np.zeros(n, HIT_DTYPE)
    mask = np.zeros(n, np.uint8)
    base = rays.ctypes.data

    def cb(user, ray_ptr, hit_ptr):
        h = np.ctypeslib.as_array((C.c_uint8 * 68).from_address(hit_ptr)).view(HIT_DTYPE)[0]
        return bool(accept((ray_ptr - base) // 32, h))
    fn = FILTER_FN(cb)
    r = lib().rtk_trace_rays_filter(C.c_void_p(scene_ptr), rays.ctypes.data, n, hits.ctypes.data, mask.ctypes.data,
                                    C.cast(fn, C.c_void_p), None)
    if r == C.c_size_t(-1).value:
        raise RtkError("rtk_trace_rays_filter failed: " + last_error())
    return hits, mask.astype(bool)


def trace_rays(scene_ptr, rays):
    """rtk_trace_rays: host arrays in, host arrays out (PCIe inclusive)."""
    _torch()
    rays = np.ascontiguousarray(rays)
    n = rays.shape[0]
    hits = np.zeros(n, HIT_DTYPE)
    mask = np.zeros(n, np.uint8)
    r = lib().rtk_trace_rays(C.c_void_p(scene_ptr), rays.ctypes.data, n, hits.ctypes.data, mask.ctypes.data)
    if r == C.c_size_t(-1).value:
        raise RtkError("rtk_trace_rays failed: " + last_error())
    return hits, mask.astype(bool)
