"""ctypes / numpy mirrors of the POD types in include/rtk.h and include/rtk_amd.h.

Pure declarations (no compute): shared by the product binding (rtk_amd/api.py) and by
the test-only oracle binding (oracle/pyoracle.py). Sizes follow reference rtk.h:15-115
(rtk_ray 32, rtk_hit 68, rtk_vertex 16, rtk_mesh 96, rtk_scene 56, rtk_scene_desc 32).
"""
import ctypes as C

import numpy as np

RTK_INF = np.float32(3.402823e+38)  # reference rtk.h:11
RTK_NO_HIT = 0xFFFFFFFF

# -- numpy record layouts ---------------------------------------------------------------

VERTEX_DTYPE = np.dtype([("position", "<f4", (3,)), ("index", "<u4")])
RAY_DTYPE = np.dtype([("origin", "<f4", (3,)), ("direction", "<f4", (3,)), ("min_t", "<f4"), ("max_t", "<f4")])
HIT_DTYPE = np.dtype([("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("vertex", VERTEX_DTYPE, (3,)),
                      ("mesh_index", "<u4"), ("triangle_index", "<u4")])
# compact device hit record of include/rtk_amd.h
HIT_RECORD_DTYPE = np.dtype([("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("prim", "<u4")])
# rtk_point_query and rtk_closest_record of include/rtk_amd.h (rtk_dev_closest_points): the record has the shape of the hit record
POINT_QUERY_DTYPE = np.dtype([("point", "<f4", (3,)), ("max_dist2", "<f4")])
CLOSEST_RECORD_DTYPE = np.dtype([("dist2", "<f4"), ("u", "<f4"), ("v", "<f4"), ("prim", "<u4")])
# rtk_box_query of include/rtk_amd.h (rtk_dev_triangles_in_box_count / _all): a float32 [n, 6] array is one
BOX_QUERY_DTYPE = np.dtype([("lo", "<f4", (3,)), ("hi", "<f4", (3,))])
# rtk_tri_query of include/rtk_amd.h (rtk_dev_triangles_touching_count / _all): a float32 [n, 9] array is one
TRI_QUERY_DTYPE = np.dtype([("v0", "<f4", (3,)), ("v1", "<f4", (3,)), ("v2", "<f4", (3,))])
# an entry of the overlap queries on a world (rtk_dev_world_triangles_in_box_all and its kin): one little-endian uint64,
# instance << 32 | prim. An int64 / uint64 array viewed with this dtype is decoded; entries sort by instance, then by prim
WORLD_ENTRY_DTYPE = np.dtype([("prim", "<u4"), ("instance", "<u4")])
assert WORLD_ENTRY_DTYPE.itemsize == 8
# rtk_sphere_sweep of include/rtk_amd.h (rtk_dev_sweep_spheres): a float32 [n, 9] array is one; its record is HIT_RECORD_DTYPE
SPHERE_SWEEP_DTYPE = np.dtype([("origin", "<f4", (3,)), ("direction", "<f4", (3,)), ("min_t", "<f4"), ("max_t", "<f4"), ("radius", "<f4")])

assert SPHERE_SWEEP_DTYPE.itemsize == 36
# rtk_box_sweep (rtk_dev_sweep_boxes): a float32 [n, 11] array is one; its record is HIT_RECORD_DTYPE
BOX_SWEEP_DTYPE = np.dtype([("origin", "<f4", (3,)), ("direction", "<f4", (3,)), ("min_t", "<f4"), ("max_t", "<f4"), ("half", "<f4", (3,))])
assert BOX_SWEEP_DTYPE.itemsize == 44
# rtk_capsule_sweep (rtk_dev_sweep_capsules): a float32 [n, 12] array is one; its record is HIT_RECORD_DTYPE
CAPSULE_SWEEP_DTYPE = np.dtype([("origin", "<f4", (3,)), ("direction", "<f4", (3,)), ("min_t", "<f4"), ("max_t", "<f4"), ("radius", "<f4"),
                                ("half_axis", "<f4", (3,))])
assert CAPSULE_SWEEP_DTYPE.itemsize == 48
# rtk_obb_sweep (rtk_dev_sweep_obbs): a float32 [n, 20] array is one; the rows of `axes` are the box's own axes; its record is HIT_RECORD_DTYPE
OBB_SWEEP_DTYPE = np.dtype([("origin", "<f4", (3,)), ("direction", "<f4", (3,)), ("min_t", "<f4"), ("max_t", "<f4"), ("half", "<f4", (3,)),
                            ("axes", "<f4", (3, 3))])
assert OBB_SWEEP_DTYPE.itemsize == 80
# rtk_obb_query (rtk_dev_triangles_in_obb_count / _all): a float32 [n, 15] array is one; the rows of `axes` are the box's own axes
OBB_QUERY_DTYPE = np.dtype([("centre", "<f4", (3,)), ("half", "<f4", (3,)), ("axes", "<f4", (3, 3))])
assert OBB_QUERY_DTYPE.itemsize == 60
assert POINT_QUERY_DTYPE.itemsize == 16 and CLOSEST_RECORD_DTYPE.itemsize == 16 and BOX_QUERY_DTYPE.itemsize == 24
assert TRI_QUERY_DTYPE.itemsize == 36
assert VERTEX_DTYPE.itemsize == 16 and RAY_DTYPE.itemsize == 32
assert HIT_DTYPE.itemsize == 68 and HIT_RECORD_DTYPE.itemsize == 16

# rtk_type (reference rtk.h:45-52)
RTK_TYPE_DEFAULT, RTK_TYPE_F32, RTK_TYPE_F64, RTK_TYPE_REAL, RTK_TYPE_U16, RTK_TYPE_U32 = range(6)


# -- ctypes structures ------------------------------------------------------------------

class Buffer(C.Structure):
    _fields_ = [("data", C.c_void_p), ("stride", C.c_size_t), ("type", C.c_int)]


class Mesh(C.Structure):
    _fields_ = [("user", C.c_void_p), ("num_triangles", C.c_size_t),
                ("position", Buffer), ("index", Buffer),
                ("position_cb", C.c_void_p), ("position_cb_user", C.c_void_p),
                ("index_cb", C.c_void_p), ("index_cb_user", C.c_void_p)]


class SceneDesc(C.Structure):
    _fields_ = [("meshes", C.POINTER(Mesh)), ("num_meshes", C.c_size_t),
                ("log_fn", C.c_void_p), ("log_user", C.c_void_p)]


class SceneHeader(C.Structure):
    _fields_ = [("magic", C.c_char * 8), ("endian", C.c_uint16), ("sizeof_real", C.c_uint8),
                ("pad_0", C.c_uint8), ("version", C.c_uint32), ("pad_1", C.c_uint32),
                ("size_in_bytes", C.c_uint64), ("node_offset", C.c_uint64),
                ("leaf_offset", C.c_uint64), ("vertex_offset", C.c_uint64)]


class Task(C.Structure):
    _fields_ = [("build", C.c_void_p), ("fn", C.c_void_p), ("cost", C.c_double),
                ("index", C.c_size_t), ("arg", C.c_size_t)]


assert C.sizeof(Buffer) == 24 and C.sizeof(Mesh) == 96 and C.sizeof(SceneDesc) == 32
assert C.sizeof(SceneHeader) == 56 and C.sizeof(Task) == 40


class Placement(C.Structure):
    """rtk_placement: a 3 x 4 matrix row by row (include/rtk_amd.h)."""
    _fields_ = [("m", C.c_float * 12)]


assert C.sizeof(Placement) == 48


def placement_array(placements, num_meshes):
    """array-like (num_meshes, 3, 4) or (num_meshes, 12) -> the contiguous float32 [num_meshes, 12] the library reads as
    rtk_placement[num_meshes]. The values are taken as float32: anything else is rounded once, here."""
    a = np.ascontiguousarray(np.asarray(placements, np.float32).reshape(-1, 12) if np.size(placements) else np.zeros((0, 12), np.float32))
    if a.shape[0] != num_meshes:
        raise ValueError("placements: %d entries for %d meshes" % (a.shape[0], num_meshes))
    return a if a.shape[0] else np.zeros((1, 12), np.float32)      # (never a NULL pointer: NULL means "no placements given")


class MeshSet:
    """Keeps numpy buffers alive and exposes them as an rtk_scene_desc.

    meshes: list of dicts with 'positions' (float32 [nv,3] or float64) and optional
    'indices' (uint16/uint32 [nt,3]); without indices triangle i uses vertices 3i..3i+2
    (reference rtk.c:1061-1068).
    """

    def __init__(self, meshes):
        self._keep = []
        arr = (Mesh * max(1, len(meshes)))()
        self.num_triangles = 0
        for i, m in enumerate(meshes):
            me = arr[i]
            pos = m["positions"]
            if hasattr(pos, "data_ptr"):
                # a torch tensor; if it lives on the GPU the builder reads it in place (no PCIe copy)
                assert pos.is_contiguous() and pos.dim() == 2 and pos.shape[1] == 3
                f64 = str(pos.dtype) == "torch.float64"
                assert f64 or str(pos.dtype) == "torch.float32"
                self._keep.append(pos)
                me.position.data = pos.data_ptr()
                me.position.stride = 0
                me.position.type = RTK_TYPE_F64 if f64 else RTK_TYPE_F32
                assert m.get("indices") is None or hasattr(m["indices"], "data_ptr") or True
            else:
                pos = np.ascontiguousarray(pos)
                assert pos.dtype in (np.float32, np.float64) and pos.ndim == 2 and pos.shape[1] == 3
                self._keep.append(pos)
                me.position.data = pos.ctypes.data
                me.position.stride = 0
                me.position.type = RTK_TYPE_F64 if pos.dtype == np.float64 else RTK_TYPE_F32
            idx = m.get("indices")
            if idx is not None and hasattr(idx, "data_ptr"):
                assert idx.is_contiguous() and idx.dim() == 2 and idx.shape[1] == 3
                u16 = str(idx.dtype) in ("torch.uint16", "torch.int16")
                assert u16 or str(idx.dtype) in ("torch.int32", "torch.uint32")
                self._keep.append(idx)
                me.index.data = idx.data_ptr()
                me.index.stride = 0
                me.index.type = RTK_TYPE_U16 if u16 else RTK_TYPE_U32
                me.num_triangles = idx.shape[0]
            elif idx is not None:
                idx = np.ascontiguousarray(idx)
                assert idx.dtype in (np.uint16, np.uint32) and idx.ndim == 2 and idx.shape[1] == 3
                self._keep.append(idx)
                me.index.data = idx.ctypes.data
                me.index.stride = 0
                me.index.type = RTK_TYPE_U16 if idx.dtype == np.uint16 else RTK_TYPE_U32
                me.num_triangles = idx.shape[0]
            else:
                assert pos.shape[0] % 3 == 0
                me.num_triangles = pos.shape[0] // 3
            self.num_triangles += me.num_triangles
        self._arr = arr
        self.desc = SceneDesc()
        self.desc.meshes = C.cast(arr, C.POINTER(Mesh))
        self.desc.num_meshes = len(meshes)
        # global primitive id = position in concatenated mesh order (reference rtk.c:1131-1178)
        self.mesh_base = np.cumsum([0] + [arr[i].num_triangles for i in range(len(meshes))]).astype(np.uint64)


def as_rays(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == RAY_DTYPE
    return a
