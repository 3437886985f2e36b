"""CPU tests of the per-mesh refit entry points: exported, declared, and refusing bad arguments on the host before HIP is
touched (no GPU here)."""
import ctypes as C
import os

import numpy as np

from rtk_amd import api
from rtk_amd.types import MeshSet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["rtk_dev_scene_refit_meshes", "rtk_mgpu_refit_meshes", "rtk_dev_scene_last_refit_nodes"]
RTK_AMD_ERR_BAD_ARG = -2


def test_symbols_are_exported_and_declared():
    if not os.path.exists(api.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    L = C.CDLL(api.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "rtk_amd.h")).read()
    for name in SYMBOLS:
        assert hasattr(L, name), "librtk_amd.so does not export " + name
        assert name + "(" in header, "rtk_amd.h does not declare " + name
        assert name in api.RTK_AMD_H_SYMBOLS
    assert hasattr(api.DeviceScene, "last_refit_nodes")
    import inspect
    assert "only" in inspect.signature(api.DeviceScene.refit).parameters


def test_null_arguments_are_refused_without_a_gpu():
    L = api.lib()
    ms = MeshSet([dict(positions=np.zeros((3, 3), np.float32))])
    ids = (C.c_uint32 * 1)(0)
    # (NULL arguments are looked at before the scene is: any non-NULL handle will do)
    dummy = C.cast(C.create_string_buffer(8), C.c_void_p)
    assert L.rtk_dev_scene_refit_meshes(None, C.byref(ms.desc), ids, 1, None) == RTK_AMD_ERR_BAD_ARG
    assert "rtk_dev_scene_refit_meshes" in api.last_error()
    assert L.rtk_dev_scene_refit_meshes(dummy, None, ids, 1, None) == RTK_AMD_ERR_BAD_ARG
    assert "rtk_dev_scene_refit_meshes" in api.last_error()
    assert L.rtk_dev_scene_refit_meshes(dummy, C.byref(ms.desc), None, 1, None) == RTK_AMD_ERR_BAD_ARG
    assert "rtk_dev_scene_refit_meshes" in api.last_error() and "mesh_ids" in api.last_error()
    assert L.rtk_mgpu_refit_meshes(None, C.byref(ms.desc), ids, 1) == RTK_AMD_ERR_BAD_ARG
    assert "rtk_mgpu_refit_meshes" in api.last_error()
    assert L.rtk_dev_scene_last_refit_nodes(None) == 0


def test_mesh_set_of_some_describes_unlisted_meshes_by_count():
    v = np.zeros((6, 3), np.float32)
    ms = api.mesh_set_of_some([None, dict(positions=v), None], np.array([0, 5, 7, 11], np.uint64))
    assert ms.desc.num_meshes == 3
    assert [ms._arr[i].num_triangles for i in range(3)] == [5, 2, 4]
    assert ms._arr[0].position.data is None and ms._arr[2].position.data is None and ms._arr[1].position.data
