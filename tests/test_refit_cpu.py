"""CPU tests of the refit entry points: exported, declared, and refusing bad arguments on the host before HIP is touched
(no GPU here)."""
import ctypes as C
import os

import numpy as np

from rtk_amd import api
from rtk_amd.types import MeshSet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFIT_SYMBOLS = ["rtk_dev_scene_refit", "rtk_mgpu_refit", "rtk_dev_scene_last_refit_ms"]
RTK_AMD_ERR_BAD_ARG = -2


def test_refit_symbols_are_exported_and_declared():
    if not os.path.exists(api.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    L = C.CDLL(api.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "rtk_amd.h")).read()
    for name in REFIT_SYMBOLS:
        assert hasattr(L, name), "librtk_amd.so does not export " + name
        assert name + "(" in header, "rtk_amd.h does not declare " + name
        assert name in api.RTK_AMD_H_SYMBOLS
    assert hasattr(api.DeviceScene, "refit") and hasattr(api.DeviceScene, "last_refit_ms")


def test_null_arguments_are_refused_without_a_gpu():
    L = api.lib()
    ms = MeshSet([dict(positions=np.zeros((3, 3), np.float32))])
    rc = L.rtk_dev_scene_refit(None, C.byref(ms.desc), None)
    assert rc == RTK_AMD_ERR_BAD_ARG
    assert "rtk_dev_scene_refit" in api.last_error()
    # (a NULL description is looked at before the scene is: any non-NULL handle will do)
    dummy = C.create_string_buffer(8)
    rc = L.rtk_dev_scene_refit(C.cast(dummy, C.c_void_p), None, None)
    assert rc == RTK_AMD_ERR_BAD_ARG
    assert "rtk_dev_scene_refit" in api.last_error()
    assert L.rtk_mgpu_refit(None, C.byref(ms.desc)) == RTK_AMD_ERR_BAD_ARG
    assert "rtk_mgpu_refit" in api.last_error()
    assert L.rtk_dev_scene_last_refit_ms(None) == 0.0
