"""What a scene reports as total_device_bytes, step by step through everything that makes, drops and remakes one of its
device tables: the side arrays, the refit schedule, the tables of the partial refit, the measurement's buffers, the longer
node arrays of a split. The nine figures of each scene are the library's own, recorded before the allocations got one owner
(tests/golden/scene_mem_bytes.json: run_sequence below, run at the commit before), and must not move by a
byte. Twice: the 10k-triangle scene as two meshes built on the device (leaves of at most 3: the split has nothing to do) and
the CPU task builder's blob of the same meshes uploaded (leaves of up to 63: the split renumbers the tree and drops the tables)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from rtk_amd import synth

pytestmark = pytest.mark.gpu

STEPS = ["creation", "expand", "refit", "refit_meshes", "quality", "split_leaves", "refit again", "refit_meshes again", "quality again"]
FIRST = 8000            # triangles of mesh 0; mesh 1 has the other 2000


def _meshes(scale0=1.0, scale1=1.0):
    tris = synth.scene_for_config(1)
    a, b = tris[:3 * FIRST], tris[3 * FIRST:]
    return [dict(positions=(a * np.float32(scale0)).astype(np.float32)), dict(positions=(b * np.float32(scale1)).astype(np.float32))]


def _task_builder_blob(api):
    L = api.lib()
    assert L.rtk_amd_set_builder(1) == 0
    ms = api.MeshSet(_meshes())
    try:
        scene = L.rtk_build_scene(C.byref(ms.desc))
    finally:
        L.rtk_amd_set_builder(0)
    assert scene, api.last_error()
    try:
        return np.ascontiguousarray(api.scene_bytes(scene))
    finally:
        api.free_scene(scene)


def _create(api, kind):
    return api.DeviceScene.build(_meshes()) if kind == "built" else api.DeviceScene.upload(_task_builder_blob(api))


def run_sequence(api, kind):
    """The nine steps on a new scene of `kind`. Returns (the scene, total_device_bytes after each step, what the split
    reported, the blob exported right after the split, the positions the scene has at the end)."""
    ds = _create(api, kind)
    rays = synth.rays_config1(4096)
    seen = [ds.info()["total_device_bytes"]]
    ds.trace(rays)                                              # (full hits: the expansion needs the side arrays)
    seen.append(ds.info()["total_device_bytes"])
    ds.refit(_meshes(1.01, 1.01))
    seen.append(ds.info()["total_device_bytes"])
    ds.refit([None, _meshes(1.01, 1.02)[1]], only=[1])
    seen.append(ds.info()["total_device_bytes"])
    ds.quality()
    seen.append(ds.info()["total_device_bytes"])
    split = ds.split_leaves(0)
    seen.append(ds.info()["total_device_bytes"])
    exported = ds.export_blob().copy()
    ds.refit(_meshes(1.03, 1.03))
    seen.append(ds.info()["total_device_bytes"])
    last = _meshes(1.03, 1.04)
    ds.refit([None, last[1]], only=[1])
    seen.append(ds.info()["total_device_bytes"])
    ds.quality()
    seen.append(ds.info()["total_device_bytes"])
    return ds, seen, split, exported, last


@pytest.fixture(scope="module")
def recorded(golden_dir):
    return json.load(open(os.path.join(golden_dir, "scene_mem_bytes.json")))


@pytest.mark.parametrize("kind", ["built", "uploaded"])
def test_total_device_bytes_step_by_step(api, recorded, kind):
    ds, seen, split, exported, last = run_sequence(api, kind)
    print(kind, dict(zip(STEPS, seen)), split)
    if kind == "uploaded":
        assert split["leaves_split"] > 0 and split["nodes_added"] > 0      # (else nothing was dropped and nothing remade)
    else:
        assert split["leaves_split"] == 0
    assert seen == recorded[kind]
    # the schedule and the tables made after the split belong to the new tree: the partial refit left the bits a new upload of
    # the split tree has after a full refit to the same positions
    assert 0 < ds.last_refit_nodes() < ds.info()["num_nodes"]
    ok, c = ds.validate()
    assert ok and c["loose_boxes"] == 0, c
    fresh = api.DeviceScene.upload(exported)
    fresh.refit(last)
    rays = synth.rays_config1(8192)
    rec = ds.trace(rays, full=False)
    assert (rec["prim"] != 0xFFFFFFFF).sum() > 100
    assert rec.tobytes() == fresh.trace(rays, full=False).tobytes()
    fresh.free()
    # everything is given back; the same scene made again reports what the first one did
    ds.free()
    again = _create(api, kind)
    assert again.info()["total_device_bytes"] == seen[0]
    again.free()

