"""rtk_trace_rays (host rays in, full hits out, PCIe inclusive) where it cuts a batch into pieces: on a 200 k-triangle scene a
1024 x 704 frame (bands) and 100 000 and 1 000 000 incoherent rays (two staging sets in turn); on the config-1 scene its
1024 x 1024 frame. Minimum and median time of a call. RTK_AMD_LIB names another build of the library to compare against.
Usage: python scripts/host_batch_timing.py"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from rtk_amd import api, synth  # noqa: E402


def measure(scene, name, rays, warm, reps):
    n = len(rays)
    hits = np.zeros(n, api.HIT_DTYPE)
    mask = np.zeros(n, np.uint8)
    times = []
    for i in range(warm + reps):
        t0 = time.perf_counter()
        r = api.lib().rtk_trace_rays(api.C.c_void_p(scene), rays.ctypes.data, n, hits.ctypes.data, mask.ctypes.data)
        dt = time.perf_counter() - t0
        assert r == int(mask.sum())
        if i >= warm:
            times.append(dt)
    print("rtk_trace_rays %s: min %.3f ms, median %.3f ms (%d calls, %d hits)" % (name, min(times) * 1e3, float(np.median(times)) * 1e3, reps, r), flush=True)


scene, keep = api.build_scene([dict(positions=synth.triangle_soup(200_000, 0.03, seed=5))])
measure(scene, "frame 1024x704", synth.rays_pinhole(1024, 704), 2, 15)
measure(scene, "incoherent 100000", synth.rays_incoherent(100_000), 2, 30)
measure(scene, "incoherent 1000000", synth.rays_incoherent(1_000_000), 2, 8)
api.free_scene(scene)
scene, keep = api.build_scene([dict(positions=synth.scene_for_config(1))])
measure(scene, "config-1 frame 1048576 rays", synth.rays_config1(1048576), 3, 40)
api.free_scene(scene)
