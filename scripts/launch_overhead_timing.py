"""Host overhead of a trace launch: CALLS rtk_dev_trace_rays calls of 64 rays each on one stream, one wait at the end, RUNS times.
64 rays are one workgroup: no queue, no counter reset, no image look -- argument checks, the plan, the scratch set of (scene,
stream) and one kernel launch. The rays start outside the scene and point away from it, so that the kernel ends at the root and
the host is what is timed (64 incoherent rays keep one workgroup busy for ~125 us: the stream fills and every call waits for the
GPU; RTK_LAUNCH_TIMING_RAYS=incoherent measures that). Prints microseconds per call until the last call returned and until the
stream was idle, of each run (a warm-up run ahead of them is not printed). Usage: launch_overhead_timing.py [CALLS [RUNS]]
(default 10000 3)."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from rtk_amd import api, synth  # noqa: E402


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    ds = api.DeviceScene.build([dict(positions=synth.scene_for_config(1))])
    rays = synth.rays_incoherent(64)
    if os.environ.get("RTK_LAUNCH_TIMING_RAYS", "miss") != "incoherent":
        rays["origin"] = 2.0
        rays["direction"] = 1.0
    d_rays = api.to_device(rays)
    d_rec = torch.empty(64 * 16, dtype=torch.uint8, device="cuda")
    fn = api.lib().rtk_dev_trace_rays
    with torch.cuda.stream(torch.cuda.Stream()):
        args = (ds.handle, C.c_void_p(d_rays.data_ptr()), C.c_size_t(64), C.c_void_p(d_rec.data_ptr()), None, api._stream_ptr())
        torch.cuda.synchronize()
        for run in range(runs + 1):                # (the first run warms up and is not printed)
            bad = 0
            t0 = time.perf_counter()
            for _ in range(calls):
                bad |= fn(*args)
            t_enqueued = time.perf_counter()
            torch.cuda.current_stream().synchronize()
            t1 = time.perf_counter()
            assert bad == 0, api.last_error()
            if run:
                print("%d calls of 64 rays, one wait: %.3f us per call enqueued, %.3f us per call done" %
                      (calls, (t_enqueued - t0) / calls * 1e6, (t1 - t0) / calls * 1e6), flush=True)
        assert api.lib().rtk_dev_trace_status(ds.handle, api._stream_ptr()) == 0


if __name__ == "__main__":
    main()
