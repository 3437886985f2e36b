"""What rtk_dev_scene_split_leaves buys an imported scene, in one process: the 1 M-triangle scene (config 2) built by the CPU
task builder (leaves of 4 to 63 triangles, what a blob on disk holds), uploaded, and traced as config 2's frame (4096 x 4096
pinhole rays, image hint) three ways -- the upload as it is (the behaviour without the call), the same scene after
split_leaves(0), and the device build of the same triangles. Per tree: median frame time of 10 frames after 3 warm-up
frames, and the packet kernel's own counters (rtk_dev_trace_rays_packet_counted) on that frame. The GPU work runs in a
child process under `timeout`; a failing step ends the run and is logged.
Usage: python scripts/split_leaves_timing.py [--log profiles/split_leaves_timing.log]"""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W = H = 4096


def measure(api, torch, ds, d_rays, n, opts, what):
    d_rec = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
    ms = []
    for rep in range(13):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        ds.trace_device(d_rays, n, d_rec, opts)
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    ms = ms[3:]
    _, pk = ds.trace_packet_counted(d_rays, opts)
    info = ds.info()
    med = statistics.median(ms)
    print("%s: nodes %d, max_depth %d, device bytes %d: frame %.3f ms median (min %.3f, max %.3f) = %.2f Grays/s; packet kernel: "
          "%.2f triangle tests per ray (%d triangle-group tests), %.2f node steps per tile pair, %d of %d tiles handed back (%d triangle steps there)"
          % (what, info["num_nodes"], info["max_depth"], info["total_device_bytes"], med, min(ms), max(ms), n / med / 1e6,
             pk["triangle_group_tests"] * 64.0 / n, pk["triangle_group_tests"], pk["node_steps"] / max(pk["pairs"], 1), pk["tiles_handed_back"], pk["tiles"],
             pk["handed_back_triangle_steps"]), flush=True)
    return n / med / 1e6


def step():
    import numpy as np
    import torch
    from rtk_amd import api, synth
    tris = synth.scene_for_config(2)
    L = api.lib()
    L.rtk_amd_set_builder(1)
    t0 = time.time()
    try:
        scene, keep = api.build_scene([dict(positions=tris)])
    finally:
        L.rtk_amd_set_builder(0)
    blob = np.ascontiguousarray(api.scene_bytes(scene))
    api.free_scene(scene)
    print("scene: config 2, %d triangles; CPU task builder %.2f s, blob %d bytes" % (len(tris) // 3, time.time() - t0, blob.size), flush=True)
    rays = synth.rays_pinhole(W, H)
    n = len(rays)
    d_rays = api.to_device(rays)
    del rays
    opts = api.make_opts(image=(W, H))
    ds = api.DeviceScene.upload(blob)
    q0 = ds.quality()
    unsplit = measure(api, torch, ds, d_rays, n, opts, "uploaded blob, unsplit")
    s = ds.split_leaves(0)
    ok, c = ds.validate()
    q1 = ds.quality()
    print("split_leaves(0): %.3f ms; max_leaf %d, %d leaves split, %d nodes added, largest leaf %d -> %d, max_depth %d -> %d; validator %s; "
          "SAH triangle_tests %.2f -> %.2f, node_visits %.2f -> %.2f"
          % (s["split_ms"], s["max_leaf"], s["leaves_split"], s["nodes_added"], s["largest_leaf_before"], s["largest_leaf_after"], s["max_depth_before"],
             s["max_depth_after"], "green" if ok else "RED %r" % (c,), q0["triangle_tests"], q1["triangle_tests"], q0["node_visits"], q1["node_visits"]), flush=True)
    split = measure(api, torch, ds, d_rays, n, opts, "uploaded blob, after split_leaves(0)")
    again = api.DeviceScene.upload(blob)
    warm = again.split_leaves(0)["split_ms"]
    again.free()
    ds.free()
    built = api.DeviceScene.build([dict(positions=tris)])
    device = measure(api, torch, built, d_rays, n, opts, "device build of the same triangles")
    print("split_leaves(0) on a second upload of the blob (kernels loaded): %.3f ms" % warm)
    print("split / unsplit %.3f; split / device tree %.3f (unsplit / device tree %.3f)" % (split / unsplit, split / device, unsplit / device), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "--step":
        sys.exit(step())
    log = sys.argv[sys.argv.index("--log") + 1] if "--log" in sys.argv else os.path.join(ROOT, "profiles", "split_leaves_timing.log")
    lines = ["# scripts/split_leaves_timing.py, %s" % time.strftime("%Y-%m-%d")]
    # (the child is the only process that opens the GPU; `timeout` ends it at its limit, 124 / 137 then)
    p = subprocess.run(["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), "--step"], capture_output=True, text=True, cwd=ROOT)
    sys.stdout.write(p.stdout)
    lines += [ln for ln in p.stdout.splitlines() if ln.strip()]
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        lines.append("# FAILED (exit %d%s)" % (p.returncode, ": time limit of 420 s" if p.returncode in (124, 137) else ""))
    open(log, "w").write("\n".join(lines) + "\n")
    sys.exit(p.returncode if p.returncode >= 0 else 1)
