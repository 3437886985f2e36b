"""What rtk_dev_scene_rebuild costs and what it buys, in one process. (1) At 1 M and 10 M triangles: rebuild_ms of a device-built
scene beside rtk_dev_scene_build from device-resident implicit float32 positions of the same geometry -- medians of 10 calls
after 3 warm-up calls each --, then both once more under RTK_AMD_BUILD_TIMING for the per-stage split. (2) The 1 M-triangle
scene (config 2) built by the CPU task builder and uploaded: config 2's frame (4096 x 4096 pinhole rays, image hint) on the
blob as uploaded, after rebuild(), and on the device build of the same triangles -- median of 10 frames after 3 warm-up frames.
The GPU work runs in a child process under `timeout`; a failing step ends the run and is logged.
Usage: python scripts/rebuild_timing.py [--log profiles/rebuild_timing.log]"""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W = H = 4096


def frame_rate(api, torch, ds, d_rays, n, opts, what):
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
    info = ds.info()
    med = statistics.median(ms)
    print("%s: nodes %d, max_depth %d, device bytes %d: frame %.3f ms median (min %.3f, max %.3f) = %.2f Grays/s"
          % (what, info["num_nodes"], info["max_depth"], info["total_device_bytes"], med, min(ms), max(ms), n / med / 1e6), flush=True)
    return n / med / 1e6


def build_and_rebuild(api, torch, synth, num_tris):
    d_pos = synth.t_triangle_soup(num_tris, 0.02 if num_tris <= 1_000_000 else 0.01, seed=1)
    torch.cuda.synchronize()
    meshes = [dict(positions=d_pos)]
    build_ms = []
    for rep in range(13):
        ds = api.DeviceScene.build(meshes)
        build_ms.append(ds.info()["build_ms"])
        if rep < 12:
            ds.free()
    want = ds.validate()[1]["content_hash"]
    rebuild_ms, key_bits = [], 0
    for rep in range(13):
        r = ds.rebuild()
        rebuild_ms.append(r["rebuild_ms"])
        key_bits = r["key_bits"]
    ok, c = ds.validate()
    same = ok and c["content_hash"] == want
    b, r = build_ms[3:], rebuild_ms[3:]
    print("%d triangles (device-resident implicit float32, %d key bits): rtk_dev_scene_build %.3f ms median (min %.3f, max %.3f); "
          "rtk_dev_scene_rebuild %.3f ms median (min %.3f, max %.3f) = build + %.3f ms; %d nodes; hash after 13 rebuilds %s"
          % (num_tris, key_bits, statistics.median(b), min(b), max(b), statistics.median(r), min(r), max(r), statistics.median(r) - statistics.median(b),
             ds.info()["num_nodes"], "equal to the build's" if same else "DIFFERS"), flush=True)
    # the per-stage split (a device synchronisation after every stage: the stages add up to more than the figures above)
    sys.stdout.flush()
    os.environ["RTK_AMD_BUILD_TIMING"] = "1"
    try:
        print("stages of rtk_dev_scene_build at %d triangles:" % num_tris, flush=True)
        api.DeviceScene.build(meshes).free()
        print("stages of rtk_dev_scene_rebuild at %d triangles:" % num_tris, flush=True)
        ds.rebuild()
    finally:
        del os.environ["RTK_AMD_BUILD_TIMING"]
    ds.free()
    return same


def step():
    import numpy as np
    import torch
    from rtk_amd import api, synth
    os.dup2(1, 2)                                            # (the library prints its stage times on stderr: one stream, in order)
    ok = True
    for num_tris in (1_000_000, 10_000_000):
        ok = build_and_rebuild(api, torch, synth, num_tris) and ok
    api.lib().rtk_amd_release_workspace()
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
    uploaded = frame_rate(api, torch, ds, d_rays, n, opts, "uploaded blob, as it is")
    r = ds.rebuild()
    valid, c = ds.validate()
    q1 = ds.quality()
    print("rebuild(): %.3f ms (first call of the process on a blob: the staging of the vertex indices included); %d key bits, nodes %d -> %d, max_depth %d -> %d; "
          "validator %s; SAH cost %.2f -> %.2f" % (r["rebuild_ms"], r["key_bits"], r["nodes_before"], r["nodes_after"], r["max_depth_before"], r["max_depth_after"],
                                                     "green" if valid else "RED %r" % (c,), q0["sah_cost"], q1["sah_cost"]), flush=True)
    rebuilt = frame_rate(api, torch, ds, d_rays, n, opts, "uploaded blob, after rebuild()")
    built = api.DeviceScene.build([dict(positions=tris)])
    same = valid and built.validate()[1]["content_hash"] == c["content_hash"]
    device = frame_rate(api, torch, built, d_rays, n, opts, "device build of the same triangles")
    print("content hash of the rebuilt blob %s the device build's; rebuilt / uploaded %.3f; rebuilt / device tree %.3f"
          % ("equals" if same else "DIFFERS FROM", rebuilt / uploaded, rebuilt / device), flush=True)
    return 0 if ok and same else 1


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "--step":
        sys.exit(step())
    log = sys.argv[sys.argv.index("--log") + 1] if "--log" in sys.argv else os.path.join(ROOT, "profiles", "rebuild_timing.log")
    lines = ["# scripts/rebuild_timing.py, %s" % time.strftime("%Y-%m-%d")]
    # (the child is the only process that opens the GPU; `timeout` ends it at its limit, 124 / 137 then)
    p = subprocess.run(["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), "--step"], capture_output=True, text=True, cwd=ROOT)
    sys.stdout.write(p.stdout)
    lines += [ln for ln in p.stdout.splitlines() if ln.strip()]
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        lines.append("# FAILED (exit %d%s)" % (p.returncode, ": time limit of 420 s" if p.returncode in (124, 137) else ""))
    open(log, "w").write("\n".join(lines) + "\n")
    sys.exit(p.returncode if p.returncode >= 0 else 1)
