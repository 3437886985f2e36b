"""Steady-state wall time of rtk_dev_scene_refit against rtk_dev_scene_build on the same input: device-resident float32
positions, implicit indices, 1 M (config 2 scene) and 10 M (config 5 scene) triangles. Median of 20 calls after 5 warm-up
calls each; the config-2 trace throughput on build(V0) and on refit(V0) (same bytes, so it should not move). Every GPU
step runs in a child process under `timeout` with a limit of its own; the first failing step ends the run and is logged.
Usage: python scripts/refit_timing.py [--log profiles/refit_timing.log] [--step NAME ARG]"""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def step_refit(n):
    import numpy as np
    import torch
    from rtk_amd import api, synth
    tris = synth.triangle_soup(n, 0.02 if n <= 1_000_000 else 0.01, seed=1)
    d0 = torch.from_numpy(tris).cuda()
    ext = d0.max(0).values - d0.min(0).values
    d1 = d0 + 0.03 * ext * torch.stack([torch.sin(3.1 * d0[:, 1] / ext[1] + 1), torch.sin(2.3 * d0[:, 2] / ext[2] + 2),
                                        torch.sin(2.9 * d0[:, 0] / ext[0] + 3)], dim=1)
    d1 = d1.contiguous()
    torch.cuda.synchronize()
    builds = []
    for rep in range(25):
        ds = api.DeviceScene.build([dict(positions=d0)])
        builds.append(ds.info()["build_ms"])
        if rep < 24:
            ds.free()
    info = ds.info()
    t0 = time.perf_counter()
    ds.refit([dict(positions=d1)])
    first = (time.perf_counter() - t0) * 1e3
    refits = []
    for rep in range(25):
        ds.refit([dict(positions=d1 if rep & 1 else d0)])
        refits.append(ds.last_refit_ms())
    ok, c = ds.validate()
    b, r = statistics.median(builds[5:]), statistics.median(refits[5:])
    print("n=%d nodes=%d max_depth=%d: build_ms median %.3f (min %.3f), refit_ms median %.3f (min %.3f), first refit (schedule + side arrays) %.3f ms, "
          "build/refit %.2fx, valid %s loose %d" % (n, info["num_nodes"], info["max_depth"], b, min(builds[5:]), r, min(refits[5:]), first, b / r, ok,
                                                     c["loose_boxes"]), flush=True)
    return 0 if ok and r < b else 1


def step_trace(_):
    import torch
    from rtk_amd import api, synth
    tris = synth.scene_for_config(2)
    d0 = torch.from_numpy(tris).cuda()
    rays = api.to_device(synth.rays_pinhole(4096, 4096))
    n = 4096 * 4096
    opts = api.make_opts(image=(4096, 4096))
    ds = api.DeviceScene.build([dict(positions=d0)])
    out = torch.empty(n * 16, dtype=torch.uint8, device="cuda")

    def rate():
        ts = []
        for rep in range(12):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ds.trace_device(rays, n, out, opts)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return n / statistics.median(ts[2:]) / 1e9, out.cpu().numpy().tobytes()
    a, rec_a = rate()
    ds.refit([dict(positions=d0)])
    b, rec_b = rate()
    print("config 2 (4096x4096 pinhole, 1 M triangles): build(V0) %.3f Grays/s, after refit(V0) %.3f Grays/s, records identical %s"
          % (a, b, rec_a == rec_b), flush=True)
    return 0 if rec_a == rec_b else 1


STEPS = {"refit": step_refit, "trace": step_trace}

if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "--step":
        sys.exit(STEPS[sys.argv[2]](int(sys.argv[3])))
    log = sys.argv[sys.argv.index("--log") + 1] if "--log" in sys.argv else os.path.join(ROOT, "profiles", "refit_timing.log")
    lines = ["# scripts/refit_timing.py, %s" % time.strftime("%Y-%m-%d")]
    for name, arg, limit in (("refit", 1_000_000, 240), ("refit", 10_000_000, 420), ("trace", 0, 240)):
        # (the child is the only process that opens the GPU; `timeout` ends it at its limit, 124 / 137 then)
        p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, str(arg)],
                           capture_output=True, text=True, cwd=ROOT)
        sys.stdout.write(p.stdout)
        lines += [ln for ln in p.stdout.splitlines() if ln.strip()]
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-4000:])
            lines.append("# step %s %d FAILED (exit %d%s)" % (name, arg, p.returncode, ": time limit of %d s" % limit if p.returncode in (124, 137) else ""))
            open(log, "w").write("\n".join(lines) + "\n")
            sys.exit(p.returncode if p.returncode > 0 else 1)
    open(log, "w").write("\n".join(lines) + "\n")
