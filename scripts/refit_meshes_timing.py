"""Steady-state wall time of rtk_dev_scene_refit_meshes against rtk_dev_scene_refit in the same process: device-resident
float32 positions, implicit indices, the config-2 scene (1 M triangles) and the config-5 scene (10 M) cut into 64 slab
meshes along x; 1, 4, 16, 32 and 64 of the 64 meshes listed (evenly spread over the slabs). Median of 20 calls after 5
warm-up calls, min / median / max, and last_refit_nodes / num_nodes. Each count of listed meshes is measured three times:
as the library decides, with the dirty-set passes forced (RTK_AMD_REFIT_MESHES_SHARE=1) and with the full box and finish
passes forced (=0): where those two curves meet is the crossover constant of rtk_refit.hip. The scene's first per-mesh
call, which makes the tables, is reported apart. Every GPU step runs in a child process under `timeout` with a limit of
its own; the first failing step ends the run and is logged.
Usage: python scripts/refit_meshes_timing.py [--log profiles/refit_meshes_timing.log] [--step N]"""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DESIGN_FULL_MS = {1_000_000: 0.190, 10_000_000: 1.451}     # the full refit before this call existed
MESHES = 64


def stats(ts):
    ts = ts[5:]
    return min(ts), statistics.median(ts), max(ts)


def step(n):
    import torch
    from rtk_amd import api, synth
    tris = synth.triangle_soup(n, 0.02 if n <= 1_000_000 else 0.01, seed=1)
    d = torch.from_numpy(tris).cuda().reshape(-1, 3, 3)
    d = d[torch.argsort(d[:, :, 0].mean(1), stable=True)].reshape(-1, 3).contiguous()
    ext = d.max(0).values - d.min(0).values
    moved = (d + 0.03 * ext * torch.stack([torch.sin(3.1 * d[:, 1] / ext[1] + 1), torch.sin(2.3 * d[:, 2] / ext[2] + 2),
                                           torch.sin(2.9 * d[:, 0] / ext[0] + 3)], dim=1)).contiguous()
    per = (n + MESHES - 1) // MESHES
    cuts = [min(3 * per * m, 3 * n) for m in range(MESHES + 1)]
    v0 = [d[cuts[m]:cuts[m + 1]] for m in range(MESHES)]
    v1 = [moved[cuts[m]:cuts[m + 1]] for m in range(MESHES)]
    torch.cuda.synchronize()
    ds = api.DeviceScene.build([dict(positions=p) for p in v0])
    info = ds.info()
    nodes = info["num_nodes"]
    ds.refit([dict(positions=p) for p in v1])                 # (the scene's first refit: the schedule)
    full = []
    for rep in range(25):
        ds.refit([dict(positions=p) for p in (v1 if rep & 1 else v0)])
        full.append(ds.last_refit_ms())
    fmin, fmed, fmax = stats(full)
    print("n=%d meshes=%d nodes=%d: full refit min %.3f median %.3f max %.3f ms (DESIGN.md 3.4a before this call: %.3f ms)"
          % (n, MESHES, nodes, fmin, fmed, fmax, DESIGN_FULL_MS.get(n, float("nan"))), flush=True)
    t0 = time.perf_counter()
    ds.refit([dict(positions=v1[0])] + [None] * (MESHES - 1), only=[0])
    print("n=%d: first per-mesh call of the scene (tables) %.3f ms, total_device_bytes %d -> %d"
          % (n, (time.perf_counter() - t0) * 1e3, info["total_device_bytes"], ds.info()["total_device_bytes"]), flush=True)
    ok_all = True
    for k in (1, 4, 16, 32, 64):
        ids = list(range(0, MESHES, MESHES // k))
        for name, env in (("default", None), ("dirty set", "1"), ("full passes", "0")):
            if env is None:
                os.environ.pop("RTK_AMD_REFIT_MESHES_SHARE", None)
            else:
                os.environ["RTK_AMD_REFIT_MESHES_SHARE"] = env
            ts = []
            for rep in range(25):
                src = v1 if rep & 1 else v0
                ds.refit([dict(positions=src[m]) if m in ids else None for m in range(MESHES)], only=ids)
                ts.append(ds.last_refit_ms())
            mn, med, mx = stats(ts)
            print("n=%d listed %2d/%d %-11s: min %.3f median %.3f max %.3f ms, nodes %d/%d = %.4f, full/this %.2fx"
                  % (n, k, MESHES, name, mn, med, mx, ds.last_refit_nodes(), nodes, ds.last_refit_nodes() / nodes, fmed / med), flush=True)
        os.environ.pop("RTK_AMD_REFIT_MESHES_SHARE", None)
    # the scene now holds v0 everywhere but is the product of many per-mesh calls: it must be the build's, bit for bit
    ds.refit([dict(positions=p) for p in v0], only=list(range(MESHES)))
    ok, c = ds.validate()
    fresh = api.DeviceScene.build([dict(positions=p) for p in v0])
    same = fresh.validate()[1]["content_hash"] == c["content_hash"]
    print("n=%d: valid %s loose %d, hash equals a fresh build's %s" % (n, ok, c["loose_boxes"], same), flush=True)
    return 0 if ok and same and ok_all else 1


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "--step":
        sys.exit(step(int(sys.argv[2])))
    log = sys.argv[sys.argv.index("--log") + 1] if "--log" in sys.argv else os.path.join(ROOT, "profiles", "refit_meshes_timing.log")
    lines = ["# scripts/refit_meshes_timing.py, %s" % time.strftime("%Y-%m-%d")]
    for n, limit in ((1_000_000, 240), (10_000_000, 420)):
        # (the child is the only process that opens the GPU; `timeout` ends it at its limit, 124 / 137 then)
        p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", str(n)],
                           capture_output=True, text=True, cwd=ROOT)
        sys.stdout.write(p.stdout)
        lines += [ln for ln in p.stdout.splitlines() if ln.strip()]
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-4000:])
            lines.append("# step %d FAILED (exit %d%s)" % (n, p.returncode, ": time limit of %d s" % limit if p.returncode in (124, 137) else ""))
            open(log, "w").write("\n".join(lines) + "\n")
            sys.exit(p.returncode if p.returncode > 0 else 1)
    open(log, "w").write("\n".join(lines) + "\n")
