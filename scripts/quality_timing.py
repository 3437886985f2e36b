"""Steady-state wall time of rtk_dev_scene_quality next to rtk_dev_scene_refit on the same scene, in one process: the
1 M-triangle scene (config 2) and the 10 M-triangle scene (config 5), device-resident float32 positions. Median, min and
max of 20 calls after 5 warm-up calls each (the first call of each kind, which makes the scene's buffers or schedule, is
timed on its own). Every GPU step runs in a child process under `timeout` with a limit of its own; the first failing step
ends the run and is logged.
Usage: python scripts/quality_timing.py [--log profiles/quality_timing.log] [--step NAME ARG]
Kernel times: rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/quality_timing.py --step quality 2
              python scripts/quality_timing.py --kernel-stats DIR        (appends the kernels' lines to the log)"""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def step_quality(cfg):
    import torch
    from rtk_amd import api, synth
    c = synth.CONFIGS[cfg]
    d0 = synth.t_triangle_soup(c["num_tris"], c["spread"], c["scene_seed"])
    ext = d0.max(0).values - d0.min(0).values
    d1 = d0 + 0.03 * ext * torch.stack([torch.sin(3.1 * d0[:, 1] / ext[1] + 1), torch.sin(2.3 * d0[:, 2] / ext[2] + 2),
                                        torch.sin(2.9 * d0[:, 0] / ext[0] + 3)], dim=1)
    d1 = d1.contiguous()
    torch.cuda.synchronize()
    ds = api.DeviceScene.build([dict(positions=d0)])
    info = ds.info()
    first = ds.quality()
    again = ds.quality()
    same = all(first[k] == again[k] for k in first if k != "measure_ms")
    ds.refit([dict(positions=d1)])
    moved = ds.quality()
    quality, refit = [], []
    for rep in range(25):
        quality.append(ds.quality()["measure_ms"])
    for rep in range(25):
        ds.refit([dict(positions=d1 if rep & 1 else d0)])
        refit.append(ds.last_refit_ms())
    back = ds.quality()                                  # (the last refit gave d0 again)
    same = same and all(first[k] == back[k] for k in first if k != "measure_ms")
    q, r = quality[5:], refit[5:]
    print("config %d: n=%d nodes=%d: quality_ms median %.3f (min %.3f, max %.3f), first call %.3f; refit_ms median %.3f (min %.3f, max %.3f); "
          "quality/refit %.2f; build_ms %.3f; sah_cost at build %.4f (node_visits %.3f, triangle_tests %.3f), after the 3 %% deformation %.4f (ratio %.4f); "
          "same bits on every call and after the refit back %s"
          % (cfg, info["num_triangles"], info["num_nodes"], statistics.median(q), min(q), max(q), first["measure_ms"], statistics.median(r), min(r), max(r),
             statistics.median(q) / statistics.median(r), info["build_ms"], first["sah_cost"], first["node_visits"], first["triangle_tests"],
             moved["sah_cost"], moved["ratio"], same), flush=True)
    return 0 if same else 1


def kernel_stats(folder):
    """The measurement's and the refit's kernels out of the *kernel_stats.csv files a rocprofv3 --kernel-trace --stats run left
    under `folder`, one line per kernel."""
    import csv
    out = []
    for base, _, files in sorted(os.walk(folder)):
        for f in sorted(files):
            if not f.endswith("kernel_stats.csv"):
                continue
            for row in csv.DictReader(open(os.path.join(base, f))):
                name = row.get("Name", "")
                if any(k in name for k in ("k_quality", "k_refit", "k_quantize")):
                    out.append("kernel %s: calls %s, average %.1f us, min %.1f us, max %.1f us, total %.3f ms"
                               % (name.split("(")[0], row["Calls"], float(row["AverageNs"]) / 1e3, float(row["MinNs"]) / 1e3, float(row["MaxNs"]) / 1e3,
                                  float(row["TotalDurationNs"]) / 1e6))
    return out


STEPS = {"quality": step_quality}

if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "--step":
        sys.exit(STEPS[sys.argv[2]](int(sys.argv[3])))
    if len(sys.argv) >= 3 and sys.argv[1] == "--kernel-stats":
        # appends to the log: python scripts/quality_timing.py --kernel-stats DIR [--log FILE]
        log = sys.argv[sys.argv.index("--log") + 1] if "--log" in sys.argv else os.path.join(ROOT, "profiles", "quality_timing.log")
        lines = ["# rocprofv3 --kernel-trace --stats -- python scripts/quality_timing.py --step quality 2 (config 2; every call of the step, warm-up included)"]
        lines += kernel_stats(sys.argv[2])
        print("\n".join(lines))
        open(log, "a").write("\n".join(lines) + "\n")
        sys.exit(0 if len(lines) > 1 else 1)
    log = sys.argv[sys.argv.index("--log") + 1] if "--log" in sys.argv else os.path.join(ROOT, "profiles", "quality_timing.log")
    lines = ["# scripts/quality_timing.py, %s" % time.strftime("%Y-%m-%d")]
    for name, arg, limit in (("quality", 2, 240), ("quality", 5, 420)):
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
