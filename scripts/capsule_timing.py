"""Steady-state wall time of rtk_dev_sweep_capsules / rtk_dev_sweep_capsules_any on the 1M-triangle synthetic scene,
device-built, 2^22 sweeps made on the device: origins uniform in the scene's bounding box, directions random with the length of
the extent, min_t = 0, max_t = 1, the radius equal to the scene's mean edge length and the half axis twice that long in a random
direction per query; in the closest and in the any-hit form, and beside them for scale, in the same process, rtk_dev_sweep_spheres
/ _any of the same paths with that radius and rtk_dev_sweep_boxes / _any of the same paths with that length as half extents.
Median of 20 calls after 5 warm-up calls with [min, max]; wall time around work that ends in a device synchronise; the
measurements alternate inside one loop, in one process. The GPU's clock state is logged before and after. Then the three sweep
sets go once through their counting forms: nodes, leaves and triangles visited and stack pushes past the on-chip part, per query.
Two GPU steps, the timing and the counting forms, each a child process of its own under its own `timeout` (each builds the
scene again, a tenth of a second); a failing step ends the run and is logged, and what the steps before it printed is kept.
Not run by any test.
Usage: python scripts/capsule_timing.py [--log profiles/capsule_timing.log]"""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS, WARM = 25, 5


def timed_together(variants, sync):
    """variants: [(name, fn)]; one call of each per round, in turn -> {name: 'median .. [min, max] ms'}, {name: median}"""
    ts = {name: [] for name, _ in variants}
    for rep in range(REPS):
        for name, fn in variants:
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            ts[name].append((time.perf_counter() - t0) * 1e3)
    text, med = {}, {}
    for name, v in ts.items():
        v = v[WARM:]
        med[name] = statistics.median(v)
        text[name] = "median %.3f [%.3f, %.3f] ms" % (med[name], min(v), max(v))
    return text, med


def step(which):
    import numpy as np
    import torch
    from rtk_amd import api, synth
    sync = torch.cuda.synchronize
    dev = "cuda"
    positions = synth.triangle_soup(1_000_000, 0.02, seed=1)
    t = positions.reshape(-1, 3, 3).astype(np.float64)
    edge = float(np.mean([np.linalg.norm(t[:, (k + 1) % 3] - t[:, k], axis=1).mean() for k in range(3)]))
    ds = api.DeviceScene.build([dict(positions=positions)])
    verts = torch.from_numpy(positions).to(dev)
    lo, hi = verts.min(0).values, verts.max(0).values
    extent = float((hi - lo).max())
    n = 1 << 22
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    origins = lo + (hi - lo) * torch.rand(n, 3, device=dev, generator=g)
    d = torch.randn(n, 3, device=dev, generator=g)
    directions = d / d.norm(dim=1, keepdim=True) * extent

    def sweeps(width):
        s = torch.empty(n, width, dtype=torch.float32, device=dev)
        s[:, 0:3], s[:, 3:6] = origins, directions
        s[:, 6], s[:, 7], s[:, 8:] = 0.0, 1.0, edge
        return s.view(torch.uint8).view(-1)

    s_box, s_ball = sweeps(11), sweeps(9)
    a = torch.randn(n, 3, device=dev, generator=g)
    s_cap = torch.empty(n, 12, dtype=torch.float32, device=dev)
    s_cap[:, 0:3], s_cap[:, 3:6] = origins, directions
    s_cap[:, 6], s_cap[:, 7], s_cap[:, 8] = 0.0, 1.0, edge
    s_cap[:, 9:12] = a / a.norm(dim=1, keepdim=True) * (2.0 * edge)
    s_cap = s_cap.view(torch.uint8).view(-1)
    if which == "counts":
        for name, c in (("capsules", ds.sweep_capsules_counted(s_cap, n)[3]), ("spheres", ds.sweep_spheres_counted(s_ball, n)[3]),
                        ("boxes", ds.sweep_boxes_counted(s_box, n)[3])):
            print("%s: %d of %d paths blocked; per query: %.1f nodes, %.1f leaves, %.1f triangles visited, %.2f pushes past the on-chip stack" % (
                name, c["hits"], n, c["nodes"] / n, c["leaves"] / n, c["triangles"] / n, c["stack_spills"] / n), flush=True)
        i = ds.info()
        print("scene: %d triangles, %d nodes, depth %d, stack entries %d (on chip: %d)" % (
            i["num_triangles"], i["num_nodes"], i["max_depth"], i["stack_entries"], api.lib().rtk_amd_capsule_stack_entries()), flush=True)
        return 0 if api.lib().rtk_dev_trace_status(ds.handle, None) == 0 else 1
    rec = torch.empty(n * 16, dtype=torch.uint8, device=dev)
    out1 = torch.empty(n * 12, dtype=torch.uint8, device=dev)
    out2 = torch.empty(n * 12, dtype=torch.uint8, device=dev)
    blocked = torch.empty(n, dtype=torch.uint8, device=dev)
    print("radius = half extents = mean edge length %.6g, |half_axis| = %.6g (extent %.6g)" % (edge, 2.0 * edge, extent), flush=True)
    text, med = timed_together([
        ("rtk_dev_sweep_capsules", lambda: ds.sweep_capsules_device(s_cap, n, rec, out1, out2)),
        ("rtk_dev_sweep_capsules_any", lambda: ds.sweep_capsules_any_device(s_cap, n, blocked)),
        ("rtk_dev_sweep_spheres", lambda: ds.sweep_spheres_device(s_ball, n, rec, out1, out2)),
        ("rtk_dev_sweep_spheres_any", lambda: ds.sweep_spheres_any_device(s_ball, n, blocked)),
        ("rtk_dev_sweep_boxes", lambda: ds.sweep_boxes_device(s_box, n, rec, out1, out2)),
        ("rtk_dev_sweep_boxes_any", lambda: ds.sweep_boxes_any_device(s_box, n, blocked)),
    ], sync)
    for k in text:
        print("n=2^22 %-32s: %s  (%.1f M/s)" % (k, text[k], n / med[k] * 1e-3), flush=True)
    print("capsule sweep / sphere sweep: %.2f (closest), %.2f (any-hit)" % (
        med["rtk_dev_sweep_capsules"] / med["rtk_dev_sweep_spheres"], med["rtk_dev_sweep_capsules_any"] / med["rtk_dev_sweep_spheres_any"]), flush=True)
    return 0 if api.lib().rtk_dev_trace_status(ds.handle, None) == 0 else 1


def clock_state():
    """what the GPU's clocks are doing, read only (the tool is optional)"""
    try:
        p = subprocess.run(["rocm-smi", "--showclocks", "--showperflevel"], capture_output=True, text=True, timeout=60)
        return ["# " + ln for ln in p.stdout.splitlines() if ln.strip() and ("clk" in ln.lower() or "level" in ln.lower())][:40]
    except (OSError, subprocess.SubprocessError) as e:
        return ["# clock state not available: %s" % e]


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "--step":
        sys.exit(step(sys.argv[2]))
    log = sys.argv[sys.argv.index("--log") + 1] if "--log" in sys.argv else os.path.join(ROOT, "profiles", "capsule_timing.log")
    lines = ["# scripts/capsule_timing.py, %s" % time.strftime("%Y-%m-%d"), "# clock state before:"] + clock_state()
    # (a child is the only process that opens the GPU; `timeout` ends it at its limit, 124 / 137 then; nothing starts after a failure)
    rc = 0
    for which, limit in (("timing", "400"), ("counts", "200")):
        p = subprocess.run(["timeout", "-k", "10", limit, sys.executable, os.path.abspath(__file__), "--step", which], capture_output=True, text=True, cwd=ROOT)
        sys.stdout.write(p.stdout)
        lines += [ln for ln in p.stdout.splitlines() if ln.strip()]
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-4000:])
            lines.append("# step %s FAILED (exit %d%s)" % (which, p.returncode, ": time limit" if p.returncode in (124, 137) else ""))
            rc = p.returncode if p.returncode > 0 else 1
            break
    lines += ["# clock state after:"] + clock_state()
    open(log, "w").write("\n".join(lines) + "\n")
    sys.exit(rc)
