"""Steady-state wall time of rtk_dev_sweep_obbs / rtk_dev_sweep_obbs_any on the 1M-triangle synthetic scene, device-built, 2^22
sweeps made on the device: origins uniform in the scene's bounding box, directions random with the length of the extent,
min_t = 0, max_t = 1, all three half extents equal to the scene's mean edge length, one random rotation per query (a uniform
unit quaternion, converted in float64 and rounded to float32); in the closest and in the any-hit form. Beside them, in the same
process: the same call with identity axes (the cost of the rotation's arithmetic alone: the grown boxes are the axis-aligned
sweep's), and rtk_dev_sweep_boxes / _any of the same paths and half extents -- the number to read the others against. The
rotated row differs from the identity row by the larger grown boxes: a cube's reach along a scene axis grows by up to sqrt(3).
Median of 20 calls after 5 warm-up calls with [min, max]; wall time around work that ends in a device synchronise; the
measurements alternate inside one loop, in one process. The GPU's clock state is logged before and after. Then the three sweep
sets go once through their counting forms: nodes, leaves and triangles visited and stack pushes past the on-chip part, per query.
Two GPU steps, the timing and the counting forms, each a child process of its own under its own `timeout` (each builds the
scene again, a tenth of a second); a failing step ends the run and is logged, and what the steps before it printed is kept.
Not run by any test.
Usage: python scripts/obbsweep_timing.py [--log profiles/obbsweep_timing.log]"""
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
    q = torch.randn(n, 4, device=dev, generator=g, dtype=torch.float64)
    x, y, z, w = (q / q.norm(dim=1, keepdim=True)).unbind(1)
    # rows are the images of the unit vectors: the transpose of the usual rotation matrix
    rows = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y + z * w), 2 * (x * z - y * w),
                        2 * (x * y - z * w), 1 - 2 * (x * x + z * z), 2 * (y * z + x * w),
                        2 * (x * z + y * w), 2 * (y * z - x * w), 1 - 2 * (x * x + y * y)], 1).to(torch.float32)

    def sweeps(width, axes=None):
        s = torch.empty(n, width, dtype=torch.float32, device=dev)
        s[:, 0:3], s[:, 3:6] = origins, directions
        s[:, 6], s[:, 7], s[:, 8:11] = 0.0, 1.0, edge
        if axes is not None:
            s[:, 11:20] = axes
        return s.view(torch.uint8).view(-1)

    s_obb, s_box = sweeps(20, rows), sweeps(11)
    s_same = sweeps(20, torch.eye(3, device=dev).reshape(1, 9))
    if which == "counts":
        for name, c in (("obbs", ds.sweep_obbs_counted(s_obb, n)[3]), ("obbs, identity axes", ds.sweep_obbs_counted(s_same, n)[3]),
                        ("boxes", ds.sweep_boxes_counted(s_box, n)[3])):
            print("%s: %d of %d paths blocked; per query: %.1f nodes, %.1f leaves, %.1f triangles visited, %.2f pushes past the on-chip stack" % (
                name, c["hits"], n, c["nodes"] / n, c["leaves"] / n, c["triangles"] / n, c["stack_spills"] / n), flush=True)
        i = ds.info()
        print("scene: %d triangles, %d nodes, depth %d, stack entries %d (on chip: %d)" % (
            i["num_triangles"], i["num_nodes"], i["max_depth"], i["stack_entries"], api.lib().rtk_amd_obbsweep_stack_entries()), flush=True)
        return 0 if api.lib().rtk_dev_trace_status(ds.handle, None) == 0 else 1
    rec = torch.empty(n * 16, dtype=torch.uint8, device=dev)
    out1 = torch.empty(n * 12, dtype=torch.uint8, device=dev)
    out2 = torch.empty(n * 12, dtype=torch.uint8, device=dev)
    blocked = torch.empty(n, dtype=torch.uint8, device=dev)
    print("half extents = mean edge length %.6g (extent %.6g)" % (edge, extent), flush=True)
    text, med = timed_together([
        ("rtk_dev_sweep_obbs", lambda: ds.sweep_obbs_device(s_obb, n, rec, out1, out2)),
        ("rtk_dev_sweep_obbs_any", lambda: ds.sweep_obbs_any_device(s_obb, n, blocked)),
        ("rtk_dev_sweep_obbs, identity axes", lambda: ds.sweep_obbs_device(s_same, n, rec, out1, out2)),
        ("rtk_dev_sweep_obbs_any, identity axes", lambda: ds.sweep_obbs_any_device(s_same, n, blocked)),
        ("rtk_dev_sweep_boxes", lambda: ds.sweep_boxes_device(s_box, n, rec, out1, out2)),
        ("rtk_dev_sweep_boxes_any", lambda: ds.sweep_boxes_any_device(s_box, n, blocked)),
    ], sync)
    for k in text:
        print("n=2^22 %-38s: %s  (%.1f M/s)" % (k, text[k], n / med[k] * 1e-3), flush=True)
    print("oriented / axis-aligned box sweep, random rotations: %.2f (closest), %.2f (any-hit)" % (
        med["rtk_dev_sweep_obbs"] / med["rtk_dev_sweep_boxes"], med["rtk_dev_sweep_obbs_any"] / med["rtk_dev_sweep_boxes_any"]), flush=True)
    print("oriented / axis-aligned box sweep, identity axes:    %.2f (closest), %.2f (any-hit)" % (
        med["rtk_dev_sweep_obbs, identity axes"] / med["rtk_dev_sweep_boxes"],
        med["rtk_dev_sweep_obbs_any, identity axes"] / med["rtk_dev_sweep_boxes_any"]), flush=True)
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
    log = sys.argv[sys.argv.index("--log") + 1] if "--log" in sys.argv else os.path.join(ROOT, "profiles", "obbsweep_timing.log")
    lines = ["# scripts/obbsweep_timing.py, %s" % time.strftime("%Y-%m-%d"), "# clock state before:"] + clock_state()
    # (a child is the only process that opens the GPU; `timeout` ends it at its limit, 124 / 137 then; nothing starts after a failure)
    rc = 0
    for which, limit in (("timing", "240"), ("counts", "120")):
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
