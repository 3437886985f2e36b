"""Steady-state wall time of rtk_dev_sweep_spheres / rtk_dev_sweep_spheres_any on the 1M-triangle synthetic scene, device-built,
2^22 sweeps made on the device: origins uniform in the scene's bounding box, directions random with the length of the extent,
min_t = 0, max_t = 1,
    (a) radius 0;
    (b) radius a hundredth of the scene's extent;
each in the closest and in the any-hit form, and beside them, as yardsticks in the same process, rtk_dev_closest_points of the
origins (no limit) and rtk_dev_trace_rays of the same origins and directions (closest hit, the same interval).
Median of 20 calls after 5 warm-up calls with [min, max]; wall time around work that ends in a device synchronise; the
measurements alternate inside one loop, in one process. The GPU's clock state is logged before and after. The GPU step runs in a
child process under `timeout`; a failing step ends the run and is logged. After the timing each sweep set goes once through the
counting form (rtk_dev_sweep_spheres_counted): nodes, leaves and triangles visited and stack pushes past the on-chip part, per query.
Not run by any test.
Usage: python scripts/sweep_timing.py [--log profiles/sweep_timing.log]"""
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


def step():
    import torch
    from rtk_amd import api, synth
    from rtk_amd.types import RTK_INF
    sync = torch.cuda.synchronize
    dev = "cuda"
    positions = synth.triangle_soup(1_000_000, 0.02, seed=1)
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

    def sweeps(radius):
        s = torch.empty(n, 9, dtype=torch.float32, device=dev)
        s[:, 0:3], s[:, 3:6] = origins, directions
        s[:, 6], s[:, 7], s[:, 8] = 0.0, 1.0, radius
        return s.view(torch.uint8).view(-1)

    s_point, s_ball = sweeps(0.0), sweeps(0.01 * extent)
    queries = torch.empty(n, 4, dtype=torch.float32, device=dev)
    queries[:, :3], queries[:, 3] = origins, float(RTK_INF)
    queries = queries.view(torch.uint8).view(-1)
    rays = torch.empty(n, 8, dtype=torch.float32, device=dev)
    rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7] = origins, directions, 0.0, 1.0
    rays = rays.view(torch.uint8).view(-1)
    rec = torch.empty(n * 16, dtype=torch.uint8, device=dev)
    pts = torch.empty(n * 12, dtype=torch.uint8, device=dev)
    ctr = torch.empty(n * 12, dtype=torch.uint8, device=dev)
    blocked = torch.empty(n, dtype=torch.uint8, device=dev)
    hit = torch.empty(n * 16, dtype=torch.uint8, device=dev)
    text, med = timed_together([
        ("(a) sweep, radius 0", lambda: ds.sweep_spheres_device(s_point, n, rec, pts, ctr)),
        ("(a) any-hit sweep, radius 0", lambda: ds.sweep_spheres_any_device(s_point, n, blocked)),
        ("(b) sweep, radius 0.01 extent", lambda: ds.sweep_spheres_device(s_ball, n, rec, pts, ctr)),
        ("(b) any-hit sweep, radius 0.01 extent", lambda: ds.sweep_spheres_any_device(s_ball, n, blocked)),
        ("(yardstick) rtk_dev_closest_points, origins", lambda: ds.closest_points_device(queries, n, rec, pts)),
        ("(yardstick) rtk_dev_trace_rays, same paths", lambda: ds.trace_device(rays, n, hit)),
    ], sync)
    for k in text:
        print("n=2^22 %-46s: %s  (%.1f M/s)" % (k, text[k], n / med[k] * 1e-3), flush=True)
    for name, s in (("(a)", s_point), ("(b)", s_ball)):
        _, _, _, c = ds.sweep_spheres_counted(s, n)
        print("%s %d of %d paths blocked; per query: %.1f nodes, %.1f leaves, %.1f triangles visited, %.2f pushes past the on-chip stack" % (
            name, c["hits"], n, c["nodes"] / n, c["leaves"] / n, c["triangles"] / n, c["stack_spills"] / n), flush=True)
    i = ds.info()
    print("scene: %d triangles, %d nodes, depth %d, stack entries %d (on chip: %d)" % (
        i["num_triangles"], i["num_nodes"], i["max_depth"], i["stack_entries"], api.lib().rtk_amd_sweep_stack_entries()), flush=True)
    return 0 if api.lib().rtk_dev_trace_status(ds.handle, None) == 0 else 1


def clock_state():
    """what the GPU's clocks are doing, read only (the tool is optional)"""
    try:
        p = subprocess.run(["rocm-smi", "--showclocks", "--showperflevel"], capture_output=True, text=True, timeout=60)
        return ["# " + ln for ln in p.stdout.splitlines() if ln.strip() and ("clk" in ln.lower() or "level" in ln.lower())][:40]
    except (OSError, subprocess.SubprocessError) as e:
        return ["# clock state not available: %s" % e]


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "--step":
        sys.exit(step())
    log = sys.argv[sys.argv.index("--log") + 1] if "--log" in sys.argv else os.path.join(ROOT, "profiles", "sweep_timing.log")
    lines = ["# scripts/sweep_timing.py, %s" % time.strftime("%Y-%m-%d"), "# clock state before:"] + clock_state()
    # (the child is the only process that opens the GPU; `timeout` ends it at its limit, 124 / 137 then)
    p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--step"], capture_output=True, text=True, cwd=ROOT)
    sys.stdout.write(p.stdout)
    lines += [ln for ln in p.stdout.splitlines() if ln.strip()]
    lines += ["# clock state after:"] + clock_state()
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        lines.append("# step FAILED (exit %d%s)" % (p.returncode, ": time limit" if p.returncode in (124, 137) else ""))
    open(log, "w").write("\n".join(lines) + "\n")
    sys.exit(p.returncode if p.returncode >= 0 else 1)
