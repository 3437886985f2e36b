"""Steady-state wall time of rtk_dev_closest_points on the 1M-triangle synthetic scene, device-built, 2^22 queries made on the
device, no distance limit:
    (a) surface points -- a random point of a random triangle -- pushed out by 1e-3 of the scene's extent in a random direction;
    (b) points uniform in the scene's bounding box;
and beside both, as a yardstick, rtk_dev_trace_rays of the 2^22-ray incoherent closest-hit batch of the same scene.
Median of 20 calls after 5 warm-up calls with [min, max]; wall time around work that ends in a device synchronise; the three
measurements alternate inside one loop, in one process. The GPU's clock state is logged before and after. The GPU step runs in a
child process under `timeout`; a failing step ends the run and is logged. After the timing each query set goes once through the
counting form (rtk_dev_closest_points_counted): nodes, leaves and triangles visited and stack pushes past the on-chip part, per query.
Usage: python scripts/closest_timing.py [--log profiles/closest_timing.log]"""
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
    tris = torch.from_numpy(positions).to(dev).view(-1, 3, 3)
    lo, hi = tris.view(-1, 3).min(0).values, tris.view(-1, 3).max(0).values
    extent = float((hi - lo).max())
    n = 1 << 22
    g = torch.Generator(device=dev)
    g.manual_seed(7)

    def queries(points):
        q = torch.empty(n, 4, dtype=torch.float32, device=dev)
        q[:, :3] = points
        q[:, 3] = float(RTK_INF)
        return q.view(torch.uint8).view(-1)

    pick = torch.randint(0, tris.shape[0], (n,), device=dev, generator=g)
    w = torch.rand(n, 2, device=dev, generator=g)
    flip = w.sum(1) > 1.0
    w[flip] = 1.0 - w[flip]
    t = tris[pick]
    on = t[:, 0] + (t[:, 1] - t[:, 0]) * w[:, :1] + (t[:, 2] - t[:, 0]) * w[:, 1:]
    d = torch.randn(n, 3, device=dev, generator=g)
    q_surface = queries(on + d / d.norm(dim=1, keepdim=True) * (1e-3 * extent))
    q_uniform = queries(lo + (hi - lo) * torch.rand(n, 3, device=dev, generator=g))
    del pick, w, flip, t, on, d
    rays = synth.t_rays_incoherent(n, seed=3, device=dev).contiguous().view(torch.uint8).view(-1)
    rec = torch.empty(n * 16, dtype=torch.uint8, device=dev)
    pts = torch.empty(n * 12, dtype=torch.uint8, device=dev)
    hit = torch.empty(n * 16, dtype=torch.uint8, device=dev)
    text, med = timed_together([
        ("(a) closest points, surface + 1e-3 extent", lambda: ds.closest_points_device(q_surface, n, rec, pts)),
        ("(b) closest points, uniform in the box", lambda: ds.closest_points_device(q_uniform, n, rec, pts)),
        ("(yardstick) rtk_dev_trace_rays, incoherent", lambda: ds.trace_device(rays, n, hit)),
    ], sync)
    for k in text:
        print("n=2^22 %-44s: %s  (%.1f M/s)" % (k, text[k], n / med[k] * 1e-3), flush=True)
    for name, q in (("(a)", q_surface), ("(b)", q_uniform)):
        ds.closest_points_device(q, n, rec, pts)
        sync()
        r = rec.view(torch.float32).view(n, 4)
        found = int((rec.view(torch.int32).view(n, 4)[:, 3] != -1).sum().item())
        print("%s %d of %d queries answered; mean distance %.3g of the extent" % (name, found, n, float(r[:, 0].sqrt().mean()) / extent), flush=True)
        _, _, c = ds.closest_points_counted(q, n)
        print("%s per query: %.1f nodes, %.1f leaves, %.1f triangles visited, %.2f pushes past the on-chip stack" % (
            name, c["nodes"] / n, c["leaves"] / n, c["triangles"] / n, c["stack_spills"] / n), flush=True)
    i = ds.info()
    print("scene: %d triangles, %d nodes, depth %d, stack entries %d (on chip: %d)" % (
        i["num_triangles"], i["num_nodes"], i["max_depth"], i["stack_entries"], api.lib().rtk_amd_closest_stack_entries()), flush=True)
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
    log = sys.argv[sys.argv.index("--log") + 1] if "--log" in sys.argv else os.path.join(ROOT, "profiles", "closest_timing.log")
    lines = ["# scripts/closest_timing.py, %s" % time.strftime("%Y-%m-%d"), "# clock state before:"] + clock_state()
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
