"""Steady-state wall time of rtk_dev_triangles_within_count / rtk_dev_triangles_within_all on the 1M-triangle synthetic scene,
device-built, 2^22 queries uniform in the scene's bounding box, made on the device:
    (yardstick) rtk_dev_closest_points on the same points, without a limit and with the radius below;
    (a) the count at a radius chosen so that a query has about 8 triangles within it on average (bisected with the count
        itself on the first 2^16 queries);
    (b) the fill with exact offsets (the inclusive prefix sum of (a)'s counts) at that radius, records and points;
    (c) the fill with k = 8 (offsets i * 8) and no limit: the 8 nearest triangles of every point.
Median of 20 calls after 5 warm-up calls with [min, max]; wall time around work that ends in a device synchronise; the
measurements alternate inside one loop, in one process. The GPU's clock state is logged before and after. The GPU step runs in a
child process under `timeout`; a failing step ends the run and is logged. After the timing (a), (b) and (c) go once through the
counting form (rtk_dev_triangles_within_counted): nodes, leaves and triangles visited and stack pushes past the on-chip part, per
query.
Usage: python scripts/within_timing.py [--log profiles/within_timing.log]"""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS, WARM = 25, 5
K = 8


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
    del tris
    n = 1 << 22
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    points = lo + (hi - lo) * torch.rand(n, 3, device=dev, generator=g)

    def queries(max2):
        q = torch.empty(n, 4, dtype=torch.float32, device=dev)
        q[:, :3] = points
        q[:, 3] = max2
        return q.view(torch.uint8).view(-1)

    # the radius at which the mean count is about K: bisection with the count itself over the first 2^16 queries
    sample = 1 << 16
    r_lo, r_hi = 0.0, 0.1 * extent
    for _ in range(16):
        r = 0.5 * (r_lo + r_hi)
        mean = float(ds.count_within_device(queries(r * r), sample).float().mean())
        r_lo, r_hi = (r, r_hi) if mean < K else (r_lo, r)
    radius = 0.5 * (r_lo + r_hi)
    q_radius, q_inf = queries(radius * radius), queries(float(RTK_INF))
    counts = ds.count_within_device(q_radius, n)
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(counts, 0, dtype=torch.int64)
    total = int(offsets[n].item())
    print("radius %.4g of the extent: %.2f triangles within it per query on average, %d at most, %.1f %% of the queries none; %d records in all" % (
        radius / extent, total / n, int(counts.max().item()), 100.0 * float((counts == 0).float().mean()), total), flush=True)
    k_offsets = torch.arange(n + 1, dtype=torch.int64, device=dev) * K
    rec = torch.empty(max(total, n * K) * 16, dtype=torch.uint8, device=dev)
    pts = torch.empty(max(total, n * K) * 12, dtype=torch.uint8, device=dev)
    written = torch.empty(n, dtype=torch.int32, device=dev)
    c_rec = torch.empty(n * 16, dtype=torch.uint8, device=dev)
    c_pts = torch.empty(n * 12, dtype=torch.uint8, device=dev)
    text, med = timed_together([
        ("(yardstick) closest points, no limit", lambda: ds.closest_points_device(q_inf, n, c_rec, c_pts)),
        ("(yardstick) closest points, that radius", lambda: ds.closest_points_device(q_radius, n, c_rec, c_pts)),
        ("(a) count at that radius", lambda: ds.count_within_device(q_radius, n, counts)),
        ("(b) fill, exact offsets, that radius", lambda: ds.within_all_device(q_radius, n, offsets, rec, pts, written)),
        ("(c) fill, k = %d, no limit" % K, lambda: ds.within_all_device(q_inf, n, k_offsets, rec, pts, written)),
    ], sync)
    for k in text:
        print("n=2^22 %-42s: %s  (%.1f M queries/s)" % (k, text[k], n / med[k] * 1e-3), flush=True)
    print("(c) against the closest-points call without a limit: %.1f times its cost for %d answers per query" % (
        med["(c) fill, k = %d, no limit" % K] / med["(yardstick) closest points, no limit"], K), flush=True)
    for name, q, off in (("(a)", q_radius, None), ("(b)", q_radius, offsets), ("(c)", q_inf, k_offsets)):
        _, c = ds.triangles_within_counted(q, n, off, rec if off is not None else None, pts if off is not None else None, written)
        print("%s per query: %.1f nodes, %.1f leaves, %.1f triangles visited, %.2f pushes past the on-chip stack; %d queries with a triangle" % (
            name, c["nodes"] / n, c["leaves"] / n, c["triangles"] / n, c["stack_spills"] / n, c["hits"]), flush=True)
    _, _, c = ds.closest_points_counted(q_inf, n)
    print("(yardstick, no limit) per query: %.1f nodes, %.1f leaves, %.1f triangles visited, %.2f pushes past the on-chip stack" % (
        c["nodes"] / n, c["leaves"] / n, c["triangles"] / n, c["stack_spills"] / n), flush=True)
    i = ds.info()
    print("scene: %d triangles, %d nodes, depth %d, stack entries %d (on chip: %d)" % (
        i["num_triangles"], i["num_nodes"], i["max_depth"], i["stack_entries"], api.lib().rtk_amd_within_stack_entries()), flush=True)
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
    log = sys.argv[sys.argv.index("--log") + 1] if "--log" in sys.argv else os.path.join(ROOT, "profiles", "within_timing.log")
    lines = ["# scripts/within_timing.py, %s" % time.strftime("%Y-%m-%d"), "# clock state before:"] + clock_state()
    # (the child is the only process that opens the GPU; `timeout` ends it at its limit, 124 / 137 then)
    p = subprocess.run(["timeout", "-k", "10", "400", sys.executable, os.path.abspath(__file__), "--step"], capture_output=True, text=True, cwd=ROOT)
    sys.stdout.write(p.stdout)
    lines += [ln for ln in p.stdout.splitlines() if ln.strip()]
    lines += ["# clock state after:"] + clock_state()
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        lines.append("# step FAILED (exit %d%s)" % (p.returncode, ": time limit" if p.returncode in (124, 137) else ""))
    open(log, "w").write("\n".join(lines) + "\n")
    sys.exit(p.returncode if p.returncode >= 0 else 1)
