"""Steady-state wall time of rtk_dev_triangles_in_box_count / rtk_dev_triangles_in_box_all on the 1M-triangle synthetic scene,
device-built, 2^22 cubes with their centres uniform in the scene's bounding box, made on the device:
    (a) the count at a cube edge chosen so that a query has about 8 triangles on average (bisected with the count itself on
        the first 2^16 queries);
    (b) the fill with exact offsets (the inclusive prefix sum of (a)'s counts) at that edge;
    (yardstick) rtk_dev_triangles_within_count on the cubes' centres at the radius with the same mean (bisected the same way).
Median of 20 calls after 5 warm-up calls with [min, max]; wall time around work that ends in a device synchronise; the
measurements alternate inside one loop, in one process. The GPU's clock state is logged before and after. The GPU step runs in a
child process under `timeout`; a failing step ends the run and is logged. After the timing (a), (b) and the yardstick go once
through their counting forms: nodes, leaves and triangles visited and stack pushes past the on-chip part, per query.
Usage: python scripts/box_timing.py [--log profiles/box_timing.log]"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scripts.within_timing import clock_state, timed_together   # noqa: E402  (the same loop and the same clock report)

K = 8


def step():
    import torch
    from rtk_amd import api, synth
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
    centres = lo + (hi - lo) * torch.rand(n, 3, device=dev, generator=g)

    def cubes(edge):
        return torch.cat([centres - 0.5 * edge, centres + 0.5 * edge], 1).contiguous()

    def points(max2):
        q = torch.empty(n, 4, dtype=torch.float32, device=dev)
        q[:, :3] = centres
        q[:, 3] = max2
        return q.view(torch.uint8).view(-1)

    def bisect(mean_of, top):
        a, b = 0.0, top
        for _ in range(16):
            x = 0.5 * (a + b)
            a, b = (x, b) if mean_of(x) < K else (a, x)
        return 0.5 * (a + b)

    # the edge, and the radius, at which the mean count is about K: bisection with the count itself over the first 2^16 queries
    sample = 1 << 16
    edge = bisect(lambda e: float(ds.count_in_boxes_device(cubes(e), sample).float().mean()), 0.2 * extent)
    radius = bisect(lambda r: float(ds.count_within_device(points(r * r), sample).float().mean()), 0.1 * extent)
    q_box, q_pts = cubes(edge), points(radius * radius)
    counts = ds.count_in_boxes_device(q_box, n)
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(counts, 0, dtype=torch.int64)
    total = int(offsets[n].item())
    print("cube edge %.4g of the extent: %.2f triangles per query on average, %d at most, %.1f %% of the queries none; %d ids in all" % (
        edge / extent, total / n, int(counts.max().item()), 100.0 * float((counts == 0).float().mean()), total), flush=True)
    w_counts = ds.count_within_device(q_pts, n)
    print("radius %.4g of the extent: %.2f triangles within it per query on average" % (radius / extent, float(w_counts.float().mean())), flush=True)
    prims = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    written = torch.empty(n, dtype=torch.int32, device=dev)
    text, med = timed_together([
        ("(yardstick) within count, that radius", lambda: ds.count_within_device(q_pts, n, w_counts)),
        ("(a) count at that edge", lambda: ds.count_in_boxes_device(q_box, n, counts)),
        ("(b) fill, exact offsets, that edge", lambda: ds.in_boxes_all_device(q_box, n, offsets, prims, written)),
    ], sync)
    for k in text:
        print("n=2^22 %-42s: %s  (%.1f M queries/s)" % (k, text[k], n / med[k] * 1e-3), flush=True)
    for name, off in (("(a)", None), ("(b)", offsets)):
        _, c = ds.triangles_in_boxes_counted(q_box, n, off, prims if off is not None else None, written)
        print("%s per query: %.1f nodes, %.1f leaves, %.1f triangles visited, %.2f pushes past the on-chip stack; %d queries with a triangle" % (
            name, c["nodes"] / n, c["leaves"] / n, c["triangles"] / n, c["stack_spills"] / n, c["hits"]), flush=True)
    _, c = ds.triangles_within_counted(q_pts, n, None, None, None, written)
    print("(yardstick) per query: %.1f nodes, %.1f leaves, %.1f triangles visited, %.2f pushes past the on-chip stack" % (
        c["nodes"] / n, c["leaves"] / n, c["triangles"] / n, c["stack_spills"] / n), flush=True)
    i = ds.info()
    print("scene: %d triangles, %d nodes, depth %d, stack entries %d (on chip: %d)" % (
        i["num_triangles"], i["num_nodes"], i["max_depth"], i["stack_entries"], api.lib().rtk_amd_box_stack_entries()), flush=True)
    return 0 if api.lib().rtk_dev_trace_status(ds.handle, None) == 0 else 1


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "--step":
        sys.exit(step())
    log = sys.argv[sys.argv.index("--log") + 1] if "--log" in sys.argv else os.path.join(ROOT, "profiles", "box_timing.log")
    lines = ["# scripts/box_timing.py, %s" % time.strftime("%Y-%m-%d"), "# clock state before:"] + clock_state()
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
