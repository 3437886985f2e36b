"""Steady-state wall time of rtk_dev_triangles_touching_count / rtk_dev_triangles_touching_all on the 1M-triangle synthetic scene,
device-built, 2^22 query triangles of the scene's mean edge length with their first vertices uniform in the scene's bounding
box, made on the device:
    (a) the count;
    (b) the fill with exact offsets (the inclusive prefix sum of (a)'s counts);
    (yardstick) rtk_dev_triangles_in_box_count on the query triangles' own boxes: the walk is the same, the box rule's ten axes
        stand where the touch rule's seventeen do.
Median of 20 calls after 5 warm-up calls with [min, max]; wall time around work that ends in a device synchronise; the
measurements alternate inside one loop, in one process. The GPU's clock state is logged before and after. The GPU step runs in a
child process under `timeout`; a failing step ends the run and is logged. After the timing (a), (b) and the yardstick go once
through their counting forms: nodes, leaves and triangles visited and stack pushes past the on-chip part, per query.
Usage: python scripts/touching_timing.py [--log profiles/touching_timing.log]"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scripts.within_timing import clock_state, timed_together   # noqa: E402  (the same loop and the same clock report)


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
    edges = torch.stack([tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 1], tris[:, 0] - tris[:, 2]], 1)
    mean_edge = float(edges.norm(dim=2).mean())
    del tris, edges
    n = 1 << 22
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    v0 = lo + (hi - lo) * torch.rand(n, 1, 3, device=dev, generator=g)
    # two edges of the mean length in uniform directions from the first vertex
    d = torch.randn(n, 2, 3, device=dev, generator=g)
    d = d / d.norm(dim=2, keepdim=True) * mean_edge
    q_tri = torch.cat([v0, v0 + d], 1).contiguous()
    q_box = torch.cat([q_tri.min(1).values, q_tri.max(1).values], 1).contiguous()
    counts = ds.count_touching_device(q_tri, n)
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(counts, 0, dtype=torch.int64)
    total = int(offsets[n].item())
    print("query edge %.4g of the extent (the scene's mean edge): %.3f triangles per query on average, %d at most, %.1f %% of the queries none; %d ids in all" % (
        mean_edge / extent, total / n, int(counts.max().item()), 100.0 * float((counts == 0).float().mean()), total), flush=True)
    b_counts = ds.count_in_boxes_device(q_box, n)
    print("the queries' own boxes: %.3f triangles per box on average" % float(b_counts.float().mean()), flush=True)
    prims = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    written = torch.empty(n, dtype=torch.int32, device=dev)
    text, med = timed_together([
        ("(yardstick) box count, the queries' boxes", lambda: ds.count_in_boxes_device(q_box, n, b_counts)),
        ("(a) count", lambda: ds.count_touching_device(q_tri, n, counts)),
        ("(b) fill, exact offsets", lambda: ds.touching_all_device(q_tri, n, offsets, prims, written)),
    ], sync)
    for k in text:
        print("n=2^22 %-42s: %s  (%.1f M queries/s)" % (k, text[k], n / med[k] * 1e-3), flush=True)
    for name, off in (("(a)", None), ("(b)", offsets)):
        _, c = ds.triangles_touching_counted(q_tri, n, off, prims if off is not None else None, written)
        print("%s per query: %.1f nodes, %.1f leaves, %.1f triangles visited, %.2f pushes past the on-chip stack; %d queries with a triangle" % (
            name, c["nodes"] / n, c["leaves"] / n, c["triangles"] / n, c["stack_spills"] / n, c["hits"]), flush=True)
    _, c = ds.triangles_in_boxes_counted(q_box, n, None, None, written)
    print("(yardstick) per query: %.1f nodes, %.1f leaves, %.1f triangles visited, %.2f pushes past the on-chip stack" % (
        c["nodes"] / n, c["leaves"] / n, c["triangles"] / n, c["stack_spills"] / n), flush=True)
    i = ds.info()
    print("scene: %d triangles, %d nodes, depth %d, stack entries %d (on chip: %d)" % (
        i["num_triangles"], i["num_nodes"], i["max_depth"], i["stack_entries"], api.lib().rtk_amd_touch_stack_entries()), flush=True)
    return 0 if api.lib().rtk_dev_trace_status(ds.handle, None) == 0 else 1


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "--step":
        sys.exit(step())
    log = sys.argv[sys.argv.index("--log") + 1] if "--log" in sys.argv else os.path.join(ROOT, "profiles", "touching_timing.log")
    lines = ["# scripts/touching_timing.py, %s" % time.strftime("%Y-%m-%d"), "# clock state before:"] + clock_state()
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
