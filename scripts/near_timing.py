"""Steady-state wall time of rtk_dev_triangles_near_count / rtk_dev_triangles_near_all on the 1M-triangle synthetic scene,
device-built, 2^22 query triangles of the scene's mean edge length with their first vertices uniform in the scene's bounding box,
made on the device (the workload of scripts/pair_timing.py):
    (a) the count, with the limit at which rtk_dev_triangles_within_count of the queries' centroids averages 8 per query (found
        by bisection ahead of the timing);
    (b) the fill with exact offsets (the prefix sum of (a)'s counts), both point arrays;
    (c) the fill with k = 8 (offsets i * 8) and no limit, both point arrays;
    (yardstick 1) rtk_dev_closest_triangles without a limit;
    (yardstick 2) rtk_dev_closest_triangles with that limit;
    (yardstick 3) rtk_dev_triangles_touching_count on the same queries.
Median of 20 calls after 5 warm-up calls with [min, max]; wall time around work that ends in a device synchronise; the
measurements alternate inside one loop, in one process. The GPU's clock state is logged before and after. The GPU step runs in a
child process under `timeout`; a failing step ends the run and is logged. After the timing (a), (b) and (c) go once through the
counting form: nodes, leaves and triangles visited and stack pushes past the on-chip part, per query. No time is asserted.
Usage: python scripts/near_timing.py [--log profiles/near_timing.log] [--commit TEXT]"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scripts.pair_timing import commit_text                     # noqa: E402
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
    d = torch.randn(n, 2, 3, device=dev, generator=g)
    d = d / d.norm(dim=2, keepdim=True) * mean_edge
    q_tri = torch.cat([v0, v0 + d], 1).contiguous()
    q_pt = torch.empty(n, 4, dtype=torch.float32, device=dev)
    q_pt[:, :3] = q_tri.mean(1)
    # the radius at which the within count of the centroids averages 8
    r_lo, r_hi = 0.0, 0.2 * extent
    counts = None
    for _ in range(16):
        r = 0.5 * (r_lo + r_hi)
        q_pt[:, 3] = r * r
        counts = ds.count_within_device(q_pt, n, counts)
        mean = float(counts.float().mean())
        r_lo, r_hi = (r, r_hi) if mean < 8 else (r_lo, r)
    print("query edge %.4g of the extent (the scene's mean edge); limit %.4g of the extent: %.2f triangles within it of a centroid on average" % (
        mean_edge / extent, r / extent, mean), flush=True)
    max2 = torch.full((n,), r * r, dtype=torch.float32, device=dev)
    k = 8
    n_counts = ds.count_near_device(q_tri, n, max_dist2=max2)
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(n_counts, 0, dtype=torch.int64)
    total = int(offsets[n].item())
    print("within that limit of a query triangle: %.2f triangles on average, %d at most, %d records in all" % (total / n, int(n_counts.max()), total), flush=True)
    offsets_k = torch.arange(n + 1, dtype=torch.int64, device=dev) * k
    room = max(total, n * k)
    rec = torch.empty(room * 16, dtype=torch.uint8, device=dev)
    pq, ps = torch.empty(room * 12, dtype=torch.uint8, device=dev), torch.empty(room * 12, dtype=torch.uint8, device=dev)
    written = torch.empty(n, dtype=torch.int32, device=dev)
    c_rec = torch.empty(n * 16, dtype=torch.uint8, device=dev)
    c_pq, c_ps = torch.empty(n * 12, dtype=torch.uint8, device=dev), torch.empty(n * 12, dtype=torch.uint8, device=dev)
    t_counts = torch.empty(n, dtype=torch.int32, device=dev)
    text, med = timed_together([
        ("(yardstick 1) closest triangles, no limit", lambda: ds.closest_triangles_device(q_tri, n, c_rec, c_pq, c_ps)),
        ("(yardstick 2) closest triangles, the limit", lambda: ds.closest_triangles_device(q_tri, n, c_rec, c_pq, c_ps, max_dist2=max2)),
        ("(yardstick 3) touching count", lambda: ds.count_touching_device(q_tri, n, t_counts)),
        ("(a) near count, the limit", lambda: ds.count_near_device(q_tri, n, n_counts, max_dist2=max2)),
        ("(b) near fill, exact offsets, the limit", lambda: ds.near_all_device(q_tri, n, offsets, rec, pq, ps, written, max_dist2=max2)),
        ("(c) near fill, k = 8, no limit", lambda: ds.near_all_device(q_tri, n, offsets_k, rec, pq, ps, written)),
    ], sync)
    for name in text:
        print("n=2^22 %-46s: %s  (%.1f M queries/s)" % (name, text[name], n / med[name] * 1e-3), flush=True)
    for name, kw in (("(a)", dict(max_dist2=max2)), ("(b)", dict(d_offsets=offsets, d_records=rec, d_points_query=pq, d_points_scene=ps, max_dist2=max2)),
                     ("(c)", dict(d_offsets=offsets_k, d_records=rec, d_points_query=pq, d_points_scene=ps))):
        _, c = ds.near_counted(q_tri, n, d_counts=written, **kw)
        print("%s per query: %.1f nodes, %.1f leaves, %.1f triangles fetched, %.2f pushes past the on-chip stack; %d queries with a triangle" % (
            name, c["nodes"] / n, c["leaves"] / n, c["triangles"] / n, c["stack_spills"] / n, c["hits"]), flush=True)
    i = ds.info()
    print("scene: %d triangles, %d nodes, depth %d, stack entries %d (on chip: %d)" % (
        i["num_triangles"], i["num_nodes"], i["max_depth"], i["stack_entries"], api.lib().rtk_amd_near_stack_entries()), flush=True)
    return 0 if api.lib().rtk_dev_trace_status(ds.handle, None) == 0 else 1


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "--step":
        sys.exit(step())
    log = sys.argv[sys.argv.index("--log") + 1] if "--log" in sys.argv else os.path.join(ROOT, "profiles", "near_timing.log")
    lines = ["# scripts/near_timing.py, %s, commit %s" % (time.strftime("%Y-%m-%d"), commit_text()), "# clock state before:"] + clock_state()
    # (the child is the only process that opens the GPU; `timeout` ends it at its limit, 124 / 137 then)
    p = subprocess.run(["timeout", "-k", "10", "500", sys.executable, os.path.abspath(__file__), "--step"], capture_output=True, text=True, cwd=ROOT)
    sys.stdout.write(p.stdout)
    lines += [ln for ln in p.stdout.splitlines() if ln.strip()]
    lines += ["# clock state after:"] + clock_state()
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        lines.append("# step FAILED (exit %d%s)" % (p.returncode, ": time limit" if p.returncode in (124, 137) else ""))
    open(log, "w").write("\n".join(lines) + "\n")
    sys.exit(p.returncode if p.returncode >= 0 else 1)
