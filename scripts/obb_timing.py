"""Steady-state wall time of rtk_dev_triangles_in_obb_count / rtk_dev_triangles_in_obb_all on the 1M-triangle synthetic scene,
device-built, 2^22 cubes with their centres uniform in the scene's bounding box and one random rotation each (unit quaternions
made on the device, the axes rounded to float32), at the cube edge where the AXIS-ALIGNED count of the unturned cubes averages 8
triangles per query (bisected with that count on the first 2^16 queries, as scripts/box_timing.py does):
    (a) the oriented count;
    (b) the oriented fill with exact offsets (the inclusive prefix sum of (a)'s counts);
    (yardstick) rtk_dev_triangles_in_box_count on the same queries' world bounds [centre - g, centre + g]: what a host without
        this call asks for, and then filters itself. Candidates per query of both say how much it no longer filters.
    (identity) (a) and (b) once more with identity axes, beside the axis-aligned count of the same cubes: the walks are the same
        walk, so the difference is the arithmetic of the frame.
Median of 20 calls after 5 warm-up calls with [min, max]; wall time around work that ends in a device synchronise; the
measurements alternate inside one loop, in one process. The GPU's clock state is logged before and after. The GPU step runs in a
child process under `timeout`; a failing step ends the run and is logged. After the timing every form goes once through its
counting form: nodes, leaves and triangles visited and stack pushes past the on-chip part, per query.
Usage: python scripts/obb_timing.py [--log profiles/obb_timing.log]"""
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
    quat = torch.randn(n, 4, device=dev, generator=g, dtype=torch.float64)
    quat = quat / quat.norm(dim=1, keepdim=True)
    x, y, z, w = quat.unbind(1)
    # (rows = the images of the unit vectors, as rtk_amd.api.obb_axes makes them)
    turned = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y + z * w), 2 * (x * z - y * w),
                          2 * (x * y - z * w), 1 - 2 * (x * x + z * z), 2 * (y * z + x * w),
                          2 * (x * z + y * w), 2 * (y * z - x * w), 1 - 2 * (x * x + y * y)], 1).float()
    identity = torch.eye(3, device=dev).reshape(1, 9).expand(n, 9)

    def cubes(edge):
        return torch.cat([centres - 0.5 * edge, centres + 0.5 * edge], 1).contiguous()

    def obbs(edge, axes):
        return torch.cat([centres, torch.full((n, 3), 0.5 * edge, device=dev), axes], 1).contiguous()

    def bounds(q):
        """[centre - g, centre + g] in the rule's order of operations"""
        u, h = q[:, 6:15].reshape(n, 3, 3).abs(), q[:, 3:6]
        reach = (u[:, 0] * h[:, 0:1] + u[:, 1] * h[:, 1:2]) + u[:, 2] * h[:, 2:3]
        return torch.cat([q[:, 0:3] - reach, q[:, 0:3] + reach], 1).contiguous()

    a, b = 0.0, 0.2 * extent
    for _ in range(16):
        e = 0.5 * (a + b)
        a, b = (e, b) if float(ds.count_in_boxes_device(cubes(e), 1 << 16).float().mean()) < K else (a, e)
    edge = 0.5 * (a + b)
    status = 0
    for name, axes in (("turned", turned), ("identity", identity)):
        q_obb = obbs(edge, axes)
        q_box = bounds(q_obb)
        counts = ds.count_in_obbs_device(q_obb, n)
        b_counts = ds.count_in_boxes_device(q_box, n)
        offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        offsets[1:] = torch.cumsum(counts, 0, dtype=torch.int64)
        total = int(offsets[n].item())
        print("%s axes, cube edge %.4g of the extent: %.2f candidates per query in the oriented box (%d at most, %.1f %% of the queries none), "
              "%.2f in its world bounds: the host filters %.2f times fewer" % (
                  name, edge / extent, total / n, int(counts.max().item()), 100.0 * float((counts == 0).float().mean()),
                  float(b_counts.float().mean()), float(b_counts.float().mean()) / max(total / n, 1e-9)), flush=True)
        prims = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
        written = torch.empty(n, dtype=torch.int32, device=dev)
        text, med = timed_together([
            ("(yardstick) box count, world bounds", lambda: ds.count_in_boxes_device(q_box, n, b_counts)),
            ("(a) oriented count", lambda: ds.count_in_obbs_device(q_obb, n, counts)),
            ("(b) oriented fill, exact offsets", lambda: ds.in_obbs_all_device(q_obb, n, offsets, prims, written)),
        ], sync)
        for k in text:
            print("%s n=2^22 %-38s: %s  (%.1f M queries/s)" % (name, k, text[k], n / med[k] * 1e-3), flush=True)
        for form, off in (("(a)", None), ("(b)", offsets)):
            _, c = ds.triangles_in_obbs_counted(q_obb, n, off, prims if off is not None else None, written)
            print("%s %s per query: %.1f nodes, %.1f leaves, %.1f triangles visited, %.2f pushes past the on-chip stack; %d queries with a triangle" % (
                name, form, c["nodes"] / n, c["leaves"] / n, c["triangles"] / n, c["stack_spills"] / n, c["hits"]), flush=True)
        _, c = ds.triangles_in_boxes_counted(q_box, n, None, None, written)
        print("%s (yardstick) per query: %.1f nodes, %.1f leaves, %.1f triangles visited, %.2f pushes past the on-chip stack; %d queries with a triangle" % (
            name, c["nodes"] / n, c["leaves"] / n, c["triangles"] / n, c["stack_spills"] / n, c["hits"]), flush=True)
        status |= api.lib().rtk_dev_trace_status(ds.handle, None)
    i = ds.info()
    print("scene: %d triangles, %d nodes, depth %d, stack entries %d (on chip: %d)" % (
        i["num_triangles"], i["num_nodes"], i["max_depth"], i["stack_entries"], api.lib().rtk_amd_obb_stack_entries()), flush=True)
    return 0 if status == 0 else 1


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "--step":
        sys.exit(step())
    log = sys.argv[sys.argv.index("--log") + 1] if "--log" in sys.argv else os.path.join(ROOT, "profiles", "obb_timing.log")
    lines = ["# scripts/obb_timing.py, %s" % time.strftime("%Y-%m-%d"), "# clock state before:"] + clock_state()
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
