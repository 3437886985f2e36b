"""Steady-state wall time of rtk_dev_signed_distances on the 1M-triangle synthetic scene (the benchmark scene's size), device-built,
2^22 queries made on the device -- surface points pushed out by 1e-3 of the scene's extent in a random direction -- no limit:
    table     the making of the table of pseudonormals (rtk_dev_scene_prepare_signs after a refit has dropped it: table_ms of
              rtk_dev_sign_info), beside rtk_dev_scene_rebuild's time from profiles/rebuild_timing.log;
    signed    rtk_dev_signed_distances against rtk_dev_closest_points on the same queries in the same loop;
    parity    the same against the route there was before: rtk_dev_trace_rays_count with one ray per point (+x, no limit),
              whose count's parity is the side.
Median of 20 calls after 5 warm-up calls with [min, max]; wall time around work that ends in a device synchronise; the
measurements alternate inside one loop, in one process. The scene is a triangle soup: the timing does not care, the sign of
course means nothing there (the counts say so). The GPU step runs in a child process under `timeout`; a failing step ends the
run and is logged. No threshold is set on any figure: the log is the record.
Usage: python scripts/signed_timing.py [--log profiles/signed_timing.log]"""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scripts.closest_timing import clock_state, timed_together  # noqa: E402


def step():
    import torch
    from rtk_amd import api, synth
    from rtk_amd.types import RTK_INF
    sync = torch.cuda.synchronize
    dev = "cuda"
    positions = synth.triangle_soup(1_000_000, 0.02, seed=1)
    d_pos = torch.from_numpy(positions).to(dev)
    ds = api.DeviceScene.build([dict(positions=d_pos)])
    tris = d_pos.view(-1, 3, 3)
    lo, hi = tris.view(-1, 3).min(0).values, tris.view(-1, 3).max(0).values
    extent = float((hi - lo).max())
    n = 1 << 22
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    pick = torch.randint(0, tris.shape[0], (n,), device=dev, generator=g)
    w = torch.rand(n, 2, device=dev, generator=g)
    flip = w.sum(1) > 1.0
    w[flip] = 1.0 - w[flip]
    t = tris[pick]
    on = t[:, 0] + (t[:, 1] - t[:, 0]) * w[:, :1] + (t[:, 2] - t[:, 0]) * w[:, 1:]
    d = torch.randn(n, 3, device=dev, generator=g)
    points = on + d / d.norm(dim=1, keepdim=True) * (1e-3 * extent)
    q = torch.empty(n, 4, dtype=torch.float32, device=dev)
    q[:, :3] = points
    q[:, 3] = float(RTK_INF)
    q = q.view(torch.uint8).view(-1)
    rays = torch.zeros(n, 8, dtype=torch.float32, device=dev)               # rtk_ray: origin, direction, min_t, max_t
    rays[:, :3] = points
    rays[:, 3] = 1.0
    rays[:, 7] = float(RTK_INF)
    rays = rays.view(torch.uint8).view(-1)
    del pick, w, flip, t, on, d
    # the table: made, dropped by a refit to the same positions, made again -- five times
    ms = []
    for _ in range(6):
        ms.append(ds.prepare_signs()["table_ms"])
        ds.refit([dict(positions=d_pos)])
    ms = ms[1:]
    info = ds.prepare_signs()
    print("table: table_ms median %.3f [%.3f, %.3f] ms for %d triangles, %d bytes (%d places, %d degenerate records); rtk_dev_scene_rebuild of "
          "the same size: 0.996 ms (profiles/rebuild_timing.log)" % (statistics.median(ms), min(ms), max(ms), ds.info()["num_triangles"],
                                                                     info["table_bytes"], info["places"], info["degenerate_triangles"]), flush=True)
    rec = torch.empty(n * 16, dtype=torch.uint8, device=dev)
    pts = torch.empty(n * 12, dtype=torch.uint8, device=dev)
    sg = torch.empty(n, dtype=torch.float32, device=dev)
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    text, med = timed_together([
        ("rtk_dev_signed_distances", lambda: ds.signed_distances_device(q, n, rec, pts, sg)),
        ("rtk_dev_closest_points", lambda: ds.closest_points_device(q, n, rec, pts)),
        ("rtk_dev_trace_rays_count, one ray per point", lambda: ds.count_hits_device(rays, n, cnt)),
    ], sync)
    for k in text:
        print("n=2^22 %-44s: %s  (%.1f M/s)" % (k, text[k], n / med[k] * 1e-3), flush=True)
    print("signed: %.1f M queries/s against closest points %.1f M/s on the same queries (x %.3f the time)" % (
        n / med["rtk_dev_signed_distances"] * 1e-3, n / med["rtk_dev_closest_points"] * 1e-3, med["rtk_dev_signed_distances"] / med["rtk_dev_closest_points"]), flush=True)
    print("parity: %.1f M points/s by rtk_dev_trace_rays_count; closest points + parity together take x %.2f the time of rtk_dev_signed_distances" % (
        n / med["rtk_dev_trace_rays_count, one ray per point"] * 1e-3,
        (med["rtk_dev_closest_points"] + med["rtk_dev_trace_rays_count, one ray per point"]) / med["rtk_dev_signed_distances"]), flush=True)
    return 0 if api.lib().rtk_dev_trace_status(ds.handle, None) == 0 else 1


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "--step":
        sys.exit(step())
    log = sys.argv[sys.argv.index("--log") + 1] if "--log" in sys.argv else os.path.join(ROOT, "profiles", "signed_timing.log")
    lines = ["# scripts/signed_timing.py, %s" % time.strftime("%Y-%m-%d"), "# clock state before:"] + clock_state()
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
