"""Steady-state wall time of rtk_dev_winding_numbers on the 1M-triangle synthetic scene (the benchmark scene's size), device-built,
queries made on the device -- surface points pushed out by 1e-3 of the scene's extent in a random direction:
    table     the making of the table of winding moments (rtk_dev_scene_prepare_winding after a refit has dropped it: table_ms
              of rtk_dev_winding_info);
    fast      rtk_dev_winding_numbers at beta 2 against rtk_dev_closest_points on the same 2^20 points in the same loop, and
              the visit counts of one counted call;
    exact     RTK_WINDING_EXACT on the first 4096 of those points: every triangle summed for every query.
Median of the calls after the warm-up calls with [min, max] (scripts/closest_timing.py: timed_together); wall time around work
that ends in a device synchronise. The scene is a triangle soup: the timing does not care, the numbers of course mean nothing
there. Each GPU step runs in a child process of its own under `timeout`, one after the other; a failing step ends the run and
is logged. No threshold is set on any figure: the log is the record.
Usage: python scripts/winding_timing.py [--log profiles/winding_timing.log]"""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scripts.closest_timing import clock_state, timed_together  # noqa: E402

N_FAST, N_EXACT = 1 << 20, 4096


def scene_and_queries(n):
    import torch
    from rtk_amd import api, synth
    from rtk_amd.types import RTK_INF
    dev = "cuda"
    d_pos = torch.from_numpy(synth.triangle_soup(1_000_000, 0.02, seed=1)).to(dev)
    ds = api.DeviceScene.build([dict(positions=d_pos)])
    tris = d_pos.view(-1, 3, 3)
    lo, hi = tris.view(-1, 3).min(0).values, tris.view(-1, 3).max(0).values
    extent = float((hi - lo).max())
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    pick = torch.randint(0, tris.shape[0], (n,), device=dev, generator=g)
    w = torch.rand(n, 2, device=dev, generator=g)
    flip = w.sum(1) > 1.0
    w[flip] = 1.0 - w[flip]
    t = tris[pick]
    on = t[:, 0] + (t[:, 1] - t[:, 0]) * w[:, :1] + (t[:, 2] - t[:, 0]) * w[:, 1:]
    d = torch.randn(n, 3, device=dev, generator=g)
    q = torch.empty(n, 4, dtype=torch.float32, device=dev)
    q[:, :3] = on + d / d.norm(dim=1, keepdim=True) * (1e-3 * extent)
    q[:, 3] = float(RTK_INF)
    return api, ds, d_pos, q.view(torch.uint8).view(-1)


def step_fast():
    import torch
    sync = torch.cuda.synchronize
    n = N_FAST
    api, ds, d_pos, q = scene_and_queries(n)
    # the table: made, dropped by a refit to the same positions, made again -- five times
    ms = []
    for _ in range(6):
        ms.append(ds.prepare_winding()["table_ms"])
        ds.refit([dict(positions=d_pos)])
    ms = ms[1:]
    info = ds.prepare_winding()
    print("table: table_ms median %.3f [%.3f, %.3f] ms for %d triangles, %d nodes, %d bytes" % (
        statistics.median(ms), min(ms), max(ms), ds.info()["num_triangles"], info["nodes"], info["table_bytes"]), flush=True)
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    rec = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
    pts = torch.empty(n * 12, dtype=torch.uint8, device="cuda")
    text, med = timed_together([
        ("rtk_dev_winding_numbers, beta 2", lambda: ds.winding_numbers_device(q, n, out)),
        ("rtk_dev_closest_points", lambda: ds.closest_points_device(q, n, rec, pts)),
    ], sync)
    for k in text:
        print("n=2^20 %-34s: %s  (%.2f M queries/s)" % (k, text[k], n / med[k] * 1e-3), flush=True)
    _, counts = ds.winding_numbers_counted(q, n)
    print("beta 2, per query: %.1f table records, %.1f leaves, %.1f triangle terms, %.1f far terms, %.2f pushes past the on-chip stack" % (
        counts["nodes"] / n, counts["leaves"] / n, counts["triangles"] / n, counts["hits"] / n, counts["stack_spills"] / n), flush=True)
    return 0 if api.lib().rtk_dev_trace_status(ds.handle, None) == 0 else 1


def step_exact():
    import torch
    sync = torch.cuda.synchronize
    n = N_EXACT
    api, ds, d_pos, q = scene_and_queries(N_FAST)                            # (the same points: the first 4096 of them)
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    text, med = timed_together([("rtk_dev_winding_numbers, RTK_WINDING_EXACT", lambda: ds.winding_numbers_device(q, n, out, exact=True))], sync)
    for k in text:
        print("n=4096 %-34s: %s  (%.4f M queries/s, %.1f G triangle terms/s)" % (k, text[k], n / med[k] * 1e-3, n * ds.info()["num_triangles"] / med[k] * 1e-6), flush=True)
    return 0 if api.lib().rtk_dev_trace_status(ds.handle, None) == 0 else 1


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "--step":
        sys.exit({"fast": step_fast, "exact": step_exact}[sys.argv[2]]())
    log = sys.argv[sys.argv.index("--log") + 1] if "--log" in sys.argv else os.path.join(ROOT, "profiles", "winding_timing.log")
    lines = ["# scripts/winding_timing.py, %s" % time.strftime("%Y-%m-%d"), "# clock state before:"] + clock_state()
    rc = 0
    # (each child is the only process that opens the GPU while it runs; `timeout` ends it at its limit, 124 / 137 then; the
    # second step starts only after the first has ended well)
    for name, limit in (("fast", "300"), ("exact", "300")):
        p = subprocess.run(["timeout", "-k", "10", limit, sys.executable, os.path.abspath(__file__), "--step", name], capture_output=True, text=True, cwd=ROOT)
        sys.stdout.write(p.stdout)
        lines += [ln for ln in p.stdout.splitlines() if ln.strip()]
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-4000:])
            lines.append("# step %s FAILED (exit %d%s)" % (name, p.returncode, ": time limit" if p.returncode in (124, 137) else ""))
            rc = p.returncode if p.returncode > 0 else 1
            break
    lines += ["# clock state after:"] + clock_state()
    open(log, "w").write("\n".join(lines) + "\n")
    sys.exit(rc)
