"""Steady-state wall time of closest points on an instanced world (rtk_dev_world_closest_points) beside rtk_dev_closest_points on
its flat placed twin, on scripts/world_timing.py's world: 4096 instances of the 16 384-triangle height field placed by random
rotations over a cube. 2^20 queries, half uniform in the cube, half within one mesh size of an instance's position:
    closest   rtk_dev_world_closest_points against the twin's rtk_dev_closest_points on the same queries, and the share of
              queries whose records are the same bits (all of them, by the rule);
    rays      rtk_dev_world_trace_rays on 2^20 incoherent rays in the same process, for scale;
    visits    nodes, leaves and triangles per query from both counted forms.
Median of the calls after the warm-up calls with [min, max] (scripts/closest_timing.py: timed_together: 20 timed calls after 5);
wall time around work that ends in a device synchronise. One child process under `timeout`; a failing step is logged. No
threshold is set on any figure: the log is the record.
Usage: python scripts/world_closest_timing.py [--log profiles/world_closest_timing.log]"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scripts.closest_timing import clock_state, timed_together  # noqa: E402
from scripts.world_timing import height_field, placements  # noqa: E402

N = 1 << 20


def step(n_inst):
    import torch
    from rtk_amd import api, synth
    from rtk_amd.types import POINT_QUERY_DTYPE, RTK_INF
    sync = torch.cuda.synchronize
    tris = height_field()
    spread = 2.0 * n_inst ** (1.0 / 3.0)
    P0 = placements(n_inst, 1, spread)
    which = np.zeros(n_inst, np.uint32)
    mesh = dict(positions=torch.from_numpy(tris.reshape(-1, 3)).cuda())
    scene = api.DeviceScene.build([mesh])
    world = api.DeviceWorld.create([scene], which, P0)
    twin = api.DeviceScene.build([mesh] * n_inst, placements=P0)
    rng = np.random.RandomState(3)
    q = np.zeros(N, POINT_QUERY_DTYPE)
    q["point"][:N // 2] = rng.uniform(-spread, spread, (N // 2, 3))
    q["point"][N // 2:] = P0.reshape(n_inst, 3, 4)[rng.randint(0, n_inst, N - N // 2), :, 3] + rng.uniform(-1, 1, (N - N // 2, 3))
    q["max_dist2"] = RTK_INF
    d_q = api.to_device(q)
    rec = torch.empty(N * 16, dtype=torch.uint8, device="cuda")
    rec2 = torch.empty(N * 16, dtype=torch.uint8, device="cuda")
    inst = torch.empty(N, dtype=torch.int32, device="cuda")
    pts = torch.empty(N * 12, dtype=torch.uint8, device="cuda")
    pts2 = torch.empty(N * 12, dtype=torch.uint8, device="cuda")
    rays = synth.rays_incoherent(N)
    rays["origin"] *= spread / max(1e-9, np.abs(rays["origin"]).max())
    d_rays = api.to_device(rays)
    hrec = torch.empty(N * 16, dtype=torch.uint8, device="cuda")
    text, med = timed_together([("rtk_dev_world_closest_points", lambda: world.closest_points_device(d_q, N, rec, inst, pts)),
                                ("rtk_dev_closest_points, flat twin", lambda: twin.closest_points_device(d_q, N, rec2, pts2)),
                                ("rtk_dev_world_trace_rays", lambda: world.trace_device(d_rays, N, hrec, inst))], sync)
    for k in text:
        print("%4d instances, 2^20 %s: %-34s: %s  (%.1f M/s)" % (n_inst, "rays" if "trace" in k else "queries", k, text[k], N / med[k] * 1e-3), flush=True)
    a, b = rec.cpu().numpy().view(np.uint32).reshape(N, 4), rec2.cpu().numpy().view(np.uint32).reshape(N, 4)
    print("%4d instances: dist2, u, v the same bits as the flat twin's on %d of %d queries; points on %d" % (
        n_inst, (a[:, :3] == b[:, :3]).all(1).sum(), N, (pts.cpu().numpy().view(np.uint32).reshape(N, 3) == pts2.cpu().numpy().view(np.uint32).reshape(N, 3)).all(1).sum()), flush=True)
    ratio = med["rtk_dev_world_closest_points"] / med["rtk_dev_closest_points, flat twin"]
    print("%4d instances: the world takes %.2f x the flat twin's time for closest points, %.2f x its own time for rays; not tuned" % (
        n_inst, ratio, med["rtk_dev_world_closest_points"] / med["rtk_dev_world_trace_rays"]), flush=True)
    _, _, _, cw = world.closest_points_counted(d_q, N)
    _, _, ct = twin.closest_points_counted(d_q, N)
    for name, c in (("world", cw), ("flat twin", ct)):
        print("%4d instances: visits per query, %-9s: %.1f nodes, %.1f leaves, %.1f triangles%s; stack spills %d" % (
            n_inst, name, c["nodes"] / N, c["leaves"] / N, c["triangles"] / N, " (proxies included)" if name == "world" else "", c["stack_spills"]), flush=True)
    world.status()
    return 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "--step":
        sys.exit(step(int(sys.argv[2])))
    log = sys.argv[sys.argv.index("--log") + 1] if "--log" in sys.argv else os.path.join(ROOT, "profiles", "world_closest_timing.log")
    lines = ["# scripts/world_closest_timing.py, %s" % time.strftime("%Y-%m-%d"), "# clock state before:"] + clock_state()
    # (the child is the only process that opens the GPU while it runs; `timeout` ends it at its limit, 124 / 137 then)
    p = subprocess.run(["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), "--step", "4096"], capture_output=True, text=True, cwd=ROOT)
    sys.stdout.write(p.stdout)
    lines += [ln for ln in p.stdout.splitlines() if ln.strip()]
    rc = 0
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        lines.append("# step FAILED (exit %d%s)" % (p.returncode, ": time limit" if p.returncode in (124, 137) else ""))
        rc = p.returncode if p.returncode > 0 else 1
    lines += ["# clock state after:"] + clock_state()
    open(log, "w").write("\n".join(lines) + "\n")
    sys.exit(rc)
