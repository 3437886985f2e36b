"""Steady-state wall time of an instanced world (rtk_dev_world) beside its flat placed twin (rtk_dev_scene_build_placed of the
same instances) in the same process, for 64 and 4096 instances of one 16 384-triangle mesh (a 128 x 64 height field, 2 triangles
per cell) placed by random rotations over a cube:
    create    rtk_dev_world_create (the mesh's scene exists already) against rtk_dev_scene_build_placed;
    update    rtk_dev_world_update with new placements against rtk_dev_scene_refit_placed with the same;
    trace     rtk_dev_world_trace_rays against the twin's rtk_dev_trace_rays on the same 2^20 incoherent rays;
    bytes     rtk_dev_world_info.total_device_bytes plus the one scene's, against the twin's total_device_bytes.
Median of the calls after the warm-up calls with [min, max] (scripts/closest_timing.py: timed_together: 20 timed calls after 5);
wall time around work that ends in a device synchronise. Each instance count runs in a child process of its own under `timeout`,
one after the other; a failing step ends the run and is logged. No threshold is set on any figure: the log is the record.
Usage: python scripts/world_timing.py [--log profiles/world_timing.log]"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scripts.closest_timing import clock_state, timed_together  # noqa: E402

N_RAYS = 1 << 20


def height_field(nx=128, ny=64):
    """nx * ny * 2 = 16 384 triangles over [-1, 1] x [-0.5, 0.5], heights of a few sines"""
    x, y = np.meshgrid(np.linspace(-1, 1, nx + 1), np.linspace(-0.5, 0.5, ny + 1), indexing="ij")
    z = 0.1 * np.sin(7 * x) * np.cos(9 * y) + 0.05 * np.sin(23 * x + 11 * y)
    p = np.stack([x, y, z], -1)
    a, b, c, d = p[:-1, :-1], p[1:, :-1], p[1:, 1:], p[:-1, 1:]
    return np.concatenate([np.stack([a, b, c], 2).reshape(-1, 3, 3), np.stack([a, c, d], 2).reshape(-1, 3, 3)]).astype(np.float32)


def placements(n, seed, spread):
    rng = np.random.RandomState(seed)
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).reshape(n, 3, 3)
    m = np.zeros((n, 3, 4), np.float32)
    m[:, :, :3] = R
    m[:, :, 3] = rng.uniform(-spread, spread, (n, 3))
    return m.reshape(n, 12)


def step(n_inst):
    import torch
    from rtk_amd import api, synth
    sync = torch.cuda.synchronize
    tris = height_field()
    spread = 2.0 * n_inst ** (1.0 / 3.0)
    P0, P1 = placements(n_inst, 1, spread), placements(n_inst, 2, spread)
    which = np.zeros(n_inst, np.uint32)
    mesh = dict(positions=torch.from_numpy(tris.reshape(-1, 3)).cuda())
    scene = api.DeviceScene.build([mesh])
    rays = synth.rays_incoherent(N_RAYS)
    rays["origin"] *= spread / max(1e-9, np.abs(rays["origin"]).max())
    d_rays = api.to_device(rays)
    made = {}

    def create_world():
        made["world"] = api.DeviceWorld.create([scene], which, P0)

    def build_twin():
        made["twin"] = api.DeviceScene.build([mesh] * n_inst, placements=P0)
    text, med = timed_together([("rtk_dev_world_create", create_world), ("rtk_dev_scene_build_placed", build_twin)], sync)
    for k in text:
        print("%4d instances x %d triangles: %-28s: %s" % (n_inst, len(tris), k, text[k]), flush=True)
    world, twin = made["world"], made["twin"]
    flip = [0]

    def update_world():
        flip[0] ^= 1
        world.update(P1 if flip[0] else P0)

    def refit_twin():
        twin.refit([mesh] * n_inst, placements=P1 if flip[0] else P0)
    text, med = timed_together([("rtk_dev_world_update", update_world), ("rtk_dev_scene_refit_placed", refit_twin)], sync)
    for k in text:
        print("%4d instances x %d triangles: %-28s: %s" % (n_inst, len(tris), k, text[k]), flush=True)
    world.update(P0)
    twin.refit([mesh] * n_inst, placements=P0)
    rec = torch.empty(N_RAYS * 16, dtype=torch.uint8, device="cuda")
    rec2 = torch.empty(N_RAYS * 16, dtype=torch.uint8, device="cuda")
    inst = torch.empty(N_RAYS, dtype=torch.int32, device="cuda")
    text, med = timed_together([("rtk_dev_world_trace_rays", lambda: world.trace_device(d_rays, N_RAYS, rec, inst)),
                                ("rtk_dev_trace_rays, flat twin", lambda: twin.trace_device(d_rays, N_RAYS, rec2))], sync)
    for k in text:
        print("%4d instances, 2^20 incoherent rays: %-28s: %s  (%.1f Mrays/s)" % (n_inst, k, text[k], N_RAYS / med[k] * 1e-3), flush=True)
    a, b = rec.cpu().numpy().view(api.HIT_RECORD_DTYPE), rec2.cpu().numpy().view(api.HIT_RECORD_DTYPE)
    print("%4d instances: rays that hit: world %d, twin %d; same hit / miss on %d of %d" % (
        n_inst, (a["prim"] != 0xFFFFFFFF).sum(), (b["prim"] != 0xFFFFFFFF).sum(), ((a["prim"] != 0xFFFFFFFF) == (b["prim"] != 0xFFFFFFFF)).sum(), N_RAYS), flush=True)
    wi, si, ti = world.info(), scene.info(), twin.info()
    print("%4d instances: device bytes: world %d + its one scene %d = %d; flat twin %d (%.1f x); top tree %d nodes, depth %d, stack entries %d" % (
        n_inst, wi["total_device_bytes"], si["total_device_bytes"], wi["total_device_bytes"] + si["total_device_bytes"], ti["total_device_bytes"],
        ti["total_device_bytes"] / (wi["total_device_bytes"] + si["total_device_bytes"]), wi["top_nodes"], wi["top_max_depth"], wi["stack_entries"]), flush=True)
    world.status()
    return 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "--step":
        sys.exit(step(int(sys.argv[2])))
    log = sys.argv[sys.argv.index("--log") + 1] if "--log" in sys.argv else os.path.join(ROOT, "profiles", "world_timing.log")
    lines = ["# scripts/world_timing.py, %s" % time.strftime("%Y-%m-%d"), "# clock state before:"] + clock_state()
    rc = 0
    # (each child is the only process that opens the GPU while it runs; `timeout` ends it at its limit, 124 / 137 then; the
    # second step starts only after the first has ended well)
    for name, limit in (("64", "240"), ("4096", "420")):
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
