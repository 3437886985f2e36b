"""Steady-state wall time of the placed calls beside their unplaced siblings in the same process: device-resident float32
positions, implicit indices, the config-2 scene (1 M triangles) and the config-5 scene (10 M) cut into 64 slab meshes along x,
every mesh with a rigid placement of its own. Per size:
    refit_placed(rest, placements)                 beside  refit(pre-placed positions)
    refit_meshes_placed, 1/64 and 16/64 listed     beside  refit_meshes
    build_placed                                   beside  build
    what a host does today: a torch matmul that writes the placed copy, then the plain call (full refit, and 1/64)
Median of 20 calls after 5 warm-up calls with [min, max], wall time around the synchronous call. --plain-tree DIR: the plain
calls alone, timed once more with the rtk_amd package and library of another checkout (the parent commit's, built) in the same
session, to show that they have not moved. Every GPU step runs in a child process under `timeout` with a limit of its own; the first failing step ends
the run and is logged.
Usage: python scripts/placed_timing.py [--log profiles/placed_timing.log] [--plain-tree DIR]"""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.environ.get("PLACED_TIMING_TREE") or ROOT       # (where a step imports rtk_amd from)
sys.path.insert(0, TREE)
MESHES = 64


def timed(fn, sync, reps=25):
    ts = []
    for rep in range(reps):
        sync()
        t0 = time.perf_counter()
        fn(rep)
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts = ts[5:]
    return "median %.3f [%.3f, %.3f] ms" % (statistics.median(ts), min(ts), max(ts))


def step(n, plain_only):
    import numpy as np
    import torch
    from rtk_amd import api, synth
    sync = torch.cuda.synchronize
    tris = synth.triangle_soup(n, 0.02 if n <= 1_000_000 else 0.01, seed=1)
    d = torch.from_numpy(tris).cuda().reshape(-1, 3, 3)
    d = d[torch.argsort(d[:, :, 0].mean(1), stable=True)].reshape(-1, 3).contiguous()
    assert n % MESHES == 0
    per = 3 * n // MESHES
    rest = d.reshape(MESHES, per, 3)

    def placements(phase):
        """a small rotation about z and a small shift per mesh, float32 [64, 3, 4]"""
        a = 0.02 * np.sin(phase + np.arange(MESHES))
        m = np.zeros((MESHES, 3, 4), np.float32)
        m[:, 0, 0], m[:, 0, 1], m[:, 1, 0], m[:, 1, 1], m[:, 2, 2] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a), 1.0
        m[:, :, 3] = 0.01 * np.cos(phase + np.arange(MESHES))[:, None]
        return m
    P = [placements(0.0), placements(1.0)]
    dP = [torch.from_numpy(p).cuda() for p in P]

    def matmul(k, out, ids=None):
        """the placed copy a host writes today (not bit-identical to the rule: one fused kernel of torch's choosing)"""
        if ids is None:
            torch.baddbmm(dP[k][:, None, :, 3], rest, dP[k][:, :, :3].transpose(1, 2), out=out)
        else:
            for m in ids:
                torch.addmm(dP[k][m, :, 3], rest[m], dP[k][m, :, :3].t(), out=out[m])
    world = [torch.empty_like(rest), torch.empty_like(rest)]
    for k in (0, 1):
        matmul(k, world[k])
    sync()
    rest_meshes = [dict(positions=rest[m]) for m in range(MESHES)]
    world_meshes = [[dict(positions=world[k][m]) for m in range(MESHES)] for k in (0, 1)]
    tag = "n=%d%s" % (n, " [the other checkout]" if plain_only else "")
    assert os.path.dirname(os.path.dirname(os.path.abspath(api.__file__))) == os.path.abspath(TREE)

    ds = api.DeviceScene.build(world_meshes[0])
    ds.refit(world_meshes[1])                                          # (the scene's first refit: the schedule)
    ds.refit([world_meshes[1][m] if m == 0 else None for m in range(MESHES)], only=[0])      # (and the per-mesh tables)
    print("%s: nodes %d" % (tag, ds.info()["num_nodes"]), flush=True)
    print("%s refit                    : %s" % (tag, timed(lambda r: ds.refit(world_meshes[r & 1]), sync)), flush=True)
    if not plain_only:
        print("%s refit_placed             : %s" % (tag, timed(lambda r: ds.refit(rest_meshes, placements=P[r & 1]), sync)), flush=True)

        def today_full(r):
            matmul(r & 1, world[r & 1])
            ds.refit(world_meshes[r & 1])
        print("%s torch matmul + refit     : %s" % (tag, timed(today_full, sync)), flush=True)
    for k in (1, 16):
        ids = list(range(0, MESHES, MESHES // k))
        some_world = [[world_meshes[j][m] if m in ids else None for m in range(MESHES)] for j in (0, 1)]
        some_rest = [rest_meshes[m] if m in ids else None for m in range(MESHES)]
        print("%s refit_meshes %2d/64       : %s" % (tag, k, timed(lambda r: ds.refit(some_world[r & 1], only=ids), sync)), flush=True)
        if plain_only:
            continue
        print("%s refit_meshes_placed %2d/64: %s" % (tag, k, timed(lambda r: ds.refit(some_rest, only=ids, placements=P[r & 1]), sync)), flush=True)

        def today_some(r):
            matmul(r & 1, world[r & 1], ids)
            ds.refit(some_world[r & 1], only=ids)
        print("%s torch matmul + refit_meshes %2d/64: %s" % (tag, k, timed(today_some, sync)), flush=True)
    keep = []

    def build(r, placed):
        keep[:] = [api.DeviceScene.build(rest_meshes, placements=P[0]) if placed else api.DeviceScene.build(world_meshes[0])]
    for k in (0, 1):
        matmul(k, world[k])
    sync()
    print("%s build                    : %s" % (tag, timed(lambda r: build(r, False), sync)), flush=True)
    if plain_only:
        return 0
    print("%s build_placed             : %s" % (tag, timed(lambda r: build(r, True), sync)), flush=True)
    return 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "--step":
        sys.exit(step(int(sys.argv[2]), "--plain-only" in sys.argv))
    log = sys.argv[sys.argv.index("--log") + 1] if "--log" in sys.argv else os.path.join(ROOT, "profiles", "placed_timing.log")
    plain_tree = sys.argv[sys.argv.index("--plain-tree") + 1] if "--plain-tree" in sys.argv else None
    lines = ["# scripts/placed_timing.py, %s" % time.strftime("%Y-%m-%d")]
    steps = [(n, limit, None) for n, limit in ((1_000_000, 240), (10_000_000, 420))]
    if plain_tree:
        steps += [(n, limit, os.path.abspath(plain_tree)) for n, limit, _ in steps]
    for n, limit, tree in steps:
        # (the child is the only process that opens the GPU; `timeout` ends it at its limit, 124 / 137 then)
        env = dict(os.environ)
        if tree:
            env["PLACED_TIMING_TREE"] = tree
        p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", str(n)] + (["--plain-only"] if tree else []),
                           capture_output=True, text=True, cwd=ROOT, env=env)
        sys.stdout.write(p.stdout)
        lines += [ln for ln in p.stdout.splitlines() if ln.strip()]
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-4000:])
            lines.append("# step %d FAILED (exit %d%s)" % (n, p.returncode, ": time limit of %d s" % limit if p.returncode in (124, 137) else ""))
            open(log, "w").write("\n".join(lines) + "\n")
            sys.exit(p.returncode if p.returncode > 0 else 1)
    open(log, "w").write("\n".join(lines) + "\n")
