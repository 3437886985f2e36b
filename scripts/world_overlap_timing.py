"""Steady-state time of the box overlap query on an instanced world (rtk_dev_world_triangles_in_box_count / _all) beside
rtk_dev_triangles_in_box_count / _all on its flat placed twin, on the 257-instance world of tests/test_gpu_world.py (cubes,
icospheres and a few deep line scenes), 2^20 boxes built around placed vertices as tests/world_overlap_ref.py builds them (half
extents 0.1 to 0.75):
    count, fill   the world's call against the twin's on the same boxes, device events around each of 20 launches after 5
                  warm-up launches, median [min, max]; the fill at the exact offsets of the count; and whether counts and
                  entries (the twin's prims mapped through mesh_base) are the same on every query;
    visits        nodes, leaves and triangles per query from both counted forms;
    cost          the world's create and update time against the twin's build time, and both device-memory totals (the world's
                  own plus its three scenes, against the twin).
One child process under `timeout`; a failing step is logged. No threshold is set on any figure: the log is the record.
Usage: python scripts/world_overlap_timing.py [--log profiles/world_overlap_timing.log]"""
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scripts.closest_timing import clock_state  # noqa: E402

N = 1 << 20
WARM, REPS = 5, 20


def boxes_around_vertices(placed, rng, n, size):
    """[n, 6] float32: instances drawn evenly, a vertex of theirs inside each box"""
    which = rng.randint(0, len(placed), n)
    v = np.zeros((n, 3))
    for k, p in enumerate(placed):
        rows = np.flatnonzero(which == k)
        v[rows] = p.reshape(-1, 3)[rng.randint(0, p.shape[0] * 3, len(rows))]
    s = size * rng.uniform(0.5, 1.5, (n, 1))
    return np.concatenate([v - s * rng.uniform(0.2, 1.0, (n, 3)), v + s * rng.uniform(0.2, 1.0, (n, 3))], 1).astype(np.float32)


def timed(fns, torch):
    """fns: [(name, fn)], one launch of each per round, in turn, between two events -> {name: text}, {name: median ms}"""
    ts = {name: [] for name, _ in fns}
    for rep in range(WARM + REPS):
        for name, fn in fns:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[name].append(a.elapsed_time(b))
    text, med = {}, {}
    for name, v in ts.items():
        v = v[WARM:]
        med[name] = statistics.median(v)
        text[name] = "median %.3f [%.3f, %.3f] ms" % (med[name], min(v), max(v))
    return text, med


def step():
    import torch
    from rtk_amd import api
    from tests.test_gpu_world import TRIS, case
    from tests.world_closest_ref import live_instances, placed_tris
    which, places = case("257")
    live = np.flatnonzero(live_instances(TRIS, which, places))
    assert len(live) == len(which)
    meshes = [dict(positions=t.reshape(-1, 3)) for t in TRIS]
    scenes = [api.DeviceScene.build([m]) for m in meshes]
    world = api.DeviceWorld.create(scenes, which, places)
    twin = api.DeviceScene.build([meshes[k] for k in which], placements=places)
    t0 = time.perf_counter()
    world.update(places)
    update_ms = (time.perf_counter() - t0) * 1e3
    wi, ti = world.info(), twin.info()
    scene_bytes = sum(s.info()["total_device_bytes"] for s in scenes)
    print("257 instances, %d triangles placed: world create %.3f ms, update (all placements) %.3f ms wall; flat twin build %.3f ms" % (
        ti["num_triangles"], wi["build_ms"], update_ms, ti["build_ms"]), flush=True)
    print("257 instances: device memory: world %d B + its 3 scenes %d B = %d B; flat twin %d B (%.1f x)" % (
        wi["total_device_bytes"], scene_bytes, wi["total_device_bytes"] + scene_bytes, ti["total_device_bytes"],
        ti["total_device_bytes"] / (wi["total_device_bytes"] + scene_bytes)), flush=True)
    rng = np.random.RandomState(5)
    q = boxes_around_vertices([placed_tris(TRIS[which[k]], places[k]).astype(np.float64) for k in range(len(which))], rng, N, 0.5)
    d_q = api.to_device(q)
    cw = torch.empty(N, dtype=torch.int32, device="cuda")
    ct = torch.empty(N, dtype=torch.int32, device="cuda")
    world.triangles_in_box_count_device(d_q, N, cw)
    twin.count_in_boxes_device(d_q, N, ct)
    torch.cuda.synchronize()
    same_counts = int((cw == ct).sum().item())
    off = torch.zeros(N + 1, dtype=torch.int64, device="cuda")
    off[1:] = torch.cumsum(cw, 0, dtype=torch.int64)
    total = int(off[N].item())
    ew = torch.zeros(max(total, 1), dtype=torch.int64, device="cuda")
    et = torch.zeros(max(total, 1), dtype=torch.int32, device="cuda")
    text, med = timed([("world count", lambda: world.triangles_in_box_count_device(d_q, N, cw)),
                       ("twin  count", lambda: twin.count_in_boxes_device(d_q, N, ct)),
                       ("world fill", lambda: world.triangles_in_box_all_device(d_q, N, off, ew)),
                       ("twin  fill", lambda: twin.in_boxes_all_device(d_q, N, off, et))], torch)
    for k in text:
        print("257 instances, 2^20 boxes, %.1f candidates per box: %-11s: %s  (%.1f M boxes/s)" % (total / N, k, text[k], N / med[k] * 1e-3), flush=True)
    world.status()
    # the same entries: the twin's prims through mesh_base
    base = torch.from_numpy(np.asarray(twin.mesh_base(), np.int64)[:len(which)].copy()).cuda()
    prims = et[:total].to(torch.int64) & 0xFFFFFFFF
    mesh = torch.searchsorted(base, prims, right=True) - 1
    same_entries = int((((mesh << 32) | (prims - base[mesh])) == ew[:total]).sum().item()) if same_counts == N else -1
    print("257 instances: counts the same as the flat twin's on %d of %d boxes; entries on %d of %d" % (same_counts, N, same_entries, total), flush=True)
    print("257 instances: the world takes %.2f x the flat twin's time for the count and %.2f x for the fill; not tuned" % (
        med["world count"] / med["twin  count"], med["world fill"] / med["twin  fill"]), flush=True)
    _, vw = world.triangles_in_box_counted(d_q, N)
    _, vt = twin.triangles_in_boxes_counted(d_q, N)
    for name, c in (("world", vw), ("flat twin", vt)):
        print("257 instances: visits per box, %-9s: %.1f nodes, %.1f leaves, %.1f triangles%s; stack spills %d" % (
            name, c["nodes"] / N, c["leaves"] / N, c["triangles"] / N, " (proxies included)" if name == "world" else "", c["stack_spills"]), flush=True)
    world.status()
    return 0


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "--step":
        sys.exit(step())
    log = sys.argv[sys.argv.index("--log") + 1] if "--log" in sys.argv else os.path.join(ROOT, "profiles", "world_overlap_timing.log")
    lines = ["# scripts/world_overlap_timing.py, %s" % time.strftime("%Y-%m-%d"),
             "# the 8-byte stack of the world frame as it stands; a 4-byte stack was not tried", "# clock state before:"] + clock_state()
    # (the child is the only process that opens the GPU while it runs; `timeout` ends it at its limit, 124 / 137 then)
    p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--step"], capture_output=True, text=True, cwd=ROOT)
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
