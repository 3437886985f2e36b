"""Steady-state wall time of rtk_dev_trace_rays_count / rtk_dev_trace_rays_all on the 1M-triangle synthetic scene, device-built,
with the 2^22-ray incoherent batch of scripts/listed_timing.py made on the device (max_t = RTK_INF):
    (a) the count;
    (b) the fill with exact offsets (the count's prefix sum, made once outside the timed call);
    (c) the fill with k = 4 (offsets i * 4, no count);
    (d) as a yardstick, rtk_dev_trace_rays of the same rays (closest hit);
    (e) the only way to the same lists before these calls: the d_after loop of the public API run to completion -- per round one
        rtk_dev_trace_rays_listed with d_after = each ray's previous record, then rtk_dev_select_rays keeps the rays that found
        one; max + 1 rounds, no host wait (the round count is taken from (a), which favours the loop).
Median with [min, max] of 20 calls after 5 warm-up calls for (a) - (d), which alternate inside one loop; of 5 after 2 for (e), which
takes seconds. Wall time around work that ends in a device synchronise. The GPU's clock state is logged before and after. The GPU
step runs in a child process under `timeout`; a failing step ends the run and is logged.
Usage: python scripts/allhits_timing.py [--log profiles/allhits_timing.log]"""
import ctypes as C
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS, WARM = 25, 5
LOOP_REPS, LOOP_WARM = 7, 2


def summary(v, warm):
    v = v[warm:]
    return statistics.median(v), "median %.3f [%.3f, %.3f] ms" % (statistics.median(v), min(v), max(v))


def step():
    import torch
    from rtk_amd import api, synth
    from rtk_amd.types import RTK_INF
    sync = torch.cuda.synchronize
    dev = "cuda"
    ds = api.DeviceScene.build([dict(positions=synth.triangle_soup(1_000_000, 0.02, seed=1))])
    n = 1 << 22
    r = synth.t_rays_incoherent(n, seed=3, device=dev).contiguous()
    r.view(n, 8)[:, 7] = float(RTK_INF)
    rays = r.view(torch.uint8).view(-1)
    L = api.lib()
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

    counts = ds.count_hits_device(rays, n)
    sync()
    mean, most = float(counts.double().mean()), int(counts.max())
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(counts, 0, dtype=torch.int64)
    total = int(offsets[n])
    print("candidates per ray: mean %.2f, max %d; %d records (%.2f GB)" % (mean, most, total, total * 16e-9), flush=True)
    records = torch.empty(max(total, 1) * 16, dtype=torch.uint8, device=dev)
    written = torch.empty(n, dtype=torch.int32, device=dev)
    k4 = torch.arange(n + 1, dtype=torch.int64, device=dev) * 4
    rec4 = torch.empty(n * 4 * 16, dtype=torch.uint8, device=dev)
    hit = torch.empty(n * 16, dtype=torch.uint8, device=dev)
    variants = [
        ("(a) rtk_dev_trace_rays_count", lambda: ds.count_hits_device(rays, n, counts)),
        ("(b) rtk_dev_trace_rays_all, exact offsets", lambda: ds.trace_all_device(rays, n, offsets, records, written)),
        ("(c) rtk_dev_trace_rays_all, k = 4", lambda: ds.trace_all_device(rays, n, k4, rec4, written)),
        ("(d) rtk_dev_trace_rays, closest hit", lambda: ds.trace_device(rays, n, hit)),
    ]
    ts = {name: [] for name, _ in variants}
    for rep in range(REPS):
        for name, fn in variants:
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            ts[name].append((time.perf_counter() - t0) * 1e3)
    med = {}
    for name, _ in variants:
        med[name], text = summary(ts[name], WARM)
        print("n=2^22 %-44s: %s  (%.1f Mrays/s)" % (name, text, n / med[name] * 1e-3), flush=True)

    # (e) the d_after loop: `cur` is each ray's previous record and receives its next one (a lane reads its own slot before it writes it)
    cur = torch.empty(n * 16, dtype=torch.uint8, device=dev)
    miss = torch.zeros(n, 4, dtype=torch.int32, device=dev)
    miss[:, 3] = -1
    f = api.DevFilter()
    f.struct_size = C.sizeof(api.DevFilter)
    f.d_after = cur.data_ptr()
    all_count = torch.tensor([n], dtype=torch.int64, device=dev)

    def loop():
        cur.copy_(miss.view(torch.uint8).view(-1))
        ids, count = None, all_count
        for _ in range(most + 1):
            ds.trace_listed_device(rays, n, count, ids, cur, filter=f)
            ids, count = ds.select_rays(cur, api.SELECT_RECORD_HIT, n, ids, count)
        return count
    tl = []
    for rep in range(LOOP_REPS):
        sync()
        t0 = time.perf_counter()
        left = loop()
        sync()
        tl.append((time.perf_counter() - t0) * 1e3)
    assert int(left) == 0, "the loop did not finish every ray"
    med_loop, text = summary(tl, LOOP_WARM)
    print("n=2^22 %-44s: %s  (%d rounds; %d of %d calls)" % ("(e) d_after loop to completion", text, most + 1, LOOP_REPS - LOOP_WARM, LOOP_REPS), flush=True)
    both = med["(a) rtk_dev_trace_rays_count"] + med["(b) rtk_dev_trace_rays_all, exact offsets"]
    print("count + fill %.3f ms against the loop's %.3f ms: %.1f x; against one closest-hit trace: %.2f x" % (
        both, med_loop, med_loop / both, both / med["(d) rtk_dev_trace_rays, closest hit"]), flush=True)
    i = ds.info()
    print("scene: %d triangles, %d nodes, depth %d, stack entries %d (on chip: %d)" % (
        i["num_triangles"], i["num_nodes"], i["max_depth"], i["stack_entries"], L.rtk_amd_allhits_stack_entries()), flush=True)
    return 0 if L.rtk_dev_trace_status(ds.handle, stream()) == 0 else 1


def clock_state():
    """what the GPU's clocks are doing, read only (the tool is optional)"""
    try:
        p = subprocess.run(["rocm-smi", "--showclocks", "--showperflevel"], capture_output=True, text=True, timeout=60)
        return ["# " + ln for ln in p.stdout.splitlines() if ln.strip() and ("clk" in ln.lower() or "level" in ln.lower())][:40]
    except (OSError, subprocess.SubprocessError) as e:
        return ["# clock state not available: %s" % e]


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "--step":
        sys.exit(step())
    log = sys.argv[sys.argv.index("--log") + 1] if "--log" in sys.argv else os.path.join(ROOT, "profiles", "allhits_timing.log")
    lines = ["# scripts/allhits_timing.py, %s" % time.strftime("%Y-%m-%d"), "# clock state before:"] + clock_state()
    # (the child is the only process that opens the GPU; `timeout` ends it at its limit, 124 / 137 then)
    p = subprocess.run(["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), "--step"], capture_output=True, text=True, cwd=ROOT)
    sys.stdout.write(p.stdout)
    lines += [ln for ln in p.stdout.splitlines() if ln.strip()]
    lines += ["# clock state after:"] + clock_state()
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        lines.append("# step FAILED (exit %d%s)" % (p.returncode, ": time limit" if p.returncode in (124, 137) else ""))
    open(log, "w").write("\n".join(lines) + "\n")
    sys.exit(p.returncode if p.returncode >= 0 else 1)
