"""Steady-state wall time of the ray-list calls (rtk_dev_trace_rays_listed, rtk_dev_trace_rays_any_listed, rtk_dev_select_rays) on
the 1M-triangle synthetic scene, device-built, rays made on the device:
    (a) rtk_dev_trace_rays of the 2^24-ray incoherent batch beside rtk_dev_trace_rays_listed of the same batch with the identity
        list and with d_ids == NULL (the plain call also with RTK_TRACE_NO_DETECT: at this size it otherwise looks for an image,
        two small launches and a wait that the listed calls never make);
    (b) a three-bounce loop over 2^22 rays -- closest hit of the live rays, select the hits, any-hit of shadow rays in the hit
        slots, select the unoccluded, which are the next bounce's live rays -- done with lists (nothing waits, one synchronise at
        the end) and the way it has to be done without them: wait, torch.nonzero, gather the rays into a compact array, trace,
        scatter the answers back;
    (c) rtk_dev_select_rays alone on 2^24 hit records, and the bytes per second that implies (16 B read per record, 8 B written
        per kept id).
Median of 20 calls after 5 warm-up calls with [min, max]; wall time around work that ends in a device synchronise; the variants
of one measurement alternate inside one loop. The GPU's clock state is logged before and after. Every GPU step runs in a child
process under `timeout`; the first failing step ends the run and is logged.
Usage: python scripts/listed_timing.py [--log profiles/listed_timing.log]"""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS, WARM = 25, 5


def timed_together(variants, sync):
    """variants: [(name, fn)]; one call of each per round, in turn -> {name: 'median .. [min, max] ms'}, {name: median}"""
    ts = {name: [] for name, _ in variants}
    for rep in range(REPS):
        for name, fn in variants:
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            ts[name].append((time.perf_counter() - t0) * 1e3)
    text, med = {}, {}
    for name, v in ts.items():
        v = v[WARM:]
        med[name] = statistics.median(v)
        text[name] = "median %.3f [%.3f, %.3f] ms" % (med[name], min(v), max(v))
    return text, med


def step():
    import torch
    from rtk_amd import api, synth
    sync = torch.cuda.synchronize
    ds = api.DeviceScene.build([dict(positions=synth.triangle_soup(1_000_000, 0.02, seed=1))])
    dev = "cuda"

    def u8(t):
        return t.contiguous().view(torch.uint8).view(-1)

    # ---- (a)
    n = 1 << 24
    rays = u8(synth.t_rays_incoherent(n, seed=3, device=dev))
    rec = torch.empty(n * 16, dtype=torch.uint8, device=dev)
    ident = torch.arange(n, dtype=torch.int64, device=dev)
    count = torch.tensor([n], dtype=torch.int64, device=dev)
    no_detect = api.make_opts(no_detect=True)
    text, med = timed_together([
        ("rtk_dev_trace_rays", lambda: ds.trace_device(rays, n, rec)),
        ("rtk_dev_trace_rays NO_DETECT", lambda: ds.trace_device(rays, n, rec, opts=no_detect)),
        ("listed, identity ids", lambda: ds.trace_listed_device(rays, n, count, ident, rec)),
        ("listed, d_ids NULL", lambda: ds.trace_listed_device(rays, n, count, None, rec)),
    ], sync)
    for k in text:
        print("(a) n=2^24 %-30s: %s  (%.2f Grays/s)" % (k, text[k], n / med[k] * 1e-6), flush=True)
    base = med["rtk_dev_trace_rays NO_DETECT"]
    print("(a) listed over plain (NO_DETECT): identity ids %+.2f %%, d_ids NULL %+.2f %%" % (
        100.0 * (med["listed, identity ids"] / base - 1.0), 100.0 * (med["listed, d_ids NULL"] / base - 1.0)), flush=True)

    # ---- (c)
    ds.trace_device(rays, n, rec)
    sync()
    kept = int((rec.view(torch.int32).view(n, 4)[:, 3] != -1).sum().item())
    text, med = timed_together([("select", lambda: ds.select_rays(rec, api.SELECT_RECORD_HIT, n))], sync)
    moved = n * 16 + kept * 8
    print("(c) n=2^24 rtk_dev_select_rays RECORD_HIT, %d kept: %s  (%.0f GB/s of %d bytes read and written)" % (
        kept, text["select"], moved / med["select"] * 1e-6, moved), flush=True)
    del rays, rec, ident

    # ---- (b)
    n = 1 << 22
    live = u8(synth.t_rays_incoherent(n, seed=4, device=dev))
    shadow = u8(synth.t_rays_shadow(n, seed=5, device=dev))
    rec = torch.empty(n * 16, dtype=torch.uint8, device=dev)
    occ = torch.empty(n, dtype=torch.uint8, device=dev)
    all_count = torch.tensor([n], dtype=torch.int64, device=dev)
    result = {}

    def with_lists():
        ids, cnt = None, all_count
        for _ in range(3):
            ds.trace_listed_device(live, n, cnt, ids, rec)
            hit_ids, hit_cnt = ds.select_rays(rec, api.SELECT_RECORD_HIT, n, in_ids=ids, in_count=cnt if ids is not None else None) if ids is not None \
                else ds.select_rays(rec, api.SELECT_RECORD_HIT, n)
            ds.trace_any_listed_device(shadow, n, hit_cnt, hit_ids, occ)
            ids, cnt = ds.select_rays(occ, api.SELECT_BYTE_ZERO, n, in_ids=hit_ids, in_count=hit_cnt)
        result["lists"] = (ids, cnt)

    live32, shadow32 = live.view(n, 32), shadow.view(n, 32)

    def today():
        idx = torch.arange(n, dtype=torch.int64, device=dev)
        for _ in range(3):
            m = idx.numel()
            if m == 0:
                break
            c_rec = ds.trace_device(live32[idx].view(-1), m)                       # gather, trace the compact array
            hit = c_rec.view(torch.int32).view(m, 4)[:, 3] != -1
            hit_idx = idx[torch.nonzero(hit)[:, 0]]                                # (torch.nonzero waits for the stream)
            k = hit_idx.numel()
            if k == 0:
                idx = hit_idx
                break
            c_occ = ds.trace_any_device(shadow32[hit_idx].view(-1), k)
            occ[hit_idx] = c_occ                                                   # scatter
            idx = hit_idx[torch.nonzero(c_occ == 0)[:, 0]]
        result["today"] = idx

    text, med = timed_together([("with lists", with_lists), ("wait + nonzero + gather + scatter", today)], sync)
    ids, cnt = result["lists"]
    k = int(cnt.item())
    same = k == result["today"].numel() and bool((ids[:k] == result["today"]).all().item())
    for name in text:
        print("(b) n=2^22, three bounces, %-34s: %s" % (name, text[name]), flush=True)
    print("(b) %d rays live after three bounces; both ways name the same rays: %s" % (k, same), flush=True)
    return 0 if same else 1


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
    log = sys.argv[sys.argv.index("--log") + 1] if "--log" in sys.argv else os.path.join(ROOT, "profiles", "listed_timing.log")
    lines = ["# scripts/listed_timing.py, %s" % time.strftime("%Y-%m-%d"), "# clock state before:"] + clock_state()
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
