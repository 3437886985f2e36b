"""Where a steady-state rtk_dev_scene_refit spends its time and its bytes, per kernel, at 1 M and 10 M triangles:
  * one `rocprofv3 --kernel-trace` run per size (a run of its own, the program after `--`): launches and kernel times;
  * two `rocprofv3 --pmc` runs per size, FETCH_SIZE and WRITE_SIZE apart and without any tracing: fabric bytes by the
    formula of profiles/r05_build_traffic.log, traffic = (2 * FETCH_SIZE + WRITE_SIZE) KiB per launch (gfx950 counts half
    of the bytes of 16-byte reads).
The profiled program (--child N) builds the scene once, refits it once (schedule, side arrays) and then REFITS more times;
the steady refits are the dispatches from the second k_refit_tris on. Every run is a child under `timeout`; the first one
that fails ends the script. Writes profiles/refit_profile.log.
Usage: python scripts/refit_profile.py [--log FILE] [--out DIR] [sizes...]"""
import collections
import csv
import glob
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REFITS = 10


def child(n):
    import torch
    from rtk_amd import api, synth
    d0 = torch.from_numpy(synth.triangle_soup(n, 0.02 if n <= 1_000_000 else 0.01, seed=1)).cuda()
    ds = api.DeviceScene.build([dict(positions=d0)])
    ds.refit([dict(positions=d0)])
    ms = []
    for _ in range(REFITS):
        ds.refit([dict(positions=d0)])
        ms.append(ds.last_refit_ms())
    print("refit_ms_median %.4f" % statistics.median(ms), flush=True)
    return 0


def short(name):
    m = re.search(r"(k_[a-z_0-9]+|rtk_[a-z_0-9]+|__amd_[a-zA-Z_]+)", name)
    return m.group(1) if m else name[:28]


def steady(rows, key):
    """rows of one csv in dispatch order -> those of the steady refits."""
    rows = sorted(rows, key=key)
    starts = [i for i, r in enumerate(rows) if short(r["Kernel_Name"]) == "k_refit_tris"]
    assert len(starts) == REFITS + 1, "expected %d k_refit_tris launches, found %d" % (REFITS + 1, len(starts))
    first = starts[1]
    # (the memset of the constants and the copy of the mesh table come before k_refit_tris inside a refit: take them along)
    while first > 0 and short(rows[first - 1]["Kernel_Name"]).startswith("__amd_"):
        first -= 1
    return rows[first:]


def run(out, tag, args, n, limit=300):
    d = os.path.join(out, tag)
    cmd = ["timeout", "-k", "10", str(limit), "rocprofv3"] + args + ["-d", d, "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--child", str(n)]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit("%s failed (exit %d)" % (tag, p.returncode))
    m = re.search(r"refit_ms_median ([0-9.]+)", p.stdout)
    return d, float(m.group(1)) if m else float("nan")


def profile(n, out, lines):
    d, wall = run(out, "trace_%d" % n, ["--kernel-trace"], n)
    rows = []
    for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
        rows += list(csv.DictReader(open(f)))
    dur = collections.defaultdict(list)
    for r in steady(rows, lambda r: int(r["Start_Timestamp"])):
        dur[short(r["Kernel_Name"])].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    ctr = {}
    for name in ("FETCH_SIZE", "WRITE_SIZE"):
        d, _ = run(out, "%s_%d" % (name.lower(), n), ["--pmc", name], n)
        rows = []
        for f in glob.glob(d + "/**/*counter_collection.csv", recursive=True):
            rows += [r for r in csv.DictReader(open(f)) if r["Counter_Name"] == name]
        acc = collections.defaultdict(float)
        for r in steady(rows, lambda r: int(r["Dispatch_Id"])):
            acc[short(r["Kernel_Name"])] += float(r["Counter_Value"])
        ctr[name] = acc
    lines.append("# %d triangles, %d steady refits; traffic = (2*FETCH_SIZE + WRITE_SIZE) KiB per launch (gfx950 half-count of 16-B reads, MI355X_MICROARCH.md); "
                 "us and MB are per REFIT (all launches of the kernel in one refit)" % (n, REFITS))
    lines.append("%-28s %9s %8s %10s %10s %10s %9s" % ("kernel", "us/refit", "launches", "fetch MB", "write MB", "B/triangle", "GB/s"))
    tu = tf = tw = 0.0
    for k in sorted(dur, key=lambda k: -sum(dur[k])):
        us = sum(dur[k]) / 1e3 / REFITS
        f = 2.0 * ctr["FETCH_SIZE"].get(k, 0.0) * 1024 / REFITS
        w = ctr["WRITE_SIZE"].get(k, 0.0) * 1024 / REFITS
        tu += us; tf += f; tw += w
        lines.append("%-28s %9.1f %8.1f %10.1f %10.1f %10.1f %9.0f" % (k, us, len(dur[k]) / REFITS, f / 1e6, w / 1e6, (f + w) / n, (f + w) / (us * 1e-6) / 1e9 if us else 0))
    lines.append("%-28s %9.1f %8.1f %10.1f %10.1f %10.1f %9.0f" % ("all kernels", tu, sum(len(v) for v in dur.values()) / REFITS, tf / 1e6, tw / 1e6, (tf + tw) / n,
                                                                    (tf + tw) / (tu * 1e-6) / 1e9))
    lines.append("# wall time of a refit under the kernel trace: %.1f us, of which %.1f us outside kernels (launch gaps, the host's wait)" % (wall * 1e3, wall * 1e3 - tu))


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "--child":
        sys.exit(child(int(sys.argv[2])))
    argv = sys.argv[1:]
    log = os.path.join(ROOT, "profiles", "refit_profile.log")
    out = os.path.join(ROOT, "results", "refit_profile")
    if "--log" in argv:
        i = argv.index("--log"); log = argv[i + 1]; del argv[i:i + 2]
    if "--out" in argv:
        i = argv.index("--out"); out = argv[i + 1]; del argv[i:i + 2]
    sizes = [int(a) for a in argv] or [1_000_000, 10_000_000]
    lines = ["# scripts/refit_profile.py, %s" % time.strftime("%Y-%m-%d")]
    try:
        for n in sizes:
            profile(n, out, lines)
    finally:
        open(log, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
