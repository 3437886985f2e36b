"""The rule by which a batch is taken for a row-major image (rtk_amd/csrc/rtk_detect_rule.h: one copy for k_detect_row /
k_detect_check on the device and for rtk_trace_rays on the host), checked without a GPU: tests/detect_rule_driver.cpp is built by
the host compiler against that header alone, with -fsanitize=address,undefined, reads a ray array this test writes (numpy only,
the library is not loaded) and prints the image it finds. The batches of tests/test_gpu_trace.py's
test_an_image_is_recognised_without_the_hint give here what they give on the device. On every batch the driver also compares
the header's step test with the two forms it replaced (the host's ternaries, the device's fmaxf) at every ray."""
import os
import subprocess

import numpy as np
import pytest

from rtk_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _frame():
    return synth.rays_pinhole(256, 128)


def _end_replaced():
    r = _frame()                       # 128 rows: every row but the last is looked at
    r[6 * 256] = r[6 * 256 - 1]        # the step out of row 5's last ray is no jump any more
    return r


def _nan_in_ray_1():
    r = _frame()
    r["origin"][1, 0] = np.float32("nan")
    return r


# name -> (rays, (w, h)). The first six: what the device test asserts.
CASES = {
    "frame": (_frame, (256, 128)),
    "jittered": (lambda: synth.rays_pinhole(192, 320, jitter=synth.frame_jitter(3)), (192, 320)),
    "not_whole_blocks": (lambda: synth.rays_pinhole(200, 96), (200, 96)),
    "incoherent": (lambda: synth.rays_incoherent(32768), (0, 0)),
    "config1": (lambda: synth.rays_config1(32768), (0, 0)),
    "two_frames": (lambda: np.concatenate([synth.rays_pinhole(128, 64), synth.rays_pinhole(256, 96)]), (0, 0)),
    # the limits and the conditions on a candidate
    "three_rays": (lambda: _frame()[:3], (0, 0)),                       # n < 4
    "width_63": (lambda: synth.rays_pinhole(63, 128), (0, 0)),          # w >= 64
    "cut_short": (lambda: _frame()[:256 * 128 - 100], (0, 0)),          # n is no multiple of the first jump + 1
    "single_row": (lambda: synth.rays_pinhole(256, 1), (0, 0)),         # no jump at all
    "two_rows": (lambda: synth.rays_pinhole(256, 2), (256, 2)),         # n / w >= 2: the one end there is jumps
    "end_replaced": (_end_replaced, (0, 0)),                            # one looked-at row whose end does not jump
    # a NaN makes its differences NaN, and both max forms drop a NaN operand: the other five numbers of the step decide, as if
    # that component did not move. The frame stays the frame; what matters is that the forms agree (the driver compares them)
    "nan_in_ray_1": (_nan_in_ray_1, (256, 128)),
}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("detect_rule") / "detect_rule_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "rtk_amd", "csrc"),
                           os.path.join(ROOT, "tests", "detect_rule_driver.cpp"), "-o", exe])
    return exe


def test_header_includes_no_hip():
    includes = [l.split()[1] for l in open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_detect_rule.h")) if l.startswith("#include")]
    assert includes == ['"rtk.h"', "<math.h>", "<stddef.h>", "<stdint.h>"]
    assert "hip" not in open(os.path.join(ROOT, "include", "rtk.h")).read().lower()


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_image_a_batch_is_taken_for(driver, tmp_path, name):
    make, expect = CASES[name]
    rays = np.ascontiguousarray(make())
    assert rays.dtype.itemsize == 32
    path = str(tmp_path / "rays.bin")
    rays.tofile(path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([driver, path], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-4000:]
    assert tuple(int(x) for x in r.stdout.split()) == expect
