"""The child test of the entry-list pre-pass (rtk_packet_entries_kernel) without a GPU: rtk_amd/csrc/rtk_entries_rule.h, run by
tests/entries_rule_driver.cpp under the address and undefined-behaviour sanitizers. The form the kernel runs -- per plane the
one corner of (origin box) x (reciprocal box) that can be the extreme -- against the eight-product form it replaced: the
listed bound bit for bit, and the admit decision."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rtk_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """Built against the header alone (no HIP include path), no FMA contraction as in the library. -O2 and -mfma: a compiler
    that were allowed to contract (d * r - m) would do it here."""
    exe = str(tmp_path_factory.mktemp("entries_rule") / "entries_rule_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-mfma", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + CSRC, os.path.join(ROOT, "tests", "entries_rule_driver.cpp"), "-o", exe])
    return exe


def test_rule_header_includes_no_hip_and_the_kernel_uses_it():
    text = open(os.path.join(CSRC, "rtk_entries_rule.h")).read()
    assert [l.split()[1] for l in text.splitlines() if l.startswith("#include")] == ["<math.h>", "<stdint.h>"]
    kernel = open(os.path.join(CSRC, "rtk_trace_packet.hip")).read()
    assert '#include "rtk_entries_rule.h"' in kernel
    body = kernel[kernel.index("rtk_packet_entries_kernel("):kernel.index("void rtk_packet_entries_launch(")]
    assert "rtk_entries_child(" in body and "rtk_entries_child_full(" not in body
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "rtk_entries_rule.h" in mk and "-ffp-contract=off" in mk


def test_reduced_corners_equal_all_eight_products(driver):
    """Edge cases (planes equal to an origin bound, zero-width origin boxes, both signs of zero, denormal differences, +-inf
    planes of empty slots; all eight octants) and four million random cases: not one bit, not one decision differs. The
    control -- the same products without the select by the difference's sign -- differs, so the comparison can fail."""
    r = subprocess.run([driver, "4000000", "20261019"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    m = re.fullmatch(r"ok (\d+) edge (\d+) random (\d+) control\n", r.stdout)
    assert m, r.stdout[-2000:]
    assert int(m.group(1)) >= 1000000 and int(m.group(2)) == 4000000 and int(m.group(3)) > 1000
