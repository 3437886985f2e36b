"""The LISTED forms of the hand-written per-lane kernels (rtk_lane_hot_closest_listed / rtk_lane_hot_any_listed, rtk_lane_hot.S) run
on the CPU in tests/gfx950_emu.py: the kernels read the number of rays of the batch from device memory when they start, clamp it
to the n of their argument, and are the plain kernels from there on.

700 rays on the 600-triangle soup of tests/test_lane_asm_emulated.py, whose helpers, scene builder and oracle are used here; the
output is pre-filled with 0x7e, so that a slot that is not listed and is written all the same shows. The kernel argument is the
88 bytes of the plain kernels plus a pointer at 88; the count lives in a mapping of its own, EIGHT bytes long: a kernel that
read the pointer from another offset, or read more than the count's eight bytes, fails the emulator's range check instead of
passing by accident."""
import struct

import numpy as np
import pytest

from rtk_amd.types import HIT_RECORD_DTYPE

from . import gfx950_emu as emu
from .test_lane_asm_emulated import (COUNTER_WORDS, LEFTOVER_WORD, NONE, build_bvh4, chain_oracle, check_closest, lane_obj, oracle,  # noqa: F401
                                     some_rays, soup)

N = 700
COUNTS = [0, 1, 63, 64, 65, 699, 700, 5000]
WORKGROUPS = 2
BUDGET = 2_000_000


def perms():
    third = np.arange(N - 1, -1, -3, dtype=np.uint64)                 # every third ray, descending
    twice = np.arange(N, dtype=np.uint64)
    twice[10] = 7                                                      # ray 7 twice, ray 10 never
    # (the upper halves are not the kernel's business: only the low 32 bits name a ray)
    return {"none": None, "third": third | (np.uint64(0xabcd) << np.uint64(32)), "twice": twice}


def run_listed(obj, any_hit, qn, tr, rays, count, perm, max_instructions=BUDGET):
    mem = emu.Memory()
    a_q, a_t, a_r = mem.add("qnodes", qn), mem.add("tris", tr), mem.add("rays", rays)
    out = np.full(N, 0x7e, dtype=np.uint8) if any_hit else np.zeros(N, dtype=HIT_RECORD_DTYPE)
    if not any_hit:
        out.view(np.uint32)[:] = 0x7e7e7e7e
    a_o = mem.add("out", out)
    a_c = mem.add("counter", np.zeros(COUNTER_WORDS, dtype=np.uint64))
    a_l = mem.add("leftover", np.zeros(N, dtype=np.uint64))
    a_p = mem.add("perm", perm) if perm is not None else 0
    a_n = mem.add("count", np.array([count], dtype=np.uint64))        # eight bytes, a mapping of its own
    bound = max(1.0, float(np.abs(tr["v0"]).max()), float(np.abs(tr["v1"]).max()), float(np.abs(tr["v2"]).max()))
    lanes = WORKGROUPS * 256
    a_s = mem.add("spill", np.zeros(lanes * 40, dtype=np.uint64))
    karg = struct.pack("<7Q3IfQ2IQ", a_q, a_t, a_r, a_o, a_c, a_l, a_p, N, 8, 32, bound, a_s, lanes, 40, a_n)
    assert len(karg) == 96
    stats = emu.run_kernel(obj, "rtk_lane_hot_any_listed" if any_hit else "rtk_lane_hot_closest_listed", mem, karg, WORKGROUPS, 30720,
                           max_instructions=max_instructions)
    res = mem.get(a_o).view(out.dtype).copy()
    counter = mem.get(a_c).view(np.uint64)
    left = mem.get(a_l).view(np.uint64)[:int(counter[LEFTOVER_WORD])].copy()
    # the queue heads rtk_trace_kernel deals the left-over list from (the first word of each queue's line) are untouched
    assert all(int(counter[16 + 16 * q]) == 0 for q in range(8))
    assert int(mem.get(a_n).view(np.uint64)[0]) == count               # the count is read, never written
    return res, left, stats


def listed_ids(count, perm):
    m = min(count, N)
    if perm is None:
        return np.arange(m, dtype=np.int64)
    assert m <= len(perm) or count > len(perm)
    return (perm[:min(m, len(perm))] & np.uint64(0xffffffff)).astype(np.int64)


@pytest.fixture(scope="module")
def truth(oracle, soup):
    tv, _ = soup
    rays = some_rays(N, 11)
    g_hits, g_mask = chain_oracle(oracle, tv, rays)
    return rays, g_hits, g_mask


@pytest.mark.parametrize("which", ["none", "third", "twice"])
@pytest.mark.parametrize("count", COUNTS)
def test_closest_listed(lane_obj, soup, truth, count, which):
    _, (qn, tr) = soup
    rays, g_hits, g_mask = truth
    perm = perms()[which]
    if perm is not None and which == "third":
        count = min(count, len(perm))          # d_ids holds at least the entries that are traced: the contract of a list
    ids = listed_ids(count, perm)
    res, left, stats = run_listed(lane_obj, False, qn, tr, rays, count, perm)
    listed = np.zeros(N, bool)
    listed[ids] = True
    words = res.view(np.uint32).reshape(N, 4)
    assert (words[~listed] == 0x7e7e7e7e).all(), "a slot that is not listed was written"
    # listed slots: bit-equal to the oracle, or handed back (check_closest), on the listed rays alone
    sub = np.nonzero(listed)[0]
    left_ids = (left & np.uint64(0xffffffff)).astype(np.int64)
    assert np.isin(left_ids, sub).all()
    pos = {int(r): i for i, r in enumerate(sub)}
    left_sub = np.array([pos[int(r)] for r in left_ids], dtype=np.uint64)
    check_closest(res[sub], left_sub, g_hits[sub], g_mask[sub], rays[sub])
    if count == 0:
        assert not listed.any() and len(left) == 0


@pytest.mark.parametrize("which", ["none", "third", "twice"])
@pytest.mark.parametrize("count", COUNTS)
def test_any_listed(lane_obj, soup, truth, count, which):
    _, (qn, tr) = soup
    rays, g_hits, g_mask = truth
    perm = perms()[which]
    if perm is not None and which == "third":
        count = min(count, len(perm))
    ids = listed_ids(count, perm)
    res, left, _ = run_listed(lane_obj, True, qn, tr, rays, count, perm)
    listed = np.zeros(N, bool)
    listed[ids] = True
    left_ids = (left & np.uint64(0xffffffff)).astype(np.int64)
    done = listed.copy()
    done[left_ids] = False
    assert np.isin(left_ids, np.nonzero(listed)[0]).all()
    # bytes next to written bytes included: every byte that is not a finished listed ray still holds the fill
    assert (res[~done] == 0x7e).all(), "a byte that is not listed (or was handed back) was written"
    assert (res[done] == g_mask[done].astype(np.uint8)).all()
    if 0 < count < N and perm is None:
        assert res[min(count, N) - 1] != 0x7e or not done[min(count, N) - 1]
        assert res[min(count, N)] == 0x7e


def test_count_zero_ends_within_the_budget(lane_obj, soup, truth):
    """count 0: every wave asks each of the eight queues once, finds nothing and ends -- a few hundred instructions, not a spin."""
    _, (qn, tr) = soup
    rays = truth[0]
    for any_hit in (False, True):
        res, left, stats = run_listed(lane_obj, any_hit, qn, tr, rays, 0, None, max_instructions=2000)
        assert len(stats) == WORKGROUPS * 4 and all(s["total"] < 2000 for s in stats)
        assert (res.view(np.uint8) == 0x7e).all() and len(left) == 0


def test_a_count_of_2_to_the_32_and_more_is_all_rays(lane_obj, soup, truth):
    _, (qn, tr) = soup
    rays, g_hits, g_mask = truth
    res, left, _ = run_listed(lane_obj, True, qn, tr, rays, (1 << 32) + 5, None)
    assert len(left) == 0 and (res == g_mask.astype(np.uint8)).all()


def test_a_wrong_layout_fails_the_range_check(lane_obj, soup, truth):
    """The same launch with the count's pointer four bytes off: the eight-byte mapping makes that a range-check failure."""
    _, (qn, tr) = soup
    rays = truth[0]
    mem = emu.Memory()
    a_n = mem.add("count", np.array([5], dtype=np.uint64))
    karg = struct.pack("<7Q3IfQ2IQ", 0, 0, 0, 0, 0, 0, 0, N, 8, 32, 1.0, 0, 512, 40, a_n + 4)
    with pytest.raises(emu.EmuError, match="outside every buffer"):
        emu.run_kernel(lane_obj, "rtk_lane_hot_any_listed", mem, karg, 1, 30720, max_instructions=2000)


def test_the_plain_kernels_keep_their_88_bytes(lane_obj):
    """rtk_lane_hot_closest / _any never read offset 88 of their argument: the listed forms are new symbols, not a changed old one."""
    k = emu.disassemble(lane_obj)
    assert {"rtk_lane_hot_closest", "rtk_lane_hot_any", "rtk_lane_hot_closest_listed", "rtk_lane_hot_any_listed"} <= set(k)
    for name in ("rtk_lane_hot_closest", "rtk_lane_hot_any"):
        loads = [(op, ops) for _, op, ops, _ in k[name][0] if op.startswith("s_load")]
        assert len(loads) == 4 and all(ops[1] == "s[0:1]" and int(ops[2], 0) + 4 * int(op[len("s_load_dwordx"):]) <= 88 for op, ops in loads)
    for name in ("rtk_lane_hot_closest_listed", "rtk_lane_hot_any_listed"):
        loads = [(op, ops) for _, op, ops, _ in k[name][0] if op.startswith("s_load")]
        assert len(loads) == 6 and ("s_load_dwordx2", ["s[86:87]", "s[0:1]", "0x58"]) in loads


def test_no_wait_state_findings(lane_obj):
    import os
    import subprocess
    csrc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "rtk_amd", "csrc")
    out = subprocess.run(["make", "-s", "-C", csrc, "lint"], check=True, capture_output=True, text=True).stdout
    for name in ("rtk_lane_hot_closest_listed", "rtk_lane_hot_any_listed"):
        assert any(name + ":" in l and l.endswith(" 0 findings") for l in out.splitlines()), out
