"""How the host-pointer calls cut a batch (rtk_amd/csrc/rtk_host_pieces.h), checked without a GPU: tests/host_pieces_driver.cpp is
built by the host compiler against that header alone, with -fsanitize=address,undefined, allocates every buffer at exactly the
stated size and fills it, and runs the two-slot pipeline and the candidate rounds with recording callables. What is expected is
stated here independently: the layout as sizes in order, the band rule in words, the pipeline as a queue of at most two pieces
in flight, the candidate rounds by brute force over each ray's list. The run ends clean with leak detection on."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZERO_COPY_RAYS, PIPE_CHUNK_RAYS, CAND_SLOTS, CAND_RAYS = 2048, 1 << 15, 1 << 16, 1 << 14
RAY, RECORD, HIT = 32, 16, 68          # sizeof(rtk_ray), sizeof(rtk_hit_record), sizeof(rtk_hit)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("host_pieces") / "host_pieces_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "rtk_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host_pieces_driver.cpp"), "-o", exe])
    return exe


def run(driver, commands):
    """the answers' words, one list per command, from one clean run"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([driver], input="".join(c + "\n" for c in commands), capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-4000:]
    out = [line.split() for line in r.stdout.splitlines()]
    assert len(out) == len(commands)
    return out


def test_header_includes_no_hip():
    includes = [l.split()[1] for l in open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_host_pieces.h")) if l.startswith("#include")]
    assert includes == ['"rtk_amd.h"', "<string.h>", "<vector>"]


def test_the_numbers(driver):
    got = run(driver, ["consts", "ticket 0", "ticket 1", "ticket 4294967294", "ticket 4294967295"] + ["candk %d" % r for r in (1, 1024, 1025, 16383, 16384)])
    assert [int(x) for x in got[0]] == [ZERO_COPY_RAYS, PIPE_CHUNK_RAYS, CAND_SLOTS, CAND_RAYS]
    assert [int(g[0]) for g in got[1:5]] == [1, 2, 4294967295, 1]                   # after 0xffffffff comes 1: 0 means "no ticket"
    assert [int(g[0]) for g in got[5:]] == [64, 64, 63, 4, 4]                       # min(64, 65536 / rays)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 2048, 32768, 262144])
def test_staging_layout(driver, n):
    cap, total, *offsets = [int(x) for x in run(driver, ["staging %d" % n])[0]]
    assert cap >= max(n, 64) and cap & (cap - 1) == 0 and (cap == 64 or cap // 2 < n)       # the power of two at or above n, 64 at least
    sizes = [cap * RAY, cap * RECORD, cap * RECORD, cap * HIT, cap * 4, 64]         # rays, records, after, hits, mask, status
    at = 0
    for offset, size in zip(offsets, sizes):        # one after the other: nothing overlaps, nothing is left between
        assert offset == at
        at += size
    assert at == total == cap * (RAY + 2 * RECORD + HIT + 4) + 64                   # ... and the last one ends with the allocation
    assert offsets[4] % 4 == 0 and offsets[5] % 8 == 0                              # the mask, the status word


def test_candidate_layout(driver):
    total, cand, hits, count = [int(x) for x in run(driver, ["cand"])[0]]
    assert (cand, hits, count) == (0, CAND_SLOTS * RECORD, CAND_SLOTS * (RECORD + HIT)) and total == count + CAND_RAYS * 4
    assert hits % 4 == 0 and count % 4 == 0


def band_rule(w, h):
    """A frame of whole 64 x 64 blocks, at least 128 wide, whose 64 rows are at most 2^21 rays, goes in bands: 64 rows, doubled
    while the double is at most 2^18 rays and at most the frame's height. Rays per band; 0: no bands."""
    if w < 128 or w % 64 or h % 64 or w * 64 > 1 << 21:
        return 0
    rows = 64
    while rows * 2 * w <= 1 << 18 and rows * 2 <= h:
        rows *= 2
    return rows * w


def test_band_rule(driver):
    shapes = [(w, h) for w in (64, 128, 192, 4096, 32768, 32832) for h in (64, 128, 704, 4096)] + [(0, 0), (100, 64), (128, 100), (1024, 704)]
    got = [int(g[0]) for g in run(driver, ["band %d %d" % s for s in shapes])]
    assert got == [band_rule(w, h) for w, h in shapes]
    for (w, h), rays in zip(shapes, got):
        if w in (64, 32832, 0, 100) or h == 100:
            assert rays == 0                                    # narrower than two blocks; 64 rows beyond 2^21 rays; not whole blocks
            continue
        assert rays > 0 and rays % (64 * w) == 0                # whole 64-row bands
        assert rays <= 1 << 18 or rays == 64 * w                # at most 2^18 rays unless a single band is already larger
        assert rays // w <= h                                   # at most the frame's rows
    assert dict(zip(shapes, got))[(1024, 704)] == 256 * 1024    # (two bands and a lower third one: 256 + 256 + 192 rows)
    assert dict(zip(shapes, got))[(32768, 64)] == 64 * 32768


def pipeline(n, chunk, fail_enqueue, fail_finish):
    """At most two pieces in flight, finished in the order they were enqueued; piece p goes to slot p & 1, which is free once the
    older of two pieces in flight has been finished; the first failure ends the enqueueing, what is in flight is still finished."""
    calls, flight, count, failed, enqueues, finishes = [], [], 0, False, 0, 0

    def finish_oldest():
        nonlocal count, failed, finishes
        slot, at, m = flight.pop(0)
        calls.append("f%d:%d:%d" % (slot, at, m))
        if finishes == fail_finish:
            failed = True
        else:
            count += m
        finishes += 1
    for p in range((n + chunk - 1) // chunk):
        if len(flight) == 2:
            finish_oldest()
            if failed:
                break
        piece = (p & 1, p * chunk, min(chunk, n - p * chunk))
        calls.append("e%d:%d:%d" % piece)
        enqueues += 1
        if enqueues - 1 == fail_enqueue:
            failed = True
            break
        flight.append(piece)
    while flight:
        finish_oldest()
    return [str(-1 if failed else count)] + calls


def test_pipeline_order_with_and_without_failures(driver):
    cases = []
    for chunk in (PIPE_CHUNK_RAYS, 64 * 1024):
        for n in (2 * chunk - 1, 2 * chunk, 2 * chunk + 1, 5 * chunk + 7):
            pieces = (n + chunk - 1) // chunk
            cases.append((n, chunk, -1, -1))
            cases += [(n, chunk, q, -1) for q in range(pieces)] + [(n, chunk, -1, q) for q in range(pieces)]
    got = run(driver, ["pipe %d %d %d %d" % c for c in cases])
    assert got == [pipeline(*c) for c in cases]
    by_case = dict(zip(cases, got))
    c = PIPE_CHUNK_RAYS
    assert by_case[(2 * c + 1, c, -1, -1)] == [str(2 * c + 1), "e0:0:%d" % c, "e1:%d:%d" % (c, c), "f0:0:%d" % c, "e0:%d:1" % (2 * c), "f1:%d:%d" % (c, c), "f0:%d:1" % (2 * c)]
    assert by_case[(2 * c, c, -1, -1)] == [str(2 * c), "e0:0:%d" % c, "e1:%d:%d" % (c, c), "f0:0:%d" % c, "f1:%d:%d" % (c, c)]
    # piece 3 cannot be enqueued (its slot's piece 1 has been finished for it): piece 2, still in flight, is finished
    assert by_case[(5 * c + 7, c, 3, -1)] == ["-1", "e0:0:%d" % c, "e1:%d:%d" % (c, c), "f0:0:%d" % c, "e0:%d:%d" % (2 * c, c), "f1:%d:%d" % (c, c),
                                              "e1:%d:%d" % (3 * c, c), "f0:%d:%d" % (2 * c, c)]
    # the finish of piece 1 fails where slot 1 is wanted for piece 3: nothing more is enqueued, piece 2 is still finished
    assert by_case[(5 * c + 7, c, -1, 1)] == ["-1", "e0:0:%d" % c, "e1:%d:%d" % (c, c), "f0:0:%d" % c, "e0:%d:%d" % (2 * c, c), "f1:%d:%d" % (c, c), "f0:%d:%d" % (2 * c, c)]


def candidate_rounds(n, first_k, shift):
    """(accepted hits, rounds, per ray (accepted candidate or -1, offers)): the accepted candidate is the first one not rejected,
    every candidate up to it is offered once; rounds by going through them: k = min(64, 65536 / rays in the round), and a ray
    goes on while its list came back full and all of it was rejected."""
    lengths = (0, 1, first_k - 1, first_k, first_k + 1, 100, 150)
    length = [lengths[(i + shift) % 7] for i in range(n)]
    rejects = [(5 * (i + shift) + (i + shift) // 7) % 160 for i in range(n)]
    per_ray = [(rejects[i], rejects[i] + 1) if rejects[i] < length[i] else (-1, length[i]) for i in range(n)]
    rounds = 0
    for at in range(0, n, CAND_RAYS):
        todo = {i: 0 for i in range(at, min(n, at + CAND_RAYS))}          # ray -> candidates seen so far
        while todo:
            rounds += 1
            k = min(64, CAND_SLOTS // len(todo))
            todo = {i: seen + k for i, seen in todo.items() if length[i] - seen >= k and rejects[i] >= seen + k}
    return sum(1 for a, _ in per_ray if a >= 0), rounds, per_ray


@pytest.mark.parametrize("n,first_k", [(1, 64), (1024, 64), (16384, 4), (16385, 4)])
def test_candidate_rounds_against_brute_force(driver, n, first_k):
    shifts = range(0, 70, 3) if n == 1 else (0, 3)
    got = run(driver, ["rounds %d %d %d" % (n, first_k, s) for s in shifts])
    for s, g in zip(shifts, got):
        count, rounds, per_ray = candidate_rounds(n, first_k, s)
        assert [int(x) for x in g[:3]] == [count, rounds, 0], (n, s, g[:3])           # (0: nothing out of order, twice, or after a short list)
        assert g[3:] == ["%d:%d" % p for p in per_ray], (n, s)
    assert first_k == min(64, CAND_SLOTS // min(n, CAND_RAYS))


def test_leak_detection_is_on(driver):
    """The proof rests on it: memory nobody frees (the driver's `leak`) fails the run."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([driver], input="leak\n", capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode != 0 and "LeakSanitizer" in r.stderr
