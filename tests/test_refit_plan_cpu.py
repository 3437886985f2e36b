"""What the host decides in a refit between the kernels (rtk_amd/csrc/rtk_refit_plan.h), checked without a GPU:
tests/refit_plan_driver.cpp is built by the host compiler against that header alone, with -fsanitize=address,undefined, and
answers a table of cases as a child process.

What is expected was written down by reading rtk_refit.hip as it was before these decisions moved into the header (refit_all,
refit_some, check_desc, check_mesh_positions, refit_on_device, make_schedule, make_partial_tables, schedule_tmp, tables_tmp), not
by running the new code. Every buffer a plan reads is a heap block of exactly the bytes expected here -- the position data of a
staged mesh, mesh_ids, level_start, mesh_base -- and the driver reads [0, staged) of every position buffer as the staging copy
would: a plan one byte too long is a heap overflow the address sanitizer reports."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DEFAULT, F32, F64, REAL, U16 = 0, 1, 2, 3, 4                  # rtk_type
OK, BAD_ARG, UNSUPPORTED = 0, -2, -6
SHARE = "RTK_AMD_REFIT_MESHES_SHARE"
WHOS = ["rtk_dev_scene_refit", "rtk_dev_scene_refit_placed", "rtk_dev_scene_refit_meshes", "rtk_dev_scene_refit_meshes_placed"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("refit_plan") / "refit_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "rtk_amd", "csrc"),
                           os.path.join(ROOT, "tests", "refit_plan_driver.cpp"), "-o", exe])
    return exe


def run(driver, commands, env=None):
    """The driver's answers to `commands`, one line each; the run ends clean under the sanitizers."""
    full = {k: v for k, v in os.environ.items() if not k.startswith("RTK_AMD_")}
    full.update(env or {})
    r = subprocess.run([driver], input="".join(c + "\n" for c in commands), capture_output=True, text=True, timeout=120, env=full)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(commands)
    return lines


def ints(driver, commands, env=None):
    return [[int(w) for w in line.split()] for line in run(driver, commands, env)]


def padded(b):
    return (max(b, 1) + 255) // 256 * 256


def carve(pieces):
    """offsets, bytes to allocate, unpadded sum: every piece on a 256-byte step, a piece of 0 bytes still takes one"""
    offs, at = [], 0
    for p in pieces:
        offs.append(at)
        at += padded(p)
    return offs, at, sum(pieces)


def test_plan_header_includes_no_hip():
    includes = [l.split()[1] for l in open(os.path.join(ROOT, "rtk_amd", "csrc", "rtk_refit_plan.h")) if l.startswith("#include")]
    assert includes == ['"rtk.h"', '"rtk_amd.h"', '"rtk_carve.h"', "<stddef.h>", "<stdint.h>", "<stdlib.h>", "<vector>"]


# ---------------------------------------------------------------------------------------------- refusals

def mesh(nt, ptype=F32, cb=0, data=1):
    return (nt, ptype, cb, data)


def check(meshes, who=0, scene=1, desc=1, placements=None, ids=None, ids_null=False, num_ids=None, base=None, have_meshes=1):
    """One call of entry point WHOS[who]. base: the scene's mesh_base (default: the sums of the description's counts)."""
    some, placed = who >= 2, who in (1, 3)
    placements = placed if placements is None else placements
    ids = list(ids or [])
    num_ids = len(ids) if num_ids is None else num_ids
    if base is None:
        base = [0]
        for m in meshes:
            base.append(base[-1] + m[0])
    words = ["check", WHOS[who], scene, desc, int(placed), int(placements), int(some), int(not ids_null), num_ids] + ([] if ids_null else ids)
    words += [len(base)] + base + [len(meshes), have_meshes]
    for m in meshes:
        words += list(m)
    return " ".join(str(w) for w in words)


def answer(line):
    left, text = line.split(" |", 1)
    rc, nothing, full, listed_tris, flags = left.split()
    return int(rc), int(nothing), int(full), int(listed_tris), flags, text.strip()


THREE = [mesh(4), mesh(0), mesh(6)]


def refusal_cases():
    cases = []
    for w, who in enumerate(WHOS):
        some = w >= 2
        ids = [0] if some else None
        null = (BAD_ARG, who + ": NULL argument")
        cases += [(check(THREE, w, scene=0, ids=ids), null), (check(THREE, w, desc=0, ids=ids), null)]
        if w in (1, 3):
            cases.append((check(THREE, w, placements=0, ids=ids), null))
        cases += [
            (check(THREE, w, have_meshes=0, ids=ids), (BAD_ARG, who + ": NULL meshes")),
            (check(THREE[:2], w, base=[0, 4, 4, 10], ids=ids), (BAD_ARG, who + ": 2 meshes, the scene was made from 3")),
            (check(THREE, w, base=[], ids=ids), (BAD_ARG, who + ": 3 meshes, the scene was made from 0")),
            (check([mesh(4), mesh(5), mesh(6)], w, base=[0, 4, 8, 14], ids=ids), (BAD_ARG, who + ": mesh 1 has 5 triangles, the scene's has 4")),
            (check([mesh(4, cb=1), mesh(0), mesh(6)], w, ids=ids), (UNSUPPORTED, who + ": mesh 0: position callbacks are not supported by a refit")),
            (check([mesh(4, ptype=U16), mesh(0), mesh(6)], w, ids=ids), (BAD_ARG, who + ": mesh 0: bad position type 4")),
            (check([mesh(4, ptype=7), mesh(0), mesh(6)], w, ids=ids), (BAD_ARG, who + ": mesh 0: bad position type 7")),
            (check([mesh(4, data=0), mesh(0), mesh(6)], w, ids=ids), (BAD_ARG, who + ": mesh 0 has no positions")),
        ]
        if some:
            cases += [
                (check(THREE, w, ids_null=True, num_ids=3), (BAD_ARG, who + ": NULL mesh_ids with 3 ids")),
                (check(THREE, w, ids=[0, 3]), (BAD_ARG, who + ": mesh id 3, the scene has 3 meshes")),
                (check(THREE, w, ids=[4294967295]), (BAD_ARG, who + ": mesh id 4294967295, the scene has 3 meshes")),
                # a callback is refused on an empty mesh too, if it is listed
                (check([mesh(4), mesh(0, cb=1), mesh(6)], w, ids=[1]), (UNSUPPORTED, who + ": mesh 1: position callbacks are not supported by a refit")),
            ]
        else:
            cases += [
                (check([mesh(4), mesh(0, cb=1), mesh(6)], w), (UNSUPPORTED, who + ": mesh 1: position callbacks are not supported by a refit")),
                (check([mesh(4), mesh(0), mesh(6, data=0)], w), (BAD_ARG, who + ": mesh 2 has no positions")),
            ]
    return cases


def test_every_refusal_with_its_code_and_text(driver):
    cases = refusal_cases()
    for (cmd, (rc, text)), line in zip(cases, run(driver, [c for c, _ in cases])):
        got = answer(line)
        assert (got[0], got[5]) == (rc, text), cmd


def test_order_between_refusals(driver):
    """NULL arguments, NULL mesh_ids, the description (NULL meshes, count, triangle counts), the ids' range, then the positions of
    the meshes that are read, in mesh order whatever the order of the ids: callback, type, data."""
    w, who = 3, WHOS[3]
    bad = [mesh(4, ptype=U16), mesh(5, cb=1), mesh(6, data=0)]
    ladder = [
        (check(bad[:2], w, placements=0, ids_null=True, num_ids=2, base=[0, 4, 9, 15]), who + ": NULL argument"),
        (check(bad[:2], w, ids_null=True, num_ids=2, base=[0, 4, 9, 15]), who + ": NULL mesh_ids with 2 ids"),
        (check(bad[:2], w, ids=[7], base=[0, 4, 9, 15], have_meshes=0), who + ": NULL meshes"),
        (check(bad[:2], w, ids=[7], base=[0, 4, 9, 15]), who + ": 2 meshes, the scene was made from 3"),
        (check(bad, w, ids=[7], base=[0, 4, 8, 14]), who + ": mesh 1 has 5 triangles, the scene's has 4"),
        (check(bad, w, ids=[2, 7, 0]), who + ": mesh id 7, the scene has 3 meshes"),
        (check(bad, w, ids=[2, 1, 0]), who + ": mesh 0: bad position type 4"),
        (check(bad, w, ids=[2, 1]), who + ": mesh 1: position callbacks are not supported by a refit"),
        (check(bad, w, ids=[2]), who + ": mesh 2 has no positions"),
        (check([mesh(4, ptype=U16, cb=1, data=0)], w, ids=[0]), who + ": mesh 0: position callbacks are not supported by a refit"),
        (check([mesh(4, ptype=U16, data=0)], w, ids=[0]), who + ": mesh 0: bad position type 4"),
        # the full form: NULL before the count before a bad type, and the first bad mesh speaks
        (check(bad[:2], 1, placements=0, base=[0, 4, 9, 15]), WHOS[1] + ": NULL argument"),
        (check(bad[:2], 1, base=[0, 4, 9, 15]), WHOS[1] + ": 2 meshes, the scene was made from 3"),
        (check(bad, 1), WHOS[1] + ": mesh 0: bad position type 4"),
        (check(bad[1:], 0), WHOS[0] + ": mesh 0: position callbacks are not supported by a refit"),
    ]
    for (cmd, text), line in zip(ladder, run(driver, [c for c, _ in ladder])):
        got = answer(line)
        assert got[0] != OK and got[5] == text, cmd


def test_what_is_not_refused(driver):
    """(rc, nothing, full, listed_tris, flags). The full forms flag nothing; the per-mesh forms look only at the listed meshes."""
    strange = [mesh(4), mesh(5, ptype=U16, data=0), mesh(0, ptype=7, data=0), mesh(6)]
    cases = [
        (check(THREE, 0), (OK, 0, 1, 0, "-")),
        (check(THREE, 1), (OK, 0, 1, 0, "-")),
        (check([mesh(4, DEFAULT), mesh(0, ptype=7, data=0), mesh(6, REAL), mesh(1, F64)], 0), (OK, 0, 1, 0, "-")),   # an empty mesh's type and data are not looked at
        (check([], 0, base=[]), (OK, 0, 1, 0, "-")),
        (check([], 0, base=[0]), (OK, 0, 1, 0, "-")),
        # some of the meshes: an unlisted one may have anything in its position fields
        (check(strange, 2, ids=[0]), (OK, 0, 0, 4, "1000")),
        (check(strange, 3, ids=[3, 0]), (OK, 0, 0, 10, "1001")),
        (check(strange, 2, ids=[3, 2]), (OK, 0, 0, 6, "0011")),
        # an id that repeats counts once
        (check(strange, 2, ids=[3, 3, 3]), (OK, 0, 0, 6, "0001")),
        (check(THREE, 2, ids=[0, 2, 0, 2]), (OK, 0, 1, 10, "101")),
        # only empty meshes, or none: nothing moves
        (check(THREE, 2, ids=[1]), (OK, 1, 0, 0, "010")),
        (check(THREE, 3, ids=[]), (OK, 1, 0, 0, "000")),
        (check(THREE, 2, ids_null=True, num_ids=0), (OK, 1, 0, 0, "000")),
        (check([], 2, base=[]), (OK, 1, 0, 0, "0")),
        (check([mesh(0)], 2, ids=[0]), (OK, 1, 0, 0, "1")),
        # every mesh that has a triangle is listed: the full refit, with or without the empty one
        (check(THREE, 2, ids=[0, 2]), (OK, 0, 1, 10, "101")),
        (check(THREE, 3, ids=[2, 1, 0]), (OK, 0, 1, 10, "111")),
        (check(THREE, 2, ids=[2]), (OK, 0, 0, 6, "001")),
    ]
    for (cmd, want), line in zip(cases, run(driver, [c for c, _ in cases])):
        got = answer(line)
        assert got[:5] == want and got[5] == "", cmd


# ---------------------------------------------------------------------------------------------- where positions are read from

def src(nt, ptype=F32, pstride=0, device=0, flag=1, mv=None):
    return dict(nt=nt, ptype=ptype, pstride=pstride, device=device, flag=flag, mv=3 * nt - 1 if mv is None else mv)


def expected_source(meshes, placed, listed, have_mv=True):
    """(need_mv, any_device, mode, upload_bytes, places_at, places), [(read, stride, f64, staged, staged_at, placed)] as the loop at the
    head of the parent's refit_on_device left them"""
    upload, per, any_device, f32, f64 = 0, [], 0, False, False
    for m in meshes:
        if m["nt"] == 0 or (listed and not m["flag"]):
            per.append((0, 0, 0, 0, 0, 0 if placed else -1))
            continue
        d = m["ptype"] == F64
        stride = m["pstride"] or (24 if d else 12)
        f64, f32 = f64 or d, f32 or not d
        staged = at = 0
        if m["device"]:
            any_device = 1
        else:
            if not have_mv:
                return None
            staged, at = m["mv"] * stride + (24 if d else 12), upload
            upload += padded(staged)
        per.append((1, stride, int(d), staged, at, 1 if placed else -1))
    places_at = places = 0
    if placed:
        places, places_at = max(len(meshes), 1), upload
        upload += padded(places * 48)
    return (0, any_device, 2 if f64 and f32 else 1 if f64 else 0, upload, places_at, places), per


def source_command(meshes, placed=0, listed=0, have_mv=1):
    words = ["source", placed, listed, have_mv, len(meshes)]
    want = expected_source(meshes, placed, listed)
    for m, per in zip(meshes, want[1]):
        words += [m["nt"], m["ptype"], m["pstride"], m["device"], m["flag"], m["mv"], per[3]]       # (allocated: exactly what is expected to be staged)
    return " ".join(str(w) for w in words)


def parse_source(line, count):
    w = [int(x) for x in line.split()]
    assert len(w) == 6 + 6 * count, line
    return tuple(w[:6]), [tuple(w[6 + 6 * k: 12 + 6 * k]) for k in range(count)]


SOURCE_CASES = [
    ("f32 only", [src(5), src(7, DEFAULT), src(2, REAL)], 0, 0),
    ("f64 only", [src(5, F64), src(7, F64)], 0, 0),
    ("mixed", [src(5, F64), src(7)], 0, 0),
    ("explicit strides", [src(5, F32, 20), src(7, F64, 40), src(3, F32, 12), src(3, F64, 24)], 0, 0),
    ("device meshes alone", [src(5, device=1), src(7, F64, device=1)], 0, 0),
    ("device and host", [src(5, device=1), src(7, F64), src(3, device=1), src(4)], 0, 0),
    ("an unlisted mesh", [src(5), src(7, F64, flag=0), src(3)], 0, 1),
    ("an unlisted mesh, placed", [src(5), src(7, F64, flag=0), src(3)], 1, 1),
    ("only the f64 mesh listed", [src(5, flag=0), src(7, F64), src(3, flag=0)], 1, 1),
    ("an empty mesh between two", [src(5), src(0), src(3, F64)], 0, 0),
    ("an empty mesh between two, placed", [src(5), src(0, F64), src(3, F64)], 1, 0),
    ("an empty listed mesh", [src(5), src(0), src(3)], 1, 1),
    ("staged 255", [src(9, pstride=243, mv=1), src(1)], 0, 0),
    ("staged 256", [src(9, pstride=244, mv=1), src(1)], 0, 0),
    ("staged 257", [src(9, pstride=245, mv=1), src(1)], 0, 0),
    ("staged 255 256 257, placed", [src(9, pstride=243, mv=1), src(9, pstride=244, mv=1), src(9, pstride=245, mv=1)], 1, 0),
    ("placed, nothing staged", [src(5, device=1), src(7, device=1)], 1, 0),
    ("placed, positions staged", [src(5), src(7, device=1)], 1, 0),
    ("fewer vertices than corners", [src(100, mv=4), src(100, F64, mv=0)], 0, 0),
    ("five placements", [src(1)] * 5, 1, 0),
    ("six placements", [src(1, device=1)] * 6, 1, 0),
    ("no mesh", [], 0, 0),
    ("no mesh, placed", [], 1, 0),
]


def test_source_plans(driver):
    lines = run(driver, [source_command(m, placed, listed) for _, m, placed, listed in SOURCE_CASES])
    for (name, meshes, placed, listed), line in zip(SOURCE_CASES, lines):
        assert "?" not in line, (name, line)
        want = expected_source(meshes, placed, listed)
        assert parse_source(line.replace(" SOURCE?", ""), len(meshes)) == want, name


def test_source_plans_spelled_out():
    """some of the above by hand: stride 0 is 12 or 24, staged = max_vertex * stride + 12 | 24, every copy on a 256-byte step, the
    placement table (48 bytes per mesh, one entry where there is no mesh) behind them"""
    by_name = {name: expected_source(m, placed, listed) for name, m, placed, listed in SOURCE_CASES}
    assert by_name["f32 only"] == ((0, 0, 0, 768, 0, 0), [(1, 12, 0, 14 * 12 + 12, 0, -1), (1, 12, 0, 20 * 12 + 12, 256, -1), (1, 12, 0, 5 * 12 + 12, 512, -1)])
    assert by_name["f64 only"] == ((0, 0, 1, 1024, 0, 0), [(1, 24, 1, 14 * 24 + 24, 0, -1), (1, 24, 1, 20 * 24 + 24, 512, -1)])
    assert by_name["mixed"][0][2] == 2
    assert [p[1:4] for p in by_name["explicit strides"][1]] == [(20, 0, 14 * 20 + 12), (40, 1, 20 * 40 + 24), (12, 0, 8 * 12 + 12), (24, 1, 8 * 24 + 24)]
    assert by_name["device meshes alone"] == ((0, 1, 2, 0, 0, 0), [(1, 12, 0, 0, 0, -1), (1, 24, 1, 0, 0, -1)])
    assert by_name["device and host"][0] == (0, 1, 2, 768, 0, 0) and [p[4] for p in by_name["device and host"][1]] == [0, 0, 0, 512]
    assert by_name["an unlisted mesh"] == ((0, 0, 0, 512, 0, 0), [(1, 12, 0, 180, 0, -1), (0, 0, 0, 0, 0, -1), (1, 12, 0, 108, 256, -1)])
    assert by_name["an unlisted mesh, placed"] == ((0, 0, 0, 768, 512, 3), [(1, 12, 0, 180, 0, 1), (0, 0, 0, 0, 0, 0), (1, 12, 0, 108, 256, 1)])
    assert by_name["only the f64 mesh listed"][0] == (0, 0, 1, 768, 512, 3)
    assert by_name["an empty mesh between two"][0] == (0, 0, 2, 512, 0, 0)
    assert [by_name["staged %d" % b] for b in (255, 256, 257)] == [
        ((0, 0, 0, 512, 0, 0), [(1, 243, 0, 255, 0, -1), (1, 12, 0, 36, 256, -1)]),
        ((0, 0, 0, 512, 0, 0), [(1, 244, 0, 256, 0, -1), (1, 12, 0, 36, 256, -1)]),
        ((0, 0, 0, 768, 0, 0), [(1, 245, 0, 257, 0, -1), (1, 12, 0, 36, 512, -1)])]
    assert by_name["staged 255 256 257, placed"][0] == (0, 0, 0, 256 + 256 + 512 + 256, 1024, 3)
    assert by_name["placed, nothing staged"][0] == (0, 1, 0, 256, 0, 2)
    assert by_name["placed, positions staged"][0] == (0, 1, 0, 512, 256, 2)
    assert by_name["five placements"][0] == (0, 0, 0, 5 * 256 + 256, 1280, 5) and by_name["six placements"][0] == (0, 1, 0, 512, 0, 6)
    assert by_name["no mesh"] == ((0, 0, 0, 0, 0, 0), []) and by_name["no mesh, placed"] == ((0, 0, 0, 256, 0, 1), [])


def test_max_vertex_is_demanded_only_for_a_host_mesh_that_is_read(driver):
    """Without the table: device meshes, unlisted and empty host meshes plan through; a host mesh that is read says 'make it first'."""
    fine = [[src(5, device=1), src(7, F64, device=1)], [src(5, device=1), src(7, flag=0), src(0)], []]
    needs = [[src(5)], [src(5, device=1), src(0), src(7, F64)], [src(5, flag=0), src(7)]]
    lines = run(driver, [source_command(m, 1, 1, have_mv=0) for m in fine + needs])
    for m, line in zip(fine, lines):
        want = expected_source(m, 1, 1, have_mv=False)
        assert want is not None and parse_source(line, len(m)) == want
    for m, line in zip(needs, lines[len(fine):]):
        assert expected_source(m, 1, 1, have_mv=False) is None and line.split()[0] == "1" and len(line.split()) == 6


# ---------------------------------------------------------------------------------------------- sizes and offsets

def test_schedule_and_tables_temporaries(driver):
    cases = [(n, sw) for n in (1, 63, 64, 65, 10_000, 2 ** 31) for sw in (16, 64, 65, 273)]
    for (n, sw), got in zip(cases, ints(driver, ["tmp %d %d" % c for c in cases])):
        offs, total, _ = carve([n * 4, 4, n * 8, n * 8, sw * 4, (n + 2) * 4])
        assert got == offs + [total], (n, sw)
    for (n, sw), got in zip(cases, ints(driver, ["tables %d %d" % c for c in cases])):
        offs, total, _ = carve([n * 8, n * 8, sw * 4])
        assert got == offs + [total], (n, sw)
    assert ints(driver, ["tmp 64 64", "tmp 65 65", "tables 0 16"]) == [[0, 256, 512, 1024, 1536, 1792, 2304], [0, 512, 768, 1536, 2304, 2816, 3328], [0, 256, 512, 768]]


def test_kept_allocations(driver):
    """the level starts with the mesh table behind the carve (not padded; room for one record where there is no mesh, which is not
    counted), and the eight tables of the per-mesh refit"""
    small = [(h, m) for h in (1, 63, 64, 200) for m in (0, 1, 2, 16)]
    for (h, m), got in zip(small, ints(driver, ["small %d %d" % c for c in small])):
        assert got == [padded((h + 1) * 4), padded((h + 1) * 4) + max(m, 1) * 24, (h + 1) * 4 + m * 24], (h, m)
    assert ints(driver, ["small 63 0", "small 64 3"]) == [[256, 280, 256], [512, 584, 332]]
    part = [(n, nt, m, h, (n + 1023) // 1024) for n, nt in ((1, 1), (64, 63), (65, 200), (4763, 10_000), (2 ** 30, 2 ** 30)) for m in (1, 16, 31, 32) for h in (1, 63, 64)]
    for (n, nt, m, h, nb), got in zip(part, ints(driver, ["partial %d %d %d %d %d" % c for c in part])):
        offs, total, counted = carve([n * 4, nt * 4, nt * 4, n * 4, n * 4, (nb + 1) * 4, (h + 1) * 4, (m + 1) * 8])
        assert got == offs + [total, counted], (n, nt, m, h)
    assert ints(driver, ["partial 64 63 31 63 1"]) == [[0, 256, 512, 768, 1024, 1280, 1536, 1792, 2048, 64 * 12 + 63 * 8 + 8 + 256 + 256]]


def test_borrow(driver):
    """the largest of: schedule bytes if the schedule is not ready, table bytes if meshes are listed and the tables are not ready,
    upload bytes; nothing needed: 0, no loan"""
    cases = [((0, 900, 1, 500, 300), 900), ((0, 500, 1, 900, 300), 900), ((0, 500, 1, 300, 900), 900),
             ((1, 900, 1, 500, 300), 500), ((1, 900, 0, 500, 300), 300), ((0, 900, 0, 5000, 300), 900), ((1, 900, 1, 500, 700), 700),
             ((1, 900, 0, 500, 0), 0), ((1, 0, 0, 0, 0), 0), ((0, 256, 1, 256, 256), 256)]
    assert ints(driver, ["borrow %d %d %d %d %d" % c for c, _ in cases]) == [[w] for _, w in cases]


# ---------------------------------------------------------------------------------------------- rules of the schedule

def test_sort_bits(driver):
    """heights: (1 << bits) <= n from 1 on; meshes: (1 << bits) < num_meshes from 0 on, 0 = no sort"""
    assert ints(driver, ["hbits %d" % n for n in (1, 2, 255, 256, 257, 2 ** 31)]) == [[1], [2], [8], [9], [9], [32]]
    assert ints(driver, ["mbits %d" % m for m in (1, 2, 3, 256, 257)]) == [[0], [1], [2], [8], [9]]
    ns = [1, 2, 3, 4, 7, 8, 1023, 1024, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1]
    assert ints(driver, ["hbits %d" % n for n in ns]) == [[min(max(n.bit_length(), 1), 32)] for n in ns]
    ms = [0, 1, 2, 3, 4, 5, 16, 17, 2 ** 30]
    assert ints(driver, ["mbits %d" % m for m in ms]) == [[max(m - 1, 0).bit_length()] for m in ms]


def test_sweep_rounds(driver):
    """first round min(max_depth + 1, 4096), then 8; given up past n + 8 sweeps"""
    depths = [0, 1, 20, 4094, 4095, 4096, 100_000]
    assert ints(driver, ["sweep 1 %d" % d for d in depths]) == [[1], [2], [21], [4095], [4096], [4096], [4096]]
    assert ints(driver, ["sweep 0 %d" % d for d in depths]) == [[8]] * len(depths)
    assert ints(driver, ["exhausted 108 100", "exhausted 109 100", "exhausted 8 0", "exhausted 9 0", "exhausted 4096 1"]) == [[0], [1], [0], [1], [1]]


def test_level_start_sanity(driver):
    cases = [(10, [0, 4, 10], 1), (10, [0, 10], 1), (1, [0, 1], 1), (10, [1, 4, 10], 0), (10, [0, 4, 9], 0), (10, [0, 4, 11], 0),
             (10, [0, 4, 4, 10], 0), (10, [0, 0, 10], 0), (10, [0, 10, 10], 0), (10, [0, 6, 4, 10], 0)]
    got = ints(driver, ["sane %d %d %s" % (n, len(ls), " ".join(map(str, ls))) for n, ls, _ in cases])
    assert got == [[w] for _, _, w in cases]


# ---------------------------------------------------------------------------------------------- per call

def runs_command(listed, base):
    return "runs %d %s %s" % (len(listed), " ".join(map(str, listed)), " ".join(map(str, base)))


def test_runs_of_listed_meshes(driver):
    """(threads, number of runs, then entry_begin thread_begin of each)"""
    cases = [
        (([1, 1, 0, 1, 0], [0, 10, 30, 60, 100, 150]), [70, 2, 0, 0, 60, 30]),           # meshes 0, 1 and 3 of 5: two runs
        (([1, 1, 1], [0, 10, 10, 30]), [30, 1, 0, 0]),                                   # an empty listed mesh between two does not break a run
        (([1, 0, 1], [0, 10, 10, 30]), [30, 1, 0, 0]),                                   # ... nor does an empty one that is not listed
        (([1, 0, 1], [0, 10, 20, 30]), [20, 2, 0, 0, 20, 10]),                           # an unlisted mesh does
        (([0, 1, 1], [0, 5, 9, 20]), [15, 1, 5, 0]),
        (([0, 1, 0, 1, 0, 1], [0, 1, 2, 3, 4, 5, 6]), [3, 3, 1, 0, 3, 1, 5, 2]),
        (([1], [0, 7]), [7, 1, 0, 0]),
        (([1, 1], [0, 0, 0]), [0, 0]),
        (([1, 1, 1, 1], [0, 1000, 1001, 5000, 2 ** 30]), [2 ** 30, 1, 0, 0]),
    ]
    assert ints(driver, [runs_command(*c) for c, _ in cases]) == [w for _, w in cases]


def levels_of(sizes):
    ls = [0]
    for s in sizes:
        ls.append(ls[-1] + s)
    return ls


def expected_levels(ls):
    """the walk both box passes of the parent made: a height of more than 1024 nodes alone, with ceil(4 nodes / 256) workgroups
    before any cap; a run of heights of at most 1024 nodes together"""
    steps, h, heights = [], 0, len(ls) - 1
    while h < heights:
        begin, end = ls[h], ls[h + 1]
        if end - begin > 1024:
            steps += [0, h, h + 1, begin, end, ((end - begin) * 4 + 255) // 256]
            h += 1
        else:
            h1 = h + 1
            while h1 < heights and ls[h1 + 1] - ls[h1] <= 1024:
                h1 += 1
            steps += [1, h, h1, begin, ls[h1], 1]
            h = h1
    return [len(steps) // 6] + steps


LEVEL_CASES = [[1023], [1024], [1025], [5, 2000, 3000], [1024, 1024, 1025, 2000], [2000, 5, 7, 3000], [3000, 2000, 100, 10, 1], [1000, 500, 3], [2000, 1500], [1],
               [131073], [1025, 1024, 1025, 1023, 1], [5000, 1200, 300, 80, 20, 5, 2, 1]]


def test_plan_levels(driver):
    got = ints(driver, ["levels %d %s" % (len(s) + 1, " ".join(map(str, levels_of(s)))) for s in LEVEL_CASES])
    assert got == [expected_levels(levels_of(s)) for s in LEVEL_CASES]
    want = {tuple(s): expected_levels(levels_of(s)) for s in LEVEL_CASES}
    assert want[(1023,)] == [1, 1, 0, 1, 0, 1023, 1] and want[(1024,)] == [1, 1, 0, 1, 0, 1024, 1] and want[(1025,)] == [1, 0, 0, 1, 0, 1025, 17]
    assert want[(5, 2000, 3000)] == [3, 1, 0, 1, 0, 5, 1, 0, 1, 2, 5, 2005, 32, 0, 2, 3, 2005, 5005, 47]
    assert want[(2000, 5, 7, 3000)] == [3, 0, 0, 1, 0, 2000, 32, 1, 1, 3, 2000, 2012, 1, 0, 3, 4, 2012, 5012, 47]
    assert want[(3000, 2000, 100, 10, 1)] == [3, 0, 0, 1, 0, 3000, 47, 0, 1, 2, 3000, 5000, 32, 1, 2, 5, 5000, 5111, 1]
    assert want[(1000, 500, 3)] == [1, 1, 0, 3, 0, 1503, 1]                      # all small: one launch
    assert want[(2000, 1500)][0] == 2 and want[(1,)] == [1, 1, 0, 1, 0, 1, 1]
    assert want[(131073,)] == [1, 0, 0, 1, 0, 131073, 2049]                      # more than the 2048 the list form launches at most


def test_dirty_set_decision(driver):
    """listed, the other boxes exact, and listed_tris <= share * num_tris; the share is 0.25 unless the environment says otherwise"""
    assert run(driver, ["share"]) == ["0.25"]
    assert ints(driver, ["dirty 1 1 250 1000", "dirty 1 1 251 1000", "dirty 1 0 250 1000", "dirty 0 1 250 1000", "dirty 1 1 1 3", "dirty 1 1 2500 10000", "dirty 1 1 2501 10000"]) == \
        [[1], [0], [0], [0], [0], [1], [0]]
    assert ints(driver, ["dirty 1 1 1 1000", "dirty 1 1 1000 1000"], {SHARE: "0"}) == [[0], [0]]
    assert ints(driver, ["dirty 1 1 1 1000", "dirty 1 1 1000 1000", "dirty 1 0 1 1000", "dirty 0 1 1 1000"], {SHARE: "1"}) == [[1], [1], [0], [0]]
    assert ints(driver, ["dirty 1 1 500 1000", "dirty 1 1 501 1000"], {SHARE: "0.5"}) == [[1], [0]]
    assert run(driver, ["share"], {SHARE: "0"}) == ["0"] and run(driver, ["share"], {SHARE: "1"}) == ["1"] and run(driver, ["share"], {SHARE: ""}) == ["0"]
    # read at every call
    got = run(driver, ["dirty 1 1 300 1000", "setenv %s 1" % SHARE, "dirty 1 1 300 1000", "setenv %s 0" % SHARE, "dirty 1 1 300 1000"])
    assert got == ["0", "ok", "1", "ok", "0"]


def test_epoch_step(driver):
    """++epoch; a wrap to 0 clears the flags and restarts at 1"""
    assert ints(driver, ["epoch 0", "epoch 1", "epoch 41", "epoch %d" % 0xfffffffe, "epoch %d" % 0xffffffff]) == [[1, 0], [2, 0], [42, 0], [0xffffffff, 0], [1, 1]]
