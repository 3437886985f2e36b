"""CPU tests of rtk_dev_trace_rays_count / rtk_dev_trace_rays_all: the ABI, the refusals that are decided before any HIP call, and
the fixtures of tests/test_gpu_allhits.py against the oracle alone (what the GPU is compared with must itself be right: 24
crossings per generic ray of the sheets, the analytic inside / outside of the box)."""
import ctypes as C
import os

import numpy as np

from tests import allhits_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_BAD_ARG = -2


def test_symbols_are_exported_and_declared(api):
    text = open(os.path.join(ROOT, "include", "rtk_amd.h")).read()
    L = api.lib()
    for name in ("rtk_dev_trace_rays_count", "rtk_dev_trace_rays_all", "rtk_amd_allhits_stack_entries"):
        assert hasattr(L, name), name
        assert name in api.RTK_AMD_H_SYMBOLS and name + "(" in text
    for word in ("int rtk_dev_trace_rays_count(const rtk_dev_scene *ds, const rtk_ray *d_rays, size_t n,",
                 "const uint64_t *d_offsets, rtk_hit_record *d_records, uint32_t *d_written /* may be NULL */,",
                 "uint32_t rtk_amd_allhits_stack_entries(void);", "FAR BOUND FIXED", "ONLY THE EXACT NODES", "ARE NOT WRITTEN", "NOT CHECKED"):
        assert word in text, word
    assert 1 <= L.rtk_amd_allhits_stack_entries() <= 64
    assert L.rtk_dev_trace_rays_count.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(api.DevFilter), C.POINTER(api.TraceOpts), C.c_void_p]
    assert L.rtk_dev_trace_rays_all.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(api.DevFilter),
                                                 C.POINTER(api.TraceOpts), C.c_void_p]
    for name in ("count_hits_device", "trace_all_device", "trace_all", "contains", "count_hits"):
        assert callable(getattr(api.DeviceScene, name))


def test_refusals_need_no_device(api):
    """RTK_AMD_ERR_BAD_ARG for everything the host can see, a NULL scene included, on a machine without a GPU: `dummy` stands for
    a scene and for device memory, and is never looked at"""
    L = api.lib()
    dummy = C.cast(C.create_string_buffer(64), C.c_void_p)

    def filt(size):
        f = api.DevFilter()
        f.struct_size = size
        return f
    small, masked = filt(8), filt(C.sizeof(api.DevFilter))
    masked.d_mesh_mask = dummy.value                      # a mask without mesh_mask_bits
    for args in ((None, dummy, 4, dummy, None, None, None), (dummy, None, 4, dummy, None, None, None), (dummy, dummy, 4, None, None, None, None),
                 (dummy, dummy, 4, dummy, C.byref(small), None, None), (dummy, dummy, 4, dummy, C.byref(masked), None, None),
                 (dummy, dummy, 1 << 32, dummy, None, None, None), (None, None, 0, None, None, None, None)):
        assert L.rtk_dev_trace_rays_count(*args) == ERR_BAD_ARG, args
        assert "rtk_dev_trace_rays_count" in api.last_error()
    for args in ((None, dummy, 4, dummy, dummy, None, None, None, None), (dummy, None, 4, dummy, dummy, None, None, None, None),
                 (dummy, dummy, 4, None, dummy, None, None, None, None), (dummy, dummy, 4, dummy, None, dummy, None, None, None),
                 (dummy, dummy, 4, dummy, dummy, None, C.byref(small), None, None), (dummy, dummy, 4, dummy, dummy, dummy, C.byref(masked), None, None),
                 (dummy, dummy, 1 << 32, dummy, dummy, None, None, None, None)):
        assert L.rtk_dev_trace_rays_all(*args) == ERR_BAD_ARG, args
        assert "rtk_dev_trace_rays_all" in api.last_error()
    # no rays: nothing to do, nothing launched, whatever the other pointers are
    assert L.rtk_dev_trace_rays_count(dummy, None, 0, None, None, None, None) == 0
    assert L.rtk_dev_trace_rays_all(dummy, None, 0, None, None, None, None, None, None) == 0


def test_sheets_fixture_against_the_oracle_alone(oracle):
    """Case 1 of the GPU tests: every generic ray crosses the 24 squares once each, in z order; a ray aimed at the shared diagonal
    is offered both triangles of every square (rtk accepts an exact zero on both sides of an edge)"""
    meshes = R.sheets_meshes()
    assert len(meshes) == 3 and sum(len(m["positions"]) for m in meshes) == 3 * 48
    rays, generic = R.sheets_rays()
    assert len(rays) == 1024 and generic.sum() == 960
    blob = oracle.build_scene(meshes)
    want = R.oracle_lists(oracle, blob, rays, [0, 16, 32, 48])
    assert (want.counts[generic] == R.SHEETS).all()
    for i in np.nonzero(generic)[0][::37]:
        l = want.of(i)
        assert (np.diff(l["t"]) > 0).all()
        squares = l["prim"] // 2
        assert sorted(squares.tolist()) == list(range(24))
        up = rays["direction"][i][2] > 0
        assert (squares == (np.arange(24) if up else np.arange(23, -1, -1))).all()
        z = rays["origin"][i][2] + l["t"] * rays["direction"][i][2]
        assert np.allclose(z, 0.25 * squares, atol=1e-5)
    diag = np.arange(960, 1016)
    assert (want.counts[diag] == 2 * R.SHEETS).all()                     # both triangles of every square
    for i in diag[::11]:
        l = want.of(i)
        assert (l["t"][0::2] == l["t"][1::2]).all() and (l["prim"][0::2] + 1 == l["prim"][1::2]).all()   # equal t: ascending prim
    assert (want.counts[1016:] >= R.SHEETS).all()                        # corners: at least one triangle of every square


def test_box_fixture_against_the_oracle_alone(oracle):
    """Case 10: the parity of the oracle's counts is the analytic inside / outside of the box"""
    blob = oracle.build_scene(R.box_mesh())
    pts, inside = R.box_points()
    assert 100 < inside.sum() < 400
    want = R.oracle_lists(oracle, blob, R.make_rays(pts, R.CONTAINS_DIRECTION), [0, 12])
    assert ((want.counts & 1).astype(bool) == inside).all()
    assert (want.counts[inside] == 1).all() and np.isin(want.counts[~inside], (0, 2)).all()


def test_oracle_lists_follow_the_filters(oracle):
    """The reference's own paging: `after` a ray's third record gives the list from the fourth on, an ignored primitive is missing,
    a hidden mesh is missing -- on the soup, a few hundred rays"""
    meshes = R.soup_meshes()
    base = [0, 1000, 2000, 3000]
    blob = oracle.build_scene(meshes)
    rays = R.soup_rays()[:300]
    full = R.oracle_lists(oracle, blob, rays, base)
    assert full.counts.max() >= 6
    after = np.zeros(len(rays), R.HIT_RECORD_DTYPE)
    after["prim"] = R.NONE
    ignore = np.full(len(rays), R.NONE, np.uint32)
    for i in range(len(rays)):
        if full.counts[i] >= 3:
            after[i] = full.of(i)[2]
        if full.counts[i] >= 1:
            ignore[i] = full.of(i)[0]["prim"]
    paged = R.oracle_lists(oracle, blob, rays, base, after=after)
    skipped = R.oracle_lists(oracle, blob, rays, base, ignore_prim=ignore)
    hidden = R.oracle_lists(oracle, blob, rays, base, mesh_mask=[True, False, True])
    for i in range(len(rays)):
        l = full.of(i)
        assert paged.of(i).tobytes() == (l[3:] if full.counts[i] >= 3 else l).tobytes()
        assert skipped.of(i).tobytes() == l[1:].tobytes()
        assert hidden.of(i).tobytes() == l[(l["prim"] < 1000) | (l["prim"] >= 2000)].tobytes()
