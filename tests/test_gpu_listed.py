"""GPU tests of ray lists (rtk_ray_list): rtk_dev_trace_rays_listed / rtk_dev_trace_rays_any_listed trace the rays a list on the
device names -- how many is read on the device too -- and write each result to the ray's own slot.

The bar: a listed slot holds byte for byte what the unlisted call writes there for the same ray array, and every other slot
still holds the 0x7e the output was filled with. Scene: the 10k-triangle synthetic scene, device-built (two meshes of 5000
triangles, so that a mesh mask has something to mask); rays: half rays_config1, half rays_incoherent. Sizes: the one-workgroup
boundary of the launch (256 / 257), one ray, one wave, a size that is no multiple of 64, and 65553 rays: many workgroups and all
eight queues. No list names a ray beyond num_rays."""
import ctypes as C

import numpy as np
import pytest

from rtk_amd import synth
from rtk_amd.types import HIT_RECORD_DTYPE

pytestmark = pytest.mark.gpu

SIZES = [1, 64, 256, 257, 5000, 65553]
NONE = 0xFFFFFFFF
BAD_ARG = -2


def some_rays(n):
    return np.ascontiguousarray(np.concatenate([synth.rays_config1(n // 2, seed=21), synth.rays_incoherent(n - n // 2, seed=22)]))


def lists_of(n):
    """(name, ids or None, count): the lists of the issue for a batch of n rays"""
    every = np.arange(n, dtype=np.int64)
    return [("empty", every, 0), ("one ray", np.array([n // 2], np.int64), 1), ("every third", every[::3].copy(), len(every[::3])),
            ("all reversed", every[::-1].copy(), n), ("no ids, half", None, n // 2), ("count beyond the arrays", every[::-1].copy(), n + 1000),
            ("no ids, count beyond the arrays", None, n + 1000)]


def listed_slots(n, ids, count):
    m = min(count, n)
    listed = np.zeros(n, bool)
    listed[np.arange(m) if ids is None else ids[:m]] = True
    return listed


@pytest.fixture(scope="module")
def scene(api):
    tris = synth.scene_for_config(1)
    assert len(tris) == 30000
    half = len(tris) // 2
    return api.DeviceScene.build([dict(positions=tris[:half]), dict(positions=tris[half:])])


class Batch:
    """n rays on the device, the unlisted answers to them, and a filter over them (kept alive here)"""

    def __init__(self, api, ds, n):
        import torch
        self.n = n
        self.rays = some_rays(n)
        self.d_rays = api.to_device(self.rays)
        self.plain = ds.trace_device(self.d_rays, n).cpu().numpy().view(HIT_RECORD_DTYPE)
        self.plain_any = ds.trace_any_device(self.d_rays, n).cpu().numpy()
        # the filter: mesh 0 only, and never the primitive the ray hits first
        self.d_mask = api.to_device(np.array([1], np.uint32))
        self.d_ignore = api.to_device(self.plain["prim"].copy())
        f = api.DevFilter()
        f.struct_size = C.sizeof(api.DevFilter)
        f.d_mesh_mask, f.mesh_mask_bits, f.d_ignore_prim = self.d_mask.data_ptr(), 2, self.d_ignore.data_ptr()
        self.filter = f
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def batches(api, scene):
    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = Batch(api, scene, n)
        return cache[n]
    return get


def unlisted(api, ds, b, any_hit, opts, filtered):
    """what the unlisted call of the same kind writes for the whole ray array"""
    import torch
    L = api.lib()
    out = torch.empty(b.n if any_hit else b.n * 16, dtype=torch.uint8, device="cuda")
    o = C.byref(opts) if opts is not None else None
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if filtered:
        fn = L.rtk_dev_trace_rays_any_filtered if any_hit else L.rtk_dev_trace_rays_filtered
        rc = fn(ds.handle, C.c_void_p(b.d_rays.data_ptr()), b.n, C.c_void_p(out.data_ptr()), C.byref(b.filter), o, stream)
    else:
        fn = L.rtk_dev_trace_rays_any if any_hit else L.rtk_dev_trace_rays
        rc = fn(ds.handle, C.c_void_p(b.d_rays.data_ptr()), b.n, C.c_void_p(out.data_ptr()), o, stream)
    assert rc == 0, api.last_error()
    return out.cpu().numpy()


def check_lists(api, ds, b, any_hit, opts=None, listed_opts=None, filtered=False, names=None):
    """every list of the batch through the listed call: listed slots as the unlisted call, the rest untouched"""
    import torch
    want = unlisted(api, ds, b, any_hit, opts, filtered).reshape(b.n, -1)
    size = want.shape[1]
    for name, ids, count in lists_of(b.n):
        if names is not None and name not in names:
            continue
        d_count = torch.tensor([count], dtype=torch.int64, device="cuda")
        d_ids = torch.from_numpy(ids).cuda() if ids is not None else None
        out = torch.full((b.n * size,), 0x7e, dtype=torch.uint8, device="cuda")
        fn = ds.trace_any_listed_device if any_hit else ds.trace_listed_device
        fn(b.d_rays, b.n, d_count, d_ids, out, filter=b.filter if filtered else None, opts=listed_opts if listed_opts is not None else opts)
        got = out.cpu().numpy().reshape(b.n, size)
        listed = listed_slots(b.n, ids, count)
        assert (got[~listed] == 0x7e).all(), "%s: a slot that is not listed was written" % name
        assert got[listed].tobytes() == want[listed].tobytes(), "%s: a listed slot differs from the unlisted call" % name
    return want


@pytest.mark.parametrize("any_hit", [False, True], ids=["closest", "any"])
@pytest.mark.parametrize("n", SIZES)
def test_listed_slots_equal_the_unlisted_call(api, scene, batches, n, any_hit):
    b = batches(n)
    want = check_lists(api, scene, b, any_hit)
    assert want.tobytes() == (b.plain_any if any_hit else b.plain).tobytes()
    if n >= 5000:
        hit = b.plain["prim"] != NONE
        assert 0.1 < hit.mean() < 1.0


def test_listed_slots_equal_the_oracle(api, oracle, scene, batches):
    """num_rays = 5000, every third ray: bit for bit the oracle's traversal of the exported tree"""
    import torch
    b = batches(5000)
    ids = np.arange(0, 5000, 3, dtype=np.int64)
    out = torch.full((5000 * 16,), 0x7e, dtype=torch.uint8, device="cuda")
    scene.trace_listed_device(b.d_rays, 5000, torch.tensor([len(ids)], dtype=torch.int64, device="cuda"), torch.from_numpy(ids).cuda(), out)
    rec = out.cpu().numpy().view(HIT_RECORD_DTYPE)[ids]
    g_hits, g_mask = oracle.trace(oracle.Blob(scene.export_blob()), b.rays[ids])
    assert ((rec["prim"] != NONE) == g_mask).all() and g_mask.any() and not g_mask.all()
    assert (rec["prim"][g_mask] == scene.mesh_base()[g_hits["mesh_index"][g_mask]] + g_hits["triangle_index"][g_mask]).all()
    for f in ("t", "u", "v"):
        assert (rec[f][g_mask].view(np.uint32) == g_hits[f][g_mask].view(np.uint32)).all(), f
    assert (rec["t"][~g_mask] == b.rays["max_t"][ids][~g_mask]).all()


@pytest.mark.parametrize("any_hit", [False, True], ids=["closest", "any"])
@pytest.mark.parametrize("mode", ["no_asm", "exact_nodes", "filter", "image_hint"])
@pytest.mark.parametrize("n", [5000, 65553])
def test_listed_under_options_and_filters(api, scene, batches, n, mode, any_hit):
    b = batches(n)
    if mode == "no_asm":
        check_lists(api, scene, b, any_hit, opts=api.make_opts(no_asm=True))
    elif mode == "exact_nodes":
        check_lists(api, scene, b, any_hit, opts=api.make_opts(exact_nodes=True))
    elif mode == "filter":
        want = check_lists(api, scene, b, any_hit, filtered=True)
        assert want.tobytes() != (b.plain_any if any_hit else b.plain).tobytes()      # (the filter does something)
    else:
        # an image hint that matches num_rays, with the two flags a listed batch ignores: must change nothing
        w = {5000: (50, 100), 65553: (3, 21851)}[n]
        assert w[0] * w[1] == n
        hint = api.make_opts(image=w, sort_rays=True, static=True)
        check_lists(api, scene, b, any_hit, opts=None, listed_opts=hint)


def test_listed_hint_of_whole_blocks_is_ignored(api, scene):
    """128 x 128 rays with the hint that sends the unlisted call to the packet kernels: the listed call stays per lane and answers alike"""
    import torch
    n = 128 * 128
    rays = synth.rays_pinhole(128, 128)
    d_rays = api.to_device(rays)
    want = scene.trace_device(d_rays, n, opts=api.make_opts(no_packet=True)).cpu().numpy()
    out = torch.full((n * 16,), 0x7e, dtype=torch.uint8, device="cuda")
    scene.trace_listed_device(d_rays, n, torch.tensor([n - 5], dtype=torch.int64, device="cuda"), None, out, opts=api.make_opts(image=(128, 128)))
    got = out.cpu().numpy()
    assert got[:(n - 5) * 16].tobytes() == want[:(n - 5) * 16].tobytes() and (got[(n - 5) * 16:] == 0x7e).all()


def test_listed_on_an_uploaded_cpu_builder_blob(api, oracle):
    """Leaves of 4 to 63 triangles (the CPU task builder's): the assembly kernels hand rays back there, so the caller's list and
    the kernels' own left-over list are both live in one launch."""
    L = api.lib()
    before = L.rtk_amd_get_builder()
    L.rtk_amd_set_builder(1)
    try:
        p, keep = api.build_scene([dict(positions=synth.scene_for_config(1))])
    finally:
        L.rtk_amd_set_builder(before)
    try:
        ds = api.DeviceScene.upload(api.scene_bytes(p))
    finally:
        api.free_scene(p)
    b = Batch(api, ds, 5000)
    for any_hit in (False, True):
        check_lists(api, ds, b, any_hit, names=("every third", "all reversed", "no ids, half", "count beyond the arrays"))
        check_lists(api, ds, b, any_hit, opts=api.make_opts(no_asm=True), names=("every third",))
    assert (b.plain["prim"] != NONE).any()


def test_two_bounces_on_one_stream_without_a_wait(api, scene):
    """trace -> select the hits -> a torch op rewrites the hit slots as shadow rays -> any-hit of the listed slots -> select the
    unoccluded of them, all on a side stream with no synchronise in between; against the same pipeline in numpy from unlisted traces."""
    import torch
    n = 65553
    rays = some_rays(n)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        d_rays = api.to_device(rays)
        rec = scene.trace_device(d_rays, n)
        ids, count = scene.select_rays(rec, api.SELECT_RECORD_HIT, n)
        r = d_rays.view(torch.float32).view(n, 8)
        h = rec.view(torch.float32).view(n, 4)
        hit = rec.view(torch.int32).view(n, 4)[:, 3] != -1
        point = r[:, 0:3] + r[:, 3:6] * h[:, 0:1]
        light = torch.tensor([0.5, 2.0, 0.5], device="cuda")
        shadow = torch.cat([point, light - point, torch.full((n, 1), 1e-3, device="cuda"), torch.full((n, 1), 0.999, device="cuda")], dim=1)
        rays2 = torch.where(hit[:, None], shadow, r).contiguous()
        d_rays2 = rays2.view(torch.uint8).view(-1)
        occ = torch.full((n,), 0x7e, dtype=torch.uint8, device="cuda")
        scene.trace_any_listed_device(d_rays2, n, count, ids, occ)
        ids2, count2 = scene.select_rays(occ, api.SELECT_BYTE_ZERO, n, in_ids=ids, in_count=count)
    side.synchronize()
    # the same in numpy, from unlisted traces of the same arrays
    rec_np = scene.trace(rays, full=False)
    hits = np.nonzero(rec_np["prim"] != NONE)[0]
    rays2_np = rays2.cpu().numpy().view(rays.dtype).reshape(-1)
    occluded = scene.trace_any(rays2_np)
    lit = hits[~occluded[hits]]
    assert int(count.item()) == len(hits) and (ids.cpu().numpy()[:len(hits)] == hits).all()
    occ_np = occ.cpu().numpy()
    assert (occ_np[hits] == occluded[hits]).all() and (np.delete(occ_np, hits) == 0x7e).all()
    assert int(count2.item()) == len(lit) and (ids2.cpu().numpy()[:len(lit)] == lit).all()
    assert 0 < len(lit) < len(hits) < n


def test_refusals(api, scene, batches):
    import torch
    L = api.lib()
    b = batches(256)
    out = torch.empty(256 * 16, dtype=torch.uint8, device="cuda")
    count = torch.tensor([5], dtype=torch.int64, device="cuda")
    rays, outp, stream = C.c_void_p(b.d_rays.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(0)

    def mk(**kw):
        l = api.make_ray_list(count)
        for k, v in kw.items():
            setattr(l, k, v)
        return C.byref(l)

    def refused(rc):
        assert rc == BAD_ARG and api.last_error() != ""

    for fn in (L.rtk_dev_trace_rays_listed, L.rtk_dev_trace_rays_any_listed):
        refused(fn(scene.handle, rays, 256, None, outp, None, None, stream))
        refused(fn(scene.handle, rays, 256, mk(d_count=None), outp, None, None, stream))
        refused(fn(scene.handle, rays, 256, mk(struct_size=16), outp, None, None, stream))
        refused(fn(scene.handle, rays, 256, mk(flags=1), outp, None, None, stream))
        refused(fn(scene.handle, rays, 256, mk(), None, None, None, stream))
        refused(fn(scene.handle, rays, 1 << 32, mk(), outp, None, None, stream))
        refused(fn(None, rays, 256, mk(), outp, None, None, stream))
        assert fn(scene.handle, rays, 0, mk(), outp, None, None, stream) == 0          # nothing to do is not an error
    ids = torch.empty(256, dtype=torch.int64, device="cuda")
    for kind in (4, 0xffffffff):
        refused(L.rtk_dev_select_rays(scene.handle, outp, kind, 256, None, C.c_void_p(ids.data_ptr()), C.c_void_p(count.data_ptr()), stream))
    refused(L.rtk_dev_select_rays(scene.handle, outp, 0, 256, mk(flags=2), C.c_void_p(ids.data_ptr()), C.c_void_p(count.data_ptr()), stream))
    refused(L.rtk_dev_select_rays(scene.handle, outp, 0, 256, None, C.c_void_p(ids.data_ptr()), None, stream))
    torch.cuda.synchronize()
    assert int(count.item()) == 5
