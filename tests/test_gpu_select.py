"""GPU tests of rtk_dev_select_rays: the stable compaction that makes a ray list from a trace's output, against numpy.nonzero.

Sizes: around a wave, around what one workgroup of the count / scatter kernels covers and around what one workgroup of the scan
level covers (both asked of the library, not written down here), and 2^20 + 3, where the top level has more than one group to
add up. Keep rates 0, 1, about 1/2 and about 1/1000; all four kinds; with and without an input list (a shuffled subset, whose
order the output keeps)."""
import ctypes as C

import numpy as np
import pytest

from rtk_amd.types import HIT_RECORD_DTYPE

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
RATES = [0.0, 1.0, 0.5, 0.001]


@pytest.fixture(scope="module")
def scene(api):
    from rtk_amd import synth
    return api.DeviceScene.build([dict(positions=synth.triangle_soup(64, 0.2, 3))])


@pytest.fixture(scope="module")
def sizes(api):
    block, scan = api.lib().rtk_amd_select_block_items(), api.lib().rtk_amd_select_scan_items()
    assert 64 < block < scan
    return [0, 1, 63, 64, 65, block - 1, block, block + 1, scan - 1, scan, scan + 1, (1 << 20) + 3]


def source(kind, n, rate, seed):
    """(device bytes, flags as numpy bool): hit records or bytes of which about `rate` match `kind`"""
    rng = np.random.default_rng(seed)
    match = rng.random(n) < rate if 0.0 < rate < 1.0 else np.full(n, rate == 1.0)
    if n > 2 and 0.0 < rate < 1.0:
        match[0], match[n - 1] = True, False         # (both ends take part whatever the draw)
    if kind < 2:
        rec = np.zeros(n, HIT_RECORD_DTYPE)
        rec["t"] = rng.random(n, dtype=np.float32)
        is_hit = match if kind == 0 else ~match
        rec["prim"] = np.where(is_hit, rng.integers(0, 1000, n).astype(np.uint32), np.uint32(NONE))
        return rec.view(np.uint8).reshape(-1), match
    is_set = match if kind == 2 else ~match
    return np.where(is_set, rng.integers(1, 256, n), 0).astype(np.uint8), match


def run(api, scene, src_np, kind, n, in_ids=None, in_count=None):
    """-> (count, all num_rays entries of the output, which was filled with -2)"""
    import torch
    L = api.lib()
    src = torch.from_numpy(np.ascontiguousarray(src_np)).cuda() if len(src_np) else torch.zeros(16, dtype=torch.uint8, device="cuda")
    ids = torch.full((max(n, 1),), -2, dtype=torch.int64, device="cuda")
    count = torch.full((1,), -2, dtype=torch.int64, device="cuda")
    l = None
    keep = []
    if in_ids is not None:
        keep = [torch.from_numpy(in_ids).cuda(), torch.tensor([in_count], dtype=torch.int64, device="cuda")]
        l = C.byref(api.make_ray_list(keep[1], keep[0]))
    rc = L.rtk_dev_select_rays(scene.handle, C.c_void_p(src.data_ptr()), kind, n, l, C.c_void_p(ids.data_ptr()), C.c_void_p(count.data_ptr()),
                               C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, api.last_error()
    return int(count.cpu().item()), ids.cpu().numpy()


@pytest.mark.parametrize("kind", [0, 1, 2, 3], ids=["record_hit", "record_miss", "byte_nonzero", "byte_zero"])
def test_select_equals_nonzero(api, scene, sizes, kind):
    for n in sizes:
        for rate in RATES:
            src, match = source(kind, n, rate, seed=n * 7 + kind)
            want = np.nonzero(match)[0]
            count, ids = run(api, scene, src, kind, n)
            assert count == len(want), (n, rate)
            assert (ids[:count] == want).all(), (n, rate)
            assert (ids[count:] == -2).all(), "entries beyond the count were written (n %d, rate %g)" % (n, rate)
            if n == sizes[-1] and rate == 0.5:
                again = run(api, scene, src, kind, n)          # two runs: equal bytes
                assert again[0] == count and again[1].tobytes() == ids.tobytes()


@pytest.mark.parametrize("kind", [0, 3], ids=["record_hit", "byte_zero"])
def test_select_from_a_list_keeps_its_order(api, scene, sizes, kind):
    """The input list: a shuffled subset of the rays (about two thirds of them), of which only the first in_count entries count."""
    for n in [s for s in sizes if s > 0]:
        for rate in (0.5, 0.001):
            src, match = source(kind, n, rate, seed=n * 11 + kind)
            rng = np.random.default_rng(n)
            subset = rng.permutation(n)[:max(1, (2 * n) // 3)].astype(np.int64)
            for in_count in sorted({0, len(subset) // 2, len(subset), n + 77}):
                if in_count > len(subset) and len(subset) < n:
                    continue                                     # (a list holds at least the entries that count)
                m = min(in_count, n)
                want = subset[:m][match[subset[:m]]]
                # upper halves of the ids are not read
                count, ids = run(api, scene, src, kind, n, in_ids=subset | (np.int64(5) << np.int64(40)), in_count=in_count)
                assert count == len(want) and (ids[:count] == want).all(), (n, rate, in_count)
                assert (ids[count:] == -2).all()


def test_select_from_the_whole_list_with_a_count_beyond_it(api, scene):
    n = 5000
    src, match = source(2, n, 0.5, seed=1)
    order = np.random.default_rng(2).permutation(n).astype(np.int64)
    count, ids = run(api, scene, src, 2, n, in_ids=order, in_count=n + 1000)
    want = order[match[order]]
    assert count == len(want) and (ids[:count] == want).all()


def test_two_streams_at_once(api, scene, sizes):
    """Selects of different batches on two streams of one scene, interleaved: each stream has a scratch set of its own."""
    import torch
    n = sizes[-1]
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    jobs = []
    for k, s in enumerate((a, b, a, b, a, b)):
        src_np, match = source(2 + (k & 1), n - k * 1000, 0.5, seed=100 + k)
        with torch.cuda.stream(s):
            src = torch.from_numpy(src_np).cuda()
        jobs.append((s, src, match, n - k * 1000, 2 + (k & 1)))
    torch.cuda.synchronize()
    outs = []
    for _ in range(3):
        for s, src, match, m, kind in jobs:
            with torch.cuda.stream(s):
                outs.append((scene.select_rays(src, kind, m), match))
    torch.cuda.synchronize()
    for (ids, count), match in outs:
        want = np.nonzero(match)[0]
        assert int(count.item()) == len(want) and (ids.cpu().numpy()[:len(want)] == want).all()
