"""tests/many_passes.py on the CPU: the batch size against every residency, the tiling of every family's reference against that
family's brute force run on the repeated batch itself, and the three conditions that make stale per-step state visible."""
import numpy as np
import pytest

from tests import many_passes as M

CUS = 256                                    # an MI355X; the properties of the batch size are asserted for other counts too


@pytest.mark.parametrize("cus", [1, 8, 64, 104, 228, 256, 304, 997])
def test_batch_size(cus):
    assert M.LANES_PER_CU == 2048 and M.BLOCK * max(M.RESIDENCIES) == M.LANES_PER_CU and list(M.RESIDENCIES) == list(range(1, 9))
    N = M.batch_size(cus)
    assert N % 64 != 0 and N < 1 << 31
    for s in M.pass_sizes(cus):
        assert s <= M.LANES_PER_CU * cus
        assert N >= 2 * s + 64 * 5 + 37 and N % s != 0               # two whole passes and a ragged one behind them
    L = M.mix_length(cus)
    assert 900 < L <= 1000 and all(L % k for k in range(2, L)) and cus % L and all(s % L for s in M.pass_sizes(cus))
    assert L * 300 <= 500000


def test_batch_size_of_256_cus():
    assert M.batch_size(256) == 1048933 and M.mix_length(256) == 997


def repeated(name, f, n, chunk=1500):
    """the family's brute force on the repeated batch itself, in pieces that stay under the pair limit and do not line up with L"""
    inputs = tuple(M.tile_rows(x, n) for x in f.inputs)
    parts = [M.brute(name, f.tris, tuple(x[k:k + chunk] for x in inputs)) for k in range(0, n, chunk)]
    rows = tuple(np.concatenate([p.rows[j] for p in parts]) for j in range(len(parts[0].rows)))
    counts = np.concatenate([p.counts for p in parts]) if parts[0].counts is not None else None
    fills = tuple(np.concatenate([p.fills[j] for p in parts]) for j in range(len(parts[0].fills)))
    return rows, counts, fills


@pytest.mark.parametrize("name", M.FAMILIES)
def test_the_tiled_reference_is_the_brute_force_of_the_repeated_batch(name):
    f = M.family(name, CUS)
    n = 3 * f.L + 17
    rows, counts, fills = repeated(name, f, n)
    for want, mix in zip(rows, f.answer.rows):
        assert M.tile_rows(mix, n).tobytes() == want.tobytes()
        assert M.slots(mix, n, 5)[:n].tobytes() == want.tobytes() and (M.slots(mix, n, 5)[n:] == M.FILL).all()
    if counts is None:
        assert name in M.CLOSEST and not fills
        return
    assert name in M.COUNTED
    t = M.Tiled(f.answer.counts, n)
    assert t.counts.tobytes() == counts.astype(np.int64).tobytes()
    assert t.offsets.tobytes() == np.concatenate([[0], np.cumsum(counts.astype(np.int64))]).tobytes() and t.total == int(counts.sum())
    assert t.total % t.period != 0                                   # (the buffers end in a partial period)
    assert t.written(5)[:n].tobytes() == counts.astype(np.uint32).tobytes() and (t.written(5)[n:] == M.FILL).all()
    for want, period in zip(fills, f.answer.fills):
        got = t.fill(period, 5)
        assert got[:t.total].tobytes() == want.tobytes() and (got[t.total:] == M.FILL).all()
    # a list: the segments of the slots that are not listed stay 0x7e
    listed = np.random.RandomState(1).uniform(0, 1, n) < 0.6
    got = t.fill(f.answer.fills[0], 5, listed)
    want = np.full_like(got, M.FILL)
    for i in np.nonzero(listed)[0]:
        want[t.offsets[i]:t.offsets[i + 1]] = fills[0][t.offsets[i]:t.offsets[i + 1]]
    assert got.tobytes() == want.tobytes() and (t.written(5, listed)[:n][~listed] == M.FILL).all()


@pytest.mark.parametrize("name", M.FAMILIES)
def test_the_mix_makes_stale_state_visible(name):
    f = M.family(name, CUS)
    assert len(f.inputs[0]) == f.L == M.mix_length(CUS) and f.L * len(f.tris) <= 500000 and len(f.tris) == 300
    M.conditions(name, f.answer.live, f.answer.key, CUS)
    if f.answer.counts is not None:
        print("%s: a fill of %d slots holds %d entries" % (name, M.batch_size(CUS), M.Tiled(f.answer.counts, M.batch_size(CUS)).total))
        assert M.Tiled(f.answer.counts, M.batch_size(CUS)).total < 16 << 20


def test_the_all_hits_mix(oracle):
    """All hits is answered by the oracle, not by numpy: its mix is made here on the blob the oracle's own builder makes of the
    soup (the GPU test makes it on the blob its scene exports; the candidates of a ray are the triangles it meets, whatever
    the tree). The tiling of its lists is checked like the other fill forms'."""
    from tests import allhits_ref as R
    blob = oracle.build_scene([dict(positions=M.soup())])
    rays, want = M.allhits_mix(oracle, blob, [0], CUS)
    assert len(rays) == M.mix_length(CUS)
    M.conditions("all hits", np.ones(len(rays), bool), want.counts, CUS)
    assert want.counts.max() >= 2
    n = 3 * len(rays) + 17
    again = R.oracle_lists(oracle, blob, M.tile_rows(rays, n), [0])
    t = M.Tiled(want.counts, n)
    assert t.offsets.tobytes() == again.offsets.astype(np.int64).tobytes()
    assert t.fill(want.records.view(np.uint32).reshape(-1, 4)).tobytes() == again.records.tobytes()


def test_the_winding_mix():
    """Winding numbers have no hit or miss: the conditions become that the float32 sum is within the ceiling of
    tests/test_gpu_winding.py, and that at every pass size a quarter of the positions differ from the one a pass on by more
    than that ceiling. (The world mixes are answered per instance on the device: tests/test_gpu_many_passes.py asserts their
    conditions, from that reference alone, before it compares.)"""
    pts, w64, rule = M.winding_mix(CUS)
    assert len(pts) == M.mix_length(CUS) and rule <= 1e-3
    L = len(pts)
    differ = [float((np.abs(w64 - w64[(np.arange(L) + s) % L]) > 1e-3).mean()) for s in M.pass_sizes(CUS)]
    print("winding: L %d, brute32 against float64 %.3e, steps that differ %.0f .. %.0f %%, values %.3f .. %.3f" % (L, rule, 100 * min(differ), 100 * max(differ), w64.min(), w64.max()))
    assert min(differ) >= 0.25


def test_cut_raises_where_no_cut_can_differ():
    with pytest.raises(AssertionError):
        M.cut(np.ones(1200, np.int64), 997, CUS)                     # (every query hits once: no two steps differ)


def test_deep_mix():
    deep, shallow = np.arange(10, 15), np.arange(100, 103)
    got = M.deep_mix(deep, shallow, 23)
    assert got[::7].tolist() == [10, 11, 12, 13] and (np.delete(got, np.arange(0, 23, 7)) >= 100).all() and len(got) == 23
