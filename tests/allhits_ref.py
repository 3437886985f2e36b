"""Fixtures and the reference of the all-hits tests (tests/test_allhits_cpu.py, tests/test_gpu_allhits.py).

The reference is the oracle alone: oracle.pyoracle.trace_filtered on a blob with a callback that records every candidate it is
offered and rejects it. A traversal that never accepts anything keeps its far bound at the ray's max_t and offers every candidate
of the ray exactly once; sorted by (t, prim) that is the list rtk_dev_trace_rays_all writes. The callback forces one thread: cases
stay at a few thousand rays."""
import numpy as np

from rtk_amd.types import HIT_RECORD_DTYPE, RAY_DTYPE, RTK_INF

NONE = 0xFFFFFFFF


class Lists:
    """counts uint32[n], offsets int64[n + 1], records HIT_RECORD_DTYPE[offsets[n]] in (t, prim) order per ray"""

    def __init__(self, per_ray):
        self.counts = np.array([len(l) for l in per_ray], np.uint32)
        self.offsets = np.zeros(len(per_ray) + 1, np.int64)
        np.cumsum(self.counts, out=self.offsets[1:])
        self.records = np.zeros(int(self.offsets[-1]), HIT_RECORD_DTYPE)
        k = 0
        for l in per_ray:
            for t, prim, u, v in sorted(l, key=lambda c: (float(c[0]), c[1])):
                self.records[k] = (t, u, v, prim)
                k += 1

    def of(self, i):
        return self.records[self.offsets[i]:self.offsets[i + 1]]

    def first(self, room):
        """what a fill with `room[i]` records of room for ray i keeps: (offsets, records, written)"""
        room = np.broadcast_to(np.asarray(room, np.int64), self.counts.shape)
        off = np.zeros(len(room) + 1, np.int64)
        np.cumsum(room, out=off[1:])
        written = np.minimum(self.counts.astype(np.int64), room)
        rec = [self.of(i)[:written[i]] for i in range(len(room))]
        return off, rec, written.astype(np.uint32)


def split_prims(mesh_base, prims):
    """global primitive ids -> (mesh, triangle) as the oracle's filters take them; NONE stays (NONE, 0)"""
    prims = np.asarray(prims, np.uint32)
    base = np.asarray(mesh_base, np.int64)
    ok = prims != NONE
    mesh = np.searchsorted(base, np.where(ok, prims, 0).astype(np.int64), side="right") - 1
    tri = np.where(ok, prims, 0).astype(np.int64) - base[mesh]
    return np.where(ok, mesh, NONE).astype(np.uint32), np.where(ok, tri, 0).astype(np.uint32)


def oracle_lists(oracle, blob, rays, mesh_base, mesh_mask=None, ignore_prim=None, after=None):
    """Every candidate of every ray as the oracle's reject-all callback is offered them. ignore_prim: uint32[n] global ids;
    after: HIT_RECORD_DTYPE[n] (prim NONE = off), as the device takes them."""
    rays = np.ascontiguousarray(rays)
    base = [int(b) for b in mesh_base]
    got = [[] for _ in range(len(rays))]

    def reject(i, h):
        got[i].append((np.float32(h["t"]), base[int(h["mesh_index"])] + int(h["triangle_index"]), np.float32(h["u"]), np.float32(h["v"])))
        return False
    ignore = split_prims(mesh_base, ignore_prim) if ignore_prim is not None else None
    aft = None
    if after is not None:
        am, at = split_prims(mesh_base, after["prim"])
        aft = (np.ascontiguousarray(after["t"], np.float32), am, at)
    if len(rays):
        oracle.trace_filtered(blob, rays, mesh_mask=mesh_mask, ignore=ignore, after=aft, callback=reject)
    return Lists(got)


def make_rays(origin, direction, min_t=0.0, max_t=RTK_INF):
    origin = np.asarray(origin, np.float32).reshape(-1, 3)
    r = np.zeros(len(origin), RAY_DTYPE)
    r["origin"] = origin
    r["direction"] = np.broadcast_to(np.asarray(direction, np.float32), origin.shape)
    r["min_t"] = min_t
    r["max_t"] = max_t
    return r


# ---- case 1: 24 parallel unit squares z = 0.25 k, two triangles each (split along the diagonal (0,0)-(1,1)), three meshes of eight
SHEETS = 24


def sheets_meshes():
    meshes = []
    for m in range(3):
        t = []
        for k in range(8 * m, 8 * m + 8):
            z = np.float32(0.25 * k)
            a, b, c, d = (0, 0, z), (1, 0, z), (1, 1, z), (0, 1, z)
            t += [a, b, c, a, c, d]
        meshes.append(dict(positions=np.array(t, np.float32)))
    return meshes


def sheets_rays():
    """960 perpendicular rays through generic points (24 crossings each, strictly inside one triangle of every square) and 64 aimed
    exactly at the squares' shared diagonal and corners (exactly-zero edge functions): 1,024. Returns (rays, generic mask)."""
    rng = np.random.RandomState(11)
    xy = rng.uniform(0.05, 0.95, (960, 2)).astype(np.float32)
    xy[np.abs(xy[:, 0] - xy[:, 1]) < 1e-3, 0] += np.float32(0.01)          # off the diagonal
    gen = make_rays(np.concatenate([xy, np.full((960, 1), -1.0, np.float32)], 1), (0, 0, 1))
    gen["direction"][480:] = (0, 0, -1)                                   # half of them from the other side
    gen["origin"][480:, 2] = 7.0
    d = (np.arange(1, 57, dtype=np.float32) / np.float32(64.0))          # on the diagonal: x == y, exactly representable
    diag = make_rays(np.stack([d, d, np.full_like(d, -1.0)], 1), (0, 0, 1))
    corners = np.array([(0, 0), (1, 1), (1, 0), (0, 1)], np.float32)
    up = make_rays(np.concatenate([corners, np.full((4, 1), -1.0, np.float32)], 1), (0, 0, 1))
    down = make_rays(np.concatenate([corners, np.full((4, 1), 7.0, np.float32)], 1), (0, 0, -1))
    rays = np.concatenate([gen, diag, up, down])
    generic = np.zeros(len(rays), bool)
    generic[:960] = True
    return np.ascontiguousarray(rays), generic


# ---- case 2: 3,000 random triangles in three meshes, 4,097 random rays through their box
def soup_meshes(n=3000, spread=0.12, seed=21):
    from rtk_amd import synth
    p = synth.triangle_soup(n, spread, seed=seed).reshape(n, 9)
    return [dict(positions=np.ascontiguousarray(p[a:b].reshape(-1, 3))) for a, b in ((0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n))]


def soup_rays(n=4097, seed=23):
    from rtk_amd import synth
    r = synth.rays_incoherent(n, seed=seed)
    r["max_t"] = RTK_INF
    return np.ascontiguousarray(r)


# ---- case 10: a closed box, 12 triangles
BOX_LO, BOX_HI = np.float32([0.2, 0.3, 0.1]), np.float32([0.9, 0.8, 0.7])


def box_mesh():
    lo, hi = BOX_LO, BOX_HI
    c = np.array([[x, y, z] for z in (lo[2], hi[2]) for y in (lo[1], hi[1]) for x in (lo[0], hi[0])], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    t = []
    for a, b, cc, d in quads:
        t += [c[a], c[b], c[cc], c[a], c[cc], c[d]]
    return [dict(positions=np.array(t, np.float32))]


def box_points(n=512, seed=31):
    """generic points in [0, 1]^3, none within 1e-3 of a face plane; returns (points, inside)"""
    rng = np.random.RandomState(seed)
    p = rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32)
    for ax in range(3):
        for plane in (BOX_LO[ax], BOX_HI[ax]):
            near = np.abs(p[:, ax] - plane) < 1e-3
            p[near, ax] += np.float32(0.01)
    inside = ((p > BOX_LO) & (p < BOX_HI)).all(1)
    return p, inside


CONTAINS_DIRECTION = (0.5458, 0.3207, 0.7743)
