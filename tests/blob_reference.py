"""An independent check of a scene blob in numpy and Python alone: what rtk_dev_scene_validate counts, as
far as it has a definition that does not depend on the code. Imports nothing from oracle/ or from the library.

Layout read here: root node at byte 128; a node is 24 floats (bounds_x[min|max][slot], bounds_y, bounds_z) and four 64-bit child
words at byte 96 (bit 0: leaf at word ^ 1, else the byte offset of a node); a leaf is a 64-bit word (low 6 bits: count, the rest:
byte offset of its vertex group), then count records of 8 bytes (three vertex numbers, local mesh, triangle index), padded to a
multiple of four, then the table local mesh -> mesh; a vertex is 16 bytes, three floats first.

Rules:
  * a slot whose box is inverted on some axis (NaN included) is EMPTY, as the blob's readers take it; an empty slot must carry
    exactly +1 / -1 on all three axes, anything else is a box violation at that node;
  * nodes are numbered breadth-first from the root, slots in order, as the loader numbers them;
  * a child box CONTAINS when min <= union min and max >= union max on every axis, and is EXACT when all six are equal (float32
    compares); the union below a leaf child is its triangles' vertices, below an inner child the non-empty child boxes stored
    in that child node; a box that does not contain is a violation, one that contains and is not exact is loose;
  * first_bad_index: the smallest node number with a violation (None: none);
  * node_refs / leaf_refs: how often each node or leaf is referenced from a non-empty slot, the entry at the root counting as one;
    `shared` counts those referenced more than once; a leaf reached twice gives its records twice; a word that points outside the
    blob (or at a misaligned node) is counted in out_of_range and not followed;
  * leaf_count_errors: a non-empty slot whose leaf has a count outside 1..63 (0 among them); its records are not read;
  * primitive id of a record: the sum of the sizes of the meshes before its mesh (size = largest triangle index + 1) + index."""
import numpy as np


def check(blob_bytes):
    b = np.frombuffer(bytes(blob_bytes), np.uint8)
    size = len(b)

    def u64(at):
        return int(b[at:at + 8].view("<u8")[0])

    out = dict(nodes=0, leaves=0, triangles=0, box_violations=0, loose_boxes=0, bad_empty_slots=0, leaf_count_errors=0,
               out_of_range=0, first_bad_index=None, node_refs={128: 1}, leaf_refs={}, records=[])   # (the root: entered once)

    def bad(i):
        out["box_violations"] += 1
        if out["first_bad_index"] is None or i < out["first_bad_index"]:
            out["first_bad_index"] = i

    def node_at(off):
        box = b[off:off + 96].view("<f4").reshape(3, 2, 4)
        words = [u64(off + 96 + 8 * k) for k in range(4)]
        live = [k for k in range(4) if all(box[a, 0, k] <= box[a, 1, k] for a in range(3))]
        return box, words, live

    def leaf_union(off):
        """(count, min[3], max[3], [(mesh, triangle index)]) of the leaf at off"""
        info = u64(off)
        cnt, vg = info & 63, info & ~63
        n4 = (cnt + 3) & ~3
        table = off + 8 + 8 * n4
        pts, recs = [], []
        for t in range(cnt):
            r = b[off + 8 + 8 * t:off + 16 + 8 * t]
            for c in range(3):
                at = vg + 16 * int(r[c])
                pts.append(b[at:at + 12].view("<f4"))
            mesh = int(b[table + 4 * int(r[3]):table + 4 * int(r[3]) + 4].view("<u4")[0])
            recs.append((mesh, int(r[4:8].view("<u4")[0])))
        if not pts:
            return cnt, None, None, recs
        p = np.stack(pts)
        with np.errstate(all="ignore"):
            return cnt, np.fmin.reduce(p, axis=0), np.fmax.reduce(p, axis=0), recs

    order, index = [128], {128: 0}
    qi = 0
    while qi < len(order):
        off = order[qi]
        i = qi
        qi += 1
        out["nodes"] += 1
        box, words, live = node_at(off)
        for k in range(4):
            mn, mx = box[:, 0, k], box[:, 1, k]
            if k not in live:
                if not ((mn == 1.0).all() and (mx == -1.0).all()):
                    out["bad_empty_slots"] += 1
                    bad(i)
                continue
            p = words[k]
            if p & 1:
                lo = p ^ 1
                if lo < 128 or lo + 8 > size:
                    out["out_of_range"] += 1
                    continue
                out["leaf_refs"][lo] = out["leaf_refs"].get(lo, 0) + 1
                try:
                    cnt, cmn, cmx, recs = leaf_union(lo)
                except (IndexError, ValueError):                  # a record, table entry or vertex outside the blob
                    out["out_of_range"] += 1
                    continue
                if not 1 <= cnt <= 63:
                    out["leaf_count_errors"] += 1
                    continue
                out["leaves"] += 1
                out["triangles"] += cnt
                out["records"] += recs
            else:
                if p < 128 or p & 127 or p + 128 > size:
                    out["out_of_range"] += 1
                    continue
                out["node_refs"][p] = out["node_refs"].get(p, 0) + 1
                if p in index:                                    # reached twice: counted, walked once
                    continue
                index[p] = len(order)
                order.append(p)
                cbox, _, clive = node_at(p)
                if not clive:
                    cmn, cmx = np.full(3, np.inf, np.float32), np.full(3, -np.inf, np.float32)
                else:
                    cmn, cmx = cbox[:, 0, clive].min(axis=1), cbox[:, 1, clive].max(axis=1)
            contains = bool((mn <= cmn).all() and (mx >= cmx).all())
            exact = bool((mn == cmn).all() and (mx == cmx).all())
            if not contains:
                bad(i)
            elif not exact:
                out["loose_boxes"] += 1
    # primitive ids, as the loader numbers them
    sizes = {}
    for mesh, tri in out["records"]:
        sizes[mesh] = max(sizes.get(mesh, 0), tri + 1)
    base, run = {}, 0
    for mesh in range(max(sizes) + 1 if sizes else 0):
        base[mesh] = run
        run += sizes.get(mesh, 0)
    counts = np.zeros(run, np.int64)
    for mesh, tri in out["records"]:
        counts[base[mesh] + tri] += 1
    out["prim_counts"] = counts
    out["shared"] = sum(1 for v in list(out["node_refs"].values()) + list(out["leaf_refs"].values()) if v > 1)
    out["clean"] = (out["box_violations"] == 0 and out["leaf_count_errors"] == 0 and out["out_of_range"] == 0 and out["shared"] == 0
                    and bool((counts == 1).all()))
    return out
