"""numpy model of a sphere / curve refit (include/nanort_hip.h, nrtRefitPrims*): the per-primitive boxes by the two rules of the
builder (nanort_amd/csrc/prims_dev.h) in float32 — sphere: centre -/+ radius; curve: min / max over the four `control point -/+
its radius` — then the bottom-up pass of tests/refit_model.py: a leaf's box is the min / max over its slots (an empty leaf:
{+max, -max}), a branch's the min / max of its two children's, and flag / axis / data and unreachable records stay as they are."""
import numpy as np

from refit_model import assert_boxes_equal, levels, topology_bytes  # noqa: F401  (the tests take all three from here)

F32 = np.float32


def sphere_boxes(centers, radii):
    c = np.asarray(centers, dtype=F32).reshape(-1, 3)
    r = np.asarray(radii, dtype=F32).reshape(-1, 1)
    return c - r, c + r  # (float32 - float32: one rounding, as the device's)


def curve_boxes(cps, radii):
    p = np.asarray(cps, dtype=F32).reshape(-1, 4, 3)
    r = np.asarray(radii, dtype=F32).reshape(-1, 4, 1)
    return (p - r).min(axis=1), (p + r).max(axis=1)


def prim_boxes(kind, positions, radii):
    return {"spheres": sphere_boxes, "curves": curve_boxes}[kind](positions, radii)


def refit_boxes(nodes, indices, lo_p, hi_p):
    """The refit node array (a copy) from per-primitive boxes."""
    out = nodes.copy()
    big = np.finfo(F32).max
    idx = np.asarray(indices, dtype=np.int64)
    lv = levels(nodes)
    reach = np.concatenate(lv)
    leaves = reach[nodes["flag"][reach] != 0]
    cnt = nodes["data"][leaves, 0].astype(np.int64)
    first = nodes["data"][leaves, 1].astype(np.int64)
    lo = np.full((leaves.size, 3), big, dtype=F32)
    hi = np.full((leaves.size, 3), -big, dtype=F32)
    ne = cnt > 0
    if ne.any():  # per-leaf reduction over its slot range, every range on its own (as refit_model.refit: 300 000 leaves in a second)
        c = cnt[ne]
        seg = np.repeat(np.nonzero(ne)[0], c)
        slot = np.repeat(first[ne], c) + (np.arange(c.sum()) - np.repeat(np.cumsum(c) - c, c))
        np.minimum.at(lo, seg, lo_p[idx[slot]])
        np.maximum.at(hi, seg, hi_p[idx[slot]])
    out["bmin"][leaves] = lo
    out["bmax"][leaves] = hi
    for lvl in reversed(lv):
        br = lvl[nodes["flag"][lvl] == 0]
        if br.size == 0:
            continue
        a, b = nodes["data"][br, 0], nodes["data"][br, 1]
        out["bmin"][br] = np.minimum(out["bmin"][a], out["bmin"][b])
        out["bmax"][br] = np.maximum(out["bmax"][a], out["bmax"][b])
    return out


def refit(kind, nodes, indices, positions, radii):
    lo, hi = prim_boxes(kind, positions, radii)
    return refit_boxes(nodes, indices, lo, hi)


def brute_boxes(nodes, indices, lo_p, hi_p):
    """Every reachable record's box by brute force over the slots of its subtree: {id: (lo, hi)}."""
    big = np.finfo(F32).max
    idx = np.asarray(indices, dtype=np.int64)
    out = {}
    for i in np.concatenate(levels(nodes)):
        st, prims = [int(i)], []
        while st:
            n = nodes[st.pop()]
            if n["flag"] == 0:
                st += [int(n["data"][0]), int(n["data"][1])]
            else:
                prims += idx[int(n["data"][1]):int(n["data"][1]) + int(n["data"][0])].tolist()
        if prims:
            out[int(i)] = (lo_p[prims].min(axis=0), hi_p[prims].max(axis=0))
        else:
            out[int(i)] = (np.full(3, big, F32), np.full(3, -big, F32))
    return out
