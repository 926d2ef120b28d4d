"""numpy model of a BVH refit (include/nanort_hip.h, nrtRefit*): the same node array with every REACHABLE record's box
recomputed bottom-up from new vertex positions.  A leaf's box is the min / max over every coordinate of its triangles (an
empty leaf: {+max, -max}); a branch's box is the min / max of its two children's.  flag / axis / data and records the walk
from the root never reaches are kept as they are.  Boxes compare numerically (-0 == +0)."""
import numpy as np


def xyz(verts):
    """[nv, k >= 3] (strided rows) or flat xyz -> [nv, 3]."""
    v = np.asarray(verts)
    return v.reshape(-1, 3) if v.ndim == 1 else v[:, :3]


def tri_boxes(verts, faces):
    p = xyz(verts)[np.asarray(faces, dtype=np.int64)]  # [nf, 3 vertices, 3 coords]
    return p.min(axis=1), p.max(axis=1)


def levels(nodes):
    """Reachable records by depth: [array of node ids at depth 0, 1, ...]."""
    out = [np.array([0], dtype=np.int64)]
    while True:
        cur = out[-1]
        br = cur[nodes["flag"][cur] == 0]
        if br.size == 0:
            return out
        out.append(np.concatenate([nodes["data"][br, 0], nodes["data"][br, 1]]).astype(np.int64))


def refit(nodes, indices, verts, faces):
    """The refit node array (a copy)."""
    out = nodes.copy()
    real = out["bmin"].dtype
    big = np.finfo(real).max
    lo_t, hi_t = tri_boxes(verts, faces)
    lo_s = lo_t[np.asarray(indices, dtype=np.int64)]  # per slot
    hi_s = hi_t[np.asarray(indices, dtype=np.int64)]
    lv = levels(nodes)
    reach = np.concatenate(lv)
    leaves = reach[nodes["flag"][reach] != 0]
    cnt = nodes["data"][leaves, 0].astype(np.int64)
    first = nodes["data"][leaves, 1].astype(np.int64)
    lo = np.full((leaves.size, 3), big, dtype=real)
    hi = np.full((leaves.size, 3), -big, dtype=real)
    ne = cnt > 0
    if ne.any():
        # per-leaf reduction over its slot range (ranges of a tree may overlap or leave gaps: reduce each one on its own)
        seg = np.repeat(np.nonzero(ne)[0], cnt[ne])
        c = cnt[ne]
        slot = np.repeat(first[ne], c) + (np.arange(c.sum()) - np.repeat(np.cumsum(c) - c, c))
        np.minimum.at(lo, seg, lo_s[slot])
        np.maximum.at(hi, seg, hi_s[slot])
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


def brute_boxes(nodes, indices, verts, faces):
    """Every reachable record's box by brute force over the slots of its subtree: {id: (lo, hi)}."""
    real = nodes["bmin"].dtype
    big = np.finfo(real).max
    lo_t, hi_t = tri_boxes(verts, faces)
    out = {}

    def slots(i):
        st, acc = [i], []
        while st:
            k = st.pop()
            n = nodes[k]
            if n["flag"] == 0:
                st += [int(n["data"][0]), int(n["data"][1])]
            else:
                acc.append(np.arange(int(n["data"][1]), int(n["data"][1]) + int(n["data"][0])))
        return np.concatenate(acc) if acc else np.zeros(0, dtype=np.int64)

    for i in np.concatenate(levels(nodes)):
        s = slots(int(i))
        p = np.asarray(indices, dtype=np.int64)[s]
        if p.size == 0:
            out[int(i)] = (np.full(3, big, real), np.full(3, -big, real))
        else:
            out[int(i)] = (lo_t[p].min(axis=0), hi_t[p].max(axis=0))
    return out


def topology_bytes(nodes):
    """flag, axis and data of every record."""
    return b"".join(np.ascontiguousarray(nodes[k]).tobytes() for k in ("flag", "axis", "data"))


def assert_boxes_equal(a, b, what="boxes"):
    """Numeric equality of every record's box (-0 == +0)."""
    bad = np.nonzero(~(np.all(a["bmin"] == b["bmin"], axis=1) & np.all(a["bmax"] == b["bmax"], axis=1)))[0]
    assert bad.size == 0, "%s differ at %d records, first %s:\n%s\n%s" % (what, bad.size, bad[:4], a[bad[:4]], b[bad[:4]])
