"""numpy model of the GPU builder's split rule (nanort_amd/csrc/build_dev.h, eval_split in build.hip, build_subtree.hip):
the tree the stated rule gives, byte for byte.  `T` is the build's precision; every operation below is rounded to T, no
fused multiply-add, IEEE divide, denormals kept (the library is built that way), so numpy reproduces the arithmetic exactly.

Records.  Per primitive a box and a centre, as prim_box_axis (prims_dev.h) gives them for each kind.  Triangles:
min(p0, min(p1, p2)), the same for max, centre ((p0 + p1) + p2) * (T(1) / T(3)).  Spheres: c -/+ r, centre c.  Cylinders: over
the whole cylinder, min(a1 - r1, a0 - r0) and max(a1 + r1, a0 + r0), centre (a0 + a1) / 2.  Curves: control point -/+ its own
radius, centre (((p0 + p1) + p2) + p3) / 4.  The initial order is primitive order 0..n-1.

Leaf.  A node is a leaf when depth >= max_tree_depth or n <= max(min_leaf_primitives, 1).  The root has depth 0.

Bins.  K0 = clamp(bin_size, 2, 64).  A node of n <= 256 primitives uses min(K0, 16) bins, a larger node K0.  Bins span the
node's centre bounds, the exact min and max of its primitives' centres.  Per axis, scale = T(K) / ext when ext > 0, else 0;
bin = clamp((int)((c - lo) * scale), 0, K - 1).  The conversion is the GPU's: it truncates, a NaN gives 0 and a value too
large gives the top bin (scale overflows to infinity over a denormal extent: 0 * inf is the NaN, the rest of the node lands
in the top bin).

Cut search.  Per axis, each bin's count and the union box of its primitives.  The candidates are s = 1..K-1, the low side is
bins < s.  cost = T(nl) * ha(L) + T(nr) * ha(R), ha(e) = (a*b + b*c) + c*a over the extents max - min.  An empty side or a NaN
cost is +inf.  The smallest cost wins; ties go to the lowest axis, then the lowest s (across axes the comparison is a strict <).
The code compares order-preserving integer images, for which -0.0 < +0.0: a cost of -0.0 needs a negative extent, and inverted
boxes are kept out of the exact cases (see below), so the model compares the floats.

Median fallback.  When no candidate is finite, or when the node is inside a subtree task and pending >= 36 (kSubStackSafe):
axis = 0, and the first n >> 1 records in the node's current order go low.  A task starts at the first node on a path with
n <= 256 (the root when the whole input is that small); the task's root has pending = 0, a low-side child its parent's
pending + 1, a high-side child its parent's pending (the number of high-side children the one-node-per-step subtree kernel has
waiting at that node; the row form carries the same number along as `vsp`).

Partition.  Stable; a record goes low when bin(c[axis]) < s.

Emission.  Pre-order, the low child at parent + 1.  Every node's box is the min and max over its primitives' boxes.  A branch is
{flag 0, axis, data = (low, high)}, a leaf {flag 1, axis 0, data = (count, first)}.  The index array lists the leaves'
primitives in pre-order.

Outside the model: non-finite coordinates, negative radii (inverted boxes), bounds at which -0.0 and +0.0 meet, the Morton
pre-pass and cylinder segments.

`python tests/builder_model.py --all` rebuilds the twelve grid9k / soup60k lines of tests/golden/tree_fingerprints.txt (GPU
output recorded long before the model existed) and compares node count and md5; tests/test_builder_model.py runs the eight
quick ones."""
import functools
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from nanort_amd.wire import NODE_F32, NODE_F64  # noqa: E402

K_SMALL = 256        # kSmall: nodes at or below it are binned with at most K_SMALL_BINS bins
K_HANDOFF = 256      # kHandoff: the first node of a path at or below it is a subtree task's root
K_MAX_BINS = 64      # kMaxBins
K_SMALL_BINS = 16    # kSmallBins
K_STACK_SAFE = 36    # kSubStackSafe

SAH, MEDIAN_NONE_FINITE, MEDIAN_FORCED = 0, 1, 2  # decisions["cause"]
MEDIAN = -1                                        # decisions["s"] of a median split

DECISION = np.dtype([
    ("node", "<i8"),       # pre-order index of the branch
    ("n", "<i8"), ("depth", "<i8"), ("K", "<i8"),
    ("pending", "<i8"),    # -1: a top-phase node (above the hand-off)
    ("axis", "<i8"), ("s", "<i8"), ("cause", "<i8"), ("nleft", "<i8"),
    ("cost", "<f8"),       # the winning candidate's cost (inf: none finite); for a forced median, the cost it overrode
    ("alt_cost", "<f8"),   # the best cost among candidates with a DIFFERENT low set (inf: none)
    ("tie_axis", "?"),     # a candidate on a higher axis, with a different low set, had exactly the winning cost
    ("tie_s", "?"),        # a candidate at a higher s of the winning axis, with a different low set, had exactly the winning cost
    ("scale_inf", "?"),    # a bin scale overflowed to infinity
])


def _t(real):
    return np.dtype(real).type


def records(kind, real, *a):
    """(bmin, bmax, centre), each (n, 3) of `real`, of the primitives of `kind`:
    "triangles": vertices (nv, 3), faces (n, 3);  "spheres": centres (n, 3), radii (n,);
    "cylinders": end points (n, 2, 3), radii (n, 2);  "curves": control points (n, 4, 3), radii (n, 4)."""
    T = _t(real)
    if kind == "triangles":
        p = np.asarray(a[0], dtype=T)[np.asarray(a[1], dtype=np.int64)]
        p0, p1, p2 = p[:, 0], p[:, 1], p[:, 2]
        return np.minimum(p0, np.minimum(p1, p2)), np.maximum(p0, np.maximum(p1, p2)), ((p0 + p1) + p2) * (T(1) / T(3))
    if kind == "spheres":
        c, r = np.asarray(a[0], dtype=T).reshape(-1, 3), np.asarray(a[1], dtype=T).reshape(-1, 1)
        return c - r, c + r, c.copy()
    if kind == "cylinders":
        e, r = np.asarray(a[0], dtype=T).reshape(-1, 2, 3), np.asarray(a[1], dtype=T).reshape(-1, 2, 1)
        return np.minimum(e[:, 1] - r[:, 1], e[:, 0] - r[:, 0]), np.maximum(e[:, 1] + r[:, 1], e[:, 0] + r[:, 0]), (e[:, 0] + e[:, 1]) / T(2)
    if kind == "curves":
        p, r = np.asarray(a[0], dtype=T).reshape(-1, 4, 3), np.asarray(a[1], dtype=T).reshape(-1, 4, 1)
        lo, hi = p[:, 0] - r[:, 0], p[:, 0] + r[:, 0]
        for j in range(1, 4):
            lo, hi = np.minimum(p[:, j] - r[:, j], lo), np.maximum(p[:, j] + r[:, j], hi)
        return lo, hi, (((p[:, 0] + p[:, 1]) + p[:, 2]) + p[:, 3]) / T(4)
    raise ValueError(kind)


def median_count(n):
    """Records that go low at an object-median split of n."""
    return n >> 1


def node_bins(n, bin_size):
    K0 = min(max(int(bin_size), 2), K_MAX_BINS)
    return min(K0, K_SMALL_BINS) if n <= K_SMALL else K0


def bins_of(c, lo, hi, K, T):
    """((m, 3) bins, (3,) scale) of the centres `c` of a node whose centre bounds are lo, hi."""
    ext = hi - lo
    with np.errstate(all="ignore"):
        scale = np.where(ext > 0, T(K) / np.where(ext > 0, ext, T(1)), T(0)).astype(T)
        x = (c - lo) * scale
    # (int) as the GPU converts: NaN -> 0, too large -> INT_MAX, then the clamp (x is never negative: c >= lo)
    x = np.where(np.isnan(x), T(0), np.minimum(x, T(K - 1)))
    return np.clip(x.astype(np.int64), 0, K - 1), scale


def _half_area(mn, mx):
    e = mx - mn
    a, b, c = e[..., 0], e[..., 1], e[..., 2]
    return (a * b + b * c) + c * a


def candidate_cost(nl, area_l, nr, area_r):
    """cost = T(nl) * ha(L) + T(nr) * ha(R); the counts arrive converted to T."""
    return nl * area_l + nr * area_r


def pick(cost):
    """(axis, s) of the winning candidate of costs (3, K - 1): the first minimum in axis-major order — lowest axis, then lowest s."""
    j = int(np.argmin(cost))
    return j // cost.shape[1], j % cost.shape[1] + 1


def cut_search(bmin, bmax, b, K, T):
    """Costs (3, K - 1) of the candidates (axis, s = 1..K-1) — inf where a side is empty or the cost is NaN — and their low-side
    counts (3, K - 1), from the node's records' boxes and bins `b` (m, 3)."""
    m = b.shape[0]
    big = np.finfo(T).max
    flat = (b + K * np.arange(3)).T.reshape(-1)        # bin id over the three axes, axis-major
    cnt = np.bincount(flat, minlength=3 * K).reshape(3, K)
    mn = np.full((3 * K, 3), big, dtype=T)
    mx = np.full((3 * K, 3), -big, dtype=T)
    np.minimum.at(mn, flat, np.tile(bmin, (3, 1)))
    np.maximum.at(mx, flat, np.tile(bmax, (3, 1)))
    mn, mx = mn.reshape(3, K, 3), mx.reshape(3, K, 3)
    pmn, pmx = np.minimum.accumulate(mn, axis=1), np.maximum.accumulate(mx, axis=1)
    smn, smx = np.minimum.accumulate(mn[:, ::-1], axis=1)[:, ::-1], np.maximum.accumulate(mx[:, ::-1], axis=1)[:, ::-1]
    nl = np.cumsum(cnt, axis=1)[:, :-1]                # low side of s = 1..K-1: bins [0, s)
    nr = m - nl
    with np.errstate(all="ignore"):
        cost = candidate_cost(nl.astype(T), _half_area(pmn[:, :-1], pmx[:, :-1]), nr.astype(T), _half_area(smn[:, 1:], smx[:, 1:]))
    ok = (nl > 0) & (nr > 0) & (cost == cost)
    return np.where(ok, cost, T(np.inf)).astype(T), nl


def _rivals(cost, nl, b, ka, sa):
    """(best cost among candidates whose low set differs from the winner's (axis ka, cut sa), tie on a higher axis, tie at a higher s)."""
    K1 = cost.shape[1]
    win, nla = cost[ka, sa - 1], nl[ka, sa - 1]
    differs = (nl != nla) & np.isfinite(cost)
    for k in range(3):                                 # (another axis may cut off the very same records: compare the sets)
        if k == ka:
            continue
        same_n = np.nonzero((nl[k] == nla) & np.isfinite(cost[k]))[0]
        if same_n.size:
            low = b[:, ka] < sa
            for j in same_n:
                differs[k, j] = not np.array_equal(b[:, k] < j + 1, low)
    alt = cost[differs].min() if differs.any() else np.inf
    tied = differs & (cost == win)
    return float(alt), bool(tied[ka + 1:].any()), bool(tied[ka, sa:].any()) if sa < K1 else False


def build(bmin, bmax, centre, real, min_leaf=4, max_depth=256, bin_size=64):
    """(nodes, indices, decisions): the tree of the rule in this module's docstring over the records (bmin, bmax, centre) — see
    records() — in precision `real`, and one DECISION row per branch, in pre-order."""
    T = _t(real)
    bmin, bmax, centre = (np.ascontiguousarray(x, dtype=T) for x in (bmin, bmax, centre))
    n = centre.shape[0]
    assert n >= 1
    leaf_max = max(int(min_leaf), 1)
    lo_, hi_, flag_, axis_, d0_, d1_ = [], [], [], [], [], []
    out_idx, dec = [], []
    # (ids, depth, pending, the branch whose data[1] this node is, or -1); pending None: top phase
    stack = [(np.arange(n, dtype=np.int64), 0, None, -1)]
    while stack:
        ids, depth, pending, high_of = stack.pop()
        m = ids.shape[0]
        me = len(flag_)
        if high_of >= 0:
            d1_[high_of] = me
        lo_.append(bmin[ids].min(axis=0))
        hi_.append(bmax[ids].max(axis=0))
        if depth >= max_depth or m <= leaf_max:
            flag_.append(1), axis_.append(0), d0_.append(m), d1_.append(len(out_idx))
            out_idx.extend(ids.tolist())
            continue
        if pending is None and m <= K_HANDOFF:
            pending = 0                                 # a subtree task starts here
        K = node_bins(m, bin_size)
        c = centre[ids]
        b, scale = bins_of(c, c.min(axis=0), c.max(axis=0), K, T)
        cost, nl = cut_search(bmin[ids], bmax[ids], b, K, T)
        ka, sa = pick(cost)
        found = bool(np.isfinite(cost[ka, sa - 1]))
        forced = pending is not None and pending >= K_STACK_SAFE
        row = np.zeros((), dtype=DECISION)
        row["node"], row["n"], row["depth"], row["K"] = me, m, depth, K
        row["pending"] = -1 if pending is None else pending
        row["scale_inf"] = bool(np.isinf(scale).any())
        row["cost"], row["alt_cost"] = (cost[ka, sa - 1], np.inf) if found else (np.inf, np.inf)
        if found:
            row["alt_cost"], row["tie_axis"], row["tie_s"] = _rivals(cost, nl, b, ka, sa)
        if not found or forced:
            axis, nleft = 0, median_count(m)
            low = np.arange(m) < nleft
            row["s"], row["cause"] = MEDIAN, (MEDIAN_FORCED if found else MEDIAN_NONE_FINITE)
        else:
            axis, nleft = ka, int(nl[ka, sa - 1])
            low = b[:, ka] < sa
            row["s"], row["cause"] = sa, SAH
        row["axis"], row["nleft"] = axis, nleft
        dec.append(row)
        flag_.append(0), axis_.append(axis), d0_.append(me + 1), d1_.append(0)
        stack.append((ids[~low], depth + 1, pending, me))
        stack.append((ids[low], depth + 1, None if pending is None else pending + 1, -1))
    nodes = np.zeros(len(flag_), dtype=NODE_F32 if T is np.float32 else NODE_F64)
    nodes["bmin"], nodes["bmax"] = np.array(lo_, dtype=T), np.array(hi_, dtype=T)
    nodes["flag"], nodes["axis"] = flag_, axis_
    nodes["data"][:, 0], nodes["data"][:, 1] = d0_, d1_
    decisions = np.array(dec, dtype=DECISION) if dec else np.zeros(0, dtype=DECISION)
    return nodes, np.array(out_idx, dtype=np.uint32), decisions


def fingerprint(nodes, indices):
    """What tools/tree_hash.py prints of a tree: (node count, md5 of node array + index array)."""
    return nodes.shape[0], hashlib.md5(nodes.tobytes() + indices.tobytes()).hexdigest()


def _parents(nodes):
    parent = np.full(nodes.shape[0], -1, dtype=np.int64)
    br = np.nonzero(nodes["flag"] == 0)[0]
    parent[nodes["data"][br, 0].astype(np.int64)] = br
    parent[nodes["data"][br, 1].astype(np.int64)] = br
    return parent


def _decision_text(decisions, node):
    hit = decisions[decisions["node"] == node]
    if hit.size == 0:
        return "    (no decision: the model has a leaf there)"
    return "    " + ", ".join("%s=%s" % (k, hit[0][k]) for k in DECISION.names)


def first_difference(nodes_a, idx_a, nodes_b, idx_b, decisions):
    """The message of a failing comparison: the first record in pre-order at which the tree (nodes_a, idx_a) departs from the
    model's (nodes_b, idx_b), with the model's decision for that node and for its parent — the split that made it.  None: equal."""
    if nodes_a.tobytes() == nodes_b.tobytes() and idx_a.tobytes() == idx_b.tobytes():
        return None
    parent = _parents(nodes_b)
    lines = ["nodes: %d, the model's: %d" % (nodes_a.shape[0], nodes_b.shape[0])]
    k = min(nodes_a.shape[0], nodes_b.shape[0])
    raw_a = np.frombuffer(nodes_a[:k].tobytes(), dtype=np.uint8).reshape(k, -1)
    raw_b = np.frombuffer(nodes_b[:k].tobytes(), dtype=np.uint8).reshape(k, -1)
    bad = np.nonzero((raw_a != raw_b).any(axis=1))[0]
    if bad.size or nodes_a.shape[0] != nodes_b.shape[0]:
        i = int(bad[0]) if bad.size else k
        lines.append("first differing node: %d" % i)
        if i < nodes_a.shape[0]:
            lines.append("  got   %s" % (nodes_a[i],))
        if i < nodes_b.shape[0]:
            lines.append("  model %s" % (nodes_b[i],))
            lines.append("  the model's decision at node %d:" % i)
            lines.append(_decision_text(decisions, i))
            if parent[i] >= 0:
                lines.append("  the model's decision at its parent, node %d:" % parent[i])
                lines.append(_decision_text(decisions, parent[i]))
    else:
        q = min(idx_a.shape[0], idx_b.shape[0])
        slot = np.nonzero(idx_a[:q] != idx_b[:q])[0]
        s = int(slot[0]) if slot.size else q
        lines.append("node arrays equal; first differing index slot: %d (got %s, model %s)" %
                     (s, idx_a[s] if s < idx_a.shape[0] else None, idx_b[s] if s < idx_b.shape[0] else None))
        leaves = np.nonzero(nodes_b["flag"] == 1)[0]
        first = nodes_b["data"][leaves, 1].astype(np.int64)
        cnt = nodes_b["data"][leaves, 0].astype(np.int64)
        inside = leaves[(first <= s) & (s < first + cnt)]
        if inside.size and parent[inside[0]] >= 0:
            lines.append("  in leaf %d; the model's decision at its parent, node %d:" % (inside[0], parent[inside[0]]))
            lines.append(_decision_text(decisions, parent[inside[0]]))
    return "\n".join(lines)


FINGERPRINT_OPTIONS = ((4, 64, 256), (1, 8, 256), (16, 200, 12))  # (min_leaf, bin_size, max_depth) of tools/tree_hash.py
QUICK_FINGERPRINTS = [("grid9k", real, o) for real in (np.float32, np.float64) for o in FINGERPRINT_OPTIONS] + \
                     [("soup60k", real, (16, 200, 12)) for real in (np.float32, np.float64)]
ALL_FINGERPRINTS = [(name, real, o) for name in ("soup60k", "grid9k") for real in (np.float32, np.float64) for o in FINGERPRINT_OPTIONS]


def recorded_fingerprints():
    """{(mesh, precision name, min_leaf, bin_size, max_depth): (node count, md5)} of tests/golden/tree_fingerprints.txt."""
    out = {}
    for line in open(os.path.join(HERE, "golden", "tree_fingerprints.txt")):
        w = line.split()
        if len(w) == 7:
            out[(w[0], w[1], int(w[2]), int(w[3]), int(w[4]))] = (int(w[5]), w[6])
    return out


@functools.lru_cache(maxsize=None)
def tree_hash_inputs():
    """The numpy-only meshes of tools/tree_hash.py, {"soup60k": (v, f), "grid9k": (v, f)}, from its own generator."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("tree_hash", os.path.join(os.path.dirname(HERE), "tools", "tree_hash.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.numpy_meshes()


def model_fingerprint(inputs, name, real, options):
    v, f = inputs[name]
    ml, bins, md = options
    nodes, idx, _ = build(*records("triangles", real, v.astype(real), f), real, ml, md, bins)
    return fingerprint(nodes, idx)


if __name__ == "__main__":
    import time

    cases = ALL_FINGERPRINTS if "--all" in sys.argv[1:] else QUICK_FINGERPRINTS
    want, inputs, bad = recorded_fingerprints(), tree_hash_inputs(), 0
    for name, real, o in cases:
        t0 = time.time()
        got = model_fingerprint(inputs, name, real, o)
        ok = got == want[(name, real.__name__) + o]
        bad += not ok
        print(name, real.__name__, *o, *got, "OK" if ok else "DIFFERS from %s %s" % want[(name, real.__name__) + o], "%.1f s" % (time.time() - t0), flush=True)
    sys.exit(1 if bad else 0)
