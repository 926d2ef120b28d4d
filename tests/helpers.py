"""Shared test helpers (CPU side): tie-aware hit comparison, option builders, recorded answers of the reference."""
import hashlib
import os

import numpy as np

from nanort_amd.wire import default_trace_options

LIVE_REF_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "live_ref")


def outputs_digest(*arrays, canonical_nan=False):
    """sha256 over the arrays, field by field (the padding of fp64 records left out); equal digests = equal bits.  With
    canonical_nan every NaN counts as the same NaN (np.array_equal(..., equal_nan=True) field by field)."""
    d = hashlib.sha256()
    for a in arrays:
        for k in a.dtype.names or (None,):
            x = np.ascontiguousarray(a if k is None else a[k])
            if canonical_nan and x.dtype.kind == "f":
                x = np.where(np.isnan(x), np.nan, x).astype(x.dtype)
            d.update(x.tobytes())
    return d.hexdigest()


def reference_answers(case, live=None):
    """The unmodified reference's answers for one case of a test against it: (nodes, indices, digest of its outputs).
    Where the reference libraries are built (oracle/_ref), `live()` computes them and they must equal the record under
    tests/golden/live_ref/ (RECORD_REFERENCE_ANSWERS=1 writes the record instead); elsewhere the record stands in for them."""
    path = os.path.join(LIVE_REF_DIR, case + ".npz")
    if live is None:
        rec = np.load(path)
        return (rec["nodes"] if rec["nodes"].size else None), (rec["indices"] if rec["indices"].size else None), str(rec["digest"])
    nodes, indices, digest = live()
    tree = None
    if nodes is not None:
        tree = nodes.copy()
        tree["axis"][tree["flag"] == 1] = 0  # (the reference never writes a leaf's axis)
    if os.environ.get("RECORD_REFERENCE_ANSWERS") == "1":
        os.makedirs(LIVE_REF_DIR, exist_ok=True)
        np.savez_compressed(path, nodes=tree if tree is not None else np.zeros(0), indices=indices if indices is not None else np.zeros(0),
                            digest=np.array(digest))
    rec = np.load(path)
    assert str(rec["digest"]) == digest, "%s: the reference's outputs differ from the record" % case
    if tree is not None:
        assert rec["nodes"].tobytes() == tree.tobytes() and np.array_equal(rec["indices"], indices), "%s: tree differs from the record" % case
    return nodes, indices, digest


def trace_options(range_=None, skip=None, cull=None):
    o = default_trace_options()
    if range_ is not None:
        o["prim_ids_range"] = range_
    if skip is not None:
        o["skip_prim_id"] = skip
    if cull is not None:
        o["cull_back_face"] = 1 if cull else 0
    return o


def _fields_equal(a, b):
    """Bitwise equality of the four meaningful fields (fp64 records carry 4 padding bytes)."""
    return all(np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes() for k in ("t", "u", "v", "prim_id"))


def assert_hits_identical(a_hits, a_mask, b_hits, b_mask):
    """Bit-for-bit equality of hit records (same tree => same tie breaks)."""
    assert np.array_equal(a_mask, b_mask), "hit masks differ at %s" % np.nonzero(a_mask != b_mask)[0][:8]
    if not _fields_equal(a_hits, b_hits):
        bad = np.nonzero(
            (a_hits["t"] != b_hits["t"]) | (a_hits["prim_id"] != b_hits["prim_id"])
            | (a_hits["u"] != b_hits["u"]) | (a_hits["v"] != b_hits["v"])
        )[0]
        raise AssertionError("hit records differ at %d rays, first %s:\n%s\n%s" % (
            bad.size, bad[:4], a_hits[bad[:4]], b_hits[bad[:4]]))


def assert_hits_match(ref_hits, ref_mask, hits, mask, oracle, onodes, oindices, verts, faces, rays,
                      base_opts=None, max_ties=None):
    """Parity across DIFFERENT trees: hit flags and t bit-equal
    everywhere; u, v, prim_id bit-equal except at true ties — two primitives at
    exactly the same t along the ray (shared edges/vertices), where the
    reference itself keeps whichever it tested last (nanort.h:1133 accepts
    equality).  Every such ray is verified: the oracle restricted to the
    reported primitive must reproduce the reported record bit-for-bit.
    Returns the number of ties."""
    assert np.array_equal(ref_mask, mask), "hit masks differ at %s" % np.nonzero(ref_mask != mask)[0][:8]
    rt, ht = np.ascontiguousarray(ref_hits["t"]), np.ascontiguousarray(hits["t"])
    ubits = np.uint32 if rt.dtype.itemsize == 4 else np.uint64
    same_bits = rt.view(ubits) == ht.view(ubits)
    # (the one pair of equal values with different bits is +0.0 / -0.0: two primitives met at t == 0, e.g. a ray that starts
    # on a shared vertex — a tie like any other, verified below)
    t_ok = same_bits | (rt == ht)
    assert t_ok.all(), "t differs at %s" % np.nonzero(~t_ok)[0][:8]
    diff_mask = (ref_hits["prim_id"] != hits["prim_id"]) | ~same_bits
    diff = np.nonzero(diff_mask)[0]
    same = ~diff_mask
    assert np.array_equal(ref_hits["u"][same], hits["u"][same]) and np.array_equal(ref_hits["v"][same], hits["v"][same]), \
        "u/v differ on rays that report the same primitive"
    if max_ties is not None:
        assert diff.size <= max_ties, "%d prim_id mismatches" % diff.size
    for i in diff:
        o = default_trace_options() if base_opts is None else base_opts.copy()
        p = int(hits["prim_id"][i])
        lo = max(p, int(o["prim_ids_range"][0]))
        hi = min(p + 1, int(o["prim_ids_range"][1]))
        o["prim_ids_range"] = (lo, hi)
        h1, m1 = oracle.traverse(onodes, oindices, verts, faces, rays[i:i + 1], o)
        assert m1[0] == 1 and _fields_equal(h1, hits[i:i + 1]), \
            "ray %d: reported prim %d is not an exact tie of the reference's prim %d" % (i, p, ref_hits["prim_id"][i])
    return int(diff.size)


def walk_order_bits(kernel_name):
    """Template arguments of k_traverse_wide: <T, STACK, STATS, KIND, PLAIN, CLOCK, WIDTH, ORDER> -> (WIDTH, ORDER).  ORDER bit 0:
    slots entered by entry distance (opt-in, tunable order4); bit 1: the leaf phase over items (tunable leaf_compact, default on —
    records bit-identical either way)."""
    args = kernel_name.split("<", 1)[1].rstrip(">").split(", ")
    return int(args[6]), int(args[7])


def is_reference_order_two_level_walk(kernel_name):
    w, o = walk_order_bits(kernel_name)
    return w == 4 and (o & 1) == 0


def is_distance_order_two_level_walk(kernel_name):
    w, o = walk_order_bits(kernel_name)
    return w == 4 and (o & 1) == 1


def first_leaf_stack_bound(nodes):
    """Entries the two-level walk holds, at the least, when a ray that hits EVERY box reaches its first leaf: a step over a record
    with k occupied slots pushes k - 1 and enters one; whichever slot the ray's signs rank first, the minimum over the slots bounds
    it from below (nothing is culled before the first leaf: there is no hit yet)."""
    leaf = nodes["flag"] != 0
    kids = nodes["data"]
    g = {}
    todo = [0]
    while todo:  # post-order without recursion
        i = todo[-1]
        slots = []
        for c in kids[i]:
            slots += [int(c)] if leaf[c] else [int(x) for x in kids[c]]
        missing = [s for s in slots if not leaf[s] and s not in g]
        if missing:
            todo += missing
            continue
        g[i] = len(slots) - 1 + min(0 if leaf[s] else g[s] for s in slots)
        todo.pop()
    return g[0]


def deep_stack_case(n_rays=1500, nt=6144, ndup=2048, seed=11):
    """A pile of nt large triangles that all straddle the z axis plus `ndup` exact duplicates (of the two that the rays hit first
    and of random others), and n_rays rays along that axis, alternately from z = -5 and z = +5, through |x|, |y| < 0.3.  Built with
    min_leaf_primitives = 1, every box of the pile's tree is hit by every ray: every two-level step pushes three entries and the
    walk's stack passes its LDS entries into the spill arrays (the tests establish both from the built tree: the boxes, and
    first_leaf_stack_bound).  Returns (verts, faces, dup, nt, rays): faces nt.. are the duplicates of faces dup."""
    from nanort_amd import scenes

    rng = np.random.default_rng(seed)
    z = rng.uniform(-0.5, 0.5, nt).astype(np.float32)
    base = np.array([[-1.0, -1.0], [1.0, -1.0], [0.0, 1.5]], dtype=np.float32)
    v = np.zeros((nt, 3, 3), dtype=np.float32)
    v[:, :, :2] = base[None] + rng.uniform(-0.1, 0.1, (nt, 3, 2)).astype(np.float32)
    v[:, :, 2] = z[:, None]
    v = v.reshape(-1, 3)
    f = np.arange(3 * nt, dtype=np.uint32).reshape(nt, 3)
    dup = np.concatenate([[int(np.argmin(z)), int(np.argmax(z))], rng.integers(0, nt, ndup - 2)])  # (the two triangles the rays hit first among them)
    f = np.concatenate([f, f[dup]]).astype(np.uint32)  # exact duplicates
    rays = np.zeros(n_rays, dtype=scenes.camera_rays(2, 2).dtype)
    rays["org"][:, :2] = rng.uniform(-0.3, 0.3, (n_rays, 2))
    rays["org"][:, 2] = np.where(np.arange(n_rays) % 2 == 0, -5.0, 5.0)
    rays["dir"][:, 2] = -np.sign(rays["org"][:, 2])
    rays["max_t"] = np.finfo(np.float32).max
    return v, f, dup, nt, rays
