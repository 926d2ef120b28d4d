"""Helpers of the size-threshold tests (test_size_thresholds.py on the CPU, test_gpu_size_thresholds.py on the GPU): the caps of
every kernel and host loop that runs a fixed number of workgroups or fixed-size pieces and covers the rest by looping, read from
the sources; rays tiled from a base set whose length shares no factor with any cap; and a complete binary tree wide enough to
put more branches on one level than a capped grid covers in one trip."""
import os
import re

import numpy as np

import refit_model
from nanort_amd.wire import default_trace_options, hit_dtype, node_dtype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nanort_amd", "csrc")

# Base length of every tiled ray set: prime, so the same offset in two pieces, or in two trips of a grid-stride loop, never holds
# the same base ray (4093 divides none of 256, 524 288 = 2048 * 256, 2^19; 2^19 mod 4093 = 384).
B = 4093

# What the GPU cases were sized for.  test_size_thresholds.py asserts the sources still say so; each entry names the GPU cases to
# resize when it changes.
CAPS = {
    "kRefitMaxGrid": (1024, "refit.hip", r"constexpr\s+unsigned\s+kRefitMaxGrid\s*=\s*(\d+)\s*;",
                      "B1, B2 (leaf list) and B3 (one level) of test_gpu_size_thresholds.py: REFIT_CAP"),
    "kRefitBlock": (256, "refit.hip", r"constexpr\s+unsigned\s+kRefitBlock\s*=\s*(\d+)\s*;",
                    "B1, B2 (leaf list) and B3 (one level) of test_gpu_size_thresholds.py: REFIT_CAP"),
    "kMeshMaxGrid": (2048, "prims.hip", r"constexpr\s+unsigned\s+kMeshMaxGrid\s*=\s*(\d+)\s*;",
                     "B5 (k_max_index) of test_gpu_size_thresholds.py: MAX_INDEX_CAP_WORDS"),
    "kMeshBlock": (256, "prims.hip", r"constexpr\s+unsigned\s+kMeshBlock\s*=\s*(\d+)\s*;",
                   "B5 (k_max_index) of test_gpu_size_thresholds.py: MAX_INDEX_CAP_WORDS"),
    "post pass grid": (2048, "prims.hip", r"const\s+dim3\s+grid\(std::min\(\(n \+ 255u\) / 256u,\s*(\d+)u\)\),\s*block\(256\);",
                       "B4 (post passes) of test_gpu_size_thresholds.py: POST_PASS_CAP"),
    "kPiece": (1 << 19, "api_query.hip", r"const\s+uint64_t\s+kPiece\s*=\s*1ull\s*<<\s*(\d+)\s*;",
               "B6 (pipelined host path) of test_gpu_size_thresholds.py: PIECE"),
}

REFIT_CAP = 1024 * 256            # list entries one trip of k_refit_leaves / k_plan_expand / k_refit_branches covers
POST_PASS_CAP = 2048 * 256        # rays one trip of k_sphere_uv / k_cylinder_post / k_curve_post covers
MAX_INDEX_CAP_WORDS = 2048 * 256 * 4  # index words one trip of k_max_index covers (128-bit loads)
PIECE = 1 << 19                   # rays per piece of the pipelined host path; it starts at 2 * PIECE
POST_PASS_N = POST_PASS_CAP + 2 * B + 17  # the part past the cap holds every base ray at least twice


def source_cap(name):
    """The value the source states for CAPS[name] (kPiece: the shifted value)."""
    _, fname, pattern, _ = CAPS[name]
    text = open(os.path.join(CSRC, fname)).read()
    found = re.findall(pattern, text)
    assert len(found) == 1, "%s: %d matches of %r in %s (the constant moved: update size_thresholds.CAPS)" % (name, len(found), pattern, fname)
    v = int(found[0])
    return (1 << v) if name == "kPiece" else v


def tiled(base, n):
    """n records: base[0], base[1], ..., base[len - 1], base[0], ..."""
    return base[np.arange(n) % len(base)]


def cut(rays, n=B):
    """n rays of a fixture's set, evenly spaced over all of it (its camera rays and its extras)."""
    assert rays.shape[0] >= n
    return np.ascontiguousarray(rays[np.linspace(0, rays.shape[0] - 1, n).astype(np.int64)])


def crossing_trips(n, cap):
    """Trips a grid-stride loop (or a loop over pieces) of `cap` items per trip needs for n items."""
    return (n + cap - 1) // cap


def reachable_leaves(nodes):
    reach = np.concatenate(refit_model.levels(nodes))
    return int((nodes["flag"][reach] != 0).sum())


def widest_level(nodes):
    """The largest number of branches on one level of the walk from the root."""
    return max(int((nodes["flag"][lvl] == 0).sum()) for lvl in refit_model.levels(nodes))


def balanced_topology(n_leaves, real):
    """(nodes, indices) of balanced_tree with every box zero: flag, axis and data alone."""
    assert n_leaves >= 2 and n_leaves & (n_leaves - 1) == 0
    nb = n_leaves - 1
    nodes = np.zeros(2 * n_leaves - 1, dtype=node_dtype(real))
    i = np.arange(nb, dtype=np.uint32)
    nodes["data"][:nb, 0] = 2 * i + 1
    nodes["data"][:nb, 1] = 2 * i + 2
    nodes["flag"][nb:] = 1
    nodes["data"][nb:, 0] = 1
    nodes["data"][nb:, 1] = np.arange(n_leaves, dtype=np.uint32)
    return nodes, np.arange(n_leaves, dtype=np.uint32)


def balanced_tree(n_leaves, real, verts, faces):
    """(nodes, indices): a complete binary tree over the first n_leaves faces in heap order — node i has the children 2 i + 1 and
    2 i + 2, the n_leaves - 1 branches come first, leaf k (record n_leaves - 1 + k) holds slot k alone, indices = arange — with
    the boxes tests/refit_model.py gives it over `verts`: a tree nrtSetTree adopts.  n_leaves is a power of two."""
    assert n_leaves <= faces.shape[0]
    nodes, indices = balanced_topology(n_leaves, real)
    return refit_model.refit(nodes, indices, np.asarray(verts, dtype=real), faces), indices


def in_pre_order(nodes):
    """The same tree with its records renumbered in depth-first pre-order (low child first), the numbering the reference's builder
    emits and bvh_check.validate_bvh asks for; every record keeps its box, and a leaf its slots."""
    order, stack = [], [0]
    while stack:
        i = stack.pop()
        order.append(i)
        if nodes["flag"][i] == 0:
            stack += [int(nodes["data"][i, 1]), int(nodes["data"][i, 0])]
    order = np.array(order, dtype=np.int64)
    new_id = np.empty(nodes.shape[0], dtype=np.int64)
    new_id[order] = np.arange(order.size)
    out = nodes[order].copy()
    br = out["flag"] == 0
    out["data"][br] = new_id[out["data"][br].astype(np.int64)].astype(np.uint32)
    return out


def per_ray_skip(oracle, nodes, indices, verts, faces, rays, ids):
    """The CPU restatement with BVHTraceOptions::skip_prim_id = ids[i] for ray i: one oracle call per distinct id (as
    test_gpu_skip_ids.oracle_per_ray_skip)."""
    hits = np.zeros(rays.shape[0], dtype=hit_dtype(verts.dtype))
    mask = np.zeros(rays.shape[0], dtype=np.uint8)
    for p in np.unique(ids):
        sel = np.nonzero(ids == p)[0]
        o = default_trace_options()
        o["skip_prim_id"] = p
        h, m = oracle.traverse(nodes, indices, verts, faces, rays[sel], o)
        hits[sel], mask[sel] = h, m
    return hits, mask
