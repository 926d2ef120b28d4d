"""The numpy model of a sphere / curve refit (tests/refit_prims_model.py) checked on its own: on hand-made node arrays every
reachable record's box equals brute force over the slots of its subtree, an empty leaf gets {+max, -max}, unreachable records
keep their bytes, and the curve rule equals the C model of the example's BoundingBoxAndCenter (tests/curves_model.c)."""
import numpy as np
import pytest

import curves_fixture as cf
from nanort_amd.wire import NODE_F32
from refit_prims_model import brute_boxes, curve_boxes, prim_boxes, refit, refit_boxes, sphere_boxes, topology_bytes

BIG = np.finfo(np.float32).max


def spheres(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-3, 3, size=(n, 3)).astype(np.float32), rng.uniform(0.01, 0.7, size=n).astype(np.float32)


def curves(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-3, 3, size=(n, 4, 3)).astype(np.float32), rng.uniform(0.0, 0.4, size=(n, 4)).astype(np.float32)


def leaf(nodes, i, count, first):
    nodes[i]["flag"], nodes[i]["data"] = 1, (count, first)


def branch(nodes, i, a, b, axis=0):
    nodes[i]["flag"], nodes[i]["axis"], nodes[i]["data"] = 0, axis, (a, b)


def root_is_leaf(n):
    nodes = np.zeros(1, NODE_F32)
    leaf(nodes, 0, n, 0)
    return nodes, np.arange(n, dtype=np.uint32)[::-1].copy()


def three_nodes(n):
    nodes = np.zeros(3, NODE_F32)
    branch(nodes, 0, 1, 2, axis=2)
    leaf(nodes, 1, n // 2, 0)
    leaf(nodes, 2, n - n // 2, n // 2)
    return nodes, np.random.default_rng(1).permutation(n).astype(np.uint32)


def empty_and_unreachable(n):
    """0 -> (1, 4); 1 -> (2, 3); 3 is an empty leaf; 5 (a leaf) and 6 (a branch) are never reached."""
    nodes = np.zeros(7, NODE_F32)
    branch(nodes, 0, 1, 4)
    branch(nodes, 1, 2, 3, axis=1)
    leaf(nodes, 2, 2, 0)
    leaf(nodes, 3, 0, 2)
    leaf(nodes, 4, n - 2, 2)
    leaf(nodes, 5, 1, 0)
    nodes[5]["bmin"], nodes[5]["bmax"] = (9, 9, 9), (10, 10, 10)
    branch(nodes, 6, 2, 4)
    nodes[6]["bmin"], nodes[6]["bmax"] = (-7, -7, -7), (7, 7, 7)
    return nodes, np.arange(n, dtype=np.uint32)


def random_topology(n, seed):
    """A random binary tree over a permutation of n primitives, leaves of 1..4 slots, the records in a shuffled order (root at 0)."""
    rng = np.random.default_rng(seed)
    recs = []  # (is_leaf, a, b): a leaf's (count, first), a branch's child positions in recs

    def make(first, count):
        me = len(recs)
        recs.append(None)
        if count <= int(rng.integers(1, 5)):
            recs[me] = (True, count, first)
        else:
            cut = int(rng.integers(1, count))
            a = make(first, cut)
            b = make(first + cut, count - cut)
            recs[me] = (False, a, b)
        return me

    make(0, n)
    order = np.concatenate([[0], 1 + rng.permutation(len(recs) - 1)]).astype(np.int64)  # creation position -> record id
    nodes = np.zeros(len(recs), NODE_F32)
    for pos, (is_leaf, a, b) in enumerate(recs):
        if is_leaf:
            leaf(nodes, order[pos], a, b)
        else:
            branch(nodes, order[pos], order[a], order[b], axis=int(rng.integers(0, 3)))
    return nodes, rng.permutation(n).astype(np.uint32)


TREES = {
    "root_is_leaf": lambda: root_is_leaf(3),
    "three_nodes": lambda: three_nodes(7),
    "empty_and_unreachable": lambda: empty_and_unreachable(6),
    "random_200": lambda: random_topology(260, 5),
}


@pytest.mark.parametrize("kind", ["spheres", "curves"])
@pytest.mark.parametrize("tree", sorted(TREES))
def test_model_equals_brute_force_over_each_subtree(tree, kind):
    nodes, idx = TREES[tree]()
    n = idx.shape[0]
    pos, rad = spheres(n, 3) if kind == "spheres" else curves(n, 4)
    r = refit(kind, nodes, idx, pos, rad)
    assert topology_bytes(r) == topology_bytes(nodes)
    lo, hi = prim_boxes(kind, pos, rad)
    bf = brute_boxes(nodes, idx, lo, hi)
    if tree == "random_200":
        assert 150 <= nodes.shape[0] <= 400 and len(bf) == nodes.shape[0]
    for i, (blo, bhi) in bf.items():
        assert np.array_equal(r["bmin"][i], blo) and np.array_equal(r["bmax"][i], bhi), "node %d" % i


def test_empty_leaf_and_unreachable_records():
    nodes, idx = empty_and_unreachable(6)
    c, rad = spheres(6, 9)
    r = refit("spheres", nodes, idx, c, rad)
    assert np.array_equal(r["bmin"][3], [BIG] * 3) and np.array_equal(r["bmax"][3], [-BIG] * 3)
    assert np.array_equal(r["bmin"][1], r["bmin"][2]) and np.array_equal(r["bmax"][1], r["bmax"][2])  # the empty leaf adds nothing
    assert r[5].tobytes() == nodes[5].tobytes() and r[6].tobytes() == nodes[6].tobytes()
    lo, hi = sphere_boxes(c, rad)
    assert np.array_equal(r["bmin"][0], lo.min(axis=0)) and np.array_equal(r["bmax"][0], hi.max(axis=0))


def test_sphere_rule_is_one_float32_rounding():
    c, rad = spheres(1000, 11)
    lo, hi = sphere_boxes(c, rad)
    assert lo.dtype == np.float32 and hi.dtype == np.float32
    want_lo = (c.astype(np.float64) - rad[:, None].astype(np.float64)).astype(np.float32)  # (exact in double, then rounded once)
    want_hi = (c.astype(np.float64) + rad[:, None].astype(np.float64)).astype(np.float32)
    assert np.array_equal(lo, want_lo) and np.array_equal(hi, want_hi)


@pytest.mark.parametrize("scene", ["1", "5", "64", "fur"])
def test_curve_rule_equals_the_c_model(scene):
    cps, radii = cf.scene(scene)
    lo, hi = curve_boxes(cps, radii)
    mlo, mhi, _ = cf.model_boxes(cps, radii)
    assert np.array_equal(lo, mlo) and np.array_equal(hi, mhi)


def test_refit_with_the_arrays_of_the_tree_reproduces_the_reference_boxes():
    """The fur fixture's reference-built tree: the model over the fixture's own curves gives back every box the reference wrote."""
    g = cf.fur_golden()
    lo, hi = curve_boxes(g["cps"], g["radii"])
    r = refit_boxes(g["nodes"], g["indices"], lo, hi)
    assert np.array_equal(r["bmin"], g["nodes"]["bmin"]) and np.array_equal(r["bmax"], g["nodes"]["bmax"])
