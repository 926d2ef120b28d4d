"""The numpy refit model (tests/refit_model.py) pinned to the reference: with a build's own vertices it reproduces the
reference builder's node boxes exactly, and on moved vertices every box equals brute force over its subtree's slots."""
import numpy as np
import pytest

from refit_model import assert_boxes_equal, brute_boxes, refit, topology_bytes

REALS = [np.float32, np.float64]


def soup(real, seed, nv=600, nf=2000):
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1, 1, size=(nv, 3)).astype(real)
    f = rng.integers(0, nv, size=(nf, 3), dtype=np.uint32)
    f[:10, 1] = f[:10, 0]  # degenerate triangles
    return v, f


def moved(v, seed):
    rng = np.random.default_rng(seed)
    w = v + rng.normal(scale=0.2, size=v.shape).astype(v.dtype)
    w[:5] = w[0]  # a few collapsed vertices
    return w


@pytest.mark.parametrize("real", REALS, ids=["f32", "f64"])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_model_reproduces_the_reference_boxes_on_soups(oracle, real, seed):
    v, f = soup(real, seed)
    nodes, idx, _ = oracle.build(v, f)
    r = refit(nodes, idx, v, f)
    assert topology_bytes(r) == topology_bytes(nodes)
    assert_boxes_equal(r, nodes)


@pytest.mark.parametrize("real", REALS, ids=["f32", "f64"])
def test_model_reproduces_the_reference_boxes_on_c1(oracle, c1_mesh, real):
    v, f = c1_mesh
    v = v.astype(real)
    nodes, idx, _ = oracle.build(v, f)
    assert_boxes_equal(refit(nodes, idx, v, f), nodes)


@pytest.mark.parametrize("real", REALS, ids=["f32", "f64"])
def test_model_on_strided_vertices(oracle, real):
    v, f = soup(real, 4)
    vb = np.concatenate([v, np.full((v.shape[0], 1), 7, real)], axis=1)
    nodes, idx, _ = oracle.build(np.ascontiguousarray(vb), f, stride=4 * vb.dtype.itemsize)
    assert_boxes_equal(refit(nodes, idx, vb, f), nodes)


@pytest.mark.parametrize("real", REALS, ids=["f32", "f64"])
@pytest.mark.parametrize("seed", [5, 6])
def test_model_on_moved_vertices_equals_brute_force(oracle, real, seed):
    v, f = soup(real, seed, nv=300, nf=800)
    nodes, idx, _ = oracle.build(v, f)
    w = moved(v, seed + 10)
    r = refit(nodes, idx, w, f)
    assert topology_bytes(r) == topology_bytes(nodes)
    bf = brute_boxes(nodes, idx, w, f)
    for i, (lo, hi) in bf.items():
        assert np.array_equal(r["bmin"][i], lo) and np.array_equal(r["bmax"][i], hi), "node %d" % i


def test_model_empty_and_unreachable_records():
    """A hand-made tree: an empty leaf adds nothing to its parent, an unreachable record keeps its box."""
    from nanort_amd.wire import node_dtype

    real = np.float32
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5], [6, 5, 5], [5, 6, 5]], real)
    f = np.array([[0, 1, 2], [3, 4, 5]], np.uint32)
    nodes = np.zeros(5, node_dtype(real))
    nodes[0]["flag"], nodes[0]["data"] = 0, (1, 2)
    nodes[1]["flag"], nodes[1]["data"] = 1, (2, 0)
    nodes[2]["flag"], nodes[2]["data"] = 1, (0, 2)  # empty leaf
    nodes[3]["flag"], nodes[3]["data"] = 1, (1, 0)  # unreachable
    nodes[3]["bmin"], nodes[3]["bmax"] = (9, 9, 9), (10, 10, 10)
    nodes[4]["flag"], nodes[4]["data"] = 0, (3, 3)  # unreachable branch
    idx = np.array([0, 1], np.uint32)
    r = refit(nodes, idx, v, f)
    big = np.finfo(real).max
    assert np.array_equal(r["bmin"][2], [big] * 3) and np.array_equal(r["bmax"][2], [-big] * 3)
    assert np.array_equal(r["bmin"][0], [0, 0, 0]) and np.array_equal(r["bmax"][0], [6, 6, 5])
    assert r[3].tobytes() == nodes[3].tobytes() and r[4].tobytes() == nodes[4].tobytes()
