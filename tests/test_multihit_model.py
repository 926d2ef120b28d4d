"""CPU pins of the multi-hit model (tests/multihit_model.c, the contract of include/nanort_hip.h nrtMultiHitTraverseBatch*):
at K = 1 it is the closest-hit oracle up to exact-t ties, at K = 64 it is the brute-force enumeration of every primitive."""
import numpy as np
import pytest

from multihit_fixture import brute, check_k1_against_closest, header_check, hits_bytes, hostile_rays, model, random_window_rays, soup, tie_checker
from nanort_amd import scenes
from nanort_amd.wire import widen_rays


def c1_case(oracle, c1_mesh, real):
    v, f = c1_mesh
    v = v.astype(real)
    nodes, idx, _ = oracle.build(v, f)
    rays = scenes.camera_rays(96, 54)
    if real == np.float64:
        rays = widen_rays(rays)
    return v, f, None, nodes, idx, rays


def soup_case(oracle, real):
    v, f, stride = soup(real)
    nodes, idx, _ = oracle.build(v, f, stride=stride)
    return v, f, stride, nodes, idx, hostile_rays(real, 3000)


@pytest.mark.parametrize("real", [np.float32, np.float64])
@pytest.mark.parametrize("case", ["c1", "soup"])
def test_k1_is_the_closest_hit_oracle(oracle, c1_mesh, real, case):
    v, f, stride, nodes, idx, rays = c1_case(oracle, c1_mesh, real) if case == "c1" else soup_case(oracle, real)
    for cull in (0, 1):
        opts = None
        if cull:
            from helpers import trace_options

            opts = trace_options(cull=True)
        ch, cm = oracle.traverse(nodes, idx, v, f, rays, opts, stride=stride)
        h, c = model(nodes, idx, v, f, rays, 1, opts, stride)
        assert cm.any()
        check_k1_against_closest(h, c, ch, cm, tie_checker(v, f, rays, opts, stride))


@pytest.mark.parametrize("real", [np.float32, np.float64])
@pytest.mark.parametrize("case", ["c1", "soup"])
def test_k64_is_the_brute_force_enumeration(oracle, c1_mesh, real, case):
    v, f, stride, nodes, idx, rays = c1_case(oracle, c1_mesh, real) if case == "c1" else soup_case(oracle, real)
    h, c = model(nodes, idx, v, f, rays, 64, None, stride)
    bh, bc = brute(v, f, rays, 64, None, stride)
    assert np.array_equal(c, bc)
    assert hits_bytes(h) == hits_bytes(bh)
    assert c.max() > 3  # rays through several surfaces


def test_rows_are_sorted_and_padded_with_miss_records(oracle, c1_mesh):
    v, f, stride, nodes, idx, rays = c1_case(oracle, c1_mesh, np.float32)
    K = 8
    h, c = model(nodes, idx, v, f, rays, K)
    for i in range(rays.shape[0]):
        row = h[i]
        held = row[: c[i]]
        keys = list(zip(held["t"].tolist(), held["prim_id"].tolist()))
        assert keys == sorted(keys)
        assert (held["t"] < rays["max_t"][i]).all() and (held["t"] >= rays["min_t"][i]).all()
        miss = row[c[i]:]
        assert (miss["prim_id"] == 0xFFFFFFFF).all() and (miss["t"] == rays["max_t"][i]).all()
        assert (miss["u"] == 0).all() and (miss["v"] == 0).all()


def test_prefix_property_across_k(oracle, c1_mesh):
    """The K smallest keys: the first j records of a row at K are the row at j (the walk reaches every candidate leaf)."""
    v, f, stride, nodes, idx, rays = c1_case(oracle, c1_mesh, np.float64)
    h64, c64 = model(nodes, idx, v, f, rays, 64)
    for K in (1, 2, 3, 8):
        h, c = model(nodes, idx, v, f, rays, K)
        assert np.array_equal(c, np.minimum(c64, K))
        for i in np.nonzero(c)[0][::7]:
            assert hits_bytes(h[i, : c[i]]) == hits_bytes(h64[i, : c[i]])


@pytest.mark.parametrize("K", [1, 3, 8])
def test_header_host_multihit_traverse_equals_the_model(tmp_path, c1_mesh, K):
    """include/nanort.h MultiHitTraverse (host build, no backend) on its own tree equals the model on GetNodes() / GetIndices()."""
    v, f = c1_mesh
    rays = np.concatenate([scenes.camera_rays(64, 36), random_window_rays(scenes.camera_rays(48, 27), 3)])
    counts, rows, nodes, idx = header_check(str(tmp_path), v, f, rays, K)
    mh, mc = model(nodes, idx, v, f, rays, K)
    assert np.array_equal(counts, mc)
    assert hits_bytes(rows) == hits_bytes(mh)
    assert counts.max() >= min(K, 3)
