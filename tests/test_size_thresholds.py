"""The caps behind tests/test_gpu_size_thresholds.py, and its helpers, on the CPU (tests/size_thresholds.py): the sources still
state the grid caps and the piece size the GPU cases were sized to cross; the tiling puts different base rays at the same offset
of any two trips; the adopted tree of case B3 is a valid tree with one level wider than a capped refit grid; and the mesh of case
B1 builds into more reachable leaves than one trip of the leaf pass covers."""
import numpy as np
import pytest

import refit_model
import size_thresholds as sz
from bvh_check import validate_bvh
from nanort_amd import scenes


@pytest.mark.parametrize("name", list(sz.CAPS))
def test_the_sources_state_the_caps_the_gpu_cases_cross(name):
    want, fname, _, resize = sz.CAPS[name]
    got = sz.source_cap(name)
    assert got == want, "%s is %d in nanort_amd/csrc/%s, the size-threshold tests assume %d: resize %s" % (name, got, fname, want, resize)


def test_the_derived_caps_follow_from_the_constants():
    c = {k: v[0] for k, v in sz.CAPS.items()}
    assert sz.REFIT_CAP == c["kRefitMaxGrid"] * c["kRefitBlock"] == 262144
    assert sz.POST_PASS_CAP == c["post pass grid"] * 256 == 524288
    assert sz.MAX_INDEX_CAP_WORDS == c["kMeshMaxGrid"] * c["kMeshBlock"] * 4 == 2097152
    assert sz.MAX_INDEX_CAP_WORDS // 3 == 699050  # face 699 051 is the first one wholly in the second trip
    assert sz.PIECE == c["kPiece"] == 524288
    assert sz.POST_PASS_N - sz.POST_PASS_CAP >= 2 * sz.B


def test_base_length_shares_no_factor_with_a_cap():
    B = sz.B
    assert all(B % p for p in range(2, int(B ** 0.5) + 1)), "B is prime"
    for cap in (256, sz.REFIT_CAP, sz.POST_PASS_CAP, sz.PIECE):
        assert cap % B != 0
    assert (1 << 19) % B == 384


def test_tiled_repeats_the_base_in_order_and_trips_never_line_up():
    base = np.arange(sz.B, dtype=np.int64) * 7 + 3
    n = 5 * sz.PIECE + 77
    t = sz.tiled(base, n)
    assert t.shape == (n,) and np.array_equal(t[:sz.B], base) and np.array_equal(t[sz.B:2 * sz.B], base)
    assert np.array_equal(t, base[np.arange(n) % sz.B])
    assert np.array_equal(sz.tiled(base, 5), base[:5])
    # the same offset of two different pieces (or grid trips) holds different base records, at every offset and for every pair
    pieces = sz.crossing_trips(n, sz.PIECE)
    assert pieces == 6
    for a in range(pieces):
        for b in range(a + 1, pieces):
            m = min(sz.PIECE, n - b * sz.PIECE)
            assert not (t[a * sz.PIECE:a * sz.PIECE + m] == t[b * sz.PIECE:b * sz.PIECE + m]).any(), (a, b)
    m = sz.POST_PASS_N - sz.POST_PASS_CAP
    u = sz.tiled(base, sz.POST_PASS_N)
    assert not (u[:m] == u[sz.POST_PASS_CAP:]).any()
    assert np.array_equal(np.unique(u[sz.POST_PASS_CAP:], return_counts=True)[1] >= 2, np.ones(sz.B, bool))  # every base record, twice
    # structured records tile as plain ones
    rays = scenes.camera_rays(8, 8)
    assert sz.tiled(rays, 150).tobytes() == np.concatenate([rays, rays, rays[:22]]).tobytes()


def test_cut_takes_evenly_spaced_records_first_and_last_included():
    a = np.arange(31760)
    c = sz.cut(a)
    assert c.shape == (sz.B,) and c[0] == 0 and c[-1] == 31759 and (np.diff(c) >= 7).all() and (np.diff(c) <= 8).all()


def test_balanced_tree_is_valid_at_1024_leaves():
    v, f = scenes.plane(32, 16)  # 1024 triangles
    nodes, idx = sz.balanced_tree(1 << 10, np.float32, v, f)
    assert nodes.shape[0] == 2047 and np.array_equal(idx, np.arange(1024))
    i = np.arange(1023)
    assert (nodes["flag"][:1023] == 0).all() and np.array_equal(nodes["data"][:1023, 0], 2 * i + 1) and np.array_equal(nodes["data"][:1023, 1], 2 * i + 2)
    assert (nodes["flag"][1023:] == 1).all() and (nodes["data"][1023:, 0] == 1).all() and np.array_equal(nodes["data"][1023:, 1], np.arange(1024))
    lv = refit_model.levels(nodes)
    assert [len(x) for x in lv] == [1 << d for d in range(11)]
    # bvh_check reads the reference's record numbering (a low child follows its parent); heap order is another numbering of the same
    # tree, so it is given the tree renumbered, and everything else it checks (one parent per record, leaves that tile the index
    # array in order, exact boxes bottom-up, depth) is checked of this tree
    pre = sz.in_pre_order(nodes)
    m = validate_bvh(pre, idx, v, f, min_leaf=1)
    assert m["num_leaves"] == 1024 and m["max_depth"] == 10
    assert refit_model.topology_bytes(pre) != refit_model.topology_bytes(nodes)
    # every record's box, by brute force over the slots of its subtree
    brute = refit_model.brute_boxes(nodes, idx, v, f)
    for k, (lo, hi) in brute.items():
        assert np.array_equal(nodes["bmin"][k], lo) and np.array_equal(nodes["bmax"][k], hi), k
    with pytest.raises(AssertionError):
        bad = pre.copy()
        bad["bmax"][5, 0] -= 1.0
        validate_bvh(bad, idx, v, f, min_leaf=1)


def test_balanced_tree_of_2_to_the_20_leaves_has_a_level_past_the_refit_cap():
    """Case B3: one level of 524 288 branches, twice what one trip of k_plan_expand / k_refit_branches covers."""
    nodes, _ = sz.balanced_topology(1 << 20, np.float32)  # (the boxes play no part in the levels)
    lv = refit_model.levels(nodes)
    widths = [int((nodes["flag"][x] == 0).sum()) for x in lv]
    assert widths == [1 << d for d in range(20)] + [0]
    assert sz.widest_level(nodes) == 524288 > sz.REFIT_CAP
    assert sz.crossing_trips(sz.widest_level(nodes), sz.REFIT_CAP) == 2
    assert sz.reachable_leaves(nodes) == 1 << 20
    # and balanced_tree builds exactly this topology (at a size whose boxes cost nothing)
    v, f = scenes.plane(8, 4)
    small, _ = sz.balanced_tree(64, np.float32, v, f)
    assert refit_model.topology_bytes(small[:63]) == refit_model.topology_bytes(nodes[:63])


def test_the_mesh_of_case_b1_builds_into_more_leaves_than_one_trip_of_the_leaf_pass(oracle):
    v, f = scenes.plane(400, 375)
    nodes, idx, st = oracle.build(v, f, min_leaf=1)
    n = sz.reachable_leaves(nodes)
    assert n == int(st["num_leaf_nodes"]) and n > sz.REFIT_CAP, n
    assert sz.widest_level(nodes) < sz.REFIT_CAP  # (no built tree of a size a test can afford crosses the per-level cap: hence B3)


def test_per_ray_skip_equals_one_call_per_ray(oracle, c1_mesh):
    v, f = c1_mesh
    nodes, idx, _ = oracle.build(v, f)
    rays = sz.cut(scenes.camera_rays(96, 64), 257)
    h1, m1 = oracle.traverse(nodes, idx, v, f, rays)
    ids = np.where((m1 == 1) & (np.arange(257) % 2 == 1), h1["prim_id"], 0xFFFFFFFF).astype(np.uint32)
    assert (ids != 0xFFFFFFFF).sum() > 20
    h, m = sz.per_ray_skip(oracle, nodes, idx, v, f, rays, ids)
    for k in range(0, 257, 5):
        o = sz.default_trace_options()
        o["skip_prim_id"] = ids[k]
        hk, mk = oracle.traverse(nodes, idx, v, f, rays[k:k + 1], o)
        assert mk[0] == m[k] and hk.tobytes() == h[k:k + 1].tobytes()
    sel = ids != 0xFFFFFFFF
    assert (h["prim_id"][sel] != ids[sel]).all()
    assert h[~sel].tobytes() == h1[~sel].tobytes()
