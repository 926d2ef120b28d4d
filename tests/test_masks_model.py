"""Visibility masks without a GPU (include/nanort_hip.h, "visibility masks"): the expectation of
tests/masks_fixture.py against an independent statement, the fixture condition that makes the GPU tests able to see a walk that
ignores the masks or rejects everything, include/nanort.h's MaskedTriangleIntersector on the host, and the ten new symbols in the
binding table, the header and the library."""
import os
import subprocess

import numpy as np
import pytest

import masks_fixture as kf
import motion_fixture as mf
from helpers import assert_hits_identical, assert_hits_match, trace_options
from nanort_amd import capi, scenes
from nanort_amd.wire import hit_dtype, ray_dtype, widen_rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REALS = [np.float32, np.float64]
UNSUFFIXED = ("nrtSetPrimMasks", "nrtSetPrimMasksDevice")
NAMES = UNSUFFIXED + tuple(base + sfx for base in ("nrtTraverseBatchMasked_", "nrtTraverseBatchMaskedDevice_", "nrtOccludedBatchMasked_",
                                                    "nrtOccludedBatchMaskedDevice_") for sfx in ("f32", "f64"))


@pytest.fixture(scope="module")
def world(oracle, c1_mesh):
    v, f = c1_mesh
    nodes, idx, _ = oracle.build(v, f)
    return v, f, nodes, idx, scenes.camera_rays(96, 64)


def test_fixture_values_and_assignment():
    w = kf.assign_ray_masks(4099)
    assert w.dtype == np.uint32 and (w[1:] != w[:-1]).all()
    assert sorted(np.unique(w)) == sorted(kf.RAY_MASK_VALUES)
    p = kf.prim_patterns(1000)
    assert sorted(p) == ["bit31", "mod3", "ones", "random", "zeros"]
    assert all(a.dtype == np.uint32 and a.shape == (1000,) for a in p.values())
    assert np.array_equal(p["mod3"][:4], [1, 2, 4, 1]) and (p["bit31"] == 0x80000000).all()
    for bit in range(32):  # every bit of the random words hides about half of the mesh
        assert 400 < int(kf.visible(p["random"], 1 << bit).sum()) < 600, bit
    f = np.arange(12, dtype=np.uint32).reshape(4, 3)
    f_m = kf.hidden_faces(f, np.array([1, 2, 3, 0], dtype=np.uint32), 2)
    assert np.array_equal(f_m, [[0, 0, 0], [3, 4, 5], [6, 7, 8], [9, 9, 9]])


# ---- 1. the expectation against an independent statement ---------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["random", "mod3"])
def test_expectation_equals_a_tree_over_the_visible_faces_alone(oracle, world, pattern):
    """Per mask group: the oracle builds its own tree over only the faces the group sees and traces it; prim ids mapped back.  The
    trees differ, so the comparison is the topology-independent one (helpers.assert_hits_match: flags and t bit-equal, prim_id / u /
    v too except at exact ties, each of which is verified)."""
    v, f, nodes, idx, rays = world
    pm = kf.prim_patterns(f.shape[0])[pattern]
    words = kf.assign_ray_masks(rays.shape[0])
    eh, em = kf.expected(oracle, nodes, idx, v, f, pm, rays, words)
    seen_groups = 0
    for m in np.unique(words):
        sel = np.nonzero(words == m)[0]
        r = np.ascontiguousarray(rays[sel])
        keep = np.nonzero(kf.visible(pm, m))[0]
        if keep.size == 0:
            ih, im = kf.miss_records(r, np.float32)
        else:
            f_vis = np.ascontiguousarray(f[keep])
            n2, i2, _ = oracle.build(v, f_vis)
            ih, im = oracle.traverse(n2, i2, v, f_vis, r)
            ih = ih.copy()
            hit = im != 0
            ih["prim_id"][hit] = keep[ih["prim_id"][hit]].astype(np.uint32)
            seen_groups += 1
        assert_hits_match(ih, im, eh[sel], em[sel], oracle, nodes, idx, v, kf.hidden_faces(f, pm, m), r)
    assert seen_groups >= (7 if pattern == "random" else 5)  # (mod3: bits 0..2 only — the words 0, 0x80000000 and 0x00010000 see nothing)
    assert em.sum() > 100


# ---- 2. the fixture condition ------------------------------------------------------------------------------------------------------
def test_fixture_condition_the_masks_matter(oracle, world):
    """With the random prim masks and the ray mask 1 at least a tenth of the rays get a record that differs both from the unmasked
    record and from a miss: a walk that ignored the masks, or rejected everything, fails the GPU tests.

    The rays are masks_fixture.through_rays, which the GPU tests trace beside motion's three sets — not the camera set: C1 is one layer
    deep seen from its camera (an open box and a small mesh inside), so a camera ray whose first hit is hidden misses, and the share
    that is BOTH different from the unmasked record and a hit is 0.0 ... 1.7 % over the seeds 0 .. 63 (1.7 % with SEED), whatever the
    seed.  On the camera set each half of the condition is asserted on its own."""
    v, f, nodes, idx, cam = world
    pm = kf.random_prim_masks(f.shape[0])

    def shares(rays):
        n = rays.shape[0]
        h1, m1 = kf.expected(oracle, nodes, idx, v, f, pm, rays, np.full(n, 1, dtype=np.uint32))
        h0, m0 = oracle.traverse(nodes, idx, v, f, rays)
        hm, mm = kf.miss_records(rays, np.float32)
        d0, dm = mf.differs(h1, m1, h0, m0), mf.differs(h1, m1, hm, mm)
        return float((d0 & dm).mean()), float(d0.mean()), float(dm.mean())

    both, _, _ = shares(kf.through_rays(cam))
    assert both >= 0.10, both
    _, not_unmasked, not_miss = shares(cam)
    assert not_unmasked >= 0.10 and not_miss >= 0.10, (not_unmasked, not_miss)


def test_all_ones_is_the_plain_query_and_zero_sees_nothing(oracle, world):
    v, f, nodes, idx, rays = world
    pat = kf.prim_patterns(f.shape[0])
    h0, m0 = oracle.traverse(nodes, idx, v, f, rays)
    assert_hits_identical(h0, m0, *kf.expected(oracle, nodes, idx, v, f, pat["ones"], rays, None))
    hm, mm = kf.miss_records(rays, np.float32)
    assert_hits_identical(hm, mm, *kf.expected(oracle, nodes, idx, v, f, pat["zeros"], rays, None))
    assert_hits_identical(hm, mm, *kf.expected(oracle, nodes, idx, v, f, pat["random"], rays, np.zeros(rays.shape[0], dtype=np.uint32)))


@pytest.mark.parametrize("real", REALS, ids=["f32", "f64"])
def test_fixture_conditions_of_the_own_walk_tests(oracle, real):
    """What tests/test_gpu_own_walks.py rests on, from the reference alone (measured, f32 and f64 alike unless said): the pile's tree is
    138 deep and the walk's max-stack counter is 137 for each of the eight ray words — past the masked walk's 32 LDS entries — with
    the random and with the mod3 prim words; with the random words 1318 of the 1500 rays hit and 667 get a hit on another primitive
    than the unmasked record's (a quarter is asked for).  Over the soup 975 of the 6000 hostile rays hit through the masks and 288
    (f64: 286) hit another primitive than without them (150 asked for)."""
    import own_walks_fixture as ow

    v, f, rays, words = ow.pile(real)
    nodes, idx, st = oracle.build(v, f)
    assert st["max_tree_depth"] > ow.PILE_MIN_STACK
    assert sorted(np.unique(words)) == sorted(kf.RAY_MASK_VALUES)
    for name in ("random", "mod3"):
        pm = kf.prim_patterns(f.shape[0])[name]
        _, _, depth, hits, other = ow.masked_figures(oracle, nodes, idx, v, f, pm, rays, words)
        assert len(depth) == len(kf.RAY_MASK_VALUES) and min(depth.values()) > ow.PILE_MIN_STACK, (name, depth)
        assert hits > 0
        if name == "random":
            assert other >= ow.PILE_MIN_OTHER, other
    vbuf, f, stride, rays, words, pm = ow.soup_masked(real)
    nodes, idx, _ = oracle.build(vbuf, f, stride=stride)
    _, _, _, hits, other = ow.masked_figures(oracle, nodes, idx, vbuf, f, pm, rays, words, stride)
    assert hits > 0 and other >= ow.SOUP_MIN_OTHER, (hits, other)


# ---- 3. include/nanort.h, MaskedTriangleIntersector on the host ------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("masks_host_check") / "masks_host_check")
    r = subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "masks_host_check.cc"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    return exe


OPTIONS = {
    "default": dict(),
    "all": dict(range_=(50, 900), skip=412, cull=True),
}


@pytest.mark.parametrize("opt", sorted(OPTIONS))
@pytest.mark.parametrize("real", REALS, ids=["f32", "f64"])
def test_header_intersector_equals_the_expectation_on_the_oracles_tree(oracle, host_check, tmp_path, c1_mesh, real, opt):
    v, f = c1_mesh
    v = np.ascontiguousarray(v.astype(real))
    f = np.ascontiguousarray(f, dtype=np.uint32)
    nodes, idx, _ = oracle.build(v, f)
    cam = scenes.camera_rays(48, 32)
    rays = np.ascontiguousarray(widen_rays(cam) if real == np.float64 else cam, dtype=ray_dtype(real))
    words = kf.assign_ray_masks(rays.shape[0])
    pm = kf.prim_patterns(f.shape[0])["mod3" if opt == "all" else "random"]
    o = trace_options(**OPTIONS[opt])
    mesh, tree, rp, out = (os.path.join(str(tmp_path), x) for x in ("mesh.bin", "tree.bin", "rays.bin", "out.bin"))
    with open(mesh, "wb") as fp:
        fp.write(np.array([v.shape[0], f.shape[0]], dtype=np.uint32).tobytes() + v.tobytes() + f.tobytes() + pm.tobytes())
    with open(tree, "wb") as fp:  # BVHAccel::Load's format
        fp.write(np.array([nodes.shape[0]], dtype=np.uint64).tobytes() + np.ascontiguousarray(nodes).tobytes()
                 + np.array([idx.shape[0]], dtype=np.uint64).tobytes() + np.ascontiguousarray(idx, dtype=np.uint32).tobytes())
    with open(rp, "wb") as fp:
        fp.write(np.array([rays.shape[0]], dtype=np.uint64).tobytes() + rays.tobytes() + words.tobytes())
    oo = o[()] if o.shape == () else o[0]
    r = subprocess.run([host_check, "f32" if real == np.float32 else "f64", mesh, tree, rp, out, str(int(oo["prim_ids_range"][0])),
                        str(int(oo["prim_ids_range"][1])), str(int(oo["skip_prim_id"])), str(int(oo["cull_back_face"]))],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    raw = open(out, "rb").read()
    H = hit_dtype(real)
    n = rays.shape[0]
    h = np.frombuffer(raw, H, n, 0)
    m = np.frombuffer(raw, np.uint8, n, n * H.itemsize)
    eh, em = kf.expected(oracle, nodes, idx, v, f, pm, rays, words, o)
    assert em.sum() > (100 if opt == "default" else 0)  # (culling leaves little of a box seen from inside)
    assert_hits_identical(eh, em, h, m)


# ---- 4. the binding table, the header and the library -----------------------------------------------------------------------------
def test_binding_table_header_and_library_carry_the_ten_symbols():
    header = open(os.path.join(ROOT, "include", "nanort_hip.h")).read()
    assert len(NAMES) == 10
    for name in NAMES:
        assert name in capi.SYMBOLS and hasattr(capi.lib(), name) and ("NRT_API nrt_status %s(" % name) in header, name
    L = capi.lib()
    want = {"nrtSetPrimMasks": 3, "nrtSetPrimMasksDevice": 4, "nrtTraverseBatchMasked": 7, "nrtTraverseBatchMaskedDevice": 8,
            "nrtOccludedBatchMasked": 6, "nrtOccludedBatchMaskedDevice": 7}
    for name in NAMES:
        assert len(getattr(L, name).argtypes) == want[name.rsplit("_f", 1)[0]], name


def test_exports_equal_the_declarations():
    """nm -D of the library: exactly the symbols the header declares."""
    r = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True)
    exported = sorted(line.split()[-1] for line in r.stdout.splitlines() if line.split()[-2:-1] == ["T"] and line.split()[-1].startswith("nrt"))
    assert exported == sorted(capi.SYMBOLS)


def test_null_context_is_refused_without_a_device():
    L = capi.lib()
    assert L.nrtSetPrimMasks(None, 16, 1) == capi.NRT_ERR_INVALID
    assert L.nrtSetPrimMasks(None, None, 0) == capi.NRT_ERR_INVALID
    assert L.nrtSetPrimMasksDevice(None, 16, 1, None) == capi.NRT_ERR_INVALID
    for s in ("f32", "f64"):
        assert getattr(L, "nrtTraverseBatchMasked_" + s)(None, 16, 16, 1, None, 16, None) == capi.NRT_ERR_INVALID
        assert getattr(L, "nrtTraverseBatchMaskedDevice_" + s)(None, 16, 16, 1, None, 16, None, None) == capi.NRT_ERR_INVALID
        assert getattr(L, "nrtOccludedBatchMasked_" + s)(None, 16, 16, 1, None, 16) == capi.NRT_ERR_INVALID
        assert getattr(L, "nrtOccludedBatchMaskedDevice_" + s)(None, 16, 16, 1, None, 16, None) == capi.NRT_ERR_INVALID
