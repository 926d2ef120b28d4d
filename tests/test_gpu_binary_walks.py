"""The eleven kernels that run the binary walk (nanort_amd/csrc/binary_walk_dev.h) under odd thresholds and work splits: closest hit
with the literal walk (tunable wide = 0, k_traverse), multi-hit (k_traverse_multihit), motion closest hit / occlusion
(k_traverse_motion), masked closest hit / occlusion (k_traverse_masked), the three forms of the combined query, closest hit /
occlusion (k_traverse_query<MOTION, MASKED>) and the four of multi-hit under it (k_multihit_query<MOTION, MASKED>).  The walk's refill
gate, its early exit from the inner-node loop and the static / dynamic hand-out of rays are one piece of code under all eleven;
whatever the setting, every ray is traced exactly once and its walk is its own, so records, masks and counts equal the default
configuration's byte for byte.  (The defaults themselves are tied to the oracle by test_gpu_traverse.py, test_gpu_launch_variants.py,
test_gpu_skip_ids.py, test_gpu_multihit.py, test_gpu_motion.py, test_gpu_masks.py, test_gpu_own_walks.py, test_gpu_query.py and
test_gpu_multihit_query.py; test_work_distribution_tunables_cover_every_ray sweeps the same settings on the default wide walk.)"""
import itertools

import numpy as np
import pytest

import masks_fixture as kf
import motion_fixture as mf
from nanort_amd import BVHAccel, MotionTriangleMesh, TriangleMesh, scenes

pytestmark = pytest.mark.gpu

K = 3
# (97, 13): more than one wave, more than one chunk, a ragged end; (1, 1): one ray, 63 idle lanes, every other wave with nothing to claim
SIZES = [(97, 13), (1, 1)]
COMBOS = [dict(refill_min=1, trav_min=1), dict(refill_min=64, trav_min=64), dict(static_pct=0, chunk=16, parts=3), dict(static_pct=100),
          dict(blocks_per_cu=1, static_bands=3)]


def run_walks(plain, moving, rays, times, words, ids):
    """name -> bytes of everything the walk's launch wrote."""
    out = {}
    h, m = plain.TraverseBatch(rays)
    assert plain.LastKernelName() == "nrt::k_traverse<float>"
    out["closest"] = h.tobytes() + m.tobytes()
    h, c = plain.MultiHitTraverseBatch(rays, K)
    assert plain.LastKernelName() == "nrt::k_traverse_multihit<float>"
    out["multihit"] = h.tobytes() + c.tobytes()
    h, m = moving.TraverseBatchMotion(rays, times)
    assert moving.LastKernelName() == "nrt::k_traverse_motion<float>"
    out["motion"] = h.tobytes() + m.tobytes()
    out["motion occlusion"] = moving.OccludedBatchMotion(rays, times).tobytes()
    h, m = plain.TraverseBatchMasked(rays, words)
    assert plain.LastKernelName() == "nrt::k_traverse_masked<float>"
    out["masked"] = h.tobytes() + m.tobytes()
    out["masked occlusion"] = plain.OccludedBatchMasked(rays, words).tobytes()
    assert plain.LastKernelName() == "nrt::k_traverse_masked<float>"
    for motion, masked in itertools.product((False, True), repeat=2):  # every ray with its skip id, and with its time and / or its word
        kw = dict(times=times if motion else None, ray_masks=words if masked else None, skip_prim_ids=ids)
        form = "<float, 32, %s, %s>" % (str(motion).lower(), str(masked).lower())
        h, c = moving.MultiHitQueryBatch(rays, K, **kw)
        assert moving.LastKernelName() == "nrt::k_multihit_query" + form
        out["multihit query" + form] = h.tobytes() + c.tobytes()
        if not (motion or masked):
            continue  # (ids alone: the wide walk's, no kernel of this file's)
        h, m = moving.QueryBatch(rays, **kw)
        assert moving.LastKernelName() == "nrt::k_traverse_query" + form
        out["query" + form] = h.tobytes() + m.tobytes()
        out["query occlusion" + form] = moving.QueryBatch(rays, occlusion=True, **kw).tobytes()
        assert moving.LastKernelName() == "nrt::k_traverse_query" + form
    return out


@pytest.fixture(scope="module")
def world():
    v, f = scenes.plane(120, 60)
    v = np.ascontiguousarray(v, dtype=np.float32)
    plain, moving = BVHAccel(np.float32), BVHAccel(np.float32)
    assert plain.Build(f.shape[0], TriangleMesh(v, f))
    plain.SetTunable("wide", 0)
    plain.SetPrimMasks(kf.prim_patterns(f.shape[0])["random"])
    assert moving.Build(f.shape[0], MotionTriangleMesh(v, mf.deformations(v)["wave"], f))
    moving.SetPrimMasks(kf.prim_patterns(f.shape[0])["random"])
    cases = {}
    for size in SIZES:
        rays = scenes.camera_rays(*size)
        times = mf.assign_times(rays.shape[0], np.float32)
        words = kf.assign_ray_masks(rays.shape[0])
        h, m = moving.QueryBatch(rays, times=times, ray_masks=words)
        ids = np.where(m != 0, h["prim_id"], 0xFFFFFFFF).astype(np.uint32)  # every ray skips the triangle it would hit
        cases[size] = (rays, times, words, ids, run_walks(plain, moving, rays, times, words, ids))  # under the default tunables, computed once
    rays, times, words, ids, _ = cases[SIZES[0]]
    h, m = moving.QueryBatch(rays, times=times, ray_masks=words)
    ih, im = moving.QueryBatch(rays, times=times, ray_masks=words, skip_prim_ids=ids)
    assert 0 < int(m.sum()) and int(mf.differs(ih, im, h, m).sum()) > 0  # (not vacuous: the ids change records)
    h, m = plain.TraverseBatch(rays)
    assert 0 < int(m.sum())  # (not vacuous: rays hit the mesh)
    kh, km = plain.TraverseBatchMasked(rays, words)
    assert 0 < int(km.sum()) and int(mf.differs(kh, km, h, m).sum()) > 0  # (... also through the masks, which change records)
    yield plain, moving, cases
    plain.close()
    moving.close()


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: ",".join("%s=%d" % kv for kv in c.items()))
def test_thresholds_and_work_split_leave_every_record_as_it_is(world, combo, size):
    plain, moving, cases = world
    rays, times, words, ids, ref = cases[size]
    saved = [(a, k, a.GetTunable(k)) for a in (plain, moving) for k in combo]
    try:
        for a in (plain, moving):
            for k, val in combo.items():
                a.SetTunable(k, val)
        got = run_walks(plain, moving, rays, times, words, ids)
    finally:
        for a, k, val in saved:
            a.SetTunable(k, val)
    for name in ref:
        assert got[name] == ref[name], (name, size, combo)
