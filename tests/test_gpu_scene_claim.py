"""The per-partition ray claim of the scene kernels (scene_kernels.hip scene_claim_ray: one statement for k_scene_trace and
k_scene_walk) at the batch sizes where a partition cursor can drop or double a ray: one ray, one ray past a wave, nine blocks
with a last partition one ray longer than the others, a partition length that is no multiple of 64.  Through the
device-resident entry points, into buffers pre-filled with 0xCD: every record and every flag is the restatement's
(oracle/nanosg_oracle.c, same local trees), so no ray was skipped (its 0xCD record would survive) and none was traced into
another ray's slot; nothing is written behind the n-th record or flag.  Repeated with the wave's refill threshold at 1 and 64."""
import numpy as np
import pytest

from nanort_amd import BVHAccel, Scene, TriangleMesh, scenes
from nanort_amd.wire import RAY_F32, SCENE_HIT_F32
from oracle import bindings as ob
from scene_fixture import xform

pytestmark = pytest.mark.gpu

COUNTS = (1, 65, 2049, 2303)
KEYS = ("t", "u", "v", "prim_id", "node_id")
SLACK = 64  # records / flags behind the batch that must stay untouched


@pytest.fixture(scope="module")
def material(oracle):
    """{instances: (scene, restatement's records, flags)} for 70 instances (the walk, or the listing path over the top-level
    tree) and 5 (the fused scan), and the one ray set, aimed at the crowd, whose first n rays every case uses."""
    rng = np.random.default_rng(77)
    sv, sf = scenes.sphere(8, 4)
    sv = (sv - np.array([0, 5, 0], dtype=np.float32)).astype(np.float32)  # (about the origin, radius 7.5)
    a = BVHAccel(np.float32)
    assert a.Build(sf.shape[0], TriangleMesh(sv, sf))
    tree = a.GetTree()
    n = max(COUNTS)
    org = rng.uniform(-7, 7, size=(n, 3))
    tgt = rng.uniform(-3, 3, size=(n, 3))
    d = tgt - org
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros(n, dtype=RAY_F32)
    rays["org"] = org.astype(np.float32)
    rays["dir"] = d.astype(np.float32)
    rays["max_t"] = 3.0e38
    out = {"rays": rays, "keep": a}
    for count in (70, 5):
        sc = Scene()
        O = ob.SceneOracle(oracle)
        for _ in range(count):
            x = xform(tuple(rng.uniform(0.04, 0.12, 3) * (1 if count == 70 else 3)), rng.uniform(0, 6.28), rng.uniform(0, 6.28), tuple(rng.uniform(-3, 3, 3)))
            sc.AddNode(a, x)
            O.add_node(sv, sf, x, tree=tree)
        assert sc.Commit() and O.commit()
        oh, om = O.traverse(rays)
        assert 0.1 < om.mean() < 0.9 and om[0] == 1, om.mean()  # both outcomes among the rays; n = 1: a hit, more than the miss record
        out[count] = (sc, oh, om)
    return out


# (instances, single_pass, the refill tunable of the kernel that path claims rays in, LastPath)
PATHS = {"walk": (70, 2, "walk_refill_min", 1), "listing": (70, 0, "refill_min", 0), "fused_scan": (5, 1, "refill_min", 0)}


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("path", sorted(PATHS))
def test_every_ray_claimed_once(material, path, n):
    import torch

    count, single_pass, refill, last_path = PATHS[path]
    sc, oh, om = material[count]
    rays = material["rays"][:n]
    sc.SetTunable("single_pass", single_pass)
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    d_hits = torch.empty((n + SLACK) * SCENE_HIT_F32.itemsize, dtype=torch.uint8, device="cuda")
    d_mask = torch.empty(n + SLACK, dtype=torch.uint8, device="cuda")
    for value in (None, 1, 64):
        if value is not None:
            sc.SetTunable(refill, value)
        for occluded in (False, True):
            d_hits.fill_(0xCD)
            d_mask.fill_(0xCD)
            if occluded:
                sc.OccludedBatchDevice(d_rays, d_mask)
            else:
                sc.TraverseBatchDevice(d_rays, d_hits, d_mask)
            what = (path, n, value, occluded)
            assert sc.LastPath() == last_path, what
            h = d_hits.cpu().numpy()
            m = d_mask.cpu().numpy()
            assert np.array_equal(m[:n], om[:n]), what
            assert (m[n:] == 0xCD).all(), what
            if occluded:  # no record is written by the occlusion form
                assert (h == 0xCD).all(), what
            else:
                rec = h[:n * SCENE_HIT_F32.itemsize].view(SCENE_HIT_F32)
                for k in KEYS:
                    assert np.ascontiguousarray(rec[k]).tobytes() == np.ascontiguousarray(oh[k][:n]).tobytes(), (what, k)
                assert (h[n * SCENE_HIT_F32.itemsize:] == 0xCD).all(), what
    sc.SetTunable(refill, 56 if refill == "refill_min" else 24)  # the defaults, for the cases that share the scene
