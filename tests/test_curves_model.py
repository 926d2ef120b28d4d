"""The curve primitive, CPU side: the plain-C model (tests/curves_model.c) against the unmodified curve example of the reference
(tests/ref_curves_shim.cc, compiled where the reference tree exists; its recorded answers under tests/golden/ elsewhere), digest
for digest, on the tree the reference builds.  Every GPU parity test of tests/test_gpu_curves.py compares with this model."""
import numpy as np
import pytest

import curves_fixture as cf
from helpers import outputs_digest, reference_answers

LIVE = cf.have_reference()


@pytest.fixture(scope="module")
def rays():
    return cf.all_rays()


@pytest.mark.parametrize("name,scene,subdiv,rng", cf.CASES, ids=[c[0] for c in cf.CASES])
def test_model_matches_the_reference(name, scene, subdiv, rng, rays):
    cps, radii = cf.scene(scene)

    def live():
        a = cf.RefAccel(cps, radii)
        h, m = a.traverse(rays, subdiv, rng)
        out = a.nodes, a.indices, outputs_digest(h, m, canonical_nan=True)
        a.close()
        return out

    nodes, idx, digest = reference_answers("curves_" + name, live if LIVE else None)
    h, m = cf.model_traverse(nodes, idx, cps, radii, rays, subdiv, rng)
    assert outputs_digest(h, m, canonical_nan=True) == digest
    if scene not in ("1", "degenerate"):
        assert int(m.sum()) > 0
    miss = m == 0  # the miss record: every field as the contract says
    assert np.array_equal(h["t"][miss], rays["max_t"][miss], equal_nan=True) and np.all(h["prim_id"][miss] == 0xFFFFFFFF)
    for f in ("u", "v", "tangent", "normal"):
        assert not np.any(h[f][miss])
    if rng is not None:
        p = h["prim_id"][m == 1]
        assert p.size and np.all((p >= rng[0]) & (p < rng[1]))


def test_fur_fixture_is_what_the_example_writes_and_is_not_vacuous():
    g = cf.fur_golden()
    cam = cf.camera()
    assert g["cps"].shape == (400, 4, 3) and g["radii"].shape == (400, 4) and g["hits"].shape == (4096,)
    h, m = cf.model_traverse(g["nodes"], g["indices"], g["cps"], g["radii"], cam)
    assert h.tobytes() == g["hits"].tobytes() and np.array_equal(m, g["mask"])
    # floors observed with the reference alone (1099 hits; 196 / 230 / 263 / 410 per quarter of u)
    assert int(m.sum()) > 1000
    quarter = np.clip(np.floor(h["u"][m == 1] * 4.0), 0, 3).astype(int)
    assert np.all(np.bincount(quarter, minlength=4) >= 150)
    hit = m == 1
    assert np.allclose(np.linalg.norm(h["tangent"][hit], axis=1), 1.0, atol=1e-5)
    nl = np.linalg.norm(h["normal"][hit], axis=1)  # (a ray along the tangent has no normal: vnormalize leaves the zero vector)
    assert np.all((np.abs(nl - 1.0) < 1e-5) | (nl == 0.0)) and int((nl == 0.0).sum()) < 10
    if LIVE:  # the scene, the tree and the records come out of the example again
        L = cf.ref_lib()
        cps, radii = np.zeros((400, 4, 3), np.float32), np.zeros((400, 4), np.float32)
        assert L.refcv_fur(cf._p(cps), cf._p(radii), 400, cf.FUR_THICKNESS) == 400
        assert cps.tobytes() == g["cps"].tobytes() and radii.tobytes() == g["radii"].tobytes()
        a = cf.RefAccel(cps, radii)
        rh, rm = a.traverse(cam)
        assert rh.tobytes() == g["hits"].tobytes() and np.array_equal(rm, g["mask"]) and np.array_equal(a.indices, g["indices"])
        a.close()


def test_hostile_rays_reach_both_branches_of_the_frame():
    r = cf.hostile_rays()
    d = r["dir"]
    along_y = (d[:, 0] == 0) & (d[:, 2] == 0)
    assert np.any(along_y & (d[:, 1] > 0)) and np.any(along_y & (d[:, 1] < 0)) and np.any(along_y & (d[:, 1] == 0))
    assert np.any(np.isinf(r["max_t"])) and np.any(np.isnan(r["org"])) and np.any(np.isnan(d))
    # ... and rays along +-y do hit hair (the branch is not only taken, it produces records)
    cps, radii = cf.hair(3000)
    nodes, idx, _ = reference_answers("curves_n3000_s4")
    for sign in (1.0, -1.0):
        h, m = cf.model_traverse(nodes, idx, cps, radii, r[along_y & (d[:, 1] == sign)])
        assert 8 <= int(m.sum()) < m.shape[0]  # (three in four of them are aimed to hit)


def test_boxes_are_the_hull_of_the_control_points_grown_by_their_radii():
    cps, radii = cf.degenerate()
    lo, hi, c = cf.model_boxes(cps, radii)
    ok = ~np.isnan(cps).any(axis=(1, 2))
    assert np.array_equal(lo[ok], (cps - radii[:, :, None]).min(axis=1)[ok]) and np.array_equal(hi[ok], (cps + radii[:, :, None]).max(axis=1)[ok])
    want = (((cps[:, 0] + cps[:, 1]) + cps[:, 2]) + cps[:, 3]) / np.float32(4.0)
    assert np.array_equal(c[ok], want[ok])
