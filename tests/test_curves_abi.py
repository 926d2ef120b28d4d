"""The curve entry points of include/nanort_hip.h without a GPU: the export list, refusals that never reach HIP, the layout of
nrt_curve_hit_f32 against the header class and the numpy dtype, and the header's host classes against the C model."""
import os
import subprocess

import numpy as np
import pytest

import curves_fixture as cf
from nanort_amd import capi
from nanort_amd.wire import CURVE_HIT_F32, NODE_F32, RAY_F32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nrtSetCurves_f32", "nrtSetCurvesDevice_f32", "nrtTraverseBatchCurves_f32", "nrtTraverseBatchCurvesDevice_f32")


def test_binding_table_and_library_carry_the_four_symbols():
    header = open(os.path.join(ROOT, "include", "nanort_hip.h")).read()
    for name in NAMES:
        assert name in capi.SYMBOLS and hasattr(capi.lib(), name) and ("NRT_API nrt_status %s(" % name) in header


def test_null_context_is_refused_without_a_device():
    L = capi.lib()
    assert L.nrtSetCurves_f32(None, 16, 16, 1, 4) == capi.NRT_ERR_INVALID
    assert L.nrtSetCurves_f32(None, None, None, 0, 0) == capi.NRT_ERR_INVALID
    assert L.nrtSetCurvesDevice_f32(None, 16, 16, 1, 4, None) == capi.NRT_ERR_INVALID
    assert L.nrtTraverseBatchCurves_f32(None, 16, 1, None, 16, None) == capi.NRT_ERR_INVALID
    assert L.nrtTraverseBatchCurvesDevice_f32(None, 16, 1, None, 16, None, None) == capi.NRT_ERR_INVALID


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("curves_check") / "curves_check")
    r = subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-invalid-offsetof", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "curves_check.cc"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    return exe


def test_hit_record_layout(host_check):
    out = subprocess.run([host_check, "layout"], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    want = [40, 0, 4, 8, 12, 16, 28]
    assert [int(x) for x in out[0].split()] == want  # nanort::BezierCurveIntersection
    assert [int(x) for x in out[1].split()] == want  # nrt_curve_hit_f32
    assert [CURVE_HIT_F32.itemsize] + [CURVE_HIT_F32.fields[k][1] for k in ("t", "prim_id", "u", "v", "tangent", "normal")] == want


def run_check(exe, tmp, cps, radii, rays, subdiv):
    cb, rb, ob = (os.path.join(str(tmp), x) for x in ("curves.bin", "rays.bin", "out.bin"))
    with open(cb, "wb") as fp:
        fp.write(np.array([radii.shape[0]], dtype=np.uint32).tobytes() + np.ascontiguousarray(cps, np.float32).tobytes()
                 + np.ascontiguousarray(radii, np.float32).tobytes())
    with open(rb, "wb") as fp:
        fp.write(np.array([rays.shape[0]], dtype=np.uint64).tobytes() + np.ascontiguousarray(rays, RAY_F32).tobytes())
    r = subprocess.run([exe, "run", cb, rb, str(subdiv), ob], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    raw = open(ob, "rb").read()
    nn, ni = (int(x) for x in np.frombuffer(raw, np.uint64, 2))
    o = 16
    nodes = np.frombuffer(raw, NODE_F32, nn, o)
    o += nn * 40
    idx = np.frombuffer(raw, np.uint32, ni, o)
    o += ni * 4
    hits = np.frombuffer(raw, CURVE_HIT_F32, rays.shape[0], o)
    o += rays.shape[0] * 40
    return nodes, idx, hits, np.frombuffer(raw, np.uint8, rays.shape[0], o)


def same_hits(h, m, mh, mm):
    """The header's loop leaves a missed ray's record as constructed: flags everywhere, records where a ray hit."""
    assert np.array_equal(m, mm)
    hit = m == 1
    for f in CURVE_HIT_F32.names:
        assert np.array_equal(h[f][hit], mh[f][hit], equal_nan=True), f
    return int(hit.sum())


@pytest.mark.parametrize("scene,subdiv", [("fur", 4), ("64", 7), ("degenerate", 4)])
def test_header_host_classes_give_the_model_records(host_check, tmp_path, scene, subdiv):
    cps, radii = cf.scene(scene)
    rays = cf.all_rays()
    nodes, idx, h, m = run_check(host_check, tmp_path, cps, radii, rays, subdiv)
    mh, mm = cf.model_traverse(nodes, idx, cps, radii, rays, subdiv)
    assert same_hits(h, m, mh, mm) > (0 if scene == "degenerate" else 50)  # (not vacuous: 98 rays meet the 64 strands)
