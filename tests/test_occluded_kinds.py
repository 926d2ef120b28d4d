"""Occlusion queries of the sphere, cylinder and curve kinds without a GPU: the two nrtOccludedBatchPrims*_f32 entry points in the
export list, their refusals that never reach HIP, and the host statement of their contract — the generic
BVHAccel::OccludedBatch(rays, n, intersector, out) of include/nanort.h equals the flag of Traverse(), ray by ray, for the three
built-in intersectors (tests/cpp/occluded_kinds_check.cc, compiled without the backend)."""
import os
import subprocess

import numpy as np
import pytest

import curves_fixture as cf
import sphere_fixture
from nanort_amd import capi, scenes
from nanort_amd.wire import RAY_F32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nrtOccludedBatchPrims_f32", "nrtOccludedBatchPrimsDevice_f32")
SOURCE = os.path.join(ROOT, "tests", "cpp", "occluded_kinds_check.cc")
CXX = ["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), SOURCE]


def test_binding_table_and_library_carry_the_two_symbols():
    header = open(os.path.join(ROOT, "include", "nanort_hip.h")).read()
    for name in NAMES:
        assert name in capi.SYMBOLS and hasattr(capi.lib(), name) and ("NRT_API nrt_status %s(" % name) in header


def test_null_context_and_empty_batch_without_a_device():
    L = capi.lib()
    assert L.nrtOccludedBatchPrims_f32(None, 16, 1, None, 16) == capi.NRT_ERR_INVALID
    assert L.nrtOccludedBatchPrimsDevice_f32(None, 16, 1, None, 16, None) == capi.NRT_ERR_INVALID
    assert L.nrtOccludedBatchPrims_f32(None, None, 0, None, None) == capi.NRT_ERR_INVALID  # (a NULL context even with no rays)


def small_scene(kind):
    """One small scene per kind, from what sphere_fixture and curves_fixture describe, with at most 2 000 rays: (positions, radii, rays)."""
    if kind == "spheres":
        c, r = sphere_fixture.scene()
        return c, r, sphere_fixture.rays()[::16]
    if kind == "cylinders":
        v, r = scenes.random_cylinders(sphere_fixture.N_CYLINDERS)
        return v, r, sphere_fixture.rays()[::16]
    cps, radii = cf.fur()
    return cps, radii, cf.all_rays()[::3]


def run_check(exe, tmp, kind, pos, radii, rays, timeout=300):
    """Runs the program over the scene; returns the host flags of the kind's first intersector variant under the default options."""
    pb, rb, fb = (os.path.join(str(tmp), x) for x in ("prims.bin", "rays.bin", "flags.bin"))
    n = {"spheres": 1, "cylinders": 2, "curves": 4}[kind]
    radii = np.ascontiguousarray(radii, np.float32)
    with open(pb, "wb") as fp:
        fp.write(np.array([radii.size // n], dtype=np.uint32).tobytes() + np.ascontiguousarray(pos, np.float32).tobytes() + radii.tobytes())
    with open(rb, "wb") as fp:
        fp.write(np.array([rays.shape[0]], dtype=np.uint64).tobytes() + np.ascontiguousarray(rays, RAY_F32).tobytes())
    r = subprocess.run([exe, kind, pb, rb, fb], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout)
    assert r.returncode == 0 and "occluded_kinds_check ok" in r.stdout, r.stdout[-3000:]
    return np.fromfile(fb, dtype=np.uint8)


def mixed(flags):
    """At least a tenth of the rays hit and at least a tenth miss: a mask of all zeros or all ones shows nothing."""
    return flags.size >= 10 and 0.1 <= float((flags != 0).mean()) <= 0.9


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("occluded_kinds_check") / "occluded_kinds_check")
    r = subprocess.run(CXX + ["-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    return exe


@pytest.mark.parametrize("kind", ["spheres", "cylinders", "curves"])
def test_generic_occluded_batch_equals_the_traverse_flag(host_check, tmp_path, kind):
    pos, radii, rays = small_scene(kind)
    assert rays.shape[0] <= 2000
    flags = run_check(host_check, tmp_path, kind, pos, radii, rays)
    assert flags.shape[0] == rays.shape[0] and set(np.unique(flags).tolist()) <= {0, 1}
    assert mixed(flags), float(flags.mean())
