"""include/nanort.h's HIP-backed BVHAccel across the states a C++ application can put it in: copies and rebuilds of either
side, Load() into a copy, the cylinder cap flag, moves, std::vector growth, primitive-kind changes, an empty rebuild,
concurrent batch calls, and a motion mesh with masks and a curve accel through a move, a copy and a copy-on-write detach
(tests/cpp/accel_lifecycle_check.cc).  After every step every live accel's batch methods must
return exactly what the same object's per-ray host walk returns on its own tree, or refuse where the contract says so;
the original's records of one scenario are also checked against the oracle on its read-back tree."""
import os
import subprocess

import numpy as np
import pytest

import curves_fixture
import masks_fixture
import motion_fixture
from nanort_amd import scenes
from nanort_amd.wire import HIT_F32, HIT_F64, NODE_F32, NODE_F64, widen_rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
LIBDIR = os.path.join(ROOT, "nanort_amd", "lib")
SRC = os.path.join(ROOT, "tests", "cpp", "accel_lifecycle_check.cc")

# scenario -> (precisions, refusals the contract documents in one run, time limit in seconds)
SCENARIOS = {
    "batch_first": (("f32", "f64"), {"f32": 0, "f64": 0}, 120),
    "cyl_cap_first": (("f32",), {"f32": 0}, 120),
    "copy_then_rebuild_copy": (("f32", "f64"), {"f32": 0, "f64": 0}, 120),
    "copy_then_rebuild_original": (("f32", "f64"), {"f32": 0, "f64": 0}, 120),
    "copy_then_kind_change": (("f32",), {"f32": 0}, 120),
    "copy_then_load": (("f32", "f64"), {"f32": 0, "f64": 0}, 120),
    "copy_cyl_cap_flip": (("f32",), {"f32": 0}, 120),
    # the moved-from object: all eight triangle batch entry points refuse
    "move": (("f32", "f64"), {"f32": 8, "f64": 8}, 120),
    "vector_growth": (("f32", "f64"), {"f32": 0, "f64": 0}, 180),
    # triangles: the sphere and cylinder overloads (2); spheres: the eight triangle entries and the cylinder overload (9);
    # cylinders: the eight and the sphere overload (9); triangles again (2)
    "kind_cycle": (("f32",), {"f32": 22}, 120),
    # after Build(0, ...): the eight triangle entries (+ the sphere and cylinder overloads in fp32)
    "empty_rebuild": (("f32", "f64"), {"f32": 10, "f64": 8}, 120),
    # after Load(): OccludedBatch and the four device entries until one TraverseBatch() has run
    "load_refusals": (("f32", "f64"), {"f32": 5, "f64": 5}, 120),
    "threads_same_object": (("f32", "f64"), {"f32": 0, "f64": 0}, 120),
    "threads_copies": (("f32", "f64"), {"f32": 0, "f64": 0}, 120),
    # the copy / move scenarios with NANORT_HIP_DEVICES=0,0 (the moved-from object's eight refusals)
    "replicas": (("f32", "f64"), {"f32": 8, "f64": 8}, 420),
    # a MotionTriangleMesh accel that holds masks, moved, moved again, copied and detached by SetPrimMasks(): the four motion /
    # masked queries of the two moved-from objects (4 + 8 + 8) and the two masked queries after a Build() dropped the masks
    "motion_masks": (("f32", "f64"), {"f32": 22, "f64": 22}, 120),
    # a curve accel the same way, detached by another subdivision count: TraverseBatch(BezierCurveIntersection*) and
    # OccludedBatchCurves of the two moved-from objects (2 + 4 + 4)
    "curve_subdiv": (("f32",), {"f32": 10}, 120),
}


def compile_driver(exe):
    args = ["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-DNANORT_USE_HIP_BACKEND", "-DNANORT_ENABLE_SERIALIZATION", "-pthread",
            "-D__HIP_PLATFORM_AMD__", "-I", INC, "-isystem", "/opt/rocm/include", SRC, "-o", str(exe),
            "-L", LIBDIR, "-lnanort_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"]
    r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, "g++ failed:\n" + r.stdout[-3000:]
    return str(exe)


def test_lifecycle_driver_builds_and_lists_its_scenarios(tmp_path):
    """No GPU needed: the driver compiles against the header and `--list` names every scenario without a HIP call."""
    exe = compile_driver(tmp_path / "accel_lifecycle_check")
    r = subprocess.run([exe, "--list"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0, r.stdout
    listed = dict(line.split() for line in r.stdout.strip().splitlines())
    assert listed == {name: ",".join(p) for name, (p, _, _) in SCENARIOS.items()}


def _mesh_file(path, v, f):
    with open(path, "wb") as fp:
        fp.write(np.array([v.shape[0], f.shape[0]], dtype=np.uint32).tobytes())
        fp.write(np.ascontiguousarray(v, dtype=np.float32).tobytes())
        fp.write(np.ascontiguousarray(f, dtype=np.uint32).tobytes())


def _rays_file(path, rays):
    with open(path, "wb") as fp:
        fp.write(np.array([rays.shape[0]], dtype=np.uint64).tobytes())
        fp.write(rays.tobytes())


def _prims_file(path, a, b):
    with open(path, "wb") as fp:
        fp.write(np.array([b.shape[0]], dtype=np.uint32).tobytes())
        fp.write(np.ascontiguousarray(a, dtype=np.float32).tobytes())
        fp.write(np.ascontiguousarray(b, dtype=np.float32).tobytes())


def _motion_file(path, v0, v1, f, masks, other):
    with open(path, "wb") as fp:
        fp.write(np.array([v0.shape[0], f.shape[0]], dtype=np.uint32).tobytes())
        for a in (v0, v1):
            fp.write(np.ascontiguousarray(a, dtype=np.float32).tobytes())
        for a in (f, masks, other):
            fp.write(np.ascontiguousarray(a, dtype=np.uint32).tobytes())


@pytest.fixture(scope="module")
def lifecycle(tmp_path_factory):
    d = tmp_path_factory.mktemp("lifecycle")
    exe = compile_driver(d / "accel_lifecycle_check")
    va, fa = scenes.sphere(128, 64)
    vb, fb = scenes.sphere(96, 48)  # another face count, moved off the first
    vb = vb + np.array([0.05, -0.04, 0.03], dtype=np.float32)
    _mesh_file(d / "mesh_a.bin", va, fa)
    _mesh_file(d / "mesh_b.bin", vb, fb)
    rays = scenes.camera_rays(160, 90)
    _rays_file(d / "rays.bin", rays)
    _rays_file(d / "prays.bin", scenes.particle_camera_rays(160, 90))
    _prims_file(d / "spheres.bin", *scenes.random_spheres(3000))
    _prims_file(d / "cylinders.bin", *scenes.random_cylinders(2000))
    # motion_masks: C1 (980 faces) with the wave deformation as keyframe 1, two sets of random masks (every bit hides about half
    # of the faces), 2000 camera rays turned to look through the box's side walls (the camera's own rays meet one layer of geometry
    # nearly everywhere: under a tenth of them can tell masked from unmasked); curve_subdiv: 100 strands of synthetic hair under the curve camera moved in, 2025 rays
    vm, fm = scenes.load_c1_mesh()
    _motion_file(d / "motion.bin", vm, motion_fixture.deformations(vm)["wave"], fm, masks_fixture.random_prim_masks(fm.shape[0]),
                 masks_fixture.random_prim_masks(fm.shape[0], masks_fixture.SEED + 1))
    _rays_file(d / "mrays.bin", masks_fixture.through_rays(scenes.camera_rays(50, 40)))
    _prims_file(d / "curves.bin", *curves_fixture.hair(100))
    crays = curves_fixture.camera(45, 45)
    crays["org"][:, 2] = 9.0  # (from z = 20: the ball and its hair, 5.5 in radius, more than fill the frame; a 30th of the rays hit before)
    _rays_file(d / "crays.bin", crays)
    return exe, d, (va, fa), rays


def test_lifecycle_fixture_tells_keyframes_masks_and_subdivisions_apart(lifecycle):
    """No GPU needed: over host-built trees and through the header's host classes alone, at least a tenth of the motion_masks rays
    answer differently at time 0.5 than at time 0, with the masks than without and with the other masks than with the first, and
    at least a tenth of the curve_subdiv rays differ between 2 and 4 subdivisions — an object that traced against the wrong
    keyframe, words or count after a copy, a move or a detach cannot pass its scenario."""
    exe, d, _, _ = lifecycle
    r = subprocess.run([exe, "--fixture", str(d)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("fixture ")]
    assert [ln[1:3] for ln in lines] == [["motion", "f32"], ["motion", "f64"], ["curves", "rays"]]
    for ln in lines[:2]:
        got = dict(zip(ln[3::2], ln[4::2]))
        assert 1500 <= int(got["rays"]) <= 2500 and 200 <= int(got["faces"]) <= 1000
        for what in ("time", "masks", "other_masks"):
            assert float(got[what]) >= 0.1, (ln[2], what, got[what])
    got = dict(zip(lines[2][2::2], lines[2][3::2]))
    assert 1500 <= int(got["rays"]) <= 2500 and int(got["curves"]) == 100
    assert float(got["hit"]) >= 0.1 and float(got["subdivisions"]) >= 0.1, got


def _run(lifecycle, name, prec, *extra):
    exe, d, _, _ = lifecycle
    r = subprocess.run([exe, name, prec, str(d)] + list(extra), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=SCENARIOS[name][2])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("scenario ")]
    assert lines, "no result line (exit %d):\n%s" % (r.returncode, r.stdout[-4000:])
    w = lines[-1].split()
    return r, int(w[3]), int(w[5]), int(w[7])


@pytest.mark.gpu
@pytest.mark.parametrize("name,prec", [(n, p) for n, (ps, _, _) in SCENARIOS.items() for p in ps])
def test_accel_lifecycle(lifecycle, name, prec):
    r, checks, mismatches, refused = _run(lifecycle, name, prec)
    print(r.stdout)
    assert mismatches == 0 and r.returncode == 0, r.stdout[-4000:]
    assert refused == SCENARIOS[name][1][prec], r.stdout[-4000:]
    assert checks > 0


@pytest.mark.gpu
@pytest.mark.parametrize("f64", [False, True])
def test_copy_rebuilt_original_matches_the_oracle(lifecycle, oracle, f64):
    """copy_then_rebuild_copy: after its copies were rebuilt over another mesh, the original's TraverseBatch records equal the
    oracle's walk of the original's own (read-back) tree over the original's mesh — every field, bit for bit."""
    _, d, (v, f), rays = lifecycle
    out = os.path.join(str(d), "original_%s.bin" % ("f64" if f64 else "f32"))
    r, _, mismatches, _ = _run(lifecycle, "copy_then_rebuild_copy", "f64" if f64 else "f32", out)
    assert mismatches == 0 and r.returncode == 0, r.stdout[-4000:]
    if f64:
        v, rays = v.astype(np.float64), widen_rays(rays)
    hd, nd = (HIT_F64, NODE_F64) if f64 else (HIT_F32, NODE_F32)
    raw = open(out, "rb").read()
    n = rays.shape[0]
    hits = np.frombuffer(raw, dtype=hd, count=n)
    o = n * hd.itemsize
    mask = np.frombuffer(raw, dtype=np.uint8, count=n, offset=o)
    o += n
    nn = int(np.frombuffer(raw, dtype=np.uint64, count=1, offset=o)[0])
    nodes = np.frombuffer(raw, dtype=nd, count=nn, offset=o + 8)
    o += 8 + nn * nd.itemsize
    ni = int(np.frombuffer(raw, dtype=np.uint64, count=1, offset=o)[0])
    idx = np.frombuffer(raw, dtype=np.uint32, count=ni, offset=o + 8)
    assert ni == f.shape[0] and o + 8 + 4 * ni == len(raw)
    oh, om = oracle.traverse(nodes, idx, v, f, rays)
    assert np.array_equal(mask, om)
    assert 0 < int(mask.sum()) < n
    hit = mask.astype(bool)
    for k in ("u", "v", "t", "prim_id"):  # (fields: the fp64 record ends in padding)
        assert hits[k][hit].tobytes() == oh[k][hit].tobytes(), k
