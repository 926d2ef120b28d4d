"""BVHAccel::Refit of include/nanort.h with the HIP backend (tests/cpp/refit_check.cc): after a refit every batch method
equals the object's own per-ray host walk on the new positions; a copy made before the refit still answers on the old
tree and old positions; a moved-into object refits; NANORT_HIP_DEVICES=0,0 replicas all see the refit; sphere and cylinder
accels refuse.  The driver compiles without a GPU (a CPU test)."""
import os
import subprocess

import numpy as np
import pytest

from nanort_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
LIBDIR = os.path.join(ROOT, "nanort_amd", "lib")
SRC = os.path.join(ROOT, "tests", "cpp", "refit_check.cc")


def compile_driver(exe):
    args = ["g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-DNANORT_USE_HIP_BACKEND", "-pthread", "-D__HIP_PLATFORM_AMD__", "-I", INC,
            "-isystem", "/opt/rocm/include", SRC, "-o", str(exe), "-L", LIBDIR, "-lnanort_hip", "-Wl,-rpath," + LIBDIR,
            "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"]
    r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, "g++ failed:\n" + r.stdout[-3000:]
    return str(exe)


def test_refit_driver_compiles(tmp_path):
    compile_driver(tmp_path / "refit_check")


def _mesh_file(path, v, f):
    with open(path, "wb") as fp:
        fp.write(np.array([v.shape[0], f.shape[0]], dtype=np.uint32).tobytes())
        fp.write(np.ascontiguousarray(v, dtype=np.float32).tobytes())
        fp.write(np.ascontiguousarray(f, dtype=np.uint32).tobytes())


@pytest.fixture(scope="module")
def inputs(tmp_path_factory, c1_mesh):
    d = tmp_path_factory.mktemp("refit_check")
    v, f = c1_mesh
    v = v.astype(np.float64)
    w1 = v.copy()
    w1[:, 1] += 0.1 * np.sin(5.0 * w1[:, 0])
    w2 = (v - v.mean(axis=0)) * (1.3, 0.8, 1.0) + v.mean(axis=0) + (0.1, 0.0, -0.05)
    for name, x in (("mesh0.bin", v), ("mesh1.bin", w1), ("mesh2.bin", w2)):
        _mesh_file(str(d / name), x.astype(np.float32), f)
    rays = scenes.camera_rays(96, 64)
    with open(str(d / "rays.bin"), "wb") as fp:
        fp.write(np.array([rays.shape[0]], dtype=np.uint64).tobytes())
        fp.write(rays.tobytes())
    return str(d), compile_driver(d / "refit_check")


@pytest.mark.gpu
@pytest.mark.parametrize("real", ["f32", "f64"])
@pytest.mark.parametrize("devices", [None, "0,0"], ids=["one", "replicas"])
def test_header_refit(inputs, real, devices):
    d, exe = inputs
    env = dict(os.environ)
    env.pop("NANORT_HIP_DEVICES", None)
    if devices:
        env["NANORT_HIP_DEVICES"] = devices
    r = subprocess.run([exe, real, d], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=240)
    assert r.returncode == 0, r.stdout[-4000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("devices ")][-1].split()
    assert int(line[1]) == (2 if devices else 1), r.stdout
    assert int(line[3]) > 40 and int(line[5]) == 0, r.stdout
