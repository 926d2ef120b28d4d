"""The sphere / curve refit entry points of include/nanort_hip.h (nrtRefitPrims_f32 / nrtRefitPrimsDevice_f32) without a GPU:
the export list, the refusal of a NULL context before any device is touched, the declared signatures as C99 and C++11, and the
header-only layer's RefitGeometry overloads compiling without the backend's library."""
import os
import subprocess

from nanort_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nrtRefitPrims_f32", "nrtRefitPrimsDevice_f32")


def test_binding_table_header_and_library_carry_the_two_symbols():
    header = open(os.path.join(ROOT, "include", "nanort_hip.h")).read()
    for name in NAMES:
        assert name in capi.SYMBOLS and hasattr(capi.lib(), name) and ("NRT_API nrt_status %s(" % name) in header


def test_null_context_and_null_positions_are_refused_without_a_device():
    L = capi.lib()
    assert L.nrtRefitPrims_f32(None, 16, 16, 1) == capi.NRT_ERR_INVALID
    assert L.nrtRefitPrims_f32(None, None, None, 0) == capi.NRT_ERR_INVALID
    assert L.nrtRefitPrimsDevice_f32(None, 16, 16, 1, None) == capi.NRT_ERR_INVALID
    assert L.nrtRefitPrimsDevice_f32(None, 16, None, 1, None) == capi.NRT_ERR_INVALID


def test_declared_signatures_compile_as_c_and_cxx(tmp_path):
    src = tmp_path / "t.c"
    src.write_text(
        '#include "nanort_hip.h"\n'
        "typedef nrt_status (*host_form)(nrt_ctx *, const float *, const float *, uint32_t);\n"
        "typedef nrt_status (*device_form)(nrt_ctx *, const float *, const float *, uint32_t, void *);\n"
        "int main(void){ host_form a = nrtRefitPrims_f32; device_form b = nrtRefitPrimsDevice_f32;\n"
        "  return a(0, 0, 0, 0) == NRT_ERR_INVALID && b(0, 0, 0, 0, 0) == NRT_ERR_INVALID ? 0 : 1; }\n")
    for cc, std in (("gcc", "-std=c99"), ("g++", "-std=c++11")):  # (compiled, not linked: the declarations against the typedefs)
        obj = tmp_path / ("t_" + cc + ".o")
        subprocess.check_call([cc, std, "-x", "c" if cc == "gcc" else "c++", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                               "-c", str(src), "-o", str(obj)])
        assert obj.exists()


def compile_driver(exe):
    """tests/cpp/refit_prims_check.cc against the header with the backend macro and the built library (no GPU needed to compile)."""
    inc, libdir = os.path.join(ROOT, "include"), os.path.join(ROOT, "nanort_amd", "lib")
    args = ["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-invalid-offsetof", "-DNANORT_USE_HIP_BACKEND", "-pthread",
            "-D__HIP_PLATFORM_AMD__", "-I", inc, "-isystem", "/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "refit_prims_check.cc"),
            "-o", str(exe), "-L", libdir, "-lnanort_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"]
    r = subprocess.run(args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, "g++ failed:\n" + r.stdout[-3000:]
    return str(exe)


def test_refit_prims_driver_compiles(tmp_path):
    compile_driver(tmp_path / "refit_prims_check")
