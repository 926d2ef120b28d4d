"""The device-geometry entry points of include/nanort_hip.h (nrtSetMeshDevice_* / nrtSetSpheresDevice_f32) without a GPU: a
NULL context is refused before any device is touched, and the header with their declarations is still C99 and C++11."""
import os
import subprocess

from nanort_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_null_context_is_refused_without_a_device():
    L = capi.lib()
    assert L.nrtSetMeshDevice_f32(None, 16, 3, 12, 16, 1, None) == capi.NRT_ERR_INVALID
    assert L.nrtSetMeshDevice_f64(None, 16, 3, 24, 16, 1, None) == capi.NRT_ERR_INVALID
    assert L.nrtSetSpheresDevice_f32(None, 16, 16, 1, None) == capi.NRT_ERR_INVALID
    assert L.nrtSetMeshDevice_f32(None, None, 0, 0, None, 0, None) == capi.NRT_ERR_INVALID
    assert L.nrtSetSpheresDevice_f32(None, None, None, 0, None) == capi.NRT_ERR_INVALID


def test_binding_table_carries_the_three_symbols():
    for name in ("nrtSetMeshDevice_f32", "nrtSetMeshDevice_f64", "nrtSetSpheresDevice_f32"):
        assert name in capi.SYMBOLS and hasattr(capi.lib(), name)


def test_header_with_the_device_geometry_calls_compiles_as_c_and_cxx(tmp_path):
    src = tmp_path / "t.c"
    src.write_text(
        '#include "nanort_hip.h"\n'
        "typedef nrt_status (*mesh32)(nrt_ctx *, const float *, uint32_t, size_t, const uint32_t *, uint32_t, void *);\n"
        "typedef nrt_status (*mesh64)(nrt_ctx *, const double *, uint32_t, size_t, const uint32_t *, uint32_t, void *);\n"
        "typedef nrt_status (*sph32)(nrt_ctx *, const float *, const float *, uint32_t, void *);\n"
        "int main(void){ mesh32 a = nrtSetMeshDevice_f32; mesh64 b = nrtSetMeshDevice_f64; sph32 c = nrtSetSpheresDevice_f32;\n"
        "  return a(0, 0, 0, 0, 0, 0, 0) == NRT_ERR_INVALID && b(0, 0, 0, 0, 0, 0, 0) == NRT_ERR_INVALID && c(0, 0, 0, 0, 0) == NRT_ERR_INVALID ? 0 : 1; }\n")
    for cc, std in (("gcc", "-std=c99"), ("g++", "-std=c++11")):  # (compiled, not linked: the declarations against the typedefs)
        obj = tmp_path / ("t_" + cc + ".o")
        subprocess.check_call([cc, std, "-x", "c" if cc == "gcc" else "c++", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                               "-c", str(src), "-o", str(obj)])
        assert obj.exists()
