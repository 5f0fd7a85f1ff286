"""urf_set_sweep_outputs, urf_result_marker_points and urf_result_ordered_indices are declared in include/urf.h (tests/test_abi.py: then
exported), refuse a NULL context and unknown bits before anything touches a device, are wrapped by the Python API, and the C++ adapter
has the switch."""
import ctypes
import os
import re

import pytest

import urban_road_filter_amd as u
from urban_road_filter_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("urf_set_sweep_outputs", "urf_result_marker_points", "urf_result_ordered_indices")


def _header():
    src = open(os.path.join(ROOT, "include", "urf.h")).read()
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


def test_the_three_entry_points_are_declared():
    h = _header()
    assert "#define URF_SWEEP_OUT_MARKER_POINTS 1u" in h and "#define URF_SWEEP_OUT_ORDER 2u" in h
    assert "int urf_set_sweep_outputs(urf_ctx* ctx, uint32_t bits);" in h
    assert "int urf_result_marker_points(urf_ctx* ctx, uint32_t ticket, const float** pts, uint32_t* count);" in h
    assert ("int urf_result_ordered_indices(urf_ctx* ctx, uint32_t ticket, const uint32_t** road, const uint32_t** curb, "
            "const uint32_t** ring10, uint32_t counts[3]);") in h
    assert "#define URF_ABI_VERSION 5" in h and "#define URF_NUM_KERNELS 8" in h and "#define URF_MAX_IN_FLIGHT 4" in h   # additive


@pytest.mark.parametrize("hooks", [False, True], ids=["product", "hooks_build"])
def test_the_libraries_export_them_and_refuse_a_null_context_first(hooks):
    lib = ctypes.CDLL(u.lib_path(hooks=hooks))
    for n in NAMES:
        assert hasattr(lib, n), n
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    lib.urf_set_sweep_outputs.argtypes = [vp, u32]
    lib.urf_result_marker_points.argtypes = [vp, u32, vp, vp]
    lib.urf_result_ordered_indices.argtypes = [vp, u32, vp, vp, vp, vp]
    for bits in (0, 1, 2, 3, 4, 0xffffffff):
        assert lib.urf_set_sweep_outputs(None, bits) == -1
    p, n, cnt = vp(), u32(7), (u32 * 3)(7, 7, 7)
    assert lib.urf_result_marker_points(None, 0, ctypes.byref(p), ctypes.byref(n)) == -1
    assert lib.urf_result_ordered_indices(None, 0, ctypes.byref(p), None, None, cnt) == -1


def test_bits_above_three_are_refused():
    """With a context where there is a device; the refusal comes before any allocation.  Without one the rule is still in the
    source: the check on the bits stands in front of everything that needs the device."""
    from conftest import gpu_available
    src = open(os.path.join(os.path.dirname(api.__file__), "csrc", "urf_api_sweep.hpp")).read()   # (the callback path's part of urf_api.hip)
    body = src[src.index('extern "C" int urf_set_sweep_outputs('):]
    body = body[:body.index("\n}\n")]
    assert body.index("bits & ~(URF_SWEEP_OUT_MARKER_POINTS | URF_SWEEP_OUT_ORDER)") < body.index("sweep_outputs_alloc(") < body.index("pol.set(")
    assert "URF_ERR_BUSY" in body and "sl.pending" in body
    if gpu_available():
        with u.Context(4096, 1) as ctx:
            for bits in (4, 5, 8, 0x80000000):
                assert ctx._lib.urf_set_sweep_outputs(ctx._h, bits) == -1
                assert b"URF_SWEEP_OUT" in ctx._lib.urf_last_error(ctx._h)
            for bits in (1, 2, 3, 0):
                ctx.set_sweep_outputs(bits)


def test_the_python_api_wraps_them():
    for m in ("set_sweep_outputs", "result_marker_points", "result_ordered_indices"):
        assert callable(getattr(u.Context, m, None)), m
    assert (u.SWEEP_OUT_MARKER_POINTS, u.SWEEP_OUT_ORDER) == (1, 2)
    src = open(api.__file__).read()
    for n in NAMES:
        assert '"%s": [' % n in src and "self._lib.%s(self._h" % n in src, n


def test_the_cpp_adapter_has_the_switch():
    pkg = os.path.dirname(api.__file__)
    hpp = open(os.path.join(pkg, "csrc", "detector.hpp")).read()
    det = hpp[hpp.index("class Detector"):hpp.index("class BatchDetector : ")]
    assert re.search(r"void\s+setSweepOutputs\s*\(\s*bool\s+on\s*\)", det)
    assert "bool sweep_outputs_ = false;" in det   # off by default
    cpp = open(os.path.join(pkg, "csrc", "detector.cpp")).read()
    for n in NAMES:
        assert n + "(ctx_" in cpp, n
    assert "urf_marker_points(ctx_" in cpp and "urf_ordered_indices(ctx_" in cpp   # the switch off: the two synchronous calls
    assert "setSweepOutputs" in hpp[hpp.index("static std::string describe("):hpp.index("protected:")]


def test_the_cpp_client_builds_against_the_product_library(tmp_path):
    """tests/cpp/detector_sweep_outputs_demo.cpp (tests/test_gpu_detector_sweep_outputs.py runs it) with g++, include/urf.h and
    csrc/detector.hpp only."""
    import shutil
    import subprocess
    if not shutil.which("g++"):
        pytest.skip("no g++")
    u.lib()   # (built)
    pkg = os.path.dirname(api.__file__)
    exe = str(tmp_path / "detector_sweep_outputs_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(pkg, "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "detector_sweep_outputs_demo.cpp"), "-o", exe,
                           "-L" + pkg, "-l:liburf_hip.so", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"])
    undefined = subprocess.run(["nm", "-u", exe], capture_output=True, text=True).stdout
    assert "urf_set_sweep_outputs" in undefined or "applySweepOutputs" in undefined
