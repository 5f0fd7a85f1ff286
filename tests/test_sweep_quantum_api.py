"""urf_set_sweep_quantum and urf_callback_path_captures are declared in include/urf.h (tests/test_abi.py: then exported), refuse a NULL
context before anything touches a device, are wrapped by the Python API, and the C++ adapter has the switch."""
import ctypes
import os
import re

import pytest

import urban_road_filter_amd as u
from urban_road_filter_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("urf_set_sweep_quantum", "urf_callback_path_captures")


def _header():
    src = open(os.path.join(ROOT, "include", "urf.h")).read()
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


def test_the_two_entry_points_are_declared():
    h = _header()
    assert "#define URF_SWEEP_SEQS 8" in h
    assert "int urf_set_sweep_quantum(urf_ctx* ctx, uint32_t points);" in h
    assert "int urf_callback_path_captures(const urf_ctx* ctx, uint32_t* n_captured, uint32_t* n_resident);" in h
    assert "int urf_callback_path_state(const urf_ctx* ctx, uint32_t* n_rerun, uint32_t* sequence);" in h   # keeps its signature
    assert "#define URF_ABI_VERSION 5" in h and "#define URF_MAX_IN_FLIGHT 4" in h   # additive


@pytest.mark.parametrize("hooks", [False, True], ids=["product", "hooks_build"])
def test_the_libraries_export_them_and_refuse_a_null_context_first(hooks):
    lib = ctypes.CDLL(u.lib_path(hooks=hooks))
    for n in NAMES:
        assert hasattr(lib, n), n
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    lib.urf_set_sweep_quantum.argtypes = [vp, u32]
    lib.urf_callback_path_captures.argtypes = [vp, vp, vp]
    for q in (0, 1000, 2048, 0xffffffff):
        assert lib.urf_set_sweep_quantum(None, q) == -1
    a, b = u32(7), u32(7)
    assert lib.urf_callback_path_captures(None, ctypes.byref(a), ctypes.byref(b)) == -1
    assert (a.value, b.value) == (7, 7)


def test_the_checks_stand_in_front_of_the_switch():
    """The value, then the sweeps in flight, then the allocation, then the policy field -- in the source, and on a device where there is one."""
    from conftest import gpu_available
    src = open(os.path.join(os.path.dirname(api.__file__), "csrc", "urf_api_sweep.hpp")).read()   # (the callback path's part of urf_api.hip)
    body = src[src.index('extern "C" int urf_set_sweep_quantum('):]
    body = body[:body.index("\n}\n")]
    assert body.index("points % URF_TILE") < body.index("sl.pending") < body.index("grow(") < body.index("pol.set(")
    assert "URF_ERR_BUSY" in body and "points > c->max_points" in body
    pol = open(os.path.join(os.path.dirname(api.__file__), "csrc", "urf_policy.hpp")).read()
    plan = pol[pol.index("void plan("):pol.index("struct reasons")]
    assert "uint32_t sweep_quantum = 0;" in pol and "sweep_quantum" not in plan   # a field plan() does not read
    if gpu_available():
        with u.Context(4096, 1) as ctx:
            for q in (1000, 2049, 6144):
                assert ctx._lib.urf_set_sweep_quantum(ctx._h, q) == -1
                assert b"urf_set_sweep_quantum" in ctx._lib.urf_last_error(ctx._h)
            for q in (2048, 4096, 0):
                ctx.set_sweep_quantum(q)
            assert ctx.callback_path_captures() == (0, 0)


def test_the_python_api_wraps_them():
    for m in ("set_sweep_quantum", "callback_path_captures"):
        assert callable(getattr(u.Context, m, None)), m
    src = open(api.__file__).read()
    for n in NAMES:
        assert '"%s": [' % n in src and "self._lib.%s(self._h" % n in src, n


def test_the_cpp_adapter_has_the_switch():
    pkg = os.path.dirname(api.__file__)
    hpp = open(os.path.join(pkg, "csrc", "detector.hpp")).read()
    det = hpp[hpp.index("class Detector"):hpp.index("class BatchDetector : ")]
    assert re.search(r"void\s+setSweepQuantum\s*\(\s*uint32_t\s+points\s*\)", det)
    assert "setSweepQuantum" not in hpp[hpp.index("class BatchDetector : "):]   # no callback path there
    cpp = open(os.path.join(pkg, "csrc", "detector.cpp")).read()
    assert "urf_set_sweep_quantum(ctx_" in cpp


def test_the_cpp_client_builds_against_the_product_library(tmp_path):
    """tests/cpp/detector_sweep_quantum_demo.cpp (tests/test_gpu_detector_sweep_quantum.py runs it) with g++, include/urf.h and
    csrc/detector.hpp only."""
    import shutil
    import subprocess
    if not shutil.which("g++"):
        pytest.skip("no g++")
    u.lib()   # (built)
    pkg = os.path.dirname(api.__file__)
    exe = str(tmp_path / "detector_sweep_quantum_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(pkg, "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "detector_sweep_quantum_demo.cpp"), "-o", exe,
                           "-L" + pkg, "-l:liburf_hip.so", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"])
    undefined = subprocess.run(["nm", "-u", exe], capture_output=True, text=True).stdout
    assert "setSweepQuantum" in undefined
