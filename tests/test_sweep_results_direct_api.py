"""urf_set_sweep_results_direct is declared in include/urf.h as an entry point of its own (urf_set_sweep_outputs keeps refusing every bit
above 3), exported by both libraries, refuses a NULL context and every value but 0 / 1 before anything touches a device, is wrapped by the
Python API, and the C++ adapter has the member, off by default.  The ABI is still 5."""
import ctypes
import os
import re

import pytest

import urban_road_filter_amd as u
from urban_road_filter_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "urf_set_sweep_results_direct"


def _header():
    src = open(os.path.join(ROOT, "include", "urf.h")).read()
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


def _body(src, start):
    body = src[src.index(start):]
    return body[:body.index("\n}\n")]


def test_the_entry_point_is_declared_and_the_abi_is_still_5():
    h = _header()
    assert "int urf_set_sweep_results_direct(urf_ctx* ctx, int on);" in h
    assert "int urf_set_sweep_outputs(urf_ctx* ctx, uint32_t bits);" in h   # (its own function: the bits' entry point is as it was)
    assert "#define URF_ABI_VERSION 5" in h and "#define URF_SWEEP_OUT_MARKER_POINTS 1u" in h and "#define URF_SWEEP_OUT_ORDER 2u" in h
    assert u.lib().urf_abi_version() == 5


@pytest.mark.parametrize("hooks", [False, True], ids=["product", "hooks_build"])
def test_the_libraries_export_it_and_refuse_bad_arguments_first(hooks):
    lib = ctypes.CDLL(u.lib_path(hooks=hooks))
    assert hasattr(lib, NAME)
    f = getattr(lib, NAME)
    f.argtypes = [ctypes.c_void_p, ctypes.c_int]
    f.restype = ctypes.c_int
    for on in (0, 1, 2, -1, 3, 0x7fffffff):
        assert f(None, on) == -1


def test_other_values_are_refused_in_front_of_everything_that_needs_the_device():
    src = open(os.path.join(os.path.dirname(api.__file__), "csrc", "urf_api_sweep.hpp")).read()   # (the callback path's part of urf_api.hip)
    body = _body(src, 'extern "C" int urf_set_sweep_results_direct(')
    assert body.index("on != 0 && on != 1") < body.index("URF_ERR_INVALID_ARG") < body.index("sl.pending") < body.index("URF_ERR_BUSY")
    assert body.index("URF_ERR_BUSY") < body.index("hipSetDevice") < body.index("sweep_outputs_alloc(") < body.index("pol.set(")
    assert "c->pol.sweep_outputs &&" in body       # with no bit set it allocates nothing
    outputs = _body(src, 'extern "C" int urf_set_sweep_outputs(')
    assert "bits & ~(URF_SWEEP_OUT_MARKER_POINTS | URF_SWEEP_OUT_ORDER)" in outputs and "sweep_direct" in outputs
    from conftest import gpu_available
    if gpu_available():
        with u.Context(4096, 1) as ctx:
            for on in (2, -1, 7):
                assert ctx._lib.urf_set_sweep_results_direct(ctx._h, on) == -1
            for on in (1, 0, 1):
                ctx.set_sweep_results_direct(on)
            assert ctx._lib.urf_set_sweep_outputs(ctx._h, 4) == -1


def test_the_switch_is_a_policy_field_that_plan_does_not_read():
    pol = open(os.path.join(os.path.dirname(api.__file__), "csrc", "urf_policy.hpp")).read()
    assert re.search(r"bool\s+sweep_direct\s*=\s*false;", pol)
    uses = [m.start() for m in re.finditer(r"\bsweep_direct\b", pol)]
    assert len(uses) == 1, "only its declaration: plan() and the questions it asks do not read it"


def test_the_python_api_wraps_it():
    assert callable(getattr(u.Context, "set_sweep_results_direct", None))
    src = open(api.__file__).read()
    assert '"%s": [' % NAME in src and "self._lib.%s(self._h" % NAME in src


def test_the_cpp_adapter_has_the_member():
    pkg = os.path.dirname(api.__file__)
    hpp = open(os.path.join(pkg, "csrc", "detector.hpp")).read()
    det = hpp[hpp.index("class Detector"):hpp.index("class BatchDetector : ")]
    assert re.search(r"void\s+setSweepResultsDirect\s*\(\s*bool\s+on\s*\)", det)
    assert "bool sweep_outputs_ = false;" in det   # (the existing members as they are)
    assert "setSweepResultsDirect" in hpp[hpp.index("static std::string describe("):hpp.index("protected:")]
    cpp = open(os.path.join(pkg, "csrc", "detector.cpp")).read()
    assert NAME + "(ctx_" in cpp


def test_the_cpp_client_builds_against_the_product_library(tmp_path):
    """tests/cpp/detector_sweep_direct_demo.cpp (tests/test_gpu_sweep_results_direct.py runs it) with g++, include/urf.h and
    csrc/detector.hpp only."""
    import shutil
    import subprocess
    if not shutil.which("g++"):
        pytest.skip("no g++")
    u.lib()   # (built)
    pkg = os.path.dirname(api.__file__)
    exe = str(tmp_path / "detector_sweep_direct_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(pkg, "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "detector_sweep_direct_demo.cpp"), "-o", exe,
                           "-L" + pkg, "-l:liburf_hip.so", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"])
    undefined = subprocess.run(["nm", "-u", exe], capture_output=True, text=True).stdout
    assert "setSweepResultsDirect" in undefined
