"""urf_set_dense_outputs -- the switch under which the reference-order read-outs answer after a dense call, in the caller's indices -- is
declared in include/urf.h (tests/test_abi.py: then exported) under the same ABI version, exported by the product library, wrapped by the
Python API, and urf::BatchDetector has setDenseOutputs; tests/cpp/batch_dense_ref_demo.cpp (tests/test_gpu_dense_outputs.py runs it)
builds against include/urf.h and csrc/detector.hpp only."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

import urban_road_filter_amd as u
from urban_road_filter_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "urf_set_dense_outputs"


def test_the_switch_is_declared_under_the_same_abi_version():
    src = open(os.path.join(ROOT, "include", "urf.h")).read()
    h = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    assert "int urf_set_dense_outputs(urf_ctx* ctx, int on);" in h
    assert "#define URF_ABI_VERSION 5" in h and "#define URF_NUM_KERNELS 8" in h   # additive
    # the header says what the switch does and what stays refused, and no longer defers it
    assert "left to a later version" not in src
    assert re.search(r"urf_read_stage stays refused after a dense call", src)


def test_the_product_library_exports_it_and_refuses_a_null_context():
    for lib in (ctypes.CDLL(os.path.join(os.path.dirname(api.__file__), "liburf_hip.so")), u.lib()):
        assert hasattr(lib, ENTRY)
        f = getattr(lib, ENTRY)
        f.argtypes, f.restype = [ctypes.c_void_p, ctypes.c_int], ctypes.c_int
        for on in (0, 1, 2, -1):
            assert f(None, on) == -1   # (no context: URF_ERR_INVALID_ARG, before anything touches a device)


def test_the_python_api_wraps_it():
    assert callable(getattr(u.Context, "set_dense_outputs", None))
    f = getattr(u.lib(), ENTRY)
    assert list(f.argtypes) == [ctypes.c_void_p, ctypes.c_int] and f.restype is ctypes.c_int
    src = open(api.__file__).read()
    assert '"%s": [vp, C.c_int]' % ENTRY in src and "self._lib.%s(self._h, int(on))" % ENTRY in src


def test_the_batch_detector_has_the_setter():
    pkg = os.path.dirname(api.__file__)
    hpp = open(os.path.join(pkg, "csrc", "detector.hpp")).read()
    batch = hpp[hpp.index("class BatchDetector"):]
    body = re.search(r"void\s+setDenseOutputs\s*\(\s*bool\s+on\s*\)\s*\{([^}]*)\}", batch)
    assert body and re.search(r'set\s*\(\s*%s\s*,\s*"%s"\s*,\s*on\s*\)\s*;' % (ENTRY, ENTRY), body.group(1)), body
    assert "setDenseOutputs" not in hpp[:hpp.index("class BatchDetector")]   # (a dense call is a batch call: Detector has none)
    cpp = open(os.path.join(pkg, "csrc", "detector.cpp")).read()
    assert re.search(r"dense_firings_\s*!=\s*0\s*&&\s*\(\s*!reference_order_\s*\|\|\s*dense_outputs_\s*\)", cpp)


def test_the_cpp_client_builds_against_the_product_library(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    u.lib()   # (built)
    pkg = os.path.dirname(api.__file__)
    exe = str(tmp_path / "batch_dense_ref_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(pkg, "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "batch_dense_ref_demo.cpp"), "-o", exe,
                           "-L" + pkg, "-l:liburf_hip.so", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"])
    undefined = subprocess.run(["nm", "-u", exe], capture_output=True, text=True).stdout
    assert ENTRY in undefined and "setDenseRealign" in undefined   # (setDenseOutputs is inline: the entry point itself is linked)
    # ... and nothing but the two public headers of the project
    src = open(os.path.join(ROOT, "tests", "cpp", "batch_dense_ref_demo.cpp")).read()
    assert re.findall(r'#include\s+"([^"]+)"', src) == ["detector.hpp"]
