"""urf_set_front_outputs is declared in include/urf.h (tests/test_abi.py: then exported), exported by the library, wrapped by the Python API
and passed through by both C++ adapters (urf::Detector, urf::BatchDetector)."""
import os
import re
import subprocess

import urban_road_filter_amd as u
from urban_road_filter_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_switch_is_declared_and_wrapped():
    header = open(os.path.join(ROOT, "include", "urf.h")).read()
    assert re.search(r"\bint\s+urf_set_front_outputs\s*\(\s*urf_ctx\s*\*\s*ctx\s*,\s*int\s+on\s*\)\s*;", header)
    assert callable(getattr(u.Context, "set_front_outputs", None))
    import ctypes
    f = u.lib().urf_set_front_outputs
    assert list(f.argtypes) == [ctypes.c_void_p, ctypes.c_int] and f.restype is ctypes.c_int


def test_the_library_exports_it():
    import ctypes
    lib = ctypes.CDLL(os.path.join(os.path.dirname(api.__file__), "liburf_hip.so"))
    assert hasattr(lib, "urf_set_front_outputs")
    for on in (0, 1, 2):
        assert lib.urf_set_front_outputs(None, on) == -1   # (no context: URF_ERR_INVALID_ARG, before anything touches a device)


def test_the_adapters_compile_with_their_setters(tmp_path):
    tu = tmp_path / "setters.cpp"
    tu.write_text('#include "detector.hpp"\n'
                  "void both(urf::Detector& d, urf::BatchDetector& b) { d.setFrontOutputs(true); b.setFrontOutputs(false); }\n"
                  "void (urf::Detector::*one)(bool) = &urf::Detector::setFrontOutputs;\n")
    pkg = os.path.join(ROOT, "urban_road_filter_amd")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(pkg, "csrc"), str(tu)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
