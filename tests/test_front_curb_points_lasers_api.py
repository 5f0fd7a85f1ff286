"""urf_set_front_curb_points is declared in include/urf.h (tests/test_abi.py: then exported), wrapped by the Python API and by both
C++ adapters."""
import os
import re

import urban_road_filter_amd as u
from urban_road_filter_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_switch_is_declared_and_wrapped():
    header = open(os.path.join(ROOT, "include", "urf.h")).read()
    assert re.search(r"\bint\s+urf_set_front_curb_points\s*\(\s*urf_ctx\s*\*\s*ctx\s*,\s*int\s+on\s*\)\s*;", header)
    assert callable(getattr(u.Context, "set_front_curb_points", None))
    src = open(api.__file__).read()
    assert '"urf_set_front_curb_points": [vp, C.c_int]' in src and "self._lib.urf_set_front_curb_points(self._h, int(on))" in src


def test_both_adapters_wrap_it():
    src = open(os.path.join(os.path.dirname(api.__file__), "csrc", "detector.hpp")).read()
    assert len(re.findall(r"void\s+setFrontCurbPoints\s*\(\s*bool\s+on\s*\)", src)) == 2   # Detector and BatchDetector
    assert src.count("urf_set_front_curb_points(ctx_, on ? 1 : 0)") == 2


def test_the_library_exports_it():
    import ctypes
    lib = ctypes.CDLL(os.path.join(os.path.dirname(api.__file__), "liburf_hip.so"))
    assert hasattr(lib, "urf_set_front_curb_points")
    assert lib.urf_set_front_curb_points(None, 1) == -1   # (no context: URF_ERR_INVALID_ARG, before anything touches a device)
