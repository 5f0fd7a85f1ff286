"""urf_set_front_lasers128 is declared in include/urf.h (tests/test_abi.py: then exported) and wrapped by the Python API."""
import os
import re

import urban_road_filter_amd as u
from urban_road_filter_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_switch_is_declared_and_wrapped():
    header = open(os.path.join(ROOT, "include", "urf.h")).read()
    assert re.search(r"\bint\s+urf_set_front_lasers128\s*\(\s*urf_ctx\s*\*\s*ctx\s*,\s*int\s+on\s*\)\s*;", header)
    assert callable(getattr(u.Context, "set_front_lasers128", None))
    src = open(api.__file__).read()
    assert '"urf_set_front_lasers128": [vp, C.c_int]' in src and "self._lib.urf_set_front_lasers128(self._h, int(on))" in src


def test_the_library_exports_it():
    import ctypes
    lib = ctypes.CDLL(os.path.join(os.path.dirname(api.__file__), "liburf_hip.so"))
    assert hasattr(lib, "urf_set_front_lasers128")
    assert lib.urf_set_front_lasers128(None, 1) == -1   # (no context: URF_ERR_INVALID_ARG, before anything touches a device)
