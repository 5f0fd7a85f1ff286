"""urf_set_front_auto / urf_front_auto_query: declared in include/urf.h, exported by both libraries, refused without a context before
anything touches a device, wrapped by the Python API, and passed through by both C++ adapters from their common base
(urf::FrontSwitches, detector.hpp) -- the pattern of tests/test_front_switches_api.py."""
import ctypes
import os
import re
import subprocess

import numpy as np

import urban_road_filter_amd as u
from urban_road_filter_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "urf.h")).read()
HPP = open(os.path.join(os.path.dirname(api.__file__), "csrc", "detector.hpp")).read()


def test_the_entry_points_are_declared():
    assert re.search(r"\bint\s+urf_set_front_auto\s*\(\s*urf_ctx\s*\*\s*ctx\s*,\s*int\s+on\s*\)\s*;", HEADER)
    assert re.search(r"\bint\s+urf_front_auto_query\s*\(\s*urf_ctx\s*\*\s*ctx\s*,\s*urf_front_auto_info\s*\*\s*out\s*\)\s*;", HEADER)
    assert re.search(r"#define\s+URF_ABI_VERSION\s+5\b", HEADER)   # (no bump, as with the earlier switches)


def test_both_libraries_export_them_and_refuse_a_null_context():
    for lib in (ctypes.CDLL(os.path.join(os.path.dirname(api.__file__), "liburf_hip.so")), u.lib()):
        for on in (0, 1, 2):
            assert lib.urf_set_front_auto(None, on) == -1   # URF_ERR_INVALID_ARG
        out = np.zeros(1, u.FRONT_AUTO_DTYPE)
        assert lib.urf_front_auto_query(None, ctypes.c_void_p(out.ctypes.data)) == -1
        assert lib.urf_front_auto_query(None, None) == -1


def test_the_record_is_64_bytes_in_the_headers_order(tmp_path):
    body = re.search(r"typedef\s+struct\s+urf_front_auto_info\s*\{(.*?)\}\s*urf_front_auto_info\s*;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in re.findall(r"uint32_t\s+([^;]+);", body):
        for name in decl.split(","):
            m = re.fullmatch(r"\s*(\w+)\s*(?:\[(\d+)\])?\s*", name)
            names.append((m.group(1), int(m.group(2) or 1)))
    assert sum(n for _, n in names) * 4 == 64 == u.FRONT_AUTO_DTYPE.itemsize
    assert [n for n, _ in names] == list(u.FRONT_AUTO_DTYPE.names)
    tu = tmp_path / "size.c"
    tu.write_text('#include "urf.h"\n_Static_assert(sizeof(urf_front_auto_info) == 64, "64 bytes");\n')
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_python_wrapper():
    assert callable(getattr(u.Context, "set_front_auto", None)) and callable(getattr(u.Context, "front_auto", None))
    f = u.lib().urf_set_front_auto
    assert list(f.argtypes) == [ctypes.c_void_p, ctypes.c_int] and f.restype is ctypes.c_int
    src = open(api.__file__).read()
    assert '"urf_set_front_auto": [vp, C.c_int]' in src and "self._lib.urf_set_front_auto(self._h, int(on))" in src
    assert u.AUTO_PHASE == {"IDLE": 0, "LEARNING": 1, "SETTLED": 2}
    mask = re.search(r"#define\s+URF_ADVICE_AUTO_MASK\s+\(([^)]*)\)", HEADER.replace("\\\n", " ")).group(1)
    assert u.ADVICE_AUTO_MASK == sum(u.ADVICE[n] for n in re.findall(r"URF_ADVICE_(\w+)", mask))


def test_the_setter_sits_once_in_the_base_and_forwards_by_name():
    base = re.search(r"class\s+FrontSwitches\s*\{(.*?)\n\};", HPP, re.S).group(1)
    bodies = re.findall(r"void\s+setFrontAuto\s*\(\s*bool\s+on\s*\)\s*\{([^}]*)\}", HPP)
    assert len(bodies) == 1 and bodies[0] in base, bodies
    assert re.fullmatch(r'\s*set\s*\(\s*urf_set_front_auto\s*,\s*"urf_set_front_auto"\s*,\s*on\s*\)\s*;\s*', bodies[0]), bodies[0]
    assert len(re.findall(r"urf_front_auto_info\s+frontAuto\s*\(\s*\)\s*const", HPP)) == 1 and re.search(r"urf_front_auto_info\s+frontAuto\s*\(\s*\)\s*const", base)


def test_both_adapters_compile_with_them(tmp_path):
    tu = tmp_path / "auto.cpp"
    tu.write_text('#include "detector.hpp"\n'
                  "unsigned both(urf::Detector& d, urf::BatchDetector& b) { d.setFrontMode(2); d.setFrontAuto(true); b.setFrontMode(2); b.setFrontAuto(false);\n"
                  "    return d.frontAuto().phase + b.frontAuto().applied; }\n"
                  "void (urf::Detector::*ds)(bool) = &urf::Detector::setFrontAuto;\nvoid (urf::BatchDetector::*bs)(bool) = &urf::BatchDetector::setFrontAuto;\n"
                  "urf_front_auto_info (urf::Detector::*dq)() const = &urf::Detector::frontAuto;\n"
                  "urf_front_auto_info (urf::BatchDetector::*bq)() const = &urf::BatchDetector::frontAuto;\n")
    pkg = os.path.join(ROOT, "urban_road_filter_amd")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(pkg, "csrc"), str(tu)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
