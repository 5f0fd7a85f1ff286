"""urf_set_front_multi_sector_curb_points, the sixth on / off switch of the fused front end, checked as tests/test_front_switches_api.py
checks the other five: declared in include/urf.h, exported by both libraries, wrapped by the Python API, one setter body in
urf::FrontSwitches (detector.hpp) that forwards by name, and both C++ adapters compile with it."""
import ctypes
import os
import re
import subprocess

import urban_road_filter_amd as u
from urban_road_filter_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY, WRAPPER, SETTER = "urf_set_front_multi_sector_curb_points", "set_front_multi_sector_curb_points", "setFrontMultiSectorCurbPoints"


def test_the_switch_is_declared_and_wrapped():
    header = open(os.path.join(ROOT, "include", "urf.h")).read()
    assert re.search(r"\bint\s+%s\s*\(\s*urf_ctx\s*\*\s*ctx\s*,\s*int\s+on\s*\)\s*;" % ENTRY, header)
    assert re.search(r"#define\s+URF_ABI_VERSION\s+5\b", header)   # (an addition: the version stays)
    assert callable(getattr(u.Context, WRAPPER, None))
    f = getattr(u.lib(), ENTRY)
    assert list(f.argtypes) == [ctypes.c_void_p, ctypes.c_int] and f.restype is ctypes.c_int
    src = open(api.__file__).read()
    assert '"%s": [vp, C.c_int]' % ENTRY in src and "self._lib.%s(self._h, int(on))" % ENTRY in src


def test_the_libraries_export_it():
    for lib in (ctypes.CDLL(os.path.join(os.path.dirname(api.__file__), "liburf_hip.so")), u.lib()):
        assert hasattr(lib, ENTRY)
        for on in (0, 1, 2):
            assert getattr(lib, ENTRY)(None, on) == -1   # (no context: URF_ERR_INVALID_ARG, before anything touches a device)


def test_the_setter_forwards_to_the_entry_point_of_its_name():
    hpp = open(os.path.join(os.path.dirname(api.__file__), "csrc", "detector.hpp")).read()
    base = re.search(r"class\s+FrontSwitches\s*\{(.*?)\n\};", hpp, re.S).group(1)
    bodies = re.findall(r"void\s+%s\s*\(\s*bool\s+on\s*\)\s*\{([^}]*)\}" % SETTER, hpp)
    assert len(bodies) == 1 and bodies[0] in base, bodies
    assert re.fullmatch(r'\s*set\s*\(\s*%s\s*,\s*"%s"\s*,\s*on\s*\)\s*;\s*' % (ENTRY, ENTRY), bodies[0]), bodies[0]


def test_the_adapters_compile_with_the_setter(tmp_path):
    tu = tmp_path / "setter.cpp"
    tu.write_text('#include "detector.hpp"\n'
                  "void both(urf::Detector& d, urf::BatchDetector& b) { d.%s(true); b.%s(false); }\n" % (SETTER, SETTER) +
                  "void (urf::Detector::*pd)(bool) = &urf::Detector::%s;\nvoid (urf::BatchDetector::*pb)(bool) = &urf::BatchDetector::%s;\n" % (SETTER, SETTER))
    pkg = os.path.join(ROOT, "urban_road_filter_amd")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(pkg, "csrc"), str(tu)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
