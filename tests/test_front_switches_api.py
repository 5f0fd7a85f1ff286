"""The five on / off switches of the fused front end -- urf_set_front_outputs, _lasers128, _long_sweeps, _curb_points, _multi_sector -- each
declared in include/urf.h (tests/test_abi.py: then exported), exported by the library, wrapped by the Python API and passed through by both
C++ adapters (urf::Detector, urf::BatchDetector), which have their setters from one base (urf::FrontSwitches, detector.hpp)."""
import ctypes
import os
import re
import subprocess

import pytest

import urban_road_filter_amd as u
from urban_road_filter_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (entry point, Python wrapper, adapter setter)
SWITCHES = [("urf_set_front_outputs", "set_front_outputs", "setFrontOutputs"),
            ("urf_set_front_lasers128", "set_front_lasers128", "setFrontLasers128"),
            ("urf_set_front_long_sweeps", "set_front_long_sweeps", "setFrontLongSweeps"),
            ("urf_set_front_curb_points", "set_front_curb_points", "setFrontCurbPoints"),
            ("urf_set_front_multi_sector", "set_front_multi_sector", "setFrontMultiSector")]
switches = pytest.mark.parametrize("entry,wrapper,setter", SWITCHES, ids=[s[1] for s in SWITCHES])


@switches
def test_the_switch_is_declared_and_wrapped(entry, wrapper, setter):
    header = open(os.path.join(ROOT, "include", "urf.h")).read()
    assert re.search(r"\bint\s+%s\s*\(\s*urf_ctx\s*\*\s*ctx\s*,\s*int\s+on\s*\)\s*;" % entry, header)
    assert callable(getattr(u.Context, wrapper, None))
    f = getattr(u.lib(), entry)
    assert list(f.argtypes) == [ctypes.c_void_p, ctypes.c_int] and f.restype is ctypes.c_int
    src = open(api.__file__).read()
    assert '"%s": [vp, C.c_int]' % entry in src and "self._lib.%s(self._h, int(on))" % entry in src


@switches
def test_the_library_exports_it(entry, wrapper, setter):
    for lib in (ctypes.CDLL(os.path.join(os.path.dirname(api.__file__), "liburf_hip.so")), u.lib()):
        assert hasattr(lib, entry)
        for on in (0, 1, 2):
            assert getattr(lib, entry)(None, on) == -1   # (no context: URF_ERR_INVALID_ARG, before anything touches a device)


@switches
def test_the_setter_forwards_to_the_entry_point_of_its_name(entry, wrapper, setter):
    """Once, in the base both adapters have it from (that both have it: the compile check below)."""
    hpp = open(os.path.join(os.path.dirname(api.__file__), "csrc", "detector.hpp")).read()
    base = re.search(r"class\s+FrontSwitches\s*\{(.*?)\n\};", hpp, re.S).group(1)
    bodies = re.findall(r"void\s+%s\s*\(\s*bool\s+on\s*\)\s*\{([^}]*)\}" % setter, hpp)
    assert len(bodies) == 1 and bodies[0] in base, (setter, bodies)
    assert re.fullmatch(r'\s*set\s*\(\s*%s\s*,\s*"%s"\s*,\s*on\s*\)\s*;\s*' % (entry, entry), bodies[0]), bodies[0]
    # ... and set() calls what it is handed with the adapter's context and throws an Error with the name it is handed
    helper = re.search(r"void\s+set\s*\(\s*int\s*\(\s*\*\s*entry\s*\)\s*\(\s*urf_ctx\s*\*\s*,\s*int\s*\)\s*,\s*const\s+char\s*\*\s*name\s*,\s*bool\s+on\s*\)\s*\{(.*?)\n    \}", base, re.S)
    assert helper and re.search(r"entry\s*\(\s*ctx_\s*,\s*on\s*\?\s*1\s*:\s*0\s*\)", helper.group(1)) and re.search(r"throw\s+Error\s*\(\s*rc\s*,\s*name\s*\)", helper.group(1))


def test_the_adapters_compile_with_their_setters(tmp_path):
    tu = tmp_path / "setters.cpp"
    names = [s[2] for s in SWITCHES]
    tu.write_text('#include "detector.hpp"\n'
                  "void both(urf::Detector& d, urf::BatchDetector& b) { %s }\n" % " ".join("d.%s(true); b.%s(false);" % (n, n) for n in names) +
                  "".join("void (urf::Detector::*d%d)(bool) = &urf::Detector::%s;\nvoid (urf::BatchDetector::*b%d)(bool) = &urf::BatchDetector::%s;\n" % (k, n, k, n)
                          for k, n in enumerate(names)))
    pkg = os.path.join(ROOT, "urban_road_filter_amd")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(pkg, "csrc"), str(tu)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
