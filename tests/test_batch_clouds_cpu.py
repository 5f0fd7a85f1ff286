"""The batch clouds' ABI without a GPU: both libraries export urf_classify_batch_pc2_ragged / urf_clouds_batch_soa /
urf_clouds_batch_pc2, struct urf_point_xyzi of include/urf.h has pcl::PointXYZI's layout (and the binding's), and the
C++ batch adapter (tests/cpp/batch_detector_demo.cpp) builds against the product library alone."""
import ctypes
import os
import shutil
import subprocess

import pytest

import urban_road_filter_amd as u

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("urf_classify_batch_pc2_ragged", "urf_clouds_batch_soa", "urf_clouds_batch_pc2")


@pytest.mark.parametrize("hooks", [False, True], ids=["product", "hooks"])
def test_both_libraries_export_the_batch_cloud_entry_points(hooks):
    L = ctypes.CDLL(u.lib_path(hooks=hooks))
    assert [n for n in NEW if not hasattr(L, n)] == []
    assert u.ORDER_INPUT == 0 and u.ORDER_REFERENCE == 1


def test_point_record_layout(tmp_path):
    """urf_point_xyzi as a C compiler lays it out from include/urf.h, against the ctypes binding: 32 bytes, x y z w at 0 / 4 / 8 / 12,
    intensity at 16, pad at 20 (pcl::PointXYZI)."""
    want = {"size": 32, "x": 0, "y": 4, "z": 8, "w": 12, "intensity": 16, "pad": 20}
    got = {"size": ctypes.sizeof(u.PointXYZI)}
    got.update({k: getattr(u.PointXYZI, k).offset for k in ("x", "y", "z", "w", "intensity", "pad")})
    assert got == want
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "urf.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(urf_point_xyzi), offsetof(urf_point_xyzi, x), offsetof(urf_point_xyzi, y),\n'
                   '         offsetof(urf_point_xyzi, z), offsetof(urf_point_xyzi, w), offsetof(urf_point_xyzi, intensity),\n'
                   '         offsetof(urf_point_xyzi, pad));\n  printf("%d %d\\n", URF_ORDER_INPUT, URF_ORDER_REFERENCE);\n  return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [want[k] for k in ("size", "x", "y", "z", "w", "intensity", "pad")] + [0, 1]


def test_batch_adapter_builds_against_the_product_library(tmp_path):
    """What test_abi.py's test_cpp_clients_build_against_the_product_library checks for the other clients: g++, csrc/detector.hpp and
    include/urf.h, linked against liburf_hip.so only, and every urf symbol the client needs is exported by it."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    u.lib()
    pkg = os.path.join(ROOT, "urban_road_filter_amd")
    exe = str(tmp_path / "batch_detector_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(pkg, "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "batch_detector_demo.cpp"), "-o", exe,
                           "-L" + pkg, "-l:liburf_hip.so", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"])
    undefined = subprocess.run(["nm", "-u", exe], capture_output=True, text=True).stdout.split()
    wanted = {w.split("@")[0] for w in undefined if "urf" in w}
    exported = set(subprocess.run(["nm", "-D", "--defined-only", u.lib_path()], capture_output=True, text=True).stdout.split())
    assert any("BatchDetector" in w for w in wanted) and wanted <= exported, wanted - exported
