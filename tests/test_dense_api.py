"""The dense-sweep entry points (urf_classify_batch_soa_dense, urf_classify_batch_pc2_dense, urf_set_dense_slots, urf_dense_scans) are
declared in include/urf.h (tests/test_abi.py: then exported), wrapped by the Python API, and the C++ adapter's BatchDetector has
setDenseRealign / denseAligned."""
import ctypes
import os
import re

import urban_road_filter_amd as u
from urban_road_filter_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("urf_classify_batch_soa_dense", "urf_classify_batch_pc2_dense", "urf_set_dense_slots", "urf_dense_scans")


def _header():
    src = open(os.path.join(ROOT, "include", "urf.h")).read()
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


def test_the_four_entry_points_are_declared():
    h = _header()
    assert ("int urf_classify_batch_soa_dense(urf_ctx* ctx, const float* d_x, const float* d_y, const float* d_z, const void* d_laser, "
            "uint32_t laser_bytes, const uint32_t* d_offsets, uint32_t max_len, uint32_t n_scans, uint32_t max_firings, uint8_t* d_labels, "
            "urf_scan_info* d_info);") in h
    assert ("int urf_classify_batch_pc2_dense(urf_ctx* ctx, const uint8_t* d_data, const uint32_t* d_offsets, uint64_t n_total, "
            "uint32_t max_len, uint32_t n_scans, uint32_t point_step, uint32_t off_x, uint32_t off_y, uint32_t off_z, uint32_t off_laser, "
            "uint32_t laser_bytes, uint32_t max_firings, uint8_t* d_labels, urf_scan_info* d_info);") in h
    assert "int urf_set_dense_slots(urf_ctx* ctx, const uint8_t* slot_of_id, uint32_t n_ids);" in h
    assert "int urf_dense_scans(urf_ctx* ctx, uint32_t* n_aligned);" in h
    assert "#define URF_ABI_VERSION 5" in h and "#define URF_NUM_KERNELS 8" in h   # additive


def test_the_library_exports_them_and_refuses_a_null_context_first():
    lib = ctypes.CDLL(os.path.join(os.path.dirname(api.__file__), "liburf_hip.so"))
    for n in NAMES:
        assert hasattr(lib, n), n
    one = ctypes.c_void_p(16)   # (never dereferenced: the context is looked at first, before anything touches a device)
    u32, u64 = ctypes.c_uint32, ctypes.c_uint64
    lib.urf_classify_batch_soa_dense.argtypes = [ctypes.c_void_p] * 5 + [u32, ctypes.c_void_p, u32, u32, u32, ctypes.c_void_p, ctypes.c_void_p]
    lib.urf_classify_batch_pc2_dense.argtypes = [ctypes.c_void_p] * 3 + [u64] + [u32] * 9 + [ctypes.c_void_p, ctypes.c_void_p]
    lib.urf_set_dense_slots.argtypes = [ctypes.c_void_p, ctypes.c_void_p, u32]
    lib.urf_dense_scans.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    assert lib.urf_classify_batch_soa_dense(None, one, one, one, one, 2, one, 64, 1, 4, one, None) == -1
    assert lib.urf_classify_batch_pc2_dense(None, one, one, 64, 64, 1, 32, 0, 4, 8, 20, 2, 4, one, None) == -1
    assert lib.urf_set_dense_slots(None, None, 0) == -1
    n = u32(7)
    assert lib.urf_dense_scans(None, ctypes.byref(n)) == -1


def test_the_cpp_client_builds_against_the_product_library(tmp_path):
    """tests/cpp/batch_dense_demo.cpp (tests/test_gpu_dense.py runs it) with g++, include/urf.h and csrc/detector.hpp only."""
    import shutil
    import subprocess
    import pytest
    if not shutil.which("g++"):
        pytest.skip("no g++")
    u.lib()   # (built)
    pkg = os.path.dirname(api.__file__)
    exe = str(tmp_path / "batch_dense_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(pkg, "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "batch_dense_demo.cpp"), "-o", exe,
                           "-L" + pkg, "-l:liburf_hip.so", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"])
    undefined = subprocess.run(["nm", "-u", exe], capture_output=True, text=True).stdout
    assert "setDenseRealign" in undefined


def test_the_python_api_wraps_them():
    for m in ("classify_batch_soa_dense", "classify_batch_pc2_dense", "set_dense_slots", "dense_scans"):
        assert callable(getattr(u.Context, m, None)), m
    src = open(api.__file__).read()
    for n in NAMES:
        assert '"%s": [' % n in src and "self._lib.%s(self._h" % n in src, n


def test_the_cpp_adapter_has_the_switch():
    hpp = open(os.path.join(os.path.dirname(api.__file__), "csrc", "detector.hpp")).read()
    batch = hpp[hpp.index("class BatchDetector"):]
    assert re.search(r"void\s+setDenseRealign\s*\(\s*uint32_t\s+max_firings\s*,\s*const\s+std::vector<uint8_t>&\s*slot_of_ring\s*=\s*\{\}\s*\)\s*;", batch)
    assert re.search(r"size_t\s+denseAligned\s*\(\s*\)\s*const", batch)
    cpp = open(os.path.join(os.path.dirname(api.__file__), "csrc", "detector.cpp")).read()
    assert "urf_classify_batch_pc2_dense(ctx_" in cpp and "urf_classify_batch_pc2_ragged(ctx_" in cpp and "urf_dense_scans(ctx_" in cpp
