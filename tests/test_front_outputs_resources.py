"""The read-out kernels for scans of the fused front end (urf_k_front_outputs.hpp) exist in the gfx950 code object under their own names and
use no scratch; the kernels the benchmark and tests/test_kernel_resources.py pin -- k_front, k_label_front, k_label, k_ring -- compile to the
figures they had before these kernels and the early returns in urf_k_outputs.hpp came (VGPRs, scratch, waves per SIMD, LDS: read from a build
of the commit before, same compiler).  hipcc cross-compiles without a GPU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

NEW = ["k_front_out_prep", "k_ring_order_front", "k_marker_ring_front", "k_marker_ring_literal_front", "k_marker_bins_front"]
# kernel: (VGPRs, scratch bytes per lane, waves per SIMD, LDS bytes per block) before
BEFORE = {"k_front": (92, 0, 5, 2048), "k_label_front": (52, 0, 8, 4620), "k_label": (64, 0, 8, 7088), "k_ring": (68, 0, 6, 11832)}


@pytest.fixture(scope="module")
def table():
    rows = kernel_resources.resources()
    assert rows, "hipcc did not report kernel resources"
    return {r["name"]: r for r in rows}


@pytest.mark.parametrize("kernel", NEW)
def test_new_kernels_exist_without_scratch(table, kernel):
    assert kernel in table, sorted(k for k in table if "front" in k)
    assert int(table[kernel]["ScratchSize [bytes/lane]"]) == 0, table[kernel]


@pytest.mark.parametrize("kernel", sorted(BEFORE))
def test_pinned_kernels_are_unchanged(table, kernel):
    r = table[kernel]
    got = (int(r["VGPRs"]), int(r["ScratchSize [bytes/lane]"]), int(r["Occupancy [waves/SIMD]"]), int(r["LDS Size [bytes/block]"]))
    assert got == BEFORE[kernel], (kernel, got)
