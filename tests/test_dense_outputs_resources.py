"""The two kernels behind urf_set_dense_outputs (urf_k_dense.hpp: k_dense_inverse, k_dense_unmap_lists) are in the gfx950 code object, use
no scratch memory and no LDS, and stay streaming kernels; the dense kernels from before are still there without scratch.  hipcc
cross-compiles without a GPU (one compilation per process, shared with the other resource tests)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402
import test_dense_resources as RD  # noqa: E402

NEW = ["k_dense_inverse", "k_dense_unmap_lists"]


@pytest.fixture(scope="module")
def table():
    rows = kernel_resources.resources()
    assert rows, "hipcc did not report kernel resources"
    return {r["name"]: r for r in rows}


@pytest.mark.parametrize("kernel", NEW + RD.DENSE)
def test_the_kernels_are_there_without_scratch(table, kernel):
    assert kernel in table, sorted(k for k in table if "dense" in k)
    assert int(table[kernel]["ScratchSize [bytes/lane]"]) == 0, table[kernel]


def test_the_new_kernels_are_streaming_kernels(table):
    """One load, one dependent load or store per element: a handful of registers, no LDS, 8 waves per SIMD."""
    for k in NEW:
        assert int(table[k]["LDS Size [bytes/block]"]) == 0, table[k]
        assert int(table[k]["VGPRs"]) <= 16 and int(table[k]["Occupancy [waves/SIMD]"]) == 8, table[k]
