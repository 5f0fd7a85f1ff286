"""The kernels of urf_k_dense.hpp (dense sweeps put back into firing slots by laser id) are in the gfx950 code object and use no scratch
memory, and every kernel that test_front_long_sweeps_resources.py lists is still there without it.  hipcc cross-compiles without a GPU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402
import test_front_long_sweeps_resources as RL  # noqa: E402

DENSE = ["k_dense_count", "k_dense_scan", "k_dense_scatter_soa", "k_dense_scatter_pc2", "k_dense_labels"]


@pytest.fixture(scope="module")
def table():
    rows = kernel_resources.resources()
    assert rows, "hipcc did not report kernel resources"
    return {r["name"]: r for r in rows}


@pytest.mark.parametrize("kernel", DENSE + RL.LISTED)
def test_the_kernels_are_there_without_scratch(table, kernel):
    assert kernel in table, sorted(k for k in table if "dense" in k)
    assert int(table[kernel]["ScratchSize [bytes/lane]"]) == 0, table[kernel]


def test_the_dense_kernels_fit_eight_workgroups_per_cu(table):
    """256 threads, a 256-byte map and a few words of LDS: nothing that limits occupancy below the 8 waves per SIMD of a streaming kernel."""
    for k in DENSE:
        assert int(table[k]["LDS Size [bytes/block]"]) <= 1024, table[k]
        assert int(table[k]["VGPRs"]) <= 64, table[k]
