"""The id kernels of urf_k_dense.hpp (laser ids from the points' elevation) are in the gfx950 code object and use no scratch memory, and
the five dense kernels they run in front of are still there.  hipcc cross-compiles without a GPU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402
from test_dense_resources import DENSE  # noqa: E402

IDS = ["k_dense_ids_soa", "k_dense_ids_pc2"]


@pytest.fixture(scope="module")
def table():
    rows = kernel_resources.resources()
    assert rows, "hipcc did not report kernel resources"
    return {r["name"]: r for r in rows}


@pytest.mark.parametrize("kernel", IDS + DENSE)
def test_the_kernels_are_there_without_scratch(table, kernel):
    assert kernel in table, sorted(k for k in table if "dense" in k)
    assert int(table[kernel]["ScratchSize [bytes/lane]"]) == 0, table[kernel]


def test_the_id_kernels_keep_eight_workgroups_per_cu(table):
    """256 threads, 127 thresholds + 128 slots in LDS (640 bytes): nothing that limits occupancy below a streaming kernel's."""
    for k in IDS:
        assert int(table[k]["LDS Size [bytes/block]"]) <= 1024, table[k]
        assert int(table[k]["VGPRs"]) <= 64, table[k]
