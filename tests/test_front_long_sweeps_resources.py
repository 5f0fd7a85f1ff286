"""urf_set_front_long_sweeps sends scans of 129..256 tiles through the finish kernels the fused front end already has, with more dynamic
LDS (instances of their own were built, measured slower at 128 x 4096 and taken out again): the gfx950 code object still holds every kernel that
test_front_lasers128_resources.py lists, free of scratch.  hipcc cross-compiles
without a GPU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402
import test_front_lasers128_resources as R128  # noqa: E402

LISTED = sorted(R128.BUDGET) + ["k_front", "k_front32", "k_front16", "k_front_finish", "k_label_front", "k_transpose", "k_rows_probe"]


@pytest.fixture(scope="module")
def table():
    rows = kernel_resources.resources()
    assert rows, "hipcc did not report kernel resources"
    return {r["name"]: r for r in rows}


@pytest.mark.parametrize("kernel", LISTED)
def test_the_listed_kernels_are_still_there_without_scratch(table, kernel):
    assert kernel in table, sorted(k for k in table if "front" in k or "128" in k)
    assert int(table[kernel]["ScratchSize [bytes/lane]"]) == 0, table[kernel]
