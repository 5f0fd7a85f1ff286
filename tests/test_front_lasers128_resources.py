"""The 128-laser instances of the fused front end (k_front128*, k_front_finish128*, urf_front.hpp) exist in the gfx950 code object under their own names, do not
spill and stay inside the budgets DESIGN.md section 4 states: k_front128 -- one wave, two lasers per lane, two windows -- 151 VGPRs at
three waves per SIMD (ceiling 168: what three waves leave each); its siblings the figures of the 64-lane kernels they mirror.  The
kernels of urf_front.hpp keep their names and stay free of scratch.  hipcc cross-compiles without a GPU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

# kernel: (VGPR ceiling, waves per SIMD at least)
BUDGET = {"k_front128": (168, 3), "k_front_finish128": (64, 8), "k_label_front128": (64, 8), "k_transpose128": (40, 6),
          "k_rows_probe128": (80, 6)}


@pytest.fixture(scope="module")
def table():
    rows = kernel_resources.resources()
    assert rows, "hipcc did not report kernel resources"
    return {r["name"]: r for r in rows}


@pytest.mark.parametrize("kernel", sorted(BUDGET))
def test_instances_exist_without_scratch_inside_their_budget(table, kernel):
    assert kernel in table, sorted(k for k in table if "front" in k or "128" in k)
    r = table[kernel]
    vgprs, waves = BUDGET[kernel]
    assert int(r["ScratchSize [bytes/lane]"]) == 0, r
    assert int(r["VGPRs"]) <= vgprs and int(r["Occupancy [waves/SIMD]"]) >= waves, r


@pytest.mark.parametrize("kernel", ["k_front", "k_front32", "k_front16", "k_front_finish", "k_label_front", "k_transpose", "k_rows_probe"])
def test_the_kernels_of_64_lanes_keep_their_names(table, kernel):
    assert kernel in table and int(table[kernel]["ScratchSize [bytes/lane]"]) == 0
