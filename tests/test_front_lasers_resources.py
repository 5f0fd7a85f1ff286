"""The fused front end's instances for 32 and 16 lasers per firing (urf_front.hpp: k_front32, k_front16) exist in the gfx950 code
object, do not spill and stay inside the budget k_front's occupancy was tuned for (tests/test_kernel_resources.py: 96 VGPRs, five
waves per SIMD).  hipcc cross-compiles without a GPU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402


@pytest.fixture(scope="module")
def table():
    rows = kernel_resources.resources()
    assert rows, "hipcc did not report kernel resources"
    return {r["name"]: r for r in rows}


@pytest.mark.parametrize("kernel", ["k_front32", "k_front16"])
def test_instances_exist_and_keep_k_fronts_budget(table, kernel):
    assert kernel in table, sorted(k for k in table if "front" in k)
    r = table[kernel]
    assert int(r["ScratchSize [bytes/lane]"]) == 0, r
    assert int(r["VGPRs"]) <= 96 and int(r["Occupancy [waves/SIMD]"]) >= 5, r


def test_the_64_laser_kernel_keeps_its_name(table):
    assert "k_front" in table and int(table["k_front"]["ScratchSize [bytes/lane]"]) == 0
