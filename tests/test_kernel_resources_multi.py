"""The multi-sector instances of the march (urf_set_front_multi_sector: k_front_ms, k_front32_ms, k_front16_ms, k_front128_ms,
urf_front.hpp) and k_front_sectors (urf_k_front_sectors.hpp) exist in the gfx950 code object under their own names, use no scratch and
stay inside the budgets of their plain siblings: five waves per SIMD (at most 96 VGPRs) at 64 / 32 / 16 lasers, three (at most 168) at
128.  k_front_sectors keeps its LDS below 40 KB per workgroup: four workgroups of 256 threads per CU.  hipcc cross-compiles without a
GPU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

# kernel: (VGPR ceiling, waves per SIMD at least)
BUDGET = {"k_front_ms": (96, 5), "k_front32_ms": (96, 5), "k_front16_ms": (96, 5), "k_front128_ms": (168, 3), "k_front_sectors": (128, 4)}


@pytest.fixture(scope="module")
def table():
    rows = kernel_resources.resources()
    assert rows, "hipcc did not report kernel resources"
    return {r["name"]: r for r in rows}


@pytest.mark.parametrize("kernel", sorted(BUDGET))
def test_instances_exist_without_scratch_inside_their_budget(table, kernel):
    assert kernel in table, sorted(k for k in table if "front" in k)
    r = table[kernel]
    vgprs, waves = BUDGET[kernel]
    assert int(r["ScratchSize [bytes/lane]"]) == 0, r
    assert int(r["VGPRs"]) <= vgprs and int(r["Occupancy [waves/SIMD]"]) >= waves, r


def test_the_sector_pass_leaves_room_for_four_workgroups_per_cu(table):
    assert int(table["k_front_sectors"]["LDS Size [bytes/block]"]) < 40 * 1024


@pytest.mark.parametrize("kernel", ["k_front", "k_front32", "k_front16", "k_front128"])
def test_the_plain_instances_keep_their_names(table, kernel):
    assert kernel in table and int(table[kernel]["ScratchSize [bytes/lane]"]) == 0
