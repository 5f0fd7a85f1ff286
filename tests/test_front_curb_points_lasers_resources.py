"""The fused front end's instances for curbPoints other than 5 at 16, 32 and 128 lasers per firing (urf_set_front_curb_points: k_front32_cp*,
k_front16_cp*, k_front128_cp* and k_front_finish128_cp*, all in urf_front.hpp) exist in the
gfx950 code object under their own names and keep their windows in registers: no scratch.  The register counts are a record (DESIGN.md
section 4: what hipcc reports), pinned as the ceiling the instance's waves per SIMD leave each wave -- 512 registers per SIMD in blocks
of 8: 96 at five waves, 128 at four, 168 at three, 256 at two; a workgroup of k_front_finish128_cp* is four waves, its floor the reported
occupancy.  No spill is the condition.  hipcc cross-compiles without a GPU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

CPS = (1, 2, 3, 4, 6, 7, 8)
# kernel: (VGPR ceiling, waves per SIMD at least).  Reported: k_front32_cp1..8 83 87 91 96 | 105 109 114; k_front16_cp1..8 85 89 93 96 |
# 107 111 116; k_front128_cp1..8 116 126 133 143 161 168 | 179; k_front_finish128_cp1..8 58 58 58 58 | 66 | 74 | 82
BUDGET = {}
for _cp in CPS:
    BUDGET["k_front32_cp%d" % _cp] = BUDGET["k_front16_cp%d" % _cp] = (96, 5) if _cp < 5 else (128, 4)
    BUDGET["k_front128_cp%d" % _cp] = (168, 3) if _cp < 8 else (256, 2)
    BUDGET["k_front_finish128_cp%d" % _cp] = {6: (72, 7), 7: (80, 6), 8: (96, 5)}.get(_cp, (64, 8))


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


@pytest.mark.parametrize("kernel", ["k_front", "k_front32", "k_front16", "k_front128", "k_front_finish", "k_front_finish128", "k_label_front",
                                    "k_label_front128"] + ["k_front_cp%d" % cp for cp in CPS] + ["k_front_finish_cp%d" % cp for cp in CPS])
def test_the_kernels_there_were_keep_their_names(table, kernel):
    assert kernel in table and int(table[kernel]["ScratchSize [bytes/lane]"]) == 0
