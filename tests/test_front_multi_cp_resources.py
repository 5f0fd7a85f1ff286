"""The multi-sector instances of the march for curbPoints other than 5 (urf_front.hpp: k_front_ms_cp<n>, k_front32_ms_cp<n>,
k_front16_ms_cp<n>, k_front128_ms_cp<n>, n of URF_FRONT_CP_OTHERS; taken with urf_set_front_multi_sector_curb_points on top of
urf_set_front_multi_sector) exist in the gfx950 code object under their own names and keep their windows in registers: no scratch.  The four
instances for curbPoints 5 keep their names.  hipcc cross-compiles without a GPU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

MARCHES = ("k_front16_ms", "k_front32_ms", "k_front_ms", "k_front128_ms")


@pytest.fixture(scope="module")
def table():
    rows = kernel_resources.resources()
    assert rows, "hipcc did not report kernel resources"
    return {r["name"]: r for r in rows}


@pytest.mark.parametrize("cp", [1, 2, 3, 4, 6, 7, 8])
@pytest.mark.parametrize("march", MARCHES)
def test_every_instance_exists_without_scratch(table, march, cp):
    name = "%s_cp%d" % (march, cp)
    assert name in table, sorted(k for k in table if "_ms" in k)
    r = table[name]
    print("%s: %s VGPRs, %s waves per SIMD, LDS %s" % (name, r.get("VGPRs"), r.get("Occupancy [waves/SIMD]"), r.get("LDS Size [bytes/block]")))
    assert int(r["ScratchSize [bytes/lane]"]) == 0, r


def test_there_are_twenty_eight_of_them(table):
    assert len([k for k in table if "_ms_cp" in k]) == 28


def test_the_kernels_for_five_keep_their_names(table):
    for name in MARCHES:
        assert name in table and int(table[name]["ScratchSize [bytes/lane]"]) == 0
