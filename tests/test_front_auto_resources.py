"""k_front_digest (urf_k_front_digest.hpp: the learning pass of urf_set_front_auto) exists in the gfx950 code object under its own name, uses
no scratch and no LDS and spills nothing; k_front_explain, whose header gained the per-scan rule both share, compiles to the figures it
had.  The figures are written down in profiles/front_auto_resources.json from what the compiler reports; hipcc cross-compiles without a GPU."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

FIELDS = (("vgprs", "VGPRs"), ("agprs", "AGPRs"), ("sgprs", "TotalSGPRs"), ("scratch_bytes_per_lane", "ScratchSize [bytes/lane]"), ("sgpr_spills", "SGPRs Spill"),
          ("vgpr_spills", "VGPRs Spill"), ("waves_per_simd", "Occupancy [waves/SIMD]"), ("lds_bytes_per_block", "LDS Size [bytes/block]"))


@pytest.fixture(scope="module")
def table():
    rows = kernel_resources.resources()
    assert rows, "hipcc did not report kernel resources"
    return {r["name"]: r for r in rows}


def test_the_digest_kernel_exists_without_scratch(table):
    assert "k_front_digest" in table, sorted(k for k in table if "front" in k)
    r = table["k_front_digest"]
    assert int(r["ScratchSize [bytes/lane]"]) == 0 and r["Dynamic Stack"] == "False", r
    assert int(r["LDS Size [bytes/block]"]) == 0 and int(r["SGPRs Spill"]) == 0 and int(r["VGPRs Spill"]) == 0, r


@pytest.mark.parametrize("kernel", ["k_front_digest", "k_front_explain"])
def test_the_figures_written_down_are_the_compilers(table, kernel):
    noted = {k["name"]: k for k in json.load(open(os.path.join(ROOT, "profiles", "front_auto_resources.json")))["kernels"]}
    assert {key: noted[kernel][key] for key, _ in FIELDS} == {key: int(table[kernel][col]) for key, col in FIELDS}
