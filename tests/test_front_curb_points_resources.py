"""The fused front end's instances for curbPoints other than 5 (urf_front.hpp: k_front_cp1 .. k_front_cp8, k_front_finish_cp1 .. _cp8; taken
with urf_set_front_mode(ctx, 3)) exist in the gfx950 code object under their own names and keep their windows in registers: no scratch.
k_front itself keeps its name and what tests/test_kernel_resources.py pins.  hipcc cross-compiles without a GPU."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402


def gate():
    """The curbPoints the host lets through in mode 3: URF_FRONT_CP_MASK (bit cp)."""
    with open(os.path.join(ROOT, "urban_road_filter_amd", "csrc", "urf_front.hpp")) as f:
        m = re.search(r"#define\s+URF_FRONT_CP_MASK\s+(0x[0-9a-fA-F]+)u", f.read())
    assert m, "URF_FRONT_CP_MASK"
    mask = int(m.group(1), 16)
    return [cp for cp in range(1, 9) if (mask >> cp) & 1]


@pytest.fixture(scope="module")
def table():
    rows = kernel_resources.resources()
    assert rows, "hipcc did not report kernel resources"
    return {r["name"]: r for r in rows}


def test_the_gate_holds_five_and_nothing_beyond_eight():
    assert 5 in gate() and len(gate()) > 1


@pytest.mark.parametrize("cp", [1, 2, 3, 4, 6, 7, 8])
def test_every_instance_in_the_gate_exists_without_scratch(table, cp):
    if cp not in gate():
        assert "k_front_cp%d" % cp not in table   # (taken out by measurement: its instance is not built either)
        return
    for name in ("k_front_cp%d" % cp, "k_front_finish_cp%d" % cp):
        assert name in table, sorted(k for k in table if "front" in k)
        assert int(table[name]["ScratchSize [bytes/lane]"]) == 0, table[name]


def test_the_kernels_for_five_keep_their_names(table):
    for name in ("k_front", "k_front_finish"):
        assert name in table and int(table[name]["ScratchSize [bytes/lane]"]) == 0
