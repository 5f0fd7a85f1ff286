"""The two kernels of urf_set_sweep_results_direct -- k_sweep_lists_direct (the packed lists and the marker points in one launch, 384
threads) and k_ordered_lists_direct (the packed lists alone, 256 threads) -- exist in the gfx950 code object, use no scratch memory and
leave room for at least one wave; their siblings with the strided layout, instances of the same body (urf_ordered_lists), keep theirs.
VGPRs, LDS and occupancy are printed the way tests/test_sweep_outputs_resources.py reads them.  hipcc cross-compiles without a GPU."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

NEW = ["k_sweep_lists_direct", "k_ordered_lists_direct"]
SIBLINGS = {"k_sweep_lists_direct": "k_sweep_lists", "k_ordered_lists_direct": "k_ordered_lists"}
LDS_PER_WORKGROUP = 160 * 1024


@pytest.fixture(scope="module")
def table():
    rows = kernel_resources.resources()
    assert rows, "hipcc did not report kernel resources"
    return {r["name"]: r for r in rows}


def figures(r):
    return (int(r["VGPRs"]), int(r["ScratchSize [bytes/lane]"]), int(r["Occupancy [waves/SIMD]"]), int(r["LDS Size [bytes/block]"]))


@pytest.mark.parametrize("kernel", NEW + sorted(SIBLINGS.values()))
def test_kernels_exist_without_scratch(table, kernel):
    assert kernel in table, sorted(k for k in table if "lists" in k)
    vgprs, scratch, occupancy, lds = figures(table[kernel])
    print("%s: %d VGPRs, %d SGPRs, %d bytes of scratch per lane, %d waves per SIMD, %d bytes of LDS per block" % (
        kernel, vgprs, int(table[kernel].get("TotalSGPRs", -1)), scratch, occupancy, lds))
    assert scratch == 0, table[kernel]
    assert lds <= LDS_PER_WORKGROUP, table[kernel]
    assert occupancy >= 1


@pytest.mark.parametrize("kernel", NEW)
def test_the_packed_body_adds_two_words_of_lds(table, kernel):
    """The scan's two totals beside the two bases: a few bytes, no table."""
    lds, sibling = figures(table[kernel])[3], figures(table[SIBLINGS[kernel]])[3]
    assert sibling <= lds <= sibling + 64, (lds, sibling)


def test_the_host_launches_them_and_copies_nothing_for_them():
    """The read-out chain (launch_readouts, urf_api.hip) launches the new kernels beside the ones it had, still as one linear chain,
    and sweep_outputs_launch (urf_api_sweep.hpp), which is that chain and two copies, returns in front of the copies when the switch is
    on; DESIGN.md section 4 names them."""
    csrc = os.path.join(ROOT, "urban_road_filter_amd", "csrc")
    api = open(os.path.join(csrc, "urf_api.hip")).read()
    sweep = open(os.path.join(csrc, "urf_api_sweep.hpp")).read()
    chain = api[api.index("static int launch_readouts("):]
    chain = chain[:chain.index("\n}\n")]
    body = sweep[sweep.index("static int sweep_outputs_launch("):]
    body = body[:body.index("\n}\n")]
    for k in NEW:
        assert re.search(r"hipLaunchKernelGGL\(%s," % k, chain), k
    for text in (chain, body):
        assert "hipStreamWaitEvent" not in text and "hipEventRecord" not in text
    assert "hipMemcpy" not in chain and body.count("hipMemcpyAsync") == 2
    assert body.index("launch_readouts(") < body.index("if (direct)\n        return URF_OK;") < body.index("hipMemcpyAsync")
    alloc = sweep[sweep.index("static int sweep_outputs_alloc("):]
    assert "hipHostMallocMapped | hipHostMallocCoherent" in alloc[:alloc.index("\n}\n")]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for k in NEW:
        assert k in design, k
