"""The two kernels of urf_set_sweep_outputs with both bits -- k_sweep_rings (published order and marker tables of a ring in one
workgroup) and k_sweep_lists (ordered lists and marker points in one launch) -- exist in the gfx950 code object, use no scratch memory, and
their LDS is what one workgroup may ask for; k_ring_order and k_marker_ring, now instances of the same body (urf_ring_readout), keep
theirs.  VGPRs, LDS and occupancy are printed the way tests/test_front_outputs_resources.py reads them.  hipcc cross-compiles without a GPU."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

NEW = ["k_sweep_rings", "k_sweep_lists"]
INSTANCES = ["k_ring_order", "k_marker_ring", "k_ordered_lists"]
LDS_PER_WORKGROUP = 160 * 1024  # a CU's LDS: what the runtime grants one workgroup on the MI355X without being asked (urf_api.hip: long_sweeps_lds)
MAP_LDS = (2 * 4096 + 1) * 4    # the dynamic part of the per-ring kernels at URF_MAX_TILES tiles: the ring's run table


@pytest.fixture(scope="module")
def table():
    rows = kernel_resources.resources()
    assert rows, "hipcc did not report kernel resources"
    return {r["name"]: r for r in rows}


def figures(r):
    return (int(r["VGPRs"]), int(r["ScratchSize [bytes/lane]"]), int(r["Occupancy [waves/SIMD]"]), int(r["LDS Size [bytes/block]"]))


@pytest.mark.parametrize("kernel", NEW + INSTANCES)
def test_kernels_exist_without_scratch(table, kernel):
    assert kernel in table, sorted(k for k in table if "sweep" in k or "ring" in k)
    vgprs, scratch, occupancy, lds = figures(table[kernel])
    print("%s: %d VGPRs, %d bytes of scratch per lane, %d waves per SIMD, %d bytes of LDS per block" % (kernel, vgprs, scratch, occupancy, lds))
    assert scratch == 0, table[kernel]
    assert lds + (MAP_LDS if kernel in ("k_sweep_rings", "k_ring_order", "k_marker_ring") else 0) <= LDS_PER_WORKGROUP, table[kernel]
    assert occupancy >= 1


def test_the_merged_ring_kernel_holds_what_its_two_parts_hold(table):
    """k_sweep_rings = the sort's 16 KiB of keys, counters and scratch (k_ring_order) + the three 361-entry marker tables (k_marker_ring)
    + the ring's entries by position (8 KiB): not less than the two together, not more than that plus the staging."""
    both, order, mark = (figures(table[k])[3] for k in ("k_sweep_rings", "k_ring_order", "k_marker_ring"))
    assert order >= 2048 * 8 and mark >= 361 * 16
    assert order + mark - 64 <= both <= order + mark + 2048 * 4 + 64, (both, order, mark)


def test_the_host_launches_them_and_names_them():
    """The read-out chain (launch_readouts, urf_api.hip: the one launcher of the callback path's sequence and of the batch read-backs)
    launches the new kernels with both bits and the existing ones otherwise, each from one place, as one linear chain;
    sweep_outputs_launch (urf_api_sweep.hpp) is that chain and nothing that forks or joins; DESIGN.md section 4 names them.
    (urf_kernel_name's table is the eight timed stages of the classification, URF_NUM_KERNELS, fixed by the ABI: the read-out kernels
    never had a stage there.)"""
    csrc = os.path.join(ROOT, "urban_road_filter_amd", "csrc")
    api = open(os.path.join(csrc, "urf_api.hip")).read()
    sweep = open(os.path.join(csrc, "urf_api_sweep.hpp")).read()
    chain = api[api.index("static int launch_readouts("):]
    chain = chain[:chain.index("\n}\n")]
    body = sweep[sweep.index("static int sweep_outputs_launch("):]
    body = body[:body.index("\n}\n")]
    for k in NEW + ["k_ring_order", "k_marker_ring", "k_marker_ring_literal", "k_ordered_lists", "k_marker_bins", "k_front_out_prep",
                    "k_ring_order_front", "k_marker_ring_front", "k_marker_ring_literal_front", "k_marker_bins_front"]:
        assert re.search(r"hipLaunchKernelGGL\(%s," % k, chain), k
        assert len(re.findall(r"hipLaunchKernelGGL\(%s," % k, api + sweep)) == 1, k   # ... and from nowhere else
    assert "launch_readouts(" in body and "hipLaunchKernelGGL" not in body
    for text in (chain, body):
        assert "hipStreamWaitEvent" not in text and "hipEventRecord" not in text   # one linear chain: no fork, no join
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for k in NEW:
        assert k in design, k
