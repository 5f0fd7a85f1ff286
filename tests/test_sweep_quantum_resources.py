"""k_pc2_to_soa_pad -- the record gather of a sweep padded to a quantum of points (urf_set_sweep_quantum) -- exists in the gfx950 code
object next to k_pc2_to_soa, which it leaves as it is; it uses no scratch memory and no LDS, and its VGPR count is the one written here.
Printed the way tests/test_sweep_outputs_resources.py prints its kernels.  hipcc cross-compiles without a GPU."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

PAD_VGPRS = 34       # k_pc2_to_soa_pad, hipcc -O3 for gfx950
GATHER_VGPRS = 34    # k_pc2_to_soa: what it was before the pad kernel stood next to it


@pytest.fixture(scope="module")
def table():
    rows = kernel_resources.resources()
    assert rows, "hipcc did not report kernel resources"
    return {r["name"]: r for r in rows}


def figures(r):
    return (int(r["VGPRs"]), int(r["ScratchSize [bytes/lane]"]), int(r["Occupancy [waves/SIMD]"]), int(r["LDS Size [bytes/block]"]))


@pytest.mark.parametrize("kernel,want", [("k_pc2_to_soa_pad", PAD_VGPRS), ("k_pc2_to_soa", GATHER_VGPRS)])
def test_the_gathers_use_no_scratch_and_the_registers_written_here(table, kernel, want):
    assert kernel in table, sorted(k for k in table if "pc2" in k)
    vgprs, scratch, occupancy, lds = figures(table[kernel])
    print("%s: %d VGPRs, %d bytes of scratch per lane, %d waves per SIMD, %d bytes of LDS per block" % (kernel, vgprs, scratch, occupancy, lds))
    assert scratch == 0 and lds == 0, table[kernel]
    assert vgprs == want, table[kernel]
    assert occupancy == 8   # (a streaming kernel: nothing keeps a SIMD from its eight waves)


def test_the_host_launches_it_in_a_padded_sequence_only():
    """slot_launch launches k_pc2_to_soa_pad for a padded sweep and k_pc2_to_soa otherwise; the sweep's length is no kernel argument
    frozen in the graph but a device word, copied in front of the launch; DESIGN.md names the kernel."""
    csrc = os.path.join(ROOT, "urban_road_filter_amd", "csrc")
    api = open(os.path.join(csrc, "urf_api_sweep.hpp")).read()   # (the callback path's part of urf_api.hip's translation unit)

    def function(start):
        text = api[api.index(start):]
        return text[:text.index("\n}\n")]
    body = function("static int slot_launch(")
    assert re.search(r"if \(sl\.pad\)[^;]*hipLaunchKernelGGL\(k_pc2_to_soa_pad,[^;]*sl\.d_n\.p", body, re.S)
    assert re.search(r"else\s+hipLaunchKernelGGL\(k_pc2_to_soa,", body)
    # the path through urf_classify_pc2_async: the stage step, which holds the copy of the length word, stands in front of the sequence
    # step, which holds the capture -- and the copy is nowhere else, so no captured sequence holds it
    sub, stage, seq = function('extern "C" int urf_classify_pc2_async('), function("static int sweep_stage("), function("static int sweep_sequence(")
    copy = "hipMemcpyAsync(sl.d_n.p, sl.h_n.p, sizeof(uint32_t)"
    assert copy in stage and api.count(copy) == 1 and "hipStreamBeginCapture(" not in stage
    assert "hipStreamBeginCapture(" in seq and api.count("hipStreamBeginCapture(") == 1
    assert seq.index("hipStreamBeginCapture(") < seq.index("slot_launch(") < seq.index("hipStreamEndCapture(")
    assert sub.index("sweep_stage(") < sub.index("sweep_sequence(") and "hipStreamBeginCapture(" not in sub
    assert "k_pc2_to_soa_pad" in open(os.path.join(ROOT, "DESIGN.md")).read()
