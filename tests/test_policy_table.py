"""The launch policy on the CPU: tests/cpp/policy_table.cpp runs urf_policy::plan and urf_front_family_of (csrc/urf_policy.hpp, no HIP) over a
fixed cross product of policy states and calls.

(1) Its checksums equal tests/golden/policy_table.json, recorded when plan() and the choice of the fused kernels had been moved into the header
word for word, before anything in them was rearranged: the file holds the decisions of the code before the move.  A slice that differs is
located with `policy_table --rows MODE:CHANNELS`, row by row against a build of the earlier header.
(2) The Python shadow of plan()'s history-free part (tests/fuzz_history.py: Shadow.excluded), which the call-history tests steer by, agrees
with the real function on every row it can speak about."""
import json
import os
import subprocess

import numpy as np
import pytest

import fuzz_history as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES, CHANNELS = (0, 1, 2, 3), (8, 16, 32, 64, 128)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("policy") / "policy_table")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "urban_road_filter_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "policy_table.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_the_decisions_are_the_recorded_ones(program):
    with open(os.path.join(ROOT, "tests", "golden", "policy_table.json")) as f:
        want = json.load(f)
    got = {}
    for line in subprocess.run([program], capture_output=True, text=True, check=True).stdout.splitlines():
        name, rows, fnv = line.split()
        got[name] = {"rows": int(rows), "fnv1a64": fnv}
    assert sorted(got) == sorted(["%d:%d" % (m, c) for m in MODES for c in CHANNELS] + ["spec"])
    assert {k: v for k, v in got.items() if v != want.get(k)} == {}   # (the slices that differ, with what they give now)
    assert got == want


def rows_of(program, mode, channels, want, *where):
    """The columns `want` of the slice's rows as integer arrays (the program prints fixed width: two header lines, names and widths)."""
    out = subprocess.run([program, "--rows", "%d:%d" % (mode, channels)] + list(where), capture_output=True, check=True).stdout
    names, widths, body = out.split(b"\n", 2)
    names, widths = names.decode().split()[1:], [int(w) for w in widths.decode().split()[2:]]
    assert len(names) == len(widths)
    line = sum(widths) + len(widths)   # (a space between two columns, the newline)
    assert len(body) % line == 0 and len(body) > 0
    text = np.frombuffer(body, np.uint8).reshape(-1, line)
    cols, at = {}, 0
    for name, w in zip(names, widths):   # (front_tpb stands twice, the setting and the decision: not asked for here)
        if name in want:
            digits = text[:, at:at + w].astype(np.int64)
            assert name not in cols and ((digits == 32) | ((digits >= 48) & (digits <= 57))).all(), name
            cols[name] = (np.where(digits == 32, 0, digits - 48) * 10 ** np.arange(w - 1, -1, -1)).sum(axis=1)
        at += w + 1
    assert sorted(cols) == sorted(want)
    return cols


@pytest.mark.parametrize("mode", MODES)
def test_the_shadow_of_the_history_tests_agrees_with_plan(program, mode):
    """Where Shadow.excluded says "excluded", plan() launches no fused kernel; where it says "not excluded" on a batch call in mode 2 or 3
    with want_ring_sorted clear, plan() launches them.  The rows: the switches the shadow does not know off (curb_points, multi_sector), no
    general_only, front_off clear (the shadow calls both history)."""
    n = 0
    for channels in CHANNELS:
        seen = ("lasers128", "long_sweeps", "capture", "curbPoints", "tiles", "want_ring_sorted")
        c = rows_of(program, mode, channels, seen + ("front_mode", "channels", "slot", "front"),
                    "curb_points=0", "multi_sector=0", "general_only=0", "front_off=0")
        assert (c["front_mode"] == mode).all() and (c["channels"] == channels).all()
        packed = sum(c[k] << (10 * i) for i, k in enumerate(seen))   # (every value is below 1024)
        keys, inverse = np.unique(packed, return_inverse=True)
        excluded = np.zeros(len(keys), bool)
        for i, key in enumerate(keys.tolist()):
            l128, long_sweeps, capture, cp, tiles, wrs = ((key >> (10 * j)) & 1023 for j in range(len(seen)))
            s = H.Shadow("small")
            s.mode, s.l128, s.long, s.capture, s.wrs = mode, l128, long_sweeps, capture, bool(wrs)
            s.tag = "L%d/-/cp%d" % (channels, cp)
            assert (s.lasers, H.tag_curb_points(s.tag)) == (channels, cp)
            excluded[i] = s.excluded(tiles)
        excluded = excluded[inverse.reshape(-1)]
        assert (c["front"][excluded] == 0).all()
        certain = ~excluded & (c["slot"] == 0) & (c["want_ring_sorted"] == 0) & (mode >= 2)
        assert (c["front"][certain] == 1).all()
        assert excluded.any() and (mode < 2 or channels == 8 or certain.any())
        n += len(excluded)
    assert n == 5 * 6451200 // 16   # every row of the five slices with the four values above
