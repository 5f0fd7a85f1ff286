"""urf_policy::why on the CPU (csrc/urf_policy.hpp, no HIP): the reasons and the advice urf_front_explain reports for the CALL's decision.

tests/cpp/policy_why.cpp walks the cross product of tests/cpp/policy_table.cpp's inputs plus multi_sector_cp (and front_outputs, which
why() reads) and checks on every row: (a) why == 0 <=> plan() fuses the call; (b) the advice applied gives a fused call; (c) the advice
without any one bit does not; (d) NEVER exactly where no mode and no switches fuse the row's channels / curbPoints / tiles.  A few rows
are pinned by name below: what a user of the common sensors is told."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def constants(prefix):
    header = open(os.path.join(ROOT, "include", "urf.h")).read()
    return {m.group(1): int(m.group(2), 16) for m in re.finditer(r"#define\s+%s(\w+)\s+(0x[0-9a-fA-F]+)u" % prefix, header)}


WHY, ADVICE = constants("URF_WHY_CALL_"), constants("URF_ADVICE_")


def bits(table, *names):
    return sum(table[n] for n in names)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("policy") / "policy_why")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "urban_road_filter_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "policy_why.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_the_names_are_one_bit_each():
    assert sorted(WHY) == sorted(["MODE_OFF", "STOPPED", "READOUT", "CAPTURE", "LASERS", "CURB_POINTS", "TILES", "FEW_SCANS", "CALLBACK"])
    assert sorted(ADVICE) == sorted(["MODE_2", "MODE_3", "LASERS128", "LONG_SWEEPS", "CURB_POINTS", "MULTI_SECTOR", "MULTI_SECTOR_CP", "FRONT_OUTPUTS",
                                     "RESET", "CAPTURE_OFF", "BATCH", "NEVER", "CAPACITY", "CALL_AGAIN"])
    for table in (WHY, ADVICE):
        assert all(v and not (v & (v - 1)) for v in table.values()) and len(set(table.values())) == len(table)


def test_every_row_of_the_cross_product(program):
    r = subprocess.run([program], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    rows, front, never, failures = (int(x) for x in re.fullmatch(r"rows (\d+) front (\d+) never (\d+) failures (\d+)\n", r.stdout).groups())
    # policy_table.cpp's 129 024 000 rows, times multi_sector_cp and front_outputs; the fused ones, and the rows nothing helps
    # (channels 8, curbPoints 9 or 257 tiles: 1 - 4/5 * 4/5 * 5/6 of them, less the fused ones' none)
    assert rows == 129024000 * 4 and failures == 0
    assert 0 < front < rows and never == rows * 7 // 15


# (the row's inputs, the terms that are false, the advice)
ROWS = [
    # a VLP-16 stream in the default mode: "mode 2" is all it takes
    ("front_mode=1 channels=16 curbPoints=5 n_scans=192", ["FEW_SCANS"], ["MODE_2"]),
    ("front_mode=1 channels=64 curbPoints=5 n_scans=192", [], []),
    ("front_mode=1 channels=64 curbPoints=5 n_scans=191", ["FEW_SCANS"], ["MODE_2"]),
    ("front_mode=0 channels=64 curbPoints=5 n_scans=512", ["MODE_OFF"], ["MODE_2"]),
    # 128 lasers, curbPoints 4, 129 tiles in the default mode: the mode and three switches
    ("front_mode=1 channels=128 curbPoints=4 n_scans=512 tiles=129", ["LASERS", "CURB_POINTS", "TILES", "FEW_SCANS"],
     ["MODE_3", "LASERS128", "LONG_SWEEPS", "CURB_POINTS"]),
    ("front_mode=2 channels=64 curbPoints=8 n_scans=16", ["CURB_POINTS"], ["MODE_3"]),
    # the callback path in firing order: a batch call; once row-major sweeps have been sighted, 16 lasers lack only the mode
    ("front_mode=1 channels=64 curbPoints=5 slot=1", ["CALLBACK"], ["BATCH"]),
    ("front_mode=1 channels=16 curbPoints=5 slot=1", ["CALLBACK"], ["BATCH", "MODE_2"]),
    ("front_mode=1 channels=16 curbPoints=5 slot=1 rows_state=2", ["CALLBACK"], ["MODE_2"]),
    ("front_mode=1 channels=64 curbPoints=5 slot=1 rows_state=2", [], []),
    # after a read-out, with and without urf_set_front_outputs; a whole batch handed back in mode 1; stage capture
    ("front_mode=2 channels=64 curbPoints=5 want_ring_sorted=1", ["READOUT"], ["RESET", "FRONT_OUTPUTS"]),
    ("front_mode=2 channels=64 curbPoints=5 want_ring_sorted=1 front_outputs=1", ["READOUT"], ["RESET"]),
    ("front_mode=2 channels=64 curbPoints=5 general_only=1 front_outputs=1", ["READOUT"], ["RESET"]),
    ("front_mode=1 channels=64 curbPoints=5 n_scans=512 front_off=1", ["STOPPED"], ["RESET"]),
    ("front_mode=2 channels=64 curbPoints=5 capture=1", ["CAPTURE"], ["CAPTURE_OFF"]),
    # nothing helps, and what else was missing is still named
    ("front_mode=2 channels=64 curbPoints=9 want_ring_sorted=1 capture=1", ["READOUT", "CAPTURE", "CURB_POINTS"],
     ["NEVER", "CAPTURE_OFF", "RESET", "FRONT_OUTPUTS"]),
    ("front_mode=2 channels=8 curbPoints=5", ["LASERS"], ["NEVER"]),
    ("front_mode=1 channels=64 curbPoints=5 n_scans=512 tiles=257", ["TILES"], ["NEVER"]),
    ("front_mode=1 channels=64 curbPoints=5 n_scans=512 tiles=256", ["TILES"], ["MODE_2", "LONG_SWEEPS"]),
]


@pytest.mark.parametrize("inputs,why,advice", ROWS, ids=[r[0].replace(" ", ",") for r in ROWS])
def test_named_rows(program, inputs, why, advice):
    front, w, a = (int(x) for x in subprocess.run([program] + inputs.split(), capture_output=True, text=True, check=True).stdout.split())
    assert (w, a) == (bits(WHY, *why), bits(ADVICE, *advice)), (front, hex(w), hex(a))
    assert front == (0 if why else 1)
