"""urf_set_front_auto's host policy on the CPU (csrc/urf_policy.hpp, no HIP): urf_policy::auto_call and urf_policy::auto_digest.

tests/cpp/policy_auto.cpp walks policy_why.cpp's cross product of settings and calls (less three inputs that neither why() nor a.front
reads) and checks on every row: plan() reads no auto field; nothing is applied with the switch off or in front modes 0 and 1; in modes 2
and 3 the applied bits lie inside URF_ADVICE_AUTO_MASK, applying them is a fixed point in one step, and the call is fused exactly where
the advice held nothing outside the mask; a refused bit is not asked for again.  Then auto_digest over a hand-written table of digests:
MULTI_SECTOR (and _CP off curbPoints 5) once, clean and all-never digests settle, OTHER is taken three times."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("policy") / "policy_auto")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "urban_road_filter_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "policy_auto.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_every_row_of_the_cross_product_and_the_digest_table(program):
    r = subprocess.run([program], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    rows, applied, fused, failures = (int(x) for x in re.fullmatch(r"rows (\d+) applied (\d+) fused (\d+) failures (\d+)\n", r.stdout).groups())
    # policy_why.cpp's product without front_direct (2), front_tpb (3) and front_outputs (2), with multi_sector_cp (2)
    assert rows == 129024000 * 2 // 6 and failures == 0
    assert 0 < applied < fused < rows // 2   # (modes 2 and 3 are half the rows; some calls nothing fuses)


def test_the_mask_is_the_mode_and_the_five_switches():
    header = open(os.path.join(ROOT, "include", "urf.h")).read()
    mask = re.search(r"#define\s+URF_ADVICE_AUTO_MASK\s+\(([^)]*)\)", header.replace("\\\n", " ")).group(1)
    assert sorted(re.findall(r"URF_ADVICE_(\w+)", mask)) == sorted(["MODE_3", "LASERS128", "LONG_SWEEPS", "CURB_POINTS", "MULTI_SECTOR", "MULTI_SECTOR_CP"])
    assert [int(re.search(r"#define\s+URF_AUTO_%s\s+(\d)u" % n, header).group(1)) for n in ("IDLE", "LEARNING", "SETTLED")] == [0, 1, 2]
