"""urf_set_front_multi_sector_curb_points in the launch policy, on the CPU: tests/cpp/policy_ms_cp.cpp walks urf_policy::plan and
urf_front_family_of (csrc/urf_policy.hpp, no HIP) over front mode x channels x curbPoints 1..9 x star-shaped search x the switches x slot /
batch x batch size, and checks row by row that with urf_policy::multi_sector_cp false front_ms follows the rule from before the switch, that
nothing but front_ms differs between false and true, that with it true front_ms == front && multi_sector && star && 1 <= curbPoints <= 8,
and that the family's ms and cp follow.  (tests/test_policy_table.py: the recorded decisions, the field at its default.)"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_switch_changes_front_ms_and_nothing_else(tmp_path):
    exe = str(tmp_path / "policy_ms_cp")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "urban_road_filter_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "policy_ms_cp.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    words = r.stdout.split()
    got = dict(zip(words[0::2], (int(w) for w in words[1::2])))
    assert got["rows"] == 4 * 4 * 9 * 2 ** 7
    # (a walk that never meets a fused call, or a multi-sector one, would pass everything above)
    assert 0 < got["ms_off"] < got["ms_on"] < got["fused"] < got["rows"]
