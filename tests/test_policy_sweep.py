"""The callback path's host decisions on the CPU (csrc/urf_policy.hpp, no HIP): urf_sweep_shape and urf_seq_cache.

tests/cpp/policy_sweep.cpp checks the shape a sweep runs as under urf_set_sweep_quantum -- quantum 0; k q - 1, k q and k q + 1 points; a
padded length of exactly max_points and one tile beyond it; point_step 12, 16 and 32 staged as planes and as records; a buffer that fits
and one that does not (room for twice the padded length) -- and a slot's sequence cache: one entry or URF_SWEEP_SEQS, least recently
used, epoch changes, the resident count urf_callback_path_captures reports.  Here: the program's verdict, and its padded lengths against
tests/sweep_quantum_cases.padded_len, the rule the GPU tests of urf_set_sweep_quantum pad their reference inputs by."""
import os
import re
import subprocess

import pytest

import sweep_quantum_cases as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("policy") / "policy_sweep")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "urban_road_filter_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "policy_sweep.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_every_shape_and_every_walk_of_the_sequence_cache(program):
    r = subprocess.run([program], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    checks, failures = (int(x) for x in re.fullmatch(r"checks (\d+) failures (\d+)\n", r.stdout).groups())
    assert checks >= 60 and failures == 0


@pytest.mark.parametrize("quantum,max_points", [(2048, 16384), (4096, 16384), (2048, 15000)])
def test_the_padded_length_is_the_reference_inputs_padded_length(program, quantum, max_points):
    """Every length from 1 to max_points: n_run is padded_len(n) where that fits the context, else the sweep's own length, unpadded."""
    r = subprocess.run([program, "lengths", str(quantum), str(max_points), "1", str(max_points + 1)], capture_output=True, text=True)
    assert r.returncode == 0
    rows = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]
    assert [n for n, _, _ in rows] == list(range(1, max_points + 1))
    for n, n_run, pad in rows:
        up = Q.padded_len(n, quantum)
        assert (n_run, pad) == ((up, 1) if up <= max_points else (n, 0)), (n, n_run, pad)
    assert any(pad == 0 for _, _, pad in rows) == (max_points % quantum != 0)
