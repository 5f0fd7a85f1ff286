#!/usr/bin/env python3
"""Records ORACLE A's outputs (the reference's own unmodified sources, built by oracle/Makefile) for every input
the differential tests hand it, into tests/golden/oracle_a/records_*.npz: key = sha256 of the exact input bytes
(tests/oracles.py: _record_key), value = the binary's output file, xz-compressed.  Where the binary is absent,
tests/oracles.py run_a replays these, so the tests compare oracle B with the reference on every machine.

Run where the reference is mounted (oracle A builds):   python tests/golden/make_oracle_a_records.py"""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
TESTS = ["tests/test_fuzz_cpu.py", "tests/test_markers.py", "tests/test_oracle.py", "tests/test_param_edges_cpu.py",
         "tests/test_sensor_models_cpu.py"]

if __name__ == "__main__":
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "urf_ref")):
        sys.exit("oracle A is not built (the reference's sources are not mounted): nothing to record")
    shutil.rmtree(os.path.join(HERE, "oracle_a"), ignore_errors=True)
    env = dict(os.environ, URF_RECORD_ORACLE_A="1")
    sys.exit(subprocess.call([sys.executable, "-m", "pytest", "-q", "-m", "not gpu", "-p", "no:cacheprovider"] + TESTS,
                             cwd=ROOT, env=env))
