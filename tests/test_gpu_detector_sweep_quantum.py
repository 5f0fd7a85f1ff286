"""urf::Detector::setSweepQuantum from C++ (tests/cpp/detector_sweep_quantum_demo.cpp, g++ against the product library): three dense
messages of different lengths through two detectors -- filtered() with the switch off, submit / collect at quantum 2048.  The four
clouds of every message are equal byte for byte; how many road and curb points that is comes from oracle B."""
import re
import struct
import subprocess

import numpy as np
import pytest

import sweep_quantum_cases as Q
from test_gpu_detector import build_demo


@pytest.mark.gpu
def test_submit_collect_with_the_quantum_equals_filtered_without(tmp_path):
    exe = build_demo(tmp_path, "detector_sweep_quantum_demo")
    named, files = Q.stream()[:3], []
    p = Q.params32()
    assert len({len(c[0]) for _, c in named}) == 3
    for k, (_, (x, y, z)) in enumerate(named):
        path = str(tmp_path / ("sweep%d.bin" % k))
        with open(path, "wb") as f:
            f.write(struct.pack("<I", len(x)))
            for a in (x, y, z):
                f.write(np.ascontiguousarray(a, np.float32).tobytes())
        files.append(path)
    refs = [Q.ref(key, c, p) for key, c in named]
    r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, (r.stdout, r.stderr)
    m = re.match(r"messages (\d+) equal (\d+) road (\d+) curb (\d+)", r.stdout)
    assert m, r.stdout
    got = tuple(map(int, m.groups()))
    assert got == (3, 3, sum(x[1]["n_road"] for x in refs), sum(x[1]["n_curb"] for x in refs)), got
