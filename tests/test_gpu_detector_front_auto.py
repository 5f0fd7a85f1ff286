"""urf::BatchDetector::setFrontMode(2) / setFrontAuto(true) (csrc/detector.hpp) on a sensor model's batch: tests/cpp/detector_front_auto_demo.cpp
runs filtered() six times and compares every published cloud and summary, byte for byte, with a detector whose switches are set by hand to
what frontAuto().applied reports; the first detector must have settled, with urf_set_front_multi_sector applied (an HDL-64E's lasers carry
azimuth offsets)."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import urban_road_filter_amd as u
from test_front_why_cpu import model_scans
from test_gpu_detector import build_demo

pytestmark = pytest.mark.gpu


def test_the_batch_adapter_settles_and_publishes_what_hand_set_switches_publish(tmp_path):
    exe = build_demo(tmp_path, "detector_front_auto_demo")
    scans = model_scans("hdl64e")
    path = str(tmp_path / "clouds.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<II", len(scans), 64))
        for x, y, z in scans:
            f.write(struct.pack("<I", len(x)))
            for a in (x, y, z):
                f.write(np.ascontiguousarray(a, np.float32).tobytes())
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, (r.stdout, r.stderr)
    m = re.search(r"messages (\d+) calls 6 equal (\d+) phase (\d+) applied (0x[0-9a-f]+|0) explained (\d+)", r.stdout)
    assert m, r.stdout
    k, equal, phase, applied, explained = int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4), 16), int(m.group(5))
    assert k == len(scans) and equal == 6 * k and phase == u.AUTO_PHASE["SETTLED"]
    assert applied == u.ADVICE["MULTI_SECTOR"] and 1 <= explained <= 5
