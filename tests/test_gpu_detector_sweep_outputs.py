"""urf::Detector::setSweepOutputs from C++ (tests/cpp/detector_sweep_outputs_demo.cpp, g++ against the product library): eight 64 x 256
sweeps through two detectors with road_marker and the reference order on -- one filtered() per sweep with the switch off, submit x 4 /
collect with it on.  The four clouds and the MarkerArrays, DELETE ghosts included, are equal byte for byte; how many arrays, ghosts and
road points that is comes from oracle B and the host's strip builder."""
import re
import struct
import subprocess

import numpy as np
import pytest

import oracles as O
import urban_road_filter_amd as u
from test_gpu_detector import build_demo


def sweeps():
    """Scenes 1 and 3 (a street with curbs; the same with range noise and drop-outs), two of them cut short in azimuth: fewer marker
    points than the sweep before, so that the marker builder has ghosts to delete."""
    out = []
    for k, (scene, seed) in enumerate([(1, 21), (3, 22), (1, 23), (3, 24), (3, 25), (1, 26), (3, 27), (1, 28)]):
        x, y, z = u.synth_cloud(64, 256, scene, seed)
        if k in (2, 5):
            x[64 * 96:], y[64 * 96:], z[64 * 96:] = 1.0e6, 1.0e6, 0.0   # outside the region of interest
        out.append((x, y, z))
    return out


def expected(clouds):
    """(MarkerArrays published, DELETE markers, road points) of the sequence: oracle B's marker points through urf_marker_strips."""
    p, mp = u.default_params().wide_roi(), u.default_marker_params()
    ghost = published = deletes = road = 0
    for c in clouds:
        _, ib, st = O.run_b(*c, p, debug=True)
        if ib["status"] != 0:
            continue
        road += len(st["road_order"])
        pub, strips, _, ghost = u.marker_strips(st["marker_pts"], mp, ghost)
        published += int(pub)
        deletes += int((strips["action"] == u.MARKER_DELETE).sum()) if pub else 0
    return published, deletes, road


def test_the_sequence_has_ghosts_to_delete():
    published, deletes, road = expected(sweeps())
    assert published == 8 and deletes > 0 and road > 8000


@pytest.mark.gpu
def test_submit_collect_with_the_switch_equals_filtered_without(tmp_path):
    exe = build_demo(tmp_path, "detector_sweep_outputs_demo")
    clouds, files = sweeps(), []
    for k, (x, y, z) in enumerate(clouds):
        path = str(tmp_path / ("sweep%d.bin" % k))
        with open(path, "wb") as f:
            f.write(struct.pack("<I", len(x)))
            for a in (x, y, z):
                f.write(np.ascontiguousarray(a, np.float32).tobytes())
        files.append(path)
    r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, (r.stdout, r.stderr)
    m = re.match(r"sweeps (\d+) equal (\d+) published (\d+) deletes (\d+) road (\d+)", r.stdout)
    assert m, r.stdout
    got = tuple(map(int, m.groups()))
    assert got[:2] == (8, 8) and got[2:] == expected(clouds), (got, expected(clouds))
