#!/usr/bin/env python3
"""Generates tests/golden/lasers/*.npz from ORACLE A (the reference's own sources, oracle/Makefile) for sweeps of 32 and 16 lasers,
params.channels = the laser count: the same keys as make_golden.py's files (labels, info_*, cloud_sha, params).  The clouds are
regenerated bit-identically by urf_synth_cloud.  In a directory of its own: tests/test_oracle.py counts the files next to make_golden.py.

    python tests/golden/make_golden_lasers.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracles as O  # noqa: E402
from golden.make_golden import cloud_sha  # noqa: E402

OUT = os.path.join(HERE, "lasers")
# (name, lasers, columns, scene of urf_synth_cloud, seed)
CASES = [
    ("lasers32_s1", 32, 2048, 1, 1),
    ("lasers32_sensor_s3", 32, 2048, 3, 3),
    ("lasers16_sensor_s3", 16, 2048, 3, 3),
]


def case_params(lasers):
    import urban_road_filter_amd as u
    p = u.default_params().wide_roi()
    p.channels = lasers
    return p


def case_cloud(lasers, cols, scene, seed):
    import urban_road_filter_amd as u
    return u.synth_cloud(lasers, cols, scene, seed)


def main():
    os.makedirs(OUT, exist_ok=True)
    for name, lasers, cols, scene, seed in CASES:
        p = case_params(lasers)
        x, y, z = case_cloud(lasers, cols, scene, seed)
        labels, infos, _, _ = O.run_a([(x, y, z)], p)
        info = infos[0]
        out = os.path.join(OUT, name + ".npz")
        np.savez_compressed(out, labels=labels[0], cloud_sha=cloud_sha(x, y, z), params=np.frombuffer(bytes(p), np.uint8),
                            **{"info_" + k: info[k] for k in ("status", "n_roi", "n_road", "n_curb", "n_ring10")})
        print("%-20s n=%d road=%d curb=%d roi=%d (%d bytes)" % (name, len(x), info["n_road"], info["n_curb"], info["n_roi"], os.path.getsize(out)))


if __name__ == "__main__":
    main()
