"""tests/fuzz_organised.py's idea for sensors with fewer lasers: a synthetic sweep of L = 16 or 32 rings in firing order
(urf_synth_cloud, tie-free or sensor-like) with random drop-outs (single points, whole firings, whole rings, azimuth ranges, runs
inside a ring), points moved off their ring or their sector, a random region of interest and random detector parameters;
params.channels = L, as a user of such a sensor sets it.  GPU against oracle B (tests/test_gpu_front_lasers.py).
Holes here are (0, 0, 0) only; other encodings: sensor_models.py."""
import numpy as np

import urban_road_filter_amd as u


def case(seed, L):
    rng = np.random.default_rng(seed)
    cols = int(rng.choice([256, 512, 1024, 2048]))
    scene = int(rng.choice([1, 2, 3, 4]))
    x, y, z = u.synth_cloud(L, cols, scene, int(rng.integers(1, 1 << 30)))
    n = L * cols
    drop = np.zeros(n, bool)
    ring = np.arange(n) % L
    col = np.arange(n) // L
    kinds = rng.integers(0, 2, 7)
    if kinds[0]:
        drop |= rng.random(n) < float(rng.choice([0.002, 0.02, 0.2]))                       # single points
    if kinds[1]:
        drop |= np.isin(col, rng.integers(0, cols, int(rng.integers(1, 12))))               # whole firings
    if kinds[2]:
        drop |= np.isin(ring, rng.integers(0, L, int(rng.integers(1, 4))))                  # whole rings
    if kinds[3]:
        a0 = int(rng.integers(0, cols))
        drop |= ((col - a0) % cols) < int(rng.integers(1, cols // 3))                       # an azimuth range
    if kinds[4]:
        for _ in range(int(rng.integers(1, 8))):                                            # a run inside one ring
            r, c0 = int(rng.integers(0, L)), int(rng.integers(0, cols))
            drop |= (ring == r) & (((col - c0) % cols) < int(rng.integers(1, 200)))
    x[drop] = y[drop] = z[drop] = 0.0
    if kinds[5]:                                                                            # a few points off their ring / sector
        k = rng.integers(0, n, int(rng.integers(1, 20)))
        z[k] = (z[k] * rng.uniform(0.3, 1.7, len(k))).astype(np.float32)
        k = rng.integers(0, n, int(rng.integers(1, 20)))
        x[k], y[k] = y[k].copy(), x[k].copy()
    p = u.default_params()
    if rng.random() < 0.5:
        p = p.wide_roi()
    else:                                                                                   # a wedge / box that cuts rings and firings
        p.min_X, p.max_X = float(rng.choice([-200.0, 0.0, 3.0])), float(rng.choice([15.0, 30.0, 200.0]))
        p.min_Y, p.max_Y = float(rng.choice([-200.0, -10.0, -3.0])), float(rng.choice([2.0, 10.0, 200.0]))
    p.channels = L
    p.x_zero_method = int(rng.random() < 0.9)
    p.z_zero_method = int(rng.random() < 0.9)
    p.star_shaped_method = int(rng.random() < 0.85)
    p.blind_spots = int(rng.random() < 0.7)
    p.xDirection = int(rng.integers(0, 3))
    p.curbHeight = float(rng.choice([0.02, 0.05, 0.1]))
    p.curbPoints = int(rng.choice([5, 5, 5, 2, 9]))
    p.angleFilter1 = float(rng.choice([120.0, 150.0, 175.0]))
    p.angleFilter2 = float(rng.choice([100.0, 140.0, 170.0]))
    p.angleFilter3 = float(rng.choice([20.0, 30.0, 50.0]))
    p.starbeam_filter = int(rng.random() < 0.2)
    p.interval = float(rng.choice([0.18, 0.18, 0.1]))
    return (x, y, z), p
