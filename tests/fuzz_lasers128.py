"""tests/fuzz_lasers.py's idea for 128 lasers per firing (k_front128*, urf_front.hpp: two lasers per lane, a tile = 16 firings, a presence word = 32):
a synthetic sweep of 128 rings in firing order, 96 .. 300 firings, with random drop-outs -- single points, whole firings, firings
whose lasers 0..63 or 64..127 are all missing, whole rings, azimuth ranges, runs inside a ring, holes that straddle the borders of
tiles (every 16 firings) and of the march's blocks (every 32) -- a few points moved off their ring or their sector, a scan that ends
inside a firing, a random region of interest and random detector parameters.  params.channels = 128 and an interval of 0.05 (0.03)
degrees, so that neighbouring lasers keep rings of their own.  GPU against oracle B (tests/test_gpu_front_lasers128.py).
Holes here are (0, 0, 0) only; other encodings: sensor_models.py."""
import numpy as np

import urban_road_filter_amd as u

L = 128


def case(seed):
    rng = np.random.default_rng(seed)
    cols = int(rng.integers(96, 301))
    scene = int(rng.choice([1, 2, 3, 4]))
    x, y, z = u.synth_cloud(L, cols, scene, int(rng.integers(1, 1 << 30)))
    n = L * cols
    drop = np.zeros(n, bool)
    ring = np.arange(n) % L
    col = np.arange(n) // L
    kinds = rng.integers(0, 2, 9)
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
            drop |= (ring == r) & (((col - c0) % cols) < int(rng.integers(1, 60)))
    # firings without their lasers 0..63 / without their lasers 64..127: in every case (what a wrong cross-half slot rank would trip over)
    drop |= np.isin(col, rng.integers(0, cols, int(rng.integers(1, 6)))) & (ring < 64)
    drop |= np.isin(col, rng.integers(0, cols, int(rng.integers(1, 6)))) & (ring >= 64)
    if kinds[5]:                                                                            # holes across tile and block borders
        for border in rng.choice(np.arange(16, cols, 16), int(rng.integers(1, 5))):
            w0, w1 = int(rng.integers(0, 7)), int(rng.integers(1, 7))
            lasers = rng.random(L) < float(rng.choice([0.1, 0.5, 1.0]))
            drop |= (col >= border - w0) & (col < border + w1) & lasers[ring]
    x[drop] = y[drop] = z[drop] = 0.0
    if kinds[6]:                                                                            # a few points off their ring / sector
        k = rng.integers(0, n, int(rng.integers(1, 20)))
        z[k] = (z[k] * rng.uniform(0.3, 1.7, len(k))).astype(np.float32)
        k = rng.integers(0, n, int(rng.integers(1, 20)))
        x[k], y[k] = y[k].copy(), x[k].copy()
    if kinds[7]:                                                                            # the scan ends inside a firing
        n = L * (cols - 1) + int(rng.integers(1, L))
        x, y, z = x[:n].copy(), y[:n].copy(), z[:n].copy()
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
    p.interval = float(rng.choice([0.05, 0.05, 0.03]))
    return (x, y, z), p
