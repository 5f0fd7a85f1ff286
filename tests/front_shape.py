"""What of a sweep the fused front end's march decides on, computed on the CPU from oracle B's stages (TEST CODE): shared by
tests/test_front_multi_cpu.py and tests/test_gpu_front_multi.py.

fusable(cloud, params, layout): the rules of k_front that urf_set_front_multi_sector leaves in force -- one laser slot, one ring; one
ring, one laser slot; no ring point on the sensor's axis (its azimuth is NaN); the planar ranges of the star-shaped search's
participants inside [2^-45, 2^63] (urf_sqrt_rn_normal's interval).  multi_sector_firings and tiles_where_sectors_fall count what the
switch is for: firings whose participants lie in more than one sector, tiles of 2048 points in which a sector is followed by a smaller
one."""
import numpy as np

import oracles as O

TILE = 2048
_STAGES = {}


def stages(cloud, params):
    """oracle B's per-point stages of a sweep, computed once per (sweep, parameters) and read only."""
    key = (id(cloud[0]), len(cloud[0]), bytes(params))
    if key not in _STAGES:
        lb, ib, st = O.run_b(*cloud, params, debug=True)
        _STAGES[key] = (cloud, lb, ib, st)   # (the sweep is kept alive: its id stays its own)
    return _STAGES[key][1:]


def firing_order(a, L, layout):
    """(firings, L) view of a per-point array of a whole number of firings."""
    a = np.asarray(a)
    assert len(a) % L == 0
    return a.reshape(L, -1).T if layout == "rows" else a.reshape(-1, L)


def fusable(cloud, params, layout="firing"):
    L = int(params.channels)
    n = len(cloud[0]) // L * L   # (a scan that ends inside a firing: the whole firings decide; the rest is checked below)
    _, ib, st = stages(cloud, params)
    if ib["status"] != 0:
        return True   # (fewer than 30 points in the region of interest: nothing to hand back)
    ring_all, sec_all = st["ring"], st["sector"]
    x, y = cloud[0], cloud[1]
    on = ring_all >= 0
    if ((x == 0) & (y == 0) & on).any():
        return False   # a ring point on the sensor's axis
    lane_all = np.arange(len(ring_all)) % L if layout == "firing" else None
    if layout == "rows":
        if n != len(cloud[0]):
            return False
        lane_all = np.arange(n) // (n // L)
    lane_of_ring, ring_of_lane = {}, {}
    for l, r in set(zip(lane_all[on].tolist(), ring_all[on].tolist())):
        if lane_of_ring.setdefault(r, l) != l or ring_of_lane.setdefault(l, r) != r:
            return False   # a ring fed by two laser slots, a laser slot that meets two rings
    part = sec_all >= 0
    with np.errstate(invalid="ignore", over="ignore"):
        rho2 = x[part].astype(np.float32) ** 2 + y[part].astype(np.float32) ** 2
    if part.any() and not ((rho2 >= np.float32(2.0 ** -90)) & (rho2 <= np.float32(2.0 ** 126))).all():
        return False
    return True


def _sectors(cloud, params, layout):
    L = int(params.channels)
    sec = stages(cloud, params)[2]["sector"]
    n = len(sec) // L * L
    return firing_order(sec[:n], L, layout)


def multi_sector_firings(cloud, params, layout="firing"):
    """(firings whose participants lie in more than one sector, the largest number of sectors in one firing)"""
    s = _sectors(cloud, params, layout)
    counts = np.array([len(set(row[row >= 0].tolist())) for row in s])
    return int((counts > 1).sum()), int(counts.max()) if len(counts) else 0


def tiles_where_sectors_fall(cloud, params, layout="firing"):
    """Tiles (2048 points in firing order) in which a participant's sector is smaller than an earlier participant's."""
    s = _sectors(cloud, params, layout).reshape(-1)
    tiles = 0
    for t0 in range(0, len(s), TILE):
        k = s[t0:t0 + TILE]
        k = k[k >= 0]
        tiles += int(len(k) > 1 and (np.diff(k.astype(np.int32)) < 0).any())
    return tiles
