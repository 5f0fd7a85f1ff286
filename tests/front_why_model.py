"""What urf_front_explain counts in a scan, computed on the CPU from oracle B's stages (TEST CODE): tests/front_shape.py's `fusable` split
into its four counters, with its multi_sector_firings and tiles_where_sectors_fall beside them.  Shared by tests/test_front_why_cpu.py,
which pins the figures, and tests/test_gpu_front_explain.py, which asks the kernel for the same ones.

counters(cloud, params, layout) -> dict with the fields of urf_front_why that k_front_explain fills:
  lanes_two_rings   laser slots whose ring points lie on more than one ring
  rings_two_lanes   rings whose points come from more than one laser slot
  axis_points       ring points with x == y == 0 (their azimuth is NaN)
  range_points      participants of the star-shaped search whose squared planar range (float) lies outside [2^-90, 2^126]
  multi_sector_firings, max_sectors_per_firing, tiles_sectors_fall   front_shape's, over the scan's firings -- a last firing that the scan
                    ends in counts with the points it has
A scan without a result (fewer than 30 points in the region of interest), and a row-major one whose length is not `channels` whole rows:
all zero.  fusable(cloud, ...) == not any of the first four, by construction (test_front_why_cpu.py checks it against front_shape's)."""
import numpy as np

import front_shape as FS

FIELDS = ("lanes_two_rings", "rings_two_lanes", "axis_points", "range_points", "multi_sector_firings", "max_sectors_per_firing", "tiles_sectors_fall")
SHAPE = FIELDS[:4]


def _padded_sectors(sec, L):
    """(firings, L) of a scan in firing order that ends inside a firing: the missing slots take no part"""
    pad = -len(sec) % L
    return np.concatenate([sec, np.full(pad, -1, sec.dtype)]).reshape(-1, L)


def counters(cloud, params, layout="firing"):
    L = int(params.channels)
    n = len(cloud[0])
    out = dict.fromkeys(FIELDS, 0)
    _, ib, st = FS.stages(cloud, params)
    if ib["status"] != 0 or (layout == "rows" and n % L != 0):
        return out
    ring, sec = st["ring"], st["sector"]
    x, y = cloud[0], cloud[1]
    on = ring >= 0
    lane = np.arange(n) % L if layout == "firing" else np.arange(n) // (n // L)
    pairs = set(zip(lane[on].tolist(), ring[on].tolist()))
    out["lanes_two_rings"] = sum(1 for l in {l for l, _ in pairs} if sum(1 for a, _ in pairs if a == l) > 1)
    out["rings_two_lanes"] = sum(1 for r in {r for _, r in pairs} if sum(1 for _, b in pairs if b == r) > 1)
    out["axis_points"] = int(((x == 0) & (y == 0) & on).sum())
    part = sec >= 0
    with np.errstate(invalid="ignore", over="ignore"):
        rho2 = x[part].astype(np.float32) ** 2 + y[part].astype(np.float32) ** 2
    out["range_points"] = int((~((rho2 >= np.float32(2.0 ** -90)) & (rho2 <= np.float32(2.0 ** 126)))).sum())
    if not bool(params.star_shaped_method):
        return out   # (oracle B reports no sectors then: nothing to count)
    if n % L == 0:
        nm, most = FS.multi_sector_firings(cloud, params, layout)
        fall = FS.tiles_where_sectors_fall(cloud, params, layout)
    else:   # front_shape looks at the whole firings only: the same two counts with the last firing's points
        s = _padded_sectors(sec, L)
        per = np.array([len(set(row[row >= 0].tolist())) for row in s])
        nm, most = int((per > 1).sum()), int(per.max())
        flat, fall = s.reshape(-1), 0
        for t0 in range(0, len(flat), FS.TILE):
            k = flat[t0:t0 + FS.TILE]
            k = k[k >= 0]
            fall += int(len(k) > 1 and (np.diff(k.astype(np.int32)) < 0).any())
    out["multi_sector_firings"], out["max_sectors_per_firing"], out["tiles_sectors_fall"] = nm, most, fall
    return out


def fusable(cloud, params, layout="firing"):
    c = counters(cloud, params, layout)
    L = int(params.channels)
    if layout == "rows" and len(cloud[0]) % L != 0 and FS.stages(cloud, params)[1]["status"] == 0:
        return False
    return not any(c[k] for k in SHAPE)
