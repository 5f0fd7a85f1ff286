"""The id rule of urf_classify_batch_*_dense_elev (include/urf.h) in numpy (TEST CODE).

The caller's table holds the elevation in degrees of the laser in every slot of a firing.  Host: the slots ranked by ascending elevation,
the lower slot first among equals; T[k] = float32(tan((e_k + e_{k+1}) / 2 * pi / 180)) in double for the ranked e.  Per point: h =
float32 sqrt(x * x + y * y), rank = the number of k with z > T[k] * h (a float32 product), id = slot_of_rank[rank].  The model COUNTS; the
kernel searches, which is the same thing as long as T[k] * h does not decrease with k (monotone_products)."""
import math

import numpy as np


def table(elev):
    """(T float32[n - 1], slot_of_rank uint8[n]) of a table of elevations (float32, as the C ABI takes them)."""
    e = np.asarray(elev, np.float32).astype(np.float64)
    order = np.argsort(e, kind="stable")
    r = e[order]
    # (math.tan: the C library's, as the host code calls it; numpy's vectorised tangent may differ from it in the last place)
    T = np.asarray([math.tan(v) for v in (r[:-1] + r[1:]) / 2 * math.pi / 180], np.float64).astype(np.float32)
    return T, order.astype(np.uint8)


def products(T, x, y):
    """T[k] * h per point and threshold, float32 [n_points, n - 1]; h as the kernel computes it."""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    with np.errstate(all="ignore"):
        h = np.sqrt(x * x + y * y, dtype=np.float32)
        return T[None, :] * h[:, None]


def ranks(elev, cloud):
    T, _ = table(elev)
    z = np.asarray(cloud[2], np.float32)
    with np.errstate(all="ignore"):
        return (z[:, None] > products(T, cloud[0], cloud[1])).sum(axis=1)


def ids(elev, cloud):
    """The derived id (a firing slot) of every point of cloud = (x, y, z)."""
    return table(elev)[1][ranks(elev, cloud)].astype(np.int64)


def monotone_products(elev, cloud):
    """T[k] * h never decreases with k wherever both neighbours are numbers: what lets the kernel search instead of count."""
    p = products(table(elev)[0], cloud[0], cloud[1])
    with np.errstate(all="ignore"):
        return not (p[:, 1:] < p[:, :-1]).any()


def midpoint_margin_deg(elev, cloud):
    """The smallest distance [deg] of a point's elevation from a midpoint between two ranked elevations (inf: one laser)."""
    e = np.sort(np.asarray(elev, np.float32).astype(np.float64))
    mid = (e[:-1] + e[1:]) / 2
    if len(mid) == 0:
        return np.inf
    x, y, z = (np.asarray(a, np.float64) for a in cloud)
    ang = np.degrees(np.arctan2(z, np.sqrt(x * x + y * y)))
    return float(np.abs(ang[:, None] - mid[None, :]).min()) if len(ang) else np.inf
