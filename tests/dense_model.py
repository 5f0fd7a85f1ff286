"""The re-alignment rule of urf_classify_batch_*_dense (include/urf.h) in numpy (TEST CODE).

A dense scan (non-returns dropped by the driver) has points i = 0..n-1 with slot s_i (the laser id through an optional slot map).  A
firing starts at i = 0 and wherever s_i <= s_{i-1}; f_i = starts up to and including i, minus 1; point i goes to f_i * L + s_i of a
padded scan of W * L points that is NaN everywhere else.  A scan with a slot >= L (or an id the map does not hold) or with more than W
firings is "not aligned": point i stays at position i."""
import numpy as np

BAD = 0xFFFF


def slots_of(ids, L, slot_map=None):
    """The slots of the ids (BAD where there is none: id beyond the map, slot >= L)."""
    ids = np.asarray(ids).astype(np.int64)
    if slot_map is None:
        s = ids.copy()
    else:
        table = np.full(65536, BAD, np.int64)
        table[:len(slot_map)] = np.asarray(slot_map).astype(np.int64)
        s = table[ids]
    return np.where((s >= 0) & (s < L), s, BAD)


def realign(ids, L, W, slot_map=None):
    """-> (positions int64[n], firing count, aligned)."""
    s = slots_of(ids, L, slot_map)
    n = len(s)
    if n == 0:
        return np.zeros(0, np.int64), 0, True
    start = np.ones(n, bool)
    start[1:] = s[1:] <= s[:-1]
    f = np.cumsum(start) - 1
    firings = int(f[-1]) + 1
    aligned = bool((s != BAD).all()) and firings <= W
    if not aligned:
        return np.arange(n, dtype=np.int64), firings, False
    pos = f * L + s
    assert n == 1 or (np.diff(pos) > 0).all()   # the property everything rests on
    assert pos[-1] < W * L
    return pos, firings, True


def pad(cloud, pos, L, W):
    """The padded twin of a dense scan: W * L points, NaN where no point landed."""
    out = []
    for a in cloud:
        p = np.full(W * L, np.nan, np.float32)
        p[pos] = a
        out.append(p)
    return tuple(out)


def densify(cloud, L, missing):
    """Drops `missing` points of an organised firing-order sweep (point f * L + l): (dense cloud, slot per kept point)."""
    keep = ~missing
    slot = (np.arange(len(cloud[0])) % L)[keep]
    return tuple(np.ascontiguousarray(a[keep]) for a in cloud), slot
