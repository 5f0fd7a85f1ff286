"""What of a sweep the fused front end's march decides on, computed on the CPU from oracle B's stages (TEST CODE): shared by
tests/test_front_multi_cpu.py and tests/test_gpu_front_multi.py.

fusable(cloud, params, layout): the rules of k_front that urf_set_front_multi_sector leaves in force -- one laser slot, one ring; one
ring, one laser slot; no ring point on the sensor's axis (its azimuth is NaN); the planar ranges of the star-shaped search's
participants inside [2^-45, 2^63] (urf_sqrt_rn_normal's interval).  multi_sector_firings and tiles_where_sectors_fall count what the
switch is for: firings whose participants lie in more than one sector, tiles of 2048 points in which a sector is followed by a smaller
one.

One rule of the march depends on the CONTEXT and is kept apart: a full candidate list hands the scan back.  front_candidates counts the
entries a scan files, as urf_front_body files them; fits(cloud, params, max_points, n_scans) compares them with the list of a context
of max_points (tests/test_front_crossings_cpu.py pins it for the long sweeps, whose halos' holes fill the list)."""
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


# ---- the candidate list (urf_front.hpp: urf_front_push / urf_front_flush; "a list that overflows hands its scan back") ----
HPRE, HPRE_WIDE, HPOST = 8, 12, 8   # URF_FRONT_HPRE, URF_FRONT_HPRE_WIDE, URF_FRONT_HPOST: firings in front of and behind a block of the march


def tiles_per_block(n_scans, L):
    """urf_policy::tiles_per_block without URF_FRONT_TPB."""
    tpb = 4 if n_scans >= 512 else (2 if n_scans >= 16 else 1)
    return tpb if L != 128 else max(2, tpb & ~1)


def candidate_cap(max_points, L, lasers128=True):
    """front_cand_cap of a context (urf_api.hip; URF_FRONT128_CAND_CAP once urf_set_front_lasers128 has been on)."""
    return max(max_points // 8, 16384) if (L == 128 and lasers128) else max(max_points // 8, 4096)


def front_candidates(cloud, params, n_scans, layout="firing"):
    """The entries the march of k_front files in a scan's candidate list, counted as the kernel counts them (urf_front_body).  Per laser
    the window holds its last 2 CP + 1 ring points' heights; a block of tiles_per_block tiles starts HPRE firings early with an EMPTY
    window and ends HPOST firings late.  With its k-th ring point since the block's first firing a laser files: one entry for z_zero when
    the centre (CP back) is the block's and the window is full and passes z_zero's height test (urf_front_window::hz) -- or is NOT full
    and the block is not the scan's first (an EDGE item: k_front_finish decides) --, one for x_zero likewise (the point CP - CP / 2 back,
    hx); and behind a block that is not the scan's last, one per point among the CP newest that is the block's.  Holes in the halo in
    front of a block -- a sweep with many drop-outs -- make EDGE items: a few per laser and block."""
    L, CP = int(params.channels), int(params.curbPoints)
    H, NW = CP // 2, 2 * CP + 1
    hpre = HPRE if CP <= 5 else HPRE_WIDE
    use_z, use_x = bool(params.z_zero_method), bool(params.x_zero_method)
    curb_h = np.float32(params.curbHeight)
    _, ib, st = stages(cloud, params)
    if ib["status"] != 0 or not (use_z or use_x):
        return 0
    n = len(cloud[0])
    nf = -(-n // L)
    idx = np.arange(n)
    firing_of, lane_of = (idx // L, idx % L) if layout == "firing" else (idx % (n // L), idx // (n // L))
    on = st["ring"] >= 0
    steps = TILE // L * tiles_per_block(n_scans, L)
    F0 = np.arange(0, nf, steps)
    F1 = np.minimum(F0 + steps, nf)
    Fs = np.where(F0 > hpre, F0 - hpre, 0)
    Fe = np.minimum(F1 + HPOST, nf)
    first, last = Fs == 0, Fe == nf
    total = 0
    z_all = cloud[2]
    for lane in range(L):
        sel = on & (lane_of == lane)
        f = firing_of[sel]
        order = np.argsort(f, kind="stable")
        f, z = f[order], z_all[sel][order].astype(np.float32)
        m = len(f)
        if m == 0:
            continue
        a = np.abs(z)
        hz = np.zeros(m + 1, np.int64)   # prefix sums over the CENTRE's index
        hx = np.zeros(m + 1, np.int64)   # ... over the NEWEST point's index
        if m >= NW:
            win = np.lib.stride_tricks.sliding_window_view(a, NW)          # window j: points j .. j + 2 CP, centre j + CP
            a5 = win[:, CP]
            m1, m2 = win[:, :CP + 1].max(axis=1), win[:, CP:].max(axis=1)
            pz = (((m1 - a5) >= curb_h) | ((m2 - a5) >= curb_h)) & (np.abs(m1 - m2) >= np.float32(0.05))
            hz[CP + 1:m - CP + 1] = np.cumsum(pz)
            hz[m - CP + 1:] = hz[m - CP]
            wz = np.lib.stride_tricks.sliding_window_view(z, NW)
            c, mid, new = wz[:, CP], wz[:, CP + H], wz[:, 2 * CP]
            px = ((np.abs(c - mid) >= curb_h) | (np.abs(new - mid) >= curb_h)) & (np.abs(c - new) >= np.float32(0.05))
            hx[2 * CP + 1:] = np.cumsum(px)
        i_s, i0, i1, ie = (np.searchsorted(f, v) for v in (Fs, F0, F1, Fe))
        n_pre, nb, tot = i0 - i_s, i1 - i0, ie - i0
        full_from = np.maximum(NW - n_pre, 1)   # the first k at which the window is full
        for use, back, pre in ((use_z, CP, hz), (use_x, CP - H, hx)):
            if not use:
                continue
            lo, hi = back + 1, np.minimum(nb + back, tot)   # k of the entries: the point `back` behind the newest is the block's
            edge = np.clip(np.minimum(hi, full_from - 1) - lo + 1, 0, None)
            total += int(edge[~first].sum())
            k0 = np.maximum(lo, full_from)
            some = hi >= k0
            # k-th point since F0 is lane point i0 + k - 1; hz is indexed by the centre (CP back), hx by the newest
            shift = CP if pre is hz else 0
            a_lo, a_hi = i0 + k0 - 1 - shift, i0 + hi - 1 - shift
            total += int((pre[np.clip(a_hi + 1, 0, m)] - pre[np.clip(a_lo, 0, m)])[some].sum())
        for b in range(CP):
            if use_z or (use_x and b < CP - H):
                total += int(((tot > b) & (tot - b <= nb) & ~last).sum())
    return total


def fits(cloud, params, max_points, n_scans, layout="firing"):
    """The candidate list of a context of max_points holds the scan's entries (more: the scan is handed back, urf_front_flush)."""
    return front_candidates(cloud, params, n_scans, layout) <= candidate_cap(max_points, int(params.channels))
