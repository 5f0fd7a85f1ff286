"""Inputs of tests/test_gpu_front_crossings.py, built on the CPU (TEST CODE): the multi-sector switches crossed with the other paths a
real sensor's sweep takes -- dense entry points, sweeps of more than 128 tiles, 128 lasers, a long-lived context.
tests/test_front_crossings_cpu.py pins the properties the inputs are used for.

Long sweeps: the small models of tests/test_front_multi_cpu.py at 64 x 4128, 128 x 2064 and 16 x 16512 (129 tiles) and 64 x 8192 (256
tiles), started so that the wrap from the last sector to sector 0 falls into the LAST tile, and for one scan of the 256-tile batch into
tile 128 exactly (seam_tiles).  Dense sweeps: real geometries started at 77.7 and 123.4 degrees (the seam inside a tile), non-returns
dropped (dense_model.densify); the padded twin (dense_model.pad of dense_model.realign) is what the device classifies."""
import numpy as np

import dense_model as D
import front_shape as FS
import sensor_models as SM
import urban_road_filter_amd as u
from test_front_multi_cpu import small_models, small_params

_CACHE = {}


def at_k(p, K):
    q = p.copy()
    q.sectors = K
    return q


def rows_of(c, L):
    return tuple(np.ascontiguousarray(a.reshape(-1, L).T.reshape(-1)) for a in c)


# ---- sweeps of more than 128 tiles ----
# name -> (small model, firings, [(firing at which the sweep wraps, world, seed, noise), ...])
LONG = {
    "64 x 4128": ("64 offsets", 4128, [(4112, 0, 41, False), (4100, 1, 42, True)]),          # tile 128 = the last one: firings 4096..4127
    "64 x 8192": ("64 offsets", 8192, [(8176, 2, 43, False), (4112, 2, 44, False)]),         # the last tile (255); tile 128 exactly
    "128 x 2064": ("128 stagger", 2064, [(2056, 0, 45, False), (2050, 1, 46, True)]),        # firings 2048..2063
    "16 x 16512": ("16 drift", 16512, [(16448, 0, 47, False), (16400, 1, 48, True)]),        # firings 16384..16511
}

# Returns dropped from every long sweep (four of five at half a million points, half elsewhere): oracle B's time goes with the points it keeps, the tiles,
# firings and sectors the kernels see stay as they are (a test has to stay below the slowest of tests/test_gpu_front_multi.py).  What
# grows with the holes is the march's candidate list -- a halo with holes in front of a block makes EDGE items, a few per laser and
# block (front_shape.front_candidates): 106 000 and 113 000 entries for the two 64 x 8192 sweeps, where a context of 64 x 8192 points
# holds 65 536.  long_max_points sizes the context for them, as tests/test_gpu_dense.context does for its sweeps; on a context of the
# sweep's own size both are handed back, and that is a test of its own.
LONG_DROP = {"64 x 8192": 0.8, "64 x 4128": 0.5, "128 x 2064": 0.5, "16 x 16512": 0.5}


def long_max_points(name):
    """max_points of the context a long batch runs on: its candidate list (max_points / 8 entries per scan) holds every sweep's."""
    n = len(long_sweeps(name)[0][0])
    return {"64 x 8192": 3 * n, "64 x 4128": 2 * n, "128 x 2064": 2 * n}.get(name, max(64 * 2048, n))


def long_model(name):
    small, F, _ = LONG[name]
    return dict(small_models()[small], firings=F)


def long_params(name):
    return small_params(LONG[name][0])


def long_sweeps(name):
    if name not in _CACHE:
        m = long_model(name)
        F = m["firings"]
        _CACHE[name] = [SM.sweep(m, world=w, seed=seed, noise=noise, start_deg=360.0 - fw * 360.0 / F, holes=("nan",) if noise else ("zero",),
                                 drop=LONG_DROP.get(name, 0.01)) for fw, w, seed, noise in LONG[name][2]]
    return _CACHE[name]


def long_rows(name):
    if (name, "rows") not in _CACHE:
        L = len(long_model(name)["elev"])
        _CACHE[name, "rows"] = [rows_of(c, L) for c in long_sweeps(name)]
    return _CACHE[name, "rows"]


def short_sweep():
    """64 x 128: four tiles, for the ragged batch next to a 129-tile sweep."""
    if "short" not in _CACHE:
        _CACHE["short"] = SM.sweep(dict(small_models()["64 offsets"], firings=128), world=1, seed=49, noise=True, start_deg=77.7)
    return _CACHE["short"]


def seam_tiles(cloud, p, layout="firing"):
    """The tiles (2048 points in firing order) that hold participants of the last quarter of the sectors AND of the first: the sweep's
    wrap.  (With azimuth offsets every tile has falling sectors: tiles_where_sectors_fall does not single the seam out.)"""
    K = int(p.sectors)
    s = FS._sectors(cloud, p, layout).reshape(-1)
    out = []
    for t0 in range(0, len(s), FS.TILE):
        k = s[t0:t0 + FS.TILE]
        k = k[k >= 0]
        if len(k) and (k >= 3 * K // 4).any() and (k < K // 4).any():
            out.append(t0 // FS.TILE)
    return out


def tail_falls(cloud, p, layout="firing"):
    """tiles_where_sectors_fall of the last tile alone (0 or 1), from the whole sweep's stages."""
    s = FS._sectors(cloud, p, layout).reshape(-1)
    k = s[(len(s) - 1) // FS.TILE * FS.TILE:]
    k = k[k >= 0]
    return int(len(k) > 1 and (np.diff(k.astype(np.int32)) < 0).any())


# ---- dense sweeps ----
# model -> (firings, sweep keywords)
DENSE = {
    "hdl64e": (256, dict(noise=True, holes=("zero", "nan1", "inf"))),
    "vlp16": (304, dict(noise=True)),
    "vlp32c": (136, dict()),
    "128 stagger": (128, dict()),
}
DENSE_DROP = {"hdl64e": 0.01, "vlp16": 0.10, "vlp32c": 0.01, "128 stagger": 0.01}
DENSE_START = (77.7, 123.4, 77.7)
MERGED_AT = (5, 40, 42, 90)   # the third scan: firings that lose their trailing half, each followed by one that loses its leading half


def half_firings(cloud, L):
    """Random drops do not merge firings in the re-alignment at 64 and 128 lasers (none at a drop of 0.85: a firing's last laser or the
    next one's first is nearly always there), and a whole drop rate is not how a sensor loses them either: it loses a BLOCK -- the lower
    lasers of one firing, the upper ones of the next.  The firings of MERGED_AT lose lasers L/2.., their successors lasers ..L/2: the
    re-alignment joins each such pair into one firing (40..43: two pairs in a row)."""
    out = []
    for a in cloud:
        v = a.reshape(-1, L).copy()
        for f in MERGED_AT:
            v[f, L // 2:] = np.nan
            v[f + 1, :L // 2] = np.nan
        out.append(np.ascontiguousarray(v.reshape(-1)))
    return tuple(out)


def dense_model_of(name):
    return dict(small_models()[name], firings=DENSE[name][0]) if name == "128 stagger" else SM.MODELS[name]


def dense_lasers(name):
    return len(dense_model_of(name)["elev"])


def dense_params(name, K=360, cp=5):
    p = u.default_params().wide_roi()
    p.channels = dense_lasers(name)
    if p.channels == 128:
        p.interval = 0.05
    p.sectors, p.curbPoints = K, cp
    return p


def dense_width(name):
    return DENSE[name][0] + 3


def dense_scans(name):
    """Three scans per model: (dense cloud, slot per point, firings of the organised sweep, key) as tests/test_gpu_dense.py holds them,
    the padded twin appended."""
    if ("dense", name) not in _CACHE:
        F, kw = DENSE[name]
        L, W = dense_lasers(name), dense_width(name)
        out = []
        for k in range(3):
            cloud = SM.sweep(dense_model_of(name), firings=F, world=k, seed=200 + k, start_deg=DENSE_START[k], drop=DENSE_DROP[name], **kw)
            if k == 2:
                cloud = half_firings(cloud, L)
            dense, slot = D.densify(cloud, L, SM.missing_mask(cloud))
            pos, firings, aligned = D.realign(slot, L, W)
            assert aligned
            out.append((dense, slot, F, ("crossing", name, k), D.pad(dense, pos, L, W), firings))
        _CACHE["dense", name] = out
    return _CACHE["dense", name]


# ---- histories on one context ----
SHORT_W = 140


def short_dense_scans():
    """Two hdl64e scans of 128 firings: fewer scans, fewer points and another W than dense_scans("hdl64e")."""
    if "short dense" not in _CACHE:
        out = []
        for k in range(2):
            cloud = SM.sweep("hdl64e", firings=128, world=1 + k, seed=260 + k, start_deg=DENSE_START[k], noise=True, drop=0.01)
            dense, slot = D.densify(cloud, 64, SM.missing_mask(cloud))
            pos, firings, aligned = D.realign(slot, 64, SHORT_W)
            assert aligned
            out.append((dense, slot, 128, ("crossing", "short", k), D.pad(dense, pos, 64, SHORT_W), firings))
        _CACHE["short dense"] = out
    return _CACHE["short dense"]


def ideal_sweep():
    """64 x 256 without azimuth offsets: what the plain kernels keep at every sector count used."""
    if "ideal" not in _CACHE:
        _CACHE["ideal"] = SM.sweep("ideal64", firings=256, world=2, seed=21, holes=("nan",))
    return _CACHE["ideal"]


def shuffled_sweep():
    """An unorganised scan: the points of a 64 x 96 sweep in random order."""
    if "shuffled" not in _CACHE:
        c = u.synth_cloud(64, 96, 1, 77)
        pm = np.random.default_rng(3).permutation(len(c[0]))
        _CACHE["shuffled"] = tuple(np.ascontiguousarray(a[pm]) for a in c)
    return _CACHE["shuffled"]


# ---- 128 lasers, multi-sector fuzz ----
FUZZ128_BASE = 13_900_000   # (a base of its own)


def fuzz128_case(seed):
    """A 128-laser model with azimuth offsets per laser (the Ouster stagger, the HDL-64E's +- 2.4 degrees, or drift inside a firing), 64 /
    128 / 256 firings, curbPoints 1..8, 90 / 360 / 1022 sectors, interval 0.05; the rest as sensor_models.fuzz_case draws it."""
    rng = np.random.default_rng(FUZZ128_BASE + seed)
    elev = SM.MODELS["ideal128"]["elev"]
    kind = int(rng.integers(0, 3))
    if kind == 0:
        model = SM._model(elev, az=[SM._OS_STAGGER[l % 4] for l in range(128)])
    elif kind == 1:
        model = SM._model(elev, az=[(-2.4, -0.8, 0.8, 2.4)[l % 4] for l in range(128)])
    else:
        model = SM._model(elev, drift=float(rng.integers(2, 11)) * 0.001)
    firings = int((64, 128, 256)[int(rng.integers(0, 3))])
    nh = int(rng.integers(1, 4))
    holes = tuple(SM.HOLES[int(k)] for k in rng.integers(0, len(SM.HOLES), nh))
    start = float(rng.integers(0, 3600)) * 0.1 if rng.random() < 0.6 else 0.0
    cloud = SM.sweep(model, firings=firings, world=int(rng.integers(0, len(SM.WORLDS))), seed=int(rng.integers(1, 1 << 30)), start_deg=start,
                     noise=bool(rng.random() < 0.5), drop=float((0.0, 0.01, 0.1)[int(rng.integers(0, 3))]), holes=holes)
    p = u.default_params()
    if rng.random() < 0.6:
        p = p.wide_roi()
    else:
        p.min_X, p.max_X = float((-200.0, 0.0, 3.0)[int(rng.integers(0, 3))]), float((15.0, 30.0, 200.0)[int(rng.integers(0, 3))])
        p.min_Y, p.max_Y = float((-200.0, -10.0, -3.0)[int(rng.integers(0, 3))]), float((2.0, 10.0, 200.0)[int(rng.integers(0, 3))])
    p.max_Z = float((-1.0, -1.0, 0.5, 2.0, 10.0)[int(rng.integers(0, 5))])
    p.channels = 128
    p.x_zero_method = int(rng.random() < 0.9)
    p.z_zero_method = int(rng.random() < 0.9)
    p.star_shaped_method = int(rng.random() < 0.85)
    p.blind_spots = int(rng.random() < 0.7)
    p.xDirection = int(rng.integers(0, 3))
    p.curbHeight = float((0.02, 0.05, 0.1)[int(rng.integers(0, 3))])
    p.curbPoints = int(rng.integers(1, 9))
    p.angleFilter1 = float((120.0, 150.0, 175.0)[int(rng.integers(0, 3))])
    p.angleFilter2 = float((100.0, 140.0, 170.0)[int(rng.integers(0, 3))])
    p.starbeam_filter = int(rng.random() < 0.2)
    p.interval = 0.05
    p.sectors = int((90, 360, 1022)[int(rng.integers(0, 3))])
    return cloud, p, ("stagger", "offsets", "drift")[kind]


# ---- the switch walk: (multi_sector, multi_sector_curb_points, curbPoints) per step, front mode 3, 64 lasers, star-shaped search on ----
SWITCH_WALK = ((0, 0, 3), (1, 0, 3), (1, 1, 3), (0, 1, 3), (1, 1, 3), (1, 1, 5), (1, 0, 5))
# what urf_policy::plan makes of each step from the settings alone: (front, front_ms); tests/test_front_crossings_cpu.py reads it off plan()
SWITCH_PLAN = ((1, 0), (1, 0), (1, 1), (1, 0), (1, 1), (1, 1), (1, 1))


def plain_twins():
    """The "64 offsets" geometry WITHOUT its azimuth offsets, 64 x 256 in the worlds of small_sweeps: what the plain kernels keep, with as
    many rings per sweep as the multi-sector sweep it alternates with on a context (the ring count of a row's previous call is
    k_ring_table's hint: a call with another count would be handed back for it once)."""
    if "plain twins" not in _CACHE:
        m = dict(small_models()["64 offsets"], az=[0.0] * 64)
        _CACHE["plain twins"] = [SM.sweep(m, world=0, seed=5), SM.sweep(m, world=1, seed=6, noise=True, holes=("nan",))]
    return _CACHE["plain twins"]
