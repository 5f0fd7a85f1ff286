"""Sweeps as real spinning LiDARs' drivers deliver them (TEST CODE): a ray caster over small sensor models and a street with
obstacles.  What urf_synth_cloud (synth.cpp) does not model and the fused front end (urf_front.hpp) decides on per lane and per
firing: lasers that point upward (the reference measures a point with z >= 0 as asin + 90, so a laser at +e gets a ring of its own above
90 degrees once max_Z lets it in -- it does NOT share the ring of the laser at -e), uneven laser spacing, azimuth offsets per laser and drift inside a firing (a firing in several star sectors),
missing returns written as NaN / +Inf / far points, sweeps of any length, obstacles (holes in a ring's window, walls whose points
share a planar range).

Deterministic across numpy builds: float64 arrays through + - * / sqrt floor and comparisons only (sine and cosine by det_sincos
below, synth.cpp's polynomial without fma), random numbers from default_rng(seed).integers / .random, float32 out.
tests/test_sensor_models_cpu.py pins the sha256 of two sweeps: oracles._record_key hashes the input.

Holes in tests/fuzz_organised.py and tests/fuzz_lasers.py are (0, 0, 0) only; every other encoding comes from here."""
import numpy as np

DEG = 0.017453292519943295
H = 1.8              # sensor above the road [m]; the sensor is the origin
CURB_H = 0.15
MAX_RANGE = 120.0

HOLES = ("zero", "nan", "nan1", "inf", "far")   # how a missing return is written
FAR = (3.0e4, -2.0e4, 2.5e4)                    # "far": a finite point outside every region of interest (x + y + z != 0)


def det_sincos(a):
    """sin, cos of a float64 array, |a| < ~1e3, from IEEE basic operations: accuracy ~1e-16."""
    a = np.asarray(a, np.float64)
    kf = np.floor(a * 0.6366197723675814 + 0.5)
    r = (a - kf * 1.5707963267948966) - kf * 6.123233995736766e-17
    r2 = r * r
    ps = np.full_like(r, 1.0 / 355687428096000.0)
    for c in (-1.0 / 1307674368000.0, 1.0 / 6227020800.0, -1.0 / 39916800.0, 1.0 / 362880.0, -1.0 / 5040.0, 1.0 / 120.0, -1.0 / 6.0):
        ps = ps * r2 + c
    sn = r + (r * r2) * ps
    pc = np.full_like(r, -1.0 / 6402373705728000.0)
    for c in (1.0 / 20922789888000.0, -1.0 / 87178291200.0, 1.0 / 479001600.0, -1.0 / 3628800.0, 1.0 / 40320.0, -1.0 / 720.0,
              1.0 / 24.0, -0.5):
        pc = pc * r2 + c
    cs = 1.0 + r2 * pc
    q = kf - 4.0 * np.floor(kf * 0.25)   # kf mod 4
    s = np.where(q == 0.0, sn, np.where(q == 1.0, cs, np.where(q == 2.0, -sn, -cs)))
    c = np.where(q == 0.0, cs, np.where(q == 1.0, -sn, np.where(q == 2.0, -cs, sn)))
    return s, c


def _even(hi, lo, n):
    return [hi + (lo - hi) * k / (n - 1) for k in range(n)]


_VLP32C_ELEV = [-25, -1, -1.667, -15.639, -11.31, 0, -0.667, -8.843, -7.254, 0.333, -0.333, -6.148, -5.333, 1.333, 0.667, -4,
                -4.667, 1.667, 1, -3.667, -3.333, 3.333, 2.333, -2.667, -3, 7, 4.667, -2.333, -2, 15, 10.333, -1.333]
_VLP32C_AZ = [1.4, -4.2, 1.4, -1.4, 1.4, -1.4, 4.2, -1.4, 1.4, -4.2, 1.4, -1.4, 4.2, -1.4, 4.2, -1.4,
              1.4, -4.2, 1.4, -4.2, 4.2, -1.4, 1.4, -1.4, 1.4, -1.4, 1.4, -4.2, 4.2, -1.4, 1.4, -1.4]
_OS_STAGGER = [3.2, 1.1, -1.1, -3.2]


def _model(elev, az=None, drift=0.0, firings=2048, layout="firing"):
    """elev [deg] per laser slot in firing order, az: azimuth offset [deg] per slot, drift: azimuth [deg] the sensor turns from one
    slot of a firing to the next, firings per revolution, layout: "firing" (point f * L + l) or "rows" (point l * F + f)."""
    L = len(elev)
    return {"elev": [float(e) for e in elev], "az": [float(v) for v in (az or [0.0] * L)], "drift": float(drift),
            "firings": int(firings), "layout": layout}


MODELS = {
    "vlp16": _model([(-15 + l) if l % 2 == 0 else l for l in range(16)], drift=0.0083, firings=1808),
    "hdl32e": _model([(-30.67 if l % 2 == 0 else -9.33) + 1.3333 * (l // 2) for l in range(32)], drift=0.0057, firings=2170),
    "vlp32c": _model(_VLP32C_ELEV, az=_VLP32C_AZ, drift=0.0041, firings=1808),
    "hdl64e": _model(_even(2.0, 2.0 - 31 / 3.0, 32) + _even(-8.83, -24.33, 32), az=[(-2.4, -0.8, 0.8, 2.4)[l % 4] for l in range(64)],
                     firings=2083),
    "os64": _model(_even(22.5, -22.5, 64), az=[_OS_STAGGER[l % 4] for l in range(64)], firings=1024, layout="rows"),
    "os64d": _model(_even(22.5, -22.5, 64), firings=1024, layout="rows"),            # destaggered by the driver
    "os32": _model(_even(22.5, -22.5, 32), az=[_OS_STAGGER[l % 4] for l in range(32)], firings=1024, layout="rows"),
    "os32d": _model(_even(22.5, -22.5, 32), firings=1024, layout="rows"),
    "os128d": _model(_even(22.5, -22.5, 128), firings=1024, layout="rows"),          # channels = 128: the general kernels
    # the control: synth.cpp's sensor (downward only, one azimuth per firing) -- must take the fused kernels
    "ideal16": _model(_even(-15.0, -1.0, 16)),
    "ideal32": _model(_even(-24.8, -2.0, 32)),
    "ideal64": _model(_even(-24.8, -2.0, 64)),
    "ideal128": _model(_even(-24.8, -2.0, 128)),
}


def lasers(model):
    return len(MODELS[model]["elev"])


# worlds: |y| of the curb faces, y of the walls behind the sidewalks (left, right; None: none), boxes (x0, x1, y0, y1, z0, z1), z from the sensor
def _pole(x, y, top=3.0):
    return (x - 0.06, x + 0.06, y - 0.06, y + 0.06, -H, top)


WORLDS = [
    {"curb": 4.0, "walls": (9.0, -9.0), "top": 6.0,
     "boxes": [(6.0, 10.5, -3.2, -1.4, -H, -0.3), (-14.0, -9.5, 1.2, 3.0, -H, -0.35), (22.0, 26.4, 1.5, 3.3, -H, -0.2),
               _pole(5.0, 4.6), _pole(12.0, -4.7), _pole(-8.0, 4.5)]},
    {"curb": 3.0, "walls": (6.5, -7.5), "top": 5.0,
     "boxes": [(8.0, 12.4, 0.9, 2.7, -H, -0.3), (-30.0, -18.0, -2.8, -0.3, -H, 1.6), _pole(7.0, -3.5), _pole(-5.0, 3.6, 2.0)]},
    {"curb": 4.0, "walls": (7.0, None), "top": 8.0,
     "boxes": [(15.0, 15.3, -4.0, 4.0, -H, -0.6), (-6.0, -4.2, -3.4, -1.6, -H, -0.4), _pole(9.0, 4.4), _pole(9.0, -4.4),
               _pole(18.0, 4.4), _pole(18.0, -4.4)]},
    {"curb": 4.0, "walls": (None, None), "top": 0.0, "boxes": []},   # synth.cpp's street: nothing on it, nothing above the sensor
]


def _cast(dx, dy, dz, world):
    """Range along every ray to the nearest surface (inf: none)."""
    w = WORLDS[world]
    inf = np.inf
    down = dz < 0.0
    dzs = np.where(down, dz, -1.0)
    ady = np.where(dy < 0.0, -dy, dy)
    adys = np.where(ady > 0.0, ady, 1.0)
    t = -H / dzs                                   # the road
    tc = w["curb"] / adys
    beyond = (ady > 0.0) & (t * ady >= w["curb"])
    face = beyond & (tc * dzs < -H + CURB_H)
    t = np.where(face, tc, np.where(beyond, -(H - CURB_H) / dzs, t))
    t = np.where(down, t, inf)
    for wy in w["walls"]:                          # a wall: the plane y = wy from the sidewalk up to `top`
        if wy is None:
            continue
        toward = (dy > 0.0) if wy > 0 else (dy < 0.0)
        tw = (wy if wy > 0 else -wy) / adys
        hit = toward & (tw * dz <= w["top"]) & (tw * dz >= -(H - CURB_H))
        t = np.where(hit & (tw < t), tw, t)
    for x0, x1, y0, y1, z0, z1 in w["boxes"]:      # slabs
        lo, hi = np.zeros_like(dx), np.full_like(dx, inf)
        for d, a0, a1 in ((dx, x0, x1), (dy, y0, y1), (dz, z0, z1)):
            ds = np.where(d == 0.0, 1e-300, d)
            ta, tb = a0 / ds, a1 / ds
            lo = np.maximum(lo, np.where(ta < tb, ta, tb))
            hi = np.minimum(hi, np.where(ta < tb, tb, ta))
        hit = (lo <= hi) & (lo > 0.0)
        t = np.where(hit & (lo < t), lo, t)
    return t


def sweep(model, firings=None, world=0, seed=1, start_deg=0.0, noise=False, drop=0.01, holes=("zero",), layout=None, points=None):
    """One sweep of `model` (MODELS) through world `world`: (x, y, z) float32 in the model's layout (or `layout`).
    firings: per revolution (default: the model's); start_deg: azimuth of the first firing; noise: range noise (sigma ~1 cm) and
    2 mm range steps, which make planar-range ties; drop: share of returns lost at random; holes: the encodings (HOLES) missing
    returns are written in, drawn per point when several are given; points: cut a firing-order sweep to that many points."""
    m = MODELS[model] if isinstance(model, str) else model   # (a dict: a model of the caller's own)
    L = len(m["elev"])
    F = int(firings or m["firings"])
    rng = np.random.default_rng(seed)
    f = np.arange(F, dtype=np.float64)[:, None]
    l = np.arange(L, dtype=np.float64)[None, :]
    az = (np.asarray(m["az"], np.float64)[None, :] + m["drift"] * l) * DEG
    th = start_deg * DEG + (f + 0.5) * (6.283185307179586 / F) + az
    st, ct = det_sincos(th)
    se, ce = det_sincos(np.asarray(m["elev"], np.float64) * DEG)
    dx, dy, dz = ce[None, :] * ct, ce[None, :] * st, se[None, :] + 0.0 * ct
    t = _cast(dx, dy, dz, world)
    n = F * L
    if noise:
        u = rng.random((4, F, L))
        g = ((u[0] + u[1]) + (u[2] + u[3]) - 2.0) * 1.7320508075688772   # Irwin-Hall of four: variance 1
        t = np.where(t < np.inf, np.floor((t + 0.01 * g) / 0.002 + 0.5) * 0.002, t)
    else:
        t = t * (1.0 + 1e-4 * (2.0 * rng.random((F, L)) - 1.0))
    missing = ~(t < MAX_RANGE) | (rng.random((F, L)) < drop)
    tt = np.where(t < MAX_RANGE, t, MAX_RANGE)
    x, y, z = (tt * dx).astype(np.float32), (tt * dy).astype(np.float32), (tt * dz).astype(np.float32)
    # what the reference leaves undefined: no azimuth in (-5e-7, 0) rad (sector 360), no point on the sensor's axis
    y = np.where((x > 0.0) & (y < 0.0) & (-y <= np.float32(1e-6) * x), np.float32(0.0), y)
    assert not ((x == 0.0) & (y == 0.0) & ~missing).any()
    kind = rng.integers(0, len(holes), (F, L))
    which = rng.integers(0, 3, (F, L))
    nan, inf32 = np.float32(np.nan), np.float32(np.inf)
    for k, h in enumerate(holes):
        sel = missing & (kind == k)
        if h == "zero":
            x, y, z = (np.where(sel, np.float32(0.0), a) for a in (x, y, z))
        elif h == "nan":
            x, y, z = (np.where(sel, nan, a) for a in (x, y, z))
        elif h == "nan1":      # one field only; the other two keep the ray's point at its range (or the maximum range)
            x, y, z = (np.where(sel & (which == j), nan, a) for j, a in enumerate((x, y, z)))
        elif h == "inf":
            x, y, z = np.where(sel, inf32, x), np.where(sel, np.float32(0.0), y), np.where(sel, np.float32(0.0), z)
        elif h == "far":
            x, y, z = (np.where(sel, np.float32(v), a) for v, a in zip(FAR, (x, y, z)))
        else:
            raise KeyError(h)
    if (layout or m["layout"]) == "rows":
        x, y, z = x.T, y.T, z.T
    out = tuple(np.ascontiguousarray(a, np.float32).reshape(-1) for a in (x, y, z))
    return out if points is None else tuple(a[:points].copy() for a in out)


def missing_mask(cloud):
    """The points no region of interest keeps, whichever way they are written."""
    x, y, z = cloud
    with np.errstate(invalid="ignore"):
        return ~(np.isfinite(x) & np.isfinite(y) & np.isfinite(z)) | ((x == 0) & (y == 0) & (z == 0)) | (x == np.float32(FAR[0]))


def params_for(model, wide=True, max_Z=None, interval=None, channels=None):
    import urban_road_filter_amd as u
    p = u.default_params()
    if wide:
        p = p.wide_roi()
    p.channels = channels or lasers(model)
    if max_Z is not None:
        p.max_Z = max_Z
    if interval is not None:
        p.interval = interval
    return p


def fuzz_case(seed, L):
    """A random model of L lasers, world, encoding mix, start azimuth, region of interest (max_Z too) and detector parameters
    (tests/fuzz_lasers.py's idea)."""
    import urban_road_filter_amd as u
    rng = np.random.default_rng(seed)
    names = sorted(k for k in MODELS if lasers(k) == L)
    model = names[int(rng.integers(0, len(names)))]
    firings = int((256, 512, 1024, 1808, 2048, 2170)[int(rng.integers(0, 6))])
    nh = int(rng.integers(1, 4))
    holes = tuple(HOLES[int(k)] for k in rng.integers(0, len(HOLES), nh))
    start = float(rng.integers(0, 3600)) * 0.1 if rng.random() < 0.6 else 0.0
    cloud = sweep(model, firings=firings, world=int(rng.integers(0, len(WORLDS))), seed=int(rng.integers(1, 1 << 30)), start_deg=start,
                  noise=bool(rng.random() < 0.5), drop=float((0.0, 0.01, 0.1)[int(rng.integers(0, 3))]), holes=holes)
    p = u.default_params()
    if rng.random() < 0.6:
        p = p.wide_roi()
    else:
        p.min_X, p.max_X = float((-200.0, 0.0, 3.0)[int(rng.integers(0, 3))]), float((15.0, 30.0, 200.0)[int(rng.integers(0, 3))])
        p.min_Y, p.max_Y = float((-200.0, -10.0, -3.0)[int(rng.integers(0, 3))]), float((2.0, 10.0, 200.0)[int(rng.integers(0, 3))])
    p.max_Z = float((-1.0, -1.0, 0.5, 2.0, 10.0)[int(rng.integers(0, 5))])
    p.channels = L
    p.x_zero_method = int(rng.random() < 0.9)
    p.z_zero_method = int(rng.random() < 0.9)
    p.star_shaped_method = int(rng.random() < 0.85)
    p.blind_spots = int(rng.random() < 0.7)
    p.xDirection = int(rng.integers(0, 3))
    p.curbHeight = float((0.02, 0.05, 0.1)[int(rng.integers(0, 3))])
    p.curbPoints = int((5, 5, 5, 5, 2, 9)[int(rng.integers(0, 6))])
    p.angleFilter1 = float((120.0, 150.0, 175.0)[int(rng.integers(0, 3))])
    p.angleFilter2 = float((100.0, 140.0, 170.0)[int(rng.integers(0, 3))])
    p.starbeam_filter = int(rng.random() < 0.2)
    p.interval = float((0.18, 0.18, 0.5, 1.5, 0.1)[int(rng.integers(0, 5))])
    return cloud, p, model
