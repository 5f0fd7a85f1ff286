"""The cases of tests/test_gpu_param_edges.py (built on the CPU), shared with tests/test_param_edges_cpu.py, which judges oracle B on
them against the reference's own sources: every live parameter of cfg/LidarFilters.cfg at the ends of its declared range.

The box comes from urf_param_table() (u.param_table()), not from literals: a new cfg row or a changed range is a new case.

ONE_AT_A_TIME  the defaults of the cloud's model with one field changed: every numeric hot-path row at its min and at its max, every
               bool at its other value, xDirection 1 and 2, angleFilter3 90 (slope_param = pi / 2), curbPoints 8 (the fused front end's last).  The ends of the region-of-interest
               rows hold the empty regions min_X 200, max_X -200, min_Z 200, max_Y -200 (EMPTY_ROI).
CORNERS        48 seeded corners of the box: every numeric field from {min, default, max}, every bool from {0, 1}; min_Z from {-200, -3}
               and max_Z from {-1, 200} (the region is not empty in z by construction).
OUTSIDE        values outside the box that urf_set_params accepts and the reference stays defined at, one field at a time.

A case is (name, tweak): tweak maps urf_params members to values, params(base, tweak) applies it to a copy of the base."""
import numpy as np

import fuzz
import gpu_sensor_cases as G
import sensor_models as SM
import urban_road_filter_amd as u

IN_PARAMS = 0   # URF_PARAM_IN_PARAMS
NAN, INF = float("nan"), float("inf")
FIRINGS = 256
FRONT_MAX_CURB_POINTS = 8   # the last curbPoints the fused front end has an instance for (include/urf.h: front mode 3)


def hot_rows():
    """The rows of the live parameter surface that live in urf_params."""
    return [t for t in u.param_table() if t["where"] == IN_PARAMS]


def _value(t, v):
    return float(v) if t["type"] == u.PARAM_DOUBLE else int(v)


def _name(field, v):
    return "%s %s" % (field, ("%g" % v) if isinstance(v, float) else v)


def one_at_a_time():
    cases = []
    for t in hot_rows():
        f = t["field"]
        if t["type"] == u.PARAM_BOOL:
            vals = [1 - int(t["default"])]
        else:
            vals = [_value(t, t["min"]), _value(t, t["max"])]
            if f == "xDirection":
                vals = [0, 1, 2]
            if f == "angleFilter3":
                vals.insert(1, 90.0)
            if f == "curbPoints":
                vals.insert(1, FRONT_MAX_CURB_POINTS)
        cases += [(_name(f, v), {f: v}) for v in vals]
    return cases


def corners(count=48, seed=20240):
    rng = np.random.default_rng(seed)
    cases = []
    for k in range(count):
        tweak = {}
        for t in hot_rows():
            f = t["field"]
            if t["type"] == u.PARAM_BOOL:
                tweak[f] = int(rng.integers(0, 2))
            elif f == "min_Z":
                tweak[f] = (_value(t, t["min"]), _value(t, t["default"]))[int(rng.integers(0, 2))]
            elif f == "max_Z":
                tweak[f] = (_value(t, t["default"]), _value(t, t["max"]))[int(rng.integers(0, 2))]
            else:
                tweak[f] = _value(t, (t["min"], t["default"], t["max"])[int(rng.integers(0, 3))])
        cases.append(("corner %02d" % k, tweak))
    return cases


def outside():
    vals = [("interval", (0.0, 100.0, INF)), ("beamZone", (0.5, 180.0, 200.0, 360.0)), ("angleFilter1", (-1.0, 200.0, NAN)),
            ("angleFilter2", (-1.0, 200.0, NAN)), ("angleFilter3", (-10.0, NAN)), ("curbHeight", (0.0, -0.1, NAN)),
            ("kdist_param", (0.0,)), ("kdev_param", (0.0, -1.0)), ("dmin_param", (0, -5, 100000)), ("max_Z", (INF,)),
            ("min_X", (NAN,)), ("beam_width", (0.0, 5.0))]
    cases = [(_name(f, v), {f: v}) for f, vs in vals for v in vs]
    # (the beam's width is read with the rectangular beam on only: the two values once more where they decide something)
    return cases + [(_name("beam_width", v) + " starbeam", {"beam_width": v, "starbeam_filter": 1}) for v in (0.0, 5.0)]


ONE_AT_A_TIME = one_at_a_time()
CORNERS = corners()
OUTSIDE = outside()
TABLES = {"one": ONE_AT_A_TIME, "corner": CORNERS, "outside": OUTSIDE}
EMPTY_ROI = ("min_X 200", "max_X -200", "min_Z 200", "max_Y -200")
# The edges that change no label on any cloud below although they change the parameters: the region of interest's z keeps every return
# of these worlds from -3 m down already.  (An edge equal to the base value changes nothing by construction: is_base_value.)
NEUTRAL = ("min_Z -200",)


def params(base, tweak):
    p = base.copy()
    for f, v in tweak.items():
        setattr(p, f, v)
    return p


def is_base_value(base, tweak):
    return bytes(params(base, tweak)) == bytes(base)


def case(table, name):
    return dict(TABLES[table])[name]


# ---- clouds ----
def base_params(L):
    """The defaults of a sweep of L lasers per firing, every return of the worlds inside the region (the upward lasers too)."""
    return SM.params_for("ideal%d" % L if L in (16, 32, 64) else "ideal64", max_Z=2.0, channels=L)


FUSED = [(L, layout) for L in (16, 32, 64) for layout in ("firing", "rows")]
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def ideal_batch(L, layout):
    """Two ideal sweeps of 256 firings (2 / 4 / 8 tiles of 2048 points): world 0, and world 1 with range noise and NaN holes."""
    return _cached(("ideal", L, layout), lambda: [
        G.control("ideal%d" % L, FIRINGS, world=w, seed=90 + w, layout=layout, noise=w == 1, holes=("zero",) if w == 0 else ("nan",))
        for w in (0, 1)])


REAL = ("hdl64e", "vlp16", "hdl32e")


def real_sweep(model):
    return _cached(("real", model), lambda: SM.sweep(model, firings=FIRINGS, world=0, seed=95, noise=True, holes=("nan",)))


def fuzz_cloud(tie_grid):
    """3000 unorganised points (tests/fuzz.py), with and without planar-range ties."""
    def make():
        rng = np.random.default_rng(4242)
        while True:
            c = fuzz.random_cloud(rng, 3000, tie_grid)
            if len(c[0]) > 2500:   # (a cloud of a few rings keeps one point per planar range: a few dozen)
                return c
    return _cached(("fuzz", tie_grid), make)


def fuzz_params():
    return u.default_params().wide_roi()


JITTER_DEG = 0.04


def jitter_sweep():
    """An ideal64 sweep in firing order whose points leave their laser's cone by up to +-0.04 degrees of elevation (z moves, the planar
    range stays) from the second firing on; the first firing is complete and exact, so the ring table is the 64 lasers' at any interval.
    Range noise alone moves a point along its ray: it stays on its ring whatever the interval.  With interval 0.01 the points further
    than that from their laser's table entry find no ring (n_ring_pts falls, n_rings stays 64); with 0.18 all of them do."""
    def make():
        m = SM.MODELS["ideal64"]
        rng = np.random.default_rng(77)
        x, y, z = G.control("ideal64", FIRINGS, world=3, seed=97, drop=0.0)
        d = (2.0 * rng.random(len(x)) - 1.0) * JITTER_DEG * SM.DEG
        d[:64] = 0.0
        e = np.tile(np.asarray(m["elev"], np.float64) * SM.DEG, FIRINGS)
        s0, c0 = SM.det_sincos(e)
        s1, c1 = SM.det_sincos(e + d)
        rho_z = z.astype(np.float64) * (c0 / s0)            # z / tan(e): the planar range (signed as z)
        return x, y, (rho_z * (s1 / c1)).astype(np.float32)
    return _cached("jitter", make)


def ring_per_laser(st, info, L, layout):
    """Oracle B's ring stage of an organised sweep: every laser slot's ring points on ONE ring and every ring one slot's -- what the fused
    front end's lane per laser presumes.  The ring count alone does not say it: with interval 0 the table's L entries are the first L
    bit-different angles, and a laser whose angles differ in the last bit owns two of them."""
    n = len(st["ring"])
    slot = (np.arange(n) % L) if layout == "firing" else (np.arange(n) // (n // L))
    on = st["ring"] >= 0
    pairs = set(zip(slot[on].tolist(), st["ring"][on].tolist()))
    return info["status"] == 0 and info["n_rings"] == L and len(pairs) == len({s for s, _ in pairs}) == len({r for _, r in pairs}) == L


def general_clouds():
    """(name, cloud, base parameters) of the single scans the general kernels take."""
    out = [("fuzz", fuzz_cloud(0.0), fuzz_params()), ("fuzz ties", fuzz_cloud(1.0 / 16), fuzz_params())]
    out += [(m, real_sweep(m), base_params(SM.lasers(m))) for m in REAL]
    out += [("ideal%d %s w%d" % (L, layout, w), ideal_batch(L, layout)[w], base_params(L)) for L, layout, w in
            ((64, "firing", 0), (32, "rows", 1), (16, "firing", 1))]
    out.append(("jitter", jitter_sweep(), base_params(64)))
    return out


def corner_params(tweak, L):
    """A corner on a cloud of L lasers: channels is the cloud's laser count."""
    p = params(u.default_params(), tweak)
    p.channels = L
    return p
