"""The sweeps and parameters of tests/test_gpu_sensor_models.py (built on the CPU, from tests/sensor_models.py): shared with
tests/test_sensor_models_cpu.py, which checks that oracle B finds road and curb on every one of them -- no GPU comparison passes on
an empty result."""
import sensor_models as SM

REAL = ("vlp16", "hdl32e", "vlp32c", "hdl64e", "os64", "os64d", "os32", "os32d")
SETTINGS = {"default": {}, "max_Z 0.5": {"max_Z": 0.5}, "max_Z 2.0": {"max_Z": 2.0}, "interval 0.5": {"interval": 0.5},
            "interval 1.5": {"interval": 1.5}}   # (interval 0.18 is the default)
ENCODINGS = ("nan", "nan1", "inf", "far", SM.HOLES)          # the last one: all five mixed in one sweep
ENCODING_MODELS = (("ideal16", "firing"), ("ideal32", "firing"), ("ideal64", "firing"), ("vlp16", "firing"), ("hdl32e", "firing"),
                   ("hdl64e", "firing"), ("ideal64", "rows"), ("ideal32", "rows"), ("os64d", "rows"), ("os32", "rows"))
TILE = 2048
MAX_TILES = 128   # URF_FRONT_MAX_TILES


def ideal_of(model):
    return "ideal%d" % SM.lasers(model)


def control(model, firings, **kw):
    """The ideal sweep of the model's laser count and length, started a fraction of a firing off zero where firings would otherwise
    lie on whole degrees (2170 firings: number 108 at 18 degrees) -- on a sector's border the float azimuths of one firing's points
    fall on either side, and a firing in two sectors is handed back by contract."""
    for ph in (0.0, 0.125, 0.0625, 0.1875):
        deg = [(f + 0.5 + ph) * 360.0 / firings for f in range(firings)]
        if min(abs(d - round(d)) for d in deg) > 1e-3:
            break
    return SM.sweep(ideal_of(model), firings=firings, start_deg=ph * 360.0 / firings, **kw)


def model_batch(model):
    """The model in its own layout in three worlds, the ideal control (same laser count, layout and length) second."""
    m = SM.MODELS[model]
    return [SM.sweep(model, world=0, seed=31, noise=True, holes=("nan",)),
            control(model, m["firings"], world=0, seed=32, layout=m["layout"]),
            SM.sweep(model, world=1, seed=33),
            SM.sweep(model, world=2, seed=34, start_deg=77.7, noise=True, holes=SM.HOLES)]


def ideal_batch(L, layout, firings=2048):
    """Ideal sweeps whose seam falls on a tile border (the start, or 45 degrees = a whole number of tiles at 2048 firings)."""
    name = "ideal%d" % L
    return [SM.sweep(name, firings=firings, world=w, seed=40 + w, layout=layout, noise=w == 1, start_deg=45.0 if w == 2 else 0.0,
                     holes=("nan",) if w == 0 else ("zero",)) for w in (0, 1, 2, 3)]


def encoding_pair(model, layout, holes, world):
    """The same sweep with (0, 0, 0) holes and with `holes`."""
    kw = dict(world=world, seed=50 + world, layout=layout, noise=world == 1, drop=0.03)
    return SM.sweep(model, holes=("zero",), **kw), SM.sweep(model, holes=holes if isinstance(holes, tuple) else (holes,), **kw)


def long_sweep(L, tiles, extra_points=0, seed=60, holes=("nan",)):
    """An ideal sweep of exactly tiles * 2048 (+ extra_points) points."""
    pts = tiles * TILE + extra_points
    F = (pts + L - 1) // L
    return SM.sweep("ideal%d" % L, firings=F, world=0, seed=seed, holes=holes, points=pts)


def five_hertz_batch(model, firings):
    scans = [SM.sweep(model, firings=firings, world=w, seed=70 + w, noise=w == 1, holes=("nan",)) for w in (0, 1)]
    return scans + [control(model, firings, world=2, seed=73, holes=("nan",))]


def long_ragged_batch(L):
    """127 tiles and a partial one that ends inside a firing, a short sweep, 128 tiles."""
    return [long_sweep(L, MAX_TILES - 1, 1000 + 7, seed=66), SM.sweep("ideal%d" % L, firings=512, world=1, seed=65, noise=True),
            long_sweep(L, MAX_TILES, seed=61)]


def chain_batch():
    return [SM.sweep("vlp16", world=s % 3, seed=80 + s, noise=s % 2 == 1, holes=("nan",) if s < 2 else SM.HOLES) for s in range(4)]


def params(model, setting="default", **kw):
    return SM.params_for(model, **dict(SETTINGS[setting], **kw))


def all_cpu_checkable_cases():
    """(name, scans, params) of the fixed GPU cases (the fuzz aside; of a pair of encodings the one with other holes than (0, 0, 0): B's
    result is the same for both)."""
    for model in REAL + ("os128d",):
        scans = model_batch(model)
        for sname in SETTINGS:
            yield "%s / %s" % (model, sname), scans, params(model, sname)
    for L in (16, 32, 64):
        for layout in ("firing", "rows"):
            scans = ideal_batch(L, layout)
            for sname in ("default", "max_Z 2.0", "interval 0.5"):
                yield "ideal%d %s" % (L, layout), scans, params("ideal%d" % L, sname)
    for model, layout in ENCODING_MODELS:
        for h in ENCODINGS:
            yield "%s %s %s" % (model, layout, h), [encoding_pair(model, layout, h, w)[1] for w in (0, 1)], params(model, "max_Z 2.0")
    for L in (16, 32, 64):
        yield "long %d" % L, long_ragged_batch(L) + [long_sweep(L, MAX_TILES + 1, seed=63)], params("ideal%d" % L)
    for model, firings in (("vlp16", 3616), ("hdl32e", 4340)):
        for sname in ("default", "max_Z 2.0"):
            yield "%s 5 Hz" % model, five_hertz_batch(model, firings), params(model, sname)
    yield "chain", chain_batch(), params("vlp16", "max_Z 0.5")
