"""urf_set_front_multi_sector, the CPU side: what stands between a real sensor's sweep and the fused front end, pinned from oracle
B's stages (tests/front_shape.py), so that the GPU counts of tests/test_gpu_front_multi.py have something to be compared with.

With the switch on, the one-sector rule and the seam rule are gone; what remains is front_shape.fusable.  The figures: every sweep of the
eight real models' batches (tests/gpu_sensor_cases.py) is fusable at the settings `default`, `max_Z 0.5` and `max_Z 2.0`; at `interval
0.5` exactly the sweeps whose neighbouring lasers merge into one ring are not; every non-control sweep of the six models with azimuth
offsets or drift has firings in several sectors; sweep 3 of every batch (started at 77.7 degrees) has its seam inside a tile."""
import os
import re

import numpy as np
import pytest

import front_shape as FS
import gpu_sensor_cases as G
import sensor_models as SM
import urban_road_filter_amd as u

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFFSET_MODELS = ("vlp16", "hdl32e", "vlp32c", "hdl64e", "os64", "os32")   # drift inside a firing, or an azimuth offset per laser
# interval 0.5: the sweeps in which neighbouring lasers share a ring (handed back by design)
MERGED = {"vlp32c": (0, 2, 3), "hdl64e": (0, 1, 2, 3), "os64": (1,), "os64d": (1,)}
# sweeps a context with the switch OFF fuses on its second mode-2 call ("Real sensor geometries"): the ideal control
# (sweep 1) of every batch, and of the destaggered Ouster batches every sweep whose seam lies on a tile border (0, 1, 2)
FUSED_TODAY = {"vlp16": (1,), "hdl32e": (1,), "vlp32c": (1,), "hdl64e": (1,), "os64": (1,), "os32": (1,), "os64d": (0, 1, 2), "os32d": (0, 1, 2)}
_BATCH = {}


def batch(model):
    if model not in _BATCH:
        _BATCH[model] = G.model_batch(model)
    return _BATCH[model]


def layout(model):
    return SM.MODELS[model]["layout"]


# the small custom models of tests/test_gpu_front_multi.py: (lasers, firings, model dict)
def small_models():
    hd = SM.MODELS["hdl64e"]
    return {
        "64 offsets": SM._model(hd["elev"], az=[(-2.4, -0.8, 0.8, 2.4)[l % 4] for l in range(64)], firings=256),
        "32 vlp32c": SM._model(SM._VLP32C_ELEV, az=SM._VLP32C_AZ, firings=256),
        "16 drift": SM._model(SM.MODELS["vlp16"]["elev"], drift=0.05, firings=512),
        "128 stagger": SM._model(SM.MODELS["ideal128"]["elev"], az=[SM._OS_STAGGER[l % 4] for l in range(128)], firings=64),
    }


def small_params(name):
    p = u.default_params().wide_roi()
    p.channels = len(small_models()[name]["elev"])
    if p.channels == 128:
        p.interval = 0.05   # (neighbouring lasers keep rings of their own)
    return p


_SMALL = {}


def small_sweeps(name):
    """Two sweeps of a small model (built once, read only): the second with range noise, whose equal planar ranges make the input order
    inside a sector matter."""
    if name not in _SMALL:
        m = small_models()[name]
        _SMALL[name] = [SM.sweep(m, world=0, seed=5, start_deg=77.7), SM.sweep(m, world=1, seed=6, noise=True, start_deg=123.4, holes=("nan",))]
    return _SMALL[name]


def seam_sweeps(name):
    """The wrap from sector 359 to 0 in the middle of the second tile, and on the last firing of the second tile."""
    m = small_models()[name]
    F, fpt = m["firings"], FS.TILE // len(m["elev"])
    return [SM.sweep(m, world=0, seed=7 + k, noise=bool(k), start_deg=360.0 - fw * 360.0 / F) for k, fw in enumerate((fpt + fpt // 2, 2 * fpt - 1))]


def ragged_scans():
    """A scan that ends inside a firing and inside a tile; one with a tile without a participant (a stretch of NaN firings); one with a
    tile whose 2048 points all take part (64 downward lasers over an empty street, no drop-outs)."""
    m = small_models()["64 offsets"]
    cut = SM.sweep(m, world=0, seed=11, noise=True, start_deg=50.0, points=64 * 100 + 17)
    gap = tuple(a.copy() for a in SM.sweep(m, world=1, seed=12, start_deg=200.0))
    for a in gap:
        a[2 * FS.TILE:3 * FS.TILE] = np.nan
    down = SM._model(SM.MODELS["ideal64"]["elev"], az=m["az"], firings=256)
    full = SM.sweep(down, world=3, seed=13, drop=0.0, start_deg=300.0)
    return [cut, gap, full]


@pytest.mark.parametrize("setting", ["default", "max_Z 0.5", "max_Z 2.0"])
@pytest.mark.parametrize("model", G.REAL)
def test_every_real_sweep_is_fusable_but_for_its_sectors(model, setting):
    p = G.params(model, setting)
    assert [FS.fusable(c, p, layout(model)) for c in batch(model)] == [True] * 4


@pytest.mark.parametrize("model", G.REAL)
def test_interval_half_a_degree_merges_neighbouring_lasers(model):
    p = G.params(model, "interval 0.5")
    got = tuple(k for k, c in enumerate(batch(model)) if not FS.fusable(c, p, layout(model)))
    assert got == MERGED.get(model, ())


@pytest.mark.parametrize("model", G.REAL)
def test_the_predicate_accepts_what_is_fused_today(model):
    for setting in ("default", "max_Z 0.5", "max_Z 2.0"):
        p = G.params(model, setting)
        for k in FUSED_TODAY[model]:
            assert FS.fusable(batch(model)[k], p, layout(model)), (setting, k)


@pytest.mark.parametrize("model", OFFSET_MODELS)
def test_offsets_and_drift_put_a_firing_into_several_sectors(model):
    p = G.params(model, "default")
    for k in (0, 2, 3):
        n, most = FS.multi_sector_firings(batch(model)[k], p, layout(model))
        print("%s sweep %d: %d firings of %d in more than one sector, at most %d" % (model, k, n, SM.MODELS[model]["firings"], most))
        assert n > 0 and 2 <= most <= 5
    if model in ("vlp32c", "hdl64e", "os64", "os32"):   # a fixed offset per laser: every firing
        assert FS.multi_sector_firings(batch(model)[0], p, layout(model))[0] == SM.MODELS[model]["firings"]


@pytest.mark.parametrize("model", G.REAL)
def test_the_seam_of_sweep_three_lies_inside_a_tile(model):
    assert FS.tiles_where_sectors_fall(batch(model)[3], G.params(model, "default"), layout(model)) >= 1


@pytest.mark.parametrize("name", sorted(small_models()))
def test_the_small_models_have_both_properties_and_a_result(name):
    p = small_params(name)
    for c in small_sweeps(name) + seam_sweeps(name):
        lb, ib, st = FS.stages(c, p)
        assert ib["status"] == 0 and ib["n_road"] > 0 and ib["n_curb"] > 0, ib
        assert FS.fusable(c, p)
        assert FS.multi_sector_firings(c, p)[0] > 0 and FS.tiles_where_sectors_fall(c, p) >= 1


def test_the_seam_sweeps_wrap_where_they_say():
    """(64 x 256: 32 firings per tile; the first sector-0 participant of laser 1, offset -0.8 degrees, after the wrap)"""
    name = "64 offsets"
    p = small_params(name)
    for c, fw in zip(seam_sweeps(name), (48, 63)):
        sec = FS.firing_order(FS.stages(c, p)[2]["sector"], 64, "firing")
        before, after = sec[:fw - 4], sec[fw + 4:fw + 20]   # (the offsets spread a firing over +- 2.4 degrees: under two firings)
        assert (before[before >= 0] > 180).all() and (after[after >= 0] < 180).all() and (after >= 0).any()


def test_the_ragged_scans_hold_what_they_are_for():
    p = small_params("64 offsets")
    cut, gap, full = ragged_scans()
    assert len(cut[0]) % 64 != 0 and len(cut[0]) % FS.TILE != 0
    for c in (cut, gap, full):
        ib = FS.stages(c, p)[1]
        assert ib["status"] == 0 and ib["n_road"] > 0 and FS.fusable(c, p) and FS.multi_sector_firings(c, p)[0] > 0
    part = FS.stages(gap, p)[2]["sector"] >= 0
    assert not part[2 * FS.TILE:3 * FS.TILE].any() and part[:2 * FS.TILE].any() and part[3 * FS.TILE:].any()
    part = (FS.stages(full, p)[2]["sector"] >= 0).reshape(-1, FS.TILE)
    assert part.all(axis=1).any()


def test_the_symbol_is_declared_wrapped_and_exported():
    header = open(os.path.join(ROOT, "include", "urf.h")).read()
    assert re.search(r"\bint\s+urf_set_front_multi_sector\s*\(\s*urf_ctx\s*\*\s*ctx\s*,\s*int\s+on\s*\)\s*;", header)
    assert callable(getattr(u.Context, "set_front_multi_sector", None))
    # (both C++ adapters have its setter: tests/test_front_switches_api.py)
    lib = u.lib()
    assert hasattr(lib, "urf_set_front_multi_sector")
    assert lib.urf_set_front_multi_sector(None, 1) == -1   # (no context: URF_ERR_INVALID_ARG, before anything touches a device)
