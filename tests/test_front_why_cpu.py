"""What urf_front_explain counts, pinned on the CPU: tests/front_why_model.py (oracle B's stages) on the small sweeps and the sensor models'
batches that tests/test_gpu_front_explain.py asks the kernel about -- a GPU comparison against a model that counts nothing shows nothing.

The counters, in front_why_model.FIELDS' order: (laser slots with two rings, rings with two slots, ring points on the axis, participants
out of range, firings in several sectors, the most sectors in one firing, tiles in which the sectors fall)."""
import os
import re

import numpy as np
import pytest

import front_shape as FS
import front_why_model as WM
import fuzz_history as H
import gpu_sensor_cases as G
import sensor_models as SM
import urban_road_filter_amd as u
from test_front_multi_cpu import batch as real_batch
from test_front_multi_cpu import ragged_scans, small_params, small_sweeps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CASES = {}


def rows_of(c, L):
    return tuple(np.ascontiguousarray(a.reshape(-1, L).T.reshape(-1)) for a in c)


def small_cases():
    """name -> (sweep, parameters, layout): built once, read only."""
    if _CASES:
        return _CASES
    p16 = SM.params_for("ideal16")
    a = SM.sweep("ideal16", firings=256, world=0, seed=1)
    _CASES["ideal16"] = (a, p16, "firing")
    _CASES["ideal16 from 77.7"] = (SM.sweep("ideal16", firings=256, world=0, seed=1, start_deg=77.7), p16, "firing")
    # a ring point of laser slot 3: lifted onto slot 4's elevation / put on the sensor's axis
    ring = FS.stages(a, p16)[2]["ring"]
    i = [k for k in np.flatnonzero(ring >= 0) if k % 16 == 3][10]
    lifted = tuple(v.copy() for v in a)
    lifted[2][i] = np.float32(np.hypot(float(a[0][i]), float(a[1][i])) * np.tan(np.deg2rad(SM.MODELS["ideal16"]["elev"][4])))
    _CASES["lifted"] = (lifted, p16, "firing")
    axis = tuple(v.copy() for v in a)
    axis[0][i] = axis[1][i] = 0
    _CASES["on the axis"] = (axis, p16, "firing")
    _CASES["interval 1.5"] = (a, SM.params_for("ideal16", interval=1.5), "firing")
    E = H.pool("small")   # (16 x 300 and 32 x 130 with a firing astride a sector border)
    _CASES["16 x 300"] = (E["a16s1"].cloud, H.make_params(16, True, 5, H.VARIANTS[0]), "firing")
    _CASES["32 x 130"] = (E["a32s1"].cloud, H.make_params(32, True, 5, H.VARIANTS[0]), "firing")
    _CASES["ideal64 x 64"] = (SM.sweep("ideal64", firings=64, world=0, seed=1), SM.params_for("ideal64"), "firing")
    _CASES["ideal16 rows"] = (rows_of(a, 16), p16, "rows")
    _CASES["ends inside a firing"] = (ragged_scans()[0], small_params("64 offsets"), "firing")
    _CASES["128 stagger"] = (small_sweeps("128 stagger")[0], small_params("128 stagger"), "firing")
    beam = small_params("64 offsets")
    beam.starbeam_filter = 1
    _CASES["64 offsets, beam filter"] = (small_sweeps("64 offsets")[0], beam, "firing")
    no_star = small_params("64 offsets")
    no_star.star_shaped_method = 0
    _CASES["64 offsets, no star search"] = (small_sweeps("64 offsets")[0], no_star, "firing")
    return _CASES


SMALL = {
    "ideal16": (0, 0, 0, 0, 0, 1, 0),
    "ideal16 from 77.7": (0, 0, 0, 0, 0, 1, 1),
    "lifted": (1, 1, 0, 0, 0, 1, 0),
    "on the axis": (0, 0, 0, 1, 1, 2, 1),   # (on no ring any more; its planar range is 0 and its sector 0: a second sector in its firing)
    "interval 1.5": (0, 8, 0, 0, 0, 1, 0),
    "16 x 300": (0, 0, 0, 0, 6, 2, 2),
    "32 x 130": (0, 0, 0, 0, 1, 2, 1),
    "ideal64 x 64": (0, 0, 0, 0, 0, 1, 0),
    "ideal16 rows": (0, 0, 0, 0, 0, 1, 0),
    "ends inside a firing": (0, 0, 0, 0, 101, 4, 4),
    "128 stagger": (0, 0, 0, 0, 64, 4, 4),
    "64 offsets, beam filter": (0, 0, 0, 0, 256, 4, 8),
    "64 offsets, no star search": (0, 0, 0, 0, 0, 0, 0),
}
# (model, setting) -> the four sweeps of tests/gpu_sensor_cases.py's model_batch (the second is the ideal control)
MODELS = {
    ("vlp16", "default"): [(0, 0, 0, 0, 152, 2, 1), (0, 0, 0, 0, 0, 1, 0), (0, 0, 0, 0, 131, 2, 1), (0, 0, 0, 0, 163, 2, 1)],
    ("vlp16", "interval 0.5"): [(0, 0, 0, 0, 152, 2, 1), (0, 0, 0, 0, 0, 1, 0), (0, 0, 0, 0, 131, 2, 1), (0, 0, 0, 0, 163, 2, 1)],
    ("hdl64e", "default"): [(0, 0, 0, 0, 2083, 4, 66), (0, 0, 0, 0, 0, 1, 0), (0, 0, 0, 0, 2083, 4, 66), (0, 0, 0, 0, 2083, 4, 66)],
    ("hdl64e", "interval 0.5"): [(6, 28, 0, 0, 2083, 4, 66), (0, 32, 0, 0, 0, 1, 0), (7, 28, 0, 0, 2083, 4, 66), (7, 28, 0, 0, 2083, 4, 66)],
    ("os64", "default"): [(0, 0, 0, 0, 1024, 4, 32), (0, 0, 0, 0, 0, 1, 0), (0, 0, 0, 0, 1024, 4, 32), (0, 0, 0, 0, 1024, 4, 32)],
    ("os64", "interval 0.5"): [(0, 0, 0, 0, 1024, 4, 32), (0, 32, 0, 0, 0, 1, 0), (0, 0, 0, 0, 1024, 4, 32), (0, 0, 0, 0, 1024, 4, 32)],
    ("os128d", "default"): [(0, 0, 0, 0, 0, 1, 0), (0, 64, 0, 0, 0, 1, 0), (0, 0, 0, 0, 0, 1, 0), (0, 0, 0, 0, 0, 1, 1)],
    ("os128d", "interval 0.5"): [(0, 31, 0, 0, 0, 1, 0), (0, 43, 0, 0, 0, 1, 0), (0, 31, 0, 0, 0, 1, 0), (0, 31, 0, 0, 0, 1, 1)],
}
_BATCH = {}


def model_scans(model):
    if model not in _BATCH:
        _BATCH[model] = real_batch(model) if model in G.REAL else G.model_batch(model)
    return _BATCH[model]


def as_tuple(w):
    return tuple(int(w[k]) for k in WM.FIELDS)


@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_sweeps(name):
    c, p, layout = small_cases()[name]
    assert FS.stages(c, p)[1]["status"] == 0
    assert as_tuple(WM.counters(c, p, layout)) == SMALL[name]
    assert WM.fusable(c, p, layout) == FS.fusable(c, p, layout) == (not any(SMALL[name][:4]))


@pytest.mark.parametrize("model,setting", sorted(MODELS))
def test_the_models_batches(model, setting):
    p, layout = G.params(model, setting), SM.MODELS[model]["layout"]
    got = [as_tuple(WM.counters(c, p, layout)) for c in model_scans(model)]
    assert got == MODELS[(model, setting)]
    assert [WM.fusable(c, p, layout) for c in model_scans(model)] == [FS.fusable(c, p, layout) for c in model_scans(model)]


@pytest.mark.parametrize("model", G.REAL)
def test_every_control_sweep_is_clean_and_the_split_agrees_with_the_predicate(model):
    p, layout = G.params(model, "default"), SM.MODELS[model]["layout"]
    w = WM.counters(model_scans(model)[1], p, layout)
    assert (w["multi_sector_firings"], w["tiles_sectors_fall"]) == (0, 0) and not any(w[k] for k in WM.SHAPE)
    for c in model_scans(model):
        assert WM.fusable(c, p, layout) == FS.fusable(c, p, layout)


def test_a_scan_without_a_result_and_rows_that_do_not_divide_count_nothing():
    a, p16, _ = small_cases()["ideal16"]
    few = tuple(v[:20].copy() for v in a)
    assert FS.stages(few, p16)[1]["status"] != 0 and not any(as_tuple(WM.counters(few, p16)))
    rows = tuple(v[:-1].copy() for v in small_cases()["ideal16 rows"][0])
    assert not any(as_tuple(WM.counters(rows, p16, "rows"))) and not WM.fusable(rows, p16, "rows") and not FS.fusable(rows, p16, "rows")


def test_the_entry_point_is_declared_wrapped_and_exported():
    header = open(os.path.join(ROOT, "include", "urf.h")).read()
    assert re.search(r"\bint\s+urf_front_explain\s*\(\s*urf_ctx\s*\*\s*ctx\s*,\s*int\s+layout\b[^;]*,\s*urf_front_why\s*\*\s*out\b[^;]*,\s*uint32_t\s+n\s*\)\s*;", header)
    assert u.FRONT_WHY_DTYPE.itemsize == 64 and callable(getattr(u.Context, "front_explain", None))
    for table, prefix in ((u.WHY_CALL, "URF_WHY_CALL_"), (u.WHY_SCAN, "URF_WHY_SCAN_"), (u.ADVICE, "URF_ADVICE_")):
        declared = {m.group(1): int(m.group(2), 16) for m in re.finditer(r"#define\s+%s(\w+)\s+(0x[0-9a-fA-F]+)u" % prefix, header)}
        assert declared == table
    lib = u.lib()
    assert lib.urf_front_explain(None, 0, None, 0) == -1   # (no context: URF_ERR_INVALID_ARG, before anything touches a device)
