"""tests/sensor_models.py on the CPU: the generator does what it says (layout, pinned bytes, hole encodings, upward lasers that
hit the walls), oracle B equals the reference's own sources (oracle A, shared libm) on one sweep per model and layout -- NaN holes
in organised order, upward lasers, neighbouring lasers on one ring, staggered firings -- and B finds road and curb on every sweep the GPU tests
(tests/test_gpu_sensor_models.py) use."""
import hashlib

import numpy as np
import pytest

import oracles as O
import sensor_models as SM

ALL_HOLES = SM.HOLES


def sha(cloud):
    return hashlib.sha256(b"".join(np.ascontiguousarray(a, np.float32).tobytes() for a in cloud)).hexdigest()


# ---- the generator ----
@pytest.mark.parametrize("model", sorted(SM.MODELS))
def test_layout_point_f_L_plus_l_is_slot_l(model):
    """Firing order: point f * L + l is slot l (its elevation is the model's); rows: point l * F + f."""
    m, L, F = SM.MODELS[model], SM.lasers(model), 128
    x, y, z = SM.sweep(model, firings=F, world=3 if max(m["elev"]) < 0 else 0, seed=2, drop=0.0)
    ok = ~SM.missing_mask((x, y, z))
    assert ok.sum() > F * L // 4
    with np.errstate(invalid="ignore", divide="ignore"):
        tan_e = z.astype(np.float64) / np.sqrt(x.astype(np.float64) ** 2 + y.astype(np.float64) ** 2)
    slot = (np.arange(F * L) % L) if m["layout"] == "firing" else (np.arange(F * L) // F)
    se, ce = SM.det_sincos(np.asarray(m["elev"]) * SM.DEG)
    want = (se / ce)[slot]
    assert np.allclose(tan_e[ok], want[ok], rtol=0, atol=2e-6)
    # the other layout is the same sweep transposed
    other = SM.sweep(model, firings=F, world=3 if max(m["elev"]) < 0 else 0, seed=2, drop=0.0, layout="rows" if m["layout"] == "firing" else "firing")
    a = x.reshape(F, L) if m["layout"] == "firing" else x.reshape(L, F).T
    b = other[0].reshape(L, F).T if m["layout"] == "firing" else other[0].reshape(F, L)
    assert np.array_equal(a, b, equal_nan=True)


def test_det_sincos():
    a = np.linspace(-50.0, 50.0, 20001)
    s, c = SM.det_sincos(a)
    assert np.abs(s - np.sin(a)).max() < 1e-14 and np.abs(c - np.cos(a)).max() < 1e-14


PINS = {
    ("vlp16", 1808): "ea2b1a219f34feeeff09dff90daf6b200840a4f976aea5dcf8f5f1e4b017672b",
    ("vlp32c", 512): "f1cfea62555c008511beddb9798a817ae925ab9f2599d607990e136678373f0b",
}


@pytest.mark.parametrize("model,firings", sorted(PINS))
def test_generated_bytes_are_pinned(model, firings):
    """A cloud that drifts (another numpy, an edit of the generator) fails here: oracle A's records are keyed by the input's bytes."""
    c = SM.sweep(model, firings=firings, world=1, seed=11, start_deg=33.3, noise=True, drop=0.02, holes=ALL_HOLES)
    assert sha(c) == PINS[(model, firings)]


@pytest.mark.parametrize("hole", ALL_HOLES)
def test_hole_encodings_appear_where_asked_for(hole):
    zero = SM.sweep("hdl32e", firings=256, seed=4, drop=0.05, holes=("zero",))
    x, y, z = SM.sweep("hdl32e", firings=256, seed=4, drop=0.05, holes=(hole,))
    miss = (zero[0] == 0) & (zero[1] == 0) & (zero[2] == 0)
    assert 0.05 * len(x) < miss.sum() < 0.6 * len(x)
    assert all(np.array_equal(a[~miss], b[~miss]) for a, b in zip((x, y, z), zero))   # the returns are the same sweep's
    nn = np.isnan(x).astype(int) + np.isnan(y) + np.isnan(z)
    if hole == "zero":
        assert np.array_equal(SM.missing_mask((x, y, z)), miss) and not np.isnan(x).any()
    elif hole == "nan":
        assert (nn[miss] == 3).all() and (nn[~miss] == 0).all()
    elif hole == "nan1":
        assert (nn[miss] == 1).all() and (nn[~miss] == 0).all()
        assert all(np.isnan(a[miss]).sum() > miss.sum() // 6 for a in (x, y, z))   # each field in turn
    elif hole == "inf":
        assert np.isposinf(x[miss]).all() and not np.isinf(x[~miss]).any() and nn.sum() == 0
    else:
        assert (x[miss] == np.float32(SM.FAR[0])).all() and np.isfinite(np.concatenate([x, y, z])).all()
    assert np.array_equal(SM.missing_mask((x, y, z)), miss)


def test_a_mixed_sweep_holds_every_encoding():
    x, y, z = SM.sweep("vlp16", firings=512, seed=5, drop=0.05, holes=ALL_HOLES)
    nn = np.isnan(x).astype(int) + np.isnan(y) + np.isnan(z)
    assert (nn == 3).any() and (nn == 1).any() and np.isposinf(x).any() and (x == np.float32(SM.FAR[0])).any()
    assert ((x == 0) & (y == 0) & (z == 0)).any()


def test_upward_lasers_of_vlp16_return_wall_points():
    x, y, z = SM.sweep("vlp16", world=0, seed=1)
    L = 16
    up = np.arange(len(x)) % L % 2 == 1
    ok = ~SM.missing_mask((x, y, z))
    assert (z[up & ok] > 0).all() and (up & ok).sum() > 3000
    assert (np.abs(np.abs(y[up & ok]) - 9.0) < 0.01).mean() > 0.9          # ... on the walls (a few on the tall box and the poles)
    # The reference measures a point with z >= 0 from the horizon up (asin + 90, lidar_segmentation.cpp:159-165) and one below from the
    # nadir (acos): the laser at +e and the one at -e do NOT share a ring -- every slot has its own, the upper ones above 90 degrees.
    p = SM.params_for("vlp16", max_Z=2.0)
    _, ib, st = O.run_b(x, y, z, p, debug=True)
    ring, slot = st["ring"], np.arange(len(x)) % L
    assert ib["n_rings"] == 16
    rings_of = [set(ring[(slot == l) & (ring >= 0)].tolist()) for l in range(L)]
    assert all(len(r) == 1 for r in rings_of) and len(set.union(*rings_of)) == 16
    assert all(st["angle_table"][next(iter(rings_of[l]))] > 90.0 for l in range(1, L, 2))
    assert all(st["angle_table"][next(iter(rings_of[l]))] < 90.0 for l in range(0, L, 2))


def test_neighbouring_lasers_of_vlp32c_share_rings_at_wider_intervals():
    """0.333 degrees apart near the horizon: two slots on one ring (what urf_front_open hands back) once the interval lets them merge."""
    x, y, z = SM.sweep("vlp32c", world=0, seed=1)
    slot = np.arange(len(x)) % 32
    shared = {}
    for iv in (0.18, 0.5, 1.5):
        _, ib, st = O.run_b(x, y, z, SM.params_for("vlp32c", max_Z=2.0, interval=iv), debug=True)
        owners = {}
        for l in range(32):
            for r in set(st["ring"][(slot == l) & (st["ring"] >= 0)].tolist()):
                owners.setdefault(r, set()).add(l)
        shared[iv] = sum(len(v) > 1 for v in owners.values())
        assert ib["n_rings"] == len(owners)
    assert shared[0.18] == 0 and 0 < shared[0.5] and shared[1.5] > 0, shared


def test_no_azimuth_just_below_zero_and_no_point_on_the_axis():
    for model in ("vlp16", "hdl64e", "os64"):
        x, y, z = SM.sweep(model, seed=9, start_deg=359.99)
        assert not ((x > 0) & (y < 0) & (-y < 6e-7 * x)).any()
        assert not ((x == 0) & (y == 0) & ~SM.missing_mask((x, y, z))).any()


# ---- oracle B == oracle A (the reference's sources, shared libm) ----
A_MODELS = ("hdl32e", "hdl64e", "ideal16", "ideal32", "ideal64", "os128d", "os32", "os32d", "os64", "os64d", "vlp16", "vlp32c")
A_CASES = [(m, s) for m in A_MODELS for s in (0, 1)]


def a_case(model, setting):
    """One small sweep per model in its own layout; setting 0: every encoding mixed, max_Z 2.0 (the upward lasers enter); 1: NaN holes, sensor-like
    ranges (ties), interval 0.5 (neighbouring lasers merge), started at 123.4 degrees."""
    k = A_MODELS.index(model)
    F = 512 if SM.MODELS[model]["layout"] == "rows" else 300
    if SM.lasers(model) == 128:
        F = 256
    if setting == 0:
        return SM.sweep(model, firings=F, world=k % 3, seed=100 + k, drop=0.03, holes=ALL_HOLES), SM.params_for(model, max_Z=2.0)
    return (SM.sweep(model, firings=F, world=(k + 1) % 3, seed=200 + k, start_deg=123.4, noise=True, drop=0.02, holes=("nan",)),
            SM.params_for(model, interval=0.5))


@pytest.mark.parametrize("model,setting", A_CASES)
def test_oracle_b_equals_reference_on_sensor_model_sweeps(model, setting):
    (x, y, z), p = a_case(model, setting)
    la, ia, _, _ = O.run_a([(x, y, z)], p, libm=True)
    lb, ib, st = O.run_b(x, y, z, p, debug=True)
    assert ib["status"] == 0 == ia[0]["status"] and ib["n_road"] > 0 and ib["n_curb"] > 0, ib
    assert np.array_equal(la[0], lb & O.MASK_NO_RING), "%d labels differ" % int((la[0] != (lb & O.MASK_NO_RING)).sum())
    for key in ("n_roi", "n_road", "n_curb", "n_ring10"):
        assert ia[0][key] == ib[key], key
    for key in ("road_order", "curb_order", "ring10_order"):
        assert np.array_equal(ia[0][key], st[key]), key


# ---- every sweep of the GPU tests says something ----
def test_oracle_b_finds_road_and_curb_on_every_gpu_case():
    import gpu_sensor_cases as G
    n = 0
    for name, scans, p in G.all_cpu_checkable_cases():
        for k, c in enumerate(scans):
            _, ib, _ = O.run_b(*c, p)
            assert ib["status"] == 0 and ib["n_road"] > 0 and ib["n_curb"] > 0, (name, k, ib)
            n += 1
    assert n > 100
