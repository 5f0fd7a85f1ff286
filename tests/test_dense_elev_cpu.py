"""The id rule of urf_classify_batch_*_dense_elev (include/urf.h, tests/dense_ids_model.py) on the sensor models: the ids derived from the
points' elevation ARE the true firing slots, for every point of every sweep, so the re-alignment rule (tests/dense_model.py) puts every
point where the true slots put it.  Plus the rule's edges: ties, a reversed table, non-finite / (0, 0, 0) / on-axis points, and the
monotonicity that lets the kernel search instead of count.  No GPU."""
import numpy as np
import pytest

import dense_ids_model as I
import dense_model as D
import sensor_models as SM

MODELS = ["vlp16", "hdl32e", "vlp32c", "hdl64e", "ideal16", "ideal32", "ideal64", "ideal128"]
FIRINGS = 256
_SWEEP = {}


def elev(model):
    return np.asarray(SM.MODELS[model]["elev"], np.float32)


def dense_sweep(model, noise):
    if (model, noise) not in _SWEEP:
        cloud = SM.sweep(model, firings=FIRINGS, world=1, seed=40 + len(model), noise=noise, drop=0.05)
        _SWEEP[model, noise] = D.densify(cloud, SM.lasers(model), SM.missing_mask(cloud))
    return _SWEEP[model, noise]


@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("model", MODELS)
def test_derived_ids_are_the_true_slots(model, noise):
    dense, slot = dense_sweep(model, noise)
    L = SM.lasers(model)
    assert len(slot) > 3000 and len(np.unique(slot)) == L   # (every laser has returns)
    got = I.ids(elev(model), dense)
    assert np.array_equal(got, slot), "%d of %d ids wrong" % (int((got != slot).sum()), len(slot))
    # far from every midpoint: the smallest half-spacing of the eight tables is 0.09 degrees (ideal128)
    assert I.midpoint_margin_deg(elev(model), dense) > 1e-3
    want, have = D.realign(slot, L, FIRINGS + 3), D.realign(got, L, FIRINGS + 3)
    assert want[2] and have[2] and have[1] == want[1] and np.array_equal(have[0], want[0])


@pytest.mark.parametrize("model", MODELS)
def test_the_products_do_not_decrease(model):
    dense, _ = dense_sweep(model, True)
    assert I.monotone_products(elev(model), dense)
    T, _ = I.table(elev(model))
    assert (np.diff(T) >= 0).all()


def test_thresholds_come_from_double_midpoints():
    e = np.asarray([-15.0, 1.0, -13.0, 3.0], np.float32)
    T, sor = I.table(e)
    assert list(sor) == [0, 2, 1, 3]
    want = [np.float32(np.tan(np.float64(m) * np.pi / 180)) for m in (-14.0, -6.0, 2.0)]
    assert T.dtype == np.float32 and list(T) == want


def test_ties_go_to_the_lower_slot():
    e = [-10.0, -4.0, -10.0, -4.0, 2.0]
    T, sor = I.table(e)
    assert list(sor) == [0, 2, 1, 3, 4]
    assert T[0] == np.float32(np.tan(np.radians(-10.0))) and T[2] == np.float32(np.tan(np.radians(-4.0)))
    # the threshold between two equal elevations is their own tangent: what lies below it takes the lower slot, what lies above the other
    ang = np.radians(np.asarray([-12.0, -9.0, -5.0, -3.0, 1.5]))
    cloud = (np.cos(ang).astype(np.float32) * 10, np.zeros(5, np.float32), np.sin(ang).astype(np.float32) * 10)
    assert list(I.ranks(e, cloud)) == [0, 1, 2, 3, 4]
    assert list(I.ids(e, cloud)) == [0, 2, 1, 3, 4]
    assert I.monotone_products(e, cloud)


def test_all_equal_table_gives_two_slots_at_most():
    e = [-7.0] * 16
    dense, _ = dense_sweep("ideal16", False)
    got = np.unique(I.ids(e, dense))
    assert set(got) <= {0, 15} and I.monotone_products(e, dense)


@pytest.mark.parametrize("model", ["vlp16", "hdl64e", "ideal32"])
def test_a_reversed_table_reverses_the_ids(model):
    dense, slot = dense_sweep(model, False)
    L = SM.lasers(model)
    got = I.ids(elev(model)[::-1].copy(), dense)
    assert np.array_equal(got, L - 1 - slot)


def test_edge_points_get_what_the_compares_give():
    e = elev("vlp16")            # -15 .. 15: thresholds of both signs and one that is 0
    n = len(e)
    T, sor = I.table(e)
    assert (T < 0).any() and (T > 0).any() and (T == 0).any()
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    pts = [((nan, 1, 1), 0), ((1, nan, 1), 0), ((1, 1, nan), 0), ((nan, nan, nan), 0),
           ((0, 0, 0), 0), ((0, 0, -2), 0), ((0, 0, 2), n - 1),               # the origin and the axis
           ((inf, 0, 0), int((T < 0).sum())), ((inf, 0, 5), int((T < 0).sum())),   # h = inf: -inf, then NaN at T == 0, then +inf
           ((1, 1, inf), n - 1), ((1, 1, -inf), 0), ((inf, 1, inf), int((T < 0).sum())),
           ((3, 0, 100), n - 1), ((3, 0, -100), 0)]                            # outside the fan
    cloud = tuple(np.asarray([p[0][k] for p in pts], np.float32) for k in range(3))
    want = [p[1] for p in pts]
    assert list(I.ranks(e, cloud)) == want
    assert list(I.ids(e, cloud)) == [int(sor[r]) for r in want]
    assert I.monotone_products(e, cloud)
    # the compares of every such point are true up to the rank and false behind it: a search finds the count
    with np.errstate(all="ignore"):
        c = cloud[2][:, None] > I.products(T, cloud[0], cloud[1])
    for row, r in zip(c, want):
        assert row[:r].all() and not row[r:].any()
