"""The premise of urf_set_dense_outputs (include/urf.h), on the CPU against oracle B: the padded twin of a dense scan (tests/dense_model.py)
holds the dense points in input order with NaN holes between them, the reference drops the holes before anything else, and its per-ring
quicksort sees only the sequence of the points that remain -- so the orders it publishes on the twin (road, curb, ring 10) are the dense
scan's with every index i replaced by pos[i].  Mapped back through the inverse of pos they must equal the dense scan's element by element:
with the right ids, with uniformly random ids, for a scan that is not aligned (pos[i] = i), and for a grid-snapped cloud whose rings hold
bit-identical azimuths, where the literal quicksort decides the order."""
import numpy as np
import pytest

import dense_model as D
import fuzz
import oracles as O
import sensor_models as SM

ORDERS = ("road_order", "curb_order", "ring10_order")
# model -> (firings, sweep keywords): the sweeps of tests/test_gpu_dense.py
CASES = {
    "ideal64": (256, dict(drop=0.01)),
    "hdl64e": (256, dict(noise=True, drop=0.01, holes=("zero", "nan1", "inf"))),
    "ideal16": (304, dict(drop=0.01)),
    "ideal32": (136, dict(drop=0.01)),
    "vlp16": (304, dict(noise=True, drop=0.10)),
    "ideal128": (128, dict(drop=0.01)),
}
RANDOM_IDS = ("ideal16", "ideal32", "vlp16")   # a firing per two points: W * L = n * L stays below 2^18 for these


def params(model, roi):
    """(ideal128: the ring tolerance of tests/test_gpu_dense.py, which keeps its lasers apart)"""
    return SM.params_for(model, wide=roi == "wide", interval=0.05 if model == "ideal128" else None)


def mapped_back(dense, pos, L, W, p):
    """Oracle B on the padded twin; its three orders through the inverse of pos, its labels at pos, its marker points."""
    pos = np.asarray(pos, np.int64)
    lp, ip, st = O.run_b(*D.pad(dense, pos, L, W), p, debug=True)
    inv = np.full(W * L, -1, np.int64)
    inv[pos] = np.arange(len(pos))
    out = {}
    for key in ORDERS:
        out[key] = inv[st[key].astype(np.int64)]
        assert (out[key] >= 0).all(), key   # (a hole is NaN: the reference never lists one)
    return out, lp[pos], ip, st["marker_pts"]


def check(dense, ids, L, W, p, want_aligned=True, ring10=True):
    ld, idn, sd = O.run_b(*dense, p, debug=True)
    pos, _, aligned = D.realign(ids, L, W)
    assert aligned == want_aligned
    got, labels, ip, markers = mapped_back(dense, pos, L, W, p)
    assert np.array_equal(labels, ld) and ip == idn
    assert np.array_equal(markers.view(np.uint32), sd["marker_pts"].view(np.uint32))
    for key in ORDERS:
        assert np.array_equal(got[key], sd[key].astype(np.int64)), key
    assert len(sd["road_order"]) > 0 and len(sd["curb_order"]) > 0   # (no comparison passes on empty lists)
    assert (len(sd["ring10_order"]) > 0) == ring10
    return sd


@pytest.mark.parametrize("roi", ["wide", "default"])
@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("model", sorted(CASES))
def test_the_orders_of_the_padded_twin_mapped_back_are_the_dense_scans(model, seed, roi):
    F, kw = CASES[model]
    L = SM.lasers(model)
    cloud = SM.sweep(model, firings=F, world=seed % 3, seed=100 + seed, **kw)
    dense, slot = D.densify(cloud, L, SM.missing_mask(cloud))
    p = params(model, roi)
    ring10 = model != "vlp16"   # (fewer than eleven of its rings reach the region of interest)
    check(dense, slot, L, F + 3, p, ring10=ring10)
    if model in RANDOM_IDS:   # any ids whatever: about n / 2 firings
        ids = np.random.default_rng(50 + seed).integers(0, L, len(slot))
        assert D.realign(ids, L, len(ids))[1] > len(ids) // 4
        check(dense, ids, L, len(ids), p, ring10=ring10)


def test_a_scan_that_is_not_aligned_maps_through_the_identity():
    model, L, F = "ideal32", 32, 136
    cloud = SM.sweep(model, firings=F, world=1, seed=101, drop=0.01)
    dense, slot = D.densify(cloud, L, SM.missing_mask(cloud))
    ids = slot.copy()
    ids[len(ids) // 2] = L   # a slot >= L
    pos = D.realign(ids, L, F + 3)[0]
    assert np.array_equal(pos, np.arange(len(ids)))
    check(dense, ids, L, F + 3, params(model, "wide"), want_aligned=False)


@pytest.mark.parametrize("seed", [7006, 7007, 7019])   # (of the first 24: road, curb and ring 10 all listed, hundreds of ties)
def test_equal_azimuths_inside_a_ring_keep_the_quicksorts_order(seed):
    """x / y on a grid (tests/test_gpu_parity.py::test_published_order_and_markers_with_equal_azimuths): many points of a ring share their
    azimuth to the bit, and the order the reference's Lomuto quicksort leaves them in depends on the sequence it is handed alone."""
    rng = np.random.default_rng(seed)
    cloud = fuzz.random_cloud(rng, 3000, tie_grid=0.25)
    p = SM.params_for("ideal16", wide=True)
    p.channels = 16
    n, L = len(cloud[0]), 16
    lb, ib, st = O.run_b(*cloud, p, debug=True)
    az, ring = st["azimuth"], st["ring"]
    ties = sum(len(a) - len(np.unique(a)) for a in (az[ring == r] for r in range(int(ring.max()) + 1)))
    assert ties > 50, ties   # (bit-identical azimuths inside rings)
    ids = rng.integers(0, L, n)
    sd = check(cloud, ids, L, n, p)
    assert len(sd["road_order"]) > 50 and len(sd["curb_order"]) > 50 and len(sd["ring10_order"]) > 50
