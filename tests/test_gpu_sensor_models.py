"""Sweeps as real LiDAR drivers deliver them (tests/sensor_models.py) through the batch entry points, bit for bit against oracle B on
the same input: labels and the seven summary fields.  Upward lasers (rings above 90 degrees once max_Z lets them in), uneven laser
spacing with interval 0.18 / 0.5 / 1.5, azimuth offsets per laser (a firing in several star sectors: handed back, same labels),
non-returns written as NaN / one NaN field / +Inf / a far point, sweeps of 127 + a bit, 128 and 129 tiles, obstacles.

How many sweeps take the fused front end (urf_front_scans) is asserted only where include/urf.h states it: ideal sweeps whose seam
falls on a tile border (all -- from a context's second call on, and where every laser keeps a ring of its own: see
test_ideal_sweeps_are_all_fused), more than 128 tiles, channels other than 16 / 32 / 64, curbPoints != 5 (none).  Everywhere else the
count is printed ("Real sensor geometries", holds the table measured on an MI355X) and has to be the same on a repeated
identical call."""
import numpy as np
import pytest

import gpu_sensor_cases as G
import oracles as O
import sensor_models as SM
import urban_road_filter_amd as u
from hipmem import DevBuf
from test_gpu_batch_clouds import Batch
from test_gpu_front import fused_batch
from test_gpu_parity import check_against_b

pytestmark = pytest.mark.gpu
KEYS = ("status", "n_roi", "n_rings", "n_ring_pts", "n_road", "n_curb", "n_ring10")


def says_something(scans, p):
    for x, y, z in scans:
        _, ib, _ = O.run_b(x, y, z, p)
        assert ib["status"] == 0 and ib["n_road"] > 0 and ib["n_curb"] > 0, ib


def same(labels, infos, labels0, infos0):
    assert all(np.array_equal(a, b) for a, b in zip(labels, labels0)) and np.array_equal(infos, infos0)


def three_calls(ctx, scans, p, ragged=False):
    """Mode 2 twice (the second call: row-major sighting, table_upto hints), then mode 0 on the same context; every call against B.
    Returns the fused counts of the two mode-2 calls."""
    labels0, infos0, nf0 = fused_batch(ctx, scans, p, ragged=ragged)
    check_against_b(labels0, infos0, scans, p)
    labels, infos, nf1 = fused_batch(ctx, scans, p, ragged=ragged)
    same(labels, infos, labels0, infos0)
    labels, infos, nf = fused_batch(ctx, scans, p, mode=0, ragged=ragged)
    assert nf == 0
    same(labels, infos, labels0, infos0)
    return nf0, nf1


def repeatable(scans, p, counts, ragged=False):
    """The repeat rule: an identical sequence of calls on a new context fuses the same sweeps."""
    with u.Context(max(len(s[0]) for s in scans), len(scans)) as ctx:
        again = tuple(fused_batch(ctx, scans, p, ragged=ragged)[2] for _ in counts)
    assert again == tuple(counts), (again, counts)


@pytest.mark.parametrize("setting", list(G.SETTINGS))
@pytest.mark.parametrize("model", G.REAL)
def test_every_model_in_its_own_layout_next_to_the_ideal_control(model, setting):
    p = G.params(model, setting)
    scans = G.model_batch(model)
    with u.Context(len(scans[0][0]), len(scans)) as ctx:
        counts = three_calls(ctx, scans, p)
    print("FUSED %s | %s | %s | first call %d, second %d of %d" % (model, SM.MODELS[model]["layout"], setting, counts[0], counts[1], len(scans)))
    repeatable(scans, p, counts)


@pytest.mark.parametrize("setting", ["default", "max_Z 2.0", "interval 0.5"])
def test_a_128_laser_model_takes_the_general_kernels(setting):
    p = G.params("os128d", setting)
    assert p.channels == 128
    scans = G.model_batch("os128d")
    with u.Context(len(scans[0][0]), len(scans)) as ctx:
        assert three_calls(ctx, scans, p) == (0, 0)


@pytest.mark.parametrize("setting", ["default", "max_Z 2.0", "interval 0.5"])
@pytest.mark.parametrize("layout", ["firing", "rows"])
@pytest.mark.parametrize("L", [16, 32, 64])
def test_ideal_sweeps_are_all_fused(L, layout, setting):
    """The control: downward lasers, one azimuth per firing, the seam on a tile border -- in worlds with cars, walls and poles, with NaN holes."""
    p = G.params("ideal%d" % L, setting)
    scans = G.ideal_batch(L, layout)
    says_something(scans, p)
    with u.Context(len(scans[0][0]), len(scans)) as ctx:
        nf0, nf1 = three_calls(ctx, scans, p)
    print("FUSED ideal%d | %s | %s | first call %d, second %d of 4" % (L, layout, setting, nf0, nf1))
    # "the lasers of a firing in one fixed order": a lane per laser presumes a ring per laser.  Where the interval merges neighbouring
    # lasers into one ring (64 lasers 0.36 degrees apart, interval 0.5) two lanes share a ring and the sweep is handed back.
    if all(O.run_b(*c, p)[1]["n_rings"] == L for c in scans):
        # (the first call of a context may still hand a sweep back whose speculative ring table was incomplete -- it repairs the table and
        # stops speculating: tests/test_gpu_front.py::test_rear_stored_default_roi_sweeps_repair_their_ring_table; the second call has them all)
        assert nf1 == 4 and (layout == "firing" or nf0 == 0)
        # max_Z 2.0 keeps every return of these worlds: all rings show up within the first firings, the speculative table is complete
        if layout == "firing" and setting == "max_Z 2.0":
            assert nf0 == 4


@pytest.mark.parametrize("L", [16, 32, 64])
def test_what_urf_h_excludes_is_not_fused(L):
    """channels other than 16 / 32 / 64, curbPoints != 5."""
    scans = G.ideal_batch(L, "firing")[:2]
    with u.Context(len(scans[0][0]), len(scans)) as ctx:
        for ch, cp in ((L, 2), (L, 9), (L + 4, 5), (128, 5)):
            p = G.params("ideal%d" % L, "max_Z 0.5", channels=ch)
            p.curbPoints = cp
            labels, infos, nf = fused_batch(ctx, scans, p)
            assert nf == 0, (ch, cp)
            check_against_b(labels, infos, scans, p)
        p = G.params("ideal%d" % L, "max_Z 0.5")
        labels, infos, nf = fused_batch(ctx, scans, p)
        assert nf == 2
        check_against_b(labels, infos, scans, p)


# ---- non-return encodings ----
@pytest.mark.parametrize("holes", G.ENCODINGS, ids=lambda h: h if isinstance(h, str) else "mixed")
@pytest.mark.parametrize("model,layout", G.ENCODING_MODELS)
def test_every_non_return_encoding(model, layout, holes):
    """The same sweeps with (0, 0, 0) holes and with another encoding: both drop the same points, so the labels are the same, equal to B's,
    and as many sweeps are fused -- a NaN hole must not cost the fused path."""
    p = G.params(model, "max_Z 2.0")
    pairs = [G.encoding_pair(model, layout, holes, w) for w in (0, 1)]
    zero, enc = [a for a, _ in pairs], [b for _, b in pairs]
    for a, b in pairs:
        assert np.array_equal(SM.missing_mask(a), SM.missing_mask(b))
    says_something(enc, p)
    res = []
    for scans in (zero, enc):
        with u.Context(len(scans[0][0]), len(scans)) as ctx:
            labels0, infos0, nf0 = fused_batch(ctx, scans, p)
            check_against_b(labels0, infos0, scans, p)
            labels, infos, nf1 = fused_batch(ctx, scans, p)
            same(labels, infos, labels0, infos0)
            res.append((labels0, infos0, (nf0, nf1)))
    same(res[1][0], res[1][1], res[0][0], res[0][1])
    assert res[1][2] == res[0][2], "fused sweeps with (0, 0, 0) holes %s, with %s: %s" % (res[0][2], holes, res[1][2])
    if model.startswith("ideal"):
        assert res[1][2][1] == 2


@pytest.mark.parametrize("model,layout", [("vlp16", "firing"), ("ideal64", "firing"), ("os64d", "rows")])
def test_nan_holes_through_the_pointcloud2_batch_entry(model, layout):
    p = G.params(model, "max_Z 2.0")
    scans = [G.encoding_pair(model, layout, h, w)[1] for h, w in (("nan", 0), ("nan1", 1), (SM.HOLES, 0))]
    b = Batch(scans)
    with u.Context(len(scans[0][0]), len(scans), params=p) as ctx:
        ctx.set_front_mode(2)
        for _ in range(2):
            labels, infos = b.classify(ctx, "pc2")
            check_against_b(labels, infos, scans, p)
        if model == "ideal64":
            assert ctx.front_scans() == len(scans)


@pytest.mark.parametrize("model,layout", [("vlp16", "firing"), ("ideal64", "rows"), ("os64d", "rows")])
def test_nan_holes_on_the_callback_path(model, layout):
    """classify_xyz, then four sweeps in flight."""
    p = G.params(model, "max_Z 2.0")
    scans = [G.encoding_pair(model, layout, h, w)[1] for h, w in (("nan", 0), ("nan1", 1), (SM.HOLES, 0), ("nan", 1))]
    ref = [O.run_b(*c, p) for c in scans]
    n = len(scans[0][0])
    with u.Context(n, 4, params=p) as ctx:
        ctx.set_front_mode(2)
        for rep in range(3):
            for k, c in enumerate(scans):
                lab, info = ctx.classify_xyz(*c)
                assert np.array_equal(lab, ref[k][0]), (rep, k)
                assert {f: getattr(info, f) for f in KEYS} == {f: ref[k][1][f] for f in KEYS}, (rep, k)
        recs = []
        for c in scans:
            r = np.zeros((n, 4), np.float32)
            r[:, 0], r[:, 1], r[:, 2] = c
            recs.append(r)
        for rep in range(2):
            tickets = [ctx.classify_pc2_async(r, n, 16, 0, 4, 8) for r in recs]
            for k, t in enumerate(tickets):
                lab = np.zeros(n, np.uint8)
                info = ctx.classify_pc2_wait(t, lab)
                assert np.array_equal(lab, ref[k][0]), (rep, k)
                assert {f: getattr(info, f) for f in KEYS} == {f: ref[k][1][f] for f in KEYS}, (rep, k)


# ---- long sweeps ----
@pytest.mark.parametrize("L", [16, 32, 64])
def test_sweeps_of_128_tiles_are_fused_and_of_129_are_not(L):
    p = G.params("ideal%d" % L)
    full = [G.long_sweep(L, G.MAX_TILES, seed=61), G.long_sweep(L, G.MAX_TILES, seed=62, holes=("zero",))]
    over = [G.long_sweep(L, G.MAX_TILES + 1, seed=63), G.long_sweep(L, G.MAX_TILES + 1, seed=64, holes=("zero",))]
    says_something(full[:1] + over[:1], p)
    with u.Context(len(over[0][0]), 2) as ctx:
        labels, infos, nf = fused_batch(ctx, full, p)
        assert nf == 2
        check_against_b(labels, infos, full, p)
        labels, infos, nf = fused_batch(ctx, over, p)
        assert nf == 0
        check_against_b(labels, infos, over, p)
        labels, infos, nf = fused_batch(ctx, full, p)   # ... and back
        assert nf == 2
        check_against_b(labels, infos, full, p)


@pytest.mark.parametrize("L", [16, 32, 64])
def test_long_sweeps_in_ragged_batches(L):
    """127 tiles and a partial one that ends inside a firing, 128 tiles and a short sweep in one ragged batch; then 129 tiles next to the
    short one: the call's longest scan decides, nothing is fused."""
    p = G.params("ideal%d" % L)
    scans = G.long_ragged_batch(L)
    short = scans[1]
    assert len(scans[0][0]) % L != 0 and len(scans[2][0]) == G.MAX_TILES * G.TILE
    says_something(scans, p)
    with u.Context((G.MAX_TILES + 1) * G.TILE, 3) as ctx:
        labels, infos, nf = fused_batch(ctx, scans, p, ragged=True)
        check_against_b(labels, infos, scans, p)
        labels1, infos1, nf1 = fused_batch(ctx, scans, p, ragged=True)
        same(labels1, infos1, labels, infos)
        assert nf1 == nf
        print("FUSED long ragged L=%d: %d of 3" % (L, nf))
        over = [G.long_sweep(L, G.MAX_TILES + 1, seed=68), short]
        labels, infos, nf = fused_batch(ctx, over, p, ragged=True)
        assert nf == 0
        check_against_b(labels, infos, over, p)


@pytest.mark.parametrize("model,firings", [("vlp16", 3616), ("hdl32e", 4340)])
@pytest.mark.parametrize("setting", ["default", "max_Z 2.0"])
def test_sweeps_at_five_hertz(model, firings, setting):
    p = G.params(model, setting)
    scans = G.five_hertz_batch(model, firings)
    says_something(scans, p)
    with u.Context(len(scans[0][0]), len(scans)) as ctx:
        counts = three_calls(ctx, scans, p)
    print("FUSED %s %d firings | %s | %s of 3" % (model, firings, setting, counts))
    repeatable(scans, p, counts)


# ---- one chain through the outputs ----
def test_published_clouds_and_marker_chain_on_vlp16_sweeps_with_nan_holes():
    """classify_batch_soa -> urf_clouds_batch_soa in both orders -> marker_points_batch -> marker_strips_batch against oracle B's chain."""
    import marker_sets as M
    from test_gpu_marker_strips import STRIDE_P, assert_equal_oracle, oracle_chain, unpack
    p, mp = G.params("vlp16", "max_Z 0.5"), M.marker_params(1, 1)
    scans = G.chain_batch()
    says_something(scans, p)
    S = len(scans)
    want_b, g_b, status = oracle_chain(scans, p, mp)
    assert any(w for w in want_b)
    b = Batch(scans)
    with u.Context(len(scans[0][0]), S, params=p) as ctx:
        ctx.set_front_mode(2)
        labels, infos = b.classify(ctx, "soa")
        check_against_b(labels, infos, scans, p)
        b.check_clouds(ctx, "soa", u.ORDER_INPUT, p)
        b.check_clouds(ctx, "soa", u.ORDER_REFERENCE, p)
        assert all(np.array_equal(a, c) for a, c in zip(labels, b.labels()))
        ctx.set_front_mode(2)
        labels, infos = b.classify(ctx, "soa")
        d_ghost = DevBuf.from_numpy(np.zeros(1, np.int32))
        d_pts, d_cnt = DevBuf(S * STRIDE_P * 4), DevBuf(S * 4)
        d_strips, d_xyz, d_n = DevBuf(S * u.MARKER_MAX_STRIPS * 32), DevBuf(S * u.MARKER_MAX_STRIP_POINTS * 12), DevBuf(S * 12)
        ctx.marker_points_batch(d_pts, d_cnt)
        ctx.marker_strips_batch(mp, d_pts, d_cnt, S, 1, d_ghost, d_strips, d_xyz, d_n)
        ctx.synchronize()
        assert [int(v) for v in infos[:, 0].astype(np.int32)] == status
        assert_equal_oracle(unpack(d_strips, d_xyz, d_n, S), want_b, "vlp16, NaN holes")
        assert int(d_ghost.to_numpy(np.int32)[0]) == g_b[-1]


# ---- fuzz ----
@pytest.mark.parametrize("L", [16, 32, 64])
@pytest.mark.parametrize("seed", range(40))
def test_random_models_worlds_encodings_and_parameters(L, seed):
    (x, y, z), p, model = SM.fuzz_case(7_500_000 + 1000 * L + seed, L)
    lb, ib, _ = O.run_b(x, y, z, p)
    with u.Context(len(x), 1) as ctx:
        for call in range(2):   # (row-major: sighted by the first call)
            labels, infos, nf = fused_batch(ctx, [(x, y, z)], p)
            assert np.array_equal(labels[0], lb), "%s, call %d: %d labels differ (fused %d)" % (model, call, int((labels[0] != lb).sum()), nf)
            assert {f: int(v) for f, v in zip(KEYS, infos[0][:7])} == {f: ib[f] for f in KEYS}, (model, call)
            assert p.curbPoints == 5 or nf == 0
