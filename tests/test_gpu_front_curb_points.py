"""urf_set_front_mode(ctx, 3): the fused front end (urban_road_filter_amd/csrc/urf_front.hpp) for curbPoints 1..8 at 64 lasers per firing --
k_front_cp1 .. k_front_cp8 and k_front_finish_cp1 .. _cp8, the detectors' window of 2 * curbPoints + 1 heights in registers -- through the C
ABI: labels and summaries against oracle B, exact.  What takes it (firing order and row-major, batches and the callback path, block borders
crossed with and without holes in the halos, rings barely long enough for one window), what must not (curbPoints 9..30, 16 / 32 lasers with
curbPoints != 5, modes 1 and 2 with curbPoints != 5), and that one context follows its parameters from call to call."""
import numpy as np
import pytest

import oracles as O
import urban_road_filter_amd as u
from fuzz_lasers import case as lasers_case
from fuzz_organised import case
from test_gpu_front import fused_batch, ring_major
from test_gpu_parity import check_against_b, run_batch

pytestmark = pytest.mark.gpu
N = 64 * 2048
OTHER = (1, 2, 3, 4, 6, 7, 8)
_SCANS = {}


def scans4():
    """Three one-tile blocks (every block border crossed at one tile per block), four tiles, a sensor-like and a narrow full sweep."""
    if not _SCANS:
        _SCANS["s"] = [u.synth_cloud(64, 96, 1, 7), u.synth_cloud(64, 256, 3, 8), O.cfg_cloud("sensor", 2), O.cfg_cloud("narrow", 1)]
    return _SCANS["s"]


def params(cp, name="cfg2", **tweak):
    p = O.cfg_params(name)
    p.curbPoints = cp
    for k, v in tweak.items():
        setattr(p, k, v)
    return p


def test_mode_three_is_accepted_and_four_is_not():
    with u.Context(64 * 96, 1) as ctx:
        ctx.set_front_mode(3)
        for bad in (4, -1):
            with pytest.raises(u.api.UrfError):
                ctx.set_front_mode(bad)
            assert ctx._lib.urf_set_front_mode(ctx._h, bad) == -1   # URF_ERR_INVALID_ARG
        ctx.set_front_mode(3)   # (still a valid context)


@pytest.mark.parametrize("cp", OTHER)
def test_other_curb_points_take_the_fused_front_end(cp):
    p = params(cp)
    scans = scans4()
    with u.Context(N, len(scans)) as ctx:
        for batch in (scans, scans, scans[::-1]):   # (second call: the row's previous ring count as a hint)
            labels, infos, nf = fused_batch(ctx, batch, p, mode=3, ragged=True)
            assert nf == len(batch)
            check_against_b(labels, infos, batch, p)


def test_five_in_mode_three_is_mode_two():
    p = params(5)
    scans = scans4()
    with u.Context(N, len(scans)) as ctx:
        l3, i3, nf = fused_batch(ctx, scans, p, mode=3, ragged=True)
        assert nf == len(scans)
        check_against_b(l3, i3, scans, p)
        l2, i2, nf = fused_batch(ctx, scans, p, mode=2, ragged=True)
        assert nf == len(scans)
        assert all(np.array_equal(a, b) for a, b in zip(l3, l2)) and np.array_equal(i3, i2)


@pytest.mark.parametrize("cp", (9, 30))
def test_more_than_eight_keeps_the_general_kernels(cp):
    p = params(cp)
    scans = scans4()
    with u.Context(N, len(scans)) as ctx:
        labels, infos, nf = fused_batch(ctx, scans, p, mode=3, ragged=True)
        assert nf == 0
        check_against_b(labels, infos, scans, p)


@pytest.mark.parametrize("L", (32, 16))
def test_fewer_lasers_with_other_curb_points_keep_the_general_kernels(L):
    sw, p = lasers_case(7_400_000 + L, L)
    p.curbPoints = 3
    with u.Context(len(sw[0]), 1) as ctx:
        labels, infos, nf = fused_batch(ctx, [sw], p, mode=3)
        assert nf == 0
        check_against_b(labels, infos, [sw], p)


@pytest.mark.parametrize("mode", (1, 2))
def test_modes_one_and_two_keep_the_general_kernels(mode):
    p = params(3)
    scans = scans4()[:2]
    with u.Context(64 * 256, len(scans)) as ctx:
        labels, infos, nf = fused_batch(ctx, scans, p, mode=mode, ragged=True)
        assert nf == 0
        check_against_b(labels, infos, scans, p)


@pytest.mark.parametrize("tweak", [{"x_zero_method": 0}, {"z_zero_method": 0}, {"star_shaped_method": 0}, {"starbeam_filter": 1}, {"curbHeight": 0.01}],
                         ids=lambda t: "-".join("%s=%s" % kv for kv in t.items()))
@pytest.mark.parametrize("cp", (1, 4, 7))
def test_detector_switches(cp, tweak):
    """(curbHeight 0.01: many candidates, rings with more curb points than their list holds -- the per-degree tables)"""
    p = params(cp, **tweak)
    scans = scans4()
    with u.Context(N, len(scans)) as ctx:
        labels, infos, nf = fused_batch(ctx, scans, p, mode=3, ragged=True)
        assert nf == len(scans)
        check_against_b(labels, infos, scans, p)


@pytest.mark.parametrize("cp", (2, 5, 6, 8))
def test_holes_in_the_halos(cp):
    """Firings 24..40 and 58..70 of some lasers missing: the gaps straddle the tile borders at 32 and 64 -- the halos of one-tile blocks --
    and are wider (17) and narrower (13) than the window of 2 * cp + 1: windows that begin inside a march, decided by k_front_finish."""
    x, y, z = (a.copy().reshape(96, 64) for a in u.synth_cloud(64, 96, 1, 7))
    lanes = [0, 3, 10, 11, 31, 32, 40, 63]
    for a in (x, y, z):
        a[24:41, lanes] = 0.0
        a[58:71, lanes[::2]] = 0.0
    sw = tuple(a.reshape(-1) for a in (x, y, z))
    p = params(cp)
    with u.Context(64 * 96, 2) as ctx:
        labels, infos, nf = fused_batch(ctx, [sw, sw], p, mode=3)
        print("cp %d: fused %d of 2" % (cp, nf))
        check_against_b(labels, infos, [sw, sw], p)


@pytest.mark.parametrize("cp", (1, 3, 5, 8))
def test_rings_barely_long_enough(cp):
    """Lasers that keep exactly 2 cp, 2 cp + 1 and 2 cp + 2 points (no centre, one, two): the detectors' [cp, n - 1 - cp] bounds."""
    x, y, z = (a.copy().reshape(64, 64) for a in u.synth_cloud(64, 64, 1, 9))
    rng = np.random.default_rng(cp)
    for lane, keep in ((5, 2 * cp), (6, 2 * cp + 1), (7, 2 * cp + 2), (20, 2 * cp), (21, 2 * cp + 1), (40, 2 * cp + 2)):
        gone = np.ones(64, bool)
        gone[rng.choice(64, keep, replace=False)] = False
        for a in (x, y, z):
            a[gone, lane] = 0.0
    sw = tuple(a.reshape(-1) for a in (x, y, z))
    p = params(cp)
    with u.Context(64 * 64, 2) as ctx:
        labels, infos, nf = fused_batch(ctx, [sw, sw], p, mode=3)
        print("cp %d: fused %d of 2" % (cp, nf))
        check_against_b(labels, infos, [sw, sw], p)


_FUZZ_NF = {}


@pytest.mark.parametrize("seed", range(40))
def test_organised_sweeps_with_holes(seed):
    """tests/fuzz_organised.py (curbPoints 5, 2 and 9) in mode 3."""
    (x, y, z), p = case(7_300_000 + seed)
    lb, ib, _ = O.run_b(x, y, z, p)
    with u.Context(len(x), 1) as ctx:
        labels, infos, nf = fused_batch(ctx, [(x, y, z)], p, mode=3)
    _FUZZ_NF[seed] = (p.curbPoints, nf)
    assert np.array_equal(labels[0], lb), "%d labels differ (fused %d)" % (int((labels[0] != lb).sum()), nf)
    keys = ("status", "n_roi", "n_rings", "n_ring_pts", "n_road", "n_curb", "n_ring10")
    assert {f: int(v) for f, v in zip(keys, infos[0][:7])} == {f: ib[f] for f in keys}
    assert p.curbPoints <= 8 or nf == 0


def test_some_fuzzed_sweep_with_two_curb_points_was_fused():
    """(a gate that lets none of them through would pass everything above)"""
    for seed in range(40):
        if seed not in _FUZZ_NF:   # (run on its own)
            (x, y, z), p = case(7_300_000 + seed)
            if p.curbPoints != 2:
                continue
            with u.Context(len(x), 1) as ctx:
                _FUZZ_NF[seed] = (2, fused_batch(ctx, [(x, y, z)], p, mode=3)[2])
    twos = [nf for cp, nf in _FUZZ_NF.values() if cp == 2]
    assert twos and max(twos) == 1, _FUZZ_NF


def test_one_context_follows_its_parameters():
    scans = scans4()[2:]
    with u.Context(N, 2) as ctx:
        for cp, want in ((5, 2), (3, 2), (8, 2), (9, 0), (5, 2)):
            p = params(cp)
            labels, infos, nf = fused_batch(ctx, scans, p, mode=3)
            assert nf == want, (cp, nf)
            check_against_b(labels, infos, scans, p)


def test_a_batch_of_520_scans():
    """(four tiles per block of the march)"""
    p = params(3)
    base = [u.synth_cloud(64, 256, 1 + (s % 2) * 2, 50 + s) for s in range(8)]
    many = [base[s % 8] for s in range(520)]
    with u.Context(64 * 256, 520) as ctx:
        ctx.set_front_mode(3)
        labels, infos = run_batch(ctx, many, p)
        assert ctx.front_scans() == 520
        for s in range(520):
            assert np.array_equal(labels[s], labels[s % 8]) and np.array_equal(infos[s], infos[s % 8])
        check_against_b(labels[:8], infos[:8], many[:8], p)


@pytest.mark.parametrize("cp", (3, 8))
def test_row_major_sweeps(cp):
    p = params(cp)
    scans = [ring_major(O.cfg_cloud("cfg2", s)) for s in (1, 2)]
    with u.Context(N, 2) as ctx:
        labels, infos, nf0 = fused_batch(ctx, scans, p, mode=3)   # (the first call sights the layout)
        check_against_b(labels, infos, scans, p)
        labels, infos, nf = fused_batch(ctx, scans, p, mode=3)
        assert nf == 2, (nf0, nf)
        check_against_b(labels, infos, scans, p)


def test_callback_path_follows_set_params():
    """A row-major context in mode 3: urf_set_params starts the captured per-slot sequences afresh, the sweeps that follow take the fused
    kernels with the instance for the new curbPoints (include/urf.h)."""
    p5, p3 = params(5), params(3)
    rows = [ring_major(O.cfg_cloud(name, s)) for name, s in (("cfg2", 1), ("sensor", 2))]
    with u.Context(N, 4, params=p5) as ctx:
        ctx.set_front_mode(3)
        fused = []
        for rep in range(3):
            for c in rows:
                lab, info = ctx.classify_xyz(*c)
                assert np.array_equal(lab, O.run_b(*c, p5)[0]), rep
                fused.append(ctx.front_scans())
        assert fused[0] == 0 and fused[-1] == 1, fused
        ctx.set_params(p3)
        for rep in range(2):
            for c in rows:
                lab, info = ctx.classify_xyz(*c)
                lb, ib, _ = O.run_b(*c, p3)
                assert np.array_equal(lab, lb) and info.n_curb == ib["n_curb"] and info.n_road == ib["n_road"], rep
                assert ctx.front_scans() == 1
        ctx.set_front_mode(2)   # ... and mode 2 hands curbPoints 3 back to the general kernels there too
        lab, info = ctx.classify_xyz(*rows[0])
        assert np.array_equal(lab, O.run_b(*rows[0], p3)[0]) and ctx.front_scans() == 0
