"""urf_set_front_curb_points(ctx, 1): front mode 3's instances for curbPoints 1..8 at 16, 32 and 128 lasers per firing (urf_front.hpp:
k_front32_cp*, k_front16_cp*, k_front128_cp*, k_front_finish128_cp*; 128 lasers with urf_set_front_lasers128 on)
through the C ABI: labels and the seven summary fields against oracle B, exact.  What takes them (firing order and row-major, batches
and the callback path, block borders crossed with and without holes in the halos, rings barely long enough for one window, long
sweeps, the read-outs of urf_set_front_outputs, sensor models) and what must not (the switch off, modes 1 and 2, curbPoints 9).
Wherever a test asserts that every scan was fused it first asserts the same for the same scans with curbPoints 5: a failure is then
the new instances' and not the input's.

Shapes: 16 x 304, 32 x 136 and 128 x 96 are three blocks of the march at small batches (one tile per block; 128 lasers: two);
L x 512 where a street is needed."""
import numpy as np
import pytest

import gpu_sensor_cases as G
import oracles as O
import sensor_models as SM
import urban_road_filter_amd as u
from fuzz_lasers import case as lasers_case
from fuzz_lasers128 import case as lasers128_case
from test_gpu_front import fused_batch
from test_gpu_front_outputs import Soa, batch_readouts, same
from test_gpu_parity import check_against_b

pytestmark = pytest.mark.gpu
LASERS = (16, 32, 128)
OTHER = (1, 2, 3, 4, 6, 7, 8)
SMALL = {16: 304, 32: 136, 128: 96}       # columns of the small shape
BORDERS = {16: (128, 256), 32: (64, 128), 128: (32, 64)}   # block borders (firings) of the small shape
KEYS = ("status", "n_roi", "n_rings", "n_ring_pts", "n_road", "n_curb", "n_ring10")
_CLOUD = {}


def cloud(L, cols, scene, seed):
    """urf_synth_cloud, generated once per shape (read-only: whoever changes a sweep copies it first)."""
    key = (L, cols, scene, seed)
    if key not in _CLOUD:
        _CLOUD[key] = u.synth_cloud(L, cols, scene, seed)
    return _CLOUD[key]


def params(L, cp, **tweak):
    p = u.default_params().wide_roi()
    p.channels = L
    if L == 128:
        p.interval = 0.05   # (cfg5's: neighbouring lasers keep rings of their own)
    p.curbPoints = cp
    for k, v in tweak.items():
        setattr(p, k, v)
    return p


def fused(ctx, scans, p, mode=3, on=1, ragged=False):
    """One batch call with the switch in position `on` (128 lasers: urf_set_front_lasers128 on in every case)."""
    if p.channels == 128:
        ctx.set_front_lasers128(1)
    ctx.set_front_curb_points(on)
    return fused_batch(ctx, scans, p, mode=mode, ragged=ragged)


def two_scans(L):
    return [cloud(L, SMALL[L], 1, 7), cloud(L, 512, 3, 8)]


def all_fused_with_five(ctx, scans, p, ragged=False, calls=1):
    """The input's part of "every scan was fused": the same scans, the same context, curbPoints 5."""
    p5 = params(p.channels, 5)
    for f in ("x_zero_method", "z_zero_method", "star_shaped_method", "starbeam_filter", "curbHeight"):
        setattr(p5, f, getattr(p, f))
    for _ in range(calls):
        nf = fused(ctx, scans, p5, ragged=ragged)[2]
    assert nf == len(scans), "curbPoints 5: %d of %d fused" % (nf, len(scans))


def ring_major(c, L):
    return tuple(np.ascontiguousarray(a.reshape(-1, L).T.reshape(-1)) for a in c)


# ---- 1. the switch ----
@pytest.mark.parametrize("L", LASERS)
def test_switch_off_is_today_and_on_takes_the_new_instances(L):
    p = params(L, 3)
    scans = two_scans(L)
    with u.Context(L * 512, len(scans)) as ctx:
        all_fused_with_five(ctx, scans, p, ragged=True)
        l0, i0, nf = fused(ctx, scans, p, on=0, ragged=True)
        assert nf == 0
        check_against_b(l0, i0, scans, p)
        l1, i1, nf = fused(ctx, scans, p, on=1, ragged=True)
        assert nf == len(scans)
        check_against_b(l1, i1, scans, p)
        assert all(np.array_equal(a, b) for a, b in zip(l0, l1)) and np.array_equal(i0, i1)
        for mode in (1, 2):
            labels, infos, nf = fused(ctx, scans, p, mode=mode, ragged=True)
            assert nf == 0, mode
            check_against_b(labels, infos, scans, p)
        p9 = params(L, 9)
        labels, infos, nf = fused(ctx, scans, p9, ragged=True)
        assert nf == 0
        check_against_b(labels, infos, scans, p9)
        for bad in (2, -1):
            with pytest.raises(u.api.UrfError):
                ctx.set_front_curb_points(bad)
            assert ctx._lib.urf_set_front_curb_points(ctx._h, bad) == -1   # URF_ERR_INVALID_ARG
        labels, infos, nf = fused(ctx, scans, p, ragged=True)   # (still a usable context)
        assert nf == len(scans)
        check_against_b(labels, infos, scans, p)


# ---- 2. every instance ----
@pytest.mark.parametrize("L", LASERS)
@pytest.mark.parametrize("cp", OTHER)
def test_every_instance(L, cp):
    p = params(L, cp)
    scans = two_scans(L)
    with u.Context(L * 512, len(scans)) as ctx:
        all_fused_with_five(ctx, scans, p, ragged=True)
        for batch in (scans, scans, scans[::-1]):   # list-driven, then grids, then other batch positions
            labels, infos, nf = fused(ctx, batch, p, ragged=True)
            assert nf == len(batch)
            check_against_b(labels, infos, batch, p)


# ---- 3. detector switches ----
@pytest.mark.parametrize("tweak", [{"x_zero_method": 0}, {"z_zero_method": 0}, {"star_shaped_method": 0}, {"starbeam_filter": 1}, {"curbHeight": 0.01}],
                         ids=lambda t: "-".join("%s=%s" % kv for kv in t.items()))
@pytest.mark.parametrize("cp", (1, 4, 7))
@pytest.mark.parametrize("L", (16, 128))
def test_detector_switches(L, cp, tweak):
    """(curbHeight 0.01: many candidates, rings with more curb points than their list holds -- the per-degree tables)"""
    p = params(L, cp, **tweak)
    scans = two_scans(L)
    with u.Context(L * 512, len(scans)) as ctx:
        all_fused_with_five(ctx, scans, p, ragged=True)
        labels, infos, nf = fused(ctx, scans, p, ragged=True)
        assert nf == len(scans)
        check_against_b(labels, infos, scans, p)


# ---- 4. holes in the halos ----
@pytest.mark.parametrize("L", LASERS)
@pytest.mark.parametrize("cp", (2, 5, 6, 8))
def test_holes_in_the_halos(L, cp):
    """Some lasers lose all firings of two runs that straddle the block borders of the small shape -- 17 firings (as wide as the widest
    window, 2 * 8 + 1) around the first, 13 (wider than the windows of 2 and 6, narrower than that of 8) around the second: windows that
    begin inside a march, decided by the finish step.  128 lasers: both lasers of a lane, j and j + 64, among them."""
    cols, (b1, b2) = SMALL[L], BORDERS[L]
    x, y, z = (a.copy().reshape(cols, L) for a in cloud(L, cols, 1, 7))
    lanes = {16: [0, 3, 10, 11, 15], 32: [0, 3, 10, 11, 16, 31], 128: [0, 3, 10, 11, 31, 32, 40, 63, 64, 67, 74, 127]}[L]
    for a in (x, y, z):
        a[b1 - 8:b1 + 9, lanes] = 0.0
        a[b2 - 6:b2 + 7, lanes[::2] if L != 128 else [0, 64, 10, 74, 31, 40]] = 0.0
    sw = tuple(a.reshape(-1) for a in (x, y, z))
    p = params(L, cp)
    with u.Context(L * cols, 2) as ctx:
        labels, infos, nf = fused(ctx, [sw, sw], p)
        print("L %d cp %d: fused %d of 2" % (L, cp, nf))
        check_against_b(labels, infos, [sw, sw], p)


# ---- 5. rings barely long enough ----
@pytest.mark.parametrize("L", LASERS)
@pytest.mark.parametrize("cp", (1, 3, 5, 8))
def test_rings_barely_long_enough(L, cp):
    """Lasers that keep exactly 2 cp, 2 cp + 1 and 2 cp + 2 points (no centre, one, two): the detectors' [cp, n - 1 - cp] bounds."""
    cols = SMALL[L]
    x, y, z = (a.copy().reshape(cols, L) for a in cloud(L, cols, 1, 9))
    rng = np.random.default_rng(cp)
    slots = {16: (2, 3, 4, 9, 10, 13), 32: (5, 6, 7, 20, 21, 30), 128: (5, 6, 7, 69, 70, 127)}[L]
    for lane, keep in zip(slots, (2 * cp, 2 * cp + 1, 2 * cp + 2, 2 * cp, 2 * cp + 1, 2 * cp + 2)):
        gone = np.ones(cols, bool)
        gone[rng.choice(cols, keep, replace=False)] = False
        for a in (x, y, z):
            a[gone, lane] = 0.0
    sw = tuple(a.reshape(-1) for a in (x, y, z))
    p = params(L, cp)
    with u.Context(L * cols, 2) as ctx:
        labels, infos, nf = fused(ctx, [sw, sw], p)
        print("L %d cp %d: fused %d of 2" % (L, cp, nf))
        check_against_b(labels, infos, [sw, sw], p)


# ---- 6. fuzz ----
FUZZ_BASE = 7_700_000
_FUZZ_NF = {}


def fuzz_case(L, seed):
    sw, p = lasers128_case(FUZZ_BASE + seed) if L == 128 else lasers_case(FUZZ_BASE + seed, L)
    p.curbPoints = 1 + seed % 8
    return sw, p


@pytest.mark.parametrize("L", LASERS)
@pytest.mark.parametrize("seed", range(30))
def test_organised_sweeps_with_holes(L, seed):
    """tests/fuzz_lasers.py / tests/fuzz_lasers128.py with curbPoints 1 + seed % 8: labels and summaries whatever was fused."""
    (x, y, z), p = fuzz_case(L, seed)
    lb, ib, _ = O.run_b(x, y, z, p)
    with u.Context(len(x), 1) as ctx:
        labels, infos, nf = fused(ctx, [(x, y, z)], p)
    _FUZZ_NF[(L, seed)] = (p.curbPoints, nf)
    assert np.array_equal(labels[0], lb), "%d labels differ (fused %d)" % (int((labels[0] != lb).sum()), nf)
    assert {f: int(v) for f, v in zip(KEYS, infos[0][:7])} == {f: ib[f] for f in KEYS}


@pytest.mark.parametrize("L", LASERS)
def test_some_fuzzed_sweep_with_other_curb_points_was_fused(L):
    """(a gate that lets none of them through would pass everything above)"""
    for seed in range(30):
        if (L, seed) not in _FUZZ_NF:   # (run on its own)
            (x, y, z), p = fuzz_case(L, seed)
            if p.curbPoints == 5:
                continue
            with u.Context(len(x), 1) as ctx:
                _FUZZ_NF[(L, seed)] = (p.curbPoints, fused(ctx, [(x, y, z)], p)[2])
            if _FUZZ_NF[(L, seed)][1] == 1:
                break
    others = [nf for (l, _), (cp, nf) in _FUZZ_NF.items() if l == L and cp != 5]
    assert others and max(others) == 1, {k: v for k, v in _FUZZ_NF.items() if k[0] == L}


# ---- 7. a mixed batch ----
def test_mixed_batch():
    """Two organised sweeps, a shuffled one and one rolled by 700 firings (its seam inside a tile): the same scans are fused as with
    curbPoints 5, call after call (lists first, then grids)."""
    L = 32
    x, y, z = cloud(L, 1024, 1, 3)
    pm = np.random.default_rng(1).permutation(len(x))
    roll = tuple(np.ascontiguousarray(np.roll(a.reshape(-1, L), 700, axis=0).reshape(-1)) for a in cloud(L, 1024, 2, 4))
    scans = [cloud(L, 1024, 1, 1), (x[pm], y[pm], z[pm]), cloud(L, 1024, 3, 2), roll]
    p = params(L, 3)
    with u.Context(L * 1024, len(scans)) as ctx:
        want = fused(ctx, scans, params(L, 5))[2]
        assert want >= 2
    with u.Context(L * 1024, len(scans)) as ctx:
        for _ in range(3):
            labels, infos, nf = fused(ctx, scans, p)
            assert nf == want
            check_against_b(labels, infos, scans, p)


# ---- 8. row-major ----
@pytest.mark.parametrize("L", LASERS)
@pytest.mark.parametrize("cp", (3, 8))
def test_row_major_sweeps(L, cp):
    p = params(L, cp)
    scans = [ring_major(cloud(L, 512, scene, 20 + scene), L) for scene in (1, 3)]
    with u.Context(L * 512, 2) as ctx:
        all_fused_with_five(ctx, scans, p, calls=2)   # (the first call sights the layout)
    with u.Context(L * 512, 2) as ctx:
        labels, infos, nf0 = fused(ctx, scans, p)
        check_against_b(labels, infos, scans, p)
        labels, infos, nf = fused(ctx, scans, p)
        assert nf == 2, (nf0, nf)
        check_against_b(labels, infos, scans, p)


def test_callback_path_follows_set_params():
    """A row-major 32-laser context in mode 3 with the switch on: urf_set_params starts the captured per-slot sequences afresh, the
    sweeps that follow take the fused kernels with the instance for the new curbPoints."""
    L = 32
    p5, p3 = params(L, 5), params(L, 3)
    rows = [ring_major(cloud(L, 1024, scene, 30 + scene), L) for scene in (1, 3)]
    with u.Context(L * 1024, 4, params=p5) as ctx:
        ctx.set_front_mode(3)
        ctx.set_front_curb_points(1)
        seen = []
        for rep in range(3):
            for c in rows:
                lab, info = ctx.classify_xyz(*c)
                assert np.array_equal(lab, O.run_b(*c, p5)[0]), rep
                seen.append(ctx.front_scans())
        assert seen[0] == 0 and seen[-1] == 1, seen
        ctx.set_params(p3)
        for rep in range(2):
            for c in rows:
                lab, info = ctx.classify_xyz(*c)
                lb, ib, _ = O.run_b(*c, p3)
                assert np.array_equal(lab, lb) and info.n_curb == ib["n_curb"] and info.n_road == ib["n_road"], rep
                assert ctx.front_scans() == 1
        ctx.set_front_curb_points(0)   # ... and without the switch curbPoints 3 is the general kernels' there too
        lab, info = ctx.classify_xyz(*rows[0])
        assert np.array_equal(lab, O.run_b(*rows[0], p3)[0]) and ctx.front_scans() == 0


# ---- 9. neighbours ----
def test_a_long_sweep_of_sixteen_lasers():
    """129 tiles of 2048 points (urf_set_front_long_sweeps): the finish step with the LDS that many tiles need, curbPoints 3."""
    L, cols = 16, 129 * 2048 // 16
    sw = cloud(L, cols, 1, 41)
    p = params(L, 3)
    with u.Context(L * cols, 1) as ctx:
        ctx.set_front_long_sweeps(1)
        all_fused_with_five(ctx, [sw], p)
        labels, infos, nf = fused(ctx, [sw], p)
        assert nf == 1
        check_against_b(labels, infos, [sw], p)


def test_read_outs_of_a_fused_call():
    """urf_set_front_outputs at 128 lasers, curbPoints 3: the published order and the marker points straight from the fused call."""
    L = 128
    p = params(L, 3)
    scans = [cloud(L, 512, 1, 5), cloud(L, 512, 3, 6)]
    refs = [O.run_b(*c, p, debug=True) for c in scans]
    assert all(r[1]["status"] == 0 and r[1]["n_road"] > 0 and r[1]["n_curb"] > 0 for r in refs)
    b = Soa(scans)
    with u.Context(L * 512, 2, params=p) as ctx:
        ctx.set_front_lasers128(1)
        ctx.set_front_curb_points(1)
        ctx.set_front_mode(3)
        ctx.set_front_outputs(1)
        b.classify(ctx)
        assert ctx.front_scans() == 2
        assert all(np.array_equal(lab, r[0]) for lab, r in zip(b.labels(), refs))
        for s, got in enumerate(batch_readouts(ctx, 2, L * 512)):
            same(got, refs[s][2], ("128 lasers, curbPoints 3", s))
        assert ctx.front_scans() == 2   # (no second run through the general kernels)


@pytest.mark.parametrize("model", ["vlp16", "hdl32e", "os128d"])
def test_sensor_model_sweeps(model):
    """One sweep of a sensor's model as its driver delivers it (os128d: row-major, fused from the second call on if at all), curbPoints 3:
    labels and summaries; how many calls were fused is printed."""
    p = G.params(model, "max_Z 2.0")
    if SM.lasers(model) == 128:
        p.interval = 0.05
    p.curbPoints = 3
    sw = SM.sweep(model, world=1, seed=33)
    with u.Context(len(sw[0]), 1) as ctx:
        counts = []
        for _ in range(2):
            labels, infos, nf = fused(ctx, [sw], p)
            check_against_b(labels, infos, [sw], p)
            counts.append(nf)
    print("FUSED %s curbPoints 3 | first call %d, second %d of 1" % (model, counts[0], counts[1]))
