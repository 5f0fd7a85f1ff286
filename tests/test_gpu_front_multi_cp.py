"""urf_set_front_multi_sector_curb_points(ctx, 1) on top of urf_set_front_multi_sector(ctx, 1): the fused front end keeps scans whose firings
span several star sectors, and scans whose sectors fall inside a tile, at curbPoints 1..4 and 6..8 as well (k_front*_ms_cp<n>, urf_front.hpp;
k_front_sectors behind them).  Always: labels and the seven summary fields equal oracle B, exactly.

An "all fused" assertion is made on one context in three steps, so that a failure points at the new instances and not at the input:
curbPoints 5 with urf_set_front_multi_sector on -- all fused (the input's part); the tested curbPoints with the new switch off -- none fused
(the behaviour without the switch); the new switch on -- all fused.  tests/test_front_multi_cp_cpu.py checks on the CPU that the sweeps used
here have the properties they are used for at every curbPoints.

Front mode 3 throughout; 16 / 32 / 128 lasers with urf_set_front_curb_points on, 128 with urf_set_front_lasers128 on.  Shapes: 64 x 256,
32 x 256, 16 x 512 and 128 x 64 (four to eight tiles); the eight real sensors' batches of tests/gpu_sensor_cases.py."""
import numpy as np
import pytest

import front_shape as FS
import gpu_sensor_cases as G
import oracles as O
import sensor_models as SM
import urban_road_filter_amd as u
from test_front_multi_cpu import batch as real_batch
from test_front_multi_cpu import layout, ragged_scans, seam_sweeps, small_models, small_params, small_sweeps
from test_gpu_batch_clouds import Batch
from test_gpu_front_outputs import batch_readouts, same
from test_gpu_parity import run_batch

pytestmark = pytest.mark.gpu
KEYS = ("status", "n_roi", "n_rings", "n_ring_pts", "n_road", "n_curb", "n_ring10")
NAMES = sorted(small_models())
OTHERS = (1, 2, 3, 4, 6, 7, 8)
CAPACITY = 64 * 2048   # max_points of every context below: a sensor-sized one (the candidate lists do not hand scans back)


def check(labels, infos, scans, p):
    """Labels and summaries against oracle B (computed once per sweep and parameters: front_shape.stages)."""
    for k, c in enumerate(scans):
        lb, ib, _ = FS.stages(c, p)
        assert np.array_equal(labels[k], lb), "scan %d: %d labels differ" % (k, int((labels[k] != lb).sum()))
        assert dict(zip(KEYS, (int(v) for v in infos[k][:7]))) == {f: ib[f] for f in KEYS}, "scan %d" % k
        assert infos[k][7] == 0, "scan %d: NaN azimuths counted" % k


def rows_of(c, L):
    return tuple(np.ascontiguousarray(a.reshape(-1, L).T.reshape(-1)) for a in c)


def at(p, cp):
    q = p.copy()
    q.curbPoints = cp
    return q


def switches(ctx, p):
    """What lets a call with these parameters take the fused kernels at curbPoints 1..8, whatever the two multi-sector switches say."""
    if p.channels == 128:
        ctx.set_front_lasers128(1)
    if p.channels != 64:
        ctx.set_front_curb_points(1)


def context(scans, p, **kw):
    ctx = u.Context(max(CAPACITY, max(len(c[0]) for c in scans)), len(scans), **kw)
    switches(ctx, p)
    return ctx


def call(ctx, scans, p, ms, ms_cp, mode=3, calls=1):
    ctx.set_front_mode(mode)
    ctx.set_front_multi_sector(ms)
    ctx.set_front_multi_sector_curb_points(ms_cp)
    ragged = len({len(c[0]) for c in scans}) > 1
    for _ in range(calls):
        labels, infos = run_batch(ctx, scans, p, ragged=ragged)
    return labels, infos, ctx.front_scans()


def three_steps(scans, p, calls=1):
    """p.curbPoints is the tested value.  The last step: other batch positions, grids instead of lists."""
    assert p.curbPoints in OTHERS
    p5 = at(p, 5)
    with context(scans, p) as ctx:
        labels, infos, nf = call(ctx, scans, p5, 1, 0, calls=calls)
        check(labels, infos, scans, p5)
        assert nf == len(scans), "curbPoints 5: %d of %d fused" % (nf, len(scans))
        labels, infos, nf = call(ctx, scans, p, 1, 0, calls=calls)
        check(labels, infos, scans, p)
        assert nf == 0, "new switch off: %d of %d fused" % (nf, len(scans))
        labels, infos, nf = call(ctx, scans, p, 1, 1, calls=calls)
        check(labels, infos, scans, p)
        assert nf == len(scans), "new switch on: %d of %d fused" % (nf, len(scans))
        labels, infos, nf = call(ctx, scans[::-1], p, 1, 1, calls=calls)
        check(labels, infos, scans[::-1], p)
        assert nf == len(scans), "new switch on, reversed: %d of %d fused" % (nf, len(scans))


# ---- 1. small shapes ----
@pytest.mark.parametrize("cp", OTHERS)
@pytest.mark.parametrize("name", NAMES)
def test_small_sweeps_in_firing_order(name, cp):
    three_steps(small_sweeps(name), at(small_params(name), cp))


@pytest.mark.parametrize("cp", OTHERS)
@pytest.mark.parametrize("name", NAMES)
def test_small_sweeps_row_major(name, cp):
    """(the first call sights the layout: asserted from the second call on)"""
    p = at(small_params(name), cp)
    three_steps([rows_of(c, p.channels) for c in small_sweeps(name)], p, calls=2)


# ---- 2. the seam ----
@pytest.mark.parametrize("cp", (1, 3, 8))
@pytest.mark.parametrize("name", NAMES)
def test_the_seam_inside_a_tile_and_on_its_last_firing(name, cp):
    p = at(small_params(name), cp)
    scans = seam_sweeps(name)
    three_steps(scans, p)
    three_steps([rows_of(c, p.channels) for c in scans], p, calls=2)


# ---- 3. a ragged batch ----
@pytest.mark.parametrize("cp", (3, 8))
def test_ragged_batch(cp):
    """A scan that ends inside a firing and a tile, a tile without a participant, a tile whose 2048 points all take part."""
    three_steps(ragged_scans(), at(small_params("64 offsets"), cp))


# ---- 4. parameters ----
@pytest.mark.parametrize("cp", (2, 7))
@pytest.mark.parametrize("name", NAMES)
def test_the_beam_body(name, cp):
    p = at(small_params(name), cp)
    p.starbeam_filter = 1
    three_steps(small_sweeps(name), p)


@pytest.mark.parametrize("name", NAMES)
def test_without_the_star_shaped_search_sectors_do_not_matter(name):
    """The plain instance is launched and the scans are fused, whatever the switches say."""
    p = at(small_params(name), 3)
    p.star_shaped_method = 0
    scans = small_sweeps(name)
    with context(scans, p) as ctx:
        for ms, ms_cp in ((1, 1), (1, 0), (0, 1), (0, 0)):
            labels, infos, nf = call(ctx, scans, p, ms, ms_cp)
            check(labels, infos, scans, p)
            assert nf == len(scans), (ms, ms_cp)


@pytest.mark.parametrize("name", ("64 offsets", "16 drift"))
def test_what_the_switch_does_not_decide(name):
    """curbPoints 9: never fused.  Front mode 2 with curbPoints 3: never fused.  The new switch on with urf_set_front_multi_sector off: the
    plain instance, which hands these sweeps back."""
    scans = small_sweeps(name)
    p3, p9 = at(small_params(name), 3), at(small_params(name), 9)
    with context(scans, p3) as ctx:
        for what, p, ms, mode in (("curbPoints 9", p9, 1, 3), ("mode 2", p3, 1, 2), ("multi_sector off", p3, 0, 3)):
            labels, infos, nf = call(ctx, scans, p, ms, 1, mode=mode, calls=2)
            check(labels, infos, scans, p)
            assert nf == 0, what
        labels, infos, nf = call(ctx, scans, p3, 1, 1)   # (... and the context has lost nothing over it)
        check(labels, infos, scans, p3)
        assert nf == len(scans)


def test_invalid_arguments():
    with u.Context(4096, 1) as ctx:
        for bad in (2, -1):
            with pytest.raises(u.api.UrfError):
                ctx.set_front_multi_sector_curb_points(bad)
        ctx.set_front_multi_sector_curb_points(1)
        ctx.set_front_multi_sector_curb_points(0)


# ---- 5. one call, three kinds of scans ----
def test_multi_sector_ideal_and_unorganised_scans_in_one_call():
    name = "64 offsets"
    p = at(small_params(name), 3)
    ms = small_sweeps(name)[1]
    ideal = SM.sweep("ideal64", firings=256, world=2, seed=21, holes=("nan",))
    pm = np.random.default_rng(3).permutation(len(ms[0]))
    shuffled = tuple(np.ascontiguousarray(a[pm]) for a in small_sweeps(name)[0])
    scans = [ms, ideal, shuffled]
    with context(scans, p) as ctx:
        for k, batch in enumerate((scans, scans, scans[::-1], scans)):
            labels, infos, nf = call(ctx, batch, p, 1, 1)
            check(labels, infos, batch, p)
            print("call %d: %d of 3 fused" % (k, nf))
            assert nf == 2 or k == 0   # (the first call may still hand a sweep back for its speculative ring table, as without the switch)
        labels, infos, nf = call(ctx, scans, p, 1, 0)
        check(labels, infos, scans, p)
        assert nf == 1   # (the ideal sweep)


# ---- 6. the real sensors' batches ----
@pytest.mark.parametrize("cp", (3, 8))
@pytest.mark.parametrize("model", G.REAL)
def test_real_sensor_batches_are_fused(model, cp):
    """A fresh context with every switch on: the second call fuses every sweep front_shape.fusable accepts -- 4 of 4
    (tests/test_front_multi_cp_cpu.py)."""
    p = at(G.params(model, "default"), cp)
    scans = real_batch(model)
    want = sum(FS.fusable(c, p, layout(model)) for c in scans)
    with context(scans, p) as ctx:
        counts = []
        for _ in range(2):
            labels, infos, nf = call(ctx, scans, p, 1, 1)
            check(labels, infos, scans, p)
            counts.append(nf)
    print("FUSED multi-sector %s / curbPoints %d | first call %d, second %d of %d (fusable: %d)" % (model, cp, counts[0], counts[1], len(scans), want))
    assert counts[1] == want


# ---- 7. the read-outs ----
@pytest.mark.parametrize("outputs", (1, 0))
@pytest.mark.parametrize("name", ("64 offsets", "16 drift"))
def test_read_outs_behind_a_multi_sector_call(name, outputs):
    p = at(small_params(name), 3)
    scans = small_sweeps(name)
    refs = [FS.stages(c, p) for c in scans]
    b = Batch(scans)
    stride = len(scans[0][0])
    with context(scans, p, params=p) as ctx:
        ctx.set_front_mode(3)
        ctx.set_front_multi_sector(1)
        ctx.set_front_multi_sector_curb_points(1)
        ctx.set_front_outputs(outputs)
        labels, infos = b.classify(ctx, "soa")
        assert ctx.front_scans() == len(scans)
        check(labels, infos, scans, p)
        before = b.dl.to_numpy(np.uint8).copy()
        for s, got in enumerate(batch_readouts(ctx, len(scans), stride)):
            same(got, refs[s][2], (name, outputs, s))
        for order in (u.ORDER_REFERENCE, u.ORDER_INPUT):
            b.check_clouds(ctx, "soa", order, p)
        assert np.array_equal(b.dl.to_numpy(np.uint8), before)   # the caller's labels: unchanged
        if outputs:
            assert ctx.front_scans() == len(scans)   # (no second run through the general kernels)


# ---- 8. the callback path ----
def test_callback_path_of_a_row_major_staggered_context():
    name = "64 offsets"
    p = at(small_params(name), 3)
    L = p.channels
    m = small_models()[name]
    rows = [rows_of(c, L) for c in small_sweeps(name)] + [SM.sweep(m, world=2, seed=30 + k, noise=bool(k % 2), start_deg=40.0 * k, layout="rows") for k in range(2)]
    want = [FS.stages(c, p)[:2] for c in rows]
    rec = []
    for c in rows:
        r = np.zeros((len(c[0]), 4), np.float32)
        r[:, 0], r[:, 1], r[:, 2] = c
        rec.append(r)
    seen = []
    with u.Context(CAPACITY, 4, params=p) as ctx:
        ctx.set_front_mode(3)
        ctx.set_front_multi_sector(1)
        for on in (1, 0, 1):
            ctx.set_front_multi_sector_curb_points(on)
            for rep in range(3):
                for c, (lb, ib) in zip(rows, want):
                    lab, info = ctx.classify_xyz(*c)
                    assert np.array_equal(lab, lb) and info.n_road == ib["n_road"] and info.n_curb == ib["n_curb"], (on, rep)
                    seen.append((on, ctx.front_scans()))
            tickets = [ctx.classify_pc2_async(r, len(r), 16, 0, 4, 8) for r in rec]   # four sweeps in flight
            for t, (lb, ib) in zip(tickets, want):
                lab = np.zeros(len(lb), np.uint8)
                info = ctx.classify_pc2_wait(t, lab)
                assert np.array_equal(lab, lb) and info.n_road == ib["n_road"] and info.n_curb == ib["n_curb"], on
    print("callback path, (new switch, fused) per sweep: %s" % seen)
    assert not any(n for on, n in seen if not on)   # (the new switch off: an astride sweep at curbPoints 3 is never a fused one)
    assert any(n for on, n in seen if on)           # (... and on, the path does take the fused kernels)


# ---- 9. fuzz ----
FUZZ_SEEDS = [seed for seed in range(23) if 1 + seed % 8 != 5]   # twenty seeds: curbPoints 1 + seed % 8, the seeds that give 5 left out
_FUZZ_NF = {}


def fuzz_case(L, seed):
    cloud, p, model = SM.fuzz_case(7_600_000 + 1000 * L + seed, L)
    p.curbPoints = 1 + seed % 8
    return cloud, p, model


def fuzz_call(ctx, cloud, p):
    switches(ctx, p)
    return call(ctx, [cloud], p, 1, 1)


@pytest.mark.parametrize("L", (16, 32, 64))
@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_fuzzed_sensor_sweeps(L, seed):
    """A random sensor model, world, encoding mix, start azimuth, region of interest and detector parameters, curbPoints overridden, every
    switch on, two calls."""
    cloud, p, model = fuzz_case(L, seed)
    lb, ib, _ = O.run_b(*cloud, p)
    with u.Context(len(cloud[0]), 1) as ctx:
        for _ in range(2):
            labels, infos, nf = fuzz_call(ctx, cloud, p)
            assert np.array_equal(labels[0], lb), "%s: %d labels differ (fused %d)" % (model, int((labels[0] != lb).sum()), nf)
            assert dict(zip(KEYS, (int(v) for v in infos[0][:7]))) == {f: ib[f] for f in KEYS}
    _FUZZ_NF[(L, seed)] = nf


def test_some_fuzzed_sweep_was_fused():
    """(a gate that lets none of them through would pass everything above)"""
    assert len(FUZZ_SEEDS) == 20
    for L in (16, 32, 64):
        for seed in FUZZ_SEEDS:
            if (L, seed) not in _FUZZ_NF:   # (run on its own)
                cloud, p, _ = fuzz_case(L, seed)
                with u.Context(len(cloud[0]), 1) as ctx:
                    fuzz_call(ctx, cloud, p)
                    _FUZZ_NF[(L, seed)] = fuzz_call(ctx, cloud, p)[2]
            if _FUZZ_NF[(L, seed)]:
                break
        assert any(nf for (l, _), nf in _FUZZ_NF.items() if l == L), L
