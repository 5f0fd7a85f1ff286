"""urf_set_front_multi_sector(ctx, 1): the fused front end keeps scans whose firings span several star sectors and scans whose sectors
fall inside a tile (k_front*_ms, urf_front.hpp; k_front_sectors, urf_k_front_sectors.hpp).  Always: labels and the seven summary fields
equal oracle B.  Where a test asserts that every scan was fused with the switch on, it asserts on the same context that none is with
the switch off: the count is the new kernels' doing.  tests/test_front_multi_cpu.py checks on the CPU that the sweeps used here have
the properties they are used for (firings in several sectors, a seam inside a tile, road and curb in oracle B).

Shapes: 64 x 256, 32 x 256, 16 x 512 and 128 x 64 (four to eight tiles, two to four blocks of the march at small batches); the eight
real sensors' batches of tests/gpu_sensor_cases.py for the counts of DESIGN.md section 4."""
import numpy as np
import pytest

import front_shape as FS
import fuzz_history as H
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


def check(labels, infos, scans, p):
    """Labels and summaries against oracle B (computed once per sweep and parameters: front_shape.stages)."""
    for k, c in enumerate(scans):
        lb, ib, _ = FS.stages(c, p)
        assert np.array_equal(labels[k], lb), "scan %d: %d labels differ" % (k, int((labels[k] != lb).sum()))
        assert dict(zip(KEYS, (int(v) for v in infos[k][:7]))) == {f: ib[f] for f in KEYS}, "scan %d" % k
        assert infos[k][7] == 0, "scan %d: NaN azimuths counted" % k


def rows_of(c, L):
    return tuple(np.ascontiguousarray(a.reshape(-1, L).T.reshape(-1)) for a in c)


CAPACITY = 64 * 2048   # max_points of every context below: a sensor-sized one


def context(scans, p):
    """(The candidate lists of the march hold max(max_points / 8, 4096) entries per scan, and a list that overflows hands its scan back,
    with or without the switch.  A street with cars, walls and poles at 64 lasers passes more than 4096 points however short the sweep is:
    a context sized for the 64 x 256 sweeps alone hands them back for that, the plain kernel -- star-shaped search off -- as well.)"""
    ctx = u.Context(max(CAPACITY, max(len(c[0]) for c in scans)), len(scans))
    if p.channels == 128:
        ctx.set_front_lasers128(1)
    return ctx


def call(ctx, scans, p, on, mode=2, calls=1):
    ctx.set_front_mode(mode)
    ctx.set_front_multi_sector(on)
    ragged = len({len(c[0]) for c in scans}) > 1
    for _ in range(calls):
        labels, infos = run_batch(ctx, scans, p, ragged=ragged)
    return labels, infos, ctx.front_scans()


def on_all_off_none(scans, p, calls=1):
    """Every scan fused with the switch on, none with it off, on one context; equal to oracle B either way."""
    with context(scans, p) as ctx:
        labels, infos, nf = call(ctx, scans, p, 1, calls=calls)
        check(labels, infos, scans, p)
        assert nf == len(scans), "switch on: %d of %d fused" % (nf, len(scans))
        labels, infos, nf = call(ctx, scans, p, 0, calls=calls)
        check(labels, infos, scans, p)
        assert nf == 0, "switch off: %d of %d fused" % (nf, len(scans))
        labels, infos, nf = call(ctx, scans[::-1], p, 1, calls=calls)   # (other batch positions; grids instead of lists)
        check(labels, infos, scans[::-1], p)
        assert nf == len(scans)


# ---- 1. small shapes ----
@pytest.mark.parametrize("name", NAMES)
def test_small_sweeps_in_firing_order(name):
    on_all_off_none(small_sweeps(name), small_params(name))


@pytest.mark.parametrize("name", NAMES)
def test_small_sweeps_row_major(name):
    """(the first call sights the layout: asserted from the second call on)"""
    p = small_params(name)
    on_all_off_none([rows_of(c, p.channels) for c in small_sweeps(name)], p, calls=2)


@pytest.mark.parametrize("L", (16, 32))
@pytest.mark.parametrize("rows", (False, True))
def test_the_astride_entries_of_the_call_histories(L, rows):
    """tests/fuzz_history.py: 16 x 300 and 32 x 130 sweeps of urf_synth_cloud with a firing on a whole degree, astride a sector border."""
    E = H.pool("small")
    scans = [E["%s%ds%d" % ("ar" if rows else "a", L, s)].cloud for s in (1, 2, 3, 4)]
    p = H.make_params(L, True, 5, H.VARIANTS[0])
    on_all_off_none(scans, p, calls=2 if rows else 1)


# ---- 2. the seam ----
@pytest.mark.parametrize("name", NAMES)
def test_the_seam_inside_a_tile_and_on_its_last_firing(name):
    p = small_params(name)
    scans = seam_sweeps(name)
    on_all_off_none(scans, p)
    on_all_off_none([rows_of(c, p.channels) for c in scans], p, calls=2)


# ---- 3. a ragged batch ----
def test_ragged_batch():
    """A scan that ends inside a firing and a tile, a tile without a participant, a tile whose 2048 points all take part."""
    on_all_off_none(ragged_scans(), small_params("64 offsets"))


# ---- 4. parameters ----
@pytest.mark.parametrize("name", NAMES)
def test_the_beam_body(name):
    p = small_params(name)
    p.starbeam_filter = 1
    on_all_off_none(small_sweeps(name), p)


@pytest.mark.parametrize("name", NAMES)
def test_without_the_star_shaped_search_sectors_do_not_matter(name):
    """The plain kernel is launched and the scans are fused, whatever the switch says."""
    p = small_params(name)
    p.star_shaped_method = 0
    scans = small_sweeps(name)
    with context(scans, p) as ctx:
        for on in (1, 0):
            labels, infos, nf = call(ctx, scans, p, on)
            check(labels, infos, scans, p)
            assert nf == len(scans), on


def test_other_curb_points_keep_the_plain_instances():
    """curbPoints 3 in mode 3: the plain instance, which hands astride sweeps back as documented."""
    name = "64 offsets"
    p = small_params(name)
    p.curbPoints = 3
    scans = small_sweeps(name)
    with context(scans, p) as ctx:
        labels, infos, nf = call(ctx, scans, p, 1, mode=3)
        check(labels, infos, scans, p)
        assert nf == 0
        p5 = small_params(name)
        labels, infos, nf = call(ctx, scans, p5, 1, mode=3)   # (... and 5 in mode 3 takes the new ones)
        check(labels, infos, scans, p5)
        assert nf == len(scans)


def test_invalid_arguments():
    with u.Context(4096, 1) as ctx:
        for bad in (2, -1):
            with pytest.raises(u.api.UrfError):
                ctx.set_front_multi_sector(bad)
        ctx.set_front_multi_sector(1)
        ctx.set_front_multi_sector(0)


# ---- 5. one call, three kinds of scans ----
def test_multi_sector_ideal_and_unorganised_scans_in_one_call():
    name = "64 offsets"
    p = small_params(name)
    ms = small_sweeps(name)[1]
    ideal = SM.sweep("ideal64", firings=256, world=2, seed=21, holes=("nan",))
    pm = np.random.default_rng(3).permutation(len(ms[0]))
    shuffled = tuple(np.ascontiguousarray(a[pm]) for a in small_sweeps(name)[0])
    scans = [ms, ideal, shuffled]
    with context(scans, p) as ctx:
        for k, batch in enumerate((scans, scans, scans[::-1], scans)):
            labels, infos, nf = call(ctx, batch, p, 1)
            check(labels, infos, batch, p)
            print("call %d: %d of 3 fused" % (k, nf))
            assert nf == 2 or k == 0   # (the first call may still hand a sweep back for its speculative ring table, as without the switch)
        labels, infos, nf = call(ctx, scans, p, 0)
        check(labels, infos, scans, p)
        assert nf == 1   # (the ideal sweep)


# ---- 6. the real sensors' batches ----
@pytest.mark.parametrize("setting", ["default", "max_Z 0.5", "max_Z 2.0"])
@pytest.mark.parametrize("model", G.REAL)
def test_real_sensor_batches_are_fused(model, setting):
    """A fresh context in mode 2 with the switch on: the second call fuses every sweep front_shape.fusable accepts -- 4 of 4
    (tests/test_front_multi_cpu.py)."""
    p = G.params(model, setting)
    scans = real_batch(model)
    want = sum(FS.fusable(c, p, layout(model)) for c in scans)
    with context(scans, p) as ctx:
        counts = []
        for _ in range(2):
            labels, infos, nf = call(ctx, scans, p, 1)
            check(labels, infos, scans, p)
            counts.append(nf)
    print("FUSED multi-sector %s / %s | first call %d, second %d of %d (fusable: %d)" % (model, setting, counts[0], counts[1], len(scans), want))
    assert counts[1] == want


@pytest.mark.parametrize("model", G.REAL)
def test_real_sensor_batches_with_merged_rings(model):
    """interval 0.5: neighbouring lasers of some models share a ring; such sweeps stay handed back.  Equality and a repeatable count."""
    p = G.params(model, "interval 0.5")
    scans = real_batch(model)
    with context(scans, p) as ctx:
        counts = []
        for _ in range(3):
            labels, infos, nf = call(ctx, scans, p, 1)
            check(labels, infos, scans, p)
            counts.append(nf)
    print("FUSED multi-sector %s / interval 0.5 | calls %s of %d" % (model, counts, len(scans)))
    assert counts[1] == counts[2]


# ---- 7. the read-outs ----
@pytest.mark.parametrize("outputs", (1, 0))
@pytest.mark.parametrize("name", ("64 offsets", "16 drift"))
def test_read_outs_behind_a_multi_sector_call(name, outputs):
    p = small_params(name)
    scans = small_sweeps(name)
    refs = [FS.stages(c, p) for c in scans]
    b = Batch(scans)
    stride = len(scans[0][0])
    with u.Context(CAPACITY, len(scans), params=p) as ctx:
        ctx.set_front_mode(2)
        ctx.set_front_multi_sector(1)
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
    p = small_params(name)
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
        ctx.set_front_mode(2)
        for on in (1, 0, 1):
            ctx.set_front_multi_sector(on)
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
    print("callback path, (switch, fused) per sweep: %s" % seen)
    assert not any(n for on, n in seen if not on)   # (the switch off: an astride sweep is never a fused one)


# ---- 9. fuzz ----
_FUZZ_NF = {}


@pytest.mark.parametrize("L", (16, 32, 64))
@pytest.mark.parametrize("seed", range(40))
def test_fuzzed_sensor_sweeps(L, seed):
    """A random sensor model, world, encoding mix, start azimuth, region of interest and detector parameters, switch on, two calls."""
    cloud, p, model = SM.fuzz_case(7_600_000 + 1000 * L + seed, L)
    lb, ib, _ = O.run_b(*cloud, p)
    with u.Context(len(cloud[0]), 1) as ctx:
        for _ in range(2):
            labels, infos, nf = call(ctx, [cloud], p, 1)
            assert np.array_equal(labels[0], lb), "%s: %d labels differ (fused %d)" % (model, int((labels[0] != lb).sum()), nf)
            assert dict(zip(KEYS, (int(v) for v in infos[0][:7]))) == {f: ib[f] for f in KEYS}
    _FUZZ_NF[(L, seed)] = nf


def test_some_fuzzed_sweep_was_fused():
    """(a gate that lets none of them through would pass everything above)"""
    for L in (16, 32, 64):
        for seed in range(40):
            if (L, seed) not in _FUZZ_NF:   # (run on its own)
                cloud, p, _ = SM.fuzz_case(7_600_000 + 1000 * L + seed, L)
                with u.Context(len(cloud[0]), 1) as ctx:
                    _FUZZ_NF[(L, seed)] = call(ctx, [cloud], p, 1, calls=2)[2]
            if _FUZZ_NF[(L, seed)]:
                break
        assert any(nf for (l, _), nf in _FUZZ_NF.items() if l == L), L
