"""The fused front end for sweeps of 128 lasers per firing (urf_front.hpp: k_front128 and its siblings, behind
urf_set_front_lasers128), in firing order and row-major: labels and summaries against oracle B on the same input -- on sweeps that
take it (wide and default region of interest, lasers in any fixed order, the two halves of a firing swapped, partial last tiles, ragged
batches, 128 tiles), on sweeps that must not take it next to ones that do, with the nine parameter tweaks of
test_gpu_front.test_parameters, with holes (tests/fuzz_lasers128.py), with a ring on table entry 127, as sensor models deliver them, on
the callback path -- and what must not change: the switch off, modes 0 and 1, channels = 64, curbPoints != 5, 129 tiles, the entry
points that read ring-sorted results.

channels = 128 and interval = 0.05 (cfg5's values): under the wide region of interest every urf_synth_cloud(128, cols, scene, seed) used
here has 128 rings for oracle B (asserted: says_something(rings=128)); the reference's default region of interest keeps 122 of them."""
import numpy as np
import pytest

import gpu_sensor_cases as G
import oracles as O
import sensor_models as SM
import urban_road_filter_amd as u
from fuzz_lasers128 import case
from hipmem import DevBuf
from test_gpu_front import fused_batch
from test_gpu_parity import check_against_b

pytestmark = pytest.mark.gpu
L = 128
KEYS = ("status", "n_roi", "n_rings", "n_ring_pts", "n_road", "n_curb", "n_ring10")


def params(wide=True):
    p = u.default_params()
    if wide:
        p = p.wide_roi()
    p.channels = L
    p.interval = 0.05
    return p


def says_something(scans, p, rings=None):
    """Oracle B finds road and curb on every input: no comparison passes on an empty result."""
    for x, y, z in scans:
        _, ib, _ = O.run_b(x, y, z, p)
        assert ib["n_road"] > 0 and ib["n_curb"] > 0, ib
        assert rings is None or ib["n_rings"] == rings, ib


def fused128(ctx, scans, p, mode=2, on=1, ragged=False):
    ctx.set_front_lasers128(on)
    return fused_batch(ctx, scans, p, mode=mode, ragged=ragged)


def permuted(cloud, perm):
    return tuple(np.ascontiguousarray(a.reshape(-1, L)[:, perm].reshape(-1)) for a in cloud)


def rolled(cloud, cols):
    return tuple(np.ascontiguousarray(np.roll(a.reshape(-1, L), cols, axis=0).reshape(-1)) for a in cloud)


def ring_major(cloud):
    """The same sweep stored row by row (row-major 128 x W: an organised cloud)."""
    return tuple(np.ascontiguousarray(a.reshape(-1, L).T.reshape(-1)) for a in cloud)


def firing_scans(cols, wide):
    return [u.synth_cloud(L, cols, scene, 5 + (0 if wide else 1) + scene) for scene in (1, 2, 3, 4)]


# ---- (a) firing order ----
@pytest.mark.parametrize("cols", (2048, 512))
@pytest.mark.parametrize("wide", (True, False))
def test_sweeps_in_firing_order_take_the_fused_front_end(cols, wide):
    p = params(wide)
    scans = firing_scans(cols, wide)
    says_something(scans, p, rings=128 if wide else 122)
    with u.Context(L * cols, len(scans)) as ctx:
        labels, infos, nf = fused128(ctx, scans, p)
        assert nf == len(scans)
        check_against_b(labels, infos, scans, p)
        labels, infos, nf = fused128(ctx, scans[::-1], p)
        assert nf == len(scans)
        check_against_b(labels, infos, scans[::-1], p)


# ---- (b) lasers in any fixed order ----
@pytest.mark.parametrize("order", ("random", "halves swapped"))
def test_lasers_in_any_fixed_order(order):
    """Laser slot l of a firing is one laser, whatever table entry it sits on.  With the halves swapped lasers 64..127 come first: a star
    participant's place among its firing's copies counts the participants of the OTHER half in front of it."""
    p = params()
    perm = np.random.default_rng(5).permutation(L) if order == "random" else np.concatenate([np.arange(64, 128), np.arange(64)])
    scans = [permuted(u.synth_cloud(L, 512, 3, s), perm) for s in (1, 2)] + [permuted(u.synth_cloud(L, 512, 1, 3), perm[::-1].copy())]
    says_something(scans, p, rings=128)
    with u.Context(L * 512, len(scans)) as ctx:
        labels, infos, nf = fused128(ctx, scans, p)
        assert nf == len(scans)
        check_against_b(labels, infos, scans, p)


# ---- (c) parameters ----
@pytest.mark.parametrize("tweak", [{"xDirection": 1}, {"xDirection": 2}, {"starbeam_filter": 1}, {"star_shaped_method": 0},
                                   {"x_zero_method": 0}, {"z_zero_method": 0}, {"blind_spots": 0}, {"curbHeight": 0.01},
                                   {"interval": 0.1, "angleFilter1": 120.0, "angleFilter2": 100.0}])
def test_parameters(tweak):
    p = params()
    for k, v in tweak.items():
        setattr(p, k, v)
    scans = [u.synth_cloud(L, 512, 2, 1), u.synth_cloud(L, 512, 3, 2), u.synth_cloud(L, 512, 1, 3)]
    says_something(scans, p)
    with u.Context(L * 512, len(scans)) as ctx:
        labels, infos, nf = fused128(ctx, scans, p)
        assert nf == len(scans)
        check_against_b(labels, infos, scans, p)


# ---- (d) holes ----
@pytest.mark.parametrize("seed", range(40))
def test_organised_sweeps_with_holes(seed):
    (x, y, z), p = case(7_600_000 + seed)
    lb, ib, _ = O.run_b(x, y, z, p)
    with u.Context(len(x), 1) as ctx:
        labels, infos, nf = fused128(ctx, [(x, y, z)], p)
    assert np.array_equal(labels[0], lb), "%d labels differ (fused %d)" % (int((labels[0] != lb).sum()), nf)
    assert {f: int(v) for f, v in zip(KEYS, infos[0][:7])} == {f: ib[f] for f in KEYS}
    assert p.curbPoints == 5 or nf == 0


def half_empty(cloud):
    """No return (NaN) from lasers 0..63 in firings 2 and 3 of every eight, from lasers 64..127 in firing 6, from any laser in firing 12 of
    every sixteen."""
    f = np.arange(len(cloud[0]) // L)
    out = []
    for a in cloud[:3]:
        v = a.reshape(-1, L).copy()
        v[np.isin(f % 8, (2, 3)), :64] = np.nan
        v[f % 8 == 6, 64:] = np.nan
        v[f % 16 == 12, :] = np.nan
        out.append(np.ascontiguousarray(v.reshape(-1)))
    return tuple(out)


@pytest.mark.parametrize("beam", (0, 1))
@pytest.mark.parametrize("wide", (True, False))
def test_firings_with_an_empty_half(wide, beam):
    """A lane marches two lasers, the halves of a firing, and the star-shaped search's bookkeeping crosses them: the firing's sector is its
    first participant's -- half 0's, or else half 1's -- and a copy's place counts the participants of the half in front.  Firings whose
    first half, second half or both hold no point at all, at 96 columns (six tiles) and 256."""
    p = params(wide)
    p.star_shaped_method = 1
    p.starbeam_filter = beam
    scans = [half_empty(u.synth_cloud(L, cols, scene, seed)) for cols in (96, 256) for scene, seed in ((1, 11), (3, 12))]
    says_something(scans, p, rings=128 if wide else 122)
    with u.Context(L * 256, len(scans)) as ctx:
        labels, infos, nf = fused128(ctx, scans, p, ragged=True)
        print("FUSED empty halves | wide %d beam %d: %d of %d" % (wide, beam, nf, len(scans)))
        check_against_b(labels, infos, scans, p)
        assert nf == len(scans)


# ---- (e) shape ----
@pytest.mark.parametrize("cols", [48, 17, 33, 2047])
def test_partial_last_tile_and_ragged_batches(cols):
    p = params()
    a = u.synth_cloud(L, cols, 1, 7)
    b = u.synth_cloud(L, 512, 3, 8)
    scans = [a, b, tuple(v[:L * 300 + 7].copy() for v in b)]   # (the last one ends inside a firing)
    says_something(scans, p)
    with u.Context(L * 2048, len(scans)) as ctx:
        labels, infos, nf = fused128(ctx, scans, p, ragged=True)
        assert nf >= 2
        check_against_b(labels, infos, scans, p)


def test_scans_without_the_shape_are_handed_back():
    p = params()
    x, y, z = u.synth_cloud(L, 1024, 1, 3)
    pm = np.random.default_rng(1).permutation(len(x))
    scans = [u.synth_cloud(L, 1024, 1, 1), (x[pm], y[pm], z[pm]), u.synth_cloud(L, 1024, 3, 2), rolled(u.synth_cloud(L, 1024, 2, 4), 700)]
    says_something([scans[0], scans[2], scans[3]], p)   # (a shuffled sweep has no road left)
    with u.Context(L * 1024, len(scans)) as ctx:
        for _ in range(3):   # first call: lists; then grids
            labels, infos, nf = fused128(ctx, scans, p)
            assert nf == 2
            check_against_b(labels, infos, scans, p)
        labels, infos, nf = fused128(ctx, scans, p, mode=0)
        assert nf == 0
        check_against_b(labels, infos, scans, p)


# ---- (f) table entry 127 ----
def test_a_ring_on_table_entry_127_is_fused():
    """128 rings: the laser on table entry 127 has a ring like every other (the records of these kernels keep the ring in eight bits,
    0xff is "none") -- in its own slot, and in slot 0 with the lasers reversed."""
    p = params()
    sweep = u.synth_cloud(L, 256, 1, 6)
    scans = [sweep, permuted(sweep, np.arange(L)[::-1].copy())]
    says_something(scans, p, rings=128)
    lb, ib, _ = O.run_b(*sweep, p)
    assert ib["n_ring_pts"] == ib["n_roi"] == len(sweep[0])   # (every point lies on a ring: entry 127 holds a laser's points)
    with u.Context(L * 256, len(scans)) as ctx:
        labels, infos, nf = fused128(ctx, scans, p)
        assert nf == len(scans)
        check_against_b(labels, infos, scans, p)


# ---- (g) 128 and 129 tiles ----
def test_sweeps_of_128_tiles_are_fused_and_of_129_are_not():
    p = params()
    full = [u.synth_cloud(L, 2048, 1, 61), u.synth_cloud(L, 2048, 3, 62)]
    over = [u.synth_cloud(L, 2064, 1, 63), u.synth_cloud(L, 2064, 3, 64)]
    says_something(full[:1] + over[:1], p, rings=128)
    with u.Context(L * 2064, 2) as ctx:
        labels, infos, nf = fused128(ctx, full, p)
        assert nf == 2
        check_against_b(labels, infos, full, p)
        labels, infos, nf = fused128(ctx, over, p)
        assert nf == 0
        check_against_b(labels, infos, over, p)
        labels, infos, nf = fused128(ctx, full, p)   # ... and back
        assert nf == 2
        check_against_b(labels, infos, full, p)


# ---- (h) row-major ----
@pytest.mark.parametrize("cols,wide", [(1024, True), (256, True), (256, False), (17, True), (48, True)])
def test_row_major_clouds_take_the_fused_front_end_from_the_second_call(cols, wide):
    """k_rows_probe128, k_transpose128 and k_label_front128's row-major stores: the first call sights the layout, the second takes it.
    17 columns: two tiles of 16 firings, the second with one -- k_transpose128's partial tile and the store-back of one; 48 columns: three
    tiles, an odd number, the last presence word half used."""
    p = params(wide)
    scans = [ring_major(c) for c in firing_scans(cols, wide)]
    says_something(scans, p)
    with u.Context(L * cols, len(scans)) as ctx:
        labels, infos, nf0 = fused128(ctx, scans, p)
        assert nf0 == 0
        check_against_b(labels, infos, scans, p)
        labels, infos, nf = fused128(ctx, scans, p)
        assert nf == len(scans), (nf0, nf)
        check_against_b(labels, infos, scans, p)
        labels, infos, nf = fused128(ctx, scans[::-1], p)
        assert nf == len(scans)
        check_against_b(labels, infos, scans[::-1], p)
        labels, infos, nf = fused128(ctx, scans, p, mode=0)
        assert nf == 0
        check_against_b(labels, infos, scans, p)


def sensor_params(model, **kw):
    p = G.params(model, "max_Z 2.0", **kw)
    p.interval = 0.05
    return p


@pytest.mark.parametrize("layout", ["firing", "rows"])
def test_ideal128_sweeps_with_nan_and_zero_holes_are_all_fused(layout):
    p = sensor_params("ideal128")
    scans = [SM.sweep("ideal128", firings=256, world=w, seed=40 + w, layout=layout, noise=w == 1, holes=("nan",) if w == 0 else ("zero",))
             for w in (0, 1, 2, 3)]
    says_something(scans, p, rings=128)
    with u.Context(len(scans[0][0]), len(scans)) as ctx:
        labels, infos, nf0 = fused128(ctx, scans, p)
        check_against_b(labels, infos, scans, p)
        labels, infos, nf1 = fused128(ctx, scans, p)
        check_against_b(labels, infos, scans, p)
    assert nf1 == 4 and (layout == "firing" or nf0 == 0), (nf0, nf1)


def test_os128d_sweeps_row_major_with_nan_and_zero_holes():
    """The OS-128 model as its driver publishes it (128 x 1024, row-major, upward lasers): labels either way; how many are fused is printed."""
    p = sensor_params("os128d")
    scans = [SM.sweep("os128d", world=0, seed=31, noise=True, holes=("nan",)), SM.sweep("os128d", world=1, seed=33),
             SM.sweep("os128d", world=2, seed=34, start_deg=77.7, noise=True, holes=SM.HOLES)]
    says_something(scans, p)
    with u.Context(len(scans[0][0]), len(scans)) as ctx:
        counts = []
        for _ in range(2):
            labels, infos, nf = fused128(ctx, scans, p)
            check_against_b(labels, infos, scans, p)
            counts.append(nf)
        labels, infos, nf = fused128(ctx, scans, p, on=0)
        assert nf == 0
        check_against_b(labels, infos, scans, p)
    print("FUSED os128d rows | first call %d, second %d of %d" % (counts[0], counts[1], len(scans)))


def test_row_major_sweeps_on_the_callback_path_four_in_flight():
    """classify_pc2_async of a row-major 128 x 256 context: sighting, then the captured sequences with k_front128; labels and summaries
    of every sweep of every round (how many sweeps took which kernels is not this test's business: urf_front_scans covers batch calls)."""
    p = params()
    scans = [ring_major(u.synth_cloud(L, 256, scene, 20 + scene)) for scene in (1, 2, 3, 4)]
    ref = [O.run_b(*c, p) for c in scans]
    assert all(r[1]["n_road"] > 0 and r[1]["n_curb"] > 0 and r[1]["n_rings"] == 128 for r in ref)
    n = L * 256
    recs = []
    for c in scans:
        r = np.zeros((n, 4), np.float32)
        r[:, 0], r[:, 1], r[:, 2] = c
        recs.append(r)
    with u.Context(n, 4, params=p) as ctx:
        ctx.set_front_lasers128(1)
        ctx.set_front_mode(2)
        for rep in range(4):
            tickets = [ctx.classify_pc2_async(r, n, 16, 0, 4, 8) for r in recs]
            for k, t in enumerate(tickets):
                lab = np.zeros(n, np.uint8)
                info = ctx.classify_pc2_wait(t, lab)
                assert np.array_equal(lab, ref[k][0]), (rep, k)
                assert {f: getattr(info, f) for f in KEYS} == {f: ref[k][1][f] for f in KEYS}, (rep, k)


# ---- (i) what must not change ----
@pytest.mark.parametrize("mode,on", [(2, 0), (3, 0), (0, 1), (1, 1)])
def test_switch_off_or_modes_0_and_1_keep_the_general_kernels(mode, on):
    p = params()
    inputs = [firing_scans(512, True), [permuted(c, np.concatenate([np.arange(64, 128), np.arange(64)])) for c in firing_scans(512, True)],
              [ring_major(c) for c in firing_scans(256, True)]]
    for scans in inputs:
        with u.Context(len(scans[0][0]), len(scans)) as ctx:
            for _ in range(2):   # (row-major: a sighting must not lead anywhere either)
                labels, infos, nf = fused128(ctx, scans, p, mode=mode, on=on)
                assert nf == 0
                check_against_b(labels, infos, scans, p)


def test_what_must_not_change_with_the_switch_on():
    """channels = 64 behaves as before (a 128-laser sweep is handed back, a 64-laser one fused); curbPoints 2 and 9 keep the general
    kernels at 128 lasers; after urf_ordered_indices the context stays on the general kernels; the switch takes 0 and 1 only."""
    sweep = u.synth_cloud(L, 512, 1, 5)
    p64 = params()
    p64.channels = 64
    with u.Context(L * 512, 1) as ctx:
        labels, infos, nf = fused128(ctx, [sweep], p64)
        assert nf == 0
        check_against_b(labels, infos, [sweep], p64)
        for cp in (2, 9):
            p = params()
            p.curbPoints = cp
            labels, infos, nf = fused128(ctx, [sweep], p)
            assert nf == 0
            check_against_b(labels, infos, [sweep], p)
        p = params()
        labels, infos, nf = fused128(ctx, [sweep], p)
        assert nf == 1
        lb, ib, st = O.run_b(*sweep, p, debug=True)
        n = len(sweep[0])
        dx, dy, dz, dl = DevBuf.from_numpy(sweep[0]), DevBuf.from_numpy(sweep[1]), DevBuf.from_numpy(sweep[2]), DevBuf(n)
        ctx.classify_batch_soa(dx, dy, dz, n, 1, dl, None)   # (the call's inputs stay alive for the read-back)
        assert ctx.front_scans() == 1
        road, curb, prob = ctx.ordered_indices(n, scan=0)
        assert np.array_equal(road, st["road_order"]) and np.array_equal(curb, st["curb_order"]) and np.array_equal(prob, st["ring10_order"])
        ctx.classify_batch_soa(dx, dy, dz, n, 1, dl, None)
        assert ctx.front_scans() == 0
        assert np.array_equal(dl.to_numpy(np.uint8), lb)
        for bad in (2, -1):
            with pytest.raises(Exception):
                ctx.set_front_lasers128(bad)
            assert ctx._lib.urf_set_front_lasers128(ctx._h, bad) == -1
        labels, infos, nf = fused128(ctx, [sweep], p)   # (the switch and the mode set again: a new start)
        assert nf == 1
        check_against_b(labels, infos, [sweep], p)
    big = [O.cfg_cloud("cfg2", 1), O.cfg_cloud("sensor", 2)]
    with u.Context(64 * 2048, 2) as ctx:
        labels, infos, nf = fused128(ctx, big, O.cfg_params("cfg2"))
        assert nf == 2
        check_against_b(labels, infos, big, O.cfg_params("cfg2"))
