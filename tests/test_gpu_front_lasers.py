"""The fused front end for sweeps of 32 and 16 lasers per firing, in firing order (urf_front.hpp: k_front32 / k_front16,
params.channels = L): labels and summaries against oracle B on the same input -- on sweeps that take it (analytic and
sensor-like, wide and default region of interest, lasers in any fixed order, partial last tiles, ragged batches), on sweeps that
must not take it next to ones that do, with the nine parameter tweaks of test_gpu_front.test_parameters, with holes
(tests/fuzz_lasers.py), as a full-size batch -- and what must not change: channels = 64 keeps its meaning, curbPoints != 5 keeps the general kernels,
row-major L x W clouds are sighted by a context's first call and take the fused kernels from the second on, the entry points
that read ring-sorted results run the call again."""
import numpy as np
import pytest

import oracles as O
import urban_road_filter_amd as u
from fuzz_lasers import case
from hipmem import DevBuf
from test_gpu_front import fused_batch
from test_gpu_parity import check_against_b, run_batch

pytestmark = pytest.mark.gpu
LASERS = (32, 16)


def params(L, wide=True):
    p = u.default_params()
    if wide:
        p = p.wide_roi()
    p.channels = L
    return p


def says_something(scans, p):
    """Oracle B finds road and curb on every input: no comparison passes on an empty result."""
    for x, y, z in scans:
        _, ib, _ = O.run_b(x, y, z, p)
        assert ib["n_road"] > 0 and ib["n_curb"] > 0, ib


def permuted(cloud, perm, L):
    return tuple(np.ascontiguousarray(a.reshape(-1, L)[:, perm].reshape(-1)) for a in cloud)


def rolled(cloud, cols, L):
    return tuple(np.ascontiguousarray(np.roll(a.reshape(-1, L), cols, axis=0).reshape(-1)) for a in cloud)


@pytest.mark.parametrize("L", LASERS)
@pytest.mark.parametrize("cols", (2048, 1024))
@pytest.mark.parametrize("wide", (True, False))
def test_sweeps_in_firing_order_take_the_fused_front_end(L, cols, wide):
    p = params(L, wide)
    scans = [u.synth_cloud(L, cols, scene, 5 + (0 if wide else 1) + scene) for scene in (1, 2, 3, 4)]
    says_something(scans, p)
    with u.Context(L * cols, len(scans)) as ctx:
        labels, infos, nf = fused_batch(ctx, scans, p)
        assert nf == len(scans)
        check_against_b(labels, infos, scans, p)
        labels, infos, nf = fused_batch(ctx, scans[::-1], p)
        assert nf == len(scans)
        check_against_b(labels, infos, scans[::-1], p)


@pytest.mark.parametrize("L", LASERS)
def test_lasers_in_any_fixed_order(L):
    p = params(L)
    perm = np.random.default_rng(5).permutation(L)
    scans = [permuted(u.synth_cloud(L, 2048, 3, s), perm, L) for s in (1, 2)] + [permuted(u.synth_cloud(L, 2048, 1, 3), perm[::-1].copy(), L)]
    says_something(scans, p)
    with u.Context(L * 2048, len(scans)) as ctx:
        labels, infos, nf = fused_batch(ctx, scans, p)
        assert nf == len(scans)
        check_against_b(labels, infos, scans, p)


@pytest.mark.parametrize("L", LASERS)
@pytest.mark.parametrize("tweak", [{"xDirection": 1}, {"xDirection": 2}, {"starbeam_filter": 1}, {"star_shaped_method": 0},
                                   {"x_zero_method": 0}, {"z_zero_method": 0}, {"blind_spots": 0}, {"curbHeight": 0.01},
                                   {"interval": 0.1, "angleFilter1": 120.0, "angleFilter2": 100.0}])
def test_parameters(L, tweak):
    p = params(L)
    for k, v in tweak.items():
        setattr(p, k, v)
    scans = [u.synth_cloud(L, 2048, 2, 1), u.synth_cloud(L, 2048, 3, 2), u.synth_cloud(L, 2048, 1, 3)]
    says_something(scans, p)
    with u.Context(L * 2048, len(scans)) as ctx:
        labels, infos, nf = fused_batch(ctx, scans, p)
        assert nf == len(scans)
        check_against_b(labels, infos, scans, p)


@pytest.mark.parametrize("L", LASERS)
def test_scans_without_the_shape_are_handed_back(L):
    p = params(L)
    x, y, z = u.synth_cloud(L, 2048, 1, 3)
    pm = np.random.default_rng(1).permutation(len(x))
    scans = [u.synth_cloud(L, 2048, 1, 1), (x[pm], y[pm], z[pm]), u.synth_cloud(L, 2048, 3, 2), rolled(u.synth_cloud(L, 2048, 2, 4), 700, L)]
    says_something([scans[0], scans[2], scans[3]], p)   # (a shuffled sweep has no road left)
    with u.Context(L * 2048, len(scans)) as ctx:
        for _ in range(3):   # first call: lists; then grids
            labels, infos, nf = fused_batch(ctx, scans, p)
            assert nf == 2
            check_against_b(labels, infos, scans, p)
        labels, infos, nf = fused_batch(ctx, scans, p, mode=0)
        assert nf == 0
        check_against_b(labels, infos, scans, p)


@pytest.mark.parametrize("L", LASERS)
@pytest.mark.parametrize("cols", [96, 40, 33, 2047])
def test_partial_last_tile_and_ragged_batches(L, cols):
    p = params(L)
    a = u.synth_cloud(L, cols, 1, 7)
    b = u.synth_cloud(L, 512, 3, 8)
    scans = [a, b, tuple(v[:L * 300 + 7].copy() for v in b)]   # (the last one ends inside a firing)
    says_something(scans, p)   # (B on the wedges of 40 / 33 firings: 414 / 359 road, 189 / 119 curb with 32 lasers; 403 / 514, 20 / 4 with 16)
    with u.Context(L * 2048, len(scans)) as ctx:
        labels, infos, nf = fused_batch(ctx, scans, p, ragged=True)
        assert nf >= 2
        check_against_b(labels, infos, scans, p)


@pytest.mark.parametrize("L", LASERS)
def test_what_must_not_change(L):
    """channels = 64 keeps its meaning (an L-laser sweep is handed back, a 64-laser one fused); a 64-laser sweep classified with
    channels = L equals B whichever kernels run; curbPoints != 5 keeps the general kernels."""
    sweep = u.synth_cloud(L, 2048, 1, 5)
    p64 = params(64)
    with u.Context(L * 2048, 1) as ctx:
        labels, infos, nf = fused_batch(ctx, [sweep], p64)
        assert nf == 0
        check_against_b(labels, infos, [sweep], p64)
        for cp in (2, 9):
            p = params(L)
            p.curbPoints = cp
            labels, infos, nf = fused_batch(ctx, [sweep], p)
            assert nf == 0
            check_against_b(labels, infos, [sweep], p)
    big = [O.cfg_cloud("cfg2", 1), O.cfg_cloud("sensor", 2)]
    with u.Context(64 * 2048, 2) as ctx:
        labels, infos, nf = fused_batch(ctx, big, params(L))
        check_against_b(labels, infos, big, params(L))
        labels, infos, nf = fused_batch(ctx, big, O.cfg_params("cfg2"))
        assert nf == 2
        check_against_b(labels, infos, big, O.cfg_params("cfg2"))


def test_fused_labels_equal_the_goldens_of_oracle_a():
    """tests/golden/lasers/*.npz (the reference's own sources): firing order, fused."""
    import os
    from golden.make_golden_lasers import CASES, OUT, case_cloud, case_params
    for name, lasers, cols, scene, seed in CASES:
        g = np.load(os.path.join(OUT, name + ".npz"))
        p = case_params(lasers)
        scan = case_cloud(lasers, cols, scene, seed)
        with u.Context(lasers * cols, 1) as ctx:
            labels, infos, nf = fused_batch(ctx, [scan], p)
        assert nf == 1, name
        assert np.array_equal(labels[0] & O.MASK_NO_RING, g["labels"]), name
        assert int(infos[0][4]) == int(g["info_n_road"]) > 0 and int(infos[0][5]) == int(g["info_n_curb"]) > 0, name


@pytest.mark.parametrize("L", LASERS)
def test_sensor_like_sweeps_against_oracle_a(L):
    """Two sensor-like sweeps per laser count against the reference's own sources, run live where they are built."""
    if not O.has_oracle_a():
        pytest.skip("oracle A (the reference's sources) is not built here")
    p = params(L)
    scans = [u.synth_cloud(L, 2048, 3, 21), u.synth_cloud(L, 2048, 4, 22)]
    la, ia, _, _ = O.run_a(scans, p)
    with u.Context(L * 2048, len(scans)) as ctx:
        labels, infos, nf = fused_batch(ctx, scans, p)
    assert nf == len(scans)
    for k in range(len(scans)):
        assert ia[k]["n_road"] > 0 and ia[k]["n_curb"] > 0
        assert np.array_equal(labels[k] & O.MASK_NO_RING, la[k]), k


def ring_major(cloud, L):
    """The same sweep stored row by row (row-major L x W: an organised cloud)."""
    return tuple(np.ascontiguousarray(a.reshape(-1, L).T.reshape(-1)) for a in cloud)


@pytest.mark.parametrize("L", LASERS)
@pytest.mark.parametrize("cols,wide", [(2048, True), (1024, True), (2048, False), (96, True), (2047, True)])
def test_row_major_clouds_take_the_fused_front_end_from_the_second_call(L, cols, wide):
    """k_rows_probe, k_transpose and k_label_front's row-major stores with L rows: the first call sights the layout, the second takes it."""
    p = params(L, wide)
    scans = [ring_major(u.synth_cloud(L, cols, scene, 5 + (0 if wide else 1) + scene), L) for scene in (1, 2, 3, 4)]
    if cols >= 1024:
        says_something(scans, p)
    with u.Context(L * cols, len(scans)) as ctx:
        labels, infos, nf0 = fused_batch(ctx, scans, p)
        assert nf0 == 0
        check_against_b(labels, infos, scans, p)
        labels, infos, nf = fused_batch(ctx, scans, p)
        assert nf == len(scans), (nf0, nf)
        check_against_b(labels, infos, scans, p)
        labels, infos, nf = fused_batch(ctx, scans[::-1], p)
        assert nf == len(scans)
        check_against_b(labels, infos, scans[::-1], p)
        labels, infos, nf = fused_batch(ctx, scans, p, mode=0)
        assert nf == 0
        check_against_b(labels, infos, scans, p)


@pytest.mark.parametrize("L", LASERS)
def test_a_row_major_single_sweep_on_the_callback_path(L):
    """urf_classify_pc2 of a row-major L x 2048 sweep, several times (sighting, then whichever kernels the context chooses): labels."""
    p = params(L)
    x, y, z = ring_major(u.synth_cloud(L, 2048, 3, 9), L)
    lb, ib, _ = O.run_b(x, y, z, p)
    assert ib["n_road"] > 0 and ib["n_curb"] > 0
    with u.Context(len(x), 1, params=p) as ctx:
        ctx.set_front_mode(2)   # (16 / 32 lasers: the fused kernels are opt-in, on this path too)
        for _ in range(4):
            labels, info = ctx.classify_xyz(x, y, z)
            assert np.array_equal(labels, lb)
            assert info.n_road == ib["n_road"] and info.n_curb == ib["n_curb"]


def test_ring_sorted_results_after_a_fused_call():
    L, N = 32, 32 * 2048
    p = params(L)
    scans = [u.synth_cloud(L, 2048, 3, 1), u.synth_cloud(L, 2048, 2, 2)]
    says_something(scans, p)
    with u.Context(N, 2) as ctx:
        X, Y, Z = (np.concatenate([s[k] for s in scans]) for k in range(3))
        dx, dy, dz = DevBuf.from_numpy(X), DevBuf.from_numpy(Y), DevBuf.from_numpy(Z)
        dl = DevBuf(2 * N)
        ctx.set_params(p)
        ctx.set_front_mode(2)
        ctx.classify_batch_soa(dx, dy, dz, N, 2, dl, None)
        assert ctx.front_scans() == 2
        for k, (x, y, z) in enumerate(scans):
            lb, ib, st = O.run_b(x, y, z, p, debug=True)
            road, curb, prob = ctx.ordered_indices(N, scan=k)
            assert np.array_equal(road, st["road_order"]) and np.array_equal(curb, st["curb_order"]) and np.array_equal(prob, st["ring10_order"])
            assert np.array_equal(ctx.marker_points(scan=k), st["marker_pts"])
            assert np.array_equal(ctx.read_stage(u.STAGE_DETECT, N, scan=k), st["detect"])
            assert np.array_equal(dl.to_numpy(np.uint8).reshape(2, N)[k], lb)


def test_published_clouds_and_marker_chain_after_a_fused_call():
    """classify_batch_soa (32 lasers, fused: checked) -> urf_clouds_batch_soa in both orders against oracle B's clouds, every byte ->
    marker_points_batch -> marker_strips_batch against oracle B's chain, all on the device and on one context."""
    import marker_sets as M
    from test_gpu_batch_clouds import Batch
    from test_gpu_marker_strips import STRIDE_P, assert_equal_oracle, oracle_chain, unpack
    L = 32
    p, mp = params(L), M.marker_params(1, 1)
    scans = [u.synth_cloud(L, 2048, 1 + (s % 2) * 2, 40 + s) for s in range(4)]
    says_something(scans, p)
    S = len(scans)
    want_b, g_b, status = oracle_chain(scans, p, mp)
    assert any(w for w in want_b)
    b = Batch(scans)
    with u.Context(L * 2048, S, params=p) as ctx:
        ctx.set_front_mode(2)
        labels, infos = b.classify(ctx, "soa")
        assert ctx.front_scans() == S
        check_against_b(labels, infos, scans, p)
        b.check_clouds(ctx, "soa", u.ORDER_INPUT, p)
        assert ctx.front_scans() == S                      # (input order reads labels and inputs only)
        b.check_clouds(ctx, "soa", u.ORDER_REFERENCE, p)   # (ring-sorted results: the call runs again through the general kernels)
        assert all(np.array_equal(a, c) for a, c in zip(labels, b.labels()))
        ctx.set_front_mode(2)
        labels, infos = b.classify(ctx, "soa")
        assert ctx.front_scans() == S
        d_ghost = DevBuf.from_numpy(np.zeros(1, np.int32))
        d_pts, d_cnt = DevBuf(S * STRIDE_P * 4), DevBuf(S * 4)
        d_strips, d_xyz, d_n = DevBuf(S * u.MARKER_MAX_STRIPS * 32), DevBuf(S * u.MARKER_MAX_STRIP_POINTS * 12), DevBuf(S * 12)
        ctx.marker_points_batch(d_pts, d_cnt)
        ctx.marker_strips_batch(mp, d_pts, d_cnt, S, 1, d_ghost, d_strips, d_xyz, d_n)
        ctx.synchronize()
        assert [int(v) for v in infos[:, 0].astype(np.int32)] == status
        assert_equal_oracle(unpack(d_strips, d_xyz, d_n, S), want_b, "32 lasers, fused first")
        assert int(d_ghost.to_numpy(np.int32)[0]) == g_b[-1]


@pytest.mark.parametrize("L", LASERS)
@pytest.mark.parametrize("seed", range(40))
def test_organised_sweeps_with_holes(L, seed):
    (x, y, z), p = case(7_400_000 + 1000 * L + seed, L)
    lb, ib, _ = O.run_b(x, y, z, p)
    with u.Context(len(x), 1) as ctx:
        labels, infos, nf = fused_batch(ctx, [(x, y, z)], p)
    assert np.array_equal(labels[0], lb), "%d labels differ (fused %d)" % (int((labels[0] != lb).sum()), nf)
    keys = ("status", "n_roi", "n_rings", "n_ring_pts", "n_road", "n_curb", "n_ring10")
    assert {f: int(v) for f, v in zip(keys, infos[0][:7])} == {f: ib[f] for f in keys}
    assert p.curbPoints == 5 or nf == 0


@pytest.mark.parametrize("L", LASERS)
def test_full_size_batch(L):
    """256 scans of L x 2048 built from 16 distinct sweeps, every batch call (mode 2): all fused, twins equal byte for byte."""
    p = params(L)
    base = [u.synth_cloud(L, 2048, 1 + (s % 2) * 2, 70 + s) for s in range(16)]
    says_something(base[:2], p)
    scans = [base[s % 16] for s in range(256)]
    with u.Context(L * 2048, 256) as ctx:
        labels, infos, nf = fused_batch(ctx, scans, p)
        assert nf == 256
        check_against_b(labels[:16], infos[:16], scans[:16], p)
        for s in range(16, 256):
            assert np.array_equal(labels[s], labels[s % 16]) and np.array_equal(infos[s], infos[s % 16])
