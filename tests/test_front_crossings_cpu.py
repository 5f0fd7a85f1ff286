"""The multi-sector switches crossed with dense entry points, long sweeps and a long-lived context, the CPU side: the inputs of
tests/test_gpu_front_crossings.py (tests/front_crossing_cases.py) have the properties they are used for, pinned from oracle B's stages,
so that the fused counts asserted on the GPU come from here.

Dense sweeps (hdl64e, vlp16, vlp32c, "128 stagger", three scans each, started at 77.7 / 123.4 degrees): oracle B finds road and curb on
the dense points; every padded twin is fusable, has firings in several sectors and a tile with falling sectors; the third scan of every
model has lost half-firings and its re-alignment joins firings (fewer firings than the organised sweep had).  Long sweeps (129 and 256
tiles): fusable, astride, the sweep's wrap in the last tile, and in tile 128 for the second scan of the 256-tile batch."""
import os
import subprocess

import numpy as np
import pytest

import dense_model as D
import front_crossing_cases as XC
import front_sector_cases as SC
import front_shape as FS
import sensor_models as SM
from test_front_multi_cpu import small_params, small_sweeps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def says_something(c, p):
    ib = FS.stages(c, p)[1]
    assert ib["status"] == 0 and ib["n_road"] > 0 and ib["n_curb"] > 0, ib
    return ib


# ---- dense x multi-sector ----
@pytest.mark.parametrize("K,cp", ((360, 5), (1022, 5), (360, 3)))
@pytest.mark.parametrize("name", sorted(XC.DENSE))
def test_dense_scans_and_their_padded_twins(name, K, cp):
    p = XC.dense_params(name, K, cp)
    L, W = XC.dense_lasers(name), XC.dense_width(name)
    scans = XC.dense_scans(name)
    assert len(scans) == 3
    for dense, slot, F, key, twin, firings in scans:
        says_something(dense, p)
        assert len(slot) < F * L and D.realign(slot, L, W)[2] and len(twin[0]) == W * L
        says_something(twin, p)   # (the padded twin: the same points, holes as NaN)
        assert FS.fusable(twin, p)
        assert FS.multi_sector_firings(twin, p)[0] > 0 and FS.tiles_where_sectors_fall(twin, p) >= 1
        assert not SC.clean(twin, p)   # (the plain kernels hand it back: 0 fused with the switch off)
        assert np.array_equal(FS.stages(twin, p)[0][D.realign(slot, L, W)[0]], FS.stages(dense, p)[0])   # (labels of the twin's points = the dense scan's)


@pytest.mark.parametrize("name", sorted(XC.DENSE))
def test_the_realignment_joins_firings_in_one_scan_per_model(name):
    """A firing whose leading lasers are missing is joined to the one before where that one lacks its trailing lasers: the twin has fewer
    firings than the organised sweep.  Scans 0 and 1 (random drops only) keep every firing."""
    scans = XC.dense_scans(name)
    assert [s[5] for s in scans[:2]] == [s[2] for s in scans[:2]]
    assert scans[2][5] == scans[2][2] - len(XC.MERGED_AT)


def test_the_seam_of_a_dense_sweep_lies_inside_a_tile():
    for name in XC.DENSE:
        p = XC.dense_params(name)
        for sc in XC.dense_scans(name):
            tiles = XC.seam_tiles(sc[4], p)
            assert tiles and 0 < max(tiles) < -(-len(sc[4][0]) // FS.TILE) - 1, (name, tiles)


# ---- long sweeps x multi-sector ----
@pytest.mark.parametrize("name", sorted(XC.LONG))
def test_long_sweeps(name):
    p = XC.long_params(name)
    L = p.channels
    want_tiles = 256 if name == "64 x 8192" else 129
    for k, (c, r) in enumerate(zip(XC.long_sweeps(name), XC.long_rows(name))):
        assert -(-len(c[0]) // FS.TILE) == want_tiles and len(c[0]) % L == 0
        says_something(c, p)
        assert FS.fusable(c, p) and FS.fusable(r, p, "rows")
        assert FS.multi_sector_firings(c, p)[0] > 0 and not SC.clean(c, p) and not SC.clean(r, p, "rows")
        tiles = XC.seam_tiles(c, p)
        wrap_tile = XC.LONG[name][2][k][0] * L // FS.TILE   # the tile of the firing at which the sweep wraps
        assert wrap_tile in tiles and XC.tail_falls(c, p) == 1, (name, k, tiles)
        # the candidate list of the context the GPU test uses holds the sweep's entries, in either layout (front_shape.front_candidates)
        mp = XC.long_max_points(name)
        assert FS.fits(c, p, mp, 2) and FS.fits(r, p, mp, 2, "rows")
        assert FS.front_candidates(c, p, 2) == FS.front_candidates(r, p, 2, "rows")
        if (name, k) == ("64 x 8192", 1):
            assert wrap_tile == 128 and max(tiles) < 140   # tile 128 exactly: the first row beyond the 128 the short tables hold
        else:
            assert wrap_tile == want_tiles - 1             # the last tile


def test_a_thinned_long_sweep_overflows_the_candidate_list_of_a_context_of_its_own_size():
    """The hand-back rule front_shape.fusable does not hold: "a full candidate list" (urf_front_flush).  64 x 8192 with four returns of
    five dropped: more than 100 000 entries per sweep, EDGE items of the 256 blocks' halos most of them, against 65 536 on a context of
    64 x 8192 points and 196 608 on the one the fused tests use -- a tenth and more away from either.  With one return in a hundred dropped
    the same geometry files a few thousand."""
    name = "64 x 8192"
    p = XC.long_params(name)
    n = 64 * 8192
    assert FS.candidate_cap(n, 64) == 65536 and FS.candidate_cap(XC.long_max_points(name), 64) == 196608
    for c in XC.long_sweeps(name):
        cand = FS.front_candidates(c, p, 2)
        print("64 x 8192, drop %.1f: %d candidates" % (XC.LONG_DROP[name], cand))
        assert 1.1 * 65536 < cand < 0.9 * 196608
        assert not FS.fits(c, p, n, 2) and FS.fits(c, p, XC.long_max_points(name), 2)
    whole = SM.sweep(XC.long_model(name), world=2, seed=43, start_deg=360.0 - 8176 * 360.0 / 8192)   # (one return in a hundred dropped)
    assert FS.front_candidates(whole, p, 2) < 8192


def test_the_candidate_model_counts_what_the_kernel_files():
    """A sweep without holes in any halo files full-window entries only: as many as the ring points that pass the height tests, whatever
    the block size; blocks of one tile against blocks of four add nothing but the tails' EDGE items and a window's first centres."""
    name = "64 offsets"
    p = small_params(name)
    for c in small_sweeps(name):
        few, many = FS.front_candidates(c, p, 1024), FS.front_candidates(c, p, 2)   # four tiles per block, one
        assert 0 < few <= many < 8192
    off = p.copy()
    off.x_zero_method = off.z_zero_method = 0
    assert FS.front_candidates(small_sweeps(name)[0], off, 2) == 0


def test_the_ragged_long_batch():
    p = XC.long_params("64 x 4128")
    short = XC.short_sweep()
    assert len(short[0]) == 4 * FS.TILE
    says_something(short, p)
    assert FS.fusable(short, p) and not SC.clean(short, p)
    for c in [short] + XC.long_sweeps("64 x 4128"):
        assert FS.fits(c, p, XC.long_max_points("64 x 4128"), 3)


# ---- histories ----
@pytest.mark.parametrize("K", (360, 1022, 1, 90))
def test_the_sector_walk_has_something_to_compare_at_every_step(K):
    """The multi-sector call and the plain call that take turns: fusable, their candidates fit, the plain twins clean at every K and with
    as many rings, row for row, as the sweeps they alternate with (k_ring_table's hint -- the ring count of the row's previous call --
    holds: no call is handed back for it).  The unorganised scan is not fusable at any K: the count of a call that holds it is 2."""
    name = "64 offsets"
    p = SC.at_k(small_params(name), K)
    multi, plain, sh = small_sweeps(name), XC.plain_twins(), XC.shuffled_sweep()
    for c in multi + plain:
        says_something(c, p)
        assert FS.fusable(c, p) and FS.fits(c, p, 64 * 2048, 3)
    assert all(SC.clean(c, p) for c in plain) and all((K == 1) == SC.clean(c, p) for c in multi)
    assert [FS.stages(c, p)[1]["n_rings"] for c in multi] == [FS.stages(c, p)[1]["n_rings"] for c in plain]
    ib = FS.stages(sh, p)[1]
    assert ib["status"] == 0 and ib["n_road"] > 0 and not FS.fusable(sh, p)


def test_the_dense_history():
    p = XC.dense_params("hdl64e")
    assert bytes(p) == bytes(small_params("64 offsets"))   # (one parameter set for the dense calls and the batch in between)
    for c in small_sweeps("64 offsets") + [XC.ideal_sweep()]:
        says_something(c, p)
        assert FS.fusable(c, p)
    for sc in XC.short_dense_scans():
        says_something(sc[0], p)
        assert D.realign(sc[1], 64, XC.SHORT_W)[2] and FS.fusable(sc[4], p)
    long_n = max(len(s[1]) for s in XC.dense_scans("hdl64e"))
    assert all(len(s[1]) < long_n for s in XC.short_dense_scans())   # fewer scans, fewer points, another W: stale staging would show


def test_the_switch_walk_expectations_are_plan_s(tmp_path):
    """front_crossing_cases.SWITCH_PLAN is what urf_policy::plan says of each step of SWITCH_WALK (tests/cpp/policy_switch_walk.cpp)."""
    exe = str(tmp_path / "policy_switch_walk")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "urban_road_filter_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "policy_switch_walk.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe] + [str(v) for step in XC.SWITCH_WALK for v in step], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got = tuple(tuple(int(w) for w in line.split()) for line in r.stdout.splitlines())
    assert got == XC.SWITCH_PLAN
    assert {ms for _, ms in got} == {0, 1}   # (a walk that never leaves one state would show nothing)
    for cp in (3, 5):   # ... and the sweeps of the walk: the astride ones need front_ms, the ideal one does not
        p = small_params("64 offsets")
        p.curbPoints = cp
        for c in small_sweeps("64 offsets"):
            says_something(c, p)
            assert FS.fusable(c, p) and not SC.clean(c, p)
        for k, c in enumerate(XC.plain_twins()):   # (the plain call: clean, and the ring count of the sweep it alternates with)
            says_something(c, p)
            assert SC.clean(c, p) and FS.stages(c, p)[1]["n_rings"] == FS.stages(small_sweeps("64 offsets")[k], p)[1]["n_rings"]


def test_the_128_laser_fuzz_draws_what_it_is_for():
    """Twenty seeds: every kind of offset, every firing count, every sector count; sweeps with a result that front_shape.fusable accepts
    with firings in several sectors (what the gate of the GPU test needs)."""
    kinds, firings, sectors, good = set(), set(), set(), 0
    for seed in range(20):
        cloud, p, kind = XC.fuzz128_case(seed)
        assert p.channels == 128 and p.interval == np.float32(0.05) and 1 <= p.curbPoints <= 8
        kinds.add(kind), firings.add(len(cloud[0]) // 128), sectors.add(p.sectors)
        ib = FS.stages(cloud, p)[1]
        good += bool(ib["status"] == 0 and ib["n_road"] > 0 and p.star_shaped_method and FS.fusable(cloud, p) and FS.multi_sector_firings(cloud, p)[0] > 0)
    assert kinds == {"stagger", "offsets", "drift"} and firings == {64, 128, 256} and sectors == {90, 360, 1022}
    assert good >= 5, good
