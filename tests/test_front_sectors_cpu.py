"""params.sectors other than 360, the CPU side: the inputs of tests/test_gpu_front_sectors.py have the properties they are used for at
every sector count K in {1, 90, 720, 1022} (and at 360, the control), pinned from oracle B's stages (tests/front_shape.py,
tests/front_sector_cases.py), so that the fused counts asserted on the GPU come from here and never from the code under test.

The figures.  Plain sweeps (urf_synth_cloud at the eight small shapes, in firing order and row-major, starbeam_filter 0 and 1): clean at
every K -- one sector per firing, no tile with falling sectors --, 32 x 136 at K = 720 included, whose firing 8 lies on a sector border.
The four small models with azimuth offsets or drift: fusable at every K, astride at every K but 1, where one sector holds every
participant; at 720 and 1022 a firing of "64 offsets" extends over ten and fourteen sectors (four distinct ones: the model has four
offsets).  Oracle B finds road and curb on every fixed input at every K; at K = 1 x_zero and z_zero alone supply curb points (the star
search adds at most one per sweep there: its single sector stops at the first curb)."""
import numpy as np
import pytest

import front_sector_cases as SC
import front_shape as FS
import sensor_models as SM
from test_front_multi_cpu import ragged_scans, seam_sweeps, small_models, small_params, small_sweeps

NAMES = sorted(small_models())
ALL_K = SC.KS + (360,)


def says_something(c, p):
    ib = FS.stages(c, p)[1]
    assert ib["status"] == 0 and ib["n_road"] > 0 and ib["n_curb"] > 0, ib
    return ib


def multi_scans(name):
    return small_sweeps(name) + seam_sweeps(name) + (ragged_scans() if name == "64 offsets" else [])


@pytest.mark.parametrize("K", ALL_K)
@pytest.mark.parametrize("L,cols", SC.SHAPES)
def test_every_plain_sweep_is_clean_at_every_sector_count(L, cols, K):
    """(shape, K): fused count expected on the GPU = 2 of 2, in either layout, with either beam body."""
    for beam in (0, 1):
        p = SC.plain_params(L, K, starbeam_filter=beam)
        for c, r in zip(SC.plain_sweeps(L, cols), SC.rows_sweeps(L, cols)):
            says_something(c, p)
            assert SC.clean(c, p) and SC.clean(r, p, "rows"), (L, cols, K, beam)
            used = np.unique(FS.stages(c, p)[2]["sector"])
            used = used[used >= 0]
            # (the beam body may leave a sector without a participant: K = 1 at 64 and 128 lasers leaves none at all)
            assert (len(used) or beam) and (used < K).all()
            assert beam or len(used) >= min(K, cols) // 2   # (participants all around: the tsoff rows are written across their whole width)
    assert len(c[0]) == L * cols and -(-len(c[0]) // FS.TILE) in range(3, 9)   # three to eight tiles


def test_partial_last_tiles_are_among_the_shapes():
    assert sum((L * cols) % FS.TILE != 0 for L, cols in SC.SHAPES) >= 2
    assert {L for L, _ in SC.SHAPES} == {16, 32, 64, 128}


def test_a_firing_on_a_sector_border_stays_in_one_sector():
    """32 x 136 at K = 720: firing 8 at (8 + 0.5) * 360 / 136 = 22.5 degrees, the border of sectors 44 and 45.  Its participants' float
    azimuths share one side in both sweeps (and in both layouts: the points are the same), so the sweep is a clean one; the decision is
    oracle B's, made here."""
    L, cols, K, f = SC.ON_A_BORDER
    assert (f + 0.5) * K / cols == 45.0
    p = SC.plain_params(L, K)
    for c in SC.plain_sweeps(L, cols):
        row = FS.firing_order(FS.stages(c, p)[2]["sector"], L, "firing")[f]
        assert (row >= 0).sum() > 1 and len(set(row[row >= 0].tolist())) == 1 and row.max() in (44, 45)
        assert SC.clean(c, p)


@pytest.mark.parametrize("L,cols", SC.SHAPES)
def test_at_one_sector_the_curb_comes_from_x_zero_and_z_zero(L, cols):
    """K = 1: the star search walks ONE sector outward and stops at its first curb: it cannot be what a comparison of curb labels rests on.
    With x_zero_method and z_zero_method on (the defaults) the curb points are theirs: as many without the star search, but for at most the
    one the star search adds."""
    for c in SC.plain_sweeps(L, cols):
        p = SC.plain_params(L, 1)
        assert p.x_zero_method == 1 and p.z_zero_method == 1
        with_star = says_something(c, p)["n_curb"]
        no_star = says_something(c, SC.plain_params(L, 1, star_shaped_method=0))["n_curb"]
        assert 0 < no_star <= with_star <= no_star + 1, (with_star, no_star)
        alone = FS.stages(c, SC.plain_params(L, 1, x_zero_method=0, z_zero_method=0))[1]["n_curb"]
        assert alone <= 1


@pytest.mark.parametrize("L,cols", SC.SHAPES[::2])
def test_without_the_star_shaped_search_every_sector_count_is_clean(L, cols):
    for K in SC.KS:
        p = SC.plain_params(L, K, star_shaped_method=0)
        for c in SC.plain_sweeps(L, cols):
            says_something(c, p)
            assert SC.clean(c, p)


@pytest.mark.parametrize("K", SC.KS)
@pytest.mark.parametrize("name", NAMES)
def test_the_small_models_at_every_sector_count(name, K):
    """Fusable at every K; astride (firings in several sectors, a seam inside a tile) at every K but 1, where no firing is multi-sector,
    every scan is a clean one and the plain kernels keep it."""
    p = SC.at_k(small_params(name), K)
    for c in multi_scans(name):
        says_something(c, p)
        assert FS.fusable(c, p)
        n_multi = FS.multi_sector_firings(c, p)[0]
        if K == 1:
            assert n_multi == 0 and FS.tiles_where_sectors_fall(c, p) == 0 and SC.clean(c, p)
        else:
            assert n_multi > 0 and FS.tiles_where_sectors_fall(c, p) >= 1 and not SC.clean(c, p)
    for c in small_sweeps(name):   # (the beam body's runs)
        q = p.copy()
        q.starbeam_filter = 1
        says_something(c, q)


@pytest.mark.parametrize("K,extent", ((360, 5), (720, 10), (1022, 14)))
def test_a_firing_of_the_offsets_model_extends_over_many_sectors(K, extent):
    """+- 2.4 degrees of azimuth offset: 4.8 degrees from the first laser's sector to the last's.  Four DISTINCT sectors at most (the model
    has four offsets), eight and more from end to end at 720 and 1022."""
    name = "64 offsets"
    p = SC.at_k(small_params(name), K)
    for c in small_sweeps(name):
        assert SC.widest_firing(c, p) in (extent, extent + 1), SC.widest_firing(c, p)
        assert FS.multi_sector_firings(c, p)[1] == 4
    assert K == 360 or extent >= 8


@pytest.mark.parametrize("K", (90, 1022))
@pytest.mark.parametrize("cp", (1, 8))
@pytest.mark.parametrize("name", ("64 offsets", "16 drift"))
def test_other_curb_points(name, cp, K):
    p = SC.at_k(small_params(name), K)
    p.curbPoints = cp
    for c in small_sweeps(name):
        says_something(c, p)
        assert FS.fusable(c, p) and not SC.clean(c, p)


@pytest.mark.parametrize("K", (90, 360, 1022))
def test_the_read_outs_have_something_to_show(K):
    """(tests/test_gpu_front_sectors.py: ordered lists and marker points behind a fused call)"""
    for scans, p in ((SC.plain_sweeps(64, 96), SC.plain_params(64, K)), (small_sweeps("64 offsets"), SC.at_k(small_params("64 offsets"), K))):
        for c in scans:
            st = FS.stages(c, p)[2]
            assert len(st["marker_pts"]) > 2 and len(st["road_order"]) > 0 and len(st["curb_order"]) > 0


def test_the_fuzz_draws_every_sector_count_with_sweeps_that_can_be_fused():
    """Twenty seeds per laser count, five per K; at every (L, K) a sweep in firing order that front_shape.fusable accepts with the
    star-shaped search on and curbPoints within 1..8 (what the gate of the GPU test needs: a lone row-major sweep is fused from the third
    call on only); no fusable sweep at K = 1 with more participants than FUZZ_K1_PARTICIPANTS (front_sector_cases.FUZZ_BASE)."""
    for L in (16, 32, 64):
        good = {K: 0 for K in SC.KS}
        for seed in range(20):
            cloud, p, model = SC.fuzz_case(seed, L)
            assert p.sectors == SC.KS[seed % 4]
            if not p.star_shaped_method or p.curbPoints > 8:
                continue
            lb, ib, st = FS.stages(cloud, p)
            layout = SM.MODELS[model]["layout"]
            if ib["status"] != 0 or not FS.fusable(cloud, p, layout):
                continue
            assert p.sectors != 1 or int((st["sector"] >= 0).sum()) <= SC.FUZZ_K1_PARTICIPANTS, (L, seed)
            good[p.sectors] += bool(layout == "firing" and ib["n_road"] > 0)
        print("fuzz, L = %d: fusable sweeps with road per K: %s" % (L, good))
        assert min(good.values()) >= 1, (L, good)
