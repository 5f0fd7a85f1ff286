"""The fused front end at star-sector counts other than 360 (params.sectors = K in {1, 90, 720, 1022}; urf_validate_params takes 1..1022).
What of the fused kernels depends on K: the plain march's tile_end (bisection over the step keys, tsoff rows of K + 1 entries: 16 trips at
1022, one at 1), urf_fast_sector's margin (sectors / 360), k_front_sectors' tables (four keys per thread up to 1024, [K] the total), the
beam body's [sectors] table, and every consumer of the march's records through [S][tiles][K + 1] and [S][sectors] tables (k_index, the
sort kernels with their mid and big lists -- a 64-laser sector at K = 90 holds more than 384 records, at K = 1 more than 2048 --,
k_front_finish*, k_label_front*, the read-outs).

Always: labels and the seven summary fields equal oracle B, exactly, and info[7] == 0.  Every test keeps K = 360 as the control ON THE SAME
CONTEXT, so that a failure at K points at K and not at the input.  An expected urf_front_scans() is computed on the CPU
(front_sector_cases.clean, front_shape.fusable; tests/test_front_sectors_cpu.py pins the values) and asserted from the second call after a
change of parameters on (a context's first call with new parameters may hand a sweep back for its speculative ring table).

Shapes: 64 x 96 / 256, 32 x 136 / 256, 16 x 304 / 512, 128 x 48 / 64: three to eight tiles, some ending in a partial tile."""
import numpy as np
import pytest

import front_sector_cases as SC
import front_shape as FS
import oracles as O
import urban_road_filter_amd as u
from test_front_multi_cpu import ragged_scans, seam_sweeps, small_models, small_params, small_sweeps
from test_gpu_batch_clouds import Batch
from test_gpu_front_outputs import batch_readouts, same
from test_gpu_parity import run_batch

pytestmark = pytest.mark.gpu
KEYS = ("status", "n_roi", "n_rings", "n_ring_pts", "n_road", "n_curb", "n_ring10")
NAMES = sorted(small_models())
CAPACITY = 64 * 2048   # max_points of every context below: a sensor-sized one (the candidate lists do not hand scans back)


def check(labels, infos, scans, p, what=""):
    """Labels and summaries against oracle B (computed once per sweep and parameters: front_shape.stages)."""
    for k, c in enumerate(scans):
        lb, ib, _ = FS.stages(c, p)
        assert np.array_equal(labels[k], lb), "%s K %d, scan %d: %d labels differ" % (what, p.sectors, k, int((labels[k] != lb).sum()))
        assert dict(zip(KEYS, (int(v) for v in infos[k][:7]))) == {f: ib[f] for f in KEYS}, "%s K %d, scan %d" % (what, p.sectors, k)
        assert infos[k][7] == 0, "%s K %d, scan %d: NaN azimuths counted" % (what, p.sectors, k)


def context(scans, p, **kw):
    """Every switch that lets a call with these parameters take a fused instance, but for the two multi-sector ones (call sets them)."""
    ctx = u.Context(max(CAPACITY, max(len(c[0]) for c in scans)), len(scans), **kw)
    if p.channels == 128:
        ctx.set_front_lasers128(1)
    if p.channels != 64:
        ctx.set_front_curb_points(1)
    return ctx


def call(ctx, scans, p, ms=0, ms_cp=0, mode=2, calls=2):
    ctx.set_front_mode(mode)
    ctx.set_front_multi_sector(ms)
    ctx.set_front_multi_sector_curb_points(ms_cp)
    ragged = len({len(c[0]) for c in scans}) > 1
    for _ in range(calls):
        labels, infos = run_batch(ctx, scans, p, ragged=ragged)
    return labels, infos, ctx.front_scans()


def n_clean(scans, p, layout="firing"):
    return sum(SC.clean(c, p, layout) for c in scans)


# ---- 1. plain instances ----
def plain_steps(L, cols, K, rows, **tweak):
    """360, K, 360 on one context; the count of every step is the CPU predicate's."""
    scans = SC.rows_sweeps(L, cols) if rows else SC.plain_sweeps(L, cols)
    layout = "rows" if rows else "firing"
    pk = SC.plain_params(L, K, **tweak)
    p360 = SC.at_k(pk, 360)
    with context(scans, pk) as ctx:
        for step, p in (("control", p360), ("tested", pk), ("control again", p360)):
            labels, infos, nf = call(ctx, scans, p)
            check(labels, infos, scans, p, step)
            assert nf == n_clean(scans, p, layout), "%s, K %d: %d fused, %d clean" % (step, p.sectors, nf, n_clean(scans, p, layout))
        assert n_clean(scans, pk, layout) == len(scans)   # (the gate: tests/test_front_sectors_cpu.py says every shape is clean at every K)


@pytest.mark.parametrize("beam", (0, 1))
@pytest.mark.parametrize("K", SC.KS)
@pytest.mark.parametrize("L,cols", SC.SHAPES)
def test_plain_sweeps_in_firing_order(L, cols, K, beam):
    plain_steps(L, cols, K, False, starbeam_filter=beam)


# (64 x 256 row-major at K = 1 without the beam body is left to 64 x 96: the call that sights the layout runs the general kernels, whose
# sort of ONE sector of 15 000 participants takes most of a second -- longer than any test of tests/test_gpu_front_multi.py)
ROWS_CASES = [(L, cols, K, beam) for L, cols in SC.SHAPES for K in SC.KS for beam in (0, 1) if (L, cols, K, beam) != (64, 256, 1, 0)]


@pytest.mark.parametrize("L,cols,K,beam", ROWS_CASES)
def test_plain_sweeps_row_major(L, cols, K, beam):
    """(the first call sights the layout: asserted from the second call on, as everywhere)"""
    plain_steps(L, cols, K, True, starbeam_filter=beam)


@pytest.mark.parametrize("L,cols", SC.SHAPES[::2])
def test_without_the_star_shaped_search_sectors_do_not_matter(L, cols):
    for K in SC.KS:
        plain_steps(L, cols, K, False, star_shaped_method=0)


# ---- 2. multi-sector instances ----
def multi_steps(scans, p, K, mode=2, ms_cp=0):
    """K = 360 with the switch on: all fused (the input's part).  The tested K with the switch off: the scans the plain kernels keep at
    that K (none, but at K = 1, where one sector holds every participant and every scan is kept).  The tested K with the switch on: all."""
    pk, p360 = SC.at_k(p, K), SC.at_k(p, 360)
    want_off = n_clean(scans, pk)
    with context(scans, p) as ctx:
        for step, q, on, want in (("360, switch on", p360, 1, len(scans)), ("K, switch off", pk, 0, want_off), ("K, switch on", pk, 1, len(scans)),
                                  ("K, switch on, reversed", pk, 1, len(scans))):
            batch = scans[::-1] if "reversed" in step else scans
            labels, infos, nf = call(ctx, batch, q, on, on and ms_cp, mode=mode)
            check(labels, infos, batch, q, step)
            assert nf == want, "%s (K %d): %d of %d fused, expected %d" % (step, q.sectors, nf, len(scans), want)
        assert all(FS.fusable(c, pk) for c in scans)


@pytest.mark.parametrize("K", SC.KS)
@pytest.mark.parametrize("name", NAMES)
def test_multi_sector_sweeps(name, K):
    multi_steps(small_sweeps(name), small_params(name), K)


@pytest.mark.parametrize("K", SC.KS)
@pytest.mark.parametrize("name", NAMES)
def test_the_seam_inside_a_tile_and_on_its_last_firing(name, K):
    multi_steps(seam_sweeps(name), small_params(name), K)


@pytest.mark.parametrize("K", SC.KS)
def test_ragged_batch(K):
    """A scan that ends inside a firing and a tile, a tile without a participant, a tile whose 2048 points all take part."""
    multi_steps(ragged_scans(), small_params("64 offsets"), K)


# ---- 3. other curbPoints ----
@pytest.mark.parametrize("K", (90, 1022))
@pytest.mark.parametrize("cp", (1, 8))
@pytest.mark.parametrize("name", ("64 offsets", "16 drift"))
def test_other_curb_points(name, cp, K):
    """Front mode 3 with urf_set_front_multi_sector_curb_points on."""
    p = small_params(name)
    p.curbPoints = cp
    multi_steps(small_sweeps(name), p, K, mode=3, ms_cp=1)


# ---- 4. the read-outs and the callback path ----
@pytest.mark.parametrize("outputs", (1, 0))
@pytest.mark.parametrize("K", (90, 1022))
@pytest.mark.parametrize("model", ("plain 64 x 96", "64 offsets"))
def test_read_outs_behind_a_fused_call(model, K, outputs):
    """Ordered lists, marker points and the clouds in both orders behind a fused call at K, the control at 360 first on the same context."""
    if model == "64 offsets":
        scans, p, ms = small_sweeps(model), small_params(model), 1
    else:
        scans, p, ms = SC.plain_sweeps(64, 96), SC.plain_params(64), 0
    b = Batch(scans)
    stride = len(scans[0][0])
    with context(scans, p, params=p) as ctx:
        ctx.set_front_mode(2)
        ctx.set_front_multi_sector(ms)
        ctx.set_front_outputs(outputs)
        for q in (SC.at_k(p, 360), SC.at_k(p, K)):
            refs = [FS.stages(c, q) for c in scans]
            ctx.set_params(q)
            for _ in range(2):
                labels, infos = b.classify(ctx, "soa")
            assert ctx.front_scans() == len(scans), q.sectors
            check(labels, infos, scans, q)
            before = b.dl.to_numpy(np.uint8).copy()
            for s, got in enumerate(batch_readouts(ctx, len(scans), stride)):
                same(got, refs[s][2], (model, q.sectors, outputs, s))
            for order in (u.ORDER_REFERENCE, u.ORDER_INPUT):
                b.check_clouds(ctx, "soa", order, q)
            assert np.array_equal(b.dl.to_numpy(np.uint8), before)   # the caller's labels: unchanged
            if outputs:
                assert ctx.front_scans() == len(scans)   # (no second run through the general kernels)
            ctx.set_front_mode(2)   # (outputs off: the read-outs ran the call again through the general kernels; fused again from here)


def test_callback_path_of_a_row_major_context():
    """classify_xyz and four classify_pc2_async in flight at K = 1022, 360, 90 with urf_set_params in between."""
    L, cols = 64, 256
    base = SC.plain_params(L)
    rows = SC.rows_sweeps(L, cols) + [SC.rows_of(u.synth_cloud(L, cols, scene, 40 + scene), L) for scene in (2, 4)]
    rec = []
    for c in rows:
        r = np.zeros((len(c[0]), 4), np.float32)
        r[:, 0], r[:, 1], r[:, 2] = c
        rec.append(r)
    seen = []
    with u.Context(CAPACITY, 4, params=base) as ctx:
        ctx.set_front_mode(2)
        for K in (1022, 360, 90):
            p = SC.at_k(base, K)
            ctx.set_params(p)
            want = [FS.stages(c, p)[:2] for c in rows]
            assert all(ib["status"] == 0 and ib["n_road"] > 0 and ib["n_curb"] > 0 for _, ib in want)
            for rep in range(3):
                for c, (lb, ib) in zip(rows, want):
                    lab, info = ctx.classify_xyz(*c)
                    assert np.array_equal(lab, lb) and info.n_road == ib["n_road"] and info.n_curb == ib["n_curb"], (K, rep)
                    seen.append((K, ctx.front_scans()))
            tickets = [ctx.classify_pc2_async(r, len(r), 16, 0, 4, 8) for r in rec]   # four sweeps in flight
            for t, (lb, ib) in zip(tickets, want):
                lab = np.zeros(len(lb), np.uint8)
                info = ctx.classify_pc2_wait(t, lab)
                assert np.array_equal(lab, lb) and info.n_road == ib["n_road"] and info.n_curb == ib["n_curb"], K
    print("callback path, (K, fused) per sweep: %s" % seen)
    for K in (1022, 360, 90):
        assert any(n for k, n in seen if k == K), K   # (once the layout is sighted the path does take the fused kernels, at every K)


# ---- 5. fuzz ----
_FUZZ_NF = {}


def fuzz_run(L, seed, compare=True):
    """A random sensor model, world, encoding mix, start azimuth, region of interest and detector parameters (sensor_models.fuzz_case), the
    sector count drawn by the seed, every switch on, two calls.  (The seeds' base keeps the fusable K = 1 sweeps to 16 500 participants
    -- front_sector_cases.FUZZ_BASE: the fused star search of one sector costs seconds beyond -- so the fuzz holds NO large one-sector
    input; K = 1 at 64 x 256 with 15 000 participants is the fixed tests' above.)"""
    cloud, p, model = SC.fuzz_case(seed, L)
    lb, ib, _ = O.run_b(*cloud, p) if compare else (None, None, None)
    with context([cloud], p) as ctx:
        ctx.set_front_long_sweeps(1)
        for _ in range(2):
            labels, infos, nf = call(ctx, [cloud], p, 1, 1, mode=3, calls=1)
            if compare:
                assert np.array_equal(labels[0], lb), "%s, K %d: %d labels differ (fused %d)" % (model, p.sectors, int((labels[0] != lb).sum()), nf)
                assert dict(zip(KEYS, (int(v) for v in infos[0][:7]))) == {f: ib[f] for f in KEYS}, (model, p.sectors)
                assert int(infos[0][7]) == ib["n_nan_azimuth"], (model, p.sectors)
    _FUZZ_NF[(L, seed)] = nf


@pytest.mark.parametrize("L", (16, 32, 64))
@pytest.mark.parametrize("seed", range(20))
def test_fuzzed_sensor_sweeps(L, seed):
    fuzz_run(L, seed)


@pytest.mark.parametrize("K", SC.KS)
@pytest.mark.parametrize("L", (16, 32, 64))
def test_some_fuzzed_sweep_was_fused(L, K):
    """(a gate that lets none of them through would pass everything above)"""
    seeds = [s for s in range(20) if SC.KS[s % 4] == K]
    for seed in seeds:
        if (L, seed) not in _FUZZ_NF:   # (run on its own)
            fuzz_run(L, seed, compare=False)
        if _FUZZ_NF[(L, seed)]:
            break
    assert any(_FUZZ_NF.get((L, s)) for s in seeds), (L, K)
