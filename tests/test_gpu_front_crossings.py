"""urf_set_front_multi_sector crossed with the other paths a real sensor's sweep takes: the dense entry points (velodyne_pointcloud's
default delivery), sweeps of more than 128 tiles (urf_set_front_long_sweeps: k_front_sectors at tile indices above 127 and a.tiles of 129
and 256 in its row = s * a.tiles + t), and one long-lived context whose sector count, batches and entry points change between calls (the
tsoff row stride is sectors + 1: a stale row or a stale front_skey shows as a wrong label).

Always: labels and summaries equal oracle B, exactly -- for dense calls oracle B on the DENSE points and all eight info words.  An
expected urf_front_scans() comes from the CPU (front_shape.fusable, front_sector_cases.clean; tests/test_front_crossings_cpu.py pins the
inputs' properties) and is asserted from the second call after a change on; the padded twins' count of a dense case is a second,
independent expectation.  Inputs: tests/front_crossing_cases.py."""
import numpy as np
import pytest

import front_crossing_cases as XC
import front_sector_cases as SC
import front_shape as FS
import urban_road_filter_amd as u
from test_front_multi_cpu import small_params, small_sweeps
from test_gpu_batch_clouds import Batch
from test_gpu_dense import Batch as DenseBatch
from test_gpu_dense import clouds_of, model_aligned, twin_front_scans
from test_gpu_front_outputs import batch_readouts, same
from test_gpu_parity import run_batch

pytestmark = pytest.mark.gpu
KEYS = ("status", "n_roi", "n_rings", "n_ring_pts", "n_road", "n_curb", "n_ring10")
FIELDS = [k for k, _ in u.ScanInfo._fields_]
CAPACITY = 64 * 2048


def check(labels, infos, scans, p, what=""):
    for k, c in enumerate(scans):
        lb, ib, _ = FS.stages(c, p)
        assert np.array_equal(labels[k], lb), "%s, scan %d: %d labels differ" % (what, k, int((labels[k] != lb).sum()))
        assert dict(zip(KEYS, (int(v) for v in infos[k][:7]))) == {f: ib[f] for f in KEYS}, "%s, scan %d" % (what, k)
        assert infos[k][7] == 0, "%s, scan %d: NaN azimuths counted" % (what, k)


def batch_call(ctx, scans, p, calls=2):
    ragged = len({len(c[0]) for c in scans}) > 1
    for _ in range(calls):
        labels, infos = run_batch(ctx, scans, p, ragged=ragged)
    return labels, infos, ctx.front_scans()


def n_fused(scans, p, max_points, layout="firing"):
    """What the multi-sector kernels keep of a batch on a context of max_points: front_shape.fusable, and a candidate list that holds the
    scan's entries (front_shape.fits)."""
    return sum(FS.fusable(c, p, layout) and FS.fits(c, p, max_points, len(scans), layout) for c in scans)


# ---- 1. dense x multi-sector ----
def dense_context(name):
    """Sized as tests/test_gpu_dense.context explains: the candidate list needs 64 x 2048 points for 64 lasers."""
    L = XC.dense_lasers(name)
    ctx = u.Context(L * {16: 320, 32: 320, 64: 2048, 128: 300}[L], 3)
    if L == 128:
        ctx.set_front_lasers128(1)
    if L != 64:
        ctx.set_front_curb_points(1)
    return ctx


def dense_equal_to_b(got, scans, p, what):
    """Oracle B on the dense points: labels and all eight info words."""
    for k, sc in enumerate(scans):
        lb, ib, _ = FS.stages(sc[0], p)
        assert np.array_equal(got[0][k], lb), "%s, scan %d: %d labels differ" % (what, k, int((got[0][k] != lb).sum()))
        assert [int(v) for v in got[1][k].astype(np.int64)] == [ib[f] for f in FIELDS], (what, k)


def dense_case(name, K=360, cp=5, all_runs=True):
    L, W = XC.dense_lasers(name), XC.dense_width(name)
    p = XC.dense_params(name, K, cp)
    scans = XC.dense_scans(name)
    clouds, ids = [s[0] for s in scans], [s[1] for s in scans]
    want = sum(FS.fusable(s[4], p) for s in scans)
    assert want == len(scans)   # (the gate: every twin can be fused)
    with dense_context(name) as ctx:
        ctx.set_front_mode(2 if cp == 5 else 3)
        ctx.set_front_multi_sector(1)
        ctx.set_front_multi_sector_curb_points(int(cp != 5))
        ctx.set_params(p)
        ctx.set_dense_slots(None)
        nf_twin = twin_front_scans(ctx, clouds, ids, L, W)
        assert nf_twin == want, "padded twins through classify_batch_soa: %d fused, %d fusable" % (nf_twin, want)
        b = DenseBatch(clouds, ids)
        aligned = model_aligned(ids, L, W)
        assert aligned == len(scans)
        runs = [("soa u8", lambda: b.soa_dense(ctx, W, np.uint8)), ("pc2 32 u16@20", lambda: b.pc2_dense(ctx, W, 32, 20, np.uint16))]
        if all_runs:
            runs += [("soa u16", lambda: b.soa_dense(ctx, W, np.uint16)), ("pc2 15 u8@13", lambda: b.pc2_dense(ctx, W, 15, 13, np.uint8))]   # (an odd stride)
        for what, run in runs:
            got = run()
            dense_equal_to_b(got, scans, p, "%s K %d curbPoints %d, %s" % (name, K, cp, what))
            assert got[2] == nf_twin, (what, got[2], nf_twin)
            assert got[3] == aligned, (what, got[3])
        ctx.set_front_multi_sector(0)   # the switch off on the same context: the plain kernels hand every such sweep back
        for what, run in runs[:2]:
            run()
            got = run()
            dense_equal_to_b(got, scans, p, "%s, switch off, %s" % (name, what))
            assert got[2] == 0 and got[3] == aligned, (what, got[2:])


@pytest.mark.parametrize("name", sorted(XC.DENSE))
def test_dense_sweeps_of_real_geometries(name):
    dense_case(name)


@pytest.mark.parametrize("name", ("hdl64e", "vlp16"))
def test_dense_sweeps_at_other_curb_points(name):
    """curbPoints 3, front mode 3, urf_set_front_multi_sector_curb_points on."""
    dense_case(name, cp=3, all_runs=False)


@pytest.mark.parametrize("name", ("hdl64e", "vlp32c"))
def test_dense_sweeps_at_1022_sectors(name):
    dense_case(name, K=1022, all_runs=False)


@pytest.mark.parametrize("kind", ("soa", "pc2"))
def test_read_outs_after_a_dense_multi_sector_call(kind):
    """What tests/test_gpu_dense.test_readouts_after_a_dense_call checks: the four clouds in input order equal the ragged call's on the
    same context, the marker points equal oracle B's on the dense points."""
    name = "hdl64e"
    L, W = XC.dense_lasers(name), XC.dense_width(name)
    p = XC.dense_params(name)
    scans = XC.dense_scans(name)
    with dense_context(name) as ctx:
        ctx.set_front_mode(2)
        ctx.set_front_multi_sector(1)
        ctx.set_params(p)
        ctx.set_dense_slots(None)
        b = DenseBatch([s[0] for s in scans], [s[1] for s in scans])
        cap = 3 * b.S * max(b.lens)
        b.soa_ragged(ctx) if kind == "soa" else b.pc2_ragged(ctx)
        want = clouds_of(ctx, kind, b, cap)
        assert want[0].reshape(-1, 4)[:, 0].all() and want[0].reshape(-1, 4)[:, 1].all()   # (road and curb records in every scan)
        for _ in range(2):
            got = b.soa_dense(ctx, W, np.uint8) if kind == "soa" else b.pc2_dense(ctx, W)
        assert got[2] == b.S
        dense_equal_to_b(got, scans, p, "before the read-outs")
        have = clouds_of(ctx, kind, b, cap)
        assert all(np.array_equal(x, y) for x, y in zip(want, have)), "the four clouds in input order"
        assert ctx.front_scans() == b.S and ctx.dense_scans() == b.S
        for k, sc in enumerate(scans):
            mp = FS.stages(sc[0], p)[2]["marker_pts"]
            assert len(mp) > 2
            got_mp = ctx.marker_points(scan=k)
            assert got_mp.shape == mp.shape and np.array_equal(got_mp.view(np.uint32), mp.view(np.uint32)), k
        ctx.set_front_mode(2)   # (the marker points of a fused call ran it again through the general kernels: fused again from here)
        got = b.soa_dense(ctx, W, np.uint16)
        dense_equal_to_b(got, scans, p, "after the read-outs")
        assert got[2] == b.S


# ---- 2. long sweeps x multi-sector ----
def long_context(scans, p, max_points):
    ctx = u.Context(max_points, len(scans))
    if p.channels == 128:
        ctx.set_front_lasers128(1)
    ctx.set_front_mode(2)
    return ctx


def long_steps(scans, p, max_points, layout="firing", all_fused=True):
    """Long switch off: none fused.  Multi-sector off: none.  Both on: what the CPU says (all of them, where the context's candidate
    list holds every sweep's entries) -- on one context, equal to oracle B at every step, the count of the second call."""
    assert all(not SC.clean(c, p, layout) for c in scans)
    fused = n_fused(scans, p, max_points, layout)
    assert fused == (len(scans) if all_fused else 0)   # (the gate; tests/test_front_crossings_cpu.py pins it)
    with long_context(scans, p, max_points) as ctx:
        # (a count of 0 is asserted on a step's first call: what a first call may do is hand MORE back)
        for step, long, ms, want in (("long off", 0, 1, 0), ("multi-sector off", 1, 0, 0), ("both on", 1, 1, fused)):
            ctx.set_front_long_sweeps(long)
            ctx.set_front_multi_sector(ms)
            labels, infos, nf = batch_call(ctx, scans, p, calls=2 if step == "both on" else 1)
            check(labels, infos, scans, p, step)
            assert nf == want, "%s: %d of %d fused, expected %d" % (step, nf, len(scans), want)


@pytest.mark.parametrize("name", sorted(XC.LONG))
def test_long_multi_sector_sweeps_in_firing_order(name):
    long_steps(XC.long_sweeps(name), XC.long_params(name), XC.long_max_points(name))


@pytest.mark.parametrize("name", sorted(XC.LONG))
def test_long_multi_sector_sweeps_row_major(name):
    long_steps(XC.long_rows(name), XC.long_params(name), XC.long_max_points(name), "rows")


def test_a_full_candidate_list_hands_a_long_sweep_back():
    """The 64 x 8192 sweeps have lost four returns of five: the halo in front of every block of the march has holes, and the EDGE items
    that makes -- a few per laser and block, 256 blocks -- are more than the candidate list of a context of 64 x 8192 points holds
    (front_shape.front_candidates against max_points / 8).  Both sweeps are handed back there, with every switch on; on the larger context
    of the two tests above both are fused."""
    name = "64 x 8192"
    scans = XC.long_sweeps(name)
    long_steps(scans, XC.long_params(name), len(scans[0][0]), all_fused=False)


def test_a_ragged_batch_of_129_tiles_and_four():
    p = XC.long_params("64 x 4128")
    long_steps([XC.long_sweeps("64 x 4128")[1], XC.short_sweep(), XC.long_sweeps("64 x 4128")[0]], p, XC.long_max_points("64 x 4128"))


def test_read_outs_behind_a_long_multi_sector_call():
    name = "64 x 4128"
    p = XC.long_params(name)
    scans = XC.long_sweeps(name)
    b = Batch(scans)   # (the read-outs read the caller's input: it stays on the device)
    assert n_fused(scans, p, XC.long_max_points(name)) == len(scans)
    with long_context(scans, p, XC.long_max_points(name)) as ctx:
        ctx.set_params(p)
        ctx.set_front_long_sweeps(1)
        ctx.set_front_multi_sector(1)
        ctx.set_front_outputs(1)
        for _ in range(2):
            labels, infos = b.classify(ctx, "soa")
        check(labels, infos, scans, p)
        assert ctx.front_scans() == len(scans)
        for s, got in enumerate(batch_readouts(ctx, len(scans), len(scans[0][0]))):
            st = FS.stages(scans[s], p)[2]
            assert len(st["marker_pts"]) > 2
            same(got, st, (name, s))
        assert ctx.front_scans() == len(scans)   # (no second run through the general kernels)


# ---- 4. histories on one long-lived context ----
class Runner:
    """A context, its last parameters, a check against front_shape.stages."""

    def __init__(self, max_points, max_batch):
        self.ctx = u.Context(max_points, max_batch)
        self.p, self.calls_at_p = None, 0

    def close(self):
        self.ctx.close()

    def batch(self, scans, p, what):
        if self.p is None or bytes(p) != bytes(self.p):
            self.p, self.calls_at_p = p.copy(), 0
        labels, infos, nf = batch_call(self.ctx, scans, p, calls=1)
        self.calls_at_p += 1
        check(labels, infos, scans, p, what)
        return nf


@pytest.mark.parametrize("walk", ((360, 1022, 1, 90, 360), (360, 90, 1, 1022, 360)))
def test_history_sector_walk(walk):
    """The tsoff row stride changes with every urf_set_params.  At every K two rounds of two calls on one context with the switch on: a
    batch of two "64 offsets" sweeps (two times in three with an unorganised scan behind them), then a batch of the same geometry without
    offsets, which the plain rule keeps too -- a multi-sector call and a plain one take turns over the same tsoff rows and front_skey.
    From each K's second round on: both sweeps of either call fused, the unorganised scan never (front_shape.fusable)."""
    name = "64 offsets"
    multi, plain, shuffled = small_sweeps(name), XC.plain_twins(), XC.shuffled_sweep()
    r = Runner(CAPACITY, 3)
    try:
        r.ctx.set_front_mode(2)
        r.ctx.set_front_multi_sector(1)
        n = 0
        for K in walk:
            p = SC.at_k(small_params(name), K)
            for rnd in range(2):
                for what, scans in (("multi-sector", multi + ([shuffled] if n % 3 != 1 else [])), ("plain", plain)):
                    want = n_fused(scans, p, CAPACITY)
                    assert want == 2
                    nf = r.batch(scans, p, "K %d, round %d, %s" % (K, rnd, what))
                    assert rnd == 0 or nf == want, "K %d, round %d, %s call: %d fused, %d expected" % (K, rnd, what, nf, want)
                n += 1
    finally:
        r.close()


def test_history_dense_between_multi_sector_batches():
    """A long dense call, a multi-sector batch, a dense call of fewer and shorter scans with a sweep of the callback path in flight across
    it, the batch again -- all with the switch on.  The shorter dense call must not see the longer one's points in its staging."""
    p = XC.dense_params("hdl64e")
    long_d, short_d = XC.dense_scans("hdl64e"), XC.short_dense_scans()
    batch = small_sweeps("64 offsets") + [XC.ideal_sweep()]
    one = XC.rows_of(small_sweeps("64 offsets")[0], 64)
    rec = np.zeros((len(one[0]), 4), np.float32)
    rec[:, 0], rec[:, 1], rec[:, 2] = one
    with u.Context(CAPACITY, 3, params=p) as ctx:
        ctx.set_front_mode(2)
        ctx.set_front_multi_sector(1)
        bl = DenseBatch([s[0] for s in long_d], [s[1] for s in long_d])
        bs = DenseBatch([s[0] for s in short_d], [s[1] for s in short_d])
        for _ in range(2):
            got = bl.soa_dense(ctx, XC.dense_width("hdl64e"), np.uint16)
        dense_equal_to_b(got, long_d, p, "long dense")
        assert got[2] == len(long_d) and got[3] == len(long_d)
        labels, infos, nf = batch_call(ctx, batch, p)
        check(labels, infos, batch, p, "batch")
        assert nf == len(batch)
        t = ctx.classify_pc2_async(rec.view(np.uint8).reshape(-1), len(rec), 16, 0, 4, 8)   # in flight across the dense call
        got = bs.pc2_dense(ctx, XC.SHORT_W)
        lab = np.zeros(len(rec), np.uint8)
        info = ctx.classify_pc2_wait(t, lab)
        dense_equal_to_b(got, short_d, p, "short dense after long")
        assert got[3] == len(short_d)
        lb, ib, _ = FS.stages(one, p)
        assert np.array_equal(lab, lb) and info.n_road == ib["n_road"] and info.n_curb == ib["n_curb"]
        got = bs.soa_dense(ctx, XC.SHORT_W, np.uint8)
        dense_equal_to_b(got, short_d, p, "short dense again")
        assert got[2] == len(short_d)   # (its second call: every twin is fusable, tests/test_front_crossings_cpu.py)
        labels, infos, nf = batch_call(ctx, batch, p)
        check(labels, infos, batch, p, "batch again")
        assert nf == len(batch)
        got = bl.pc2_dense(ctx, XC.dense_width("hdl64e"))
        dense_equal_to_b(got, long_d, p, "long dense again")


def test_history_switch_walk():
    """Front mode 3, curbPoints 3, then 5: the two multi-sector switches walked on one context.  Around each step a call of ideal sweeps and a
    call of sweeps with firings in several sectors; labels always, and from a step's second call on the count urf_policy::plan decides from
    the settings alone (front_crossing_cases.SWITCH_PLAN, read off plan() on the CPU): the ideal sweeps wherever front is set, the others
    wherever front_ms is."""
    name = "64 offsets"
    ideal, multi = XC.plain_twins(), small_sweeps(name)   # (the same ring count in either call: k_ring_table's hint holds)
    r = Runner(CAPACITY, 2)
    try:
        r.ctx.set_front_mode(3)
        for (ms, ms_cp, cp), (front, front_ms) in zip(XC.SWITCH_WALK, XC.SWITCH_PLAN):
            p = small_params(name)
            p.curbPoints = cp
            r.ctx.set_front_multi_sector(ms)
            r.ctx.set_front_multi_sector_curb_points(ms_cp)
            for rep in range(2):
                for what, scans, want in (("ideal", ideal, 2 * front), ("multi-sector", multi, 2 * front_ms)):
                    nf = r.batch(scans, p, "%s, switches %d %d, curbPoints %d, call %d" % (what, ms, ms_cp, cp, rep))
                    assert nf == want or (rep == 0 and nf <= want), "%s, switches %d %d, curbPoints %d, call %d: %d fused, %d expected" % (what, ms, ms_cp, cp, rep, nf, want)
    finally:
        r.close()


# ---- 3. 128 lasers, multi-sector fuzz ----
_FUZZ128_NF = {}


def fuzz128_run(seed, compare=True):
    cloud, p, kind = XC.fuzz128_case(seed)
    with u.Context(max(CAPACITY, len(cloud[0])), 1) as ctx:
        ctx.set_front_lasers128(1)
        ctx.set_front_curb_points(1)
        ctx.set_front_long_sweeps(1)
        ctx.set_front_mode(3)
        ctx.set_front_multi_sector(1)
        ctx.set_front_multi_sector_curb_points(1)
        for _ in range(2):
            labels, infos, nf = batch_call(ctx, [cloud], p, calls=1)
            if compare:
                check(labels, infos, [cloud], p, "%s, K %d, curbPoints %d (fused %d)" % (kind, p.sectors, p.curbPoints, nf))
    _FUZZ128_NF[seed] = nf


@pytest.mark.parametrize("seed", range(20))
def test_fuzzed_128_laser_sweeps(seed):
    """A random 128-laser model with azimuth offsets or drift, world, encoding mix, start azimuth, region of interest, detector parameters,
    curbPoints 1..8 and sector count (front_crossing_cases.fuzz128_case), every switch on, two calls."""
    fuzz128_run(seed)


def test_some_fuzzed_128_laser_sweep_was_fused():
    """(a gate that lets none of them through would pass everything above)"""
    for seed in range(20):
        if seed not in _FUZZ128_NF:   # (run on its own)
            fuzz128_run(seed, compare=False)
        if _FUZZ128_NF[seed]:
            break
    assert any(_FUZZ128_NF.values())
