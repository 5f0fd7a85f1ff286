"""urf_set_sweep_outputs: a sweep of the callback path brings its marker points and its ordered lists along -- produced by the sweep's own
captured launch sequence on its own scratch row, copied to result buffers of its slot, read per ticket after urf_classify_pc2_wait
(urf_result_marker_points / urf_result_ordered_indices) with no further GPU work.  Every marker point and every list against oracle B
(marker_pts, road_order, curb_order, ring10_order), exact: four sweeps in flight on 1, 2 and 4 scratch rows (the parent answers
URF_ERR_BUSY there), each bit alone, full rings, equal azimuths (the literal quicksort and the literal marker pass; rings beyond 2048
points), voided sweeps and their reruns, a sweep below the 30-point threshold, fused row-major sweeps with urf_set_front_outputs off and
on, a parameter change between submissions, the old read-outs next to the new ones, the refusals, a batch call afterwards."""
import numpy as np
import pytest

import oracles as O
import urban_road_filter_amd as u
from hipmem import DevBuf
from test_gpu_async import records
from test_gpu_front import ring_major
from test_gpu_front_outputs import Soa, batch_readouts, check_labels, lasers_params, nudged, repeated_firings, same

pytestmark = pytest.mark.gpu
N = 64 * 2048
BOTH = u.SWEEP_OUT_MARKER_POINTS | u.SWEEP_OUT_ORDER
_REF = {}


def ref(key, cloud, p):
    """Oracle B on one input, computed once (labels, summary, stages); never modified."""
    if key not in _REF:
        _REF[key] = O.run_b(*cloud, p, debug=True)
    return _REF[key]


def wide():
    return u.default_params().wide_roi()


def small(k):
    """Four different 64 x 256 sweeps: scenes 1 and 3."""
    scene, seed = [(1, 31), (3, 32), (1, 33), (3, 34)][k]
    return ("64x256", scene, seed), u.synth_cloud(64, 256, scene, seed)


def submit(ctx, cloud):
    return ctx.classify_pc2_async(records(*cloud), len(cloud[0]), 32, 0, 4, 8)


def collect(ctx, t, n):
    lab = np.empty(n, np.uint8)
    info = ctx.classify_pc2_wait(t, lab)
    return lab, info


def results(ctx, t):
    return ctx.result_ordered_indices(t) + (ctx.result_marker_points(t),)


def check_ticket(ctx, t, cloud, r, what):
    lab, info = collect(ctx, t, len(cloud[0]))
    assert info.status == r[1]["status"] == 0, what
    assert np.array_equal(lab, r[0]), what
    assert (info.n_road, info.n_curb, info.n_ring10) == (r[1]["n_road"], r[1]["n_curb"], r[1]["n_ring10"]), what
    same(results(ctx, t), r[2], what)


# ---- 1. four in flight on 1, 2 and 4 rows ----
@pytest.mark.parametrize("rows", [1, 2, 4])
def test_four_sweeps_in_flight(rows):
    p = wide()
    named = [small(k) for k in range(4)]
    refs = [ref(k, c, p) for k, c in named]
    assert all(r[1]["status"] == 0 and r[1]["n_road"] > 1000 and len(r[2]["marker_pts"]) > 50 for r in refs)
    assert len({r[0].tobytes() for r in refs}) == 4
    with u.Context(64 * 256, rows, params=p) as ctx:
        ctx.set_sweep_outputs(BOTH)
        for rep in range(2):   # (captured, then replayed)
            tickets = [submit(ctx, c) for _, c in named]   # all of them before any is waited for
            for k, t in enumerate(tickets):
                check_ticket(ctx, t, named[k][1], refs[k], (rows, rep, k))
            for k, t in enumerate(tickets):   # ... and every ticket's results are still there after the last one has been waited for
                same(results(ctx, t), refs[k][2], (rows, rep, k, "again"))


# ---- 2. each bit alone, both, and off again ----
def test_each_bit_alone_both_and_off():
    p = wide()
    key, cloud = small(0)
    r = ref(key, cloud, p)
    n = len(cloud[0])
    seen = []
    with u.Context(n, 2, params=p) as ctx:
        for bits in (0, u.SWEEP_OUT_MARKER_POINTS, u.SWEEP_OUT_ORDER, BOTH, 0):
            ctx.set_sweep_outputs(bits)
            t = submit(ctx, cloud)
            lab, info = collect(ctx, t, n)
            assert np.array_equal(lab, r[0])
            seen.append((lab.tobytes(), tuple(info.as_dict().items()), ctx.callback_path_state()))
            for bit, call, want in ((u.SWEEP_OUT_MARKER_POINTS, ctx.result_marker_points, "URF_SWEEP_OUT_MARKER_POINTS"),
                                    (u.SWEEP_OUT_ORDER, ctx.result_ordered_indices, "URF_SWEEP_OUT_ORDER")):
                if bits & bit:
                    continue
                with pytest.raises(u.UrfError) as e:
                    call(t)
                assert e.value.code == -1 and "urf_set_sweep_outputs" in str(e.value) and want in str(e.value), (bits, str(e.value))
            if bits & u.SWEEP_OUT_MARKER_POINTS:
                mk = ctx.result_marker_points(t)
                assert mk.shape == r[2]["marker_pts"].shape and np.array_equal(mk.view(np.uint32), r[2]["marker_pts"].view(np.uint32)), bits
            if bits & u.SWEEP_OUT_ORDER:
                for got, name in zip(ctx.result_ordered_indices(t), ("road_order", "curb_order", "ring10_order")):
                    assert np.array_equal(got, r[2][name]), (bits, name)
    assert all(s == seen[0] for s in seen)   # labels, summaries and callback_path_state: identical in all settings


# ---- 3. full rings: exactly 2048 points, the upper edge of the branch that sorts in LDS ----
def test_full_rings():
    p = O.cfg_params("cfg2")
    cloud = O.cfg_cloud("cfg2", 1)
    r = ref(("cfg2", 1), cloud, p)
    lens = np.bincount(r[2]["ring"][r[2]["ring"] >= 0])
    assert len(lens) == 64 and min(lens) == max(lens) == 2048
    with u.Context(N, 4, params=p) as ctx:
        ctx.set_sweep_outputs(BOTH)
        check_ticket(ctx, submit(ctx, cloud), cloud, r, "full rings")


# ---- 4. equal azimuths ----
@pytest.mark.parametrize("variant", ["repeated", "nudged"])
def test_equal_azimuths(variant):
    """Every 8th firing a copy of the one before: the literal quicksort decides the published order; in the nudged twin the order of a
    pair with one azimuth and one distance decides marker points (the literal marker pass)."""
    p = O.cfg_params("cfg2")
    key, cloud = ("cfg2", 1, "repeated8"), repeated_firings(O.cfg_cloud("cfg2", 1), 8)
    if variant == "nudged":
        key, cloud = ("cfg2", 1, "nudged8"), nudged(O.cfg_cloud("cfg2", 1), 8, ref(key, cloud, p)[2])
    r = ref(key, cloud, p)
    with u.Context(N, 1, params=p) as ctx:
        ctx.set_sweep_outputs(BOTH)
        check_ticket(ctx, submit(ctx, cloud), cloud, r, ("equal azimuths", variant))
        for bits in (u.SWEEP_OUT_MARKER_POINTS, u.SWEEP_OUT_ORDER):   # ... and from the kernels of one product alone
            ctx.set_sweep_outputs(bits)
            t = submit(ctx, cloud)
            collect(ctx, t, N)
            if bits == u.SWEEP_OUT_ORDER:
                got = ctx.result_ordered_indices(t)
                assert all(np.array_equal(g, r[2][name]) for g, name in zip(got, ("road_order", "curb_order", "ring10_order")))
            else:
                assert np.array_equal(ctx.result_marker_points(t).view(np.uint32), r[2]["marker_pts"].view(np.uint32))


@pytest.mark.parametrize("variant", ["repeated", "nudged"])
def test_long_rings_with_equal_azimuths(variant):
    """16 x 2176: rings longer than the 2048 points that sort in LDS, channels 16."""
    p = lasers_params(16)
    key, cloud = ("16x2176", 1, "repeated8"), repeated_firings(u.synth_cloud(16, 2176, 1, 5), 8, 16)
    if variant == "nudged":
        key, cloud = ("16x2176", 1, "nudged8"), nudged(u.synth_cloud(16, 2176, 1, 5), 8, ref(key, cloud, p)[2], 16)
    r = ref(key, cloud, p)
    lens = np.bincount(r[2]["ring"][r[2]["ring"] >= 0])
    assert len(lens) == 16 and min(lens) == 2176
    with u.Context(len(cloud[0]), 2, params=p) as ctx:
        ctx.set_sweep_outputs(BOTH)
        check_ticket(ctx, submit(ctx, cloud), cloud, r, ("long rings", variant))


# ---- 5. voided sweeps ----
def test_voided_sweeps_bring_the_results_of_their_rerun():
    """One scratch row.  (i) a ring point on the sensor's axis (x = y = 0: a NaN azimuth, k_nan_rings) with a second sweep in flight
    behind it; (ii) in the same context, a sensor-like sweep with equal planar ranges in every star sector (k_star_ties).  Either is
    voided by the short sequence and run again inside urf_classify_pc2_wait: its results are the rerun's, the sweep behind it keeps
    its own."""
    p = O.cfg_params("cfg2")
    first = list(O.cfg_cloud("cfg2", 120))
    for a, v in zip(first, (0.0, 0.0, -1.8)):
        a[5000] = v
    second = O.cfg_cloud("narrow", 121)
    ties = O.cfg_cloud("sensor", 1)
    wa, wb, wt = ref(("cfg2", 120, "axis"), first, p), ref(("narrow", 121), second, p), ref(("sensor", 1), ties, p)
    with u.Context(N, 1, params=p) as ctx:
        ctx.set_sweep_outputs(BOTH)
        assert ctx.callback_path_state()[0] == 0
        ta, tb = submit(ctx, first), submit(ctx, second)
        check_ticket(ctx, ta, first, wa, "axis point")
        n1 = ctx.callback_path_state()[0]
        assert n1 >= 1                                  # voided and run again
        check_ticket(ctx, tb, second, wb, "behind the voided sweep")
        same(results(ctx, ta), wa[2], "axis point, after the sweep behind it")
        tt, tb = submit(ctx, ties), submit(ctx, second)
        check_ticket(ctx, tt, ties, wt, "range ties")
        n2, seq = ctx.callback_path_state()
        assert n2 > n1 and seq & 16                     # voided for its range ties: k_star_ties in the sequence from now on
        check_ticket(ctx, tb, second, wb, "behind the second voided sweep")


# ---- 6. too few points ----
def test_a_sweep_below_the_threshold_publishes_nothing():
    p = O.cfg_params("cfg2")
    few = tuple(a.copy() for a in O.cfg_cloud("cfg2", 6))
    few[0][29:] = 1.0e6
    nxt = O.cfg_cloud("narrow", 4)
    rf, rn = ref(("cfg2", 6, "few"), few, p), ref(("narrow", 4), nxt, p)
    assert rf[1]["status"] != 0
    with u.Context(N, 2, params=p) as ctx:
        ctx.set_sweep_outputs(BOTH)
        for rep in range(2):
            tf, tn = submit(ctx, few), submit(ctx, nxt)
            lab, info = collect(ctx, tf, N)
            assert info.status == rf[1]["status"] and np.array_equal(lab, rf[0])
            road, curb, r10, mk = results(ctx, tf)
            assert (len(road), len(curb), len(r10), mk.shape) == (0, 0, 0, (0, 4))
            check_ticket(ctx, tn, nxt, rn, ("behind the short sweep", rep))


# ---- 7. fused row-major sweeps ----
@pytest.mark.parametrize("front_outputs", [0, 1])
def test_fused_row_major_sweeps(front_outputs):
    p = wide()
    named = [(("64x256", 1, seed, "rows"), ring_major(u.synth_cloud(64, 256, 1, seed))) for seed in (7, 31, 33, 35)]
    refs = [ref(k, c, p) for k, c in named]
    assert all(r[1]["status"] == 0 and r[1]["n_road"] > 1000 for r in refs)
    n = 64 * 256
    with u.Context(n, 4, params=p) as ctx:
        ctx.set_front_outputs(front_outputs)
        ctx.set_sweep_outputs(BOTH)
        fused = []
        for rep in range(3):   # the first sweep only sights the layout; fused from the second or third on
            lab, info = collect(ctx, submit(ctx, named[0][1]), n)
            assert np.array_equal(lab, refs[0][0])
            fused.append(ctx.front_scans())
        assert fused[2] == 1, fused
        for rep in range(2):
            tickets = [submit(ctx, c) for _, c in named]
            for k, t in enumerate(tickets):
                assert ctx.front_scans() == 1                      # before ...
                check_ticket(ctx, t, named[k][1], refs[k], ("rows", front_outputs, rep, k))
                assert ctx.front_scans() == 1                      # ... and after: no second run, the next sweep is fused again
                why = ctx.front_explain(layout=1)
                assert len(why) == 1 and why[0]["fused"] == 1 and not (why[0]["call"] & u.WHY_CALL["READOUT"]), why


# ---- 8. parameter change between submissions ----
def test_each_ticket_follows_the_parameters_it_was_submitted_under():
    p5 = wide()
    p9 = wide()
    p9.curbPoints = 9
    key, cloud = small(1)
    r5, r9 = ref(key, cloud, p5), ref(key + ("cp9",), cloud, p9)
    assert not np.array_equal(r5[0], r9[0]) and r9[1]["status"] == 0
    n = len(cloud[0])
    with u.Context(n, 4, params=p5) as ctx:
        ctx.set_sweep_outputs(BOTH)
        t5 = submit(ctx, cloud)
        ctx.set_params(p9)
        t9 = submit(ctx, cloud)
        ctx.set_params(p5)
        t5b = submit(ctx, cloud)
        check_ticket(ctx, t5, cloud, r5, "curbPoints 5")
        check_ticket(ctx, t9, cloud, r9, "curbPoints 9")
        check_ticket(ctx, t5b, cloud, r5, "curbPoints 5 again")


# ---- 9. the old read-outs ----
def test_the_old_readouts_agree_with_the_tickets_results():
    p = wide()
    key, cloud = small(2)
    r = ref(key, cloud, p)
    n = len(cloud[0])
    with u.Context(n, 4, params=p) as ctx:
        ctx.set_sweep_outputs(BOTH)
        t = submit(ctx, cloud)
        collect(ctx, t, n)
        new = results(ctx, t)
        old = ctx.ordered_indices(n) + (ctx.marker_points(),)
        for a, b in zip(new, old):
            assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))   # element by element
        same(new, r[2], "after the old read-outs")   # (the pinned buffer is nobody else's)
        assert np.array_equal(ctx.read_stage(u.STAGE_DETECT, n), r[2]["detect"])


# ---- 10. refusals ----
def test_refusals():
    p = wide()
    clouds = [small(k)[1] for k in range(4)]
    n = len(clouds[0][0])
    with u.Context(n, 2, params=p) as ctx:
        for call in (ctx.result_marker_points, ctx.result_ordered_indices):   # no ticket yet
            with pytest.raises(u.UrfError) as e:
                call(0)
            assert e.value.code == -1
        t_off = submit(ctx, clouds[0])                     # submitted with the switch off
        with pytest.raises(u.UrfError) as e:
            ctx.set_sweep_outputs(BOTH)                    # ... and the switch does not change under a sweep in flight
        assert e.value.code == -7
        collect(ctx, t_off, n)
        for call in (ctx.result_marker_points, ctx.result_ordered_indices):
            with pytest.raises(u.UrfError) as e:
                call(t_off)
            assert e.value.code == -1 and "urf_set_sweep_outputs" in str(e.value)
        ctx.set_sweep_outputs(BOTH)
        t0 = submit(ctx, clouds[0])
        for call in (ctx.result_marker_points, ctx.result_ordered_indices):   # in flight
            with pytest.raises(u.UrfError) as e:
                call(t0)
            assert e.value.code == -7
        for bits in (0, u.SWEEP_OUT_ORDER):
            with pytest.raises(u.UrfError) as e:
                ctx.set_sweep_outputs(bits)
            assert e.value.code == -7
        collect(ctx, t0, n)
        ctx.result_marker_points(t0)
        later = [submit(ctx, c) for c in clouds]           # four submissions later the slot holds another sweep
        for t in later:
            collect(ctx, t, n)
        for call in (ctx.result_marker_points, ctx.result_ordered_indices):   # overtaken, and never issued
            for t in (t0, later[-1] + 1):
                with pytest.raises(u.UrfError) as e:
                    call(t)
                assert e.value.code == -1
        assert ctx._lib.urf_result_ordered_indices(ctx._h, later[0], None, None, None, None) == -1
        cnt = (np.zeros(3, np.uint32))
        assert ctx._lib.urf_result_ordered_indices(ctx._h, later[0], None, None, None, cnt.ctypes.data) == 0   # unwanted lists: NULL
        assert cnt[0] > 0


# ---- 11. a batch call afterwards ----
def test_a_batch_call_after_sweeps_with_the_switch_on():
    p = wide()
    named = [small(k) for k in range(4)]
    refs = [ref(k, c, p) for k, c in named]
    n = 64 * 256
    b = Soa([c for _, c in named])
    with u.Context(n, 4, params=p) as ctx:
        ctx.set_sweep_outputs(BOTH)
        tickets = [submit(ctx, c) for _, c in named]
        for k, t in enumerate(tickets):
            check_ticket(ctx, t, named[k][1], refs[k], k)
        b.classify(ctx)
        switched = (b.label_bytes(), batch_readouts(ctx, 4, n))
    with u.Context(n, 4, params=p) as ctx:
        b.classify(ctx)
        fresh = (b.label_bytes(), batch_readouts(ctx, 4, n))
    assert np.array_equal(switched[0], fresh[0])
    for s in range(4):
        assert np.array_equal(switched[0][s * n:(s + 1) * n], refs[s][0])
        same(switched[1][s], refs[s][2], ("batch after sweeps", s))
        for a, c in zip(switched[1][s], fresh[1][s]):
            assert np.array_equal(a.view(np.uint32), c.view(np.uint32))


# ---- 12. both users of the read-out launcher in one context ----
def shuffled(cloud, seed):
    """The sweep's points in random order: no firing order, no rows -- the fused front end hands such a scan back."""
    perm = np.random.RandomState(seed).permutation(len(cloud[0]))
    return tuple(np.ascontiguousarray(a[perm]) for a in cloud)


@pytest.mark.parametrize("direct", [0, 1])
def test_the_callback_path_and_the_batch_read_backs_share_one_launcher(direct):
    """64 x 256 sweeps.  A sweep of the callback path with both products (captured); a fused batch of three scans whose middle one is
    unorganised and handed back; urf_ordered_indices for each scan (the launcher from scan 0, 1 and 2) and urf_marker_points_batch; the
    first sweep again, five times: once per slot and then in a slot that has captured it, a replay.  Every list and every marker point against oracle B, exact; the replay against the first
    result, exact.  (A context of three scans: the batch needs three rows; its four slots still share them -- slot 3 runs on row 0.)"""
    p = wide()
    n = 64 * 256
    key, sweep = small(0)
    rs = ref(key, sweep, p)
    named = [small(1), (("64x256", 3, 32, "shuffled"), shuffled(small(1)[1], 5)), small(2)]
    refs = [ref(k, c, p) for k, c in named]
    assert all(r[1]["status"] == 0 and r[1]["n_road"] > 1000 and len(r[2]["marker_pts"]) > 50 for r in refs + [rs])
    b = Soa([c for _, c in named])
    with u.Context(n, 3, params=p) as ctx:
        ctx.set_front_mode(2)
        ctx.set_front_outputs(1)
        ctx.set_sweep_outputs(BOTH)
        ctx.set_sweep_results_direct(direct)
        t = submit(ctx, sweep)
        check_ticket(ctx, t, sweep, rs, ("captured", direct))
        first = [a.copy() for a in results(ctx, t)]
        assert ctx.callback_path_captures()[0] == 1
        b.classify(ctx)
        assert ctx.front_scans() == 2                      # the middle scan went back to the general kernels
        check_labels(b, refs)
        for s in range(3):
            got = ctx.ordered_indices(n, scan=s)
            for g, name in zip(got, ("road_order", "curb_order", "ring10_order")):
                assert np.array_equal(g, refs[s][2][name]), (direct, s, name)
        dpts, dn = DevBuf(16 * 361 * 3), DevBuf(4 * 3)
        dpts.fill(0xEE)
        dn.fill(0xEE)
        ctx.marker_points_batch(dpts, dn)
        ctx.synchronize()
        pts, cnt = dpts.to_numpy(np.float32).reshape(3, 361, 4), dn.to_numpy(np.uint32)
        for s in range(3):
            want = refs[s][2]["marker_pts"]
            assert cnt[s] == len(want) and np.array_equal(pts[s][:cnt[s]].view(np.uint32), want.view(np.uint32)), (direct, s)
        assert ctx.front_scans() == 2                      # (no second run of the batch)
        # Submissions take the four slots in turn (the first sweep took slot 0), each slot keeps its own sequences, and what the batch
        # reported may have bumped the epoch: reps 0-3 go to slots 1, 2, 3, 0 and may each capture; rep 4 is back in slot 1, which
        # captured at rep 0 under the epoch that has stood since the batch, so it must replay.
        for rep in range(5):
            before = ctx.callback_path_captures()[0]
            t = submit(ctx, sweep)
            check_ticket(ctx, t, sweep, rs, ("again", direct, rep))
            for a, f in zip(results(ctx, t), first):
                assert a.shape == f.shape and np.array_equal(a.view(np.uint32), f.view(np.uint32)), (direct, rep)
            assert rep < 4 or ctx.callback_path_captures()[0] == before, "rep 4: a replay"


# ---- 13. the A/B switch of the build with the test hooks ----
def test_both_bits_with_the_kernels_of_each_product_alone():
    """Debug flag 32 (include/urf_test_hooks.h): both bits set, the sequence launches k_ring_order, k_marker_ring, k_ordered_lists and
    k_marker_bins one by one instead of k_sweep_rings / k_sweep_lists -- the arm tools/sweep_outputs_bench.py measures against."""
    p = wide()
    named = [small(k) for k in range(2)]
    refs = [ref(k, c, p) for k, c in named]
    with u.Context(64 * 256, 2, params=p, hooks=True) as ctx:
        ctx._check(ctx._lib.urf_set_debug_flags(ctx._h, 32), "urf_set_debug_flags")
        ctx.set_sweep_outputs(BOTH)
        tickets = [submit(ctx, c) for _, c in named]
        for k, t in enumerate(tickets):
            check_ticket(ctx, t, named[k][1], refs[k], ("one by one", k))
