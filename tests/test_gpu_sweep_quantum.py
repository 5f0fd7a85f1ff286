"""urf_set_sweep_quantum: a sweep of the callback path runs as the next multiple of the quantum, (NaN, NaN, NaN) behind its own points, and
sweeps of varying length replay one captured sequence per padded length.  Every comparison is exact against oracle B on the caller's
UNPADDED points: streams of 12 dense sweeps on 1, 2 and 4 scratch rows with one and four in flight, the edge lengths, the pinned-input
path (aligned and unaligned records), the count of captures (the test with teeth), eviction, the read-outs after a padded sweep, the
rerun inside urf_classify_pc2_wait, changes between sweeps, organised streams, the refusals."""
import numpy as np
import pytest

import oracles as O
import sensor_models as S
import sweep_quantum_cases as Q
import urban_road_filter_amd as u

pytestmark = pytest.mark.gpu
IN_FLIGHT = 4      # URF_MAX_IN_FLIGHT
SEQS = 8           # URF_SWEEP_SEQS
BOTH = u.SWEEP_OUT_MARKER_POINTS | u.SWEEP_OUT_ORDER
FIELDS = ("status", "n_road", "n_curb", "n_roi", "n_rings", "n_ring10", "n_ring_pts")


def submit(ctx, cloud):
    return ctx.classify_pc2_async(Q.records(*cloud), len(cloud[0]), 32, 0, 4, 8)


def collect(ctx, t, n):
    lab = np.full(n + 16, 0xEE, np.uint8)   # (nothing is written behind the caller's n bytes)
    info = ctx.classify_pc2_wait(t, lab)
    assert (lab[n:] == 0xEE).all()
    return lab[:n], info


def check(lab, info, r, what):
    d = info.as_dict()
    assert {f: d[f] for f in FIELDS} == {f: r[1][f] for f in FIELDS}, what
    assert np.array_equal(lab, r[0]), (what, int((lab != r[0]).sum()))


def run_stream(ctx, named, p, in_flight, what):
    """The sweeps with `in_flight` of them on their way, each against oracle B."""
    pending = []

    def wait_oldest():
        j, t = pending.pop(0)
        c = named[j][1]
        check(*collect(ctx, t, len(c[0])), Q.ref(named[j][0], c, p), (what, j))
    for k, (key, cloud) in enumerate(named):
        if len(pending) == in_flight:
            wait_oldest()
        pending.append((k, submit(ctx, cloud)))
    while pending:
        wait_oldest()


def prefix(cloud, n):
    return tuple(a[:n].copy() for a in cloud)


# ---- 1. streams at quantum 2048 ----
@pytest.mark.parametrize("in_flight", [1, 4])
@pytest.mark.parametrize("rows", [1, 2, 4])
def test_streams_of_varying_length(rows, in_flight):
    p = Q.params32()
    named = Q.stream()
    refs = [Q.ref(k, c, p) for k, c in named]
    assert all(r[1]["status"] == 0 and r[1]["n_road"] > 100 and r[1]["n_curb"] > 20 for r in refs)
    assert {Q.padded_len(len(c[0])) for _, c in named} == {4096, 6144}
    with u.Context(8192, rows, params=p) as ctx:
        ctx.set_sweep_quantum(2048)
        for rep in range(2):
            run_stream(ctx, named, p, in_flight, (rows, in_flight, rep))


# ---- 2. edge lengths ----
@pytest.mark.parametrize("n", [4096, 4095, 2049, 1, 29])
def test_edge_lengths(n):
    """A multiple of the quantum (no pad), n' - 1, n' - 2047, and two sweeps below the 30-point threshold (URF_TOO_FEW_POINTS)."""
    p = Q.params32()
    cloud = prefix(Q.dense_sweep("vlp16", 304, 7), n)
    assert len(cloud[0]) == n
    r = Q.ref(("edge", n), cloud, p)
    assert r[1]["status"] == (1 if n < 30 else 0)
    with u.Context(8192, 2, params=p) as ctx:
        ctx.set_sweep_quantum(2048)
        for rep in range(2):
            check(*collect(ctx, submit(ctx, cloud), n), r, (n, rep))
            lab, info = ctx.classify_pc2(Q.records(*cloud), n, 32, 0, 4, 8)   # the synchronous entry point: the same path
            check(lab, info, r, (n, rep, "sync"))


def test_a_sweep_staged_in_two_halves():
    """cfg2 seed 77 cut to 50 000 points (n' 51 200): at or above the 32 768 points from which the planes are staged in two halves."""
    p = O.cfg_params("cfg2")
    cloud = prefix(O.cfg_cloud("cfg2", 77), 50000)
    r = Q.ref(("cfg2", 77, 50000), cloud, p)
    assert r[1]["status"] == 0 and r[1]["n_road"] > 1000 and r[1]["n_curb"] > 100
    with u.Context(51200, 2, params=p) as ctx:
        ctx.set_sweep_quantum(2048)
        for rep in range(2):
            check(*collect(ctx, submit(ctx, cloud), 50000), r, rep)
        assert ctx.callback_path_captures()[0] <= 3   # (captured, perhaps once more for what the first sweep reported, then replayed)


def test_a_padded_length_beyond_max_points_runs_unpadded():
    p = Q.params32()
    cloud = prefix(Q.dense_sweep("vlp16", 304, 7), 4450)
    r = Q.ref(("edge", 4450), cloud, p)
    with u.Context(5000, 2, params=p) as ctx:
        ctx.set_sweep_quantum(4096)   # n' 8192 does not fit
        check(*collect(ctx, submit(ctx, cloud), 4450), r, "4096")
        ctx.set_sweep_quantum(2048)   # n' 6144 does not fit either
        for rep in range(2):
            check(*collect(ctx, submit(ctx, cloud), 4450), r, rep)


# ---- 3. the pinned-input path ----
@pytest.mark.parametrize("step,ox,oy,oz", [(32, 0, 4, 8), (48, 20, 4, 36), (13, 1, 5, 9)], ids=["32", "48", "13_unaligned"])
def test_records_in_the_pinned_input_buffer(step, ox, oy, oz):
    """A producer writes its records into urf_pinned_input's buffer: k_pc2_to_soa_pad gathers them and stores the pad.  Same labels as
    the staged path; of the pinned result buffer only the caller's n bytes are looked at."""
    p = Q.params32()
    named = Q.stream()[:6]
    with u.Context(8192, 4, params=p) as ctx:
        ctx.set_sweep_quantum(2048)
        for rep in range(2):
            for key, cloud in named:
                n = len(cloud[0])
                rec = Q.records(*cloud, step=step, ox=ox, oy=oy, oz=oz, fill=0xA5)
                buf = ctx.pinned_input(len(rec))
                buf[:] = rec
                t = ctx.classify_pc2_async(buf.ctypes.data, n, step, ox, oy, oz)
                info = ctx.classify_pc2_wait(t)
                check(ctx.result_labels(t, n).copy(), info, Q.ref(key, cloud, p), (step, rep, key))
                staged, info2 = ctx.classify_pc2(rec, n, step, ox, oy, oz)
                check(staged, info2, Q.ref(key, cloud, p), (step, rep, key, "staged"))


# ---- 4. counting: the test with teeth ----
def passes(ctx, named, p):
    """(n_captured, n_resident) after a warm pass and after a second pass over the same sweeps, the sequence preset first"""
    ctx.callback_path_preset(2 | 4 | 16)
    run_stream(ctx, named, p, IN_FLIGHT, "warm")
    warm = ctx.callback_path_captures()
    print("after the warm pass: captures %s, (n_rerun, sequence) %s" % (warm, ctx.callback_path_state()))
    run_stream(ctx, named, p, IN_FLIGHT, "second")
    again = ctx.callback_path_captures()
    print("after the second pass: captures %s, (n_rerun, sequence) %s" % (again, ctx.callback_path_state()))
    return warm, again


def test_a_second_pass_captures_nothing():
    """Sequence preset, one warm pass over 12 sweeps, a second pass: with the switch on nothing is captured any more, with it off every
    sweep is (sweep k and sweep k + 4 differ in length).  The 12 sweeps are one sensor's (tests/sweep_quantum_cases.py: stream16), so
    that the preset fixes the sequence: on the mixed vlp16 / hdl32e stream of the other tests the context drops the ring-count hint
    somewhere in its first passes (a 32-laser sweep whose table the hint of a 16-laser one cuts short is run again, and the hint goes:
    sequence bits 31 -> 23 on an MI355X), which forgets the sequences captured until then.  Measured on an MI355X: switch on 8
    captures after the warm pass and 8 after the second, 8 resident; switch off 12 and 24, 4 resident."""
    p = Q.params32()
    named = Q.stream16()
    assert len({Q.ref(k, c, p)[1]["n_rings"] for k, c in named}) == 1
    with u.Context(8192, 4, params=p) as ctx:
        ctx.set_sweep_quantum(2048)
        warm, again = passes(ctx, named, p)
        print("switch on: captured %d after the warm pass, %d after the second; resident %d" % (warm[0], again[0], again[1]))
        assert again[0] == warm[0]
        assert 0 < again[1] <= SEQS * IN_FLIGHT and again[1] <= 2 * IN_FLIGHT   # (two padded lengths per slot)
    with u.Context(8192, 4, params=p) as ctx:
        warm, again = passes(ctx, named, p)
        print("switch off: captured %d after the warm pass, %d after the second; resident %d" % (warm[0], again[0], again[1]))
        assert again[0] == warm[0] + len(named)
        assert again[1] <= IN_FLIGHT   # one sequence per slot


# ---- 5. eviction ----
def test_ten_padded_lengths_through_every_slot():
    """10 distinct n' through each slot, one sweep in flight: a slot keeps URF_SWEEP_SEQS sequences, the least recently used one makes
    room, results are right throughout."""
    p = Q.params32()
    big = Q.dense_sweep("hdl32e", 700, 5)
    assert len(big[0]) > 19456 + 1100
    lens = [2048 * j + 1000 + 7 * j for j in range(10)]
    assert len({Q.padded_len(n) for n in lens}) == 10 and max(Q.padded_len(n) for n in lens) <= 24576
    named = [(("evict", n), prefix(big, n)) for n in lens]
    with u.Context(24576, 4, params=p) as ctx:
        ctx.set_sweep_quantum(2048)
        ctx.callback_path_preset(2 | 4 | 16)
        for rep in range(2):
            for key, cloud in named:
                for slot in range(IN_FLIGHT):   # consecutive tickets: every slot sees every length
                    check(*collect(ctx, submit(ctx, cloud), len(cloud[0])), Q.ref(key, cloud, p), (rep, key, slot))
                    assert ctx.callback_path_captures()[1] <= SEQS * IN_FLIGHT
        n_captured, n_resident = ctx.callback_path_captures()
        assert n_resident == SEQS * IN_FLIGHT
        assert n_captured >= 2 * len(named) * IN_FLIGHT   # ten lengths through eight places, least recently used first: every sweep captured


# ---- 6. read-outs after a padded sweep ----
def test_read_outs_answer_for_the_callers_points():
    from hipmem import DevBuf
    p = Q.params32()
    key, cloud = Q.stream()[0]
    n = len(cloud[0])
    r = Q.ref(key, cloud, p, debug=True)
    assert Q.padded_len(n) != n and len(r[2]["marker_pts"]) > 2 and r[1]["n_road"] > 100
    with u.Context(8192, 4, params=p) as ctx:
        ctx.set_sweep_quantum(2048)
        ctx.enable_stage_capture(2)
        for rep in range(2):
            lab, info = collect(ctx, submit(ctx, cloud), n)
            check(lab, info, r, rep)
            ring = ctx.read_stage(u.STAGE_RING, n)   # n entries, not n'
            assert np.array_equal(ring, r[2]["ring"]), rep
            for got, name in zip(ctx.ordered_indices(n), ("road_order", "curb_order", "ring10_order")):
                assert np.array_equal(got, r[2][name]), (rep, name)
            mk = ctx.marker_points()
            assert mk.shape == r[2]["marker_pts"].shape and np.array_equal(mk.view(np.uint32), r[2]["marker_pts"].view(np.uint32)), rep
            d_lab = DevBuf.from_numpy(lab)
            lists = [DevBuf(4 * n) for _ in range(4)]
            d_cnt = DevBuf(16)
            ctx.compact_indices(d_lab, n, *lists, d_cnt)
            ctx.synchronize()
            cnt = d_cnt.to_numpy(np.uint32)
            assert (int(cnt[0]), int(cnt[1]), int(cnt[2])) == (r[1]["n_road"], r[1]["n_curb"], r[1]["n_roi"]), rep
            why = ctx.front_explain()
            assert len(why) == 1


def test_sweep_outputs_per_ticket_with_four_in_flight():
    p = Q.params32()
    named = Q.stream()[:8]
    with u.Context(8192, 4, params=p) as ctx:
        ctx.set_sweep_quantum(2048)
        ctx.set_sweep_outputs(BOTH)
        for rep in range(2):
            for base in (0, 4):
                tickets = [submit(ctx, c) for _, c in named[base:base + 4]]
                for (key, cloud), t in zip(named[base:base + 4], tickets):
                    n = len(cloud[0])
                    r = Q.ref(key, cloud, p, debug=True)
                    check(*collect(ctx, t, n), r, (rep, key))
                    road, curb, r10 = ctx.result_ordered_indices(t)
                    for got, name in ((road, "road_order"), (curb, "curb_order"), (r10, "ring10_order")):
                        assert np.array_equal(got, r[2][name]) and (got < n).all(), (rep, key, name)
                    mk = ctx.result_marker_points(t)
                    assert mk.shape == r[2]["marker_pts"].shape and np.array_equal(mk.view(np.uint32), r[2]["marker_pts"].view(np.uint32)), (rep, key)


# ---- 7. the rerun inside urf_classify_pc2_wait ----
def axis_cloud():
    """Every second laser of a short 64-laser sweep (the ring table keeps free entries), six points moved onto the sensor's axis: they
    get a ring of their own (tests/test_gpu_parity.py: half_laser_axis_cloud); cut to a length that is no multiple of the quantum."""
    from fuzz import axis_points
    base = tuple(np.ascontiguousarray(a[:16384].reshape(-1, 64)[:, ::2]).reshape(-1) for a in O.cfg_cloud("cfg2", 401))
    return prefix(axis_points(base, np.random.default_rng(1), 6), 8000)


@pytest.mark.parametrize("case", ["ties", "axis"])
def test_a_voided_sweep_is_run_again_with_its_pad(case):
    """A fresh context without preset: a sensor-like sweep with range ties cut to a non-multiple, and a sweep with a ring point on the
    axis.  Both are padded, voided by the short sequence and run again inside the wait; n_rerun is as for the unpadded twin."""
    p = O.cfg_params("cfg2")
    cloud = prefix(O.cfg_cloud("sensor", 1), 50000) if case == "ties" else axis_cloud()
    n = len(cloud[0])
    r = Q.ref(("rerun", case), cloud, p, debug=True)
    assert n % 2048 != 0 and r[1]["status"] == 0 and r[1]["n_road"] + r[1]["n_curb"] > 50
    if case == "axis":
        assert int(((cloud[0] == 0) & (cloud[1] == 0) & (r[2]["ring"] >= 0)).sum()) > 0
    reruns = []
    for quantum in (0, 2048):
        with u.Context(51200, 2, params=p) as ctx:
            ctx.set_sweep_quantum(quantum)
            check(*collect(ctx, submit(ctx, cloud), n), r, (case, quantum))
            reruns.append(ctx.callback_path_state()[0])
            check(*collect(ctx, submit(ctx, cloud), n), r, (case, quantum, "again"))
    print("%s: n_rerun %s" % (case, reruns))
    assert reruns[0] == reruns[1] > 0


# ---- 8. changes between sweeps ----
def test_parameters_and_quantum_change_between_sweeps():
    p = Q.params32()
    p2 = Q.params32(wide=False)
    named = Q.stream()[:4]
    with u.Context(8192, 4, params=p) as ctx:
        def sweep_all(pp, tag):
            for key, cloud in named:
                check(*collect(ctx, submit(ctx, cloud), len(cloud[0])), Q.ref((key, tag), cloud, pp), (tag, key))
        ctx.set_sweep_quantum(2048)
        sweep_all(p, "wide")
        assert ctx.callback_path_captures()[1] > 0
        ctx.set_params(p2)
        assert ctx.callback_path_captures()[1] == 0
        sweep_all(p2, "default")
        assert ctx.callback_path_captures()[1] > 0
        ctx.set_sweep_quantum(0)
        assert ctx.callback_path_captures()[1] == 0
        sweep_all(p2, "default")
        assert 0 < ctx.callback_path_captures()[1] <= IN_FLIGHT
        ctx.set_sweep_quantum(4096)
        assert ctx.callback_path_captures()[1] == 0
        sweep_all(p2, "default")
        before = ctx.callback_path_captures()
        sweep_all(p2, "default")   # 3 478-4 514 points at quantum 4096: n' 4096 or 8192, replayed
        assert ctx.callback_path_captures() == before


# ---- 9. organised streams lose nothing ----
def test_row_major_sweeps_stay_fused_and_a_padded_one_is_right():
    p = S.params_for("os32d")
    sweeps = [S.sweep("os32d", seed=s) for s in (1, 2, 3, 4, 5)]
    assert all(len(c[0]) == 32 * 1024 for c in sweeps)
    odd = S.sweep("os32d", firings=1000, seed=6)   # 32 x 1000 row-major: padded to 32 768
    r_odd = Q.ref(("os32d", 1000, 6), odd, p)
    assert len(odd[0]) == 32000 and r_odd[1]["status"] == 0 and r_odd[1]["n_road"] > 100
    fused = {}
    for quantum in (0, 2048):
        with u.Context(32768, 4, params=p) as ctx:
            ctx.set_front_mode(2)
            ctx.set_sweep_quantum(quantum)
            seen = []
            for k, c in enumerate(sweeps):
                check(*collect(ctx, submit(ctx, c), len(c[0])), Q.ref(("os32d", k), c, p), (quantum, k))
                seen.append(ctx.front_scans())
            fused[quantum] = seen
            if quantum:
                for rep in range(2):
                    check(*collect(ctx, submit(ctx, odd), 32000), r_odd, ("32x1000", rep))
                    print("32 x 1000 row-major, padded: front_scans %d" % ctx.front_scans())
    print("os32d row-major 32 x 1024, fused per sweep: %s" % fused)
    assert fused[2048] == fused[0] and fused[2048][2:] == [1, 1, 1]


# ---- 10. the refusals ----
def test_refusals():
    p = Q.params32()
    key, cloud = Q.stream()[0]
    with u.Context(8192, 2, params=p) as ctx:
        for bad in (1000, 2049, 10240, 0x80000000):
            with pytest.raises(u.UrfError) as e:
                ctx.set_sweep_quantum(bad)
            assert e.value.code == -1 and "urf_set_sweep_quantum" in str(e.value), bad
        ctx.set_sweep_quantum(8192)
        ctx.set_sweep_quantum(2048)
        t = submit(ctx, cloud)
        for q in (0, 4096):
            with pytest.raises(u.UrfError) as e:
                ctx.set_sweep_quantum(q)
            assert e.value.code == -7
        check(*collect(ctx, t, len(cloud[0])), Q.ref(key, cloud, p), "after the refusals")
        ctx.set_sweep_quantum(0)
