"""urf_set_sweep_results_direct: with bits of urf_set_sweep_outputs set, the kernels of a sweep's captured sequence store marker points, counts
and the three lists themselves into a mapped pinned buffer of the sweep's slot, the lists back to back, and the sequence holds no copy for
them.  Every marker point and every list against oracle B (marker_pts, road_order, curb_order, ring10_order), exact: four sweeps in flight
on 1, 2 and 4 scratch rows, the layout through the raw C call, that only what exists is written (a pattern behind the entries survives the
slot's next sweeps), each bit alone and the kernels of each product alone, voided sweeps and their reruns, a sweep below the 30-point
threshold, fused row-major sweeps, rings beyond 2048 points and equal azimuths, urf_set_sweep_quantum, the refusals, a change of the switch
between the wait and the read, a batch call afterwards, the C++ adapter."""
import ctypes as C
import re
import struct
import subprocess

import numpy as np
import pytest

import oracles as O
import sweep_quantum_cases as Q
import urban_road_filter_amd as u
from test_gpu_async import records
from test_gpu_detector import build_demo
from test_gpu_front import ring_major
from test_gpu_front_outputs import Soa, batch_readouts, lasers_params, nudged, repeated_firings, same
from test_gpu_sweep_outputs import BOTH, N, check_ticket, collect, ref, results, small, submit, wide

pytestmark = pytest.mark.gpu
PATTERN = 0xA5A5A5A5
HDR_POINTS = 361 * 4   # words of the marker points in front of their count


def direct(ctx, bits=BOTH):
    ctx.set_sweep_results_direct(1)
    ctx.set_sweep_outputs(bits)


def raw(ctx, t):
    """The raw C calls: (addresses of road, curb, ring10), counts, address of the marker points, their count."""
    ptrs = [C.c_void_p() for _ in range(3)]
    cnt = (C.c_uint32 * 3)()
    ctx._check(ctx._lib.urf_result_ordered_indices(ctx._h, t, C.byref(ptrs[0]), C.byref(ptrs[1]), C.byref(ptrs[2]), cnt), "urf_result_ordered_indices")
    mp, m = C.c_void_p(), C.c_uint32(0)
    ctx._check(ctx._lib.urf_result_marker_points(ctx._h, t, C.byref(mp), C.byref(m)), "urf_result_marker_points")
    return [p.value for p in ptrs], [int(k) for k in cnt], mp.value, int(m.value)


def words(addr, n):
    """n 32-bit words of the slot's buffer at addr, in place (the buffer is the host's to read and write between sweeps)"""
    return np.ctypeslib.as_array(C.cast(addr, C.POINTER(C.c_uint32)), shape=(n,))


def check_layout(ctx, t, what):
    ptrs, cnt, _, _ = raw(ctx, t)
    assert ptrs[1] == ptrs[0] + 4 * cnt[0] and ptrs[2] == ptrs[1] + 4 * cnt[1], (what, ptrs, cnt)
    return ptrs, cnt


# ---- 1. four in flight on 1, 2 and 4 rows ----
@pytest.mark.parametrize("rows", [1, 2, 4])
def test_four_sweeps_in_flight(rows):
    p = wide()
    named = [small(k) for k in range(4)]
    refs = [ref(k, c, p) for k, c in named]
    with u.Context(64 * 256, rows, params=p) as ctx:
        direct(ctx)
        for rep in range(2):   # (captured, then replayed)
            tickets = [submit(ctx, c) for _, c in named]   # all of them before any is waited for
            for k, t in enumerate(tickets):
                check_ticket(ctx, t, named[k][1], refs[k], (rows, rep, k))
            for k, t in enumerate(tickets):   # ... and every ticket's results are still there after the last one has been waited for
                same(results(ctx, t), refs[k][2], (rows, rep, k, "again"))


# ---- 2. the layout ----
def test_the_lists_lie_back_to_back():
    p = wide()
    named = [small(k) for k in range(4)]
    refs = [ref(k, c, p) for k, c in named]
    with u.Context(64 * 256, 4, params=p) as ctx:
        direct(ctx)
        tickets = [submit(ctx, c) for _, c in named]
        for k, t in enumerate(tickets):
            check_ticket(ctx, t, named[k][1], refs[k], k)
            ptrs, cnt = check_layout(ctx, t, k)
            st = refs[k][2]
            assert cnt == [len(st["road_order"]), len(st["curb_order"]), len(st["ring10_order"])] and cnt[0] > 1000
            assert np.array_equal(words(ptrs[0], sum(cnt)), np.concatenate([st["road_order"], st["curb_order"], st["ring10_order"]]))


# ---- 3. only what exists is written ----
def test_only_what_exists_is_written():
    """Slot 0 through three of its sweeps: after the first, the whole list area and the marker area behind the count are filled with a
    pattern; four submissions later the slot holds the same sweep again -- entries equal, every word behind them the pattern; then the
    list area is filled again, the region of interest narrowed, and four submissions later the slot holds a sweep with FEWER entries:
    counts and entries are its own, the pattern stands behind them."""
    pw, pn = wide(), u.default_params()
    named = [small(k) for k in range(4)]
    refs = [ref(k, c, pw) for k, c in named]
    key, cloud = named[0]
    rn = ref(key + ("default roi",), cloud, pn)
    assert rn[1]["status"] == 0 and 0 < len(rn[2]["road_order"]) < len(refs[0][2]["road_order"])
    assert 0 < len(rn[2]["marker_pts"]) <= len(refs[0][2]["marker_pts"])
    n = 64 * 256
    with u.Context(n, 4, params=pw) as ctx:
        direct(ctx)
        t0 = submit(ctx, cloud)
        check_ticket(ctx, t0, cloud, refs[0], "first")
        ptrs, cnt, mp, m = raw(ctx, t0)
        words(ptrs[0], 2 * n)[:] = PATTERN
        words(mp, HDR_POINTS)[4 * m:] = PATTERN
        for k in (1, 2, 3):
            check_ticket(ctx, submit(ctx, named[k][1]), named[k][1], refs[k], ("between", k))
        t4 = submit(ctx, cloud)
        assert t4 % 4 == t0 % 4                              # the same slot
        check_ticket(ctx, t4, cloud, refs[0], "the slot's second sweep")
        ptrs4, cnt4, mp4, m4 = raw(ctx, t4)
        assert (ptrs4, cnt4, mp4, m4) == (ptrs, cnt, mp, m)
        assert (words(ptrs[0], 2 * n)[sum(cnt):] == PATTERN).all()
        assert (words(mp, HDR_POINTS)[4 * m:] == PATTERN).all()
        words(ptrs[0], 2 * n)[:] = PATTERN
        ctx.set_params(pn)                                   # fewer entries than the sweep before
        for k in (1, 2, 3):
            collect(ctx, submit(ctx, named[k][1]), n)
        t8 = submit(ctx, cloud)
        assert t8 % 4 == t0 % 4
        check_ticket(ctx, t8, cloud, rn, "the slot's third sweep, fewer entries")
        ptrs8, cnt8 = check_layout(ctx, t8, "narrow")
        _, _, mp8, m8 = raw(ctx, t8)
        assert ptrs8[0] == ptrs[0] and mp8 == mp and sum(cnt8) < sum(cnt) and m8 <= m
        assert (words(ptrs[0], 2 * n)[sum(cnt8):] == PATTERN).all()
        assert (words(mp, HDR_POINTS)[4 * m:] == PATTERN).all()


# ---- 4. bits and kernels ----
@pytest.mark.parametrize("bits,flags", [(u.SWEEP_OUT_MARKER_POINTS, 0), (u.SWEEP_OUT_ORDER, 0), (BOTH, 0), (BOTH, 32)],
                         ids=["marker_points", "order", "both", "both_one_by_one"])
def test_each_bit_alone_both_and_the_kernels_of_each_product(bits, flags):
    """Debug flag 32 of the hooks build: k_ordered_lists_direct and k_marker_bins instead of k_sweep_lists_direct.  Then the switch off
    again: the same results from the copied buffers, and every slot used captured its sequence once more."""
    p = wide()
    named = [small(k) for k in range(2)]
    refs = [ref(k, c, p) for k, c in named]
    n = 64 * 256

    def one_pass(ctx, what):
        got = []
        tickets = [submit(ctx, c) for _, c in named]
        for k, t in enumerate(tickets):
            lab, info = collect(ctx, t, n)
            assert info.status == 0 and np.array_equal(lab, refs[k][0]), (what, k)
            st = refs[k][2]
            if bits & u.SWEEP_OUT_MARKER_POINTS:
                mk = ctx.result_marker_points(t)
                assert mk.shape == st["marker_pts"].shape and np.array_equal(mk.view(np.uint32), st["marker_pts"].view(np.uint32)), (what, k)
                got.append(mk)
            else:
                with pytest.raises(u.UrfError) as e:
                    ctx.result_marker_points(t)
                assert e.value.code == -1 and "URF_SWEEP_OUT_MARKER_POINTS" in str(e.value)
            if bits & u.SWEEP_OUT_ORDER:
                lists = ctx.result_ordered_indices(t)
                for g, name in zip(lists, ("road_order", "curb_order", "ring10_order")):
                    assert np.array_equal(g, st[name]), (what, k, name)
                got.extend(lists)
            else:
                with pytest.raises(u.UrfError) as e:
                    ctx.result_ordered_indices(t)
                assert e.value.code == -1 and "URF_SWEEP_OUT_ORDER" in str(e.value)
        return got

    with u.Context(n, 2, params=p, hooks=True) as ctx:
        ctx.set_debug_flags(flags)
        direct(ctx, bits)
        on = [one_pass(ctx, ("on", rep)) for rep in range(2)][-1]   # (four submissions: every slot has its sequence)
        before = ctx.callback_path_captures()[0]
        ctx.set_sweep_results_direct(0)
        off = one_pass(ctx, "off")
        assert ctx.callback_path_captures()[0] == before + len(named)
        assert len(on) == len(off) and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(on, off))


# ---- 5. voided sweeps ----
def test_a_voided_sweep_brings_the_results_of_its_rerun():
    """A sensor-like sweep with equal planar ranges in every star sector (k_star_ties): voided by the short sequence, whose kernels
    store counts of 0, and run again inside urf_classify_pc2_wait, whose kernels store the results."""
    p = O.cfg_params("cfg2")
    ties, second = O.cfg_cloud("sensor", 1), O.cfg_cloud("narrow", 121)
    wt, wb = ref(("sensor", 1), ties, p), ref(("narrow", 121), second, p)
    with u.Context(N, 1, params=p) as ctx:
        direct(ctx)
        assert ctx.callback_path_state()[0] == 0
        tt, tb = submit(ctx, ties), submit(ctx, second)
        check_ticket(ctx, tt, ties, wt, "range ties")
        n1, seq = ctx.callback_path_state()
        assert n1 >= 1 and seq & 16                     # voided and run again
        check_layout(ctx, tt, "range ties")
        check_ticket(ctx, tb, second, wb, "behind the voided sweep")
        same(results(ctx, tt), wt[2], "range ties, after the sweep behind it")


def test_a_sweep_below_the_threshold_publishes_nothing_and_writes_nothing_else():
    p = wide()
    named = [small(k) for k in range(4)]
    refs = [ref(k, c, p) for k, c in named]
    few = tuple(a.copy() for a in named[0][1])
    few[0][29:] = 1.0e6
    rf = ref(named[0][0] + ("few",), few, p)
    assert rf[1]["status"] != 0
    n = 64 * 256
    with u.Context(n, 2, params=p) as ctx:
        direct(ctx)
        t0 = submit(ctx, named[0][1])
        check_ticket(ctx, t0, named[0][1], refs[0], "first")
        ptrs, cnt, mp, m = raw(ctx, t0)
        words(ptrs[0], 2 * n)[:] = PATTERN
        words(mp, HDR_POINTS)[4 * m:] = PATTERN
        for k in (1, 2, 3):
            check_ticket(ctx, submit(ctx, named[k][1]), named[k][1], refs[k], ("between", k))
        tf, tn = submit(ctx, few), submit(ctx, named[1][1])
        assert tf % 4 == t0 % 4
        lab, info = collect(ctx, tf, n)
        assert info.status == rf[1]["status"] and np.array_equal(lab, rf[0])
        ptrs_f, cnt_f, mp_f, m_f = raw(ctx, tf)
        assert cnt_f == [0, 0, 0] and m_f == 0 and ptrs_f == [ptrs[0]] * 3 and mp_f == mp
        road, curb, r10, mk = results(ctx, tf)
        assert (len(road), len(curb), len(r10), mk.shape) == (0, 0, 0, (0, 4))
        assert (words(ptrs[0], 2 * n) == PATTERN).all()
        assert (words(mp, HDR_POINTS)[4 * m:] == PATTERN).all()
        check_ticket(ctx, tn, named[1][1], refs[1], "behind the short sweep")


# ---- 6. fused row-major sweeps ----
@pytest.mark.parametrize("front_outputs", [0, 1])
def test_fused_row_major_sweeps(front_outputs):
    p = wide()
    named = [(("64x256", 1, seed, "rows"), ring_major(u.synth_cloud(64, 256, 1, seed))) for seed in (7, 31, 33, 35)]
    refs = [ref(k, c, p) for k, c in named]
    n = 64 * 256
    with u.Context(n, 4, params=p) as ctx:
        ctx.set_front_outputs(front_outputs)
        direct(ctx)
        fused = []
        for rep in range(3):   # the first sweep only sights the layout; fused from the second or third on
            lab, info = collect(ctx, submit(ctx, named[0][1]), n)
            assert np.array_equal(lab, refs[0][0])
            fused.append(ctx.front_scans())
        assert fused[2] == 1, fused
        for rep in range(2):
            tickets = [submit(ctx, c) for _, c in named]
            for k, t in enumerate(tickets):
                assert ctx.front_scans() == 1
                check_ticket(ctx, t, named[k][1], refs[k], ("rows", front_outputs, rep, k))
                check_layout(ctx, t, ("rows", front_outputs, rep, k))
                assert ctx.front_scans() == 1                      # no second run, the next sweep is fused again


# ---- 7. long rings, equal azimuths ----
def test_full_rings():
    p = O.cfg_params("cfg2")
    cloud = O.cfg_cloud("cfg2", 1)
    r = ref(("cfg2", 1), cloud, p)
    with u.Context(N, 4, params=p) as ctx:
        direct(ctx)
        t = submit(ctx, cloud)
        check_ticket(ctx, t, cloud, r, "full rings")
        check_layout(ctx, t, "full rings")


@pytest.mark.parametrize("variant", ["repeated", "nudged"])
def test_equal_azimuths(variant):
    p = O.cfg_params("cfg2")
    key, cloud = ("cfg2", 1, "repeated8"), repeated_firings(O.cfg_cloud("cfg2", 1), 8)
    if variant == "nudged":
        key, cloud = ("cfg2", 1, "nudged8"), nudged(O.cfg_cloud("cfg2", 1), 8, ref(key, cloud, p)[2])
    r = ref(key, cloud, p)
    with u.Context(N, 1, params=p) as ctx:
        direct(ctx)
        check_ticket(ctx, submit(ctx, cloud), cloud, r, ("equal azimuths", variant))


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
        direct(ctx)
        t = submit(ctx, cloud)
        check_ticket(ctx, t, cloud, r, ("long rings", variant))
        check_layout(ctx, t, ("long rings", variant))


# ---- 8. urf_set_sweep_quantum ----
def test_padded_sweeps_of_three_lengths():
    """Dense sweeps of three lengths at a quantum of 2048 (n' 4096 and 6144), four in flight: the lists name only the caller's points
    and lie back to back, whatever the padded length."""
    p = Q.params32()
    stream = Q.stream()
    named = [stream[0], stream[4], stream[2], stream[0]]
    lens = [len(c[0]) for _, c in named]
    assert len(set(lens)) == 3 and {Q.padded_len(n) for n in lens} == {4096, 6144}
    refs = [Q.ref(k, c, p, debug=True) for k, c in named]
    assert all(r[1]["status"] == 0 and len(r[2]["road_order"]) > 100 for r in refs)
    with u.Context(8192, 4, params=p) as ctx:
        ctx.set_sweep_quantum(2048)
        direct(ctx)
        for rep in range(2):
            tickets = [ctx.classify_pc2_async(Q.records(*c), len(c[0]), 32, 0, 4, 8) for _, c in named]
            for k, t in enumerate(tickets):
                lab, info = collect(ctx, t, lens[k])
                assert info.status == 0 and np.array_equal(lab, refs[k][0]), (rep, k)
                got = results(ctx, t)
                same(got, refs[k][2], ("quantum", rep, k))
                assert all((g < lens[k]).all() for g in got[:3])
                check_layout(ctx, t, ("quantum", rep, k))


# ---- 9. refusals, and the switch between the wait and the read ----
def test_refusals_and_a_change_between_the_wait_and_the_read():
    p = wide()
    named = [small(k) for k in range(4)]
    refs = [ref(k, c, p) for k, c in named]
    n = 64 * 256
    b = Soa([c for _, c in named])
    with u.Context(n, 4, params=p) as ctx:
        for on in (2, -1):
            with pytest.raises(u.UrfError) as e:
                ctx.set_sweep_results_direct(on)
            assert e.value.code == -1
        ctx.set_sweep_outputs(BOTH)
        t_off = submit(ctx, named[0][1])                   # submitted with the switch off
        with pytest.raises(u.UrfError) as e:
            ctx.set_sweep_results_direct(1)                # ... which does not change under a sweep in flight
        assert e.value.code == -7 and "urf_set_sweep_results_direct" in str(e.value)
        collect(ctx, t_off, n)
        ctx.set_sweep_results_direct(1)
        same(results(ctx, t_off), refs[0][2], "submitted off, read with the switch on")
        ptrs, cnt, _, _ = raw(ctx, t_off)
        assert ptrs[1] == ptrs[0] + 4 * n and ptrs[2] == ptrs[1] + 4 * n   # (its own layout: three lists of the sweep's length)
        t_on = submit(ctx, named[1][1])
        with pytest.raises(u.UrfError) as e:
            ctx.set_sweep_results_direct(0)
        assert e.value.code == -7
        for call in (ctx.result_marker_points, ctx.result_ordered_indices):   # in flight
            with pytest.raises(u.UrfError) as e:
                call(t_on)
            assert e.value.code == -7
        collect(ctx, t_on, n)
        ctx.set_sweep_results_direct(0)
        same(results(ctx, t_on), refs[1][2], "submitted on, read with the switch off")
        check_layout(ctx, t_on, "submitted on, read with the switch off")
        same(results(ctx, t_off), refs[0][2], "the other slot's, still")
        ctx.set_sweep_results_direct(1)
        tickets = [submit(ctx, c) for _, c in named]
        for k, t in enumerate(tickets):
            check_ticket(ctx, t, named[k][1], refs[k], k)
        for call in (ctx.result_marker_points, ctx.result_ordered_indices):   # overtaken
            with pytest.raises(u.UrfError) as e:
                call(t_off)
            assert e.value.code == -1
        old = ctx.ordered_indices(n) + (ctx.marker_points(),)   # the old read-outs next to them: the sweep waited for last
        same(old, refs[3][2], "urf_ordered_indices / urf_marker_points")
        b.classify(ctx)                                    # a batch call afterwards
        switched = (b.label_bytes(), batch_readouts(ctx, 4, n))
    for s in range(4):
        assert np.array_equal(switched[0][s * n:(s + 1) * n], refs[s][0])
        same(switched[1][s], refs[s][2], ("batch after sweeps", s))


def test_a_context_that_sets_no_bit_allocates_and_launches_nothing_more():
    """The switch alone: labels and summaries as without it, no results to read."""
    p = wide()
    key, cloud = small(0)
    r = ref(key, cloud, p)
    n = len(cloud[0])
    with u.Context(n, 2, params=p) as ctx:
        ctx.set_sweep_results_direct(1)
        t = submit(ctx, cloud)
        lab, info = collect(ctx, t, n)
        assert np.array_equal(lab, r[0]) and info.n_road == r[1]["n_road"]
        for call in (ctx.result_marker_points, ctx.result_ordered_indices):
            with pytest.raises(u.UrfError) as e:
                call(t)
            assert e.value.code == -1 and "urf_set_sweep_outputs" in str(e.value)


# ---- 10. the C++ adapter ----
def test_the_adapter_publishes_the_same_bytes_with_the_switch_on(tmp_path):
    """tests/cpp/detector_sweep_direct_demo.cpp: eight 64 x 256 sweeps kept four in flight through two detectors with setSweepOutputs,
    road_marker and the reference order on, setSweepResultsDirect off and on; clouds and MarkerArrays byte for byte."""
    from test_gpu_detector_sweep_outputs import expected, sweeps
    exe = build_demo(tmp_path, "detector_sweep_direct_demo")
    clouds, files = sweeps(), []
    for k, (x, y, z) in enumerate(clouds):
        path = str(tmp_path / ("sweep%d.bin" % k))
        with open(path, "wb") as f:
            f.write(struct.pack("<I", len(x)))
            for a in (x, y, z):
                f.write(np.ascontiguousarray(a, np.float32).tobytes())
        files.append(path)
    r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, (r.stdout, r.stderr)
    m = re.match(r"sweeps (\d+) equal (\d+) published (\d+) deletes (\d+) road (\d+)", r.stdout)
    assert m, r.stdout
    got = tuple(map(int, m.groups()))
    assert got[:2] == (8, 8) and got[2:] == expected(clouds), (got, expected(clouds))
