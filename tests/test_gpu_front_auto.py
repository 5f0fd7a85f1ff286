"""urf_set_front_auto: the context applies urf_front_explain's advice itself (include/urf.h; k_front_digest, urf_k_front_digest.hpp;
urf_policy::auto_call / auto_digest).

1. The digest is the fold of explain's records: front mode 2, auto on, one call -- the eight words front_auto() reports equal
   tests/front_auto_model.py's fold of front_explain's records of that same call.  The records are read in the layout the pass counted
   them in: a fresh context's first call has no probe / transpose in its sequence, so that is firing order (0) for every case, the
   row-major ones included (their first call only sights, and what it counted is discarded by the sighting's new start).  They equal the
   CPU model's pinned figures (tests/test_front_auto_cpu.py) for the cases in firing order whose first call repairs no speculation
   (no OTHER among the bits).
2. Convergence: eight calls, labels equal oracle B after every one; then the fused scans are those a plain mode-2 context's explain
   advises nothing outside URF_ADVICE_AUTO_MASK | MODE_2 | CALL_AGAIN for, SETTLED, `applied` the union of their advice inside the mask and of what the first call's
   advice asked for (applied before any scan is looked at: LASERS128 at 128 lasers), at most five calls carried the pass; two more calls change nothing.
3. A fresh context with `applied` set by hand gives the same front_scans and labels, call for call from its third call on.
4. Call-level advice at the first call; what auto leaves alone.   5. Off is off.   6. New starts.   7. The callback path.

Shapes: the small sweeps and the models' four-sweep batches of tests/test_gpu_front_explain.py (4 096 .. 16 384 points resp. the suite's
own model batches); one sweep of 129 tiles for LONG_SWEEPS."""
import numpy as np
import pytest

import front_auto_model as AM
import front_shape as FS
import sensor_models as SM
import urban_road_filter_amd as u
from hipmem import DevBuf
from test_front_auto_cpu import MODEL_DIGESTS, SMALL_DIGESTS
from test_front_why_cpu import SMALL, model_scans, small_cases
from test_gpu_front_explain import CAPACITY, NAMES, Call, apply_advice, cases

pytestmark = pytest.mark.gpu
W, S, A, PH = u.WHY_CALL, u.WHY_SCAN, u.ADVICE, u.AUTO_PHASE
MASK = u.ADVICE_AUTO_MASK
WORDS = AM.WORDS
CALL_BITS = A["MODE_3"] | A["LASERS128"] | A["LONG_SWEEPS"] | A["CURB_POINTS"]   # the advice urf_policy::why gives a CALL (the two others are the scans')


def fresh(scans, mode=2, auto=1, lasers128=False):
    """a context with nothing set by hand but the mode; lasers128: test_gpu_front_explain.context's, which turns that switch on by hand"""
    ctx = u.Context(max(CAPACITY, max(len(c[0]) for c in scans)), len(scans))
    if lasers128:
        ctx.set_front_lasers128(1)
    ctx.set_front_mode(mode)
    if auto is not None:
        ctx.set_front_auto(auto)
    return ctx


def digest(info):
    return tuple(int(info[k]) for k in WORDS)


def counted(call):
    """scans of the call with a result: URF_OK and not empty (urf_scan_info: eight words, the status last)"""
    status = call.di.to_numpy(np.uint8).view(np.int32).reshape(-1, 8)[:, 7]
    return [int(s) == 0 and n > 0 for s, n in zip(status, call.lens)]


def lay(layout):
    return 1 if layout == "rows" else 0


# ---- 1. the digest ----
@pytest.mark.parametrize("name", NAMES)
def test_the_digest_is_the_fold_of_explains_records(name):
    scans, p, layout = cases()[name]
    call = Call(scans)
    with fresh(scans) as ctx:
        call.classify(ctx, p)
        info = ctx.front_auto()
        why = ctx.front_explain(0)   # (the layout the pass counted in: a first call's sequence has no probe / transpose)
        again = ctx.front_auto()
    got, want = digest(info), AM.fold(why, counted(call))
    print(name, "digest", got, "seq", int(info["digest_seq"]), "applied", hex(int(info["applied"])), "explained", int(info["explained_calls"]))
    assert info.tobytes() == again.tobytes()   # (explain and the query change nothing)
    assert (why["call"] == 0).all() and info["explained_calls"] == 1 and info["digest_seq"] != 0 and info["phase"] == PH["LEARNING"]
    assert got == want
    model = SMALL_DIGESTS[name][0] if name in SMALL else MODEL_DIGESTS[tuple(name.split(" / "))][0]
    if layout == "firing" and not got[2] & S["OTHER"]:
        assert got == model


# ---- 2. convergence; 3. equal to hand-set ----
_RUNS = {}


def run_of(name):
    """Ten calls of a fresh auto context with nothing but the mode set by hand, computed once per case, and what it is compared with:
    `plain`, what a mode-2 context's explain says after three calls -- that context is test_gpu_front_explain.context's, 128 lasers with
    urf_set_front_lasers128 set by hand, so that its scans have an advice of their own --; `call_bits`, the call-level part of the advice
    an untouched mode-2 context's first call gets (MODE_3, LASERS128, LONG_SWEEPS, CURB_POINTS: what auto applies at the call, before any
    scan has been looked at -- for the os128d batch at interval 0.5 LASERS128, although every scan then breaks a rule no setting
    lifts); `hand`, eight calls of an untouched context with `applied` set by hand."""
    if name in _RUNS:
        return _RUNS[name]
    scans, p, layout = cases()[name]
    call = Call(scans)
    r = {"labels": [], "front": [], "info": []}
    with fresh(scans) as ctx:
        for k in range(10):
            r["labels"].append([l.copy() for l in call.classify(ctx, p)])
            r["front"].append(ctx.front_scans())
            r["info"].append(ctx.front_auto())
            if k == 7:
                r["fused"] = ctx.front_explain(lay(layout))["fused"].tolist()
    with fresh(scans, auto=None, lasers128=p.channels == 128) as ctx:
        call.classify(ctx, p, times=3)
        r["plain"] = ctx.front_explain(lay(layout)).copy()
    with fresh(scans, auto=None) as ctx:
        call.classify(ctx, p)
        r["call_bits"] = int(ctx.front_explain(lay(layout))[0]["advice"]) & CALL_BITS
    applied = int(r["info"][7]["applied"])
    r["hand"] = {"labels": [], "front": []}
    with fresh(scans, auto=None) as ctx:
        apply_advice(ctx, applied, 2)
        for k in range(8):
            r["hand"]["labels"].append([l.copy() for l in call.classify(ctx, p)])
            r["hand"]["front"].append(ctx.front_scans())
    _RUNS[name] = r
    return r


@pytest.mark.parametrize("name", NAMES)
def test_convergence(name):
    scans, p, layout = cases()[name]
    r = run_of(name)
    for k, labels in enumerate(r["labels"]):
        for s, c in enumerate(scans):
            assert np.array_equal(labels[s], FS.stages(c, p)[0]), (k, s)
    liftable = [bool(w["fused"]) or not int(w["advice"]) & ~(MASK | A["MODE_2"] | A["CALL_AGAIN"]) for w in r["plain"]]
    union = 0
    for w, ok in zip(r["plain"], liftable):
        union |= int(w["advice"]) & MASK if ok else 0
    info = r["info"][7]
    union |= r["call_bits"]   # (applied at the first call, whatever the scans show afterwards)
    assert r["call_bits"] == (A["LASERS128"] if p.channels == 128 else 0)
    print(name, "fused", r["fused"], "liftable", liftable, "applied", hex(int(info["applied"])), "union", hex(union), "explained",
          [int(i["explained_calls"]) for i in r["info"]], "phase", [int(i["phase"]) for i in r["info"]], "front", r["front"])
    assert [bool(f) for f in r["fused"]] == liftable and r["front"][7] == sum(liftable)
    assert info["phase"] == PH["SETTLED"] and info["applied"] == union and info["refused"] == 0
    assert all(i["explained_calls"] <= 5 for i in r["info"])
    assert r["info"][9]["explained_calls"] == info["explained_calls"] and r["info"][9]["phase"] == PH["SETTLED"] and r["front"][8:] == [r["front"][7]] * 2


@pytest.mark.parametrize("name", NAMES)
def test_equal_to_the_switches_set_by_hand(name):
    scans, _, _ = cases()[name]
    r = run_of(name)
    assert r["front"][2:8] == r["hand"]["front"][2:8]
    for k in range(2, 8):
        for s in range(len(scans)):
            assert np.array_equal(r["labels"][k][s], r["hand"]["labels"][k][s]), (k, s)


# ---- 4. call-level advice, at the first call ----
def with_cp(p, cp):
    q = u.Params.from_buffer_copy(p)
    q.curbPoints = cp
    return q


def test_curb_points_4_at_16_lasers_is_fused_by_the_first_call():
    c, p, _ = small_cases()["ideal16"]
    q = with_cp(p, 4)
    call = Call([c])
    with fresh([c]) as ctx:
        labels = call.classify(ctx, q)
        info = ctx.front_auto()
        assert ctx.front_scans() == 1 and info["applied"] == A["MODE_3"] | A["CURB_POINTS"] and info["refused"] == 0
        assert np.array_equal(labels[0], FS.stages(c, q)[0])


def test_lasers128_and_long_sweeps():
    c, p, _ = small_cases()["128 stagger"]
    call = Call([c])
    with fresh([c]) as ctx:
        call.classify(ctx, p)
        info = ctx.front_auto()
        assert info["applied"] & A["LASERS128"] and info["explained_calls"] == 1 and not ctx.front_explain(0)[0]["call"]
    # the smallest long sweep of tests/test_gpu_front_long_sweeps.py: 64 x 4128, 129 tiles; labels against the switch set by hand
    from test_gpu_front_long_sweeps import cloud, params64
    c, p = cloud(64, 4128, 1, 71), params64()
    call = Call([c])
    with fresh([c]) as ctx:
        labels = call.classify(ctx, p)
        assert ctx.front_auto()["applied"] == A["LONG_SWEEPS"] and ctx.front_scans() == 1
    with fresh([c], auto=None) as ctx:
        ctx.set_front_long_sweeps(1)
        by_hand = call.classify(ctx, p)
        assert ctx.front_scans() == 1
    assert np.array_equal(labels[0], by_hand[0])


def test_what_auto_leaves_alone():
    c, p, _ = small_cases()["ideal16"]
    call = Call([c])
    with fresh([c]) as ctx:   # curbPoints 9: no fused kernels
        call.classify(ctx, with_cp(p, 9), times=3)
        info = ctx.front_auto()
        assert info["applied"] == 0 and info["left"] & A["NEVER"] and info["explained_calls"] == 0 and info["phase"] == PH["LEARNING"]
    with fresh([c]) as ctx:   # stage capture: its values are the general kernels'
        ctx.enable_stage_capture(2)
        call.classify(ctx, with_cp(p, 4))
        info = ctx.front_auto()
        assert info["applied"] == 0 and info["left"] & A["CAPTURE_OFF"] and ctx.front_scans() == 0
    with fresh([c]) as ctx:   # a read-out made the context sticky-general
        call.classify(ctx, p)
        assert ctx.front_scans() == 1
        ctx.ordered_indices(len(c[0]), 0)
        call.classify(ctx, with_cp(p, 4))
        info = ctx.front_auto()
        assert info["applied"] == 0 and info["left"] & A["RESET"] and ctx.front_scans() == 0
        ctx.set_front_mode(2)   # ... and urf_set_front_mode again: learning again
        assert ctx.front_auto()["phase"] == PH["LEARNING"] and ctx.front_auto()["explained_calls"] == 0
        call.classify(ctx, with_cp(p, 4))
        assert ctx.front_scans() == 1 and ctx.front_auto()["applied"] == A["MODE_3"] | A["CURB_POINTS"]


# ---- 5. off is off ----
def test_off_reads_zero():
    c, p, _ = small_cases()["ideal16"]
    with fresh([c], auto=None) as ctx:
        assert not any(ctx.front_auto().tolist()[:-1]) and not ctx.front_auto()["reserved"].any()
        ctx.set_front_auto(0)
        assert not any(ctx.front_auto().tolist()[:-1])
        ctx.set_front_auto(1)
        Call([c]).classify(ctx, with_cp(p, 4))
        ctx.set_front_auto(0)
        info = ctx.front_auto()
        assert info["applied"] == A["MODE_3"] | A["CURB_POINTS"] and not any(int(info[k]) for k in info.dtype.names[:-1] if k != "applied")
        assert ctx._lib.urf_set_front_auto(ctx._h, 2) == -1


def history(auto):
    """test_gpu_front_explain.history's pattern in front mode 1: three calls, what each gave"""
    from test_front_multi_cpu import small_params, small_sweeps
    p = small_params("64 offsets")
    c = small_sweeps("64 offsets")[0]
    scans = [c, SM.sweep("ideal64", firings=256, world=2, seed=21, holes=("nan",))]
    call = Call(scans)
    out = []
    with fresh(scans, mode=1, auto=auto) as ctx:
        ctx.enable_kernel_timing(1)
        for _ in range(3):
            labels = call.classify(ctx, p)
            out.append(([l.copy() for l in labels], ctx.front_scans(), ctx.kernel_timing()[1]))
        return out, ctx.front_auto()


def test_mode_1_is_idle_and_nothing_changes():
    with_it, info = history(1)
    without, _ = history(None)
    assert info["on"] == 1 and info["phase"] == PH["IDLE"] and info["explained_calls"] == 0 and info["applied"] == 0
    for a, b in zip(with_it, without):
        assert a[1:] == b[1:] and a[2] == 1
        for la, lb in zip(a[0], b[0]):
            assert np.array_equal(la, lb)


# ---- 6. new starts ----
def test_new_starts():
    name = "hdl64e / default"
    scans, p, layout = cases()[name]
    call = Call(scans)
    with fresh(scans) as ctx:
        call.classify(ctx, p, times=1)
        for _ in range(5):
            call.classify(ctx, p)
        info = ctx.front_auto()
        assert info["phase"] == PH["SETTLED"] and info["applied"] == A["MULTI_SECTOR"]
        q = u.Params.from_buffer_copy(p)
        q.curbHeight = p.curbHeight * 1.5
        ctx.set_params(q)
        info = ctx.front_auto()
        assert info["phase"] == PH["LEARNING"] and info["applied"] == A["MULTI_SECTOR"] and info["explained_calls"] == 0
        for _ in range(6):
            labels = call.classify(ctx, q)
        info = ctx.front_auto()
        assert info["phase"] == PH["SETTLED"] and 1 <= info["explained_calls"] <= 5
        for s, c in enumerate(scans):
            assert np.array_equal(labels[s], FS.stages(c, q)[0]), s
        # off: the switches stay and a call carries no pass.  With the switch off the query reads zero, so the pass is counted by the
        # sequence numbers the host hands out, one per pass: the first pass after the switch is on again has the number behind the last
        # one before it was turned off.
        seq = int(info["digest_seq"])
        assert seq > 0
        ctx.set_front_auto(0)
        before = ctx.front_scans()
        call.classify(ctx, q)
        call.classify(ctx, q)
        assert ctx.front_auto()["applied"] == A["MULTI_SECTOR"] and ctx.front_scans() == before == 4
        ctx.set_front_auto(1)   # (on again: a new start, the old digest is gone)
        info = ctx.front_auto()
        assert info["phase"] == PH["LEARNING"] and info["explained_calls"] == 0 and info["digest_seq"] == 0 and info["applied"] == A["MULTI_SECTOR"]
        call.classify(ctx, q)
        info = ctx.front_auto()
        assert info["explained_calls"] == 1 and info["digest_seq"] == seq + 1


# ---- 7. the callback path ----
def records(c):
    r = np.zeros((len(c[0]), 4), np.float32)
    r[:, 0], r[:, 1], r[:, 2] = c
    return r


def os64_sweeps():
    scans, p, layout = cases()["os64 / default"]
    assert layout == "rows"
    return scans, p


def test_callback_path_one_at_a_time():
    scans, p = os64_sweeps()
    n = len(scans[0][0])
    recs = [records(c) for c in scans]
    fused, captures = [], []
    with u.Context(n, 1, params=p) as ctx:
        ctx.set_front_mode(2)
        ctx.set_front_auto(1)
        for k in range(12):
            s = (0, 2, 3)[k % 3]   # (the staggered sweeps; scans[1] is the ideal control)
            labels, _ = ctx.classify_pc2(recs[s], n, 16, 0, 4, 8)
            assert np.array_equal(labels, FS.stages(scans[s], p)[0]), k
            fused.append(int(ctx.front_explain(1)[0]["fused"]))
            captures.append(ctx.callback_path_captures()[0])
            info = ctx.front_auto()
            print(k, "fused", fused[-1], "captures", captures[-1], "phase", int(info["phase"]), "applied", hex(int(info["applied"])), "explained", int(info["explained_calls"]))
        assert info["applied"] & A["MULTI_SECTOR"] and info["phase"] == PH["SETTLED"]
    first = fused.index(1)
    assert first < 11 and all(fused[first:])
    # settled: nothing is captured again.  (The first sweeps behind the application still capture: the callback path's own policy --
    # the kernels a voided sweep needed, the layout a scan took -- bumps the epoch as it does with the switch set by hand.)
    assert captures[-1] == captures[-3] == captures[-6]


@pytest.mark.parametrize("max_batch", [4, 1])
def test_callback_path_four_in_flight(max_batch):
    scans, p = os64_sweeps()
    n = len(scans[0][0])
    recs = [records(c) for c in scans]
    with u.Context(n, max_batch, params=p) as ctx:
        ctx.set_front_mode(2)
        ctx.set_front_auto(1)
        for rep in range(4):
            tickets = [ctx.classify_pc2_async(r, n, 16, 0, 4, 8) for r in recs]
            for k, t in enumerate(tickets):
                lab = np.zeros(n, np.uint8)
                ctx.classify_pc2_wait(t, lab)
                assert np.array_equal(lab, FS.stages(scans[k], p)[0]), (rep, k)
        info = ctx.front_auto()
        print(max_batch, "phase", int(info["phase"]), "applied", hex(int(info["applied"])), "explained", int(info["explained_calls"]))
        assert info["applied"] & A["MULTI_SECTOR"]
