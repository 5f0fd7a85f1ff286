"""urf_front_explain: why a scan of the last call left the fused front end, and what keeps it (include/urf.h; k_front_explain,
urf_k_front_explain.hpp; urf_policy::why).

1. The counters equal tests/front_why_model.py's (oracle B's stages; pinned in tests/test_front_why_cpu.py), exactly: on the small sweeps,
   on the sensor models' batches, at two settings, in front mode 2 and 0, and after a dense call for the padded batch.
2. Every hand-back is explained: after the third call of a context in mode 2, fused == 0 <=> call | scan != 0, never OTHER, and the fused
   ones are what urf_front_scans counts -- with urf_set_front_multi_sector off and on.
3. The advice works: a fresh context with the advised setters fuses the scan, labels as oracle B's.
4. It changes nothing: labels, urf_front_scans and the number of classify calls urf_kernel_timing saw are the same with and without an
   explain in between -- a fused context, a sticky-general one, a fused one with urf_set_front_outputs.
5. Refusals.

Shapes: the small sweeps are 4 096 .. 16 384 points (two to eight tiles: the CAS tables and the masks are shared between blocks), 16, 32,
64 and 128 lasers, firing order and row-major, a scan that ends inside a firing; the models' batches are the suite's own (oracle B's
stages of them are computed once per process, tests/front_shape.py)."""
import numpy as np
import pytest

import dense_model as D
import front_shape as FS
import front_why_model as WM
import gpu_sensor_cases as G
import sensor_models as SM
import urban_road_filter_amd as u
from hipmem import DevBuf
from test_front_multi_cpu import small_params, small_sweeps
from test_front_why_cpu import MODELS, SMALL, model_scans, small_cases

pytestmark = pytest.mark.gpu
CAPACITY = 64 * 2048   # max_points of the contexts below: a sensor-sized candidate list (tests/test_gpu_front_multi.py: context)
W, S, A = u.WHY_CALL, u.WHY_SCAN, u.ADVICE
GPU_MODELS = ("vlp16", "hdl64e", "os64", "os128d")


class Call:
    """A batch on the device, kept alive as long as the object (urf_front_explain reads the call's inputs again)."""

    def __init__(self, scans):
        self.scans = scans
        self.lens = [len(c[0]) for c in scans]
        self.offs = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.uint32)
        self.dx, self.dy, self.dz = (DevBuf.from_numpy(np.concatenate([c[k] for c in scans]).astype(np.float32)) for k in range(3))
        self.do = DevBuf.from_numpy(self.offs)
        self.dl, self.di = DevBuf(int(self.offs[-1])), DevBuf(32 * len(scans))

    def classify(self, ctx, p, times=1):
        ctx.set_params(p)
        for _ in range(times):
            if len(set(self.lens)) == 1:
                ctx.classify_batch_soa(self.dx, self.dy, self.dz, self.lens[0], len(self.scans), self.dl, self.di)
            else:
                ctx.classify_batch_soa_ragged(self.dx, self.dy, self.dz, self.do, max(self.lens), len(self.scans), self.dl, self.di)
        ctx.synchronize()
        lab = self.dl.to_numpy(np.uint8)
        return [lab[a:b] for a, b in zip(self.offs[:-1], self.offs[1:])]


def context(scans, p, capacity=CAPACITY):
    ctx = u.Context(max(capacity, max(len(c[0]) for c in scans)), len(scans))
    if p.channels == 128:
        ctx.set_front_lasers128(1)
    return ctx


def counters(rec):
    return tuple(int(rec[k]) for k in WM.FIELDS)


def cases():
    """name -> (scans, parameters, layout) of everything the tests below walk"""
    out = {name: ([c], p, layout) for name, (c, p, layout) in small_cases().items()}
    for model in GPU_MODELS:
        for setting in ("default", "interval 0.5"):
            out["%s / %s" % (model, setting)] = (model_scans(model), G.params(model, setting), SM.MODELS[model]["layout"])
    return out


def want_of(name, scans, p, layout):
    if name in SMALL:
        return [SMALL[name]]
    model, setting = name.split(" / ")
    return MODELS[(model, setting)]


NAMES = sorted(SMALL) + ["%s / %s" % (m, s) for m in GPU_MODELS for s in ("default", "interval 0.5")]


# ---- 1. the counters ----
@pytest.mark.parametrize("name", NAMES)
def test_counters_equal_the_model(name):
    scans, p, layout = cases()[name]
    want = want_of(name, scans, p, layout)
    assert want == [counters(WM.counters(c, p, layout)) for c in scans]   # (the pinned figures are the model's)
    call = Call(scans)
    got = {}
    with context(scans, p) as ctx:
        for mode in (2, 0):
            ctx.set_front_mode(mode)
            call.classify(ctx, p)
            why = ctx.front_explain(1 if layout == "rows" else 0)
            assert len(why) == len(scans)
            got[mode] = [counters(r) for r in why]
            print(name, "mode", mode, got[mode], [hex(int(r["scan"])) for r in why])
            for r, w in zip(why, want):
                assert bool(r["scan"] & S["LANE_TWO_RINGS"]) == (w[0] > 0) and bool(r["scan"] & S["RING_TWO_LANES"]) == (w[1] > 0)
                assert bool(r["scan"] & S["AXIS"]) == (w[2] > 0) and bool(r["scan"] & S["RANGE"]) == (w[3] > 0)
                assert bool(r["scan"] & S["MULTI_SECTOR"]) == (w[4] > 0) and bool(r["scan"] & S["SECTORS_FALL"]) == (w[6] > 0)   # (the switch is off)
                assert bool(r["advice"] & A["NEVER"]) == any(w[:4])
            assert bool(why[0]["call"] & W["MODE_OFF"]) == (mode == 0) and (mode == 2 or not why["fused"].any())
    assert got[2] == want and got[0] == want


def test_a_scan_without_a_result_and_rows_that_do_not_divide():
    a, p, _ = small_cases()["ideal16"]
    few = tuple(v[:20].copy() for v in a)
    rows = tuple(v[:-1].copy() for v in small_cases()["ideal16 rows"][0])
    call = Call([few, rows, a])
    with context(call.scans, p) as ctx:
        ctx.set_front_mode(2)
        call.classify(ctx, p)
        why = ctx.front_explain(1)
    assert why[0]["scan"] == 0 and not any(counters(why[0]))                       # URF_TOO_FEW_POINTS
    assert why[1]["scan"] & S["ROWS_LENGTH"] and why[1]["advice"] & A["NEVER"] and not any(counters(why[1]))
    assert not why[2]["scan"] & S["ROWS_LENGTH"] and why[2]["scan"] & S["ROWS_SIGHTING"]   # (read as rows, which it is not: the first call only sights)


def test_after_a_dense_call_the_counters_are_the_padded_batchs():
    L, F = 16, 300
    p = SM.params_for("vlp16")
    clouds = [SM.sweep("vlp16", firings=F, world=k, seed=140 + k, noise=True, drop=0.10, start_deg=k * 77.7) for k in (0, 1)]
    dense, ids, padded = [], [], []
    for c in clouds:
        d, slot = D.densify(c, L, SM.missing_mask(c))
        pos, _, aligned = D.realign(slot, L, F)
        assert aligned
        dense.append(d), ids.append(slot.astype(np.uint8)), padded.append(D.pad(d, pos, L, F))
    want = [counters(WM.counters(c, p)) for c in padded]
    assert any(w[4] for w in want)   # (drift inside a firing: something to count)
    call = Call(dense)
    did = DevBuf.from_numpy(np.concatenate(ids))
    with u.Context(CAPACITY, 2) as ctx:
        ctx.set_front_mode(2)
        ctx.set_params(p)
        ctx.classify_batch_soa_dense(call.dx, call.dy, call.dz, did, 1, call.do, max(call.lens), 2, F, call.dl, call.di)
        assert ctx.dense_scans() == 2
        why = ctx.front_explain(1)   # (a dense call is read in firing order whatever the caller says)
        assert [counters(r) for r in why] == want
        assert int(why["fused"].sum()) == ctx.front_scans()


# ---- 2. every hand-back is explained; 3. the advice works ----
def explained(ctx, call, p, layout):
    call.classify(ctx, p, times=3)
    why = ctx.front_explain(1 if layout == "rows" else 0)
    for k, r in enumerate(why):
        assert (r["fused"] == 0) == ((r["call"] | r["scan"]) != 0), (k, dict(zip(why.dtype.names, r.tolist())))
        assert not r["scan"] & S["OTHER"], k
        assert (r["candidates"] > r["candidate_cap"]) == bool(r["scan"] & S["CANDIDATES"])
    assert int(why["fused"].sum()) == ctx.front_scans()
    return why


SETTERS = (("LASERS128", "set_front_lasers128"), ("LONG_SWEEPS", "set_front_long_sweeps"), ("CURB_POINTS", "set_front_curb_points"),
           ("MULTI_SECTOR", "set_front_multi_sector"), ("MULTI_SECTOR_CP", "set_front_multi_sector_curb_points"), ("FRONT_OUTPUTS", "set_front_outputs"))


def apply_advice(ctx, advice, mode):
    for bit, setter in SETTERS:
        if advice & A[bit]:
            getattr(ctx, setter)(1)
    ctx.set_front_mode(3 if advice & A["MODE_3"] else (2 if advice & A["MODE_2"] else mode))   # (RESET: the same call)


@pytest.mark.parametrize("name", NAMES)
def test_every_hand_back_is_explained_and_the_advice_works(name):
    scans, p, layout = cases()[name]
    call = Call(scans)
    with context(scans, p) as ctx:
        for on in (0, 1):
            ctx.set_front_multi_sector(on)
            ctx.set_front_mode(2)
            why = explained(ctx, call, p, layout)
            print(name, "multi_sector", on, "fused", why["fused"].tolist(), "scan", [hex(int(v)) for v in why["scan"]], "advice", [hex(int(v)) for v in why["advice"]])
            if on == 0:
                off = why.copy()
            elif bool(p.star_shaped_method):   # (what the switch is for is no reason any more)
                assert not (why["scan"] & (S["MULTI_SECTOR"] | S["SECTORS_FALL"])).any()
    helped = [k for k, r in enumerate(off) if not r["advice"] & A["NEVER"]]
    assert helped or any(any(w[:4]) for w in want_of(name, scans, p, layout))
    advice = 0
    for k in helped:
        advice |= int(off[k]["advice"])
    if not advice:
        assert off["fused"][helped].all()
        return
    # a fresh context, the advised setters (of all these scans together: they only add), the same call three times
    with context(scans, p, capacity=4 * CAPACITY if advice & A["CAPACITY"] else CAPACITY) as ctx:
        apply_advice(ctx, advice, 2)
        labels = call.classify(ctx, p, times=3)
        why = ctx.front_explain(1 if layout == "rows" else 0)
        for k in helped:
            assert why[k]["fused"] == 1, (k, dict(zip(why.dtype.names, why[k].tolist())))
        for k, c in enumerate(scans):
            assert np.array_equal(labels[k], FS.stages(c, p)[0]), k


def test_the_calls_reasons_reach_the_record():
    """mode 1 and a small batch of 16 lasers: FEW_SCANS, MODE_2; curbPoints 4: CURB_POINTS on top, MODE_3 and the switch; 9: NEVER."""
    c, p, _ = small_cases()["ideal16"]
    call = Call([c])
    with context([c], p) as ctx:
        call.classify(ctx, p)
        r = ctx.front_explain(0)[0]
        assert (r["fused"], r["call"], r["advice"], r["scan"]) == (0, W["FEW_SCANS"], A["MODE_2"], 0)
        q = u.Params.from_buffer_copy(p)
        q.curbPoints = 4
        call.classify(ctx, q)
        r = ctx.front_explain(0)[0]
        assert (r["call"], r["advice"]) == (W["FEW_SCANS"] | W["CURB_POINTS"], A["MODE_3"] | A["CURB_POINTS"])
        apply_advice(ctx, int(r["advice"]), 1)
        call.classify(ctx, q)
        r = ctx.front_explain(0)[0]
        assert (r["fused"], r["call"], r["advice"], r["scan"]) == (1, 0, 0, 0) and ctx.front_scans() == 1
        q.curbPoints = 9
        call.classify(ctx, q)
        r = ctx.front_explain(0)[0]
        assert r["call"] == W["CURB_POINTS"] and r["advice"] == A["NEVER"]


# ---- 4. it changes nothing ----
def history(explain, prepare, readout):
    """Three calls on a fresh context, an explain (or none) in front of the last: what the last one gave."""
    p = small_params("64 offsets")
    c = small_sweeps("64 offsets")[0]
    scans = [c, SM.sweep("ideal64", firings=256, world=2, seed=21, holes=("nan",))]   # (one that is handed back, one that stays, 16 384 points each)
    call = Call(scans)
    with context(scans, p) as ctx:
        ctx.set_front_mode(2)
        prepare(ctx)
        call.classify(ctx, p, times=2)
        if readout:
            ctx.ordered_indices(len(c[0]), 1)
        first = ctx.front_scans()
        ctx.enable_kernel_timing(1)
        ctx.kernel_timing()
        why = ctx.front_explain(0) if explain else None
        labels = call.classify(ctx, p)
        n_calls = ctx.kernel_timing()[1]
        return [l.copy() for l in labels], first, ctx.front_scans(), n_calls, why


@pytest.mark.parametrize("kind", ["fused", "sticky general", "fused with front_outputs"])
def test_an_explain_in_between_changes_nothing(kind):
    prepare = (lambda ctx: ctx.set_front_outputs(1)) if kind == "fused with front_outputs" else (lambda ctx: None)
    readout = kind != "fused"
    with_it, without = history(True, prepare, readout), history(False, prepare, readout)
    for a, b in zip(with_it[0], without[0]):
        assert np.array_equal(a, b)
    assert with_it[1:4] == without[1:4] and with_it[3] == 1
    why = with_it[4]
    if kind == "sticky general":   # the read-out ran the call again through the general kernels, and the context stays with them
        assert with_it[2] == 0 and (why["call"] == W["READOUT"]).all() and (why["advice"] & (A["RESET"] | A["FRONT_OUTPUTS"]) == A["RESET"] | A["FRONT_OUTPUTS"]).all()
    else:
        assert with_it[2] == 1 and why["fused"].tolist() == [0, 1] and (why["call"] == 0).all() and why["scan"][0] & S["MULTI_SECTOR"]


# ---- 5. refusals ----
def test_refusals():
    c, p, _ = small_cases()["ideal16"]
    n = len(c[0])
    rec = np.zeros((n, 4), np.float32)
    rec[:, 0], rec[:, 1], rec[:, 2] = c
    with u.Context(n, 1, params=p) as ctx:
        out = np.zeros(4, u.FRONT_WHY_DTYPE)
        explain = lambda layout, count: ctx._lib.urf_front_explain(ctx._h, layout, out.ctypes.data, count)   # noqa: E731
        assert explain(0, 1) == -1 and ctx._lib.urf_front_explain(ctx._h, 0, None, 0) == 0   # no call yet
        for _ in range(3):   # (the callback path settles on its sequence: a sweep that is run again becomes its row's latest submission)
            ctx.classify_pc2(rec, n, 16, 0, 4, 8)
        reruns = ctx.callback_path_state()[0]
        assert explain(0, 1) == 0
        t1 = ctx.classify_pc2_async(rec, n, 16, 0, 4, 8)
        t2 = ctx.classify_pc2_async(rec, n, 16, 0, 4, 8)
        ctx.classify_pc2_wait(t1)
        assert ctx.callback_path_state()[0] == reruns
        assert explain(0, 1) == -7   # URF_ERR_BUSY: the one scratch row has been resubmitted
        ctx.classify_pc2_wait(t2)
        assert explain(0, 2) == -1 and explain(0, 0) == -1 and explain(2, 1) == -1 and explain(-1, 1) == -1
        assert ctx._lib.urf_front_explain(ctx._h, 0, None, 1) == -1 and ctx._lib.urf_front_explain(ctx._h, 0, None, 0) == 1
        assert explain(0, 1) == 0
        why = ctx.front_explain(0)
        assert (why[0]["fused"], why[0]["call"], why[0]["advice"]) == (0, W["CALLBACK"], A["BATCH"] | A["MODE_2"])
        assert counters(why[0]) == SMALL["ideal16"]
