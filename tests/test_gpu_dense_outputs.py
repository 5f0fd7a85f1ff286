"""urf_set_dense_outputs(ctx, 1): after a dense call (urf_classify_batch_*_dense) the reference-order read-outs -- urf_ordered_indices,
urf_ordered_indices_batch, urf_clouds_batch_* with URF_ORDER_REFERENCE -- answer in the CALLER'S dense indices.  Every list against oracle
B run on the dense points, element by element, and against the same read-out after the ragged call on the same context; the clouds byte
for byte against the ragged call's; front mode 0 and 2, urf_set_front_outputs off and on; the edges of the re-alignment rule in one batch
with the stride exactly the dense max_len; a history on one context; the switch off (the refusals as ever); urf::BatchDetector.

One long-lived context per laser count, built as tests/test_gpu_dense.py builds them; oracle B runs once per dense scan (its ref())."""
import struct
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import dense_model as D
import sensor_models as SM
import urban_road_filter_amd as u
from hipmem import DevBuf
from test_gpu_dense import CASES, MAX_BATCH, SEEDS, Batch, code, dense_scan, equal_to_b, params, ref, twin_front_scans
from test_gpu_detector import build_demo

pytestmark = pytest.mark.gpu
ORDERS = ("road_order", "curb_order", "ring10_order")
NONE = 0xFFFFFFFF
FILL = 0xEEEEEEEE
_CTX = {}


@pytest.fixture(scope="module", autouse=True)
def _contexts():
    yield
    for c in _CTX.values():
        c.close()
    _CTX.clear()


def context(L, mode=2, outputs=0, dense_outputs=1, multi=0):
    """(sizes: tests/test_gpu_dense.py's context())  Every switch the tests of this module touch is set, whatever the test before left."""
    if L not in _CTX:
        _CTX[L] = u.Context(L * {16: 320, 32: 320, 64: 2048, 128: 300}[L], MAX_BATCH)
        if L == 128:
            _CTX[L].set_front_lasers128(1)
    ctx = _CTX[L]
    ctx.set_front_multi_sector(multi)
    ctx.set_front_mode(mode)
    ctx.set_front_outputs(outputs)
    ctx.set_dense_outputs(dense_outputs)
    ctx.set_dense_slots(None)
    return ctx


def batch_lists(ctx, S, stride, guard=64):
    """urf_ordered_indices_batch into buffers of exactly S * stride entries (+ guard words the call must not touch), all 0xEE before:
    -> per scan (road, curb, ring10); entries at or beyond a scan's count keep the pattern."""
    bufs = [DevBuf(4 * (S * stride + guard)) for _ in range(3)]
    dcnt = DevBuf(12 * S)
    for b in bufs + [dcnt]:
        b.fill(0xEE)
    ctx.ordered_indices_batch(*bufs, stride, dcnt)
    ctx.synchronize()
    cnt = dcnt.to_numpy(np.uint32).reshape(S, 3)
    out = []
    host = [b.to_numpy(np.uint32) for b in bufs]
    for k in range(3):
        assert (host[k][S * stride:] == FILL).all(), ("behind the lists", k)
    for s in range(S):
        row = []
        for k in range(3):
            a = host[k][s * stride:(s + 1) * stride]
            assert cnt[s][k] <= stride and (a[cnt[s][k]:] == FILL).all(), ("entries at or beyond the count", s, k)
            row.append(a[:cnt[s][k]].copy())
        out.append(tuple(row))
    return out


def check_lists(ctx, b, scans, p, roi, what, want=None, single=True):
    """Both read-outs against oracle B on the dense points (and `want`: the ragged call's); returns the batch read-out."""
    stride = max(max(b.lens), 1)
    got = batch_lists(ctx, b.S, stride)
    for s, sc in enumerate(scans):
        lb, ib, st = ref(sc, p, roi, debug=True)
        rows = [got[s]] + ([ctx.ordered_indices(max(b.lens[s], 1), scan=s)] if single else [])
        for row in rows:
            for k, key in enumerate(ORDERS):
                assert not (row[k] == NONE).any() and (row[k] < max(b.lens[s], 1)).all(), (what, s, key)
                exp = st[key] if ib["status"] == 0 else np.zeros(0, np.uint32)
                assert np.array_equal(row[k], exp), (what, s, key, len(row[k]), len(exp))
                if want is not None:
                    assert np.array_equal(row[k], want[s][k]), (what, "ragged", s, key)
    return got


def non_empty(scans, p, roi, ring10=True):
    for sc in scans:
        st = ref(sc, p, roi, debug=True)[2]
        assert len(st["road_order"]) > 0 and len(st["curb_order"]) > 0
        assert (len(st["ring10_order"]) > 0) == ring10


def refused(ctx, b, W, L):
    """The refusals of tests/test_gpu_dense.py::test_readouts_after_a_dense_call."""
    road, cnt3 = DevBuf(4 * b.S * W * L), DevBuf(12 * b.S)
    assert code(lambda: ctx.ordered_indices_batch(road, None, None, W * L, cnt3)) == -1
    assert b"dense" in ctx._lib.urf_last_error(ctx._h)
    assert code(lambda: ctx.ordered_indices(W * L, 0)) == -1
    cap = 3 * b.S * max(b.lens)
    drec, dcnt, doff = DevBuf(cap * 32), DevBuf(16 * b.S), DevBuf(32 * b.S)
    assert code(lambda: ctx.clouds_batch_soa(None, 1, drec, cap, dcnt, doff)) == -1
    assert code(lambda: ctx.read_stage(u.STAGE_ANGLE_TABLE, W * L, 0)) == -1


# ---- 1. the default: off ----
def test_the_switch_is_off_by_default_and_checks_its_argument():
    model, roi, L, W = "ideal64", "wide", 64, 259
    p = params(model, roi)
    scans = [dense_scan(model, s) for s in SEEDS[model][:2]]
    b = Batch([s[0] for s in scans], [s[1] for s in scans])
    with u.Context(L * 2048, 2, params=p) as ctx:   # a context nobody has switched anything on
        ctx.set_front_mode(2)
        equal_to_b(b.soa_dense(ctx, W, np.uint8), scans, p, roi, "default off")
        refused(ctx, b, W, L)
        assert ctx._lib.urf_set_dense_outputs(ctx._h, 2) == -1 and ctx._lib.urf_set_dense_outputs(ctx._h, -1) == -1
        refused(ctx, b, W, L)   # (a refused argument switches nothing on)
        ctx.set_dense_outputs(1)
        ctx.set_dense_outputs(0)
        refused(ctx, b, W, L)
        equal_to_b(b.soa_dense(ctx, W, np.uint8), scans, p, roi, "after the refusals")


# ---- 2. the lists ----
SETTINGS = {"mode0": (0, 0), "mode2": (2, 0), "mode2_outputs": (2, 1)}


@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("kind", ["soa", "pc2"])
@pytest.mark.parametrize("model", sorted(CASES))
def test_lists_in_dense_indices(model, kind, setting):
    roi, L = "wide", SM.lasers(model)
    mode, outputs = SETTINGS[setting]
    p = params(model, roi)
    scans = [dense_scan(model, s) for s in SEEDS[model][:3]]
    W = CASES[model][0] + 3
    clouds, ids = [s[0] for s in scans], [s[1] for s in scans]
    non_empty(scans, p, roi, ring10=model != "vlp16")
    multi = 1 if model == "hdl64e" else 0
    ctx = context(L, mode, outputs, multi=multi)
    ctx.set_params(p)
    b = Batch(clouds, ids)
    what = "%s %s %s" % (model, kind, setting)
    # the same read-outs after the ragged call, on this context
    b.soa_ragged(ctx) if kind == "soa" else b.pc2_ragged(ctx)
    want = check_lists(ctx, b, scans, p, roi, what + " ragged")
    ctx.set_front_mode(mode)   # (a read-out with urf_set_front_outputs off may have left the context with the general kernels)
    nf_twin = twin_front_scans(ctx, clouds, ids, L, W) if mode else 0
    if mode and model.startswith("ideal"):
        assert nf_twin == len(scans)
    for _ in range(2):   # (the second call: see twin_front_scans)
        got = b.soa_dense(ctx, W, np.uint8) if kind == "soa" else b.pc2_dense(ctx, W)
    equal_to_b(got, scans, p, roi, what)
    assert got[2] == nf_twin and got[3] == len(scans), (what, got[2:], nf_twin)
    check_lists(ctx, b, scans, p, roi, what, want)
    if outputs:
        assert ctx.front_scans() == nf_twin, what          # no second run: the call is still the fused one
        got = b.soa_dense(ctx, W, np.uint16) if kind == "soa" else b.pc2_dense(ctx, W)
        assert got[2] == nf_twin, what                     # ... and the next dense call is fused again
    else:
        check_lists(ctx, b, scans, p, roi, what + " again", want, single=False)   # (after the rerun: the record is the general kernels')
    ctx.set_dense_outputs(0)


# ---- 3. the edges of the rule, one batch, stride == the dense max_len ----
def test_edges_in_one_batch_with_the_smallest_stride():
    L, model, roi, W = 16, "ideal16", "wide", 290
    p = params(model, roi)
    a, c, m = dense_scan(model, 9, firings=280), dense_scan(model, 10, firings=280), dense_scan(model, 11, firings=280)
    cut = lambda s, n, tag: (tuple(v[:n].copy() for v in s[0]), s[1][:n].copy(), s[2], s[3] + (tag,))  # noqa: E731
    # two short firings that merge: firing f keeps its slots < 8, firing f + 1 its slots >= 8 -- the slots keep growing across the start
    slot = m[1]
    starts = np.nonzero(np.r_[True, slot[1:] <= slot[:-1]])[0]
    f = len(starts) // 2
    i0, i1, i2 = starts[f], starts[f + 1], starts[f + 2]
    keep = np.ones(len(slot), bool)
    keep[i0:i1] = slot[i0:i1] < 8
    keep[i1:i2] = slot[i1:i2] >= 8
    merged = (tuple(v[keep].copy() for v in m[0]), slot[keep].copy(), m[2], m[3] + ("merged",))
    assert D.realign(merged[1], L, W)[1] == len(starts) - 1 and D.realign(merged[1], L, W)[2]
    scans = [cut(a, 0, "cut0"), cut(c, 20, "cut20"), c, cut(a, 1000, "cut1000"), merged, a]
    ids = [s[1].copy() for s in scans]
    ids[2][len(ids[2]) // 2] = L        # a slot >= L
    ids[3][:] = 3                       # every point its own firing: more than W
    want = [True, True, False, False, True, True]
    assert [D.realign(i, L, W)[2] for i in ids] == want
    assert ref(scans[1], p, roi)[1]["status"] == 1   # URF_TOO_FEW_POINTS
    non_empty([scans[2], scans[4], scans[5]], p, roi)
    for mode, outputs in ((0, 0), (2, 1)):
        ctx = context(L, mode, outputs)
        ctx.set_params(p)
        b = Batch([s[0] for s in scans], ids)
        b.soa_ragged(ctx)
        ragged = check_lists(ctx, b, scans, p, roi, "edges ragged")
        ctx.set_front_mode(mode)
        got = b.soa_dense(ctx, W, np.uint8)
        equal_to_b(got, scans, p, roi, "edges")
        assert got[3] == sum(want)
        check_lists(ctx, b, scans, p, roi, "edges mode %d" % mode, ragged)   # (stride == max(b.lens), buffers of exactly that)
        # one entry less: refused, and the context keeps working
        stride = max(b.lens) - 1
        bufs, dcnt = [DevBuf(4 * b.S * stride) for _ in range(3)], DevBuf(12 * b.S)
        assert code(lambda: ctx.ordered_indices_batch(*bufs, stride, dcnt)) == -1
        check_lists(ctx, b, scans, p, roi, "edges after the refusal", ragged, single=False)
        got = b.pc2_dense(ctx, W)
        equal_to_b(got, scans, p, roi, "edges pc2")
        check_lists(ctx, b, scans, p, roi, "edges pc2", ragged)
    ctx.set_dense_outputs(0)


def test_scans_cut_at_max_len():
    """max_len below a scan's length: the scan is cut there (urf_dense_range), the lists are the cut scan's, as after the ragged call."""
    L, model, roi, W, n = 16, "ideal16", "wide", 290, 3000
    p = params(model, roi)
    a, c = dense_scan(model, 9, firings=280), dense_scan(model, 10, firings=280)
    cut = lambda s, k, tag: (tuple(v[:k].copy() for v in s[0]), s[1][:k].copy(), s[2], s[3] + (tag,))  # noqa: E731
    assert len(a[1]) > n and len(c[1]) > n
    scans = [cut(a, n, "cut3000"), cut(c, n, "cut3000"), cut(a, 1000, "cut1000")]   # (the third is shorter than max_len: whole)
    non_empty(scans[:2], p, roi)
    b = Batch([a[0], c[0], scans[2][0]], [a[1], c[1], scans[2][1]])
    seen = SimpleNamespace(S=3, lens=[n, n, 1000])
    ctx = context(L, 2, 1)
    ctx.set_params(p)
    ctx.classify_batch_soa_ragged(b.dx, b.dy, b.dz, b.do, n, b.S, b.dl, b.di)
    want = check_lists(ctx, seen, scans, p, roi, "cut ragged")
    did = DevBuf.from_numpy(b.I.astype(np.uint8))
    ctx.classify_batch_soa_dense(b.dx, b.dy, b.dz, did, 1, b.do, n, b.S, W, b.dl, b.di)
    check_lists(ctx, seen, scans, p, roi, "cut dense", want)
    assert ctx.dense_scans() == 3
    ctx.set_dense_outputs(0)


# ---- 4. the clouds in the reference's order ----
def records(b, step, intensity):
    """PointCloud2 bytes: x y z at 0 / 4 / 8, (step 32) intensity at 16 and a uint16 id at 20, (step 15) a uint16 id at 13; the rest 0xa5."""
    rec = np.frombuffer(b.records(step, 20 if step == 32 else 13, np.uint16), np.uint8).reshape(b.n, step).copy()
    if step == 32:
        rec[:, 16:20] = intensity.view(np.uint8).reshape(-1, 4)
    return np.ascontiguousarray(rec.reshape(-1))


def clouds_ref_order(ctx, kind, b, d_src, step, oi):
    cap = 3 * b.S * max(b.lens)
    drec, dcnt, doff = DevBuf(cap * 32), DevBuf(16 * b.S), DevBuf(32 * b.S)
    drec.fill(0)
    if kind == "soa":
        ctx.clouds_batch_soa(d_src, 1, drec, cap, dcnt, doff)
    else:
        ctx.clouds_batch_pc2(d_src, step, 0, 4, 8, oi, 1, drec, cap, dcnt, doff)
    ctx.synchronize()
    cnt, off = dcnt.to_numpy(np.uint32), doff.to_numpy(np.uint64)
    n = int(off[-1] + cnt[-1])
    return cnt, off, drec.to_numpy(np.uint8, n * 32)


@pytest.mark.parametrize("outputs", [0, 1])
@pytest.mark.parametrize("kind,step", [("soa", 0), ("pc2", 32), ("pc2", 15)])
def test_clouds_in_the_reference_order(kind, step, outputs):
    model, roi, L, W = "ideal64", "wide", 64, 259
    p = params(model, roi)
    scans = [dense_scan(model, s) for s in SEEDS[model][:3]]
    ctx = context(L, 2, outputs)
    ctx.set_params(p)
    b = Batch([s[0] for s in scans], [s[1] for s in scans])
    intensity = (np.arange(b.n, dtype=np.float32) * np.float32(0.25)).astype(np.float32)
    oi = 16 if step == 32 else -1
    if kind == "soa":
        d_src = DevBuf.from_numpy(intensity)
        b.soa_ragged(ctx)
    else:
        d_src = DevBuf.from_numpy(records(b, step, intensity))
        ring_off = 20 if step == 32 else 13
        ctx.classify_batch_pc2_ragged(d_src, b.do, b.n, max(b.lens), b.S, step, 0, 4, 8, b.dl, b.di)
    want = clouds_ref_order(ctx, kind, b, d_src, step, oi)
    cnt = want[0].reshape(-1, 4)
    assert cnt[:, 0].all() and cnt[:, 1].all() and cnt[:, 3].all()   # road, curb and road_probably records in every scan
    ctx.set_front_mode(2)
    for _ in range(2):
        if kind == "soa":
            got = b.soa_dense(ctx, W, np.uint8)
        else:
            b.dl.fill(0xEE)
            ctx.classify_batch_pc2_dense(d_src, b.do, b.n, max(b.lens), b.S, step, 0, 4, 8, ring_off, 2, W, b.dl, b.di)
            got = b.result(ctx) + (ctx.front_scans(), ctx.dense_scans())
    equal_to_b(got, scans, p, roi, "clouds")
    assert got[2] == b.S and got[3] == b.S
    have = clouds_ref_order(ctx, kind, b, d_src, step, oi)
    for name, x, y in zip(("counts", "offsets", "records"), want, have):
        assert np.array_equal(x, y), name
    # ... and what the oracle publishes: scan 1's road cloud is its points in road_order, the intensity the point's own
    st = ref(scans[1], p, roi, debug=True)[2]
    rec = have[2].view(np.float32).reshape(-1, 8)
    road = rec[int(have[1][4]):int(have[1][4]) + int(have[0][4])]
    order = st["road_order"].astype(np.int64)
    assert len(road) == len(order) and all(np.array_equal(road[:, k], scans[1][0][k][order]) for k in range(3))
    if oi >= 0 or kind == "soa":
        assert np.array_equal(road[:, 4], intensity[int(b.offs[1]) + order])
    assert ctx.front_scans() == (b.S if outputs else 0)   # (off: the documented rerun through the general kernels)
    ctx.set_dense_outputs(0)


# ---- 5. a history on one context ----
def test_history_on_one_context():
    model, roi, L = "ideal64", "wide", 64
    p = params(model, roi)
    ctx = context(L, 2, 1)
    ctx.set_params(p)
    first = [dense_scan(model, s) for s in SEEDS[model][:3]]
    b1 = Batch([s[0] for s in first], [s[1] for s in first])
    equal_to_b(b1.soa_dense(ctx, 259, np.uint8), first, p, roi, "first")
    check_lists(ctx, b1, first, p, roi, "first")
    check_lists(ctx, b1, first, p, roi, "first, the inverse kept", single=False)
    # other scans, fewer of them, other lengths, another W: an inverse left over from the first call would show
    second = [dense_scan(model, s, firings=128) for s in (5, 4)]
    b2 = Batch([s[0] for s in second], [s[1] for s in second])
    equal_to_b(b2.pc2_dense(ctx, 140), second, p, roi, "second")
    check_lists(ctx, b2, second, p, roi, "second")
    # the switch off: the refusals are back; on again: the same call answers
    ctx.set_dense_outputs(0)
    refused(ctx, b2, 140, L)
    ctx.set_dense_outputs(1)
    check_lists(ctx, b2, second, p, roi, "second, switched on again", single=False)
    assert code(lambda: ctx.read_stage(u.STAGE_ANGLE_TABLE, 140 * L, 0)) == -1   # stage values stay refused
    assert b"dense" in ctx._lib.urf_last_error(ctx._h)
    # a ragged call: as ever, whatever the switch says
    b1.soa_ragged(ctx)
    check_lists(ctx, b1, first, p, roi, "ragged")
    # ... and a plain batch call on padded twins: padded indices, as ever (the switch decides nothing)
    W = 259
    planes = [D.pad(s[0], D.realign(s[1], L, W)[0], L, W) for s in first[:2]]
    X, Y, Z = (DevBuf.from_numpy(np.concatenate([pl[k] for pl in planes])) for k in range(3))
    dl, di = DevBuf(2 * W * L), DevBuf(64)
    ctx.classify_batch_soa(X, Y, Z, W * L, 2, dl, di)
    ctx.synchronize()
    got = batch_lists(ctx, 2, W * L)
    for s in range(2):
        pos = D.realign(first[s][1], L, W)[0]
        st = ref(first[s], p, roi, debug=True)[2]
        for k, key in enumerate(ORDERS):
            assert np.array_equal(got[s][k], pos[st[key].astype(np.int64)]), ("plain", s, key)
    equal_to_b(b1.soa_dense(ctx, 259, np.uint16), first, p, roi, "dense again")
    check_lists(ctx, b1, first, p, roi, "dense again", single=False)
    ctx.set_dense_outputs(0)


# ---- 6. urf::BatchDetector ----
def test_batch_detector_reference_order_on_the_dense_path(tmp_path):
    exe = build_demo(tmp_path, "batch_dense_ref_demo")
    scans = [dense_scan("ideal64", s) for s in SEEDS["ideal64"][:4]]
    path = tmp_path / "clouds.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<III", len(scans), 64, 259))
        for k, (cloud, slot, _, _) in enumerate(scans):
            f.write(struct.pack("<I", len(slot)))
            for a in cloud + (np.arange(len(slot), dtype=np.float32) * np.float32(0.25) + np.float32(k),):
                f.write(np.ascontiguousarray(a, np.float32).tobytes())
            f.write(slot.astype(np.uint16).tobytes())
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    lines = r.stdout.splitlines()
    ring = [ln.split() for ln in lines if ln.startswith("ring ")]
    plain = [ln.split() for ln in lines if ln.startswith("plain ")]
    assert len(ring) == 1 and len(plain) == 1 and lines[-1] == "done", r.stdout
    w = dict(zip(ring[0][1::2], ring[0][2::2]))
    assert w == {"messages": "4", "published": "4", "points": w["points"], "ordered": "4", "equal": "4", "aligned": "4", "off_equal": "4",
                 "off_aligned": "0"} and int(w["points"]) > 4000, r.stdout
    w = dict(zip(plain[0][1::2], plain[0][2::2]))
    assert w == {"messages": "4", "equal": "4", "aligned": "0", "off_equal": "4", "off_aligned": "0"}, r.stdout
