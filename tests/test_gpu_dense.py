"""urf_classify_batch_soa_dense / urf_classify_batch_pc2_dense: dense sweeps (non-returns dropped) put back into firing slots by laser id
on the device, then classified as organised sweeps.  Every label and summary against oracle B run ON THE DENSE POINTS, bit for bit, and
against the ragged entry points on the same context; the fused front end really taken (front_scans equals the padded twin's); the edges
of the rule; the slot map; a history on one context; the read-outs after a dense call; the error codes; urf::BatchDetector.

Oracle B runs once per dense scan (ref()); a scan is at most 64 x 256 points.  One context per laser count for the whole module."""
import struct
import subprocess

import numpy as np
import pytest

import dense_model as D
import oracles as O
import sensor_models as SM
import urban_road_filter_amd as u
from hipmem import DevBuf
from test_gpu_detector import build_demo

pytestmark = pytest.mark.gpu
FIELDS = [k for k, _ in u.ScanInfo._fields_]
MAX_BATCH = 8
_REF, _SCAN, _CTX = {}, {}, {}

# model -> (firings, sweep keywords); batches are the seeds below
CASES = {
    "ideal64": (256, dict(drop=0.01)),                                        # 6-7 tiles: the prefixes cross tiles
    "hdl64e": (256, dict(noise=True, drop=0.01, holes=("zero", "nan1", "inf"))),   # range ties
    "ideal16": (304, dict(drop=0.01)),
    "ideal32": (136, dict(drop=0.01)),
    "vlp16": (304, dict(noise=True, drop=0.10)),
    "ideal128": (128, dict(drop=0.01)),
}
SEEDS = {"ideal64": (1, 2, 3, 4, 5, 6), "hdl64e": (1, 2, 3), "ideal16": (1, 2, 3), "ideal32": (1, 2, 3, 4), "vlp16": (1, 2, 3), "ideal128": (1, 2, 3)}


@pytest.fixture(scope="module", autouse=True)
def _contexts():
    yield
    for c in _CTX.values():
        c.close()
    _CTX.clear()


def context(L):
    """One long-lived context per laser count, MAX_BATCH scans, front mode 2: 320 firings of 16 / 32 points, 300 of 128, and 2048 of 64 --
    the fused front end's candidate list holds max(max_points / 8, 4096) entries per scan, and a 64-laser street seen all around (the wide
    region of interest) hands on about 64 x 68 of them however short the sweep is (URF_FRONT128_CAND_CAP, urf_front.hpp): a context sized for 64 x 300 points
    would hand every such sweep back for that reason alone."""
    if L not in _CTX:
        _CTX[L] = u.Context(L * {16: 320, 32: 320, 64: 2048, 128: 300}[L], MAX_BATCH)
        _CTX[L].set_front_mode(2)
        if L == 128:
            _CTX[L].set_front_lasers128(1)
    return _CTX[L]


def dense_scan(model, seed, firings=None, **kw):
    """(dense cloud, slot per point, firings) of one sweep, computed once."""
    F, base = CASES.get(model, (firings, {}))
    F = firings or F
    kw = dict(base, **kw)
    key = (model, seed, F, tuple(sorted(kw.items())))
    if key not in _SCAN:
        # (start 0: the sweep's seam at its start -- a seam inside a tile is handed back by contract, urf_front.hpp)
        cloud = SM.sweep(model, firings=F, world=seed % 3, seed=100 + seed, **kw)
        dense, slot = D.densify(cloud, SM.lasers(model), SM.missing_mask(cloud))
        _SCAN[key] = (dense, slot, F, key)
    return _SCAN[key]


def ref(scan, p, roi, debug=False):
    """Oracle B on the dense points of one scan, once per (scan, region of interest); never modified."""
    key = (scan[3], roi, debug)
    if key not in _REF:
        _REF[key] = O.run_b(*scan[0], p, debug=debug)
    return _REF[key]


def params(model, roi):
    """(ideal128's lasers stand 0.18 degrees apart: the reference's default ring tolerance, 0.18, merges neighbours into one ring, and a
    sweep whose lanes share rings is rightly handed back -- 0.05, as tests/test_gpu_front_lasers128.py sets for this model)"""
    return SM.params_for(model, wide=roi == "wide", interval=0.05 if model == "ideal128" else None)


class Batch:
    """The dense scans of one call on the device: SoA planes, ids, offsets, labels, infos."""

    def __init__(self, clouds, ids):
        self.clouds, self.ids = clouds, [np.asarray(i) for i in ids]
        self.lens = [len(c[0]) for c in clouds]
        self.S = len(clouds)
        self.offs = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.uint32)
        self.n = int(self.offs[-1])
        cat = lambda k: np.concatenate([c[k] for c in clouds]).astype(np.float32) if self.n else np.zeros(0, np.float32)  # noqa: E731
        self.X, self.Y, self.Z = cat(0), cat(1), cat(2)
        self.I = np.concatenate(self.ids).astype(np.int64) if self.n else np.zeros(0, np.int64)
        self.dx, self.dy, self.dz = (DevBuf.from_numpy(a) for a in (self.X, self.Y, self.Z))
        self.do = DevBuf.from_numpy(self.offs)
        self.dl, self.di = DevBuf(max(self.n, 1)), DevBuf(32 * self.S)

    def records(self, step, off_ring, ring_dtype):
        """PointCloud2 bytes: x y z at 0 / 4 / 8, the id at off_ring, every other byte 0xa5."""
        rec = np.full((self.n, step), 0xA5, np.uint8)
        for k, a in enumerate((self.X, self.Y, self.Z)):
            rec[:, 4 * k:4 * k + 4] = a.view(np.uint8).reshape(-1, 4)
        w = np.dtype(ring_dtype).itemsize
        rec[:, off_ring:off_ring + w] = self.I.astype(ring_dtype).view(np.uint8).reshape(-1, w)
        return np.ascontiguousarray(rec.reshape(-1))

    def result(self, ctx):
        ctx.synchronize()
        lab = self.dl.to_numpy(np.uint8)
        infos = self.di.to_numpy(np.uint32).reshape(self.S, 8)
        return [lab[self.offs[k]:self.offs[k + 1]].copy() for k in range(self.S)], infos

    def soa_dense(self, ctx, W, dtype=np.uint8):
        self.dl.fill(0xEE)
        self.did = DevBuf.from_numpy(self.I.astype(dtype))
        ctx.classify_batch_soa_dense(self.dx, self.dy, self.dz, self.did, np.dtype(dtype).itemsize, self.do, max(self.lens), self.S, W, self.dl, self.di)
        return self.result(ctx) + (ctx.front_scans(), ctx.dense_scans())

    def pc2_dense(self, ctx, W, step=32, off_ring=20, dtype=np.uint16):
        self.dl.fill(0xEE)
        self.dd = DevBuf.from_numpy(self.records(step, off_ring, dtype))
        ctx.classify_batch_pc2_dense(self.dd, self.do, self.n, max(self.lens), self.S, step, 0, 4, 8, off_ring, np.dtype(dtype).itemsize, W, self.dl,
                                     self.di)
        return self.result(ctx) + (ctx.front_scans(), ctx.dense_scans())

    def soa_ragged(self, ctx):
        self.dl.fill(0xEE)
        ctx.classify_batch_soa_ragged(self.dx, self.dy, self.dz, self.do, max(self.lens), self.S, self.dl, self.di)
        return self.result(ctx)

    def pc2_ragged(self, ctx, step=32):
        self.dl.fill(0xEE)
        self.dd = DevBuf.from_numpy(self.records(step, 20, np.uint16))
        ctx.classify_batch_pc2_ragged(self.dd, self.do, self.n, max(self.lens), self.S, step, 0, 4, 8, self.dl, self.di)
        return self.result(ctx)


def equal_to_b(got, scans, p, roi, what):
    labels, infos = got[0], got[1]
    for k, sc in enumerate(scans):
        lb, ib, _ = ref(sc, p, roi)
        assert np.array_equal(labels[k], lb), "%s, scan %d: %d labels differ" % (what, k, int((labels[k] != lb).sum()))
        assert [int(v) for v in infos[k].astype(np.int64)] == [ib[f] for f in FIELDS], (what, k)


def model_aligned(ids, L, W, slot_map=None):
    return sum(1 for i in ids if D.realign(i, L, W, slot_map)[2])


def twin_front_scans(ctx, clouds, ids, L, W, slot_map=None):
    """front_scans of classify_batch_soa on the padded twins built by the numpy model.  The second of two calls: a context's first call
    with new parameters may hand a sweep back whose speculative ring table was incomplete (tests/test_gpu_sensor_models.py), the dense
    calls that follow are compared with the settled state."""
    planes = [D.pad(c, D.realign(i, L, W, slot_map)[0], L, W) for c, i in zip(clouds, ids)]
    X, Y, Z = (DevBuf.from_numpy(np.concatenate([pl[k] for pl in planes])) for k in range(3))
    dl, di = DevBuf(W * L * len(clouds)), DevBuf(32 * len(clouds))
    for _ in range(2):
        ctx.classify_batch_soa(X, Y, Z, W * L, len(clouds), dl, di)
        ctx.synchronize()
    return ctx.front_scans()


# ---- 1. labels and infos, 2. the fused path is really taken ----
@pytest.mark.parametrize("roi", ["wide", "default"])
@pytest.mark.parametrize("model", sorted(CASES))
def test_labels_infos_and_the_fused_path(model, roi):
    L = SM.lasers(model)
    p = params(model, roi)
    scans = [dense_scan(model, s) for s in SEEDS[model]]
    W = CASES[model][0] + 3
    clouds, ids = [s[0] for s in scans], [s[1] for s in scans]
    if roi == "wide":   # (no comparison passes on empty results)
        assert any(ref(s, p, roi)[1]["n_road"] > 0 and ref(s, p, roi)[1]["n_curb"] > 0 for s in scans)
    ctx = context(L)
    ctx.set_params(p)
    ctx.set_dense_slots(None)
    b = Batch(clouds, ids)
    want_aligned = model_aligned(ids, L, W)
    assert want_aligned == len(scans)
    nf_twin = twin_front_scans(ctx, clouds, ids, L, W)
    if model.startswith("ideal"):
        assert nf_twin == len(scans)
    runs = [("soa u8", lambda: b.soa_dense(ctx, W, np.uint8)), ("soa u16", lambda: b.soa_dense(ctx, W, np.uint16)),
            ("pc2 32 u16@20", lambda: b.pc2_dense(ctx, W, 32, 20, np.uint16)), ("pc2 32 u8@20", lambda: b.pc2_dense(ctx, W, 32, 20, np.uint8)),
            ("pc2 15 u16@13", lambda: b.pc2_dense(ctx, W, 15, 13, np.uint16)), ("pc2 15 u8@13", lambda: b.pc2_dense(ctx, W, 15, 13, np.uint8))]
    for what, run in runs:
        got = run()
        equal_to_b(got, scans, p, roi, "%s %s %s" % (model, roi, what))
        assert got[2] == nf_twin, (what, got[2], nf_twin)
        assert got[3] == want_aligned, (what, got[3])
    for what, got in (("soa ragged", b.soa_ragged(ctx)), ("pc2 ragged", b.pc2_ragged(ctx))):
        equal_to_b(got, scans, p, roi, "%s %s %s" % (model, roi, what))


# ---- 3. edges ----
def test_edges_in_one_batch():
    L, model, roi = 16, "ideal16", "wide"
    p = params(model, roi)
    many = dense_scan(model, 7, firings=300, drop=0.1)               # W + 1 firings below
    W = D.realign(many[1], L, 1 << 20)[1] - 1
    full = dense_scan(model, 8, firings=W, drop=0.0)                 # no holes at all: exactly W firings, a start every L points
    assert len(full[1]) == W * L
    a, c = dense_scan(model, 9, firings=280), dense_scan(model, 10, firings=280)   # (at most W * L points each)
    cut = lambda s, n, tag: (tuple(v[:n].copy() for v in s[0]), s[1][:n].copy(), s[2], s[3] + (tag,))  # noqa: E731
    scans = [cut(a, 0, "cut0"), cut(a, 1, "cut1"), cut(c, 20, "cut20"), full, cut(a, 1000, "cut1000"), c, many, a]
    ids = [s[1].copy() for s in scans]
    ids[4][:] = 3                                                    # every point its own firing: more than W
    ids[5][len(ids[5]) // 2] = L                                     # one id == L
    want = [True, True, True, True, False, False, False, True]
    assert [D.realign(i, L, W)[2] for i in ids] == want
    assert D.realign(ids[3], L, W)[1] == W and D.realign(ids[6], L, W)[1] == W + 1
    assert ref(scans[2], p, roi)[1]["status"] == 1 and ref(scans[3], p, roi)[1]["n_road"] > 0
    ctx = context(L)
    ctx.set_params(p)
    ctx.set_dense_slots(None)
    b = Batch([s[0] for s in scans], ids)
    for what, run in (("soa", lambda: b.soa_dense(ctx, W, np.uint8)), ("pc2", lambda: b.pc2_dense(ctx, W))):
        got = run()
        equal_to_b(got, scans, p, roi, "edges " + what)
        assert got[3] == sum(want), (what, got[3])
    equal_to_b(b.soa_ragged(ctx), scans, p, roi, "edges ragged")


# ---- 4. the slot map ----
def test_slot_map_hdl32e_ranks():
    model, roi, L = "hdl32e", "wide", 32
    p = params(model, roi)
    scans = [dense_scan(model, s, firings=136, drop=0.01) for s in (1, 2, 3)]
    W = 139
    rank = np.argsort(np.argsort(SM.MODELS[model]["elev"])).astype(np.int64)   # the driver's ring: by elevation
    slot_of_rank = np.argsort(rank).astype(np.uint8)
    assert (slot_of_rank[rank] == np.arange(L)).all() and (rank != np.arange(L)).any()
    clouds, slots = [s[0] for s in scans], [s[1] for s in scans]
    ranks = [rank[s] for s in slots]
    ctx = context(L)
    ctx.set_params(p)
    ctx.set_dense_slots(None)
    direct = Batch(clouds, slots).soa_dense(ctx, W, np.uint8)
    equal_to_b(direct, scans, p, roi, "direct slots")
    assert direct[3] == len(scans)
    br = Batch(clouds, ranks)
    ctx.set_dense_slots(slot_of_rank)
    mapped = br.pc2_dense(ctx, W)
    equal_to_b(mapped, scans, p, roi, "ranks through the map")
    assert mapped[2:] == direct[2:], (mapped[2:], direct[2:])
    ctx.set_dense_slots(None)
    unmapped = br.soa_dense(ctx, W, np.uint16)                       # wrong ids cost speed only
    equal_to_b(unmapped, scans, p, roi, "ranks without the map")
    assert unmapped[3] == model_aligned(ranks, L, W)
    again = Batch(clouds, slots).soa_dense(ctx, W, np.uint8)         # the identity is back
    assert again[2:] == direct[2:] and all(np.array_equal(x, y) for x, y in zip(again[0], direct[0]))
    ctx.set_dense_slots(slot_of_rank[:7])                            # ids at or beyond n_ids: not aligned, labels still right
    short = br.soa_dense(ctx, W, np.uint8)
    equal_to_b(short, scans, p, roi, "a map of 7 ids")
    assert short[3] == 0
    ctx.set_dense_slots(None)


# ---- 5. history on one context ----
def test_history_long_then_short_then_plain_then_a_sweep_in_flight():
    model, roi, L = "ideal64", "wide", 64
    p = params(model, roi)
    ctx = context(L)
    ctx.set_params(p)
    ctx.set_dense_slots(None)
    long_scans = [dense_scan(model, s) for s in SEEDS[model]]
    b = Batch([s[0] for s in long_scans], [s[1] for s in long_scans])
    equal_to_b(b.soa_dense(ctx, 259, np.uint16), long_scans, p, roi, "long")
    short_scans = [dense_scan("hdl64e", s, firings=128) for s in (4, 5)]   # fewer scans, fewer points, another W: a stale staging shows
    ps = params("hdl64e", roi)
    ctx.set_params(ps)
    bs = Batch([s[0] for s in short_scans], [s[1] for s in short_scans])
    got = bs.pc2_dense(ctx, 140)
    equal_to_b(got, short_scans, ps, roi, "short after long")
    assert got[3] == 2
    # a plain PointCloud2 batch of organised sweeps (holes in place)
    org = [SM.sweep("hdl64e", firings=128, world=1, seed=300 + k, noise=True) for k in range(2)]
    n = len(org[0][0])
    rec = np.zeros((2 * n, 4), np.float32)
    for k in range(3):
        rec[:, k] = np.concatenate([c[k] for c in org])
    dd, dl, di = DevBuf.from_numpy(rec), DevBuf(2 * n), DevBuf(64)
    ctx.classify_batch_pc2(dd, n, 2, 16, 0, 4, 8, dl, di)
    ctx.synchronize()
    lab = dl.to_numpy(np.uint8)
    for k in range(2):
        lb, ib, _ = O.run_b(*org[k], ps)
        assert np.array_equal(lab[k * n:(k + 1) * n], lb), "plain pc2 batch, scan %d" % k
    assert ctx.dense_scans() == 2   # (still the last dense call's)
    # a sweep of the callback path in flight while a dense call is submitted
    one = np.ascontiguousarray(rec[:n])
    t = ctx.classify_pc2_async(one.view(np.uint8).reshape(-1), n, 16, 0, 4, 8)
    got = bs.soa_dense(ctx, 140, np.uint8)
    sweep_labels = np.zeros(n, np.uint8)
    info = ctx.classify_pc2_wait(t, sweep_labels)
    equal_to_b(got, short_scans, ps, roi, "dense next to a sweep in flight")
    lb, ib, _ = O.run_b(*org[0], ps)
    assert np.array_equal(sweep_labels, lb) and info.n_road == ib["n_road"]
    ctx.set_params(p)
    equal_to_b(b.soa_dense(ctx, 259, np.uint8), long_scans, p, roi, "long again")


# ---- 6. read-outs after a dense call ----
def clouds_of(ctx, kind, b, cap, order=0, step=32):
    drec, dcnt, doff = DevBuf(cap * 32), DevBuf(16 * b.S), DevBuf(32 * b.S)
    drec.fill(0)
    if kind == "soa":
        ctx.clouds_batch_soa(None, order, drec, cap, dcnt, doff)
    else:
        ctx.clouds_batch_pc2(b.dd, step, 0, 4, 8, -1, order, drec, cap, dcnt, doff)
    ctx.synchronize()
    cnt, off = dcnt.to_numpy(np.uint32), doff.to_numpy(np.uint64)
    n = int(off[-1] + cnt[-1])
    return cnt, off, drec.to_numpy(np.uint8, n * 32)


def code(f):
    try:
        f()
    except u.UrfError as e:
        return e.code
    return 0


@pytest.mark.parametrize("kind", ["soa", "pc2"])
def test_readouts_after_a_dense_call(kind):
    model, roi, L, W = "ideal64", "wide", 64, 259
    p = params(model, roi)
    scans = [dense_scan(model, s) for s in SEEDS[model][:3]]
    ctx = context(L)
    ctx.set_params(p)
    ctx.set_dense_slots(None)
    b = Batch([s[0] for s in scans], [s[1] for s in scans])
    cap = 3 * b.S * max(b.lens)
    b.soa_ragged(ctx) if kind == "soa" else b.pc2_ragged(ctx)
    want = clouds_of(ctx, kind, b, cap)
    assert want[0].reshape(-1, 4)[:, 0].all() and want[0].reshape(-1, 4)[:, 1].all()   # (road and curb records in every scan)
    for _ in range(2):   # (the second call: see twin_front_scans)
        got = b.soa_dense(ctx, W, np.uint8) if kind == "soa" else b.pc2_dense(ctx, W)
    assert got[2] == b.S
    have = clouds_of(ctx, kind, b, cap)
    assert all(np.array_equal(x, y) for x, y in zip(want, have)), "the four clouds in input order"
    # the refused read-outs, and the context afterwards
    road = DevBuf(4 * b.S * W * L)
    cnt3 = DevBuf(12 * b.S)
    assert code(lambda: ctx.ordered_indices_batch(road, None, None, W * L, cnt3)) == -1
    assert b"dense" in ctx._lib.urf_last_error(ctx._h)
    assert code(lambda: ctx.ordered_indices(W * L, 0)) == -1
    assert code(lambda: ctx.read_stage(u.STAGE_ANGLE_TABLE, W * L, 0)) == -1
    assert code(lambda: clouds_of(ctx, kind, b, cap, order=1)) == -1
    assert ctx.front_scans() == b.S and ctx.dense_scans() == b.S
    # marker points: coordinates, from the padded batch the context owns
    dpts, dn = DevBuf(b.S * 361 * 16), DevBuf(4 * b.S)
    ctx.marker_points_batch(dpts, dn)
    ctx.synchronize()
    pts, n = dpts.to_numpy(np.float32).reshape(b.S, 361, 4), dn.to_numpy(np.uint32)
    for k, sc in enumerate(scans):
        st = ref(sc, p, roi, debug=True)[2]
        assert len(st["marker_pts"]) > 2
        assert int(n[k]) == len(st["marker_pts"]) and np.array_equal(pts[k, :n[k]].view(np.uint32), st["marker_pts"].view(np.uint32)), k
    assert np.array_equal(ctx.marker_points(scan=1), ref(scans[1], p, roi, debug=True)[2]["marker_pts"])
    ctx.set_front_mode(2)   # (the marker points of a fused call ran it again through the general kernels: fused again from here)
    equal_to_b(b.soa_dense(ctx, W, np.uint16), scans, p, roi, "after the read-outs")
    assert ctx.front_scans() == b.S


# ---- 7. errors ----
def test_error_codes():
    L, W = 16, 304
    ctx = context(L)
    p = params("ideal16", "wide")
    ctx.set_params(p)
    ctx.set_dense_slots(None)
    sc = dense_scan("ideal16", 1)
    b = Batch([sc[0]], [sc[1]])
    ids = DevBuf.from_numpy(b.I.astype(np.uint8))
    rec = DevBuf.from_numpy(b.records(32, 20, np.uint16))
    n = b.lens[0]
    soa = lambda **k: code(lambda: ctx.classify_batch_soa_dense(k.get("x", b.dx), b.dy, b.dz, k.get("ids", ids), k.get("bytes", 1), k.get("offs", b.do),  # noqa: E731
                                                               k.get("max_len", n), k.get("S", 1), k.get("W", W), k.get("labels", b.dl), b.di))
    pc2 = lambda **k: code(lambda: ctx.classify_batch_pc2_dense(k.get("data", rec), k.get("offs", b.do), k.get("total", n), k.get("max_len", n),  # noqa: E731
                                                               k.get("S", 1), k.get("step", 32), 0, 4, 8, k.get("off", 20), k.get("bytes", 2), k.get("W", W),
                                                               k.get("labels", b.dl), b.di))
    assert soa() == 0 and pc2() == 0
    for f in (soa, pc2):
        assert f(W=321) == -4                      # W * L > max_points
        assert f(W=(n - 1) // L) == -4             # max_len > W * L
        assert f(W=0) == -4 and f(W=0, max_len=0) == -1
        assert f(S=MAX_BATCH + 1) == -4
        assert f(bytes=0) == -1 and f(bytes=3) == -1 and f(bytes=4) == -1
        assert f(offs=None) == -1 and f(labels=None) == -1
        assert f(S=0) == 0                         # a no-op
    assert soa(x=None) == -1 and soa(ids=None) == -1
    assert pc2(data=None) == -1
    assert pc2(off=31) == -1 and pc2(off=31, bytes=1) == 0 and pc2(off=30) == 0 and pc2(off=32, bytes=1) == -1
    assert pc2(total=L * 320 * MAX_BATCH + 1) == -4
    assert code(lambda: ctx.set_dense_slots(np.zeros(257, np.uint8))) == -1
    ctx.set_dense_slots(np.arange(256, dtype=np.uint8))
    ctx.set_dense_slots(None)
    got = b.soa_dense(ctx, W, np.uint8)            # and the context still works
    equal_to_b(got, [sc], p, "wide", "after the errors")
    assert got[3] == 1


# ---- 8. urf::BatchDetector ----
def test_batch_detector_with_and_without_realignment(tmp_path):
    exe = build_demo(tmp_path, "batch_dense_demo")
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
    assert w == {"messages": "4", "published": "4", "points": w["points"], "equal": "4", "aligned": "4"} and int(w["points"]) > 4000, r.stdout
    w = dict(zip(plain[0][1::2], plain[0][2::2]))
    assert w == {"messages": "4", "equal": "4", "aligned": "0"}, r.stdout
