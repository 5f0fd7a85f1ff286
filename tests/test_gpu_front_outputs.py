"""urf_set_front_outputs(ctx, 1): the published order (urf_ordered_indices*, urf_clouds_batch_* in the reference order) and the road_marker
points (urf_marker_points*) of a call that took the fused front end, read from what that call left on the device
(urban_road_filter_amd/csrc/urf_k_front_outputs.hpp) -- no second run through the general kernels, the context stays fused, the caller's
labels are only read.  Every list and every marker point against oracle B (road_order, curb_order, ring10_order, marker_pts), exact:
firing order and row-major, batches and the callback path, batches that mix fused and handed-back scans, rings with bit-equal azimuths
(the literal quicksort), 16 / 32 / 64 / 128 lasers, other curbPoints in mode 3, partial tiles, rings longer than 2048 points (with bit-equal azimuths too: general
and fused kernels), drop-outs in every encoding, empty rings; the switch off; the error codes."""
import numpy as np
import pytest

import oracles as O
import sensor_models as SM
import urban_road_filter_amd as u
from hipmem import DevBuf
from test_gpu_batch_clouds import XYZI, Batch
from test_gpu_front import ring_major, rolled

pytestmark = pytest.mark.gpu
N = 64 * 2048
_REF = {}


def ref(key, cloud, p):
    """Oracle B on one input, computed once (labels, summary, stages); never modified."""
    if key not in _REF:
        _REF[key] = O.run_b(*cloud, p, debug=True)
    return _REF[key]


def three():
    return [("cfg2", 1), ("sensor", 1), ("narrow", 2)]


def three_scans(rows=False):
    scans = [O.cfg_cloud(n, s) for n, s in three()]
    return [ring_major(c) for c in scans] if rows else scans


def three_refs(p, rows=False):
    return [ref((n, s, rows), c, p) for (n, s), c in zip(three(), three_scans(rows))]


class Soa:
    """A SoA batch on the device (fixed length or ragged) and its label buffer."""

    def __init__(self, scans):
        self.scans = scans
        self.lens = [len(s[0]) for s in scans]
        self.offs = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.uint32)
        self.d = [DevBuf.from_numpy(np.concatenate([s[k] for s in scans]).astype(np.float32)) for k in range(3)]
        self.do = DevBuf.from_numpy(self.offs)
        self.dl = DevBuf(int(self.offs[-1]))
        self.di = DevBuf(32 * len(scans))

    def classify(self, ctx):
        if len(set(self.lens)) == 1:
            ctx.classify_batch_soa(*self.d, self.lens[0], len(self.scans), self.dl, self.di)
        else:
            ctx.classify_batch_soa_ragged(*self.d, self.do, max(self.lens), len(self.scans), self.dl, self.di)
        ctx.synchronize()

    def label_bytes(self):
        return self.dl.to_numpy(np.uint8).copy()

    def labels(self):
        L = self.label_bytes()
        return [L[a:b] for a, b in zip(self.offs[:-1], self.offs[1:])]


def batch_readouts(ctx, S, stride):
    """urf_ordered_indices_batch + urf_marker_points_batch -> per scan (road, curb, ring10, marker points)"""
    lists = [DevBuf(4 * S * stride) for _ in range(3)]
    dcnt, dpts, dn = DevBuf(12 * S), DevBuf(16 * 361 * S), DevBuf(4 * S)
    for b in lists + [dcnt, dpts, dn]:
        b.fill(0xEE)
    ctx.ordered_indices_batch(*lists, stride, dcnt)
    ctx.marker_points_batch(dpts, dn)
    ctx.synchronize()
    cnt = dcnt.to_numpy(np.uint32).reshape(S, 3)
    host = [b.to_numpy(np.uint32).reshape(S, stride) for b in lists]
    pts = dpts.to_numpy(np.float32).reshape(S, 361, 4)
    n = dn.to_numpy(np.uint32)
    return [tuple(host[k][s][:cnt[s][k]] for k in range(3)) + (pts[s][:n[s]],) for s in range(S)]


def same(got, st, what):
    for k, name in enumerate(("road_order", "curb_order", "ring10_order")):
        assert np.array_equal(got[k], st[name]), (what, name, len(got[k]), len(st[name]))
    assert got[3].shape == st["marker_pts"].shape and np.array_equal(got[3].view(np.uint32), st["marker_pts"].view(np.uint32)), (what, "marker_pts")


def check_readouts(ctx, refs, stride, single=True, what=""):
    S = len(refs)
    for s, got in enumerate(batch_readouts(ctx, S, stride)):
        same(got, refs[s][2], (what, "batch", s))
    if single:
        for s in range(S):
            same(ctx.ordered_indices(stride, scan=s) + (ctx.marker_points(scan=s),), refs[s][2], (what, "single", s))


def check_labels(b, refs):
    for s, lab in enumerate(b.labels()):
        assert np.array_equal(lab, refs[s][0]), s


# ---- 1. firing order, 64 lasers ----
def test_firing_order_batch_keeps_the_fused_call():
    p = O.cfg_params("cfg2")
    scans, refs = three_scans(), three_refs(p)
    assert all(r[1]["status"] == 0 and r[1]["n_road"] > 0 and len(r[2]["marker_pts"]) > 2 for r in refs)
    b = Batch(scans, XYZI)
    with u.Context(N, 3, params=p) as ctx:
        ctx.set_front_mode(2)
        ctx.set_front_outputs(1)
        labels, _ = b.classify(ctx, "soa")
        assert ctx.front_scans() == 3
        before = b.dl.to_numpy(np.uint8).copy()
        assert all(np.array_equal(a, r[0]) for a, r in zip(labels, refs))
        check_readouts(ctx, refs, N, what="firing")
        b.check_clouds(ctx, "soa", u.ORDER_REFERENCE, p)
        assert ctx.front_scans() == 3                                   # no second run: still the fused call's
        assert np.array_equal(b.dl.to_numpy(np.uint8), before)          # the caller's labels: read, never written
        labels, _ = b.classify(ctx, "soa")                              # ... and the context is still fused, without a set_front_mode
        assert ctx.front_scans() == 3
        assert all(np.array_equal(a, r[0]) for a, r in zip(labels, refs))   # (the read-outs left nothing behind that disturbs it)
        check_readouts(ctx, refs, N, single=False, what="firing, second call")
        # urf_read_stage keeps the second run in either switch position (stage values are the general kernels')
        assert np.array_equal(ctx.read_stage(u.STAGE_DETECT, N, scan=1), refs[1][2]["detect"])
        assert ctx.front_scans() == 0
        check_readouts(ctx, refs, N, single=False, what="after read_stage")


# ---- 2. the switch off equals today ----
def test_switch_off_runs_the_call_again():
    p = O.cfg_params("cfg2")
    scans, refs = three_scans(), three_refs(p)
    b = Soa(scans)
    with u.Context(N, 3, params=p) as ctx:
        ctx.set_front_mode(2)
        ctx.set_front_outputs(1)
        ctx.set_front_outputs(0)
        b.classify(ctx)
        assert ctx.front_scans() == 3
        check_readouts(ctx, refs, N, what="off")
        assert ctx.front_scans() == 0
        check_labels(b, refs)
        b.classify(ctx)
        assert ctx.front_scans() == 0                                   # (the context stays with the general kernels)
        ctx.set_front_outputs(1)
        ctx.set_front_mode(2)
        b.classify(ctx)
        assert ctx.front_scans() == 3
        check_readouts(ctx, refs, N, single=False, what="on again")
        assert ctx.front_scans() == 3


# ---- 3. row-major ----
@pytest.mark.parametrize("kind", ["soa", "pc2"])
def test_row_major_batches(kind):
    p = O.cfg_params("cfg2")
    scans, refs = three_scans(rows=True), three_refs(p, rows=True)
    b = Batch(scans, XYZI)
    with u.Context(N, 3, params=p) as ctx:
        ctx.set_front_mode(2)
        ctx.set_front_outputs(1)
        b.classify(ctx, kind)                                           # (a context's first call only sights the layout)
        labels, _ = b.classify(ctx, kind)
        assert ctx.front_scans() == 3
        before = b.dl.to_numpy(np.uint8).copy()
        assert all(np.array_equal(a, r[0]) for a, r in zip(labels, refs))
        check_readouts(ctx, refs, N, what=("rows", kind))
        b.check_clouds(ctx, kind, u.ORDER_REFERENCE, p)
        assert ctx.front_scans() == 3 and np.array_equal(b.dl.to_numpy(np.uint8), before)
        labels, _ = b.classify(ctx, kind)
        assert ctx.front_scans() == 3
        assert all(np.array_equal(a, r[0]) for a, r in zip(labels, refs))
        check_readouts(ctx, refs, N, single=False, what=("rows, next call", kind))


# ---- 4. row-major on the callback path ----
def test_row_major_sweep_of_the_callback_path():
    p = O.cfg_params("cfg2")
    rows = three_scans(rows=True)
    refs = three_refs(p, rows=True)
    with u.Context(N, 4, params=p) as ctx:
        ctx.set_front_outputs(1)
        fused = 0
        for rep in range(4):                                            # (fused from the context's second or third such sweep on)
            for k, c in enumerate(rows):
                lab, info = ctx.classify_xyz(*c)
                assert np.array_equal(lab, refs[k][0]), (rep, k)
                fused = ctx.front_scans()
        assert fused == 1
        lab, info = ctx.classify_xyz(*rows[1])
        assert ctx.front_scans() == 1
        state = ctx.callback_path_state()
        same(ctx.ordered_indices(N) + (ctx.marker_points(),), refs[1][2], "callback path")
        assert ctx.callback_path_state() == state and ctx.front_scans() == 1
        lab, info = ctx.classify_xyz(*rows[2])                          # the next sweep takes the fused kernels again
        assert np.array_equal(lab, refs[2][0]) and ctx.front_scans() == 1
        same(ctx.ordered_indices(N) + (ctx.marker_points(),), refs[2][2], "callback path, next sweep")
        rec = np.zeros((N, 5), np.float32)                              # ... and one as PointCloud2 records (x at 4, y at 12, z at 8)
        rec[:, 1], rec[:, 3], rec[:, 2] = rows[0]
        lab, info = ctx.classify_pc2(rec, N, 20, 4, 12, 8)
        assert np.array_equal(lab, refs[0][0]) and ctx.front_scans() == 1
        state = ctx.callback_path_state()
        same(ctx.ordered_indices(N) + (ctx.marker_points(),), refs[0][2], "callback path, classify_pc2")
        assert ctx.callback_path_state() == state and ctx.front_scans() == 1


# ---- 5. a batch that mixes fused and handed-back scans ----
def test_mixed_batch():
    """Two fusable sweeps around one stored from another column (its sectors fall inside a tile: handed back): two fused scans before and
    after the read-outs.  Then the same with a scan below the 30-point threshold behind them: it publishes nothing, and urf_front_scans
    counts it as well -- it keeps its flag, as tests/test_gpu_front.py pins ("nothing is published for it either way") --, so three."""
    p = O.cfg_params("cfg2")
    few = tuple(a.copy() for a in O.cfg_cloud("cfg2", 6))
    few[0][29:] = 1.0e6
    named = [(("cfg2", 1, False), O.cfg_cloud("cfg2", 1)), (("narrow", 4, "rolled700"), rolled(O.cfg_cloud("narrow", 4), 700)),
             (("sensor", 1, False), O.cfg_cloud("sensor", 1)), (("cfg2", 6, "few"), few)]
    refs = [ref(k, c, p) for k, c in named]
    assert [r[1]["status"] for r in refs[:3]] == [0, 0, 0] and refs[3][1]["status"] != 0
    with u.Context(N, 4, params=p) as ctx:
        ctx.set_front_mode(2)
        ctx.set_front_outputs(1)
        for n_scans, flagged in ((3, 2), (4, 3), (4, 3)):               # (the general kernels list-driven, then as full grids)
            b = Soa([c for _, c in named[:n_scans]])
            b.classify(ctx)
            infos = b.di.to_numpy(np.uint32).reshape(n_scans, 8)
            assert [int(np.int32(i[0])) for i in infos] == [r[1]["status"] for r in refs[:n_scans]]
            nf = ctx.front_scans()
            assert nf == flagged
            check_labels(b, refs)
            before = b.label_bytes()
            check_readouts(ctx, refs[:n_scans], N, what=("mixed", n_scans))
            assert ctx.front_scans() == flagged and np.array_equal(b.label_bytes(), before)


# ---- 6. equal azimuths: the literal quicksort ----
def repeated_firings(cloud, every, lasers=64):
    out = tuple(a.copy() for a in cloud)
    for A in out:
        R = A.reshape(-1, lasers)
        R[every::every] = R[every - 1::every][:len(R[every::every])]
    return out


def equal_azimuth_pairs(st):
    """Pairs of points of one ring whose azimuths are equal bit for bit (oracle B's stages)."""
    ring, az = st["ring"], st["azimuth"].view(np.uint32)
    on = ring >= 0
    key = (ring[on].astype(np.uint64) << np.uint64(32)) | az[on].astype(np.uint64)
    _, counts = np.unique(key, return_counts=True)
    return int((counts - 1).sum())


def nudged(cloud, every, st, lasers=64):
    """repeated_firings, and of every pair one of which is a marker point (st: oracle B on the repeated cloud) one point's z a float step
    up, the first and the second of the pair in turn: the two keep azimuth and planar distance, bit for bit, and differ in z -- WHICH of
    them the marker pass takes shows in the marker point.  (Every repeated firing moved that way leaves no road point.)"""
    out = repeated_firings(cloud, every, lasers)
    x, y, z = out
    mk = {(m[0].tobytes(), m[1].tobytes(), m[2].tobytes()) for m in st["marker_pts"]}
    R = np.arange(len(x)).reshape(-1, lasers)
    k = 0
    for fr in range(every, R.shape[0], every):
        for i, j in zip(R[fr - 1], R[fr]):
            if (x[i].tobytes(), y[i].tobytes(), z[i].tobytes()) in mk:
                z[j if k & 1 else i] = np.nextafter(z[i], np.float32(np.inf))
                k += 1
    return out


def order_decides(cloud, st):
    """Marker points whose (x, y) another point of the cloud shares with a different z."""
    x, y, z = cloud
    keys = {}
    for i in np.nonzero(st["ring"] >= 0)[0]:
        keys.setdefault((x[i].tobytes(), y[i].tobytes()), set()).add(z[i].tobytes())
    return sum(1 for m in st["marker_pts"] if len(keys.get((m[0].tobytes(), m[1].tobytes()), ())) > 1)


@pytest.mark.parametrize("variant", ["repeated", "nudged"])
def test_equal_azimuths_follow_the_reference_quicksort(variant):
    p = O.cfg_params("cfg2")
    want = {"cfg2": (54020, 681, 360), "sensor": (26192, 694, 260)}
    named = [((n, 1, "repeated8"), repeated_firings(O.cfg_cloud(n, 1), 8)) for n in ("cfg2", "sensor")]
    if variant == "nudged":
        named = [((k[0], 1, "nudged8"), nudged(O.cfg_cloud(k[0], 1), 8, ref(k, c, p)[2])) for k, c in named]
    refs = [ref(k, c, p) for k, c in named]
    for (k, c), r in zip(named, refs):
        assert r[1]["status"] == 0 and r[1]["n_rings"] == 64
        assert equal_azimuth_pairs(r[2]) > 10000, equal_azimuth_pairs(r[2])
        if variant == "repeated":
            assert (len(r[2]["road_order"]), len(r[2]["curb_order"]), len(r[2]["marker_pts"])) == want[k[0]]
        else:   # the literal marker pass: the order of a pair with one azimuth and one distance decides marker points
            assert order_decides(c, r[2]) >= 20 and r[1]["n_road"] > 20000
    b = Soa([c for _, c in named])
    with u.Context(N, 2, params=p) as ctx:
        ctx.set_front_mode(2)
        ctx.set_front_outputs(1)
        b.classify(ctx)
        assert ctx.front_scans() == 2
        check_labels(b, refs)
        check_readouts(ctx, refs, N, what=("equal azimuths", variant))
        assert ctx.front_scans() == 2


# ---- 7. small and awkward shapes ----
def lasers_params(L, cp=5, interval=None):
    p = u.default_params().wide_roi()
    p.channels = L
    p.curbPoints = cp
    if interval is not None:
        p.interval = interval
    return p


def with_holes(model, firings, seed, empty=()):
    """A sensor model's sweep whose missing returns come in every encoding, some lasers without any return at all."""
    L = SM.lasers(model)
    c = SM.sweep(model, firings=firings, world=0, seed=seed, drop=0.1, holes=SM.HOLES)
    for a in c:
        for l in empty:
            a.reshape(-1, L)[:, l] = 0.0
    return c


def shape_cases():
    return {
        "64x96_ragged": (lambda: [u.synth_cloud(64, 96, 1, 7), u.synth_cloud(64, 256, 3, 8), with_holes("ideal64", 160, 3, empty=(5, 40))],
                         lambda: O.cfg_params("cfg2"), 2, 0),
        "16x4096": (lambda: [u.synth_cloud(16, 4096, 1, 5), with_holes("ideal16", 4096, 4, empty=(3,))], lambda: lasers_params(16), 2, 0),
        "32x320": (lambda: [u.synth_cloud(32, 320, 3, 6), with_holes("ideal32", 320, 5)], lambda: lasers_params(32), 2, 0),
        "64_cp3": (lambda: [u.synth_cloud(64, 96, 1, 7), u.synth_cloud(64, 256, 3, 8)], lambda: lasers_params(64, 3), 3, 0),
        "64_cp7": (lambda: [u.synth_cloud(64, 96, 1, 7), u.synth_cloud(64, 256, 3, 8)], lambda: lasers_params(64, 7), 3, 0),
        "128x64": (lambda: [u.synth_cloud(128, 64, 1, 5), u.synth_cloud(128, 64, 3, 6)], lambda: lasers_params(128, interval=0.05), 2, 1),
    }


@pytest.mark.parametrize("name", list(shape_cases()))
def test_small_and_awkward_shapes(name):
    make, params, mode, l128 = shape_cases()[name]
    scans, p = make(), params()
    refs = [ref((name, k), c, p) for k, c in enumerate(scans)]
    assert all(r[1]["status"] == 0 and r[1]["n_road"] > 0 for r in refs), [r[1] for r in refs]
    if name == "16x4096":
        assert max(np.bincount(refs[0][2]["ring"][refs[0][2]["ring"] >= 0])) > 2048      # the sort in global memory
    b = Soa(scans)
    stride = max(b.lens)
    with u.Context(stride, len(scans), params=p) as ctx:
        ctx.set_front_lasers128(l128)
        ctx.set_front_mode(mode)
        ctx.set_front_outputs(1)
        b.classify(ctx)
        nf = ctx.front_scans()
        assert nf == len(scans)
        check_labels(b, refs)
        check_readouts(ctx, refs, stride, what=name)
        assert ctx.front_scans() == len(scans)


# ---- 7b. rings longer than 2048 points WITH bit-equal azimuths: the sort in global memory, then the literal pass on that array ----
@pytest.mark.parametrize("variant", ["repeated", "nudged"])
def test_long_rings_with_equal_azimuths(variant):
    """16 x 2176 (17 tiles: the smallest sweep whose rings pass 2048 points), every 8th firing a copy of the one before.  The general
    kernels (front mode 0) and the fused read-outs (front mode 2, urf_set_front_outputs) against oracle B, every list and marker point."""
    p = lasers_params(16)
    key, cloud = ("16x2176", 1, "repeated8"), repeated_firings(u.synth_cloud(16, 2176, 1, 5), 8, 16)
    if variant == "nudged":
        key, cloud = ("16x2176", 1, "nudged8"), nudged(u.synth_cloud(16, 2176, 1, 5), 8, ref(key, cloud, p)[2], 16)
    r = ref(key, cloud, p)
    n = len(cloud[0])
    assert n == 16 * 2176 and r[1]["status"] == 0 and r[1]["n_rings"] == 16
    lens = np.bincount(r[2]["ring"][r[2]["ring"] >= 0])
    assert len(lens) == 16 and min(lens) == max(lens) == 2176                      # every ring: sorted in global memory
    assert equal_azimuth_pairs(r[2]) > 1000, equal_azimuth_pairs(r[2])
    if variant == "repeated":
        assert equal_azimuth_pairs(r[2]) == 4336
        assert (len(r[2]["road_order"]), len(r[2]["curb_order"]), len(r[2]["marker_pts"])) == (8164, 220, 260)
    else:
        assert (len(r[2]["road_order"]), len(r[2]["marker_pts"])) == (7527, 185)
        assert order_decides(cloud, r[2]) >= 4 and r[1]["n_road"] > 5000
    b = Soa([cloud])
    with u.Context(n, 1, params=p) as ctx:                                         # arm 1: the general kernels
        ctx.set_front_mode(0)
        b.classify(ctx)
        assert ctx.front_scans() == 0
        check_labels(b, [r])
        check_readouts(ctx, [r], n, what=("long rings, general", variant))
    with u.Context(n, 1, params=p) as ctx:                                         # arm 2: the fused call's read-outs
        ctx.set_front_mode(2)
        ctx.set_front_outputs(1)
        b.classify(ctx)
        assert ctx.front_scans() == 1
        check_labels(b, [r])
        check_readouts(ctx, [r], n, what=("long rings, fused", variant))
        assert ctx.front_scans() == 1


# ---- 8. errors ----
def test_errors():
    with u.Context(64 * 96, 1) as ctx:
        assert ctx._lib.urf_set_front_outputs(ctx._h, 2) == -1          # URF_ERR_INVALID_ARG
        assert ctx._lib.urf_set_front_outputs(ctx._h, -1) == -1
        assert ctx._lib.urf_set_front_outputs(None, 1) == -1
        for on in (0, 1):
            ctx.set_front_outputs(on)
            for call in (lambda: ctx.ordered_indices(64 * 96), lambda: ctx.marker_points()):   # no call yet
                with pytest.raises(u.UrfError) as e:
                    call()
                assert e.value.code == -1
