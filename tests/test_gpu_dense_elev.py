"""urf_classify_batch_soa_dense_elev / urf_classify_batch_pc2_dense_elev: dense sweeps WITHOUT a laser id, the ids derived on the device
from the points' elevation and the table of urf_set_dense_elevations.  Every label and summary against oracle B run on the dense points,
bit for bit, and against the bytes of the `ring`-id dense call; the derived ids against the numpy model (tests/dense_ids_model.py), byte
for byte; tile and alignment edges; any table whatever gives the same labels; a history on one context (neither slot map leaks into the
other); the read-outs after such a call; the error codes; urf::BatchDetector.

Scans, oracle results and helpers are those of tests/test_gpu_dense.py (computed once per session); the contexts are this module's own,
one per laser count, in the library with the test hooks (urf_test_dense_ids)."""
import struct
import subprocess

import numpy as np
import pytest

import dense_ids_model as I
import dense_model as D
import sensor_models as SM
import urban_road_filter_amd as u
from hipmem import DevBuf
from test_gpu_dense import MAX_BATCH, Batch, code, dense_scan, equal_to_b, model_aligned, params, ref
from test_gpu_dense_outputs import batch_lists, clouds_ref_order
from test_gpu_detector import build_demo

pytestmark = pytest.mark.gpu
_CTX = {}

# model -> (firings, sweep keywords, seeds): test_gpu_dense.py's scans where it has the model
SCANS = {
    "ideal16": (304, {}, (1, 2, 3)),
    "ideal32": (136, {}, (1, 2, 3)),
    "ideal64": (256, {}, (1, 2, 3)),
    "ideal128": (128, {}, (1, 2, 3)),
    "vlp16": (304, {}, (1, 2, 3)),
    "hdl32e": (136, dict(drop=0.01), (1, 2, 3)),
    "vlp32c": (136, dict(noise=True, drop=0.05), (1, 2)),
    "hdl64e": (256, {}, (1, 2, 3)),
}


@pytest.fixture(scope="module", autouse=True)
def _contexts():
    yield
    for c in _CTX.values():
        c.close()
    _CTX.clear()


def context(L, mode=2, outputs=0, dense_outputs=0, multi=0):
    """(sizes: tests/test_gpu_dense.py's context())  Every switch this module touches is set, whatever the test before left."""
    if L not in _CTX:
        _CTX[L] = u.Context(L * {16: 320, 32: 320, 64: 2048, 128: 300}[L], MAX_BATCH, hooks=True)
        if L == 128:
            _CTX[L].set_front_lasers128(1)
    ctx = _CTX[L]
    ctx.set_front_multi_sector(multi)
    ctx.set_front_mode(mode)
    ctx.set_front_outputs(outputs)
    ctx.set_dense_outputs(dense_outputs)
    ctx.set_dense_slots(None)
    return ctx


def elev(model):
    return np.asarray(SM.MODELS[model]["elev"], np.float32)


def scans_of(model):
    F, kw, seeds = SCANS[model]
    return [dense_scan(model, s, firings=F, **kw) for s in seeds], F + 3


def records(b, step, ox, oy, oz):
    """PointCloud2 bytes without a laser id: x / y / z at ox / oy / oz of every `step` bytes, every other byte 0xa5."""
    rec = np.full((b.n, step), 0xA5, np.uint8)
    for o, a in zip((ox, oy, oz), (b.X, b.Y, b.Z)):
        rec[:, o:o + 4] = a.view(np.uint8).reshape(-1, 4)
    return np.ascontiguousarray(rec.reshape(-1))


def soa_elev(b, ctx, W, max_len=None):
    b.dl.fill(0xEE)
    ctx.classify_batch_soa_dense_elev(b.dx, b.dy, b.dz, b.do, max(b.lens) if max_len is None else max_len, b.S, W, b.dl, b.di)
    return b.result(ctx) + (ctx.front_scans(), ctx.dense_scans())


def pc2_elev(b, ctx, W, layout=(32, 0, 4, 8), max_len=None):
    b.dl.fill(0xEE)
    b.dd = DevBuf.from_numpy(records(b, *layout))
    ctx.classify_batch_pc2_dense_elev(b.dd, b.do, b.n, max(b.lens) if max_len is None else max_len, b.S, *layout, W, b.dl, b.di)
    return b.result(ctx) + (ctx.front_scans(), ctx.dense_scans())


def same_bytes(got, want, what):
    assert all(np.array_equal(x, y) for x, y in zip(got[0], want[0])), what + ": labels"
    assert np.array_equal(got[1], want[1]), what + ": infos"


# ---- 1. parity, 2. the ids ----
@pytest.mark.parametrize("roi", ["wide", "default"])
@pytest.mark.parametrize("model", sorted(SCANS))
def test_labels_infos_ids_and_the_fused_path(model, roi):
    L = SM.lasers(model)
    p = params(model, roi)
    scans, W = scans_of(model)
    clouds, slots = [s[0] for s in scans], [s[1] for s in scans]
    # the input is far from every midpoint: model and kernel cannot disagree about a compare
    assert min(I.midpoint_margin_deg(elev(model), c) for c in clouds) > 1e-3
    ids = [I.ids(elev(model), c) for c in clouds]
    want_aligned = model_aligned(ids, L, W)
    assert want_aligned == len(scans)
    if roi == "wide":   # (no comparison passes on empty results)
        assert any(ref(s, p, roi)[1]["n_road"] > 0 and ref(s, p, roi)[1]["n_curb"] > 0 for s in scans)
    ctx = context(L, multi=0 if model.startswith("ideal") else 1)
    ctx.set_params(p)
    ctx.set_dense_elevations(elev(model))
    b = Batch(clouds, slots)
    for _ in range(2):   # (the second call: a context's first call with new parameters may hand a sweep back, tests/test_gpu_dense.py)
        ring = b.soa_dense(ctx, W, np.uint8)
    equal_to_b(ring, scans, p, roi, "%s %s ring ids" % (model, roi))
    assert ring[3] == len(scans)
    if model.startswith("ideal"):
        assert ring[2] == len(scans)
    for what, run in (("soa", lambda: soa_elev(b, ctx, W)), ("pc2 32", lambda: pc2_elev(b, ctx, W)),
                      ("pc2 15", lambda: pc2_elev(b, ctx, W, (15, 2, 6, 11)))):
        got = run()
        got = run()
        what = "%s %s %s" % (model, roi, what)
        equal_to_b(got, scans, p, roi, what)
        same_bytes(got, ring, what)
        assert got[3] == want_aligned, (what, got[3])
        assert got[2] == ring[2], (what, got[2], ring[2])
        assert np.array_equal(ctx.dense_ids(b.n), np.concatenate(ids).astype(np.uint8)), what + ": ids"
    assert np.array_equal(np.concatenate(ids), np.concatenate(slots))   # (and they are the true slots: the CPU test's claim, on these inputs)


# ---- 3. tile and alignment edges ----
def test_tile_and_alignment_edges_in_one_batch():
    L, model, roi, W, max_len = 16, "ideal16", "wide", 290, 3000
    p = params(model, roi)
    a, c = dense_scan(model, 9, firings=280), dense_scan(model, 10, firings=280)
    cut = lambda s, n, tag: (tuple(v[:n].copy() for v in s[0]), s[1][:n].copy(), s[2], s[3] + (tag,))  # noqa: E731
    assert len(c[1]) > max_len and W * L >= max_len
    sent = [cut(a, 0, "cut0"), cut(a, 1, "cut1"), cut(c, 2047, "cut2047"), cut(a, 2048, "cut2048"), cut(c, 2049, "cut2049"), c]
    seen = sent[:5] + [cut(c, max_len, "cut3000")]   # the last scan is cut at max_len
    b = Batch([s[0] for s in sent], [s[1] for s in sent])
    assert [int(o) % 4 for o in b.offs[:6]] == [0, 0, 1, 0, 0, 1]   # scans that start off a multiple of 4
    ids = [I.ids(elev(model), s[0]) for s in seen]
    assert min(I.midpoint_margin_deg(elev(model), s[0]) for s in seen[1:]) > 1e-3
    want_aligned = model_aligned(ids, L, W)
    assert want_aligned == 6
    assert ref(seen[3], p, roi)[1]["n_road"] > 0 and ref(seen[5], p, roi)[1]["n_road"] > 0
    ctx = context(L)
    ctx.set_params(p)
    ctx.set_dense_elevations(elev(model))
    full_ids = I.ids(elev(model), (b.X, b.Y, b.Z)).astype(np.uint8)
    runs = [("soa", lambda: soa_elev(b, ctx, W, max_len)), ("pc2 18", lambda: pc2_elev(b, ctx, W, (18, 1, 5, 9), max_len)),
            ("pc2 22", lambda: pc2_elev(b, ctx, W, (22, 3, 9, 15), max_len)), ("pc2 32", lambda: pc2_elev(b, ctx, W, (32, 0, 4, 8), max_len))]
    for what, run in runs:
        labels, infos, _, aligned = run()
        labels = [lab[:len(s[1])] for lab, s in zip(labels, seen)]   # (behind the cut: not the call's)
        equal_to_b((labels, infos), seen, p, roi, "edges " + what)
        assert aligned == want_aligned, (what, aligned)
        got = ctx.dense_ids(b.n)
        for k, s in enumerate(seen):   # the ids of the points the call saw
            lo = int(b.offs[k])
            assert np.array_equal(got[lo:lo + len(s[1])], full_ids[lo:lo + len(s[1])]), (what, k)


# ---- 4. any table, same labels ----
def odd_points(scan, tag):
    """The scan with NaN, Inf, (0, 0, 0), on-axis and out-of-fan points written over a few of its points."""
    x, y, z = (v.copy() for v in scan[0])
    n = len(x)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    odd = [(nan, 1.0, -1.0), (2.0, 3.0, nan), (inf, 0.0, 0.0), (1.0, -inf, -1.0), (0.0, 0.0, 0.0), (0.0, 0.0, 2.0), (0.0, 0.0, -1.7),
           (3.0, 0.0, 100.0), (0.4, 0.1, -1.8), (6.0, 1.0, 0.5)]
    for k, pt in enumerate(odd):
        i = (k + 1) * n // (len(odd) + 2)
        x[i], y[i], z[i] = pt
    return ((x, y, z), scan[1], scan[2], scan[3] + (tag,))


@pytest.mark.parametrize("table", ["reversed", "shuffled", "all_equal", "true"])
def test_any_table_gives_the_same_labels(table):
    L, model, roi, W = 16, "ideal16", "wide", 307
    p = params(model, roi)
    scans = [odd_points(dense_scan(model, 1), "odd"), dense_scan(model, 2), odd_points(dense_scan(model, 3), "odd")]
    e = elev(model)
    e = {"reversed": e[::-1].copy(), "shuffled": e[np.random.default_rng(5).permutation(L)], "all_equal": np.full(L, -7.0, np.float32),
         "true": e}[table]
    ids = [I.ids(e, s[0]) for s in scans]
    want_aligned = model_aligned(ids, L, W)
    if table == "true":
        assert want_aligned >= 1     # (the scan nobody wrote over)
    assert all(I.monotone_products(e, s[0]) for s in scans)
    ctx = context(L)
    ctx.set_params(p)
    ctx.set_dense_elevations(e)
    b = Batch([s[0] for s in scans], [s[1] for s in scans])
    for what, run in (("soa", lambda: soa_elev(b, ctx, W)), ("pc2", lambda: pc2_elev(b, ctx, W, (22, 3, 9, 15)))):
        got = run()
        equal_to_b(got, scans, p, roi, "%s table, %s" % (table, what))
        assert np.array_equal(ctx.dense_ids(b.n), np.concatenate(ids).astype(np.uint8)), (table, what)
        assert got[3] == want_aligned, (table, what, got[3], want_aligned)


# ---- 5. a history on one context ----
def test_history_neither_slot_map_leaks_into_the_other():
    model, roi, L = "vlp16", "wide", 16
    p = params(model, roi)
    scans, W = scans_of(model)
    clouds, slots = [s[0] for s in scans], [s[1] for s in scans]
    rank = np.argsort(np.argsort(SM.MODELS[model]["elev"])).astype(np.int64)   # the driver's ring: by elevation
    slot_of_rank = np.argsort(rank).astype(np.uint8)
    assert (slot_of_rank[rank] == np.arange(L)).all() and (rank != np.arange(L)).any()
    ranks = [rank[s] for s in slots]
    # either map applied to the other call's ids would show in the aligned count
    assert model_aligned(ranks, L, W, slot_of_rank) == len(scans) and model_aligned(ranks, L, W) == 0
    assert model_aligned(slots, L, W, slot_of_rank) == 0
    ctx = context(L, multi=1)
    ctx.set_params(p)
    ctx.set_dense_elevations(elev(model))
    ctx.set_dense_slots(slot_of_rank)
    br, bs = Batch(clouds, ranks), Batch(clouds, slots)
    for _ in range(2):
        first = br.pc2_dense(ctx, W)
    equal_to_b(first, scans, p, roi, "ring ids through the map")
    assert first[3] == len(scans)
    mid = soa_elev(bs, ctx, W)
    equal_to_b(mid, scans, p, roi, "elevation call behind a mapped call")
    assert mid[2:] == first[2:], (mid[2:], first[2:])
    assert np.array_equal(ctx.dense_ids(bs.n), np.concatenate(slots).astype(np.uint8))
    again = br.soa_dense(ctx, W, np.uint16)
    equal_to_b(again, scans, p, roi, "ring ids again")
    assert again[2:] == first[2:], (again[2:], first[2:])
    equal_to_b(pc2_elev(bs, ctx, W), scans, p, roi, "elevation call, pc2")
    equal_to_b(bs.soa_ragged(ctx), scans, p, roi, "ragged")
    assert ctx.dense_scans() == len(scans)   # (still the last dense call's)
    ctx.set_dense_slots(None)


# ---- 6. the read-outs ----
@pytest.mark.parametrize("outputs", [0, 1])
@pytest.mark.parametrize("kind", ["soa", "pc2"])
def test_readouts_after_an_elevation_call(kind, outputs):
    model, roi, L = "ideal64", "wide", 64
    p = params(model, roi)
    scans, W = scans_of(model)
    ctx = context(L, 2, outputs, dense_outputs=1)
    ctx.set_params(p)
    ctx.set_dense_elevations(elev(model))
    b = Batch([s[0] for s in scans], [s[1] for s in scans])
    stride = max(b.lens)
    intensity = (np.arange(b.n, dtype=np.float32) * np.float32(0.25)).astype(np.float32)
    if kind == "soa":
        d_src = DevBuf.from_numpy(intensity)
        b.soa_ragged(ctx)
    else:
        rec = records(b, 32, 0, 4, 8).reshape(b.n, 32)
        rec[:, 16:20] = intensity.view(np.uint8).reshape(-1, 4)
        d_src = DevBuf.from_numpy(np.ascontiguousarray(rec.reshape(-1)))
        ctx.classify_batch_pc2_ragged(d_src, b.do, b.n, stride, b.S, 32, 0, 4, 8, b.dl, b.di)
    want_lists = batch_lists(ctx, b.S, stride)
    want_clouds = clouds_ref_order(ctx, kind, b, d_src, 32, 16)
    assert all(len(row[0]) and len(row[1]) for row in want_lists)   # road and curb entries in every scan
    ctx.set_front_mode(2)   # (a read-out with urf_set_front_outputs off may have left the context with the general kernels)
    for _ in range(2):
        if kind == "soa":
            got = soa_elev(b, ctx, W)
        else:
            b.dl.fill(0xEE)
            ctx.classify_batch_pc2_dense_elev(d_src, b.do, b.n, stride, b.S, 32, 0, 4, 8, W, b.dl, b.di)
            got = b.result(ctx) + (ctx.front_scans(), ctx.dense_scans())
    equal_to_b(got, scans, p, roi, "read-outs")
    assert got[2] == b.S and got[3] == b.S
    have_lists = batch_lists(ctx, b.S, stride)
    for s in range(b.S):
        for k in range(3):
            assert np.array_equal(have_lists[s][k], want_lists[s][k]), (s, k)
    have_clouds = clouds_ref_order(ctx, kind, b, d_src, 32, 16)
    for name, x, y in zip(("counts", "offsets", "records"), want_clouds, have_clouds):
        assert np.array_equal(x, y), name
    assert code(lambda: ctx.read_stage(u.STAGE_ANGLE_TABLE, W * L, 0)) == -1 and b"dense" in ctx._lib.urf_last_error(ctx._h)
    assert ctx.front_scans() == (b.S if outputs else 0)   # (off: the documented rerun through the general kernels)
    ctx.set_dense_outputs(0)


# ---- 7. errors ----
def test_error_codes():
    L, W = 16, 304
    model = "ideal16"
    sc = dense_scan(model, 1)
    p = params(model, "wide")
    b = Batch([sc[0]], [sc[1]])
    rec = DevBuf.from_numpy(records(b, 32, 0, 4, 8))
    n = b.lens[0]
    with u.Context(L * 320, MAX_BATCH, params=p, hooks=True) as ctx:   # a context nobody has given a table
        ctx.set_front_mode(2)
        soa = lambda **k: code(lambda: ctx.classify_batch_soa_dense_elev(k.get("x", b.dx), k.get("y", b.dy), k.get("z", b.dz), k.get("offs", b.do),  # noqa: E731
                                                                        k.get("max_len", n), k.get("S", 1), k.get("W", W), k.get("labels", b.dl), b.di))
        pc2 = lambda **k: code(lambda: ctx.classify_batch_pc2_dense_elev(k.get("data", rec), k.get("offs", b.do), k.get("total", n),  # noqa: E731
                                                                        k.get("max_len", n), k.get("S", 1), k.get("step", 32), 0, 4, k.get("oz", 8),
                                                                        k.get("W", W), k.get("labels", b.dl), b.di))
        last = lambda: ctx._lib.urf_last_error(ctx._h)  # noqa: E731
        assert soa() == -1 and b"urf_set_dense_elevations" in last()      # no table
        assert pc2() == -1 and b"urf_set_dense_elevations" in last()
        assert code(lambda: ctx.dense_ids(1)) == -1                       # (and no id buffer)
        ctx.set_dense_elevations(elev("ideal32"))                         # n != channels
        assert soa() == -1 and b"channels" in last() and pc2() == -1
        ctx.set_dense_elevations(elev(model))
        assert soa() == 0 and pc2() == 0
        want = I.ids(elev(model), sc[0]).astype(np.uint8)
        assert np.array_equal(ctx.dense_ids(n), want)
        # a refused table leaves the one before
        for bad in (np.nan, 90.0, -90.0, np.inf, 120.0):
            e = elev(model).copy()
            e[5] = bad
            assert code(lambda: ctx.set_dense_elevations(e)) == -1, bad
        assert code(lambda: ctx.set_dense_elevations(np.zeros(129, np.float32))) == -1
        assert ctx._lib.urf_set_dense_elevations(ctx._h, None, 3) == -1
        assert ctx._lib.urf_set_dense_elevations(ctx._h, elev(model).ctypes.data, 0) == -1
        got = soa_elev(b, ctx, W)
        equal_to_b(got, [sc], p, "wide", "after the refused tables")
        assert got[3] == 1 and np.array_equal(ctx.dense_ids(n), want)
        ctx.set_dense_elevations(np.zeros(128, np.float32))               # 128 values are a table (of the wrong size here)
        assert soa() == -1
        ctx.set_dense_elevations(elev(model))
        # urf_set_params changes channels under the table
        p32 = params("ideal32", "wide")
        ctx.set_params(p32)
        assert soa(W=100) == -1 and b"channels" in last() and pc2(W=100) == -1
        ctx.set_params(p)
        assert soa() == 0
        # the dense calls' own rules
        for f in (soa, pc2):
            assert f(W=321) == -4                      # W * L > max_points
            assert f(W=(n - 1) // L) == -4             # max_len > W * L
            assert f(W=0) == -4 and f(W=0, max_len=0) == -1
            assert f(S=MAX_BATCH + 1) == -4
            assert f(offs=None) == -1 and f(labels=None) == -1
            assert f(S=0) == 0                         # a no-op
        assert soa(x=None) == -1 and soa(y=None) == -1 and soa(z=None) == -1
        assert pc2(data=None) == -1 and pc2(step=3) == -1 and pc2(oz=29) == -1 and pc2(oz=28) == 0
        assert pc2(total=L * 320 * MAX_BATCH + 1) == -4
        # the `ring`-id calls keep their refusal
        assert code(lambda: ctx.classify_batch_soa_dense(b.dx, b.dy, b.dz, None, 1, b.do, n, 1, W, b.dl, b.di)) == -1
        ctx.set_dense_elevations(None)                                    # cleared
        assert soa() == -1 and b"urf_set_dense_elevations" in last()
        ctx.set_dense_elevations(elev(model))
        got = soa_elev(b, ctx, W)                                         # and the context still works
        equal_to_b(got, [sc], p, "wide", "after the errors")
        assert got[3] == 1


# ---- 8. urf::BatchDetector ----
def test_batch_detector_takes_messages_without_a_ring_field(tmp_path):
    exe = build_demo(tmp_path, "batch_dense_elev_demo")
    model = "ideal64"
    scans, W = scans_of(model)
    path = tmp_path / "clouds.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<III", len(scans), 64, W))
        f.write(elev(model).tobytes())
        for k, (cloud, slot, _, _) in enumerate(scans):
            f.write(struct.pack("<I", len(slot)))
            for a in cloud + (np.arange(len(slot), dtype=np.float32) * np.float32(0.25) + np.float32(k),):
                f.write(np.ascontiguousarray(a, np.float32).tobytes())
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    lines = r.stdout.splitlines()
    row = lambda tag: [ln.split() for ln in lines if ln.startswith(tag + " ")]  # noqa: E731
    with_table, plain, cleared = row("elev"), row("plain"), row("cleared")
    assert len(with_table) == 1 and len(plain) == 1 and len(cleared) == 1 and lines[-1] == "done", r.stdout
    k = str(len(scans))
    w = dict(zip(with_table[0][1::2], with_table[0][2::2]))
    assert w == {"messages": k, "published": k, "points": w["points"], "equal": k, "aligned": k} and int(w["points"]) > 3000, r.stdout
    for other in (plain, cleared):
        w = dict(zip(other[0][1::2], other[0][2::2]))
        assert w == {"messages": k, "equal": k, "aligned": "0"}, r.stdout
