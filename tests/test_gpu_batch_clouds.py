"""The published clouds of a batch on the device (urf_clouds_batch_soa / urf_clouds_batch_pc2) and ragged PointCloud2 batches
(urf_classify_batch_pc2_ragged), against oracle B: labels and summaries, every count and offset, every byte of every record
(x / y / z / intensity bit for bit, w = 1.0, zero padding), input order and the reference's published order; the fused front
end; the error codes; and urf::BatchDetector against urf::Detector byte for byte (tests/cpp/batch_detector_demo.cpp)."""
import struct
import subprocess

import numpy as np
import pytest

import oracles as O
import urban_road_filter_amd as u
from hipmem import DevBuf
from test_gpu_detector import build_demo

pytestmark = pytest.mark.gpu
N = 64 * 2048
ONE = 0x3F800000
# record layouts: (point_step, off_x, off_y, off_z, off_intensity)
XYZI = (32, 0, 4, 8, 16)           # pcl::PointXYZI
PERMUTED = (32, 12, 20, 4, 0)      # intensity z t x ring y (Ouster-like field table, extra fields)
STEP23 = (23, 3, 11, 17, -1)       # unaligned records without intensity


def intensity_of(n, seed):
    v = (np.arange(n) % 251).astype(np.float32) * 0.5 + seed
    b = v.view(np.uint32)
    if n:
        b[0] = 0x80000000       # -0.0
    if n > 7:
        b[7] = 0x7FC01234       # a NaN with a payload
    return v


def without_dropouts(cloud):
    """A sensor-like sweep as a driver that drops non-returns publishes it (variable length)."""
    keep = ~((cloud[0] == 0) & (cloud[1] == 0) & (cloud[2] == 0))
    return tuple(np.ascontiguousarray(a[keep]) for a in cloud)


def records(x, y, z, inten, layout):
    step, ox, oy, oz, oi = layout
    n = len(x)
    buf = np.zeros((n, step), np.uint8)
    if layout == XYZI:
        buf[:, 12:16] = np.full(n, 1.0, np.float32).view(np.uint8).reshape(n, 4)
    if layout == PERMUTED:
        buf[:, 8:12] = (np.arange(n, dtype=np.uint32) * 100).view(np.uint8).reshape(n, 4)    # t
        buf[:, 16:18] = (np.arange(n) % 64).astype(np.uint16).view(np.uint8).reshape(n, 2)  # ring
    if layout == STEP23:
        buf[:] = 0xA5
    for a, o in ((x, ox), (y, oy), (z, oz), (inten, oi)):
        if o >= 0:
            buf[:, o:o + 4] = np.ascontiguousarray(a, np.float32).view(np.uint8).reshape(n, 4)
    return buf.reshape(-1)


def expected(scans, intens, p, order):
    """-> counts [S, 4], concatenated records uint32 [k, 8] from oracle B's labels (and its published order)"""
    counts, recs = [], []
    for (x, y, z), inten in zip(scans, intens):
        lb, ib, st = O.run_b(x, y, z, p, debug=True)
        n = len(x)
        r = np.zeros((n, 8), np.uint32)
        for k, a in enumerate((x, y, z)):
            r[:, k] = np.ascontiguousarray(a, np.float32).view(np.uint32)
        r[:, 3] = ONE
        if inten is not None:
            r[:, 4] = np.ascontiguousarray(inten, np.float32).view(np.uint32)
        if ib["status"] != 0:
            counts.append([0, 0, 0, 0])
            continue
        if order == u.ORDER_REFERENCE:
            idx = [st["road_order"], st["curb_order"], np.nonzero(lb & 4)[0], st["ring10_order"]]
        else:
            idx = [np.nonzero((lb & 3) == 1)[0], np.nonzero((lb & 3) == 2)[0], np.nonzero(lb & 4)[0], np.nonzero(lb & 16)[0]]
        counts.append([len(i) for i in idx])
        recs += [r[i] for i in idx]
    counts = np.array(counts, np.uint32)
    return counts, (np.concatenate(recs) if recs else np.zeros((0, 8), np.uint32))


class Batch:
    """Scans on the device as SoA arrays and as PointCloud2 records (fixed length or ragged)."""

    def __init__(self, scans, layout=XYZI, seed=1):
        self.scans, self.layout = scans, layout
        self.lens = [len(s[0]) for s in scans]
        self.offs = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.uint32)
        self.total = int(self.offs[-1])
        self.intens = [intensity_of(n, seed + i) for i, n in enumerate(self.lens)]
        cat = lambda k: np.concatenate([s[k] for s in scans]).astype(np.float32)   # noqa: E731
        self.X, self.Y, self.Z = cat(0), cat(1), cat(2)
        self.I = np.concatenate(self.intens).astype(np.float32)
        self.dx, self.dy, self.dz, self.di = (DevBuf.from_numpy(a) for a in (self.X, self.Y, self.Z, self.I))
        self.dd = DevBuf.from_numpy(records(self.X, self.Y, self.Z, self.I, layout))
        self.do = DevBuf.from_numpy(self.offs)
        self.dl = DevBuf(max(self.total, 1))
        self.dinfo = DevBuf(32 * len(scans))

    def classify(self, ctx, kind):
        S = len(self.scans)
        self.dl.fill(0xEE)
        step, ox, oy, oz, _ = self.layout
        if kind == "soa":
            ctx.classify_batch_soa(self.dx, self.dy, self.dz, self.lens[0], S, self.dl, self.dinfo)
        elif kind == "soa_ragged":
            ctx.classify_batch_soa_ragged(self.dx, self.dy, self.dz, self.do, max(self.lens), S, self.dl, self.dinfo)
        elif kind == "pc2":
            ctx.classify_batch_pc2(self.dd, self.lens[0], S, step, ox, oy, oz, self.dl, self.dinfo)
        else:
            ctx.classify_batch_pc2_ragged(self.dd, self.do, self.total, max(self.lens), S, step, ox, oy, oz, self.dl, self.dinfo)
        ctx.synchronize()
        return self.labels(), self.dinfo.to_numpy(np.uint32).reshape(S, 8)

    def labels(self):
        L = self.dl.to_numpy(np.uint8)
        return [L[a:b] for a, b in zip(self.offs[:-1], self.offs[1:])]

    def clouds(self, ctx, kind, order, records=True, capacity=None, intensity=True):
        S = len(self.scans)
        cap = 3 * S * max(self.lens) if capacity is None else capacity
        drec = DevBuf(32 * max(cap, 1)) if records else None
        dcnt, doff = DevBuf(16 * S), DevBuf(32 * S)
        dcnt.fill(0xEE)
        doff.fill(0xEE)
        if kind.startswith("soa"):
            ctx.clouds_batch_soa(self.di if intensity else None, order, drec, cap, dcnt, doff)
        else:
            step, ox, oy, oz, oi = self.layout
            ctx.clouds_batch_pc2(self.dd, step, ox, oy, oz, oi if intensity else -1, order, drec, cap, dcnt, doff)
        ctx.synchronize()
        cnt = dcnt.to_numpy(np.uint32).reshape(S, 4)
        off = doff.to_numpy(np.uint64).reshape(S, 4)
        n = int(cnt.sum())
        rec = drec.to_numpy(np.uint32, 8 * n).reshape(n, 8) if records else None
        return cnt, off, rec

    def check_clouds(self, ctx, kind, order, p, intensity=True):
        cnt, off, rec = self.clouds(ctx, kind, order, intensity=intensity)
        carry = intensity and (kind.startswith("soa") or self.layout[4] >= 0)
        want_cnt, want_rec = expected(self.scans, self.intens if carry else [None] * len(self.scans), p, order)
        assert np.array_equal(cnt, want_cnt), (kind, order)
        flat = cnt.reshape(-1).astype(np.uint64)
        assert np.array_equal(off.reshape(-1), np.concatenate([[0], np.cumsum(flat)[:-1]]).astype(np.uint64)), (kind, order)
        assert rec.shape == want_rec.shape and np.array_equal(rec, want_rec), (kind, order)   # every byte, w and pad included
        return cnt


def check_labels(labels, infos, scans, p):
    for s, (x, y, z) in enumerate(scans):
        lb, ib, _ = O.run_b(x, y, z, p)
        assert np.array_equal(labels[s], lb), s
        assert infos[s][0] == ib["status"] and list(infos[s][1:7]) == [ib[k] for k in ("n_roi", "n_rings", "n_ring_pts", "n_road",
                                                                                          "n_curb", "n_ring10")], s


def ragged_scans():
    tiny = tuple(a[:29].copy() for a in O.cfg_cloud("cfg2", 12))
    empty = tuple(np.zeros(0, np.float32) for _ in range(3))
    part = tuple(a[:100001].copy() for a in O.cfg_cloud("narrow", 14))
    return [O.cfg_cloud("cfg2", 11), without_dropouts(O.cfg_cloud("sensor", 13)), empty, part,
            without_dropouts(O.cfg_cloud("sensor", 15)), tiny]


@pytest.mark.parametrize("layout", [XYZI, PERMUTED, STEP23], ids=["pointxyzi", "permuted", "step23"])
def test_ragged_pointcloud2_batch(layout):
    """Messages of different lengths (drop-outs removed, one empty, one below 30 ROI points) in one batch: labels and summaries
    equal oracle B and urf_classify_batch_soa_ragged on the same points; then the clouds of that call in both orders."""
    p = O.cfg_params("cfg2")
    scans = ragged_scans()
    assert len(set(len(s[0]) for s in scans)) == len(scans)
    b = Batch(scans, layout)
    with u.Context(N, len(scans), params=p) as ctx:
        lp, ip = b.classify(ctx, "pc2_ragged")
        check_labels(lp, ip, scans, p)
        assert ip[2][0] == u.api.TOO_FEW_POINTS and ip[5][0] == u.api.TOO_FEW_POINTS
        for order in (u.ORDER_INPUT, u.ORDER_REFERENCE):
            cnt = b.check_clouds(ctx, "pc2_ragged", order, p)
            assert not cnt[2].any() and not cnt[5].any()   # four empty clouds: the empty message, the one below 30 ROI points
        if layout[4] >= 0:
            b.check_clouds(ctx, "pc2_ragged", u.ORDER_INPUT, p, intensity=False)   # off_intensity = -1: intensity 0
        ls, is_ = b.classify(ctx, "soa_ragged")
        assert all(np.array_equal(a, c) for a, c in zip(lp, ls)) and np.array_equal(ip, is_)
        for order in (u.ORDER_INPUT, u.ORDER_REFERENCE):
            b.check_clouds(ctx, "soa_ragged", order, p)
        b.check_clouds(ctx, "soa_ragged", u.ORDER_INPUT, p, intensity=False)      # d_intensity = NULL


def test_ragged_pointcloud2_batch_default_roi():
    p = O.cfg_params("default_roi")
    scans = [O.cfg_cloud("default_roi", 21), without_dropouts(O.cfg_cloud("sensor_default_roi", 22))]
    b = Batch(scans, PERMUTED)
    with u.Context(N, len(scans), params=p) as ctx:
        check_labels(*b.classify(ctx, "pc2_ragged"), scans, p)
        for order in (u.ORDER_INPUT, u.ORDER_REFERENCE):
            b.check_clouds(ctx, "pc2_ragged", order, p)


@pytest.mark.parametrize("kind", ["pc2", "soa"])
def test_clouds_of_fixed_length_batches(kind):
    p = O.cfg_params("cfg2")
    scans = [O.cfg_cloud("cfg2", 31), O.cfg_cloud("narrow", 32), O.cfg_cloud("sensor", 33)]
    few = tuple(a.copy() for a in O.cfg_cloud("cfg2", 34))
    few[0][29:] = 1.0e6   # all but 29 points far outside the region of interest
    scans.append(few)
    b = Batch(scans, STEP23 if kind == "pc2" else XYZI)
    with u.Context(N, len(scans), params=p) as ctx:
        ctx.set_front_mode(0)
        check_labels(*b.classify(ctx, kind), scans, p)
        for order in (u.ORDER_INPUT, u.ORDER_REFERENCE):
            cnt = b.check_clouds(ctx, kind, order, p)
            assert not cnt[3].any()


def test_clouds_after_the_fused_front_end():
    """A fused batch: input order reads only labels and inputs (the context stays fused); the reference order runs the batch once
    more through the general kernels (documented) and is still right.  The same for row-major sweeps."""
    p = O.cfg_params("cfg2")
    fir = [O.cfg_cloud("cfg2", 41), O.cfg_cloud("sensor", 42), O.cfg_cloud("narrow", 43)]
    rows = [tuple(np.ascontiguousarray(a.reshape(-1, 64).T.reshape(-1)) for a in c) for c in fir]
    for scans, calls in ((fir, 1), (rows, 2)):   # (a context's first call with row-major sweeps only sights the layout)
        b = Batch(scans, XYZI)
        with u.Context(N, len(scans), params=p) as ctx:
            ctx.set_front_mode(2)
            for kind in ("soa", "pc2"):
                for _ in range(calls):
                    labels, infos = b.classify(ctx, kind)
                assert ctx.front_scans() == len(scans), kind
                check_labels(labels, infos, scans, p)
                b.check_clouds(ctx, kind, u.ORDER_INPUT, p)
                assert ctx.front_scans() == len(scans), kind                      # still the fused call's
                assert all(np.array_equal(a, c) for a, c in zip(labels, b.labels()))
                b.check_clouds(ctx, kind, u.ORDER_REFERENCE, p)
                assert ctx.front_scans() == 0                                     # the rerun: the context keeps to the general kernels
                assert all(np.array_equal(a, c) for a, c in zip(labels, b.labels()))
                ctx.set_front_mode(2)                                             # (fused again for the next kind)


def test_error_codes():
    p = O.cfg_params("cfg2")
    scans = [O.cfg_cloud("cfg2", 51), without_dropouts(O.cfg_cloud("sensor", 52))]
    b = Batch(scans, XYZI)
    S = len(scans)
    cap = 3 * S * max(b.lens)
    with u.Context(N, S, params=p) as ctx:
        dcnt, doff, drec = DevBuf(16 * S), DevBuf(32 * S), DevBuf(32 * cap)

        def code(fn):
            with pytest.raises(u.UrfError) as e:
                fn()
            return e.value.code

        # no call yet
        assert code(lambda: ctx.clouds_batch_soa(None, 0, drec, cap, dcnt, doff)) == -1
        # n_total beyond the staging, max_len beyond max_points
        step, ox, oy, oz, oi = XYZI
        assert code(lambda: ctx.classify_batch_pc2_ragged(b.dd, b.do, N * S + 1, max(b.lens), S, step, ox, oy, oz, b.dl)) == -4
        assert code(lambda: ctx.classify_batch_pc2_ragged(b.dd, b.do, b.total, N + 1, S, step, ox, oy, oz, b.dl)) == -4
        assert code(lambda: ctx.classify_batch_pc2_ragged(b.dd, b.do, b.total, max(b.lens), S, 32, 30, 4, 8, b.dl)) == -1
        b.classify(ctx, "pc2_ragged")
        # counts only
        cnt_only = b.clouds(ctx, "pc2_ragged", u.ORDER_REFERENCE, records=False)
        cnt, off, _ = b.clouds(ctx, "pc2_ragged", u.ORDER_INPUT)
        assert np.array_equal(cnt_only[0], cnt) and np.array_equal(cnt_only[1], off)
        # too little room
        assert code(lambda: ctx.clouds_batch_pc2(b.dd, step, ox, oy, oz, oi, 0, drec, cap - 1, dcnt, doff)) == -4
        # wrong call kind, bad intensity offset, bad order
        assert code(lambda: ctx.clouds_batch_soa(b.di, 0, drec, cap, dcnt, doff)) == -1
        assert code(lambda: ctx.clouds_batch_pc2(b.dd, step, ox, oy, oz, 29, 0, drec, cap, dcnt, doff)) == -1
        assert code(lambda: ctx.clouds_batch_pc2(b.dd, step, ox, oy, oz, -2, 0, drec, cap, dcnt, doff)) == -1
        assert code(lambda: ctx.clouds_batch_pc2(b.dd, step, ox, oy, oz, oi, 2, drec, cap, dcnt, doff)) == -1
        b.classify(ctx, "soa_ragged")
        assert code(lambda: ctx.clouds_batch_pc2(b.dd, step, ox, oy, oz, oi, 0, drec, cap, dcnt, doff)) == -1
        ctx.clouds_batch_soa(b.di, 0, drec, cap, dcnt, doff)
        # a sweep of the callback path as the last call
        x, y, z = scans[0]
        ctx.classify_xyz(x, y, z)
        assert code(lambda: ctx.clouds_batch_soa(b.di, 0, drec, cap, dcnt, doff)) == -1
        assert code(lambda: ctx.clouds_batch_pc2(b.dd, step, ox, oy, oz, oi, 0, drec, cap, dcnt, doff)) == -1


def test_batch_detector_equals_detector(tmp_path):
    """urf::BatchDetector (one upload, urf_classify_batch_pc2_ragged + urf_clouds_batch_pc2, one read-back) against
    urf::Detector::filtered message by message: same clouds byte for byte, same headers, in both orders and three layouts."""
    exe = build_demo(tmp_path, "batch_detector_demo")
    clouds = [u.synth_cloud(64, 2048, 1, 61), without_dropouts(u.synth_cloud(64, 2048, 3, 62)), (np.zeros(0, np.float32),) * 3,
              u.synth_cloud(64, 2048, 2, 63), without_dropouts(u.synth_cloud(64, 2048, 3, 64))]
    path = tmp_path / "clouds.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(clouds)))
        for k, (x, y, z) in enumerate(clouds):
            f.write(struct.pack("<I", len(x)))
            for a in (x, y, z, intensity_of(len(x), k)):
                f.write(np.ascontiguousarray(a, np.float32).tobytes())
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("layout ")]
    assert len(lines) == 6, r.stdout
    for ln in lines:
        f = ln.split()
        assert f[5] == "5" and f[7] == "4" and int(f[9]) > 0 and f[11] == "5", ln   # messages, published, points, equal
    assert "mixed layouts refused -1" in r.stdout and r.stdout.rstrip().endswith("done")
