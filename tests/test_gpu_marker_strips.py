"""road_marker's line strips for batches on the device (urf_marker_strips_batch) against urf_marker_strips and oracle B, every
scan of every call, exactly: adversarial marker-point sets, the chain classify -> marker points -> strips, splitting
invariance through the device-side ghost count, the fused front end, and urf::BatchDetector against urf::Detector."""
import struct
import subprocess

import numpy as np
import pytest

import marker_sets as M
import oracles as O
import urban_road_filter_amd as u
from hipmem import DevBuf

pytestmark = pytest.mark.gpu
STRIDE_P = u.MARKER_MAX_POINTS * 4


def strips_batch(ctx, sets, mp, sequence, ghost=None, splits=None):
    """The sets through urf_marker_strips_batch (in calls of `splits` scans, chained through one device word).
    Returns ([(published, strips, xyz)], ghost word afterwards or None)."""
    S = len(sets)
    pts = np.full((S, STRIDE_P), np.nan, np.float32)   # beyond a scan's count: never read
    for s, p in enumerate(sets):
        pts[s, :p.size] = p.reshape(-1)
    d_pts, d_cnt = DevBuf.from_numpy(pts), DevBuf.from_numpy(np.array([len(p) for p in sets], np.uint32))
    d_ghost = DevBuf.from_numpy(np.array([ghost], np.int32)) if ghost is not None else None
    d_strips, d_xyz, d_n = DevBuf(S * u.MARKER_MAX_STRIPS * 32), DevBuf(S * u.MARKER_MAX_STRIP_POINTS * 12), DevBuf(S * 12)
    for b in (d_strips, d_xyz, d_n):
        b.fill(0xEE)
    s0 = 0
    for k in (splits or [S]):
        ctx.marker_strips_batch(mp, d_pts.ptr + s0 * STRIDE_P * 4, d_cnt.ptr + s0 * 4, k, sequence, d_ghost,
                                d_strips.ptr + s0 * u.MARKER_MAX_STRIPS * 32, d_xyz.ptr + s0 * u.MARKER_MAX_STRIP_POINTS * 12, d_n.ptr + s0 * 12)
        s0 += k
    assert s0 == S
    ctx.synchronize()
    return unpack(d_strips, d_xyz, d_n, S), (int(d_ghost.to_numpy(np.int32)[0]) if d_ghost is not None else None)


def unpack(d_strips, d_xyz, d_n, S):
    n = d_n.to_numpy(np.uint32).reshape(S, 3)
    strips = d_strips.to_numpy(u.MARKER_STRIP_DTYPE).reshape(S, u.MARKER_MAX_STRIPS)
    xyz = d_xyz.to_numpy(np.float32).reshape(S, u.MARKER_MAX_STRIP_POINTS, 3)
    assert (n[:, 0] <= 1).all() and (n[:, 1] <= u.MARKER_MAX_STRIPS).all() and (n[:, 2] <= u.MARKER_MAX_STRIP_POINTS).all()
    return [(bool(n[s, 0]), strips[s, :n[s, 1]].copy(), xyz[s, :n[s, 2]].copy()) for s in range(S)]


def assert_equal_records(got, want, what):
    assert len(got) == len(want)
    for s, ((pa, sa, xa), (pb, sb, xb)) in enumerate(zip(got, want)):
        assert pa == pb and sa.tobytes() == sb.tobytes() and xa.tobytes() == xb.tobytes(), "%s: scan %d" % (what, s)


def assert_equal_oracle(got, want_b, what):
    for s, ((pub, strips, xyz), mb) in enumerate(zip(got, want_b)):
        assert O.markers_equal(M.as_markers(pub, strips, xyz), mb), "%s: scan %d against oracle B" % (what, s)


@pytest.mark.parametrize("simp,zavg", M.MP_COMBOS)
@pytest.mark.parametrize("sequence", [1, 0])
def test_batch_equals_host_and_oracle_b(simp, zavg, sequence):
    mp = M.marker_params(simp, zavg)
    small = [np.zeros((k, 4), np.float32) for k in (0, 2, 1)]   # unpublished scans at the start ...
    adv = [[p for _, p in M.adversarial_sets(seed)] for seed in (11, 12, 13)]   # ... and mixed in
    # ... and runs of 70 and 130 of them between publishing scans: the look-back takes 64 counts per step
    gap = lambda k: [np.zeros((k % 3, 4), np.float32) for k in range(k)]   # noqa: E731
    sets = small + adv[0] + gap(70) + adv[1] + gap(130) + adv[2]
    assert len(sets) > 500 and sum(len(p) <= 2 for p in sets) > 200
    with u.Context(1024, len(sets)) as ctx:
        got, ghost = strips_batch(ctx, sets, mp, sequence, ghost=9)
    want, g_host = M.host_sequence(sets, mp, 9, bool(sequence))
    want_b, g_b, _ = M.oracle_sequence(sets, mp, 9, bool(sequence))
    assert_equal_records(got, want, "urf_marker_strips")
    assert_equal_oracle(got, want_b, "sequence %d" % sequence)
    if sequence:
        assert ghost == g_host[-1] == g_b[-1]
        assert any((s["action"] == u.MARKER_DELETE).any() for _, s, _ in got)
    else:
        assert ghost == 9 and not any((s["action"] == u.MARKER_DELETE).any() for _, s, _ in got)


@pytest.mark.parametrize("tol", [0.0, 0.05, 3.0, -1.0, float("nan")])
def test_batch_tolerances(tol):
    mp = M.marker_params(1, 0, tol)
    sets = [p for _, p in M.adversarial_sets(13, n_random=10)]
    with u.Context(1024, len(sets)) as ctx:
        got, ghost = strips_batch(ctx, sets, mp, 1, ghost=0)
    want, g_host = M.host_sequence(sets, mp, 0)
    assert_equal_records(got, want, "tolerance %r" % tol)
    assert_equal_oracle(got, M.oracle_sequence(sets, mp, 0)[0], "tolerance %r" % tol)
    assert ghost == g_host[-1]


def test_ghost_chain_edges():
    """Unpublished scans only (the count passes through the call), a NULL ghost word, clamping of the incoming count."""
    mp = M.marker_params(0, 0)
    none = [np.zeros((k, 4), np.float32) for k in (0, 1, 2, 2, 0)]
    one = np.zeros((3, 4), np.float32)
    one[:, 0] = [0, 1, 2]
    with u.Context(1024, 16) as ctx:
        for g_in in (6, 10 ** 6, 180, -5):   # nothing publishes: the word is handed on as it came, as urf_marker_strips leaves it
            got, ghost = strips_batch(ctx, none, mp, 1, ghost=g_in)
            assert ghost == g_in == M.host_sequence(none, mp, g_in)[1][-1]
            assert all(not pub and len(s) == 0 and len(x) == 0 for pub, s, x in got)
        got, ghost = strips_batch(ctx, none + [one], mp, 1, ghost=None)
        assert ghost is None and got[-1][0] and len(got[-1][1]) == 1
        for g_in in (10 ** 6, 180, 179, -5, 4):
            got, ghost = strips_batch(ctx, none + [one] + none, mp, 1, ghost=g_in)
            want, g_host = M.host_sequence(none + [one] + none, mp, g_in)
            assert_equal_records(got, want, "incoming count %d" % g_in)
            assert ghost == g_host[-1] == 0 and len(got[5][1]) == min(max(g_in, 0), 179) + 1
        with pytest.raises(u.UrfError) as e:
            strips_batch(ctx, [one] * 17, mp, 1, ghost=0)   # more scans than the context's max_batch
        assert e.value.code == -4
        d = DevBuf(64)
        for args in [(None, d, d, d, d), (d, None, d, d, d), (d, d, None, d, d), (d, d, d, None, d), (d, d, d, d, None)]:
            with pytest.raises(u.UrfError) as e:
                ctx.marker_strips_batch(mp, args[0], args[1], 1, 1, None, args[2], args[3], args[4])
            assert e.value.code == -1


def sweeps_with_gap():
    """SEQ5's sweeps with one that publishes nothing (every coordinate far outside the region of interest) in the middle."""
    scans = [O.cfg_cloud(cfg, seed) for cfg, _, seed in M.SEQ5]
    assert len({len(s[0]) for s in scans}) == 1
    far = tuple(np.ascontiguousarray(a * np.float32(1000.0)) for a in scans[0])
    return scans[:2] + [far] + scans[2:]


def chain(ctx, scans, mp, splits, d_ghost):
    """classify_batch_soa -> marker_points_batch -> marker_strips_batch per group of `splits` sweeps; everything stays on the device."""
    n = len(scans[0][0])
    out, infos, s0 = [], [], 0
    for k in splits:
        grp = scans[s0:s0 + k]
        d_x, d_y, d_z = (DevBuf.from_numpy(np.concatenate([s[a] for s in grp])) for a in range(3))
        d_lab, d_info = DevBuf(k * n), DevBuf(k * 32)
        d_pts, d_cnt = DevBuf(k * STRIDE_P * 4), DevBuf(k * 4)
        d_strips, d_xyz, d_n = DevBuf(k * u.MARKER_MAX_STRIPS * 32), DevBuf(k * u.MARKER_MAX_STRIP_POINTS * 12), DevBuf(k * 12)
        ctx.classify_batch_soa(d_x, d_y, d_z, n, k, d_lab, d_info)
        ctx.marker_points_batch(d_pts, d_cnt)
        ctx.marker_strips_batch(mp, d_pts, d_cnt, k, 1, d_ghost, d_strips, d_xyz, d_n)
        ctx.synchronize()
        out += unpack(d_strips, d_xyz, d_n, k)
        infos += [int(v) for v in d_info.to_numpy(np.int32).reshape(k, 8)[:, 0]]
        s0 += k
    return out, infos


def oracle_chain(scans, p, mp):
    pts = [O.run_b(x, y, z, p, debug=True) for x, y, z in scans]
    status = [r[1]["status"] for r in pts]
    sets = [r[2]["marker_pts"] if r[1]["status"] == 0 else np.zeros((0, 4), np.float32) for r in pts]
    want_b, g_b, _ = M.oracle_sequence(sets, mp, 0)
    return want_b, g_b, status


@pytest.mark.parametrize("simp,zavg", [(1, 1), (0, 0)])
@pytest.mark.parametrize("front", [1, 2])
def test_end_to_end_and_splitting(simp, zavg, front):
    """One call, calls of one sweep, 3 + the rest: identical records, equal to oracle B; with front = 2 the batch call takes the
    fused front end first (urf_marker_points_batch then re-runs it through the general kernels)."""
    p, mp = O.cfg_params("cfg2"), M.marker_params(simp, zavg)
    scans = sweeps_with_gap()
    S = len(scans)
    want_b, g_b, status = oracle_chain(scans, p, mp)
    assert status[2] == 1 and want_b[2] is None and g_b[2] == g_b[1]   # the gap: URF_TOO_FEW_POINTS, the count passes through
    n_del = sum(m["action"] == 2 for w in want_b if w for m in w)
    n_strips = [sum(m["action"] == 0 for m in w) for w in want_b if w]
    assert n_del >= 1 and len(set(n_strips)) > 1 and all(len({m["color"] for m in w if m["action"] == 0}) == 2 for w in want_b if w)
    results = []
    for splits in ([S], [1] * S, [3, S - 3]):
        with u.Context(len(scans[0][0]), S, params=p) as ctx:
            ctx.set_front_mode(front)
            d_ghost = DevBuf.from_numpy(np.zeros(1, np.int32))
            got, infos = chain(ctx, scans, mp, splits, d_ghost)
            assert infos == status
            assert_equal_oracle(got, want_b, "splits %r" % (splits,))
            assert int(d_ghost.to_numpy(np.int32)[0]) == g_b[-1]
            results.append(got)
    assert_equal_records(results[1], results[0], "calls of one sweep")
    assert_equal_records(results[2], results[0], "3 + the rest")


def test_fused_front_end_was_taken():
    """The premise of front = 2 above: such a batch call does take the fused front end before the marker points are asked for."""
    p = O.cfg_params("cfg2")
    scans = sweeps_with_gap()
    n, S = len(scans[0][0]), len(scans)
    with u.Context(n, S, params=p) as ctx:
        ctx.set_front_mode(2)
        d_x, d_y, d_z = (DevBuf.from_numpy(np.concatenate([s[a] for s in scans])) for a in range(3))
        d_lab = DevBuf(S * n)
        ctx.classify_batch_soa(d_x, d_y, d_z, n, S, d_lab)
        assert ctx.front_scans() > 0


def read_marker_arrays(blob, n_msgs):
    pos, out = 0, []
    for _ in range(n_msgs):
        published, nm = struct.unpack_from("<2I", blob, pos)
        pos += 8
        ms = []
        for _ in range(nm):
            mid, act, typ = struct.unpack_from("<3i", blob, pos)
            col = struct.unpack_from("<4f", blob, pos + 12)
            (npt,) = struct.unpack_from("<I", blob, pos + 28)
            pos += 32
            pts = np.frombuffer(blob, np.float64, 3 * npt, pos).reshape(-1, 3).copy()
            pos += 24 * npt
            ms.append({"id": mid, "action": act, "type": typ, "color": col, "points": pts})
        out.append(ms if published else None)
    assert pos == len(blob)
    return out


@pytest.mark.parametrize("simp,zavg", [(1, 1), (0, 0), (-1, -1)])
def test_batch_detector_road_marker(tmp_path, simp, zavg):
    """urf::Detector message by message, urf::BatchDetector in batches of 2 and of 4 + the rest: the same MarkerArrays (the demo
    also compares frame_id, scale, orientation and type itself), equal to oracle B.  (-1, -1): neither detector is given marker
    parameters, both run with urf_default_marker_params."""
    from test_gpu_detector import build_demo
    exe = build_demo(tmp_path, "batch_marker_demo")
    scans = sweeps_with_gap()
    files = []
    for k, (x, y, z) in enumerate(scans):
        files.append(str(tmp_path / ("sweep%d.bin" % k)))
        with open(files[-1], "wb") as f:
            f.write(struct.pack("<I", len(x)) + x.tobytes() + y.tobytes() + z.tobytes())
    outs = [str(tmp_path / ("markers%d.bin" % k)) for k in range(3)]
    r = subprocess.run([exe, str(simp), str(zavg)] + outs + files, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    blobs = [open(o, "rb").read() for o in outs]
    assert blobs[0] == blobs[1] == blobs[2]
    p = u.default_params()   # the demo's parameters: marker_demo's
    p.min_X = p.min_Y = -200.0
    p.max_X = p.max_Y = 200.0
    want_b, _, _ = oracle_chain(scans, p, M.marker_params(simp, zavg) if simp >= 0 else u.default_marker_params())
    got = read_marker_arrays(blobs[0], len(scans))
    assert any(m["action"] == 2 for w in got if w for m in w) and got[2] is None
    for k in range(len(scans)):
        assert O.markers_equal(got[k], want_b[k]), "message %d" % k
