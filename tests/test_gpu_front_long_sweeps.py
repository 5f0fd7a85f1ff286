"""urf_set_front_long_sweeps(ctx, 1): front modes 2 and 3 send scans of 129..256 tiles of 2048 points through the fused front end (the
finish kernels with the dynamic LDS that many tiles need).  Labels and the seven summary fields against oracle B on the same input -- 129
tiles at 128 and at 64 lasers, 256 tiles (the clouds of the goldens cfg5_s1 and sensor5_s1), 257 tiles (which keep the general kernels),
ragged batches, row-major sweeps in batches and on the callback path, hand-backs, the read-outs of urf_set_front_outputs -- and what must
not change: 128 tiles with the switch on, 128 lasers without urf_set_front_lasers128, mode 1.

Oracle B runs once per input (ref()); a cloud is a handful of sweeps of at most 128 x 4112 points."""
import os

import numpy as np
import pytest

import oracles as O
import urban_road_filter_amd as u
from golden.make_golden import cloud_sha
from test_gpu_front import fused_batch
from test_gpu_front_lasers128 import KEYS, params, ring_major, rolled
from test_gpu_front_outputs import Soa, batch_readouts

pytestmark = pytest.mark.gpu
L = 128
GOLD = os.path.join(os.path.dirname(__file__), "golden")
_REF, _CLOUD = {}, {}


def cloud(lasers, cols, scene, seed):
    key = (lasers, cols, scene, seed)
    if key not in _CLOUD:
        _CLOUD[key] = u.synth_cloud(lasers, cols, scene, seed)
    return _CLOUD[key]


def ref(key, scan, p):
    """Oracle B on one input, computed once (labels, summary); never modified.  key names the input AND the parameters."""
    if key not in _REF:
        _REF[key] = O.run_b(*scan, p)[:2]
    return _REF[key]


def equal_to_b(labels, infos, scans, keys, p, something=True):
    """What test_gpu_front_lasers128.says_something and test_gpu_parity.check_against_b assert, from the one oracle run per input."""
    for k, (scan, key) in enumerate(zip(scans, keys)):
        lb, ib = ref(key, scan, p)
        if something:   # (no comparison passes on an empty result)
            assert ib["n_road"] > 0 and ib["n_curb"] > 0, (key, ib)
        assert np.array_equal(labels[k], lb), "scan %d (%s): %d labels differ" % (k, key, int((labels[k] != lb).sum()))
        assert {f: int(v) for f, v in zip(KEYS, infos[k][:7])} == {f: ib[f] for f in KEYS}, "scan %d (%s)" % (k, key)
        assert infos[k][7] == 0


def fused_long(ctx, scans, p, mode=2, lasers128=1, long=1, ragged=False):
    ctx.set_front_lasers128(lasers128)
    ctx.set_front_long_sweeps(long)
    return fused_batch(ctx, scans, p, mode=mode, ragged=ragged)


def over128():
    """the pair of test_gpu_front_lasers128.test_sweeps_of_128_tiles_are_fused_and_of_129_are_not: 128 x 2064, 129 tiles"""
    return [cloud(L, 2064, 1, 63), cloud(L, 2064, 3, 64)], [("l128", 2064, 1, 63), ("l128", 2064, 3, 64)]


def params64(cp=5):
    p = u.default_params().wide_roi()
    p.channels = 64
    p.curbPoints = cp
    return p


def golden_pair():
    """the clouds of the goldens cfg5_s1 and sensor5_s1 (128 x 4096: 256 tiles), checksum as test_gpu_parity.test_golden_cases asserts it"""
    scans, gold = [], []
    for name, cfg in (("cfg5_s1", "cfg5"), ("sensor5_s1", "sensor5")):
        g = np.load(os.path.join(GOLD, name + ".npz"))
        if name not in _CLOUD:
            _CLOUD[name] = O.case_cloud(cfg, 1, g)
        assert cloud_sha(*_CLOUD[name]) == str(g["cloud_sha"])
        scans.append(_CLOUD[name])
        gold.append(g["labels"])
    return scans, ["cfg5_s1", "sensor5_s1"], gold


def check_256_tiles(ctx):
    p = O.cfg_params("cfg5")
    scans, keys, gold = golden_pair()
    labels, infos, nf = fused_long(ctx, scans, p)
    assert nf == 2
    for k in range(2):
        assert np.array_equal(labels[k] & O.MASK_NO_RING, gold[k]), "differs from the reference's labels (%s)" % keys[k]
    equal_to_b(labels, infos, scans, keys, p)


# ---- 1. 129 tiles, 128 lasers ----
def test_129_tiles_of_128_lasers_on_off_on():
    p = params()
    scans, keys = over128()
    assert all(ref(k, s, p)[1]["n_rings"] == 128 for k, s in zip(keys, scans))
    with u.Context(L * 2064, 2) as ctx:
        for long, want in ((1, 2), (0, 0), (1, 2)):
            labels, infos, nf = fused_long(ctx, scans, p, long=long)
            assert nf == want, (long, nf)
            equal_to_b(labels, infos, scans, keys, p)


# ---- 2. 129 tiles, 64 lasers ----
@pytest.mark.parametrize("mode,cp", [(2, 5), (3, 7)])
def test_129_tiles_of_64_lasers(mode, cp):
    p = params64(cp)
    scans = [cloud(64, 4128, 1, 71), cloud(64, 4128, 3, 72)]
    keys = [("l64", 4128, 1, 71, cp), ("l64", 4128, 3, 72, cp)]
    with u.Context(64 * 4128, 2) as ctx:
        labels, infos, nf = fused_long(ctx, scans, p, mode=mode, lasers128=0)
        assert nf == 2
        equal_to_b(labels, infos, scans, keys, p)


# ---- 3. 256 tiles ----
def test_256_tiles_the_clouds_of_the_goldens():
    with u.Context(L * 4096, 2) as ctx:
        check_256_tiles(ctx)


# ---- 4. 257 tiles ----
def test_257_tiles_keep_the_general_kernels():
    p = params()
    scans = [cloud(L, 4112, 1, 81), cloud(L, 4112, 3, 82)]
    keys = [("l128", 4112, 1, 81), ("l128", 4112, 3, 82)]
    with u.Context(L * 4112, 2) as ctx:
        labels, infos, nf = fused_long(ctx, scans, p)
        assert nf == 0
        equal_to_b(labels, infos, scans, keys, p)
        check_256_tiles(ctx)


# ---- 5. ragged ----
def test_ragged_batch():
    p = params()
    b = cloud(L, 4096, 3, 91)
    scans = [cloud(L, 17, 1, 7), cloud(L, 2064, 3, 64), tuple(v[:L * 3000 + 7].copy() for v in b)]   # (the last one ends inside a firing)
    keys = [("l128", 17, 1, 7), ("l128", 2064, 3, 64), ("l128", 4096, 3, 91, "cut")]
    with u.Context(L * 4096, len(scans)) as ctx:
        labels, infos, nf = fused_long(ctx, scans, p, ragged=True)
        assert nf >= 2
        equal_to_b(labels, infos, scans, keys, p)


# ---- 6. row-major ----
@pytest.mark.parametrize("lasers,cols", [(128, 2064), (64, 4128)])
def test_row_major_batches_are_fused_from_the_second_call(lasers, cols):
    p = params() if lasers == 128 else params64()
    rm = lambda c: tuple(np.ascontiguousarray(a.reshape(-1, lasers).T.reshape(-1)) for a in c)
    scans = [rm(cloud(lasers, cols, 1, 63 if lasers == 128 else 71)), rm(cloud(lasers, cols, 3, 64 if lasers == 128 else 72))]
    keys = [("rows", lasers, cols, 1), ("rows", lasers, cols, 3)]
    with u.Context(lasers * cols, len(scans)) as ctx:
        labels, infos, nf0 = fused_long(ctx, scans, p, lasers128=int(lasers == 128))
        equal_to_b(labels, infos, scans, keys, p)   # (the call that sights the layout)
        labels, infos, nf = fused_long(ctx, scans, p, lasers128=int(lasers == 128))
        assert nf == len(scans), (nf0, nf)
        equal_to_b(labels, infos, scans, keys, p)


def test_row_major_sweeps_on_the_callback_path_two_in_flight():
    p = params()
    scans = [ring_major(c) for c in over128()[0]]
    keys = [("rows", 128, 2064, 1), ("rows", 128, 2064, 3)]
    n = L * 2064
    recs = []
    for c in scans:
        r = np.zeros((n, 4), np.float32)
        r[:, 0], r[:, 1], r[:, 2] = c
        recs.append(r)
    with u.Context(n, 2, params=p) as ctx:
        ctx.set_front_lasers128(1)
        ctx.set_front_long_sweeps(1)
        ctx.set_front_mode(2)
        for rep in range(2):   # four sweeps, two in flight
            tickets = [ctx.classify_pc2_async(r, n, 16, 0, 4, 8) for r in recs]
            for k, t in enumerate(tickets):
                lab = np.zeros(n, np.uint8)
                info = ctx.classify_pc2_wait(t, lab)
                lb, ib = ref(keys[k], scans[k], p)
                assert np.array_equal(lab, lb), (rep, k)
                assert {f: getattr(info, f) for f in KEYS} == {f: ib[f] for f in KEYS}, (rep, k)


# ---- 7. hand-back ----
def test_scans_without_the_shape_are_handed_back():
    p = params()
    street = over128()[0]
    x, y, z = street[0]
    pm = np.random.default_rng(1).permutation(len(x))
    scans = [street[0], (x[pm], y[pm], z[pm]), street[1], rolled(cloud(L, 2064, 1, 65), 700)]
    keys = [("l128", 2064, 1, 63), ("l128", 2064, 1, 63, "shuffled"), ("l128", 2064, 3, 64), ("l128", 2064, 1, 65, "rolled")]
    says = [True, False, True, True]   # (a shuffled sweep has no road left)
    with u.Context(L * 2064, len(scans)) as ctx:
        for _ in range(3):   # first call: lists; then grids
            labels, infos, nf = fused_long(ctx, scans, p)
            assert nf == 2
            for k in range(4):
                equal_to_b(labels[k:k + 1], infos[k:k + 1], scans[k:k + 1], keys[k:k + 1], p, something=says[k])


# ---- 8. read-outs ----
def test_read_outs_of_a_fused_call_equal_those_of_the_general_kernels():
    p = params()
    scans, keys = over128()
    n = L * 2064
    b = Soa(scans)
    with u.Context(n, 2, params=p) as ctx:
        ctx.set_front_mode(0)
        b.classify(ctx)
        assert ctx.front_scans() == 0
        want = batch_readouts(ctx, 2, n)
    with u.Context(n, 2, params=p) as ctx:
        ctx.set_front_lasers128(1)
        ctx.set_front_long_sweeps(1)
        ctx.set_front_mode(2)
        ctx.set_front_outputs(1)
        b.classify(ctx)
        assert ctx.front_scans() == 2
        for s, lab in enumerate(b.labels()):
            assert np.array_equal(lab, ref(keys[s], scans[s], p)[0]), s
        got = batch_readouts(ctx, 2, n)
        assert ctx.front_scans() == 2
    for s in range(2):
        assert len(want[s][0]) > 0 and len(want[s][1]) > 0 and len(want[s][3]) > 2, s
        for k in range(3):
            assert np.array_equal(got[s][k], want[s][k]), (s, k, len(got[s][k]), len(want[s][k]))
        assert got[s][3].shape == want[s][3].shape and np.array_equal(got[s][3].view(np.uint32), want[s][3].view(np.uint32)), s


# ---- 9. what must not change ----
def test_what_must_not_change_with_the_switch_on():
    p = params()
    full = [cloud(L, 2048, 1, 61), cloud(L, 2048, 3, 62)]
    with u.Context(L * 2064, 2) as ctx:
        labels, infos, nf = fused_long(ctx, full, p)
        assert nf == 2
        equal_to_b(labels, infos, full, [("l128", 2048, 1, 61), ("l128", 2048, 3, 62)], p)
        scans, keys = over128()
        labels, infos, nf = fused_long(ctx, scans, p, lasers128=0)
        assert nf == 0
        equal_to_b(labels, infos, scans, keys, p)
        for bad in (2, -1):
            with pytest.raises(Exception):
                ctx.set_front_long_sweeps(bad)
            assert ctx._lib.urf_set_front_long_sweeps(ctx._h, bad) == -1
    p64 = params64()
    scans = [cloud(64, 4128, 1, 71), cloud(64, 4128, 3, 72)]
    with u.Context(64 * 4128, 2) as ctx:
        labels, infos, nf = fused_long(ctx, scans, p64, mode=1, lasers128=0)
        assert nf == 0
        equal_to_b(labels, infos, scans, [("l64", 4128, 1, 71, 5), ("l64", 4128, 3, 72, 5)], p64)
