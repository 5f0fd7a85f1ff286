"""Every live parameter at the ends of its declared range (tests/param_edge_cases.py: one at a time, corners of the box, accepted values
outside it) through the kernels, bit for bit against oracle B on the same input -- labels and the seven summary fields, no tolerance:
the general kernels on one long-lived context that is reconfigured between scans (with stage capture and the read-outs), the fused
front end on ideal batches (with the count of fused scans asserted wherever a ring per laser survives: a silent hand-back would leave
only the general kernels under test), the multi-sector instances on real sensors' geometries, the read-outs behind a fused call, and
the callback path's captured sequences across parameter changes.  tests/test_param_edges_cpu.py judges oracle B on the same cases
against the reference's own sources."""
import numpy as np
import pytest

import gpu_sensor_cases as G
import oracles as O
import param_edge_cases as PE
import sensor_models as SM
import urban_road_filter_amd as u
from test_gpu_front import fused_batch
from test_gpu_front_outputs import Soa, batch_readouts
from test_gpu_front_outputs import same as same_readouts
from test_gpu_parity import check_against_b
from test_gpu_sensor_models import KEYS, same, three_calls

pytestmark = pytest.mark.gpu
_B = {}
GENERAL = PE.general_clouds()
ONE = [n for n, _ in PE.ONE_AT_A_TIME]
CORNER = [n for n, _ in PE.CORNERS]
OUTSIDE = [n for n, _ in PE.OUTSIDE]
MERGING = ("interval 10", "interval 100", "interval inf")   # lasers share rings: equality and a repeatable count only


def ref(key, cloud, p):
    """Oracle B on one (cloud, parameters), computed once (labels, summary, stages); never modified."""
    key = (key, bytes(p))
    if key not in _B:
        _B[key] = O.run_b(*cloud, p, debug=True)
    return _B[key]


def case_params(table, name, base):
    tweak = PE.case(table, name)
    return PE.corner_params(tweak, base.channels) if table == "corner" else PE.params(base, tweak)


def deep(table, name):
    """Every fourth case of a table: exact mode and the read-outs too."""
    return [n for n, _ in PE.TABLES[table]].index(name) % 4 == 0


# ---- a. the general kernels, one scan at a time, one context reconfigured between the scans ----
@pytest.fixture(scope="module")
def ctx():
    c = u.Context(32768, 1)
    yield c
    c.close()


def check_info(ig, ib, what):
    assert {k: getattr(ig, k) for k in KEYS} == {k: ib[k] for k in KEYS}, what


def check_scan(ctx, cname, cloud, p, with_exact, with_readouts):
    lb, ib, st = ref(cname, cloud, p)
    n = len(cloud[0])
    ctx.set_params(p)
    lg, ig = ctx.classify_xyz(*cloud)   # the production path proper (records nothing per input point)
    assert np.array_equal(lg, lb), "%s: %d labels differ" % (cname, int((lg != lb).sum()))
    check_info(ig, ib, cname)
    if with_readouts and ib["status"] == 0:
        got = ctx.ordered_indices(n) + (ctx.marker_points(),)
        same_readouts(got, st, cname)
    for mode in (2, 1) if with_exact else (2,):
        ctx.enable_stage_capture(mode)
        try:
            lg, ig = ctx.classify_xyz(*cloud)
            if ib["status"] == 0:
                assert np.array_equal(ctx.read_stage(u.STAGE_RING, n), st["ring"]), (cname, mode, "ring")
                if p.star_shaped_method:
                    assert np.array_equal(ctx.read_stage(u.STAGE_SECTOR, n), st["sector"]), (cname, mode, "sector")
                assert np.array_equal(ctx.read_stage(u.STAGE_DETECT, n), st["detect"]), (cname, mode, "detect")
                assert np.array_equal(ctx.read_stage(u.STAGE_BEAM_STOP, n), st["beam_stop"]), (cname, mode, "beam_stop")
        finally:
            ctx.enable_stage_capture(0)
        assert np.array_equal(lg, lb), "%s, capture %d: %d labels differ" % (cname, mode, int((lg != lb).sum()))
        check_info(ig, ib, (cname, mode))
    return lg, ig.as_dict()


def check_general(ctx, table, name):
    for cname, cloud, base in GENERAL:
        check_scan(ctx, cname, cloud, case_params(table, name, base), deep(table, name), deep(table, name))


@pytest.mark.parametrize("name", ONE)
def test_general_kernels_one_at_a_time(ctx, name):
    check_general(ctx, "one", name)


@pytest.mark.parametrize("name", CORNER)
def test_general_kernels_corners(ctx, name):
    check_general(ctx, "corner", name)


@pytest.mark.parametrize("name", OUTSIDE)
def test_general_kernels_outside_the_box(ctx, name):
    check_general(ctx, "outside", name)


def test_general_kernels_return_to_the_first_parameters(ctx):
    """No derived constant (the beams' table, the cosine thresholds, the key widths) survives a later urf_set_params."""
    cname, cloud, base = GENERAL[5]
    first = case_params("one", ONE[0], base)
    l0, i0 = check_scan(ctx, cname, cloud, first, False, False)
    for table in ("one", "corner", "outside"):
        check_scan(ctx, cname, cloud, case_params(table, PE.TABLES[table][-1][0], base), False, False)
    far = PE.params(base, {"angleFilter1": 180.0, "angleFilter2": 0.0, "beam_width": 5.0, "starbeam_filter": 1})
    far.sectors = 720
    check_scan(ctx, cname, cloud, far, False, False)
    l1, i1 = check_scan(ctx, cname, cloud, first, False, False)
    assert np.array_equal(l0, l1) and i0 == i1


# ---- b. the fused front end on ideal batches ----
def calls(ctx, scans, p, mode):
    """three_calls (tests/test_gpu_sensor_models.py) in front mode `mode`: twice, then mode 0, every call against B."""
    if mode == 2:
        return three_calls(ctx, scans, p)
    labels0, infos0, nf0 = fused_batch(ctx, scans, p, mode=mode)
    check_against_b(labels0, infos0, scans, p)
    labels, infos, nf1 = fused_batch(ctx, scans, p, mode=mode)
    same(labels, infos, labels0, infos0)
    labels, infos, nf = fused_batch(ctx, scans, p, mode=0)
    assert nf == 0
    same(labels, infos, labels0, infos0)
    return nf0, nf1


def capacity(scans):
    """max_points of a context for these sweeps.  The fused front end keeps the points whose detector decision is pending in a list of
    max_points / 8 entries per scan (at least 4096; urf_api.hip: front_cand_cap), sized for sweeps of a thousand firings and more.  In
    a sweep of 256 firings the neighbours on a ring are 1.4 degrees apart and more than a quarter of the points are pending: in a
    context sized for 64 x 256 points the list overflows and the scan is handed back -- capacity, not shape, and no parameter's doing.
    A context sized for sixteen times the points holds an entry for both detectors of every point."""
    return 16 * max(len(s[0]) for s in scans)


def front_context(scans, p, multi=False):
    """A context in the front mode the parameters' curbPoints need: 2, or 3 with every opt-in instance for curbPoints 1..8."""
    ctx = u.Context(capacity(scans), len(scans))
    mode = 2
    if multi:
        ctx.set_front_multi_sector(1)
    if p.curbPoints != 5 and p.curbPoints <= PE.FRONT_MAX_CURB_POINTS:
        mode = 3
        ctx.set_front_curb_points(1)
        if multi:
            ctx.set_front_multi_sector_curb_points(1)
    return ctx, mode


def check_fused(table, name, L, layout):
    scans = PE.ideal_batch(L, layout)
    p = case_params(table, name, PE.base_params(L))
    refs = [ref(("ideal", L, layout, k), c, p) for k, c in enumerate(scans)]
    ctx, mode = front_context(scans, p)
    with ctx:
        nf0, nf1 = calls(ctx, scans, p, mode)
    what = (name, L, layout, nf0, nf1)
    if p.curbPoints > PE.FRONT_MAX_CURB_POINTS:
        assert (nf0, nf1) == (0, 0), what                         # no fused instance
    elif name in MERGING:
        ctx, mode = front_context(scans, p)
        with ctx:
            again = tuple(fused_batch(ctx, scans, p, mode=mode)[2] for _ in range(2))
        assert again == (nf0, nf1), what
    elif all(r[1]["status"] == 0 for r in refs):
        # a ring per laser (inside the box: wherever B counts L rings, tests/test_param_edges_cpu.py): nothing may be handed back in
        # silence.  interval 0 leaves some sweeps without it (two table entries for one laser): those may go, the others may not.
        assert nf1 >= sum(PE.ring_per_laser(r[2], r[1], L, layout) for r in refs), what


@pytest.mark.parametrize("L,layout", PE.FUSED)
@pytest.mark.parametrize("name", ONE)
def test_fused_front_end_one_at_a_time(name, L, layout):
    check_fused("one", name, L, layout)


@pytest.mark.parametrize("L,layout", PE.FUSED)
@pytest.mark.parametrize("name", OUTSIDE)
def test_fused_front_end_outside_the_box(name, L, layout):
    check_fused("outside", name, L, layout)


@pytest.mark.parametrize("L,layout", PE.FUSED)
@pytest.mark.parametrize("name", CORNER)
def test_fused_front_end_corners(name, L, layout):
    check_fused("corner", name, L, layout)


@pytest.mark.parametrize("interval", [0.01, 0.18])
def test_fused_front_end_on_points_off_their_lasers_cone(interval):
    """The jitter sweep: at interval 0.01 three quarters of the points find no ring."""
    scans = [PE.jitter_sweep(), PE.ideal_batch(64, "firing")[1]]
    p = PE.params(PE.base_params(64), {"interval": interval})
    with u.Context(capacity(scans), 2) as ctx:
        counts = three_calls(ctx, scans, p)
    with u.Context(capacity(scans), 2) as ctx:
        assert tuple(fused_batch(ctx, scans, p)[2] for _ in range(2)) == counts


# ---- c. real geometries: the multi-sector instances ----
@pytest.mark.parametrize("model", PE.REAL)
@pytest.mark.parametrize("name", ONE)
def test_real_geometries_one_at_a_time(name, model):
    scans = [PE.real_sweep(model), G.control(model, PE.FIRINGS, world=1, seed=96, noise=True, holes=("nan",))]
    p = case_params("one", name, PE.base_params(SM.lasers(model)))
    ctx, mode = front_context(scans, p, multi=True)
    with ctx:
        counts = calls(ctx, scans, p, mode)
    ctx, mode = front_context(scans, p, multi=True)
    with ctx:
        assert tuple(fused_batch(ctx, scans, p, mode=mode)[2] for _ in range(2)) == counts, (name, model)
    if p.curbPoints > PE.FRONT_MAX_CURB_POINTS:
        assert counts == (0, 0)


# ---- d. the read-outs behind a fused call ----
@pytest.mark.parametrize("name", ONE)
def test_readouts_behind_a_fused_call(name):
    L, layout = 64, "firing"
    scans = PE.ideal_batch(L, layout)
    p = case_params("one", name, PE.base_params(L))
    refs = [ref(("ideal", L, layout, k), c, p) for k, c in enumerate(scans)]
    b = Soa(scans)
    ctx, mode = front_context(scans, p)
    with ctx:
        ctx.set_params(p)
        ctx.set_front_mode(mode)
        ctx.set_front_outputs(1)
        for call in range(2):
            b.classify(ctx)
            nf = ctx.front_scans()
            for s, lab in enumerate(b.labels()):
                assert np.array_equal(lab, refs[s][0]), (name, call, s)
            for s, got in enumerate(batch_readouts(ctx, len(scans), b.lens[0])):
                same_readouts(got, refs[s][2], (name, call, s))
            assert ctx.front_scans() == nf, name                   # no second run through the general kernels
        if p.curbPoints <= PE.FRONT_MAX_CURB_POINTS and name not in MERGING and all(PE.ring_per_laser(r[2], r[1], L, layout) for r in refs):
            assert nf == len(scans), name


# ---- f. the callback path: the captured sequence follows every parameter change ----
def test_callback_path_through_every_edge_in_sequence():
    cloud, base = PE.ideal_batch(64, "firing")[0], PE.base_params(64)
    n = len(cloud[0])
    rec = np.zeros((n, 4), np.float32)
    rec[:, 0], rec[:, 1], rec[:, 2] = cloud
    with u.Context(n, 1, params=base) as ctx:
        for name in ["xDirection 0"] + ONE + ["xDirection 0"]:
            p = case_params("one", name, base)
            lb, ib, _ = ref(("ideal", 64, "firing", 0), cloud, p)
            ctx.set_params(p)
            for call in range(2):   # (the second sweep with these parameters: the captured sequence replayed)
                lg, ig = ctx.classify_pc2(rec, n, 16, 0, 4, 8)
                assert np.array_equal(lg, lb), "%s, call %d: %d labels differ" % (name, call, int((lg != lb).sum()))
                check_info(ig, ib, (name, call))
