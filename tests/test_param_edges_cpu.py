"""The judge of tests/test_gpu_param_edges.py on the CPU: on every case of tests/param_edge_cases.py -- each live parameter at the ends
of its declared range, corners of that box, accepted values outside it -- oracle B equals the reference's own sources (oracle A, shared
libm), and the cases say something: an edge changes B's labels against the defaults on at least one cloud, the fused clouds keep a ring
per laser, the jitter sweep loses ring points at interval 0.01.

Oracle A reads array3D[10] unconditionally: every cloud it judges has more than 10 channels."""
import numpy as np
import pytest

import oracles as O
import param_edge_cases as PE
import sensor_models as SM
import urban_road_filter_amd as u

# oracle A's cloud set per table (its recorded outputs are committed: tests/golden/oracle_a); oracle B runs every cloud everywhere else
A_CLOUDS = {"one": ("fuzz ties", "hdl64e", "vlp16", "ideal64 firing w0", "jitter"),
            "outside": ("fuzz ties", "vlp16", "ideal64 firing w0"),
            "corner": ("fuzz ties", "hdl32e", "ideal16 firing w1")}
_B = {}


def clouds():
    return {n: (c, p) for n, c, p in PE.general_clouds()}


def run_b(name, p):
    key = (name, bytes(p))
    if key not in _B:
        _B[key] = O.run_b(*clouds()[name][0], p, debug=True)
    return _B[key]


def case_params(table, tweak, base):
    return PE.corner_params(tweak, base.channels) if table == "corner" else PE.params(base, tweak)


A_CASES = [(t, name) for t in ("one", "corner", "outside") for name, _ in PE.TABLES[t]]


@pytest.mark.parametrize("table,name", A_CASES)
def test_oracle_b_equals_reference(table, name):
    tweak = PE.case(table, name)
    for cname in A_CLOUDS[table]:
        cloud, base = clouds()[cname]
        p = case_params(table, tweak, base)
        assert p.channels > 10
        la, ia, _, _ = O.run_a([cloud], p, libm=True)
        lb, ib, st = run_b(cname, p)
        assert ia[0]["status"] == ib["status"], cname
        assert np.array_equal(la[0], lb & O.MASK_NO_RING), "%s: %d labels differ" % (cname, int((la[0] != (lb & O.MASK_NO_RING)).sum()))
        if ib["status"] == 0:
            for key in ("n_roi", "n_road", "n_curb", "n_ring10"):
                assert ia[0][key] == ib[key], (cname, key)
            for key in ("road_order", "curb_order", "ring10_order"):
                assert np.array_equal(ia[0][key], st[key]), (cname, key)


def test_the_case_table_holds_both_ends_of_every_hot_path_row():
    """Compared against urf_param_table(): a row that is added, or whose range changes, is a case or a failure here."""
    one = dict(PE.ONE_AT_A_TIME)
    hot = [t for t in u.param_table() if t["where"] == PE.IN_PARAMS]
    assert {t["field"] for t in hot} == {n for n, _ in u.Params._fields_} - {"size", "channels", "sectors", "beam_width"}
    seen = set()
    for t in hot:
        f = t["field"]
        if t["type"] == u.PARAM_BOOL:
            want = [1 - int(t["default"])]
        elif t["type"] == u.PARAM_INT:
            want = [int(t["min"]), int(t["max"])]
        else:
            assert t["type"] == u.PARAM_DOUBLE
            want = [float(t["min"]), float(t["max"])]
        for v in want:
            hits = [n for n, tw in one.items() if tw == {f: v}]
            assert len(hits) == 1, (f, v)
            seen.add(hits[0])
    extra = set(one) - seen
    assert extra == {"xDirection 1", "angleFilter3 90", "curbPoints 8"}, extra     # (xDirection 0 and 2 are the row's ends)
    assert len(PE.CORNERS) == 48 and all(set(tw) == {t["field"] for t in hot} for _, tw in PE.CORNERS)
    for _, tw in PE.CORNERS:
        assert tw["min_Z"] in (-200, -3) and tw["max_Z"] in (-1, 200)
    assert set(PE.EMPTY_ROI) <= set(one) and set(PE.NEUTRAL) <= set(one)


def test_every_value_is_inside_the_box_or_outside_it_as_its_table_says():
    d = u.default_params()
    for table, inside in (("one", True), ("corner", True), ("outside", False)):
        for name, tw in PE.TABLES[table]:
            p = PE.params(d, tw)
            before = bytes(p)
            changed = u.clamp_params(p)
            if inside:
                assert changed == 0 and bytes(p) == before, name
            elif "beam_width" not in tw:    # (no cfg row: the reference's compile-time 0.2)
                assert changed == 1, name


def test_every_edge_changes_a_label_on_some_cloud():
    """A condition on the inputs, checked against B alone: a kernel that ignored an edge would not pass by accident."""
    silent = []
    for name, tw in PE.ONE_AT_A_TIME:
        differs = False
        for cname, (cloud, base) in clouds().items():
            if PE.is_base_value(base, tw):
                continue
            lb, ib, _ = run_b(cname, PE.params(base, tw))
            l0, i0, _ = run_b(cname, base)
            assert i0["status"] == 0 and i0["n_road"] > 0 and i0["n_curb"] > 0, cname
            differs = differs or not np.array_equal(lb, l0)
        if not differs:
            silent.append(name)
    by_construction = [n for n, tw in PE.ONE_AT_A_TIME if all(PE.is_base_value(b, tw) for _, b in clouds().values())]
    # the region's x and y are wide open in every base (wide_roi) and xDirection 0 is the default: those ends ARE the base
    assert sorted(by_construction) == sorted(["xDirection 0", "min_X -200", "max_X 200", "min_Y -200", "max_Y 200"])
    assert sorted(silent) == sorted(by_construction + list(PE.NEUTRAL)), silent


def test_an_empty_region_is_too_few_points_for_every_cloud():
    for name in PE.EMPTY_ROI:
        for cname, (cloud, base) in clouds().items():
            lb, ib, _ = run_b(cname, PE.params(base, PE.case("one", name)))
            assert ib["status"] == u.api.TOO_FEW_POINTS and ib["n_roi"] == 0 and not lb.any(), (name, cname)


def test_some_corners_keep_a_region():
    """Most corners invert the region of interest in x or y (status 1, also a case); these keep one."""
    alive = [name for name, tw in PE.CORNERS
             if all(run_b(c, PE.corner_params(tw, clouds()[c][1].channels))[1]["status"] == 0 for c in A_CLOUDS["corner"])]
    assert len(alive) >= 8, alive


@pytest.mark.parametrize("L,layout", PE.FUSED)
def test_fused_clouds_keep_a_ring_per_laser_and_hold_road_and_curb(L, layout):
    """What the GPU test's "all fused" assertion rests on, at the defaults."""
    p = PE.base_params(L)
    scans = PE.ideal_batch(L, layout)
    assert len(scans) == 2 and all(len(c[0]) == L * PE.FIRINGS for c in scans) and L * PE.FIRINGS >= 2 * 2048
    for c in scans:
        _, ib, _ = O.run_b(*c, p)
        assert ib["status"] == 0 and ib["n_rings"] == L and ib["n_road"] > 0 and ib["n_curb"] > 0, ib
    assert np.isnan(scans[1][0]).any()


@pytest.mark.parametrize("L,layout", PE.FUSED)
def test_a_ring_count_of_L_is_a_ring_per_laser_everywhere_in_the_box(L, layout):
    """The GPU test asserts the fused count where ring_per_laser holds; inside the box that is wherever B counts L rings (and at most
    edges: at least at the defaults and 30 others), so nothing is exempted there.  interval 0, outside the box, is the counter-example."""
    held = 0
    for table in ("one",):
        for name, tweak in PE.TABLES[table]:
            p = case_params(table, tweak, PE.base_params(L))
            for c in PE.ideal_batch(L, layout):
                _, ib, st = O.run_b(*c, p, debug=True)
                if ib["status"] == 0 and ib["n_rings"] == L:
                    assert PE.ring_per_laser(st, ib, L, layout), (name, L, layout)
                    held += 1
    assert held >= 2 * 31
    zero = [PE.ring_per_laser(*O.run_b(*c, PE.params(PE.base_params(L), {"interval": 0.0}), debug=True)[2:0:-1], L, layout)
            for c in PE.ideal_batch(L, layout)]
    assert layout == "firing" or not any(zero)


def test_real_sweeps_hold_road_and_curb():
    for m in PE.REAL:
        _, ib, _ = O.run_b(*PE.real_sweep(m), PE.base_params(SM.lasers(m)))
        assert ib["status"] == 0 and ib["n_rings"] == SM.lasers(m) and ib["n_road"] > 0 and ib["n_curb"] > 0, (m, ib)


def test_the_jitter_sweep_loses_ring_points_at_the_smallest_interval():
    """Range noise alone leaves n_ring_pts where it is at any interval; elevation jitter does not."""
    c, base = PE.jitter_sweep(), PE.base_params(64)
    lo = O.run_b(*c, PE.params(base, {"interval": 0.01}))[1]
    mid = O.run_b(*c, PE.params(base, {"interval": 0.18}))[1]
    assert lo["n_rings"] == mid["n_rings"] == 64
    assert 30 * 64 < lo["n_ring_pts"] < mid["n_ring_pts"] == len(c[0])
    assert lo["n_road"] > 0 and lo["n_curb"] > 0
    for m in PE.REAL:   # ... and the noisy sweeps: the same ring points at both
        a, b = (O.run_b(*PE.real_sweep(m), PE.params(PE.base_params(SM.lasers(m)), {"interval": iv}))[1] for iv in (0.01, 0.18))
        assert a["n_ring_pts"] == b["n_ring_pts"], m
