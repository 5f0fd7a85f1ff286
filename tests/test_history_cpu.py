"""tests/fuzz_history.py on the CPU, over exactly the seeds tests/test_gpu_history.py runs: the scripts are reproducible, oracle B finds road
and curb on every organised pool entry under every parameter set of its laser count (no comparison passes on an empty result), and the
scripts hold what the GPU test is there for -- every kind of step, every setter with every value, every entry point, every ordered pair of
call classes as neighbours, every ordered pair of laser counts as consecutive urf_set_params, and enough anchor steps (batch calls whose
path the settings alone decide).  A condition that fails is a reason to change the generator's weights or add seeds."""
import collections

import pytest

import fuzz_history as H
import oracles as O


def scripts():
    return [(f, s, H.script(s, f)) for f in ("small", "long") for s in H.SEEDS[f]]


@pytest.fixture(scope="module")
def all_scripts():
    return scripts()


def test_the_same_seed_gives_the_same_script(all_scripts):
    for (f, s, steps), (_, _, again) in zip(all_scripts, scripts()):
        assert steps == again, (f, s)
        assert len(steps) == H.STEPS[f]
    assert H.script(0, "small") != H.script(1, "small")
    assert (len(H.SEEDS["small"]), H.STEPS["small"], len(H.SEEDS["long"]), H.STEPS["long"]) == (12, 48, 3, 24)


@pytest.mark.parametrize("family", ["small", "long"])
def test_oracle_b_finds_road_and_curb_on_every_organised_entry(family):
    n = 0
    for e in H.organised(family):
        for tag, p in H.param_pool(family).items():
            if H.tag_lasers(tag) != e.lasers or not (p.star_shaped_method or (p.x_zero_method and p.z_zero_method)):
                continue
            _, ib, _ = O.run_b(*e.cloud, p)
            assert ib["status"] == 0 and ib["n_road"] > 0 and ib["n_curb"] > 0, (e.name, tag, ib)
            n += 1
    assert n >= (9 * 8 + 8 * 8 + 2 * 16 * 8 if family == "small" else 13 * 4)


def firings_astride(e, tag):
    """The firings of a sweep whose participants of the star-shaped search (oracle B's sector stage) lie in more than one sector."""
    x, y, z = e.cloud
    if e.kind in ("rows", "astride_rows"):
        x, y, z = (a.reshape(e.lasers, -1).T.reshape(-1) for a in (x, y, z))
    _, _, st = O.run_b(x, y, z, H.params_of("small", tag), debug=True)
    sec = st["sector"].reshape(-1, e.lasers)
    return [f for f, row in enumerate(sec) if len(set(row[row >= 0].tolist())) > 1]


def test_one_sector_per_firing_is_what_tells_the_astride_entries_from_the_others():
    """What k_front needs of a scan's firings, on the CPU: the "firing" and "rows" entries have it under every parameter set of their laser
    count with the star-shaped search on, every "astride" entry has a firing that does not (so the path assertions of the GPU test know
    which scans the fused kernels keep without asking them)."""
    for e in H.organised("small"):
        if e.kind == "cut":
            continue
        for tag, p in H.param_pool("small").items():
            if H.tag_lasers(tag) != e.lasers or not p.star_shaped_method:
                continue
            bad = firings_astride(e, tag)
            assert bool(bad) == e.kind.startswith("astride"), (e.name, tag, bad)


def test_pool_shapes():
    for family, (max_points, _) in H.FAMILIES.items():
        E = H.pool(family)
        for e in H.organised(family):
            assert len(e) > H.TILE, e.name                                  # at least two tiles
            if e.lasers in (16, 32) or e.kind == "cut":                      # ... the last one partial (64 x 96, 128 x 48: three whole tiles, 64 x 4128: 129)
                assert len(e) % H.TILE != 0, e.name
        assert {e.kind for e in E.values()} == {"firing", "cut", "rows", "unorganised"} | ({"astride", "astride_rows"} if family == "small" else set())
        for L in H.LASERS["small"] if family == "small" else (64,):           # every laser count has sweeps the fused kernels keep
            assert sum(e.kind == "firing" and e.lasers == L for e in E.values()) >= 4 and sum(e.kind == "rows" and e.lasers == L for e in E.values()) >= 4
        assert max(len(e) for e in E.values()) <= max_points
        assert sum(e.kind == "unorganised" for e in E.values()) == 6
    assert -(-len(H.pool("long")["F64s1"]) // H.TILE) == 129 and -(-len(H.pool("long")["f64s1"]) // H.TILE) == 3


def test_every_kind_of_step_occurs(all_scripts):
    count = collections.Counter()
    for f, s, steps in all_scripts:
        for st in steps:
            op = st["op"]
            count[op] += 1
            if op == "batch":
                count["entry", st["entry"]] += 1
                count["info", st["info"]] += 1
            elif op == "callback":
                count["how", st["how"]] += 1
            elif op == "readout":
                for what, _ in st["what"]:
                    count["what", what] += 1
            elif op == "callback_path_preset":
                for b in H.PRESET_BITS:
                    if st["value"] & b:
                        count[op, b] += 1
            elif op != "set_params":
                count[op, st["value"]] += 1
    want = (["batch", "callback", "readout", "set_params"] + [("entry", e) for e in H.ENTRY_POINTS] + [("info", True), ("info", False)] +
            [("how", h) for h in ("xyz", "async16", "async32")] + [("what", k) for k in H.READOUTS] +
            [("set_front_mode", m) for m in H.MODES] + [("callback_path_preset", b) for b in H.PRESET_BITS] +
            [(op, v) for op in ("set_front_lasers128", "set_front_long_sweeps", "set_front_outputs") for v in (0, 1)] +
            [("enable_stage_capture", 0), ("enable_stage_capture", 2)])
    short = {k: count[k] for k in want if count[k] < 5}
    assert not short, short


def test_every_ordered_pair_of_call_classes_occurs_as_neighbours(all_scripts):
    seen = set()
    for f, s, steps in all_scripts:
        cls = [H.step_class(f, st) for st in steps]
        seen |= set(zip(cls, cls[1:]))
    missing = [(a, b) for a in H.CLASSES for b in H.CLASSES if (a, b) not in seen]
    assert not missing, missing


def test_every_ordered_pair_of_laser_counts_occurs_as_consecutive_set_params(all_scripts):
    seen = set()
    for f, s, steps in all_scripts:
        L = [H.tag_lasers(st["params"]) for st in steps if st["op"] == "set_params"]
        seen |= set(zip(L, L[1:]))
    missing = [(a, b) for a in (16, 32, 64, 128) for b in (16, 32, 64, 128) if (a, b) not in seen]
    assert not missing, missing


def test_a_quarter_of_the_batch_steps_are_anchor_steps(all_scripts):
    """An anchor step is one where tests/test_gpu_history.py asserts urf_front_scans() == n_scans: Shadow.expect says n_scans.  A quarter of
    the batch steps of either family, and at every laser count a share of them."""
    for family in ("small", "long"):
        batches = anchors = certain_zero = repeats = 0
        by_lasers = collections.Counter()
        for f, s, steps in all_scripts:
            if f != family:
                continue
            for step, cls, expect, anchor in H.replay(f, steps):
                if step["op"] == "batch":
                    batches += 1
                    assert not anchor or expect == len(step["scans"]), (f, s, step)
                    anchors += anchor
                    by_lasers[H.pool(f)[step["scans"][0]].lasers] += anchor
                    certain_zero += expect == 0
                    repeats += bool(step.get("repeat") and expect == len(step["scans"]))
        assert 4 * anchors >= batches, (family, anchors, batches)
        if family == "small":
            assert min(by_lasers[L] for L in (16, 32, 64, 128)) >= 4, by_lasers
            assert certain_zero >= 20 and repeats >= 5, (certain_zero, repeats)   # the path assertions' other two kinds are there too
        else:
            assert certain_zero >= 3 and repeats >= 2, (certain_zero, repeats)


def test_the_long_scripts_move_the_fused_path_between_129_and_3_tiles(all_scripts):
    """Every script of family "long" holds anchor steps of 129 tiles and anchor steps of 3 tiles (both fully fused, asserted on the GPU), and
    over the family they follow one another in both directions with no other anchor step in between."""
    moves = set()
    for f, s, steps in all_scripts:
        if f != "long":
            continue
        tiles = [-(-max(len(H.pool(f)[n]) for n in step["scans"]) // H.TILE) for step, cls, expect, anchor in H.replay(f, steps) if anchor]
        assert tiles.count(129) >= 2 and tiles.count(3) >= 2, (s, tiles)
        moves |= set(zip(tiles, tiles[1:]))
    assert {(129, 3), (3, 129)} <= moves, moves


def test_the_astride_entries_are_drawn_under_their_own_laser_count(all_scripts):
    """... in firing order and row-major, alone and next to sweeps the fused kernels keep (a count of fused scans below n_scans, asserted)."""
    count = collections.Counter()
    for f, s, steps in all_scripts:
        sh = H.Shadow(f)
        for step in steps:
            if step["op"] == "batch":
                kinds = [H.pool(f)[n].kind for n in step["scans"] if H.pool(f)[n].lasers == sh.lasers]
                count["firing"] += "astride" in kinds
                count["rows"] += "astride_rows" in kinds
                e = sh.expect(step)
                count["some fused"] += "astride" in kinds and e is not None and 0 < e < len(step["scans"])
                count["none fused"] += "astride" in kinds and e == 0 and not sh.excluded(sh.tiles(step))
                sh.call(step)
            elif step["op"] == "callback":
                sh.call(step)
            elif step["op"] == "readout":
                sh.readout(step)
            else:
                sh.setting(step)
    assert count["firing"] >= 5 and count["rows"] >= 5 and count["some fused"] >= 2 and count["none fused"] >= 2, count
