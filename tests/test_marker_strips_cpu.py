"""road_marker's line strips on the host: urf_marker_strips (the C view of urf::MarkerBuilder's implementation) against
oracle B (urf_oracle_marker_strips), exactly; the derived bounds of include/urf.h; the record layout."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import marker_sets as M
import oracles as O
import urban_road_filter_amd as u

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check_sequence(sets, mp, ghost=0):
    got, g_got = M.host_sequence(sets, mp, ghost)
    want, g_want, carried = M.oracle_sequence(sets, mp, ghost)
    for k, pts in enumerate(sets):
        pub, strips, xyz = got[k]
        assert O.markers_equal(M.as_markers(pub, strips, xyz), want[k]), "set %d (%d points)" % (k, len(pts))
        assert g_got[k] == g_want[k], "ghost count after set %d" % k
        assert carried[k] == 0, "oracle B carried strip points out of set %d: the state is more than the ghost count" % k
        assert len(strips) <= u.MARKER_MAX_STRIPS and len(xyz) <= u.MARKER_MAX_STRIP_POINTS
        if pub:   # first_point ascending in marker order, the points packed
            assert int(strips["n_points"].sum()) == len(xyz)
            assert np.array_equal(strips["first_point"], np.concatenate([[0], np.cumsum(strips["n_points"])[:-1]]))
    return got


@pytest.mark.parametrize("simp,zavg", M.MP_COMBOS)
def test_sweep_sequence_equals_oracle_b(simp, zavg):
    sets = M.seq_marker_points()
    got = check_sequence(sets, M.marker_params(simp, zavg))
    n_add = [int((s["action"] == u.MARKER_ADD).sum()) for _, s, _ in got]
    n_del = [int((s["action"] == u.MARKER_DELETE).sum()) for _, s, _ in got]
    assert n_add == [5, 5, 5, 5, 3] and n_del == [0, 0, 0, 0, 2]   # oracle B's counts for these sweeps: the drop to 3 strips is what makes DELETE markers


@pytest.mark.parametrize("simp,zavg", M.MP_COMBOS)
@pytest.mark.parametrize("seed", [1, 2])
def test_adversarial_sets_equal_oracle_b(simp, zavg, seed):
    sets = [p for _, p in M.adversarial_sets(seed)]
    got = check_sequence(sets, M.marker_params(simp, zavg), ghost=7)
    assert any((s["action"] == u.MARKER_DELETE).any() for _, s, _ in got)
    assert any(not pub for pub, _, _ in got) and sum(pub for pub, _, _ in got) > 50


@pytest.mark.parametrize("tol", [0.0, 0.05, 3.0, 1e9, -1.0, float("nan")])
def test_tolerances(tol):
    sets = [p for _, p in M.adversarial_sets(3, n_random=10)]
    check_sequence(sets, M.marker_params(1, 0, tol))


def test_bounds_are_reached_and_never_exceeded():
    """After the fix-ups every run has two points or more: 361 points give at most 180 strips, and 361 + 179 strip points
    (every joint twice) when nothing is simplified away.  Runs of 2, 2, ..., 2, 3 reach both."""
    rng = np.random.default_rng(5)
    k = u.MARKER_MAX_POINTS
    c = (np.arange(k) // 2) % 2
    c[-1] = c[-2]
    pts = np.concatenate([M.outline(rng, k, "jagged"), c[:, None]], 1).astype(np.float32)
    pub, strips, xyz, ghost = u.marker_strips(pts, M.marker_params(0, 0), 0)
    assert pub and len(strips) == u.MARKER_MAX_STRIPS == 180 and len(xyz) == u.MARKER_MAX_STRIP_POINTS == 540
    assert ghost == u.MARKER_MAX_STRIPS - 1
    # ADD + DELETE markers: a sweep with one strip after the fullest one
    pub, strips, xyz, g2 = u.marker_strips(pts[:3] * [1, 1, 1, 0], M.marker_params(0, 0), ghost)
    assert pub and len(strips) == u.MARKER_MAX_STRIPS and g2 == 0
    assert strips["id"].tolist() == list(range(180)) and strips["action"].tolist() == [0] + [2] * 179
    # an incoming count beyond what a sweep can leave is clamped: the records still fit
    for g_in, want in [(10 ** 6, 180), (180, 180), (179, 180), (-5, 1)]:
        pub, strips, _, _ = u.marker_strips(pts[:3] * [1, 1, 1, 0], M.marker_params(0, 0), g_in)
        assert len(strips) == want
    # random colourings of full sweeps stay inside
    for seed in range(200):
        r = np.random.default_rng(seed)
        cc = M.colours(r, k, M.COLOURINGS[seed % len(M.COLOURINGS)])
        pub, strips, xyz, _ = u.marker_strips(np.concatenate([pts[:, :3], cc[:, None]], 1), M.marker_params(seed % 2, 0), seed % 180)
        assert len(strips) <= 180 and len(xyz) <= 540


def test_argument_checks():
    mp = M.marker_params(1, 1)
    with pytest.raises(u.UrfError):
        u.marker_strips(np.zeros((362, 4), np.float32), mp, 0)
    bad = np.zeros((5, 4), np.float32)
    bad[2, 3] = 0.5
    with pytest.raises(u.UrfError):
        u.marker_strips(bad, mp, 0)
    for g_in in (10 ** 6, -5):   # ... as it came, out of range or not
        assert u.marker_strips(np.zeros((2, 4), np.float32), mp, g_in)[3] == g_in
    pub, strips, xyz, g = u.marker_strips(np.zeros((2, 4), np.float32), mp, 4)   # unpublished: the count passes through
    assert not pub and len(strips) == 0 and len(xyz) == 0 and g == 4


def test_record_layout(tmp_path):
    assert C.sizeof(u.MarkerStrip) == 32 and u.MARKER_STRIP_DTYPE.itemsize == 32
    for name, off in [("id", 0), ("action", 4), ("r", 8), ("g", 12), ("b", 16), ("a", 20), ("first_point", 24), ("n_points", 28)]:
        assert getattr(u.MarkerStrip, name).offset == off == u.MARKER_STRIP_DTYPE.fields[name][1]
    cc = shutil.which("cc") or shutil.which("gcc")
    if not cc:
        pytest.skip("no C compiler")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "urf.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d\\n", '
                   "sizeof(urf_marker_strip), offsetof(urf_marker_strip, id), offsetof(urf_marker_strip, action), offsetof(urf_marker_strip, r), "
                   "offsetof(urf_marker_strip, g), offsetof(urf_marker_strip, b), offsetof(urf_marker_strip, a), "
                   "offsetof(urf_marker_strip, first_point), offsetof(urf_marker_strip, n_points), URF_MARKER_MAX_POINTS, URF_MARKER_MAX_STRIPS, "
                   "URF_MARKER_MAX_STRIP_POINTS, URF_MARKER_ADD, URF_MARKER_DELETE); return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [32, 0, 4, 8, 12, 16, 20, 24, 28, u.MARKER_MAX_POINTS, u.MARKER_MAX_STRIPS, u.MARKER_MAX_STRIP_POINTS,
                                     u.MARKER_ADD, u.MARKER_DELETE]


def test_batch_marker_client_builds_against_the_product_library(tmp_path):
    """tests/cpp/batch_marker_demo.cpp (urf::BatchDetector::road_marker next to urf::Detector's) compiles with g++ and needs nothing the
    product library does not export; tests/test_gpu_marker_strips.py runs it."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    u.lib()
    pkg = os.path.join(ROOT, "urban_road_filter_amd")
    exe = str(tmp_path / "batch_marker_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(pkg, "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "batch_marker_demo.cpp"), "-o", exe,
                           "-L" + pkg, "-l:liburf_hip.so", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"])
    undefined = subprocess.run(["nm", "-u", exe], capture_output=True, text=True).stdout.split()
    wanted = {w.split("@")[0] for w in undefined if "urf" in w}
    exported = set(subprocess.run(["nm", "-D", "--defined-only", u.lib_path()], capture_output=True, text=True).stdout.split())
    assert wanted and wanted <= exported, wanted - exported
