"""Marker-point sets for the road_marker line strips (tests/test_marker_strips_cpu.py, tests/test_gpu_marker_strips.py):
adversarial colourings and outlines, the sweep sequence that produces DELETE markers, and the glue between the library's
records (urf_marker_strip + packed float xyz) and oracle B's markers (tests/oracles.py)."""
import numpy as np

import oracles as O
import urban_road_filter_amd as u

MP_COMBOS = [(1, 1), (0, 0), (1, 0), (0, 1)]   # simple_poly_allow, poly_z_avg_allow
# tests/test_markers.py's SEQ keeps 5 strips in every sweep; the fifth sweep has 3 (2 DELETE markers), all under cfg_params("cfg2")
SEQ5 = [("cfg2", 1, 1), ("narrow", 2, 2), ("cfg2", 1, 3), ("narrow", 2, 4), ("sensor", 0, 1)]


def marker_params(simp, zavg, tol=None):
    mp = u.default_marker_params()   # (the library's structure; oracle_sequence hands oracle B the same bytes)
    mp.simple_poly_allow, mp.poly_z_avg_allow = simp, zavg
    if tol is not None:
        mp.poly_s_param = tol
    return mp


def outline(rng, k, kind):
    """k points x, y, z: one per degree like the reference's marker points, radius by `kind`."""
    deg = np.sort(rng.choice(361, k, replace=False)) if k else np.zeros(0, int)
    a = np.deg2rad(deg + rng.random(k))
    if kind == "smooth":      # a slowly varying outline: Douglas-Peucker drops most points
        r = 12 + 6 * np.sin(3 * a) + 0.2 * rng.random(k)
    elif kind == "jagged":    # everything farther than the tolerance: most points stay
        r = 3 + 25 * rng.random(k)
    elif kind == "grid":      # coordinates on a coarse grid: equal distances inside a span (the arg-max's tie rule), duplicates
        r = np.full(k, 10.0)
    else:                     # "line": collinear points, distance 0 everywhere
        r = np.full(k, 0.0)
    x, y = r * np.cos(a), r * np.sin(a)
    if kind == "grid":
        x, y = np.round(x / 2.5) * 2.5, np.round(y / 2.5) * 2.5
    if kind == "line":
        x, y = np.arange(k) * 0.25, np.arange(k) * 0.5
    z = -1.8 + 0.3 * rng.random(k)
    return np.stack([x, y, z], 1).astype(np.float32)


def colours(rng, k, kind):
    i = np.arange(k)
    if kind == "alternating":
        c = i % 2
    elif kind == "pairs":
        c = (i // 2) % 2
    elif kind == "pairs_red_first":
        c = 1 - (i // 2) % 2
    elif kind == "triples":
        c = (i // 3) % 2
    elif kind == "red":
        c = np.ones(k, int)
    elif kind == "green":
        c = np.zeros(k, int)
    elif kind == "singles":    # lone points of either colour inside long runs: the two fix-up passes
        c = (rng.random(k) < 0.5).astype(int) if k < 8 else np.repeat(rng.integers(0, 2, k // 4 + 1), 4)[:k]
        flip = rng.random(k) < 0.15
        c = np.where(flip, 1 - c, c)
    else:
        c = rng.integers(0, 2, k)
    return c.astype(np.float32)


COLOURINGS = ["alternating", "pairs", "pairs_red_first", "triples", "random", "red", "green", "singles"]
SIZES = [0, 1, 2, 3, 4, 5, 6, 360, 361]


def adversarial_sets(seed, n_random=40):
    """[(name, pts float32 [k, 4])]: every colouring at every fixed size, then random sizes; outlines cycle."""
    rng = np.random.default_rng(seed)
    kinds = ["smooth", "jagged", "grid", "line"]
    sets = []
    for ci, col in enumerate(COLOURINGS):
        for si, k in enumerate(SIZES):
            sets.append(("%s/%d" % (col, k), k, col, kinds[(ci + si) % 4]))
    for j in range(n_random):
        col = COLOURINGS[int(rng.integers(len(COLOURINGS)))]
        sets.append(("%s/r%d" % (col, j), int(rng.integers(0, 362)), col, kinds[j % 4]))
    out = []
    for name, k, col, kind in sets:
        out.append((name + "/" + kind, np.concatenate([outline(rng, k, kind), colours(rng, k, col)[:, None]], 1).astype(np.float32)))
    order = rng.permutation(len(out))   # sizes mixed: unpublished sets between publishing ones, strip counts up and down
    return [out[i] for i in order]


def as_markers(published, strips, xyz):
    """The library's records in the form oracles.markers_equal compares: floats widened to double, type LINE_STRIP."""
    if not published:
        return None
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    return [{"id": int(s["id"]), "action": int(s["action"]), "type": 4, "color": (float(s["r"]), float(s["g"]), float(s["b"]), float(s["a"])),
             "points": xyz[int(s["first_point"]):int(s["first_point"]) + int(s["n_points"])].astype(np.float64)} for s in strips]


def host_sequence(sets, mp, ghost=0, sequence=True):
    """urf_marker_strips over the sets; returns ([(published, strips, xyz)], [ghost after every set])."""
    res, ghosts = [], []
    for pts in sets:
        pub, strips, xyz, g = u.marker_strips(pts, mp, ghost if sequence else 0)
        ghost = g if sequence else ghost
        res.append((pub, strips.copy(), xyz.copy()))
        ghosts.append(g)
    return res, ghosts


def oracle_sequence(sets, mp, ghost=0, sequence=True):
    """Oracle B over the sets with ONE state (sequence) or a fresh one per set; returns (markers, ghost counts, line_n)."""
    mp = O.MarkerParams.from_buffer_copy(bytes(mp))
    st = O.OracleMarkerState()
    st.ghostcount = ghost
    res, ghosts, carried = [], [], []
    for pts in sets:
        if not sequence:
            st = O.OracleMarkerState()
        res.append(O.marker_strips_b(pts, mp, st))
        ghosts.append(int(st.ghostcount))
        carried.append(int(st.line_n))
    return res, ghosts, carried


def seq_marker_points(seq=SEQ5, params=None):
    """Oracle B's marker points of the sweeps of `seq` (all classified under cfg_params("cfg2"))."""
    p = params or O.cfg_params("cfg2")
    out = []
    for cfg, _, seed in seq:
        x, y, z = O.cfg_cloud(cfg, seed)
        out.append(O.run_b(x, y, z, p, debug=True)[2]["marker_pts"])
    return out
