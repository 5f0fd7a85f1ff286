"""Inputs of tests/test_gpu_front_sectors.py, built on the CPU (TEST CODE): the small organised sweeps of the suite at star-sector counts
other than 360, and the predicate that says which of them the plain fused kernels keep at a given count.

params.sectors (K) is 1..1022.  What of a sweep depends on it: the sector of every participant of the star-shaped search, hence whether a
firing's participants share one sector (the plain march needs that) and whether a tile of 2048 points meets a smaller sector after a larger
one (the plain march hands such a scan back).  `clean` is tests/test_history_cpu.firings_astride generalised to K, plus the seam rule and
front_shape.fusable; tests/test_front_sectors_cpu.py pins its value for every (shape, K) used on the GPU.

urf_synth_cloud places firing c at (c + 0.5) * 360 / cols degrees: never on a sector border at K = 360, and at none of 90, 720 and 1022
either for the column counts below -- but for 32 x 136 at K = 720, where firing 8 lies on 22.5 degrees, the border of sectors 44 and 45
(and firing 8 + 17 j on a further one).  Oracle B's sector stage decides what that means for the two sweeps used here: the float
azimuths of such a firing's participants all round to the same side, no firing is astride, and the shape stays a clean one at every K
(pinned in the CPU file; an expected count is always sum(clean(...)), so a sweep that were astride would be expected as handed back)."""
import numpy as np

import front_shape as FS
import urban_road_filter_amd as u

KS = (1, 90, 720, 1022)
SHAPES = ((64, 96), (64, 256), (32, 136), (32, 256), (16, 304), (16, 512), (128, 48), (128, 64))
ON_A_BORDER = (32, 136, 720, 8)   # (lasers, cols, K, firing): nominal azimuth on a sector border
# Seeds of the fuzz: FUZZ_BASE + 1000 * L + seed, a base of its own.  Chosen on the CPU (the first of 9_300_000 + 100_000 j) so that at
# every (L, K) some sweep in FIRING order passes front_shape.fusable -- a lone row-major sweep is fused from its context's third call on,
# the fuzz makes two -- and so that no fusable sweep at K = 1 has more than 16 500 participants: the fused star search of ONE sector costs
# time with the square of its participants (seconds at 45 000), and every case has to stay quick.  tests/test_front_sectors_cpu.py pins both.
FUZZ_BASE = 13_700_000
FUZZ_K1_PARTICIPANTS = 16_500
_SWEEPS = {}


def at_k(p, K):
    q = p.copy()
    q.sectors = K
    return q


def plain_params(L, K=360, **tweak):
    """Wide region of interest, all three detectors, curbPoints 5; 128 lasers at interval 0.05 (rings of their own)."""
    p = u.default_params().wide_roi()
    p.channels = L
    if L == 128:
        p.interval = 0.05
    p.sectors = K
    for k, v in tweak.items():
        setattr(p, k, v)
    return p


def plain_sweeps(L, cols):
    """Two sweeps in firing order, built once and read only: the analytic street (scene 1), and a sensor-like one (scene 3: range noise,
    2 mm range steps -- planar-range ties inside a sector --, drop-outs)."""
    if (L, cols) not in _SWEEPS:
        _SWEEPS[L, cols] = [u.synth_cloud(L, cols, 1, 3 + L + cols), u.synth_cloud(L, cols, 3, 4 + L + cols)]
    return _SWEEPS[L, cols]


def rows_of(c, L):
    return tuple(np.ascontiguousarray(a.reshape(-1, L).T.reshape(-1)) for a in c)


def rows_sweeps(L, cols):
    if (L, cols, "rows") not in _SWEEPS:
        _SWEEPS[L, cols, "rows"] = [rows_of(c, L) for c in plain_sweeps(L, cols)]
    return _SWEEPS[L, cols, "rows"]


def clean(cloud, p, layout="firing"):
    """What the plain fused kernels (urf_set_front_multi_sector off) keep of a sweep with the star-shaped search on: front_shape.fusable,
    no firing with participants in two sectors, no tile in which a sector is followed by a smaller one.  Without the star-shaped search
    sectors do not matter."""
    if not FS.fusable(cloud, p, layout):
        return False
    if not p.star_shaped_method or FS.stages(cloud, p)[1]["status"] != 0:
        return True
    return FS.multi_sector_firings(cloud, p, layout)[0] == 0 and FS.tiles_where_sectors_fall(cloud, p, layout) == 0


def widest_firing(cloud, p, layout="firing"):
    """The largest extent of one firing's participants in sectors (last - first + 1, around the circle the short way): what the tables of
    k_front_sectors see of an azimuth offset of +- 2.4 degrees at K = 720 (ten sectors) that they do not at 360 (five)."""
    K = int(p.sectors)
    best = 0
    for row in FS._sectors(cloud, p, layout):
        k = np.unique(row[row >= 0]).astype(np.int64)
        if len(k) > 1:
            gaps = np.diff(np.concatenate([k, [k[0] + K]]))
            best = max(best, int(K - gaps.max() + 1))
        elif len(k) == 1:
            best = max(best, 1)
    return best


def fuzz_case(seed, L):
    """sensor_models.fuzz_case with the sector count drawn by the seed: (1, 90, 720, 1022)[seed % 4]."""
    import sensor_models as SM
    cloud, p, model = SM.fuzz_case(FUZZ_BASE + 1000 * L + seed, L)
    p.sectors = KS[seed % 4]
    return cloud, p, model
