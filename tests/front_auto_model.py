"""The digest of urf_set_front_auto's learning pass on the CPU (TEST CODE): the fold k_front_digest makes of a call's per-scan records,
from tests/front_why_model.py's counters (oracle B's stages) and front_shape's fused / handed-back expectation.

digest(scans, params, layout, multi_sector=False) -> (scans, handed_back, scan_bits, helped, never, candidates, other): the words behind
the sequence number, for a call in front mode 2 that no speculation disturbs -- no repaired ring table (OTHER), no first sighting
(ROWS_SIGHTING: the records are counted in the layout the sweeps have), no overflowing candidate list.  A scan is handed back exactly
when it breaks a rule of the march: one of the four shape counters, rows that do not divide, and -- without the multi-sector march --
firings in several sectors or sectors that fall inside a tile.

fold(why, counted) is the same fold over urf_front_explain's records (tests/test_gpu_front_auto.py)."""
import numpy as np

import front_shape as FS
import front_why_model as WM
import urban_road_filter_amd as u

S = u.WHY_SCAN
NEVER = S["LANE_TWO_RINGS"] | S["RING_TWO_LANES"] | S["AXIS"] | S["RANGE"] | S["ROWS_LENGTH"]
HELPED = S["MULTI_SECTOR"] | S["SECTORS_FALL"]
WORDS = ("digest_scans", "digest_handed_back", "digest_scan_bits", "digest_helped", "digest_never", "digest_candidates", "digest_other")


def scan_bits(cloud, params, layout="firing", multi_sector=False):
    """(counted, URF_WHY_SCAN_* bits) of one scan under front mode 2"""
    if len(cloud[0]) == 0 or FS.stages(cloud, params)[1]["status"] != 0:
        return False, 0
    w = WM.counters(cloud, params, layout)
    bits = sum(S[name] for name, key in (("LANE_TWO_RINGS", "lanes_two_rings"), ("RING_TWO_LANES", "rings_two_lanes"), ("AXIS", "axis_points"),
                                         ("RANGE", "range_points")) if w[key])
    if layout == "rows" and len(cloud[0]) % int(params.channels) != 0:
        bits |= S["ROWS_LENGTH"]
    ms_march = multi_sector and bool(params.star_shaped_method) and params.curbPoints == 5
    if not ms_march:
        bits |= (S["MULTI_SECTOR"] if w["multi_sector_firings"] else 0) | (S["SECTORS_FALL"] if w["tiles_sectors_fall"] else 0)
    return True, bits


def _fold(rows):
    """rows: (counted, handed_back, bits) per scan"""
    back = [b for counted, hb, b in rows if counted and hb]
    return (sum(1 for counted, _, _ in rows if counted), len(back), int(np.bitwise_or.reduce(back)) if back else 0,
            sum(1 for b in back if b and not b & ~HELPED), sum(1 for b in back if b & NEVER), sum(1 for b in back if b & S["CANDIDATES"]),
            sum(1 for b in back if b & S["OTHER"]))


def digest(scans, params, layout="firing", multi_sector=False):
    rows = []
    for c in scans:
        counted, bits = scan_bits(c, params, layout, multi_sector)
        assert not counted or (bits & NEVER == 0) == FS.fusable(c, params, layout)   # (front_shape's predicate: the four shape rules and the rows' length)
        rows.append((counted, bits != 0, bits))
    return _fold(rows)


def fold(why, counted):
    """the same over urf_front_explain's records of a call that launched the fused kernels; counted[k]: scan k has a result"""
    return _fold([(bool(c), int(r["fused"]) == 0, int(r["scan"])) for r, c in zip(why, counted)])
