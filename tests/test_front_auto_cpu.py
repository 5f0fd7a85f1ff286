"""The digest of urf_set_front_auto's learning pass, pinned on the CPU: tests/front_auto_model.py (front_why_model's counters folded the way
k_front_digest folds the records) on the small sweeps and the sensor models' batches that tests/test_gpu_front_auto.py asks the device
about -- and what urf_policy::auto_digest's rule makes of each (tests/cpp/policy_auto.cpp has the rule itself).

The words, in urf_front_auto_info's order behind the sequence number: (scans with a result, handed back, OR of their scan bits, helped by
the multi-sector march, with a reason no setting lifts, CANDIDATES, OTHER), without and with urf_set_front_multi_sector."""
import pytest

import front_auto_model as AM
import gpu_sensor_cases as G
import sensor_models as SM
import urban_road_filter_amd as u
from test_front_why_cpu import MODELS, SMALL, model_scans, small_cases

S = u.WHY_SCAN
MS, FALL = S["MULTI_SECTOR"], S["SECTORS_FALL"]
CLEAN = (1, 0, 0, 0, 0, 0, 0)
# name -> (switch off, switch on)
SMALL_DIGESTS = {
    "128 stagger": ((1, 1, MS | FALL, 1, 0, 0, 0), CLEAN),
    "16 x 300": ((1, 1, MS | FALL, 1, 0, 0, 0), CLEAN),
    "32 x 130": ((1, 1, MS | FALL, 1, 0, 0, 0), CLEAN),
    "64 offsets, beam filter": ((1, 1, MS | FALL, 1, 0, 0, 0), CLEAN),
    "64 offsets, no star search": (CLEAN, CLEAN),
    "ends inside a firing": ((1, 1, MS | FALL, 1, 0, 0, 0), CLEAN),
    "ideal16": (CLEAN, CLEAN),
    "ideal16 from 77.7": ((1, 1, FALL, 1, 0, 0, 0), CLEAN),
    "ideal16 rows": (CLEAN, CLEAN),
    "ideal64 x 64": (CLEAN, CLEAN),
    "interval 1.5": ((1, 1, S["RING_TWO_LANES"], 0, 1, 0, 0),) * 2,
    "lifted": ((1, 1, S["LANE_TWO_RINGS"] | S["RING_TWO_LANES"], 0, 1, 0, 0),) * 2,
    "on the axis": ((1, 1, S["RANGE"] | MS | FALL, 0, 1, 0, 0), (1, 1, S["RANGE"], 0, 1, 0, 0)),
}
MODEL_DIGESTS = {
    ("vlp16", "default"): ((4, 3, MS | FALL, 3, 0, 0, 0), (4, 0, 0, 0, 0, 0, 0)),
    ("vlp16", "interval 0.5"): ((4, 3, MS | FALL, 3, 0, 0, 0), (4, 0, 0, 0, 0, 0, 0)),
    ("hdl64e", "default"): ((4, 3, MS | FALL, 3, 0, 0, 0), (4, 0, 0, 0, 0, 0, 0)),
    ("hdl64e", "interval 0.5"): ((4, 4, 3 | MS | FALL, 0, 4, 0, 0), (4, 4, 3, 0, 4, 0, 0)),
    ("os64", "default"): ((4, 3, MS | FALL, 3, 0, 0, 0), (4, 0, 0, 0, 0, 0, 0)),
    ("os64", "interval 0.5"): ((4, 4, S["RING_TWO_LANES"] | MS | FALL, 3, 1, 0, 0), (4, 1, S["RING_TWO_LANES"], 0, 1, 0, 0)),
    ("os128d", "default"): ((4, 2, S["RING_TWO_LANES"] | FALL, 1, 1, 0, 0), (4, 1, S["RING_TWO_LANES"], 0, 1, 0, 0)),
    ("os128d", "interval 0.5"): ((4, 4, S["RING_TWO_LANES"] | FALL, 0, 4, 0, 0), (4, 4, S["RING_TWO_LANES"], 0, 4, 0, 0)),
}


def test_the_cases_are_the_suites_own():
    assert sorted(SMALL_DIGESTS) == sorted(SMALL) and sorted(MODEL_DIGESTS) == sorted(MODELS)


@pytest.mark.parametrize("name", sorted(SMALL_DIGESTS))
def test_small_sweeps(name):
    c, p, layout = small_cases()[name]
    assert (AM.digest([c], p, layout), AM.digest([c], p, layout, True)) == SMALL_DIGESTS[name]


@pytest.mark.parametrize("model,setting", sorted(MODEL_DIGESTS))
def test_the_models_batches(model, setting):
    p, layout = G.params(model, setting), SM.MODELS[model]["layout"]
    off, on = AM.digest(model_scans(model), p, layout), AM.digest(model_scans(model), p, layout, True)
    assert (off, on) == MODEL_DIGESTS[(model, setting)]
    # the rule's reading: something helped -> the switch, then a digest that settles (clean, or only reasons no setting lifts)
    assert on[1] == off[1] - off[3]   # (the switch keeps exactly the scans counted as helped)
    assert on[1] == 0 or on[4] + on[5] == on[1]


def test_a_scan_without_a_result_counts_nowhere():
    a, p, _ = small_cases()["ideal16"]
    few = tuple(v[:20].copy() for v in a)
    empty = tuple(v[:0].copy() for v in a)
    assert AM.digest([few, empty, a], p) == CLEAN
    rows = tuple(v[:-1].copy() for v in small_cases()["ideal16 rows"][0])
    assert AM.digest([rows], p, "rows") == (1, 1, S["ROWS_LENGTH"], 0, 1, 0, 0)
