"""urf_set_front_multi_sector_curb_points, the CPU side: the sweeps of tests/test_gpu_front_multi_cp.py are what they are used for at
every curbPoints 1..8, pinned from oracle B's stages (tests/front_shape.py).  Each of them has a result with road and curb, is fusable but
for its sectors, has firings in several star sectors (the seam sweeps: a seam inside a tile as well) -- and its labels at curbPoints 5
differ from those at every other value, so a kernel that ran with the wrong window would not pass there.  The real sensors' batches
(tests/gpu_sensor_cases.py) at curbPoints 3 and 8: every sweep fusable, road and curb in every batch's sweeps."""
import numpy as np
import pytest

import front_shape as FS
import gpu_sensor_cases as G
from test_front_multi_cpu import batch, layout, ragged_scans, seam_sweeps, small_models, small_params, small_sweeps

NAMES = sorted(small_models())
CURB_POINTS = (1, 2, 3, 4, 5, 6, 7, 8)
OTHERS = tuple(cp for cp in CURB_POINTS if cp != 5)


def params_at(name, cp):
    p = small_params(name)
    p.curbPoints = cp
    return p


def sweeps_under_test(name):
    """(kind, sweep): the ragged scans are sweeps of the 64-laser model"""
    return ([("small", c) for c in small_sweeps(name)] + [("seam", c) for c in seam_sweeps(name)] +
            ([("ragged", c) for c in ragged_scans()] if name == "64 offsets" else []))


@pytest.mark.parametrize("name", NAMES)
def test_the_sweeps_have_their_properties_at_every_curb_points(name):
    for kind, c in sweeps_under_test(name):
        labels, found = {}, []
        for cp in CURB_POINTS:
            p = params_at(name, cp)
            lb, ib, _ = FS.stages(c, p)
            assert ib["status"] == 0 and ib["n_road"] > 0 and ib["n_curb"] > 0, (kind, cp, ib)
            assert FS.fusable(c, p), (kind, cp)
            assert FS.multi_sector_firings(c, p)[0] > 0, (kind, cp)
            if kind == "seam":
                assert FS.tiles_where_sectors_fall(c, p) >= 1, cp
            labels[cp] = lb
            found.append("%d / %d" % (ib["n_road"], ib["n_curb"]))
        print("%s %s: road / curb at curbPoints 1..8: %s" % (name, kind, ", ".join(found)))
        for cp in OTHERS:
            assert not np.array_equal(labels[cp], labels[5]), (kind, cp)   # (the parameter matters on this input)


@pytest.mark.parametrize("cp", (3, 8))
@pytest.mark.parametrize("model", G.REAL)
def test_the_real_batches_are_fusable_with_road_and_curb(model, cp):
    p = G.params(model, "default")
    p.curbPoints = cp
    assert [FS.fusable(c, p, layout(model)) for c in batch(model)] == [True] * 4
    for c in batch(model):
        ib = FS.stages(c, p)[1]
        assert ib["status"] == 0 and ib["n_road"] > 0 and ib["n_curb"] > 0, ib
