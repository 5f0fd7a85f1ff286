"""Oracle B against the golden label vectors of 32- and 16-laser sweeps (tests/golden/lasers/, produced from oracle A -- the
reference's own sources -- by tests/golden/make_golden_lasers.py), params.channels = the laser count."""
import os

import numpy as np
import pytest

import oracles as O
from golden.make_golden import cloud_sha
from golden.make_golden_lasers import CASES, OUT, case_cloud, case_params


@pytest.mark.parametrize("name,lasers,cols,scene,seed", CASES, ids=[c[0] for c in CASES])
def test_oracle_b_equals_golden(name, lasers, cols, scene, seed):
    g = np.load(os.path.join(OUT, name + ".npz"))
    p = case_params(lasers)
    assert bytes(p) == g["params"].tobytes()
    x, y, z = case_cloud(lasers, cols, scene, seed)
    assert cloud_sha(x, y, z) == str(g["cloud_sha"]), "synthetic generator drifted"
    lb, ib, _ = O.run_b(x, y, z, p)
    assert ib["n_road"] > 0 and ib["n_curb"] > 0 and ib["n_rings"] == lasers
    assert np.array_equal(lb & O.MASK_NO_RING, g["labels"])
    for k in ("status", "n_roi", "n_road", "n_curb", "n_ring10"):
        assert ib[k] == int(g["info_" + k]), k
