"""The premise of urf_classify_batch_*_dense (include/urf.h), on the CPU against oracle B: a dense sweep put back into firing slots by
the rule of tests/dense_model.py -- with NaN holes, W = F + 3 -- gets the labels (at the kept points) and the summary counts of the
dense sweep itself, and of the sweep with its holes in place; with random ids as well as with the right ones."""
import numpy as np
import pytest

import dense_model as D
import oracles as O
import sensor_models as SM

CASES = {
    "vlp16": dict(firings=304, noise=True, drop=0.10),
    "hdl32e": dict(firings=136, drop=0.01),
    "ideal64": dict(firings=256, drop=0.30),
}


@pytest.mark.parametrize("wide", [True, False])
@pytest.mark.parametrize("model", sorted(CASES))
def test_the_realigned_sweep_is_classified_as_the_dense_one(model, wide):
    kw = CASES[model]
    L, F = SM.lasers(model), kw["firings"]
    cloud = SM.sweep(model, seed=11, **kw)
    p = SM.params_for(model, wide=wide)
    missing = SM.missing_mask(cloud)
    assert missing.any() and not missing.all()
    dense, slot = D.densify(cloud, L, missing)
    lh, ih, _ = O.run_b(*cloud, p)
    ld, idn, _ = O.run_b(*dense, p)
    assert idn["n_roi"] > 0
    assert np.array_equal(lh[~missing], ld) and ih == idn
    pos, firings, aligned = D.realign(slot, L, F + 3)
    assert aligned and firings == F   # (slots = position in the firing: the rule finds the firings)
    lp, ip, _ = O.run_b(*D.pad(dense, pos, L, F + 3), p)
    assert np.array_equal(lp[pos], ld) and ip == idn
    assert not lp[np.setdiff1d(np.arange((F + 3) * L), pos)].any()
    # any ids whatever: about n / 2 firings
    ids = np.random.default_rng(5).integers(0, L, len(slot))
    pos, firings, aligned = D.realign(ids, L, len(ids))
    assert aligned and firings > len(ids) // 4
    lp, ip, _ = O.run_b(*D.pad(dense, pos, L, len(ids)), p)
    assert np.array_equal(lp[pos], ld) and ip == idn


def test_the_rule_itself():
    pos, firings, aligned = D.realign([0, 2, 3, 1, 1, 0, 3], 4, 8)
    assert pos.tolist() == [0, 2, 3, 5, 9, 12, 15] and firings == 4 and aligned
    assert D.realign([0, 2, 3, 1, 1, 0, 3], 4, 3)[1:] == (4, False)              # more than W firings
    assert D.realign([0, 4, 1], 4, 8)[2] is False                                 # a slot >= L
    assert D.realign([0, 4, 1], 4, 8)[0].tolist() == [0, 1, 2]                     # ... point i stays at i
    assert D.realign([7, 5, 9], 4, 8, slot_map=[0] * 5 + [1, 9, 2])[2] is False   # (id 9 is beyond the map)
    assert D.realign([7, 5, 6], 4, 8, slot_map=[0] * 5 + [1, 9, 2])[2] is False   # (id 6 -> slot 9 >= L)
    pos, firings, aligned = D.realign([5, 7, 5], 4, 8, slot_map=[0] * 5 + [1, 9, 2])
    assert aligned and pos.tolist() == [1, 2, 5] and firings == 2
    assert D.realign([], 4, 8)[1:] == (0, True)
