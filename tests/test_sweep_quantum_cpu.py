"""The rule urf_set_sweep_quantum rests on, pinned against oracle B without a GPU: the reference drops non-finite points before anything
else (lidar_segmentation.cpp:100-117) and never looks at an input index, so (NaN, NaN, NaN) points appended behind a sweep change no
label and no summary.  15 dense sweeps (vlp16 at 300 and 304 firings, hdl32e at 130, ideal16 at 256, os32; range noise on, non-returns
removed), both regions of interest, each padded with NaN to the next multiple of 2048: the labels of the first n points equal the
unpadded run's bit for bit, the pad's labels are all 0, every summary field is equal."""
import numpy as np
import pytest

import oracles as O
import sensor_models as S
import sweep_quantum_cases as Q

SWEEPS = [(m, f, seed) for m, f in (("vlp16", 300), ("vlp16", 304), ("hdl32e", 130), ("ideal16", 256), ("os32", 1024)) for seed in (1, 2, 3)]


@pytest.mark.parametrize("wide", [False, True], ids=["default_roi", "wide_roi"])
@pytest.mark.parametrize("model,firings,seed", SWEEPS)
def test_a_nan_tail_changes_no_label_and_no_summary(model, firings, seed, wide):
    cloud = Q.dense_sweep(model, firings, seed, world=seed % 3)
    n = len(cloud[0])
    p = S.params_for(model, wide=wide)
    twin = Q.nan_padded(cloud)
    assert 3000 < n < 32768 and len(twin[0]) % Q.TILE == 0 and 0 < len(twin[0]) - n < Q.TILE
    assert all(np.array_equal(t[:n].view(np.uint32), a.view(np.uint32)) and np.isnan(t[n:]).all() for t, a in zip(twin, cloud))
    lab, info, _ = O.run_b(*cloud, p)
    lab2, info2, _ = O.run_b(*twin, p)
    print("%s %d firings seed %d: n %d -> %d, road %d curb %d roi %d rings %d" % (model, firings, seed, n, len(twin[0]), info["n_road"],
                                                                                  info["n_curb"], info["n_roi"], info["n_rings"]))
    assert info["status"] == 0 and info["n_road"] > 0 and info["n_curb"] > 0   # (a case that decides something)
    assert np.array_equal(lab2[:n], lab)
    assert not lab2[n:].any()
    assert info2 == info
