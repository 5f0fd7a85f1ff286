"""Dense sweeps of varying length for urf_set_sweep_quantum (TEST CODE): sensor-like sweeps of tests/sensor_models.py with range noise,
the non-returns removed as a driver's dense mode removes them (tests/dense_model.py: densify), and their NaN-padded twins.  Oracle B on
every input is computed once per process and never modified."""
import numpy as np

import dense_model as D
import oracles as O
import sensor_models as S

TILE = 2048
_REF = {}


def dense_sweep(model, firings, seed, world=0):
    """One dense sweep in firing order: (x, y, z) float32, a different length for every seed."""
    cloud = S.sweep(model, firings=firings, world=world, seed=seed, noise=True, holes=("nan",), layout="firing")
    return D.densify(cloud, S.lasers(model), S.missing_mask(cloud))[0]


def padded_len(n, quantum=TILE):
    return (n + quantum - 1) // quantum * quantum


def nan_padded(cloud, quantum=TILE):
    """The sweep with (NaN, NaN, NaN) appended up to the next multiple of the quantum."""
    n = len(cloud[0])
    tail = np.full(padded_len(n, quantum) - n, np.nan, np.float32)
    return tuple(np.concatenate([a, tail]) for a in cloud)


def params32(wide=True):
    """One parameter set for 16- and 32-laser sweeps alike (channels is the ring table's capacity)."""
    return S.params_for("hdl32e", wide=wide)


def ref(key, cloud, p, debug=False):
    """Oracle B on the caller's unpadded points: (labels, summary, stages or None)."""
    k = (key, bool(debug))
    if k not in _REF:
        _REF[k] = O.run_b(*cloud, p, debug=debug)
    return _REF[k]


#          model, firings, world: world 2's narrow street returns fewer points
STREAM12 = [("vlp16", 304, 0), ("vlp16", 304, 1), ("vlp16", 300, 2), ("vlp16", 300, 2),
            ("hdl32e", 190, 0), ("hdl32e", 190, 1), ("hdl32e", 130, 2), ("hdl32e", 130, 0),
            ("vlp16", 300, 0), ("vlp16", 300, 1), ("vlp16", 304, 2), ("vlp16", 304, 2)]


#          the same sensor throughout: 16 lasers, 8 rings in the wide region of interest, sweep after sweep
STREAM16 = [("vlp16", 304, 0), ("vlp16", 300, 2), ("vlp16", 304, 1), ("vlp16", 300, 2),
            ("vlp16", 300, 0), ("vlp16", 304, 2), ("vlp16", 300, 1), ("vlp16", 304, 2),
            ("vlp16", 304, 2), ("vlp16", 300, 0), ("vlp16", 300, 2), ("vlp16", 304, 1)]


def _stream(name, spec):
    out = []
    seed = 100
    seen = set()
    for k, (model, firings, world) in enumerate(spec):
        while True:
            seed += 1
            c = dense_sweep(model, firings, seed, world=world)
            if len(c[0]) not in seen:
                break
        seen.add(len(c[0]))
        out.append(((name, k), c))
    assert len(seen) == 12 and all(len(out[k][1][0]) != len(out[k + 4][1][0]) for k in range(8))
    assert {padded_len(len(c[0])) for _, c in out} == {4096, 6144}
    return out


def stream12():
    """12 dense sweeps of 12 distinct lengths: vlp16 at 300 and 304 firings (3 478-4 514 points) and hdl32e at 130 and 190, n' 4096 or
    6144.  Sweep k and sweep k + 4, which share a slot with four in flight, differ in length."""
    return _stream("stream12", STREAM12)


def stream16():
    """12 dense sweeps of 12 distinct lengths from ONE sensor (vlp16, 300 and 304 firings, three streets): n' 4096 or 6144, both in
    every slot with four in flight, and the same 8 rings in every sweep -- so that urf_callback_path_preset really fixes the sequence.
    (What a context learns from its sweeps changes the sequence and forgets the captured ones.  The one thing the preset cannot say
    ahead is the ring-count hint, which is dropped when a sweep has more rings than its row's previous one: in a stream that mixes 16-
    and 32-laser sweeps that happens somewhere in a first pass, or in a second one.)"""
    out = _stream("stream16", STREAM16)
    for s in range(4):
        assert {padded_len(len(out[k][1][0])) for k in (s, s + 4, s + 8)} == {4096, 6144}, s
    return out


_STREAM = []


def stream():
    if not _STREAM:
        _STREAM.extend(stream12())
    return _STREAM


def records(x, y, z, step=32, ox=0, oy=4, oz=8, fill=0):
    """PointCloud2 records of `step` bytes with x / y / z at the given offsets."""
    buf = np.full((len(x), step), fill, np.uint8)
    buf[:, ox:ox + 4] = x.view(np.uint8).reshape(-1, 4)
    buf[:, oy:oy + 4] = y.view(np.uint8).reshape(-1, 4)
    buf[:, oz:oz + 4] = z.view(np.uint8).reshape(-1, 4)
    return buf.reshape(-1)
