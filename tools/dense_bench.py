#!/usr/bin/env python3
"""tools/dense_bench.py -- dense sweeps (non-returns dropped) through urf_classify_batch_soa_dense, measured on one MI355X.
Prints ONE JSON line; recorded under profiles/dense_bench.json.

    timeout 900 python tools/dense_bench.py [--scans 1024] [--steps 20] [--warmup 3] [--distinct 32] [--firings 2048]

Per sensor model (hdl64e-like with range noise, ideal64; tests/sensor_models.py): --scans resident dense sweeps of --firings firings,
--distinct distinct ones repeated, ids = the laser's position in the firing as uint16.  Behind a label gate against oracle B
(tests/oracles.py, on the dense points) two contexts in front mode 2 are timed with device events, interleaved call by call:
  a  classify_batch_soa_ragged on the dense points   (context A: the baseline -- that entry point's code is the parent commit's)
  b  classify_batch_soa_dense                        (context B)
  c  classify_batch_soa on the organised twin        (context B: the padded sweeps built on the host, the bound)
Per side: the 10th / 50th / 90th percentiles of ms per call, the per-pair ratio a / b, urf_front_scans, urf_dense_scans.

    timeout 900 python tools/dense_bench.py --elev ... > profiles/dense_elev_bench.json

--elev adds a fourth arm, interleaved with the others (their keys and calls stay as they are):
  d  classify_batch_soa_dense_elev                   (context D, the library with the test hooks: no ids handed in, derived on the
                                                      device from the points' elevation and the model's table, urf_set_dense_elevations)
with its percentiles, the per-pair ratios a / d and b / d, the share of derived ids that are the true slots, and the id kernel's own
bracket (urf_test_dense_ids_ms: k_dense_ids_soa of the last call launched again, ms per launch)."""
import argparse
import contextlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=32, help="distinct sweeps the batch is built from")
    ap.add_argument("--firings", type=int, default=2048)
    ap.add_argument("--models", default="hdl64e,ideal64")
    ap.add_argument("--elev", action="store_true", help="add arm d: the dense call with ids derived from elevation")
    args = ap.parse_args()
    import torch
    import urban_road_filter_amd as u
    import dense_model as D
    import oracles as O
    import sensor_models as SM
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured here")
    dev = torch.device("cuda:0")
    S, W = args.scans, args.firings
    out = {"metric": "dense_elev_bench" if args.elev else "dense_bench", "device": torch.cuda.get_device_name(0), "scans": S, "firings": W, "front_mode": 2,
           "timing": "device events per call, a / b / c interleaved call by call in one process; ms", "results": []}
    t0 = time.time()
    st = torch.cuda.Stream()
    pct = lambda v: [float(np.percentile(v, q)) for q in (10, 50, 90)]  # noqa: E731
    with torch.cuda.stream(st):
        for model in args.models.split(","):
            L = SM.lasers(model)
            p = SM.params_for(model, wide=True)
            k_distinct = min(args.distinct, S)
            dense, slots, twins = [], [], []
            for k in range(k_distinct):
                # (start 0: a sweep whose seam falls inside a tile is handed back by the fused front end, by contract)
                cloud = SM.sweep(model, firings=W, world=k % 3, seed=500 + k, noise=model != "ideal64")
                d, s = D.densify(cloud, L, SM.missing_mask(cloud))
                pos, _, aligned = D.realign(s, L, W)
                assert aligned
                dense.append(d)
                slots.append(s)
                twins.append(D.pad(d, pos, L, W))
            order = [k % k_distinct for k in range(S)]
            lens = [len(slots[k]) for k in order]
            offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
            n_total, max_len, n = int(offs[-1]), max(lens), W * L
            cat = lambda src, j: torch.from_numpy(np.concatenate([src[k][j] for k in order])).to(dev)  # noqa: E731
            dx, dy, dz = (cat(dense, j) for j in range(3))
            tx, ty, tz = (cat(twins, j) for j in range(3))
            did = torch.from_numpy(np.concatenate([slots[k] for k in order]).astype(np.uint16).view(np.int16)).to(dev)
            doff = torch.from_numpy(offs.view(np.int32)).to(dev)
            lab_a = torch.empty(n_total, dtype=torch.uint8, device=dev)
            lab_b = torch.empty(n_total, dtype=torch.uint8, device=dev)
            lab_c = torch.empty(S * n, dtype=torch.uint8, device=dev)
            lab_d = torch.empty(n_total if args.elev else 1, dtype=torch.uint8, device=dev)
            arms = ("a", "b", "c", "d") if args.elev else ("a", "b", "c")
            gate = sorted({0, 1, S - 1})
            want = {k: O.run_b(*dense[order[k]], p)[0] for k in gate}
            with contextlib.ExitStack() as stack:
                A, B = stack.enter_context(u.Context(n, S, params=p)), stack.enter_context(u.Context(n, S, params=p))
                Dx = stack.enter_context(u.Context(n, S, params=p, hooks=True)) if args.elev else None
                for ctx in (A, B, Dx) if args.elev else (A, B):
                    ctx.set_stream(st.cuda_stream)
                    ctx.set_front_mode(2)
                if args.elev:
                    Dx.set_dense_elevations(SM.MODELS[model]["elev"])
                calls = {"a": lambda: A.classify_batch_soa_ragged(dx, dy, dz, doff, max_len, S, lab_a, None),
                         "b": lambda: B.classify_batch_soa_dense(dx, dy, dz, did, 2, doff, max_len, S, W, lab_b, None),
                         "c": lambda: B.classify_batch_soa(tx, ty, tz, n, S, lab_c, None),
                         "d": lambda: Dx.classify_batch_soa_dense_elev(dx, dy, dz, doff, max_len, S, W, lab_d, None)}
                fused, aligned_scans, elev_info = {}, None, {}
                for name in arms:   # the label gate and the warm-up
                    for _ in range(max(2, args.warmup)):
                        calls[name]()
                    torch.cuda.synchronize()
                    ctx = A if name == "a" else Dx if name == "d" else B
                    fused[name] = int(ctx.front_scans())
                    if name == "b":
                        aligned_scans = int(B.dense_scans())
                    if name == "d":
                        true_slots = np.concatenate([slots[k] for k in order]).astype(np.uint8)
                        elev_info = {"dense_scans_d": int(Dx.dense_scans()),
                                     "derived_ids_equal_true_slots": float((Dx.dense_ids(n_total) == true_slots).mean())}
                    if name != "c":
                        got = (lab_a if name == "a" else lab_d if name == "d" else lab_b).cpu().numpy()
                        for k, lb in want.items():
                            if not np.array_equal(got[offs[k]:offs[k + 1]], lb):
                                raise SystemExit("label gate: %s side %s scan %d differs from oracle B" % (model, name, k))
                ts = {name: [] for name in arms}
                for _ in range(args.steps):
                    for name in arms:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        calls[name]()
                        e1.record()
                        e1.synchronize()
                        ts[name].append(e0.elapsed_time(e1))
                out["results"].append({"model": model, "lasers": L, "points_dense": n_total, "points_padded": S * n,
                                       "front_scans": fused, "dense_scans": aligned_scans,
                                       "a_ragged_ms_p10_p50_p90": pct(ts["a"]), "b_dense_ms_p10_p50_p90": pct(ts["b"]),
                                       "c_twin_ms_p10_p50_p90": pct(ts["c"]),
                                       "a_over_b_p10_p50_p90": pct([a / b for a, b in zip(ts["a"], ts["b"])])})
                if args.elev:
                    calls["d"]()   # (the id kernel's bracket launches the last elevation call's again)
                    torch.cuda.synchronize()
                    ids_ms = [Dx.dense_ids_ms(5) for _ in range(args.steps)]
                    out["results"][-1].update(elev_info, d_dense_elev_ms_p10_p50_p90=pct(ts["d"]),
                                              a_over_d_p10_p50_p90=pct([a / d for a, d in zip(ts["a"], ts["d"])]),
                                              b_over_d_p10_p50_p90=pct([b / d for b, d in zip(ts["b"], ts["d"])]),
                                              k_dense_ids_soa_ms_p10_p50_p90=pct(ids_ms))
            del dx, dy, dz, tx, ty, tz, did, lab_a, lab_b, lab_c, lab_d
            torch.cuda.empty_cache()
    out["wall_s"] = time.time() - t0
    print(json.dumps(out))


if __name__ == "__main__":
    main()
