#!/usr/bin/env python3
"""tools/dense_outputs_bench.py -- the reference-order read-outs after a dense call (urf_set_dense_outputs), measured on one MI355X.
Prints ONE JSON line; recorded under profiles/dense_outputs_bench.json.

    timeout 900 python tools/dense_outputs_bench.py [--scans 1024] [--steps 10] [--warmup 2] [--distinct 32] [--firings 2048]

--scans resident dense ideal64 sweeps (tests/sensor_models.py) of --firings firings, --distinct distinct ones repeated, ids = the laser's
position in the firing as uint16, front mode 2.  Behind a gate against oracle B (tests/oracles.py, on the dense points: labels and the
road / curb / ring-10 orders of three scans) a pair "classify + read-out" is timed with device events, the arms interleaved pair by pair:
  a      classify_batch_soa_ragged + read-out                              (context A: the path the reference order took so far)
  b_off  classify_batch_soa_dense, urf_set_dense_outputs on + read-out     (context B, urf_set_front_outputs off: the read-out runs the
                                                                            padded batch again through the general kernels)
  b_on   the same with urf_set_front_outputs on                            (context B: no second run)
once with urf_ordered_indices_batch as the read-out, once with urf_clouds_batch_soa(URF_ORDER_REFERENCE).  Context B is put back into
front mode 2 in front of every pair of its own, outside the timed bracket (a read-out with urf_set_front_outputs off leaves a context
with the general kernels).  Per arm: the 10th / 50th / 90th percentiles of ms per pair and of the per-pair ratio a / b."""
import argparse
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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--distinct", type=int, default=32, help="distinct sweeps the batch is built from")
    ap.add_argument("--firings", type=int, default=2048)
    args = ap.parse_args()
    import torch
    import urban_road_filter_amd as u
    import dense_model as D
    import oracles as O
    import sensor_models as SM
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured here")
    dev = torch.device("cuda:0")
    model, S, W = "ideal64", args.scans, args.firings
    L = SM.lasers(model)
    p = SM.params_for(model, wide=True)
    out = {"metric": "dense_outputs_bench", "device": torch.cuda.get_device_name(0), "model": model, "scans": S, "firings": W, "front_mode": 2,
           "timing": "device events per pair (classify + read-out), a / b_off / b_on interleaved pair by pair in one process; ms", "results": []}
    t0 = time.time()
    st = torch.cuda.Stream()
    pct = lambda v: [float(np.percentile(v, q)) for q in (10, 50, 90)]  # noqa: E731
    with torch.cuda.stream(st):
        k_distinct = min(args.distinct, S)
        dense, slots = [], []
        for k in range(k_distinct):
            # (start 0: a sweep whose seam falls inside a tile is handed back by the fused front end, by contract)
            cloud = SM.sweep(model, firings=W, world=k % 3, seed=500 + k)
            d, s = D.densify(cloud, L, SM.missing_mask(cloud))
            assert D.realign(s, L, W)[2]
            dense.append(d)
            slots.append(s)
        order = [k % k_distinct for k in range(S)]
        lens = [len(slots[k]) for k in order]
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
        n_total, max_len, n = int(offs[-1]), max(lens), W * L
        cat = lambda j: torch.from_numpy(np.concatenate([dense[k][j] for k in order])).to(dev)  # noqa: E731
        dx, dy, dz = (cat(j) for j in range(3))
        did = torch.from_numpy(np.concatenate([slots[k] for k in order]).astype(np.uint16).view(np.int16)).to(dev)
        doff = torch.from_numpy(offs.view(np.int32)).to(dev)
        lab = {k: torch.empty(n_total, dtype=torch.uint8, device=dev) for k in ("a", "b")}
        lists = [torch.empty(S * max_len, dtype=torch.int32, device=dev) for _ in range(3)]
        lcnt = torch.empty(3 * S, dtype=torch.int32, device=dev)
        cap = 3 * S * max_len
        rec = torch.empty(cap * 8, dtype=torch.float32, device=dev)
        ccnt = torch.empty(4 * S, dtype=torch.int32, device=dev)
        coff = torch.empty(4 * S, dtype=torch.int64, device=dev)
        gate = sorted({0, 1, S - 1})
        want = {k: O.run_b(*dense[order[k]], p, debug=True) for k in gate}
        with u.Context(n, S, params=p) as A, u.Context(n, S, params=p) as B:
            for ctx in (A, B):
                ctx.set_stream(st.cuda_stream)
                ctx.set_front_mode(2)
            B.set_dense_outputs(1)
            readouts = {"lists": lambda ctx: ctx.ordered_indices_batch(*lists, max_len, lcnt),
                        "clouds": lambda ctx: ctx.clouds_batch_soa(None, u.ORDER_REFERENCE, rec, cap, ccnt, coff)}
            classify = {"a": lambda: A.classify_batch_soa_ragged(dx, dy, dz, doff, max_len, S, lab["a"], None),
                        "b": lambda: B.classify_batch_soa_dense(dx, dy, dz, did, 2, doff, max_len, S, W, lab["b"], None)}

            def prepare(arm):   # outside the timed bracket
                if arm != "a":
                    B.set_front_outputs(1 if arm == "b_on" else 0)
                    B.set_front_mode(2)

            def pair(arm, readout):
                ctx = A if arm == "a" else B
                classify["a" if arm == "a" else "b"]()
                fused = None
                if readout is None:
                    torch.cuda.synchronize()
                    fused = int(ctx.front_scans())
                    readout = "lists"
                readouts[readout](ctx)
                return fused

            for readout in ("lists", "clouds"):
                fused, after = {}, {}
                for arm in ("a", "b_off", "b_on"):   # the gate and the warm-up
                    for _ in range(max(2, args.warmup)):
                        prepare(arm)
                        pair(arm, readout)
                    prepare(arm)
                    fused[arm] = pair(arm, None)
                    torch.cuda.synchronize()
                    after[arm] = int((A if arm == "a" else B).front_scans())
                    got = lab["a" if arm == "a" else "b"].cpu().numpy()
                    cnt = lcnt.cpu().numpy().view(np.uint32).reshape(S, 3)
                    host = [t.cpu().numpy().view(np.uint32).reshape(S, max_len) for t in lists]
                    for k, (lb, ib, sd) in want.items():
                        if not np.array_equal(got[offs[k]:offs[k + 1]], lb):
                            raise SystemExit("label gate: arm %s scan %d differs from oracle B" % (arm, k))
                        for j, key in enumerate(("road_order", "curb_order", "ring10_order")):
                            if not np.array_equal(host[j][k][:cnt[k][j]], sd[key]):
                                raise SystemExit("order gate: arm %s scan %d %s differs from oracle B" % (arm, k, key))
                ts = {"a": [], "b_off": [], "b_on": []}
                for _ in range(args.steps):
                    for arm in ("a", "b_off", "b_on"):
                        prepare(arm)
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        pair(arm, readout)
                        e1.record()
                        e1.synchronize()
                        ts[arm].append(e0.elapsed_time(e1))
                out["results"].append({"readout": readout, "points_dense": n_total, "points_padded": S * n, "max_len": max_len,
                                       "front_scans_after_classify": fused, "front_scans_after_readout": after,
                                       "dense_scans": int(B.dense_scans()),
                                       "a_ragged_ms_p10_p50_p90": pct(ts["a"]), "b_off_ms_p10_p50_p90": pct(ts["b_off"]),
                                       "b_on_ms_p10_p50_p90": pct(ts["b_on"]),
                                       "a_over_b_off_p10_p50_p90": pct([a / b for a, b in zip(ts["a"], ts["b_off"])]),
                                       "a_over_b_on_p10_p50_p90": pct([a / b for a, b in zip(ts["a"], ts["b_on"])])})
    out["wall_s"] = time.time() - t0
    print(json.dumps(out))


if __name__ == "__main__":
    main()
