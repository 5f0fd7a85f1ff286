#!/usr/bin/env python3
"""tools/curb_points_bench.py -- urf_set_front_mode(3) against mode 2 for curbPoints 1..8, measured on one MI355X.  Prints ONE JSON line
(and writes it to --out).

    timeout 900 python tools/curb_points_bench.py [--scans 1024] [--rounds 9] [--warmup 3] [--cps 1,2,3,4,5,6,7,8] [--out profiles/curb_points_bench.json]

Workload: --scans resident 64 x 2048 sweeps of cfg2 (tests/oracles.py: cfg_cloud("cfg2", seed), cfg_params("cfg2")), in firing order and
row-major.  Two contexts on the same device arrays, one in mode 3 and one in mode 2 -- mode 2 is the path every curbPoints != 5 took before
mode 3 existed: the general kernels (k_split + k_ring_general + k_label); with curbPoints == 5 both launch the same kernels, the pair's
difference is the noise floor of the method.  Per curbPoints: a label-equality gate (mode 3 == mode 2 on every scan of the batch, sampled
scans == oracle B), warm-up, then --rounds rounds of ONE call of each context, interleaved, between device events.  Reported per arm:
median and minimum ms per call, and the spread (max - min) / median over the rounds; "wins" = mode 3's median is below mode 2's by more
than the larger of the two spreads.  The register counts and waves per SIMD of the instances come from tools/kernel_resources.py.

    timeout 900 python tools/curb_points_bench.py --lasers 16,32,128 [--scans 1024] [--scans128 256] [--out profiles/curb_points_lasers_bench.json]

--lasers (default 64: the run above, unchanged): for another laser count L the workload is --scans (128 lasers: --scans128) resident
urf_synth_cloud(L, 2048, scene, seed) sweeps under the wide region of interest (channels = L; 128: interval 0.05), in firing order and
row-major, and the two arms are urf_set_front_curb_points on against off, BOTH in mode 3 (128: urf_set_front_lasers128 on in both) --
off is what these parameters launch without the switch, the general kernels.  The interleaving, the label-equality gate and the
"wins" rule are the same; the rows carry "lasers" and the arms are called "on" and "off" (p10 / p90 of the rounds next to the median)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
COLS = 2048
N = 64 * COLS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cps", default="1,2,3,4,5,6,7,8")
    ap.add_argument("--distinct", type=int, default=16, help="distinct sweeps the batch is built from")
    ap.add_argument("--orders", default="firing,rows")
    ap.add_argument("--lasers", default="64", help="laser counts (64: mode 3 against mode 2 on cfg2; 16, 32, 128: the curb-points switch on against off)")
    ap.add_argument("--scans128", type=int, default=256, help="resident sweeps at 128 lasers")
    ap.add_argument("--no-resources", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import urban_road_filter_amd as u
    import oracles as O
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured here")
    dev = torch.device("cuda:0")
    out = {"metric": "curb_points_front_mode_3", "device": torch.cuda.get_device_name(0), "scans": args.scans, "cols": COLS,
           "workload": "cfg2", "timing": "device events around one call, %d interleaved rounds per pair after %d warm-up calls" % (args.rounds, args.warmup),
           "results": []}
    t0 = time.time()
    st = torch.cuda.Stream()

    def one(ctx, bufs, labels):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ctx.classify_batch_soa(bufs[0], bufs[1], bufs[2], N, args.scans, labels, None)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def stats(ts):
        ts = np.asarray(ts)
        return {"median_ms": float(np.median(ts)), "min_ms": float(ts.min()), "spread": float((ts.max() - ts.min()) / np.median(ts))}

    def one_of(ctx, bufs, labels, n, scans):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ctx.classify_batch_soa(bufs[0], bufs[1], bufs[2], n, scans, labels, None)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def stats_p(ts):
        r = stats(ts)
        r["p10_ms"], r["p90_ms"] = float(np.percentile(ts, 10)), float(np.percentile(ts, 90))
        return r

    def lasers_run(L):
        """urf_set_front_curb_points on against off, both in mode 3, at L lasers per firing."""
        S, n = (args.scans128 if L == 128 else args.scans), L * COLS
        clouds = [u.synth_cloud(L, COLS, 1 + s % 4, 100 + s) for s in range(min(args.distinct, S))]
        for order in args.orders.split(","):
            src = clouds if order == "firing" else [tuple(np.ascontiguousarray(a.reshape(-1, L).T.reshape(-1)) for a in c) for c in clouds]
            parts = [torch.from_numpy(np.concatenate([c[k] for c in src])).to(dev) for k in range(3)]
            reps = (S + len(src) - 1) // len(src)
            bufs = [t.repeat(reps)[:S * n].contiguous() for t in parts]
            lab_on = torch.empty(S * n, dtype=torch.uint8, device=dev)
            lab_off = torch.empty(S * n, dtype=torch.uint8, device=dev)
            with u.Context(n, S) as c_on, u.Context(n, S) as c_off:
                for c, on in ((c_on, 1), (c_off, 0)):
                    c.set_stream(st.cuda_stream)
                    if L == 128:
                        c.set_front_lasers128(1)
                    c.set_front_curb_points(on)
                    c.set_front_mode(3)
                for cp in [int(v) for v in args.cps.split(",")]:
                    p = u.default_params().wide_roi()
                    p.channels = L
                    if L == 128:
                        p.interval = 0.05
                    p.curbPoints = cp
                    c_on.set_params(p)
                    c_off.set_params(p)
                    for _ in range(max(args.warmup, 2)):
                        one_of(c_on, bufs, lab_on, n, S)
                        one_of(c_off, bufs, lab_off, n, S)
                    torch.cuda.synchronize()
                    if not torch.equal(lab_on, lab_off):
                        raise SystemExit("label gate: %d lasers %s curbPoints %d: switch on and off differ" % (L, order, cp))
                    got = lab_on[:2 * n].cpu().numpy().reshape(2, n)
                    for k in (0, 1):
                        if not np.array_equal(got[k], O.run_b(*src[k % len(src)], p)[0]):
                            raise SystemExit("label gate: %d lasers %s curbPoints %d scan %d differs from oracle B" % (L, order, cp, k))
                    t_on, t_off = [], []
                    for _ in range(args.rounds):
                        t_on.append(one_of(c_on, bufs, lab_on, n, S))
                        t_off.append(one_of(c_off, bufs, lab_off, n, S))
                    row = {"lasers": L, "scans": S, "order": order, "curbPoints": cp, "on": stats_p(t_on), "off": stats_p(t_off),
                           "on_front_scans": int(c_on.front_scans()), "off_front_scans": int(c_off.front_scans())}
                    row["on_scans_per_s"] = S / row["on"]["median_ms"] * 1e3
                    row["off_scans_per_s"] = S / row["off"]["median_ms"] * 1e3
                    row["speedup"] = row["off"]["median_ms"] / row["on"]["median_ms"]
                    row["wins"] = bool(row["off"]["median_ms"] - row["on"]["median_ms"] >
                                       max(row["on"]["spread"], row["off"]["spread"]) * row["off"]["median_ms"])
                    out["results"].append(row)

    lasers = [int(v) for v in args.lasers.split(",")]
    if lasers != [64]:
        out["metric"] = "curb_points_front_lasers"
        out["workload"] = "urf_synth_cloud(L, %d, scene, seed), wide region of interest; 128 lasers: %d sweeps" % (COLS, args.scans128)
    base = [O.cfg_cloud("cfg2", 1 + s) for s in range(min(args.distinct, args.scans))] if 64 in lasers else []
    with torch.cuda.stream(st):
        for L in lasers:
            if L != 64:
                lasers_run(L)
        for order in (args.orders.split(",") if 64 in lasers else []):
            src = base if order == "firing" else [tuple(np.ascontiguousarray(a.reshape(-1, 64).T.reshape(-1)) for a in c) for c in base]
            parts = [torch.from_numpy(np.concatenate([c[k] for c in src])).to(dev) for k in range(3)]
            reps = (args.scans + len(src) - 1) // len(src)
            bufs = [t.repeat(reps)[:args.scans * N].contiguous() for t in parts]
            lab3 = torch.empty(args.scans * N, dtype=torch.uint8, device=dev)
            lab2 = torch.empty(args.scans * N, dtype=torch.uint8, device=dev)
            with u.Context(N, args.scans) as c3, u.Context(N, args.scans) as c2:
                c3.set_stream(st.cuda_stream)
                c2.set_stream(st.cuda_stream)
                c3.set_front_mode(3)
                c2.set_front_mode(2)
                for cp in [int(v) for v in args.cps.split(",")]:
                    p = O.cfg_params("cfg2")
                    p.curbPoints = cp
                    c3.set_params(p)
                    c2.set_params(p)
                    # the gate (and the warm-up: a row-major context's first call only sights the layout)
                    for _ in range(max(args.warmup, 2)):
                        one(c3, bufs, lab3)
                        one(c2, bufs, lab2)
                    torch.cuda.synchronize()
                    if not torch.equal(lab3, lab2):
                        raise SystemExit("label gate: %s curbPoints %d: mode 3 and mode 2 differ" % (order, cp))
                    got = lab3[:2 * N].cpu().numpy().reshape(2, N)
                    for k in (0, 1):
                        if not np.array_equal(got[k], O.run_b(*src[k % len(src)], p)[0]):
                            raise SystemExit("label gate: %s curbPoints %d scan %d differs from oracle B" % (order, cp, k))
                    t3, t2 = [], []
                    for _ in range(args.rounds):
                        t3.append(one(c3, bufs, lab3))
                        t2.append(one(c2, bufs, lab2))
                    row = {"order": order, "curbPoints": cp, "mode3": stats(t3), "mode2": stats(t2),
                           "mode3_front_scans": int(c3.front_scans()), "mode2_front_scans": int(c2.front_scans())}
                    row["mode3_scans_per_s"] = args.scans / row["mode3"]["median_ms"] * 1e3
                    row["mode2_scans_per_s"] = args.scans / row["mode2"]["median_ms"] * 1e3
                    row["speedup"] = row["mode2"]["median_ms"] / row["mode3"]["median_ms"]
                    row["wins"] = bool(row["mode2"]["median_ms"] - row["mode3"]["median_ms"] >
                                       max(row["mode3"]["spread"], row["mode2"]["spread"]) * row["mode2"]["median_ms"])
                    out["results"].append(row)
    if not args.no_resources:
        import kernel_resources
        out["instances"] = {r["name"]: {"VGPRs": int(r["VGPRs"]), "waves_per_SIMD": int(r["Occupancy [waves/SIMD]"]), "scratch": int(r["ScratchSize [bytes/lane]"])}
                            for r in kernel_resources.resources() if r["name"].startswith("k_front")}
    out["wall_s"] = time.time() - t0
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
