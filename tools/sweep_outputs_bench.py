#!/usr/bin/env python3
"""tools/sweep_outputs_bench.py -- what marker points and the reference order cost on the callback path, measured on one MI355X: read
after the wait (today's way) against travelling with the sweep (urf_set_sweep_outputs).  Prints ONE JSON line and, with --out, writes it.

    python tools/sweep_outputs_bench.py [--reps 200] [--windows 12] [--window 64] [--reverse] [--out profiles/sweep_results_direct_bench.json]

Two workloads: cfg2 64 x 2048 sweeps in firing order (the general kernels) and row-major 64 x 1024 sweeps (the fused front end, from the
context's third sweep on), both as 32-byte PointCloud2 records through urf_classify_pc2_async / _wait on max_batch 4 contexts of the
build with the test hooks.  Four arms, each on a context of its own, interleaved sweep by sweep (latency) and window by window
(throughput), behind an equality gate on labels, marker points and the three lists of every sweep:
  (a) wait, then urf_marker_points + urf_ordered_indices            (row-major: with urf_set_front_outputs on, so that the context stays fused)
  (b) urf_set_sweep_outputs(3) with the kernels of the two products launched one by one (debug flag 32 of the hooks build)
  (c) urf_set_sweep_outputs(3) with k_sweep_rings / k_sweep_lists
  (d) (c) with urf_set_sweep_results_direct(1): the kernels store header results and packed lists into mapped pinned memory, no copy
Per arm: latency with one sweep in flight (submit .. results in host arrays), sweeps/s with four in flight, median and p10-p90; per-pair
ratios a/c and b/c (above 1: c is faster) and c/d (above 1: d is faster); the bytes per sweep that cross PCIe in each direction, for (d)
computed from the counts of the gate's last sweep: labels + 32 + 4 * (c0 + c1 + c2) + 12 + 16 * m + 4.  All arms pay the same ctypes / numpy
cost per call; the figures are the Python client's, not a C client's.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DBG_OLD_KERNELS = 32   # urf_api.hip: URF_DBG_SWEEP_OLD_KERNELS


def pct(v, q):
    return float(np.percentile(np.asarray(v, np.float64), q))


def stats(v):
    return {"median": pct(v, 50), "p10": pct(v, 10), "p90": pct(v, 90)}


def verdict(ratio):
    """ratio = other / c per pair; c is faster where it lies above 1"""
    if ratio["p10"] > 1.0:
        return "faster by more than the run's spread"
    return "SLOWER" if ratio["p90"] < 1.0 else "not faster"


class Arm:
    def __init__(self, u, name, n, params, rows):
        self.u, self.name, self.n = u, name, n
        self.ctx = u.Context(n, 4, params=params, hooks=True)
        self.switch = name != "a"
        if name == "b":
            self.ctx._check(self.ctx._lib.urf_set_debug_flags(self.ctx._h, DBG_OLD_KERNELS), "urf_set_debug_flags")
        if name == "d":
            self.ctx.set_sweep_results_direct(1)
        if self.switch:
            self.ctx.set_sweep_outputs(3)
        elif rows:
            self.ctx.set_front_outputs(1)
        self.lab = np.empty(n, np.uint8)

    def submit(self, rec):
        return self.ctx.classify_pc2_async(rec, self.n, 32, 0, 4, 8)

    def collect(self, t):
        self.ctx.classify_pc2_wait(t, self.lab)
        if self.switch:
            return self.ctx.result_ordered_indices(t) + (self.ctx.result_marker_points(t),)
        return self.ctx.ordered_indices(self.n) + (self.ctx.marker_points(),)

    def one(self, rec):
        t0 = time.perf_counter()
        out = self.collect(self.submit(rec))
        return time.perf_counter() - t0, out

    def window(self, recs, count):
        tickets, t0 = [], time.perf_counter()
        for k in range(count):
            if len(tickets) == 4:
                self.collect(tickets.pop(0))
            tickets.append(self.submit(recs[k % len(recs)]))
        for t in tickets:
            self.collect(t)
        return count / (time.perf_counter() - t0)


def workload(u, O, records, name, clouds, params, rows, args):
    n = len(clouds[0][0])
    recs = [records(*c) for c in clouds]
    arms = [Arm(u, a, n, params, rows) for a in ("dcba" if args.reverse else "abcd")]   # (created, and taking their turns, in this order)
    for arm in arms:   # warm-up: capture, the row-major sighting, the first rerun
        for _ in range(3):
            for r in recs:
                arm.one(r)
    gate = 0
    for r in recs:     # equality gate: every arm, every sweep
        outs = []
        for arm in arms:
            _, out = arm.one(r)
            outs.append((arm.lab.copy(),) + out)
        for o in outs[1:]:
            assert all(x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(o, outs[0])), name
        assert all(len(o) == 5 for o in outs)   # labels, three lists, marker points
        gate += 1
    fused = [arm.ctx.front_scans() for arm in arms]
    lat = {a.name: [] for a in arms}
    for i in range(args.reps):
        for arm in arms:
            lat[arm.name].append(arm.one(recs[i % len(recs)])[0] * 1e3)
    thr = {a.name: [] for a in arms}
    for w in range(args.windows):
        for arm in arms:
            thr[arm.name].append(arm.window(recs, args.window))
    counts = [len(x) for x in outs[0][1:4]]
    markers = len(outs[0][4])
    n4 = (n + 3) & ~3
    res = {"points": n, "sweeps_in_gate": gate, "fused_last_sweep": fused,
           "latency_ms_one_in_flight": {k: stats(v) for k, v in lat.items()},
           "sweeps_per_s_four_in_flight": {k: stats(v) for k, v in thr.items()},
           "latency_ratio": {"a_over_c": stats(np.array(lat["a"]) / np.array(lat["c"])), "b_over_c": stats(np.array(lat["b"]) / np.array(lat["c"]))},
           "throughput_ratio": {"c_over_a": stats(np.array(thr["c"]) / np.array(thr["a"])), "c_over_b": stats(np.array(thr["c"]) / np.array(thr["b"]))},
           "pcie_bytes_per_sweep": {
               "host_to_device": 12 * n4,
               "device_to_host_labels_and_summary": n + 32,
               "device_to_host_a_readouts": 4 * (361 * 4 + 4) + 12 + 4 * sum(counts),
               "device_to_host_bc_results": 4 * (361 * 4 + 4) + 12 * n,
               "lists_share_of_bc": 12 * n, "list_entries_used": counts,
               "device_to_host_d_total": n + 32 + 4 * sum(counts) + 12 + 16 * markers + 4, "marker_points": markers}}
    res["latency_ratio"]["c_over_d"] = stats(np.array(lat["c"]) / np.array(lat["d"]))
    res["throughput_ratio"]["d_over_c"] = stats(np.array(thr["d"]) / np.array(thr["c"]))
    res["outcome"] = {"c_vs_a_latency": verdict(res["latency_ratio"]["a_over_c"]), "c_vs_b_latency": verdict(res["latency_ratio"]["b_over_c"]),
                      "c_vs_a_throughput": verdict(res["throughput_ratio"]["c_over_a"]), "c_vs_b_throughput": verdict(res["throughput_ratio"]["c_over_b"]),
                      "d_vs_c_latency": verdict(res["latency_ratio"]["c_over_d"]), "d_vs_c_throughput": verdict(res["throughput_ratio"]["d_over_c"])}
    for arm in arms:
        arm.ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=12)
    ap.add_argument("--window", type=int, default=64)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reverse", action="store_true", help="create the arms' contexts, and give them their turns, in the order d c b a")
    args = ap.parse_args()
    import oracles as O
    import urban_road_filter_amd as u
    from test_gpu_async import records
    from test_gpu_front import ring_major
    out = {"tool": "tools/sweep_outputs_bench.py", "reps": args.reps, "windows": args.windows, "window": args.window,
           "arm_order": "dcba" if args.reverse else "abcd",
           "untimed": "16, 32 and 128 lasers per firing; curbPoints other than 5; a C client (the figures include ctypes / numpy per call)"}
    out["cfg2_64x2048"] = workload(u, O, records, "cfg2_64x2048", [O.cfg_cloud("cfg2", s) for s in (1, 2, 3, 4)], O.cfg_params("cfg2"), False, args)
    out["rows_64x1024"] = workload(u, O, records, "rows_64x1024", [ring_major(u.synth_cloud(64, 1024, 1, s)) for s in (5, 6, 7, 8)],
                                   u.default_params().wide_roi(), True, args)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
