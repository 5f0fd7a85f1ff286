#!/usr/bin/env python3
"""tools/sweep_lengths_bench.py -- what a stream of sweeps of varying length costs on the callback path, measured on one MI355X: a captured
sequence per sweep (today's way) against one per padded length (urf_set_sweep_quantum).  Prints ONE JSON line and, with --out, writes it.

    python tools/sweep_lengths_bench.py [--reps 200] [--windows 12] [--window 64] [--reverse] [--out profiles/sweep_lengths_bench.json]

Two streams of scene-3 sensor-like 64 x 2048 sweeps (range noise, drop-outs), 16 of them in turn, as 32-byte PointCloud2 records through
urf_classify_pc2_async / _wait on max_batch 4 contexts with the sequence preset (urf_callback_path_preset(2 | 4 | 16)):
  dense64   the drop-outs removed, as a driver's dense mode removes them: a different length each sweep
  fixed64   the same sweeps with the holes in place: one length
Arms, each on a context of its own, interleaved sweep by sweep (latency) and window by window (throughput), behind an equality gate on
the labels of every sweep:
  off      urf_set_sweep_quantum(0)
  q2048    urf_set_sweep_quantum(2048)
  q16384   urf_set_sweep_quantum(16384)           (dense64 only)
Per arm: latency with one sweep in flight (submit .. labels in a host array), sweeps/s with four in flight, median and p10-p90, and the
sequences captured while both were timed; per-pair ratios off / on (above 1: the switch is faster).  All arms pay the same ctypes /
numpy cost per call; the figures are the Python client's, not a C client's.
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

N = 64 * 2048


def pct(v, q):
    return float(np.percentile(np.asarray(v, np.float64), q))


def stats(v):
    return {"median": pct(v, 50), "p10": pct(v, 10), "p90": pct(v, 90)}


def verdict(ratio):
    """ratio = off / on per pair (latency) or on / off (throughput); the switch is faster where it lies above 1"""
    if ratio["p10"] > 1.0:
        return "faster by more than the run's spread"
    return "SLOWER" if ratio["p90"] < 1.0 else "not faster"


class Arm:
    def __init__(self, u, name, quantum, params):
        self.name = name
        self.ctx = u.Context(N, 4, params=params)
        self.ctx.callback_path_preset(2 | 4 | 16)
        self.ctx.set_sweep_quantum(quantum)
        self.lab = np.empty(N, np.uint8)

    def one(self, rec):
        t0 = time.perf_counter()
        self.ctx.classify_pc2_wait(self.ctx.classify_pc2_async(rec, len(rec) // 32, 32, 0, 4, 8), self.lab)
        return time.perf_counter() - t0

    def window(self, recs, count):
        tickets, t0 = [], time.perf_counter()
        for k in range(count):
            if len(tickets) == 4:
                self.ctx.classify_pc2_wait(tickets.pop(0), self.lab)
            r = recs[k % len(recs)]
            tickets.append(self.ctx.classify_pc2_async(r, len(r) // 32, 32, 0, 4, 8))
        for t in tickets:
            self.ctx.classify_pc2_wait(t, self.lab)
        return count / (time.perf_counter() - t0)


def workload(u, records, name, clouds, params, quanta, args):
    recs = [records(*c) for c in clouds]
    arms = [Arm(u, "off" if q == 0 else "q%d" % q, q, params) for q in (reversed(quanta) if args.reverse else quanta)]
    on = [a for a in arms if a.name != "off"]
    for arm in arms:   # warm-up: capture, what the first sweeps report
        for _ in range(2):
            for r in recs:
                arm.one(r)
    gate = 0
    for r in recs:     # equality gate: every arm, every sweep
        n = len(r) // 32
        labs = []
        for arm in arms:
            arm.one(r)
            labs.append(arm.lab[:n].copy())
        assert all(np.array_equal(x, labs[0]) for x in labs[1:]), name
        gate += 1
    start = {a.name: a.ctx.callback_path_captures()[0] for a in arms}
    lat = {a.name: [] for a in arms}
    for i in range(args.reps):
        for arm in arms:
            lat[arm.name].append(arm.one(recs[i % len(recs)]) * 1e3)
    thr = {a.name: [] for a in arms}
    for w in range(args.windows):
        for arm in arms:
            thr[arm.name].append(arm.window(recs, args.window))
    lens = [len(c[0]) for c in clouds]
    res = {"points_min": min(lens), "points_max": max(lens), "distinct_lengths": len(set(lens)), "sweeps_in_gate": gate,
           "sweeps_timed_per_arm": args.reps + args.windows * args.window,
           "n_captured_while_timed": {a.name: a.ctx.callback_path_captures()[0] - start[a.name] for a in arms},
           "n_resident": {a.name: a.ctx.callback_path_captures()[1] for a in arms},
           "latency_ms_one_in_flight": {k: stats(v) for k, v in lat.items()},
           "sweeps_per_s_four_in_flight": {k: stats(v) for k, v in thr.items()},
           "arms_in_order": [a.name for a in arms],
           "latency_ratio_off_over": {a.name: stats(np.array(lat["off"]) / np.array(lat[a.name])) for a in on},
           "throughput_ratio_over_off": {a.name: stats(np.array(thr[a.name]) / np.array(thr["off"])) for a in on}}
    res["outcome"] = {a.name: {"latency": verdict(res["latency_ratio_off_over"][a.name]),
                               "throughput": verdict(res["throughput_ratio_over_off"][a.name])} for a in on}
    for arm in arms:
        arm.ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=12)
    ap.add_argument("--window", type=int, default=64)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reverse", action="store_true", help="create and run the arms in the opposite order (the switch first): a check on what the order costs")
    args = ap.parse_args()
    import oracles as O
    import urban_road_filter_amd as u
    from sweep_quantum_cases import records
    p = O.cfg_params("sensor")
    fixed = [O.cfg_cloud("sensor", s) for s in range(1, 17)]
    dense = []
    for x, y, z in fixed:   # the drop-outs: whatever no region of interest keeps
        keep = np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & ~((x == 0) & (y == 0) & (z == 0))
        dense.append(tuple(np.ascontiguousarray(a[keep]) for a in (x, y, z)))
    out = {"tool": "tools/sweep_lengths_bench.py", "reps": args.reps, "windows": args.windows, "window": args.window,
           "untimed": "a C client (the figures include ctypes / numpy per call); records in urf_pinned_input's buffer; quanta between 2048 and 16384"}
    out["dense64"] = workload(u, records, "dense64", dense, p, (0, 2048, 16384), args)
    out["fixed64"] = workload(u, records, "fixed64", fixed, p, (0, 2048), args)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
