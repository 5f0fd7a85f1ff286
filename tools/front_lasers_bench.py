#!/usr/bin/env python3
"""tools/front_lasers_bench.py -- the fused front end on sweeps of 16 / 32 / 64 lasers per firing, measured on one MI355X.
Prints ONE JSON line.

    timeout 900 python tools/front_lasers_bench.py [--scans 1024] [--steps 20] [--warmup 3] [--lasers 16,32,64] [--no-sweep]

For L in --lasers and storage order in {firing, rows}: --scans resident L x 2048 sweeps from urf_synth_cloud(L, 2048, scene 1 and 3
alternating, seed), params.channels = L.  First a parity gate: the labels of a few sampled scans against oracle B (tests/oracles.py).
Then urf_set_front_mode 0 and 2, warm-up, --steps calls between device events: median ms per call, scans/s, urf_front_scans.
"sweep": mode 0 / 1 / 2 over batch sizes 32 .. 1024 of the firing-order sweeps, the numbers mode 1's threshold per laser count
(urf_front.hpp: urf_front_min_scans) is set from.  Uses only entry points every build since the fused front end has.

    timeout 900 python tools/front_lasers_bench.py --lasers128 [--scans 256] [--steps 20] [--warmup 3]

128 lasers per firing (urf_set_front_lasers128, k_front128* in urf_front.hpp): --scans resident 128 x 2048 and 128 x 1024 sweeps (channels = 128,
interval = 0.05), firing order and row-major, in TWO contexts of one process, both in front mode 2 -- one with the switch on, one with it
off: the same binary's general kernels, the baseline -- timed interleaved call by call (on, off, on, off, ...), behind a label gate
against oracle B for both.  Per case: the medians, the 10th / 90th percentiles of either side (the run's own spread) and the median and
percentiles of the per-pair ratio off / on.  Recorded under profiles/front_lasers128_bench.json.

    timeout 900 python tools/front_lasers_bench.py --lasers128 --cols 4096 [--scans 256]

--brackets: per case also the per-kernel event brackets of the fused call (mode 2; --lasers128: the "on" context), ms per call: what
profiles/front_one_finish.md compares between two builds (URF_LIB_PATH selects the library), process by process.

--cols W: sweeps of W columns instead (both modes; default 2048, with --lasers128 2048 and 1024).  Above 2048 columns a 128-laser sweep
has more than 128 tiles: the "on" context then also turns urf_set_front_long_sweeps on, "off" stays the general kernels, and "brackets"
holds the per-kernel event brackets (urf_enable_kernel_timing; the fused finish step runs inside "k_ring") of the "on" side at W and at
2048 columns, ms per call, in the same process.  Recorded under profiles/front_long_bench.json."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def brackets(ctx, call, steps):
    """--brackets: the fused call kernel by kernel -- the event brackets of urf_enable_kernel_timing, ms per call (the fused finish step runs
    inside "k_ring", k_label_front inside "k_label", k_transpose inside "k_split", k_rows_probe inside "k_ring_table")."""
    ctx.enable_kernel_timing(True)
    for _ in range(steps):
        call()
    ms, calls = ctx.kernel_timing()
    ctx.enable_kernel_timing(False)
    return {k: v / calls for k, v in ms.items()}


def lasers128(args):
    import torch
    import urban_road_filter_amd as u
    import oracles as O
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured here")
    L, S = 128, args.scans if args.scans != 1024 else 256
    dev = torch.device("cuda:0")
    out = {"metric": "front_lasers128", "device": torch.cuda.get_device_name(0), "scans": S, "front_mode": 2,
           "timing": "device events per call, switch on / off interleaved call by call in one process; ms", "results": []}
    t0 = time.time()
    st = torch.cuda.Stream()
    p = u.default_params().wide_roi()
    p.channels = L
    p.interval = 0.05
    pct = lambda v: [float(np.percentile(v, q)) for q in (10, 50, 90)]
    with torch.cuda.stream(st):
        for cols in ((2048, 1024) if args.cols is None else (args.cols,)):
            n = L * cols
            long = n > 128 * 2048   # more than 128 tiles: urf_set_front_long_sweeps
            base = [u.synth_cloud(L, cols, 1 + (s % 2) * 2, 100 + s) for s in range(min(args.distinct, S))]
            for order in ("firing", "rows"):
                src = base if order == "firing" else [tuple(np.ascontiguousarray(a.reshape(-1, L).T.reshape(-1)) for a in c) for c in base]
                one = [torch.from_numpy(np.concatenate([c[k] for c in src])).to(dev) for k in range(3)]
                reps = (S + len(src) - 1) // len(src)
                dx, dy, dz = (t.repeat(reps)[:S * n].contiguous() for t in one)
                labels = torch.empty(S * n, dtype=torch.uint8, device=dev)
                want = {k: O.run_b(*src[k % len(src)], p)[0] for k in (0, 1, S - 1)}
                with u.Context(n, S, params=p) as on, u.Context(n, S, params=p) as off:
                    ctxs = {"on": on, "off": off}
                    fused = {}
                    for name, ctx in ctxs.items():
                        ctx.set_stream(st.cuda_stream)
                        ctx.set_front_lasers128(1 if name == "on" else 0)
                        if long:
                            ctx.set_front_long_sweeps(1 if name == "on" else 0)
                        ctx.set_front_mode(2)
                        for call in range(max(3, args.warmup)):   # the label gate (row-major: the first call sights the layout), and the warm-up
                            ctx.classify_batch_soa(dx, dy, dz, n, S, labels, None)
                            torch.cuda.synchronize()
                            got = labels.cpu().numpy().reshape(S, n)
                            for k, lb in want.items():
                                if not np.array_equal(got[k], lb):
                                    raise SystemExit("label gate: 128 x %d %s switch %s call %d scan %d differs from oracle B" % (cols, order, name, call, k))
                        fused[name] = int(ctx.front_scans())
                    ts = {"on": [], "off": []}
                    for _ in range(args.steps):
                        for name, ctx in ctxs.items():
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record()
                            ctx.classify_batch_soa(dx, dy, dz, n, S, labels, None)
                            e1.record()
                            e1.synchronize()
                            ts[name].append(e0.elapsed_time(e1))
                    ratio = [b / a for a, b in zip(ts["on"], ts["off"])]
                    out["results"].append({"cols": cols, "order": order, "on_front_scans": fused["on"], "off_front_scans": fused["off"],
                                           "on_ms_p10_p50_p90": pct(ts["on"]), "off_ms_p10_p50_p90": pct(ts["off"]),
                                           "off_over_on_p10_p50_p90": pct(ratio)})
                    if args.brackets:
                        out["results"][-1]["on_brackets_ms"] = brackets(on, lambda: on.classify_batch_soa(dx, dy, dz, n, S, labels, None), args.steps)
            if long:   # the fused call kernel by kernel, at `cols` and at 2048 columns (firing order)
                out["brackets"] = []
                for bc in (cols, 2048):
                    bn = L * bc
                    src = [u.synth_cloud(L, bc, 1 + (s % 2) * 2, 100 + s) for s in range(min(args.distinct, S))]
                    one = [torch.from_numpy(np.concatenate([c[k] for c in src])).to(dev) for k in range(3)]
                    reps = (S + len(src) - 1) // len(src)
                    dx, dy, dz = (t.repeat(reps)[:S * bn].contiguous() for t in one)
                    labels = torch.empty(S * bn, dtype=torch.uint8, device=dev)
                    with u.Context(bn, S, params=p) as ctx:
                        ctx.set_stream(st.cuda_stream)
                        ctx.set_front_lasers128(1)
                        ctx.set_front_long_sweeps(1)
                        ctx.set_front_mode(2)
                        for _ in range(max(3, args.warmup)):
                            ctx.classify_batch_soa(dx, dy, dz, bn, S, labels, None)
                        torch.cuda.synchronize()
                        ctx.enable_kernel_timing(True)
                        for _ in range(args.steps):
                            ctx.classify_batch_soa(dx, dy, dz, bn, S, labels, None)
                        ms, calls = ctx.kernel_timing()
                        out["brackets"].append({"cols": bc, "front_scans": int(ctx.front_scans()), "calls": int(calls),
                                                "ms_per_call": {k: v / calls for k, v in ms.items()}})
    out["wall_s"] = time.time() - t0
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lasers", default="16,32,64")
    ap.add_argument("--distinct", type=int, default=32, help="distinct sweeps the batch is built from")
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--cols", type=int, default=None, help="columns per sweep (default 2048; --lasers128: 2048 and 1024)")
    ap.add_argument("--brackets", action="store_true", help="also the fused call's per-kernel event brackets (urf_enable_kernel_timing), ms per call")
    ap.add_argument("--lasers128", action="store_true", help="the 128-laser switch on against off, two contexts interleaved")
    args = ap.parse_args()
    if args.lasers128:
        return lasers128(args)
    import torch
    import urban_road_filter_amd as u
    import oracles as O
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured here")
    COLS = args.cols if args.cols is not None else 2048
    dev = torch.device("cuda:0")
    out = {"metric": "front_lasers", "device": torch.cuda.get_device_name(0), "scans": args.scans, "cols": COLS,
           "timing": "device events, median ms per call after warm-up", "results": [], "sweep": []}
    t0 = time.time()
    st = torch.cuda.Stream()

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts))

    with torch.cuda.stream(st):
        for L in [int(v) for v in args.lasers.split(",")]:
            n = L * COLS
            p = u.default_params().wide_roi()
            p.channels = L
            base = [u.synth_cloud(L, COLS, 1 + (s % 2) * 2, 100 + s) for s in range(min(args.distinct, args.scans))]
            for order in ("firing", "rows"):
                src = base if order == "firing" else [tuple(np.ascontiguousarray(a.reshape(-1, L).T.reshape(-1)) for a in c) for c in base]
                one = [torch.from_numpy(np.concatenate([c[k] for c in src])).to(dev) for k in range(3)]
                reps = (args.scans + len(src) - 1) // len(src)
                dx, dy, dz = (t.repeat(reps)[:args.scans * n].contiguous() for t in one)
                labels = torch.empty(args.scans * n, dtype=torch.uint8, device=dev)
                with u.Context(n, args.scans, params=p) as ctx:
                    ctx.set_stream(st.cuda_stream)
                    # parity gate: both modes, a few sampled scans
                    want = {k: O.run_b(*src[k % len(src)], p)[0] for k in (0, 1, args.scans - 1)}
                    for mode in (0, 2, 2):
                        ctx.set_front_mode(mode)
                        ctx.classify_batch_soa(dx, dy, dz, n, args.scans, labels, None)
                        torch.cuda.synchronize()
                        got = labels.cpu().numpy().reshape(args.scans, n)
                        for k, lb in want.items():
                            if not np.array_equal(got[k], lb):
                                raise SystemExit("parity gate: L %d %s mode %d scan %d differs from oracle B" % (L, order, mode, k))
                    row = {"lasers": L, "order": order}
                    for mode in (0, 2):
                        ctx.set_front_mode(mode)
                        ms = timed(lambda: ctx.classify_batch_soa(dx, dy, dz, n, args.scans, labels, None))
                        row["mode%d_ms" % mode] = ms
                        row["mode%d_scans_per_s" % mode] = args.scans / ms * 1e3
                        row["mode%d_front_scans" % mode] = int(ctx.front_scans())
                    if args.brackets:   # (mode 2 is the one set last)
                        row["mode2_brackets_ms"] = brackets(ctx, lambda: ctx.classify_batch_soa(dx, dy, dz, n, args.scans, labels, None), args.steps)
                    out["results"].append(row)
                    if order == "firing" and not args.no_sweep:
                        for S in (32, 64, 128, 192, 256, 384, 512, 768, 1024):
                            if S > args.scans:
                                break
                            r = {"lasers": L, "scans": S}
                            for mode in (0, 1, 2):
                                ctx.set_front_mode(mode)
                                r["mode%d_ms" % mode] = timed(lambda: ctx.classify_batch_soa(dx, dy, dz, n, S, labels, None))
                                r["mode%d_front_scans" % mode] = int(ctx.front_scans())
                            out["sweep"].append(r)
    out["wall_s"] = time.time() - t0
    print(json.dumps(out))


if __name__ == "__main__":
    main()
