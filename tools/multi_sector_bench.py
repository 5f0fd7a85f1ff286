#!/usr/bin/env python3
"""tools/multi_sector_bench.py -- urf_set_front_multi_sector on against off, measured on one MI355X.
Prints ONE JSON line; recorded under profiles/front_multi_sector_bench.json.

    timeout 900 python tools/multi_sector_bench.py [--scans 1024] [--steps 20] [--warmup 3] [--distinct 32]
    timeout 900 python tools/multi_sector_bench.py --curb-points 3,8     (urf_set_front_multi_sector_curb_points on against off, see below;
                                                                          recorded under profiles/front_multi_sector_cp_bench.json)
    rocprofv3 --kernel-trace --stats -- python tools/multi_sector_bench.py --trace-only   (k_front_sectors' own time: a run of its own)

Workloads (tests/sensor_models.py), --scans resident sweeps each, --distinct distinct ones repeated:
  hdl64e_firing   the HDL-64E's geometry (azimuth offsets per laser: every firing in four sectors) at 2048 firings, firing order
  ideal64_firing  its ideal twin (one sector per firing): what the switch costs a sweep that does not need it
  os64_rows       an Ouster's staggered cloud, row-major 64 x 1024
  ideal64_rows    its ideal twin
Behind a label gate against oracle B (tests/oracles.py) two contexts in front mode 2 -- the switch on, the switch off -- are timed with
device events, interleaved call by call.  Per side: the 10th / 50th / 90th percentiles of ms per call, the per-pair ratio off / on,
urf_front_scans (after the warm-up and after the timed calls) next to the number of scans tests/front_shape.py's predicate accepts; then, with urf_enable_kernel_timing, the context's per-stage event brackets of both (the bracket named k_split holds the
march, k_front_sectors and the general split).

--curb-points LIST (default: none, the run above, unchanged): per workload and per value of the list, curbPoints set to it, BOTH contexts in
front mode 3 with urf_set_front_multi_sector on; urf_set_front_multi_sector_curb_points is on in one and off in the other, so that "off" is
what that parameter gets without the new switch.  Same label gate, same interleaving, same figures per (workload, curbPoints)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WORKLOADS = (("hdl64e_firing", "hdl64e", 2048, "firing"), ("ideal64_firing", "ideal64", 2048, "firing"),
             ("os64_rows", "os64", 1024, "rows"), ("ideal64_rows", "ideal64", 1024, "rows"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=32, help="distinct sweeps the batch is built from")
    ap.add_argument("--workloads", default=",".join(w[0] for w in WORKLOADS))
    ap.add_argument("--curb-points", default="", help="comma-separated curbPoints (1..4, 6..8): time urf_set_front_multi_sector_curb_points instead")
    ap.add_argument("--trace-only", action="store_true", help="five calls of the switch-on context per workload, for a kernel trace")
    args = ap.parse_args()
    import torch
    import urban_road_filter_amd as u
    import front_shape as FS
    import oracles as O
    import sensor_models as SM
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured here")
    dev = torch.device("cuda:0")
    S = args.scans
    cps = [int(v) for v in args.curb_points.split(",") if v]
    if any(cp not in (1, 2, 3, 4, 6, 7, 8) for cp in cps):
        raise SystemExit("--curb-points: values of 1..4 and 6..8")
    # (switch under test, front mode of both contexts): without --curb-points the run recorded in profiles/front_multi_sector_bench.json
    mode = 3 if cps else 2
    out = {"metric": "front_multi_sector_cp_bench" if cps else "front_multi_sector_bench", "device": torch.cuda.get_device_name(0), "scans": S,
           "front_mode": mode, "timing": "device events per call, off / on interleaved call by call in one process; ms", "results": []}
    if cps:
        out["switch"] = "urf_set_front_multi_sector_curb_points (urf_set_front_multi_sector on in both contexts)"
    t0 = time.time()
    st = torch.cuda.Stream()
    pct = lambda v: [float(np.percentile(v, q)) for q in (10, 50, 90)]  # noqa: E731
    with torch.cuda.stream(st):
        for name, model, W, layout, cp in [w + (cp,) for w in WORKLOADS for cp in (cps or [None])]:
            if name not in args.workloads.split(","):
                continue
            L = SM.lasers(model)
            p = SM.params_for(model, wide=True)
            if cp is not None:
                p.curbPoints = cp
            k_distinct = min(args.distinct, S)
            # (start 0: the seam on a tile border, so that the ideal twins are fused with the switch off)
            clouds = [SM.sweep(model, firings=W, world=k % 3, seed=700 + k, noise=model != "ideal64", layout=layout) for k in range(k_distinct)]
            order = [k % k_distinct for k in range(S)]
            n = W * L
            dx, dy, dz = (torch.from_numpy(np.concatenate([clouds[k][j] for k in order])).to(dev) for j in range(3))
            labs = {"on": torch.empty(S * n, dtype=torch.uint8, device=dev), "off": torch.empty(S * n, dtype=torch.uint8, device=dev)}
            gate = sorted({0, 1, S - 1})
            want = {k: O.run_b(*clouds[order[k]], p)[0] for k in gate}
            # what the rules the switch leaves in force accept (tests/front_shape.py, from oracle B's stages): the bound of front_scans
            ok = [bool(FS.fusable(c, p, layout)) for c in clouds]
            fusable = sum(ok[k] for k in order)
            with u.Context(n, S, params=p) as on, u.Context(n, S, params=p) as off:
                ctxs = {"on": on, "off": off}
                for side, ctx in ctxs.items():
                    ctx.set_stream(st.cuda_stream)
                    ctx.set_front_mode(mode)
                    ctx.set_front_multi_sector(1 if side == "on" or cps else 0)
                    ctx.set_front_multi_sector_curb_points(1 if side == "on" and cps else 0)
                calls = {side: (lambda c=ctx, lab=labs[side]: c.classify_batch_soa(dx, dy, dz, n, S, lab, None)) for side, ctx in ctxs.items()}
                if args.trace_only:
                    for _ in range(5):
                        calls["on"]()
                    torch.cuda.synchronize()
                    continue
                fused = {}
                for side in ("off", "on"):   # the label gate and the warm-up (a row-major layout is sighted by the first call)
                    for _ in range(max(3, args.warmup)):
                        calls[side]()
                        torch.cuda.synchronize()   # (the policy reads what a call reported once that call has finished: a sighting is acted on by the next)
                    fused[side] = int(ctxs[side].front_scans())
                    got = labs[side].cpu().numpy()
                    for k, lb in want.items():
                        if not np.array_equal(got[k * n:(k + 1) * n], lb):
                            raise SystemExit("label gate: %s%s side %s scan %d differs from oracle B" % (name, " curbPoints %d" % cp if cps else "", side, k))
                ts = {"on": [], "off": []}
                for _ in range(args.steps):
                    for side in ("off", "on"):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        calls[side]()
                        e1.record()
                        e1.synchronize()
                        ts[side].append(e0.elapsed_time(e1))
                fused_after = {side: int(ctx.front_scans()) for side, ctx in ctxs.items()}
                stages = {}
                for side, ctx in ctxs.items():   # (brackets on: everything on one stream, so they add up to the call)
                    ctx.enable_kernel_timing(True)
                    for _ in range(5):
                        calls[side]()
                    torch.cuda.synchronize()
                    ms, n_calls = ctx.kernel_timing()
                    stages[side] = {k: v / max(n_calls, 1) for k, v in ms.items()}
                    ctx.enable_kernel_timing(False)
                out["results"].append({"workload": name, **({"curbPoints": cp} if cps else {}), "model": model, "lasers": L, "firings": W, "layout": layout, "points": S * n,
                                       "front_scans": fused, "front_scans_after_timing": fused_after, "fusable_scans": fusable, "off_ms_p10_p50_p90": pct(ts["off"]), "on_ms_p10_p50_p90": pct(ts["on"]),
                                       "off_over_on_p10_p50_p90": pct([a / b for a, b in zip(ts["off"], ts["on"])]),
                                       "stage_brackets_ms_per_call": stages})
            del dx, dy, dz, labs
            torch.cuda.empty_cache()
    out["wall_s"] = time.time() - t0
    print(json.dumps(out))


if __name__ == "__main__":
    main()
