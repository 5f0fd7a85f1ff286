#!/usr/bin/env python3
"""tools/front_auto_bench.py -- urf_set_front_auto against the switches set by hand, measured on one MI355X.
Prints ONE JSON line; recorded under profiles/front_auto_bench.json.

    timeout 900 python tools/front_auto_bench.py [--scans 1024] [--steps 20] [--distinct 32] [--workloads LIST]

Workloads (tests/sensor_models.py), --scans resident sweeps each, --distinct distinct ones repeated:
  hdl64e_firing   the HDL-64E's geometry (azimuth offsets per laser) at 2048 firings, firing order
  ideal64_firing  its ideal twin
  os64_rows       an Ouster's staggered cloud, row-major 64 x 1024
  ideal64_rows    its ideal twin
Four arms, each a context of its own in front mode 2, behind a label gate against oracle B (tests/oracles.py):
  a  nothing else set
  b  the switches arm c reports as applied, set by hand
  c  urf_set_front_auto(ctx, 1), timed once it reports URF_AUTO_SETTLED
  d  a second context set exactly as b: b / d shows what the order in which contexts are created does to two arms that are the same
Arm c first makes LEARN_CALLS calls, a synchronisation and a query behind each (a batch whose row-major layout is sighted by its second
call starts over then: the phase is read after all of them, and must have been SETTLED over the last two); b and d then make as many.
The timed calls are interleaved call by call (device events); the whole measurement runs twice, the contexts created in the order
a b c d and d c b a.  Per arm: the 10th / 50th / 90th percentiles of ms per call, and of the per-pair ratios b / c and b / d -- b, c and d
launch the same kernels (front_scans of b and c must agree, or the run stops), so b / c is expected inside the run's own spread and
inside what b / d shows.  The cost of learning is reported separately: the device-event time of arm c's first LEARN_CALLS calls against
arm b's, per call and summed over all of them (`calls`), with `settled_at`, the first call from which every later phase is SETTLED."""
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
LEARN_CALLS = 6
SETTERS = (("LASERS128", "set_front_lasers128"), ("LONG_SWEEPS", "set_front_long_sweeps"), ("CURB_POINTS", "set_front_curb_points"),
           ("MULTI_SECTOR", "set_front_multi_sector"), ("MULTI_SECTOR_CP", "set_front_multi_sector_curb_points"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--distinct", type=int, default=32, help="distinct sweeps the batch is built from")
    ap.add_argument("--workloads", default=",".join(w[0] for w in WORKLOADS))
    args = ap.parse_args()
    import torch
    import urban_road_filter_amd as u
    import oracles as O
    import sensor_models as SM
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured here")
    dev = torch.device("cuda:0")
    S, A, PH = args.scans, u.ADVICE, u.AUTO_PHASE
    out = {"metric": "front_auto_bench", "device": torch.cuda.get_device_name(0), "scans": S, "front_mode": 2,
           "timing": "device events per call, arms interleaved call by call in one process; ms", "results": []}
    t0 = time.time()
    st = torch.cuda.Stream()
    pct = lambda v: [float(np.percentile(v, q)) for q in (10, 50, 90)]  # noqa: E731

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    with torch.cuda.stream(st):
        for name, model, W, layout in WORKLOADS:
            if name not in args.workloads.split(","):
                continue
            L = SM.lasers(model)
            p = SM.params_for(model, wide=True)
            k_distinct = min(args.distinct, S)
            clouds = [SM.sweep(model, firings=W, world=k % 3, seed=700 + k, noise=model != "ideal64", layout=layout) for k in range(k_distinct)]
            order = [k % k_distinct for k in range(S)]
            n = W * L
            dx, dy, dz = (torch.from_numpy(np.concatenate([clouds[k][j] for k in order])).to(dev) for j in range(3))
            gate = sorted({0, 1, S - 1})
            want = {k: O.run_b(*clouds[order[k]], p)[0] for k in gate}
            for arms in ("abcd", "dcba"):
                labs = {arm: torch.empty(S * n, dtype=torch.uint8, device=dev) for arm in arms}
                ctxs = {}
                try:
                    for arm in arms:
                        ctxs[arm] = u.Context(n, S, params=p)
                        ctxs[arm].set_stream(st.cuda_stream)
                        ctxs[arm].set_front_mode(2)
                    calls = {arm: (lambda c=ctxs[arm], lab=labs[arm]: c.classify_batch_soa(dx, dy, dz, n, S, lab, None)) for arm in arms}
                    ctxs["c"].set_front_auto(1)
                    learn, phases, explained = {arm: [] for arm in "bcd"}, [], []
                    for _ in range(LEARN_CALLS):
                        learn["c"].append(timed(calls["c"]))
                        info = ctxs["c"].front_auto()
                        phases.append(int(info["phase"]))
                        explained.append(int(info["explained_calls"]))
                    if phases[-2:] != [PH["SETTLED"]] * 2:
                        raise SystemExit("%s: arm c has not settled: phases %s" % (name, phases))
                    settled_at = 1 + max([k + 1 for k, ph in enumerate(phases) if ph != PH["SETTLED"]], default=0)
                    applied = int(info["applied"])
                    for arm in "bd":   # what c applied, by hand, and their first calls the same way
                        for bit, setter in SETTERS:
                            if applied & A[bit]:
                                getattr(ctxs[arm], setter)(1)
                        ctxs[arm].set_front_mode(3 if applied & A["MODE_3"] else 2)
                        for _ in range(LEARN_CALLS):
                            learn[arm].append(timed(calls[arm]))
                            ctxs[arm].synchronize()
                    for _ in range(3):
                        calls["a"]()
                        torch.cuda.synchronize()
                    fused = {arm: int(ctxs[arm].front_scans()) for arm in arms}
                    if not fused["b"] == fused["c"] == fused["d"]:
                        raise SystemExit("%s: the hand-set arms and auto do not fuse the same scans: %s" % (name, fused))
                    for arm in arms:   # the label gate
                        got = labs[arm].cpu().numpy()
                        for k, lb in want.items():
                            if not np.array_equal(got[k * n:(k + 1) * n], lb):
                                raise SystemExit("label gate: %s arm %s scan %d differs from oracle B" % (name, arm, k))
                    ts = {arm: [] for arm in arms}
                    for _ in range(args.steps):
                        for arm in arms:
                            ts[arm].append(timed(calls[arm]))
                    after = ctxs["c"].front_auto()
                    out["results"].append({
                        "workload": name, "model": model, "lasers": L, "firings": W, "layout": layout, "points": S * n, "contexts_created": arms,
                        "applied_by_c": [k for k, v in A.items() if applied & v], "front_scans": fused,
                        "front_scans_after_timing": {arm: int(ctxs[arm].front_scans()) for arm in arms},
                        **{"%s_ms_p10_p50_p90" % arm: pct(ts[arm]) for arm in "abcd"},
                        "b_over_c_p10_p50_p90": pct([x / y for x, y in zip(ts["b"], ts["c"])]),
                        "b_over_d_p10_p50_p90": pct([x / y for x, y in zip(ts["b"], ts["d"])]),
                        "a_over_c_p10_p50_p90": pct([x / y for x, y in zip(ts["a"], ts["c"])]),
                        "learning": {"calls": LEARN_CALLS, "settled_at": settled_at, "phases": phases, "explained_calls": explained,
                                     "c_ms_per_call": learn["c"], "b_ms_per_call": learn["b"], "d_ms_per_call": learn["d"],
                                     "c_minus_b_ms_total": float(sum(learn["c"]) - sum(learn["b"])),
                                     "d_minus_b_ms_total": float(sum(learn["d"]) - sum(learn["b"]))},
                        "explained_calls_after_timing": int(after["explained_calls"]), "phase_after_timing": int(after["phase"])})
                finally:
                    for ctx in ctxs.values():
                        ctx.close()
                    del labs
                    torch.cuda.empty_cache()
            del dx, dy, dz
            torch.cuda.empty_cache()
    out["wall_s"] = time.time() - t0
    print(json.dumps(out))


if __name__ == "__main__":
    main()
