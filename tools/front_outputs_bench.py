#!/usr/bin/env python3
"""tools/front_outputs_bench.py -- what the published order and the marker points cost behind a fused batch call, with and without
urf_set_front_outputs, measured on one MI355X.  Prints ONE JSON line.

    python tools/front_outputs_bench.py [--scans 1024] [--repeats 7] [--warmup 3]

S synthetic 64 x 2048 street sweeps in firing order (scenes 1 and 2 alternating), resident, front mode 2.  One round = one
urf_classify_batch_soa + urf_ordered_indices_batch + urf_marker_points_batch, device events around the round and around its classify call,
median of --repeats after --warmup, all variants in one process one after the other:
  (a) switch_off   today's path: the read-outs run the fused call again through the general kernels, and urf_set_front_mode(2) before every
                   round makes the next call fused again (without it every later call takes the general kernels: variant a_sticky)
  (b) switch_on    urf_set_front_outputs(ctx, 1): the read-outs take the fused call as it is
  (c) mode_0       the same read-outs on a context that never takes the fused kernels
  fused_classify_only_ms   a fused call without read-outs, for the classify call that follows the read-outs of (b)
A parity gate runs first: lists and marker points of (b) equal those of (c), every scan.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_PTS = 64 * 2048


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    import urban_road_filter_amd as u
    import oracles as O
    from batch_clouds_bench import gen
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured here")
    S, dev = args.scans, torch.device("cuda:0")
    p = O.cfg_params("cfg2")
    scans = gen((S + 1) // 2, 1, 1, False) + gen(S // 2, 2, 1, False)
    scans = [scans[(s // 2) + (0 if s % 2 == 0 else (S + 1) // 2)] for s in range(S)]
    out = {"metric": "front_outputs", "device": torch.cuda.get_device_name(0), "scans": S, "repeats": args.repeats, "warmup": args.warmup,
           "timing": "device events around classify + ordered_indices_batch + marker_points_batch, median"}
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        xyz = [torch.from_numpy(np.concatenate([s[k] for s in scans])).to(dev) for k in range(3)]
        labels = torch.empty(S * N_PTS, dtype=torch.uint8, device=dev)
        lists = [torch.empty(S * N_PTS, dtype=torch.int32, device=dev) for _ in range(3)]
        d_cnt = torch.empty(3 * S, dtype=torch.int32, device=dev)
        d_pts = torch.empty(S * u.MARKER_MAX_POINTS * 4, dtype=torch.float32, device=dev)
        d_n = torch.empty(S, dtype=torch.int32, device=dev)
        results = {}

        def variant(name, mode, switch, remode, readouts=True):
            with u.Context(N_PTS, S, params=p) as ctx:
                ctx.set_stream(st.cuda_stream)
                ctx.set_front_mode(mode)
                ctx.set_front_outputs(switch)
                total, first, fused = [], [], []
                for _ in range(args.warmup + args.repeats):
                    if remode:
                        ctx.set_front_mode(mode)
                    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                    e[0].record()
                    ctx.classify_batch_soa(xyz[0], xyz[1], xyz[2], N_PTS, S, labels)
                    e[1].record()
                    if readouts:
                        ctx.ordered_indices_batch(lists[0], lists[1], lists[2], N_PTS, d_cnt)
                        ctx.marker_points_batch(d_pts, d_n)
                    e[2].record()
                    torch.cuda.synchronize()
                    total.append(e[0].elapsed_time(e[2]))
                    first.append(e[0].elapsed_time(e[1]))
                    fused.append(ctx.front_scans())
                w = args.warmup
                out[name] = {"round_ms": statistics.median(total[w:]), "round_ms_runs": total[w:], "classify_ms": statistics.median(first[w:]),
                             "front_scans_after_round": fused[-1]}
                if readouts:
                    results[name] = [t.cpu().numpy().copy() for t in lists + [d_cnt, d_pts, d_n]]

        variant("c_mode_0", 0, 0, False)
        variant("a_switch_off", 2, 0, True)
        variant("a_sticky_switch_off", 2, 0, False)
        variant("b_switch_on", 2, 1, False)
        variant("fused_classify_only", 2, 1, False, readouts=False)
    # parity: (b) against (c), every scan
    rb, rc = results["b_switch_on"], results["c_mode_0"]
    cb, cc = rb[3].reshape(S, 3), rc[3].reshape(S, 3)
    assert np.array_equal(cb, cc) and np.array_equal(rb[5], rc[5])
    for s in range(S):
        for k in range(3):
            assert np.array_equal(rb[k].reshape(S, N_PTS)[s, :cb[s, k]], rc[k].reshape(S, N_PTS)[s, :cc[s, k]]), (s, k)
        n = int(rb[5][s])
        assert rb[4].reshape(S, -1)[s, :4 * n].tobytes() == rc[4].reshape(S, -1)[s, :4 * n].tobytes(), s
    out["parity"] = "switch on equals mode 0, every scan"
    out["a_ms"], out["b_ms"], out["c_ms"] = out["a_switch_off"]["round_ms"], out["b_switch_on"]["round_ms"], out["c_mode_0"]["round_ms"]
    out["fused_classify_only_ms"] = out["fused_classify_only"]["classify_ms"]
    out["classify_after_readouts_ms"] = out["b_switch_on"]["classify_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
