#!/usr/bin/env python3
"""tools/batch_clouds_bench.py -- ragged PointCloud2 batches and the published clouds of a batch on the device
(urf_classify_batch_pc2_ragged, urf_clouds_batch_pc2), measured on one MI355X.  Prints ONE JSON line.

    python tools/batch_clouds_bench.py [--scans 1024] [--steps 20] [--warmup 3] [--parity-scans 3] [--profile] [--front-outputs]

Workload 1 (cfg3): S synthetic 64 x 2048 street sweeps (scene 1), resident, as 32-byte pcl::PointXYZI PointCloud2 records
with intensity.  Timed with device events after warm-up, mean per call:
  classify_pc2_ms / classify_pc2_ragged_ms   the same records through urf_classify_batch_pc2 and, with offsets s * 131072,
                                             urf_classify_batch_pc2_ragged
  clouds_input_ms / clouds_reference_ms      urf_clouds_batch_pc2 in both orders after a PointCloud2 call (the reference order's
                                             first call runs the fused batch once more through the general kernels: warm-up)
  clouds_input_nt_ms                         input order with non-temporal record stores (test hook, liburf_hip_test.so)
Bytes the algorithm moves, from the counts: labels read twice (count and write pass), one source record per ROI point, 32 B per
output record; the reference order adds one 4-byte list entry per gathered record and leaves its ordering kernels
(k_ring_order, k_ordered_lists) uncounted.  GB/s = bytes / call time; share of the 8 TB/s HBM peak.
Workload 2: S sensor-like sweeps (scene 3) with their drop-outs removed (every message has another length), 32-byte records.
A parity gate runs first: the records of --parity-scans sampled scans of each workload against the CPU oracle (tests/oracles.py).
--front-outputs: urf_set_front_outputs(ctx, 1) -- the reference order takes the fused batch as it is (no second run, the context stays
fused; the flag also adds classify_after_reference_ms, the classify call behind that read-out, and front_scans_after_reference).
Without the flag the tool does what it did before the flag existed.
--profile: only a few calls of each, for `rocprofv3 --kernel-trace --stats` (per-kernel times come from that run, not this one).
"""
import argparse
import concurrent.futures as cf
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

RINGS, COLS = 64, 2048
N_PTS = RINGS * COLS
STEP = 32
PEAK_BPS = 8.0e12
NT_FLAG = 16   # urf_set_debug_flags bit: non-temporal record stores (urf_api.hip: URF_DBG_CLOUDS_NT)


def gen(n_scans, scene, seed0, drop):
    import urban_road_filter_amd as u
    out = [None] * n_scans

    def one(s):
        x, y, z = u.synth_cloud(RINGS, COLS, scene, seed0 + s)
        if drop:
            keep = ~((x == 0) & (y == 0) & (z == 0))
            x, y, z = x[keep], y[keep], z[keep]
        out[s] = (x, y, z)

    with cf.ThreadPoolExecutor(max_workers=16) as ex:
        list(ex.map(one, range(n_scans)))
    return out


def intensity(n_total):
    return (np.arange(n_total) % 251).astype(np.float32) * 0.5 + 1.0


def expected_records(x, y, z, inten, p):
    """oracle B's four clouds of one scan in input order: counts [4], records uint32 [k, 8]"""
    import oracles as O
    lb, ib, _ = O.run_b(x, y, z, p)
    if ib["status"] != 0:
        return [0, 0, 0, 0], np.zeros((0, 8), np.uint32)
    r = np.zeros((len(x), 8), np.uint32)
    for k, a in enumerate((x, y, z, None, inten)):
        if a is not None:
            r[:, k] = np.ascontiguousarray(a, np.float32).view(np.uint32)
    r[:, 3] = 0x3F800000
    idx = [np.nonzero((lb & 3) == 1)[0], np.nonzero((lb & 3) == 2)[0], np.nonzero(lb & 4)[0], np.nonzero(lb & 16)[0]]
    return [len(i) for i in idx], np.concatenate([r[i] for i in idx])


def run_workload(torch, u, ctx, scans, p, args, name, ragged_only):
    dev = torch.device("cuda:0")
    S = len(scans)
    lens = np.array([len(s[0]) for s in scans], np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    total, max_len = int(offs[-1]), int(lens.max())
    # the records, built on the device: x y z w=1 intensity 0 0 0
    rec_in = torch.zeros((total, 8), dtype=torch.float32, device=dev)
    for k in range(3):
        rec_in[:, k] = torch.from_numpy(np.concatenate([s[k] for s in scans])).to(dev)
    rec_in[:, 3] = 1.0
    inten = intensity(total)
    rec_in[:, 4] = torch.from_numpy(inten).to(dev)
    d_off = torch.from_numpy(offs.astype(np.int32)).to(dev)
    labels = torch.empty(total, dtype=torch.uint8, device=dev)
    info = torch.empty((S, 8), dtype=torch.int32, device=dev)
    cap = 3 * S * max_len
    d_rec = torch.empty((cap, 8), dtype=torch.float32, device=dev)
    d_cnt = torch.empty(4 * S, dtype=torch.int32, device=dev)
    d_offs = torch.empty(4 * S, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def classify_fixed():
        ctx.classify_batch_pc2(rec_in, max_len, S, STEP, 0, 4, 8, labels, info)

    def classify_ragged():
        ctx.classify_batch_pc2_ragged(rec_in, d_off, total, max_len, S, STEP, 0, 4, 8, labels, info)

    def clouds(order):
        return lambda: ctx.clouds_batch_pc2(rec_in, STEP, 0, 4, 8, 16, order, d_rec, cap, d_cnt, d_offs)

    def timed(fn, steps, warmup):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps

    res = {"scans": S, "points": total, "max_len": max_len, "lengths_distinct": int(len(np.unique(lens)))}
    classify = classify_ragged if ragged_only else classify_fixed
    # parity gate: sampled scans against the CPU oracle, input order
    classify()
    clouds(u.ORDER_INPUT)()
    torch.cuda.synchronize()
    cnt = d_cnt.cpu().numpy().astype(np.int64).reshape(S, 4)
    off = d_offs.cpu().numpy().reshape(S, 4)
    rng = np.random.default_rng(5)
    sample = sorted(set([0, S - 1] + list(rng.choice(S, max(0, args.parity_scans - 2), replace=False))))[:max(args.parity_scans, 1)]
    for s in sample:
        x, y, z = scans[s]
        want_cnt, want = expected_records(x, y, z, inten[offs[s]:offs[s + 1]], p)
        assert list(cnt[s]) == want_cnt, (name, s, list(cnt[s]), want_cnt)
        got = d_rec[int(off[s][0]):int(off[s][0]) + len(want)].cpu().numpy().view(np.uint32)
        assert np.array_equal(got, want), (name, s)
    res["parity_checked_scans"] = [int(s) for s in sample]
    if args.profile:
        for fn in (classify_fixed if not ragged_only else None, classify_ragged, clouds(u.ORDER_INPUT), clouds(u.ORDER_REFERENCE)):
            if fn:
                timed(fn, 2, 1)
        return res
    steps, warmup = args.steps, args.warmup
    if not ragged_only:
        res["classify_pc2_ms"] = timed(classify_fixed, steps, warmup)
    res["classify_pc2_ragged_ms"] = timed(classify_ragged, steps, warmup)
    if not ragged_only:   # (the clouds below read the fixed-length call's labels: the same)
        classify_fixed()
    ctx_nt = [0, NT_FLAG] if u.lib(hooks=True) is ctx._lib else [0]
    t_in = {f: [] for f in ctx_nt}
    for rep in range(3):   # alternate plain / non-temporal stores
        for f in ctx_nt:
            if len(ctx_nt) > 1:
                ctx.set_debug_flags(f)
            t_in[f].append(timed(clouds(u.ORDER_INPUT), steps, warmup))
    if len(ctx_nt) > 1:
        ctx.set_debug_flags(0)
    res["clouds_input_ms"] = float(np.median(t_in[0]))
    if NT_FLAG in t_in:
        res["clouds_input_nt_ms"] = float(np.median(t_in[NT_FLAG]))
        res["clouds_input_ms_runs"] = t_in[0]
        res["clouds_input_nt_ms_runs"] = t_in[NT_FLAG]
    res["clouds_reference_ms"] = timed(clouds(u.ORDER_REFERENCE), steps, warmup)
    if args.front_outputs:   # the classify call behind the read-out stays fused: timed, then the state the counts below are read from again
        res["classify_after_reference_ms"] = timed(classify, steps, warmup)
        res["front_scans_after_reference"] = ctx.front_scans()
        clouds(u.ORDER_REFERENCE)()
    cnt = d_cnt.cpu().numpy().astype(np.int64).reshape(S, 4)
    n_rec = int(cnt.sum())
    n_roi = int(cnt[:, 2].sum())
    gathered = int(cnt[:, 0].sum() + cnt[:, 1].sum() + cnt[:, 3].sum())
    b_in = 2 * total + STEP * n_roi + 32 * n_rec
    b_ref = b_in + 4 * gathered
    res.update({"records": n_rec, "roi_points": n_roi,
                "bytes_input_order": b_in, "bytes_reference_order": b_ref,
                "gbps_input_order": b_in / res["clouds_input_ms"] / 1e6,
                "peak_share_input_order": b_in / (res["clouds_input_ms"] * 1e-3) / PEAK_BPS,
                "gbps_reference_order": b_ref / res["clouds_reference_ms"] / 1e6,
                "peak_share_reference_order": b_ref / (res["clouds_reference_ms"] * 1e-3) / PEAK_BPS})
    if "clouds_input_nt_ms" in res:
        res["gbps_input_order_nt"] = b_in / res["clouds_input_nt_ms"] / 1e6
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parity-scans", type=int, default=3)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--front-outputs", action="store_true")
    args = ap.parse_args()
    import torch
    import urban_road_filter_amd as u
    import oracles as O
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured here")
    p = O.cfg_params("cfg2")
    t0 = time.time()
    out = {"metric": "batch_clouds", "device": torch.cuda.get_device_name(0), "timing": "device events, mean per call after warm-up"}
    if args.front_outputs:
        out["front_outputs"] = True
    # one non-default stream for torch's copies, the library's kernels and the timing events (the null stream's handle would
    # leave the library on a stream of its own)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        with u.Context(N_PTS, args.scans, params=p, hooks=True) as ctx:
            ctx.set_stream(st.cuda_stream)
            if args.front_outputs:
                ctx.set_front_outputs(1)
            out["cfg3"] = run_workload(torch, u, ctx, gen(args.scans, 1, 1, False), p, args, "cfg3", False)
        with u.Context(N_PTS, args.scans, params=p, hooks=True) as ctx:
            ctx.set_stream(st.cuda_stream)
            if args.front_outputs:
                ctx.set_front_outputs(1)
            out["sensor_ragged"] = run_workload(torch, u, ctx, gen(args.scans, 3, 1, True), p, args, "sensor_ragged", True)
    out["wall_s"] = time.time() - t0
    print(json.dumps(out))


if __name__ == "__main__":
    main()
