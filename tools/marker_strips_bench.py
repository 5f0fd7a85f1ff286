#!/usr/bin/env python3
"""tools/marker_strips_bench.py -- road_marker's line strips for a resident batch (urf_marker_strips_batch), measured on one MI355X.
Prints ONE JSON line.

    python tools/marker_strips_bench.py [--scans 1024] [--repeats 7] [--warmup 3] [--baseline-root DIR] [--front-outputs]

S synthetic 64 x 2048 street sweeps (scenes 1 and 2 alternating), resident; urf_classify_batch_soa + urf_marker_points_batch
run first (not timed), then:
  (a) strips_device_ms      urf_marker_strips_batch alone: device events around --calls back-to-back calls (one call is tens of
                            microseconds: an event pair around it would measure launch and event granularity), per call, median
                            of --repeats after --warmup
      worst_case_device_ms  the same for S scans of 361 marker points each in runs of two (180 strips), a jagged outline,
                            simplification and the average height on: the longest zavg chain and the most spans
  (b) strips_and_copy_ms    the call + one copy of counts, records and strip points to pinned host memory + synchronise:
                            host clock (the figure ends at a host synchronisation), median
  (c) baseline_*            what a checkout without the device call offers for the same result: d_pts / d_counts copied to the
                            host (baseline_copy_ms, host clock, median) + urf::MarkerBuilder::build per sweep on one thread
                            (baseline_build_ms: tools/marker_builder_baseline.cpp compiled against --baseline-root, the root of a
                            checkout of the parent commit with its library built; default: this checkout, whose MarkerBuilder
                            runs the new host code -- say which one a recorded figure used)
--front-outputs: urf_set_front_outputs(ctx, 1) -- urf_marker_points_batch takes the fused batch as it is (marker_points_ms: the call by
itself, device events, median, only with the flag; every repeat after the first finds the pre-pass done).  Without the flag the tool does
what it did before the flag existed.
A parity gate runs first: every scan's records against urf_marker_strips on the copied marker points.
"""
import argparse
import json
import os
import statistics
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

RINGS, COLS = 64, 2048
N_PTS = RINGS * COLS


def baseline(root, pts, cnt, repeats):
    pkg = os.path.join(root, "urban_road_filter_amd")
    with tempfile.TemporaryDirectory() as tmp:
        exe, data = os.path.join(tmp, "baseline"), os.path.join(tmp, "points.bin")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(root, "include"), "-I" + os.path.join(pkg, "csrc"),
                               os.path.join(ROOT, "tools", "marker_builder_baseline.cpp"), "-o", exe, "-L" + pkg, "-l:liburf_hip.so",
                               "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"])
        with open(data, "wb") as f:
            f.write(struct.pack("<I", len(cnt)) + cnt.astype(np.uint32).tobytes() + pts.astype(np.float32).tobytes())
        return json.loads(subprocess.run([exe, data, str(repeats)], capture_output=True, text=True, check=True, timeout=600).stdout)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--baseline-root", default=ROOT)
    ap.add_argument("--front-outputs", action="store_true")
    args = ap.parse_args()
    import torch
    import urban_road_filter_amd as u
    import oracles as O
    from batch_clouds_bench import gen
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured here")
    S, dev = args.scans, torch.device("cuda:0")
    p, mp = O.cfg_params("cfg2"), u.default_marker_params()
    scans = gen((S + 1) // 2, 1, 1, False) + gen(S // 2, 2, 1, False)
    scans = [scans[(s // 2) + (0 if s % 2 == 0 else (S + 1) // 2)] for s in range(S)]   # street / narrow street alternating: strip counts vary
    out = {"metric": "marker_strips", "device": torch.cuda.get_device_name(0), "scans": S, "repeats": args.repeats, "warmup": args.warmup,
           "baseline_root_is_this_checkout": os.path.samefile(args.baseline_root, ROOT)}
    st = torch.cuda.Stream()
    with torch.cuda.stream(st), u.Context(N_PTS, S, params=p) as ctx:
        ctx.set_stream(st.cuda_stream)
        if args.front_outputs:
            ctx.set_front_outputs(1)
        d_xyz_in = [torch.from_numpy(np.concatenate([s[k] for s in scans])).to(dev) for k in range(3)]
        labels = torch.empty(S * N_PTS, dtype=torch.uint8, device=dev)
        d_pts = torch.empty(S * u.MARKER_MAX_POINTS * 4, dtype=torch.float32, device=dev)
        d_cnt = torch.empty(S, dtype=torch.int32, device=dev)
        # counts, records, strip points in one block: one copy brings them back
        n_words = 3 * S + S * u.MARKER_MAX_STRIPS * 8 + S * u.MARKER_MAX_STRIP_POINTS * 3
        block = torch.empty(n_words, dtype=torch.int32, device=dev)
        h_block = torch.empty(n_words, dtype=torch.int32).pin_memory()
        h_pts, h_cnt = torch.empty_like(d_pts, device="cpu").pin_memory(), torch.empty_like(d_cnt, device="cpu").pin_memory()
        d_n, d_strips, d_xyz = block[:3 * S], block[3 * S:3 * S + S * u.MARKER_MAX_STRIPS * 8], block[3 * S + S * u.MARKER_MAX_STRIPS * 8:]
        d_ghost = torch.zeros(1, dtype=torch.int32, device=dev)
        ctx.classify_batch_soa(d_xyz_in[0], d_xyz_in[1], d_xyz_in[2], N_PTS, S, labels)
        ctx.marker_points_batch(d_pts, d_cnt)
        torch.cuda.synchronize()
        if args.front_outputs:   # the read-out the flag changes, by itself
            mk_ms = []
            for _ in range(args.warmup + args.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ctx.marker_points_batch(d_pts, d_cnt)
                e1.record()
                torch.cuda.synchronize()
                mk_ms.append(e0.elapsed_time(e1))
            out.update({"front_outputs": True, "marker_points_ms": statistics.median(mk_ms[args.warmup:]),
                        "front_scans_after_marker_points": ctx.front_scans()})

        def call():
            d_ghost.zero_()
            ctx.marker_strips_batch(mp, d_pts, d_cnt, S, 1, d_ghost, d_strips, d_xyz, d_n)

        # parity gate
        call()
        torch.cuda.synchronize()
        pts, cnt = d_pts.cpu().numpy().reshape(S, -1, 4), d_cnt.cpu().numpy()
        n = d_n.cpu().numpy().reshape(S, 3)
        strips = d_strips.cpu().numpy().view(u.MARKER_STRIP_DTYPE).reshape(S, u.MARKER_MAX_STRIPS)
        xyz = d_xyz.cpu().numpy().view(np.float32).reshape(S, u.MARKER_MAX_STRIP_POINTS, 3)
        ghost = 0
        for s in range(S):
            pub, hs, hx, ghost = u.marker_strips(pts[s, :cnt[s]], mp, ghost)
            assert (int(pub), len(hs), len(hx)) == tuple(int(v) for v in n[s]), s
            assert strips[s, :len(hs)].tobytes() == hs.tobytes() and xyz[s, :len(hx)].tobytes() == hx.tobytes(), s
        assert int(d_ghost.cpu()[0]) == ghost
        out.update({"published_scans": int(n[:, 0].sum()), "markers": int(n[:, 1].sum()), "strip_points": int(n[:, 2].sum()),
                    "delete_markers": int(sum((strips[s, :n[s, 1]]["action"] == 2).sum() for s in range(S))), "parity": "every scan"})
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        def device_ms(pts_t, cnt_t):
            for _ in range(args.warmup):
                ctx.marker_strips_batch(mp, pts_t, cnt_t, S, 1, d_ghost, d_strips, d_xyz, d_n)
            torch.cuda.synchronize()
            runs = []
            for _ in range(args.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.calls):
                    ctx.marker_strips_batch(mp, pts_t, cnt_t, S, 1, d_ghost, d_strips, d_xyz, d_n)
                e1.record()
                torch.cuda.synchronize()
                runs.append(e0.elapsed_time(e1) / args.calls)
            return runs

        a_ms = device_ms(d_pts, d_cnt)
        import marker_sets as M
        rng = np.random.default_rng(1)
        worst = np.stack([np.concatenate([M.outline(rng, u.MARKER_MAX_POINTS, "jagged"), M.colours(rng, u.MARKER_MAX_POINTS, "pairs")[:, None]], 1)
                          for _ in range(S)]).astype(np.float32)
        w_ms = device_ms(torch.from_numpy(worst.reshape(-1)).to(dev), torch.full((S,), u.MARKER_MAX_POINTS, dtype=torch.int32, device=dev))
        torch.cuda.synchronize()
        assert int(d_n.cpu().numpy().reshape(S, 3)[:, 1].min()) == u.MARKER_MAX_STRIPS
        out.update({"calls_per_event_pair": args.calls, "worst_case_device_ms": statistics.median(w_ms), "worst_case_device_ms_runs": w_ms})
        b_ms, c_copy_ms = [], []
        for _ in range(args.warmup + args.repeats):
            d_ghost.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.marker_strips_batch(mp, d_pts, d_cnt, S, 1, d_ghost, d_strips, d_xyz, d_n)
            h_block.copy_(block, non_blocking=True)
            torch.cuda.synchronize()
            b_ms.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            h_pts.copy_(d_pts, non_blocking=True)
            h_cnt.copy_(d_cnt, non_blocking=True)
            torch.cuda.synchronize()
            c_copy_ms.append((time.perf_counter() - t0) * 1e3)
        b_ms, c_copy_ms = b_ms[args.warmup:], c_copy_ms[args.warmup:]
    base = baseline(args.baseline_root, pts, cnt, args.repeats)
    assert base["markers"] == out["markers"] and base["points"] == out["strip_points"], base
    out.update({"strips_device_ms": statistics.median(a_ms), "strips_device_ms_runs": a_ms,
                "strips_and_copy_ms": statistics.median(b_ms), "strips_and_copy_ms_runs": b_ms,
                "copied_bytes": int(n_words * 4),
                "baseline_copy_ms": statistics.median(c_copy_ms), "baseline_build_ms": statistics.median(base["ms"]),
                "baseline_build_ms_runs": base["ms"],
                "baseline_total_ms": statistics.median(c_copy_ms) + statistics.median(base["ms"])})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
