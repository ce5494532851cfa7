#!/usr/bin/env python3
"""Times the fMLLR path on one device: the accumulation (khg_acc_fmllr_stats_post, split into its kernels) beside
khg_acc_stats_post on the same posteriors in the same process, the Gram kernel's arithmetic rate as a share of the fp64-MFMA peak, the
estimate on the device (khg_fmllr_stats_estimate) beside its host form (khg_fmllr_compute), and the feature transform in GB/s.  Repetitions alternate the two accumulations; medians
of the per-kernel HIP-event times.  Prints one JSON line.

Usage: python tools/fmllr_bench.py [--utts 2000] [--speakers 50] [--pdfs 5000] [--gauss 64] [--dim 40] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kaldi_hmm_gmm_amd as khg  # noqa: E402
from kaldi_hmm_gmm_amd import synth  # noqa: E402

FP64_MFMA_PEAK = 256 * 4 * 32 * 2.4e9          # CUs x SIMDs x (16 x 16 x 4 x 2 flop / 64 cycles) x 2.4 GHz = 78.6 TFLOP/s


def kernel_sums(ctx):
    out = {}
    for n, ms in ctx.timings():
        out[n] = out.get(n, 0.0) + ms
    return out


def med(rows, key):
    return float(np.median([r.get(key, 0.0) for r in rows]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=2000)
    ap.add_argument("--speakers", type=int, default=50)
    ap.add_argument("--pdfs", type=int, default=5000)
    ap.add_argument("--gauss", type=int, default=64)
    ap.add_argument("--dim", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--num-iters", type=int, default=40)
    args = ap.parse_args()
    m = synth.make_model(args.pdfs, args.gauss, args.dim, seed=20230418)
    gc, _ = khg._kaldi_hmm_gmm_amd.compute_gconsts(m.gauss_off, m.weights, m.inv_vars, m.means_invvars)
    ut = synth.make_utts(m, args.utts, seed=2)
    U, N, D = args.utts, int(ut.frame_off[-1]), args.dim
    u2s = (np.arange(U) % args.speakers).astype(np.int32)
    ctx = khg.Context(0)
    dm = khg.DeviceModel(ctx, m.gauss_off, gc, m.means_invvars, m.inv_vars)
    tm = khg.DeviceTransitions(ctx, m.id2pdf)
    us = khg.UtteranceSet(ctx, None, np.asarray(ut.frame_off, np.int64), np.ascontiguousarray(ut.feats, np.float32))
    # ali-to-post of the generating alignment: one entry of weight 1 per frame
    post = khg.DevicePosteriors.from_arrays(ctx, np.asarray(ut.frame_off, np.int64), np.arange(N + 1, dtype=np.int64),
                                            np.asarray(ut.ref_ali, np.int32), np.ones(N, np.float64))
    accs = khg.DeviceAccs(ctx, dm, tm)
    stats = khg.DeviceFmllrStats(ctx, args.speakers, D)
    fm_rows, k3_rows, fm_wall, k3_wall = [], [], [], []
    for rep in range(args.reps + 1):            # the first repetition warms up (allocations)
        for which in ("k3", "fmllr"):
            ctx.sync()
            ctx.set_timing(True)
            t0 = time.perf_counter()
            if which == "k3":
                us.acc_stats_post(dm, tm, post, accs)
            else:
                us.acc_fmllr_stats_post(dm, tm, post, u2s, stats)
            ctx.sync()
            wall = 1e3 * (time.perf_counter() - t0)
            k = kernel_sums(ctx)
            ctx.set_timing(False)
            if rep > 0:
                (k3_rows if which == "k3" else fm_rows).append(k)
                (k3_wall if which == "k3" else fm_wall).append(wall)
    s = stats.download()
    t0 = time.perf_counter()
    est = khg.fmllr_compute(s["beta"], s["K"], s["G"], min_count=1.0, num_iters=args.num_iters)
    host_s = time.perf_counter() - t0
    dev_ms, dev_wall, same = [], [], None
    for rep in range(args.reps + 1):            # the estimate on the device, on the statistics where they are
        ctx.sync()
        ctx.set_timing(True)
        t0 = time.perf_counter()
        dev = stats.estimate(min_count=1.0, num_iters=args.num_iters)
        wall = 1e3 * (time.perf_counter() - t0)
        k = kernel_sums(ctx)
        ctx.set_timing(False)
        if rep > 0:
            dev_ms.append({n: round(v, 3) for n, v in k.items()})
            dev_wall.append(round(wall, 3))
        same = bool(dev["W"].tobytes() == est["W"].tobytes() and (dev["status"] == est["status"]).all())
    tr_ms = []
    for rep in range(args.reps + 1):
        ctx.sync()
        ctx.set_timing(True)
        khg.transform_feats_batch(us, u2s, est["W"])
        ctx.sync()
        k = kernel_sums(ctx)
        ctx.set_timing(False)
        if rep > 0:
            tr_ms.append(k["k_fmllr_transform"])
    D1 = D + 1
    npairs = D1 * (D1 + 1) // 2
    dpad = 16 * ((D + 15) // 16)
    cols_pad = 16 * ((npairs + 15) // 16) + 16 * ((D1 + 15) // 16)
    flops_pad = 2.0 * N * dpad * cols_pad
    flops_useful = 2.0 * N * D * (npairs + D1)
    gram_ms = med(fm_rows, "k_fmllr_gram")
    out = {
        "shape": [args.pdfs, args.gauss, D], "utts": U, "speakers": args.speakers, "frames": N, "entries": N, "repetitions": args.reps,
        "acc_fmllr_stats_post_kernels_ms": {k: round(med(fm_rows, k), 4) for k in sorted({k for r in fm_rows for k in r})},
        "acc_fmllr_stats_post_wall_ms": [round(x, 3) for x in fm_wall],
        "acc_stats_post_kernels_ms": {k: round(med(k3_rows, k), 4) for k in sorted({k for r in k3_rows for k in r})},
        "acc_stats_post_total_ms": [round(sum(r.values()), 4) for r in k3_rows],
        "acc_stats_post_wall_ms": [round(x, 3) for x in k3_wall],
        "gram_padded_tflops": round(flops_pad / (1e9 * gram_ms), 2) if gram_ms else None,
        "gram_share_of_fp64_mfma_peak": round(flops_pad / (1e-3 * gram_ms) / FP64_MFMA_PEAK, 4) if gram_ms else None,
        "gram_padding_share": round(1.0 - flops_useful / flops_pad, 4),
        "chunks": stats.num_chunks(),
        "fmllr_compute_host_s": round(host_s, 3), "fmllr_compute_status_ok": int((est["status"] == 0).sum()), "num_iters": args.num_iters,
        "estimate_device_kernels_ms": dev_ms, "estimate_device_wall_ms": dev_wall, "estimate_device_equals_host_bitwise": same,
        "transform_ms": [round(x, 4) for x in tr_ms],
        "transform_GBps_at_median": round(2.0 * N * D * 4 / (1e6 * float(np.median(tr_ms))), 1),
    }
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
