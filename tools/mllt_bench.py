#!/usr/bin/env python3
"""Times the MLLT path on one device: the accumulation (khg_acc_mllt_stats_post, split into its kernels) beside
its two yardsticks on the same posteriors in the same process -- khg_acc_fmllr_stats_post for a single speaker and
khg_acc_stats_post: the new call is their sum plus the Gaussian-side GEMM and the fold --, the Gaussian-side kernel's arithmetic rate
as a share of the fp64-MFMA peak with its padding share, and the host estimate (khg_mllt_compute) at D = 40 and 80.  Repetitions
alternate the three calls; medians of the per-kernel HIP-event times.  Prints one JSON line.

--skew F gives the share F of the frames to pdf 0 (silence in a real alignment): the accumulation's K3 pass runs one workgroup per
pdf whatever the pdf's bucket holds, where khg_acc_stats_post on its own cuts a large bucket into several -- the cost shows in
k3_accumulate of the new call against the yardstick's.

Usage: python tools/mllt_bench.py [--utts 2000] [--pdfs 5000] [--gauss 64] [--dim 40] [--reps 5] [--skew 0.0] [--num-iters 200]
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


def host_estimate_s(D, num_iters, seed=1):
    """khg_mllt_compute on well-conditioned synthetic statistics of dimension D"""
    rng = np.random.default_rng(seed)
    il, jl = np.tril_indices(D)
    G = []
    for _ in range(D):
        a = rng.standard_normal((4 * D, D))
        G.append((a.T @ a)[il, jl])
    t0 = time.perf_counter()
    r = khg.mllt_compute(4.0 * D, np.stack(G), num_iters=num_iters)
    return time.perf_counter() - t0, int(r["status"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=2000)
    ap.add_argument("--pdfs", type=int, default=5000)
    ap.add_argument("--gauss", type=int, default=64)
    ap.add_argument("--dim", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--num-iters", type=int, default=200)
    ap.add_argument("--skew", type=float, default=0.0)
    args = ap.parse_args()
    m = synth.make_model(args.pdfs, args.gauss, args.dim, seed=20230418)
    gc, _ = khg._kaldi_hmm_gmm_amd.compute_gconsts(m.gauss_off, m.weights, m.inv_vars, m.means_invvars)
    ut = synth.make_utts(m, args.utts, seed=2)
    U, N, D = args.utts, int(ut.frame_off[-1]), args.dim
    sumG = int(m.gauss_off[-1])
    ctx = khg.Context(0)
    dm = khg.DeviceModel(ctx, m.gauss_off, gc, m.means_invvars, m.inv_vars)
    tm = khg.DeviceTransitions(ctx, m.id2pdf)
    us = khg.UtteranceSet(ctx, None, np.asarray(ut.frame_off, np.int64), np.ascontiguousarray(ut.feats, np.float32))
    ali = np.asarray(ut.ref_ali, np.int32).copy()
    if args.skew > 0:
        tid0 = int(np.nonzero(np.asarray(m.id2pdf)[1:] == 0)[0][0]) + 1
        ali[np.random.default_rng(5).random(N) < args.skew] = tid0
    # ali-to-post of the generating alignment: one entry of weight 1 per frame
    post = khg.DevicePosteriors.from_arrays(ctx, np.asarray(ut.frame_off, np.int64), np.arange(N + 1, dtype=np.int64),
                                            ali, np.ones(N, np.float64))
    accs = khg.DeviceAccs(ctx, dm, tm)
    fstats = khg.DeviceFmllrStats(ctx, 1, D)
    mstats = khg.DeviceMlltStats(ctx, D)
    one = np.zeros(U, np.int32)
    rows = {"k3": [], "fmllr": [], "mllt": []}
    wall = {"k3": [], "fmllr": [], "mllt": []}
    for rep in range(args.reps + 1):            # the first repetition warms up (allocations)
        for which in ("k3", "fmllr", "mllt"):
            ctx.sync()
            ctx.set_timing(True)
            t0 = time.perf_counter()
            if which == "k3":
                us.acc_stats_post(dm, tm, post, accs)
            elif which == "fmllr":
                us.acc_fmllr_stats_post(dm, tm, post, one, fstats)
            else:
                us.acc_mllt_stats_post(dm, tm, post, mstats)
            ctx.sync()
            w = 1e3 * (time.perf_counter() - t0)
            k = kernel_sums(ctx)
            ctx.set_timing(False)
            if rep > 0:
                rows[which].append(k)
                wall[which].append(w)
    tot = {w: [sum(r.values()) for r in rows[w]] for w in rows}
    t_m, t_f, t_k = (float(np.median(tot[w])) for w in ("mllt", "fmllr", "k3"))
    npairs = D * (D + 1) // 2
    dpad = 16 * ((D + 15) // 16)
    cols_pad = 16 * ((npairs + 15) // 16)
    gpad = 4 * ((sumG + 3) // 4)
    flops_pad = 2.0 * gpad * dpad * cols_pad
    flops_useful = 2.0 * sumG * D * npairs
    gauss_ms = med(rows["mllt"], "k_mllt_gauss")
    h40, s40 = host_estimate_s(40, args.num_iters)
    h80, s80 = host_estimate_s(80, args.num_iters)
    out = {
        "command": "tools/mllt_bench.py " + " ".join(sys.argv[1:]),
        "shape": [args.pdfs, args.gauss, D], "skew": args.skew, "utts": U, "frames": N, "entries": N, "repetitions": args.reps,
        "acc_mllt_stats_post_kernels_ms": {k: round(med(rows["mllt"], k), 4) for k in sorted({k for r in rows["mllt"] for k in r})},
        "acc_mllt_stats_post_total_ms": [round(x, 4) for x in tot["mllt"]], "acc_mllt_stats_post_wall_ms": [round(x, 3) for x in wall["mllt"]],
        "acc_fmllr_stats_post_one_speaker_total_ms": [round(x, 4) for x in tot["fmllr"]],
        "acc_fmllr_stats_post_one_speaker_wall_ms": [round(x, 3) for x in wall["fmllr"]],
        "acc_stats_post_kernels_ms": {k: round(med(rows["k3"], k), 4) for k in sorted({k for r in rows["k3"] for k in r})},
        "acc_stats_post_total_ms": [round(x, 4) for x in tot["k3"]], "acc_stats_post_wall_ms": [round(x, 3) for x in wall["k3"]],
        "mllt_over_sum_of_yardsticks": round(t_m / (t_f + t_k), 4) if t_f + t_k else None,
        "gauss_side_ms": round(gauss_ms, 4),
        "gauss_side_padded_tflops": round(flops_pad / (1e9 * gauss_ms), 2) if gauss_ms else None,
        "gauss_side_share_of_fp64_mfma_peak": round(flops_pad / (1e-3 * gauss_ms) / FP64_MFMA_PEAK, 4) if gauss_ms else None,
        "gauss_side_padding_share": round(1.0 - flops_useful / flops_pad, 4),
        "chunks": mstats.num_chunks(), "num_iters": args.num_iters,
        "mllt_compute_host_s": {"40": round(h40, 3), "80": round(h80, 3)}, "mllt_compute_status": [s40, s80],
    }
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
