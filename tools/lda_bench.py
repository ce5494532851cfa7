#!/usr/bin/env python3
"""Times the LDA path on one device: the accumulation (khg_acc_lda_stats_post, split into its kernels), the
second-order kernel's arithmetic rate as a share of the fp64-MFMA peak with its padding share, the fused splice-and-project, and the
host estimate (khg_lda_compute).  The workload is tools/mllt_bench.py's: 5000 classes, 2000 utterances, one entry of weight 1 per
frame from the generating alignment; features of dimension 13 spliced with +-4 frames.  Medians of the per-kernel HIP-event times.
Prints one JSON line.

Usage: python tools/lda_bench.py [--utts 2000] [--pdfs 5000] [--dim 13] [--left 4] [--right 4] [--target-dim 40] [--reps 5]
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
CT = 8                                         # LD_CT of csrc/khg_lda_stats.hip.inc: column tiles of one wave


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
    ap.add_argument("--pdfs", type=int, default=5000)
    ap.add_argument("--dim", type=int, default=13)
    ap.add_argument("--left", type=int, default=4)
    ap.add_argument("--right", type=int, default=4)
    ap.add_argument("--target-dim", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    m = synth.make_model(args.pdfs, 1, args.dim, seed=20230418)
    ut = synth.make_utts(m, args.utts, seed=2)
    U, N, D, L, R = args.utts, int(ut.frame_off[-1]), args.dim, args.left, args.right
    Dz = D * (L + R + 1)
    ctx = khg.Context(0)
    tm = khg.DeviceTransitions(ctx, m.id2pdf)
    C = int(np.asarray(m.id2pdf)[1:].max()) + 1
    us = khg.UtteranceSet(ctx, None, np.asarray(ut.frame_off, np.int64), np.ascontiguousarray(ut.feats, np.float32))
    post = khg.DevicePosteriors.from_arrays(ctx, np.asarray(ut.frame_off, np.int64), np.arange(N + 1, dtype=np.int64),
                                            np.asarray(ut.ref_ali, np.int32), np.ones(N, np.float64))
    stats = khg.DeviceLdaStats(ctx, C, D, L, R)
    rows, wall = [], []
    for rep in range(args.reps + 1):            # the first repetition warms up (allocations)
        stats.zero()
        ctx.sync()
        ctx.set_timing(True)
        t0 = time.perf_counter()
        us.acc_lda_stats_post(tm, post, stats)
        ctx.sync()
        w = 1e3 * (time.perf_counter() - t0)
        k = kernel_sums(ctx)
        ctx.set_timing(False)
        if rep > 0:
            rows.append(k)
            wall.append(w)
    t0 = time.perf_counter()
    est = khg.est_lda(stats, target_dim=min(args.target_dim, Dz))
    est_s = time.perf_counter() - t0
    trows = []
    import torch
    out_t = torch.empty((N, est["M"].shape[0]), dtype=torch.float32, device="cuda:%d" % ctx.device)
    for rep in range(args.reps + 1):
        ctx.sync()
        ctx.set_timing(True)
        khg.splice_transform_feats_batch(us, est["M"], L, R, out=out_t)
        k = kernel_sums(ctx)
        ctx.set_timing(False)
        if rep > 0:
            trows.append(k)
    ntz = (Dz + 15) // 16
    tiles = ntz * (ntz + 1) // 2
    units = sorted((min(CT, ti + 1 - tj0) for ti in range(ntz) for tj0 in range(0, ti + 1, CT)), reverse=True)
    issue = sum(max(units[i:i + 4]) * 4 for i in range(0, len(units), 4))       # tile slots the workgroups' SIMDs are held for
    frames_pad = sum(4 * ((min(1024, N - s) + 3) // 4) for s in range(0, N, 1024))
    flops_tiles = 2.0 * frames_pad * 256 * tiles
    flops_useful = 2.0 * N * (Dz * (Dz + 1) // 2)
    gram_ms = med(rows, "k_lda_gram")
    tot = [sum(r.values()) for r in rows]
    out = {
        "command": "tools/lda_bench.py " + " ".join(sys.argv[1:]),
        "classes": C, "dim": D, "left": L, "right": R, "spliced_dim": Dz, "utts": U, "frames": N, "entries": N, "repetitions": args.reps,
        "acc_lda_stats_post_kernels_ms": {k: round(med(rows, k), 4) for k in sorted({k for r in rows for k in r})},
        "acc_lda_stats_post_total_ms": [round(x, 4) for x in tot], "acc_lda_stats_post_wall_ms": [round(x, 3) for x in wall],
        "gram_ms": round(gram_ms, 4),
        "gram_tiles": tiles, "gram_units": units, "gram_issue_slots_over_tiles": round(issue / tiles, 4),
        "gram_tile_tflops": round(flops_tiles / (1e9 * gram_ms), 2) if gram_ms else None,
        "gram_share_of_fp64_mfma_peak": round(flops_tiles / (1e-3 * gram_ms) / FP64_MFMA_PEAK, 4) if gram_ms else None,
        "gram_padding_share": round(1.0 - flops_useful / flops_tiles, 4),
        "chunks": stats.num_chunks(),
        "splice_transform_ms": round(med(trows, "k_lda_splice_transform"), 4), "target_dim": int(est["M"].shape[0]),
        "lda_compute_host_s": round(est_s, 3), "lda_compute_status": int(est["status"]),
        "kept_eigenvalues": [round(float(x), 4) for x in est["eig"][:est["M"].shape[0]][:8]],
    }
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
