#!/usr/bin/env python3
"""Times the feature stage on one device, on a 13-dimensional set of the benchmark's utterance count and
lengths: compute-cmvn-stats (khg_acc_cmvn_stats, split into its kernels), apply-cmvn in place, and the fused apply-cmvn | add-deltas
(order 2, window 2), each by the HIP events around its kernels.  In the same process a device-to-device copy that moves as many
bytes as the call reads plus writes is timed; every call is reported as a fraction of that copy's bandwidth, and the fused call
against the two-call sequence (apply-cmvn in place, then add-deltas).  Medians over the repetitions.  Prints one JSON line.

Usage: python tools/feat_bench.py [--utts 100000] [--dim 13] [--speakers 1000] [--order 2] [--window 2] [--reps 7]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kaldi_hmm_gmm_amd as khg  # noqa: E402
from kaldi_hmm_gmm_amd import synth  # noqa: E402


def kernel_sums(ctx):
    out = {}
    for n, ms in ctx.timings():
        out[n] = out.get(n, 0.0) + ms
    return out


def timed(ctx, fn, reps):
    """per-kernel HIP-event times of `fn`, one dict per repetition after a warm-up"""
    rows = []
    for rep in range(reps + 1):
        ctx.sync()
        ctx.set_timing(True)
        fn()
        ctx.sync()
        k = kernel_sums(ctx)
        ctx.set_timing(False)
        if rep > 0:
            rows.append(k)
    return rows


def copy_ms(torch, nbytes_moved, device, reps):
    """a device-to-device copy that reads nbytes_moved / 2 and writes as many, by HIP events: the median of the repetitions"""
    n = max(1, nbytes_moved // 8)
    src = torch.empty(n, dtype=torch.float32, device=device).normal_()
    dst = torch.empty_like(src)
    ms = []
    for rep in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        if rep > 0:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=100000)
    ap.add_argument("--dim", type=int, default=13)
    ap.add_argument("--speakers", type=int, default=1000)
    ap.add_argument("--order", type=int, default=2)
    ap.add_argument("--window", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/feat_bench.py needs a GPU: nothing is measured without one")
    m = synth.make_model(30, 1, args.dim, seed=20230418)
    ut = synth.make_utts(m, args.utts, seed=20230418 + 1000, feats=False)          # the benchmark's lengths
    fo = np.asarray(ut.frame_off, np.int64)
    U, N, D, S = args.utts, int(fo[-1]), args.dim, args.speakers
    OD = D * (args.order + 1)
    ctx = khg.Context(0)
    device = "cuda:%d" % ctx.device
    rows_t = torch.empty((N, D), dtype=torch.float32, device=device).normal_(0.5, 2.0)
    torch.cuda.synchronize()
    us = khg.UtteranceSet(ctx, None, fo, (rows_t.data_ptr(), rows_t), dim=D)
    u2s = (np.arange(U) % S).astype(np.int32)
    stats = khg.DeviceCmvnStats(ctx, S, D)
    acc = timed(ctx, lambda: (stats.zero(), us.acc_cmvn_stats(u2s, stats)), args.reps)
    r = khg.cmvn_compute(stats, norm_vars=False)                                  # offsets only: the in-place repetitions stay in range
    norm, status = r["norm"], r["status"]
    out_t = torch.empty((N, OD), dtype=torch.float32, device=device)
    torch.cuda.synchronize()
    fused = timed(ctx, lambda: us.add_deltas(args.order, args.window, out_t.data_ptr(), norm, u2s, status), args.reps)
    plain = timed(ctx, lambda: us.add_deltas(args.order, args.window, out_t.data_ptr()), args.reps)
    apply = timed(ctx, lambda: us.apply_cmvn(u2s, norm, status, None), args.reps)

    def med(rows, key=None):
        return float(np.median([sum(x.values()) if key is None else x.get(key, 0.0) for x in rows]))
    fb = 4 * N * D
    moved = {"acc_cmvn_stats": fb, "apply_cmvn_in_place": 2 * fb, "add_deltas_fused": fb + 4 * N * OD}
    ms = {"acc_cmvn_stats": med(acc), "apply_cmvn_in_place": med(apply), "add_deltas_fused": med(fused)}
    cp = {k: copy_ms(torch, b, device, args.reps) for k, b in moved.items()}
    out = {
        "command": "tools/feat_bench.py " + " ".join(sys.argv[1:]),
        "utts": U, "frames": N, "dim": D, "speakers": S, "order": args.order, "window": args.window, "repetitions": args.reps,
        "acc_cmvn_stats_kernels_ms": {k: round(med(acc, k), 4) for k in sorted({k for x in acc for k in x})}, "chunks": stats.num_chunks(),
        "ms": {k: round(v, 4) for k, v in ms.items()},
        "bytes_read_plus_written": moved,
        "gb_per_s": {k: round(moved[k] / (1e6 * ms[k]), 1) for k in ms},
        "copy_ms_same_bytes": {k: round(v, 4) for k, v in cp.items()},
        "copy_gb_per_s": {k: round(moved[k] / (1e6 * cp[k]), 1) for k in cp},
        "fraction_of_copy_bandwidth": {k: round(cp[k] / ms[k], 4) for k in ms},
        "add_deltas_without_norm_ms": round(med(plain), 4),
        "two_call_sequence_ms": round(med(apply) + med(plain), 4),
        "fused_over_two_calls": round(med(fused) / (med(apply) + med(plain)), 4),
    }
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
