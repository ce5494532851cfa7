#!/usr/bin/env python3
"""Times khg_acc_stats_post of the package under --root (this tree by default, or a tree holding another build, e.g. the parent
commit's) on the posteriors of tools/fmllr_bench.py: 5000 x 64 x 40, --utts utterances, one entry of weight 1 per frame.  Prints one
JSON line with the per-repetition sums of the call's HIP-event kernel times.  Run it alternately for two roots (one process each) to
compare two builds.

Usage: python tools/acc_stats_post_ab.py [--root DIR] [--utts 2000] [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--utts", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import kaldi_hmm_gmm_amd as khg
    from kaldi_hmm_gmm_amd import synth
    m = synth.make_model(5000, 64, 40, seed=20230418)
    gc, _ = khg._kaldi_hmm_gmm_amd.compute_gconsts(m.gauss_off, m.weights, m.inv_vars, m.means_invvars)
    ut = synth.make_utts(m, args.utts, seed=2)
    N = int(ut.frame_off[-1])
    ctx = khg.Context(0)
    dm = khg.DeviceModel(ctx, m.gauss_off, gc, m.means_invvars, m.inv_vars)
    tm = khg.DeviceTransitions(ctx, m.id2pdf)
    us = khg.UtteranceSet(ctx, None, np.asarray(ut.frame_off, np.int64), np.ascontiguousarray(ut.feats, np.float32))
    post = khg.DevicePosteriors.from_arrays(ctx, np.asarray(ut.frame_off, np.int64), np.arange(N + 1, dtype=np.int64),
                                            np.asarray(ut.ref_ali, np.int32), np.ones(N, np.float64))
    accs = khg.DeviceAccs(ctx, dm, tm)
    totals, rows = [], []
    for rep in range(args.reps + 1):
        ctx.sync()
        ctx.set_timing(True)
        us.acc_stats_post(dm, tm, post, accs)
        ctx.sync()
        k = {}
        for n, ms in ctx.timings():
            k[n] = k.get(n, 0.0) + ms
        ctx.set_timing(False)
        if rep > 0:
            rows.append(k)
            totals.append(round(sum(k.values()), 4))
    print(json.dumps({"root": os.path.abspath(khg.__file__), "frames": N, "acc_stats_post_total_ms": totals,
                      "median_ms": float(np.median(totals)), "kernels_ms_median": {n: round(float(np.median([r[n] for r in rows])), 4) for n in rows[0]}}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
