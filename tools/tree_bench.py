#!/usr/bin/env python3
"""Times the tree-building path on one device: khg_acc_tree_stats split into its kernels, against the bytes
the gather has to move, and khg_build_tree on the statistics it produced.  The workload is tools/lda_bench.py's: 5000 pdfs = 1666
three-state phones, 2000 utterances of 10 .. 40 uniformly drawn phones, the generating alignment uploaded as the resident one;
transition-id 2 pdf + 2 is the forward arc out of HMM state pdf % 3 of phone pdf // 3 + 1, 2 pdf + 1 its self-loop.  Medians of the
per-kernel HIP-event times.  Prints one JSON line.

Usage: python tools/tree_bench.py [--utts 2000] [--pdfs 5000] [--dim 40] [--reps 5] [--max-leaves 2000]
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

HBM_BYTES_PER_S = 6.29e12          # measured streaming rate of the chip (float4 copy)


def tid_tables(num_pdfs):
    t = np.arange(2 * num_pdfs + 1)
    pdf = np.where(t > 0, (t - 1) // 2, 0)
    phone = (pdf // 3 + 1).astype(np.int32)
    pdf_class = (pdf % 3).astype(np.int32)
    flags = (np.where(t % 2 == 1, 1, 0) | np.where((t % 2 == 0) & (pdf % 3 == 2), 2, 0)).astype(np.int32)
    phone[0] = pdf_class[0] = flags[0] = 0
    return phone, pdf_class, flags


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=2000)
    ap.add_argument("--pdfs", type=int, default=5000)
    ap.add_argument("--dim", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-leaves", type=int, default=2000)
    args = ap.parse_args()
    m = synth.make_model(args.pdfs, 1, args.dim, seed=20230418)
    ut = synth.make_utts(m, args.utts, seed=2)
    N, D = int(ut.frame_off[-1]), args.dim
    phone, pdf_class, flags = tid_tables(args.pdfs)
    ctx = khg.Context(0)
    us = khg.UtteranceSet(ctx, None, np.asarray(ut.frame_off, np.int64), np.ascontiguousarray(ut.feats, np.float32))
    us.upload_ali(np.asarray(ut.ref_ali, np.int32))
    stats = khg.DeviceTreeStats(ctx, D, 3, 1)
    none = np.zeros(0, np.int32)
    rows, wall = [], []
    for rep in range(args.reps + 1):            # the first repetition warms up (allocations)
        stats.zero()
        ctx.sync()
        ctx.set_timing(True)
        t0 = time.perf_counter()
        status = us._acc_tree_stats(phone, pdf_class, flags, none, stats)
        ctx.sync()
        w = 1e3 * (time.perf_counter() - t0)
        k = {}
        for n, ms in ctx.timings():
            k[n] = k.get(n, 0.0) + ms
        ctx.set_timing(False)
        if rep > 0:
            rows.append(k)
            wall.append(w)
    assert not np.asarray(status).any()
    st = dict(stats.download())
    st.update(N=3, P=1)
    counts = np.sort(st["count"])
    med = {k: round(float(np.median([r.get(k, 0.0) for r in rows])), 4) for k in sorted({k for r in rows for k in r})}
    gather_bytes = (8 + 4 * D) * N
    nphones = args.pdfs // 3
    sets = [[p] for p in range(1, nphones + 1)]
    p2n = [0] + [3] * nphones
    rng = np.random.default_rng(1)
    questions = [sorted(rng.choice(np.arange(1, nphones + 1), size=int(s), replace=False).tolist()) for s in rng.integers(2, nphones // 2, size=40)] + [[0]]
    t0 = time.perf_counter()
    tree, info = khg.build_tree(st, questions, sets, p2n, [True] * nphones, [True] * nphones, thresh=0.0, max_leaves=nphones + args.max_leaves, cluster_thresh=0.0,
                                return_info=True)
    build_s = time.perf_counter() - t0
    out = {
        "command": "tools/tree_bench.py " + " ".join(sys.argv[1:]),
        "pdfs": args.pdfs, "phones": nphones, "dim": D, "utts": args.utts, "frames": N, "repetitions": args.reps, "N": 3, "P": 1,
        "keys": int(len(counts)), "entries_per_key_median": float(np.median(counts)), "entries_per_key_max": float(counts[-1]),
        "acc_tree_stats_kernels_ms": med, "acc_tree_stats_kernel_total_ms": [round(sum(r.values()), 4) for r in rows],
        "acc_tree_stats_wall_ms": [round(x, 3) for x in wall],
        "gather_bytes": gather_bytes, "gather_floor_ms_at_hbm_rate": round(1e3 * gather_bytes / HBM_BYTES_PER_S, 4),
        "gather_share_of_hbm_rate": round(gather_bytes / (1e-3 * med["k_tree_sum"]) / HBM_BYTES_PER_S, 4) if med.get("k_tree_sum") else None,
        "build_tree_host_s": round(build_s, 3), "build_tree_questions_per_key": len(questions), "build_tree_leaves": info["num_leaves"],
        "build_tree_objf_impr_per_frame": round(info["objf_impr"] / N, 4),
    }
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
