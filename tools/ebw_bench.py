#!/usr/bin/env python3
"""Times the Extended Baum-Welch update on the device (khg_model_ebw_update, kernel k4_ebw_update) against the host form
(khg_ebw_am_diag_gmm_update) in the same process, and against the ML update (khg_model_mle_update, kernel k4_mle_update) at the
same shape, on fabricated blocks (data drawn near the model, as tests/test_gpu_mstep.py fabricates them).  Prints one JSON line.

The EBW kernel reads 4*D fp64 statistics and reads and writes 2*D floats per Gaussian (48*D bytes); the ML kernel 32*D.

Usage: python tools/ebw_bench.py [--pdfs 5000] [--gauss 64] [--dim 40] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kaldi_hmm_gmm_amd as khg  # noqa: E402
from kaldi_hmm_gmm_amd import mle as khg_mle, synth  # noqa: E402


def fabricate(m, rng, spread, lo, hi):
    G, D = int(m.gauss_off[-1]), m.dim
    occ = rng.uniform(lo, hi, G)
    mu = m.means.astype(np.float64) + spread * rng.standard_normal((G, D))
    var = m.vars.astype(np.float64) * rng.uniform(0.7, 1.4, (G, D))
    return occ, occ[:, None] * mu, occ[:, None] * (var + mu * mu)


def block(accs, blk):
    buf = np.zeros(accs.size, np.float64)
    G, D = accs.sumG, accs.dim
    buf[:G] = blk[0]
    buf[G: G + G * D] = blk[1].reshape(-1)
    buf[G + G * D: G + 2 * G * D] = blk[2].reshape(-1)
    return buf


def kernel_ms(ctx, name):
    return [ms for n, ms in ctx.timings() if n == name]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pdfs", type=int, default=5000)
    ap.add_argument("--gauss", type=int, default=64)
    ap.add_argument("--dim", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--den-spread", type=float, default=0.35, help="how far the denominator's means lie from the model's (0.3: the numerator's); "
                    "a wide denominator makes most Gaussians search for a larger D")
    args = ap.parse_args()
    m = synth.make_model(args.pdfs, args.gauss, args.dim, seed=20230418)
    rng = np.random.default_rng(1)
    num = fabricate(m, rng, 0.3, 20.0, 80.0)
    den = fabricate(m, rng, args.den_spread, 5.0, 20.0)
    go, w, miv, iv = m.gauss_off, m.weights, m.means_invvars, m.inv_vars
    gc, _ = khg._kaldi_hmm_gmm_amd.compute_gconsts(go, w, iv, miv)
    t0 = time.perf_counter()
    h_w, h_gc, h_miv, h_iv, h_res = khg_mle._flat_ebw_update(None, None, go, num, den, 0x7, w, miv, iv)
    host_s = time.perf_counter() - t0
    ctx = khg.Context(0)
    tm = khg.DeviceTransitions(ctx, m.id2pdf)
    ebw_ms, ebw_wall, mle_ms = [], [], []
    same = True
    for rep in range(args.reps + 1):        # the first repetition warms up
        dm = khg.DeviceModel(ctx, go, gc, miv, iv, weights=w)
        a_num, a_den = khg.DeviceAccs(ctx, dm, tm), khg.DeviceAccs(ctx, dm, tm)
        a_num.upload(block(a_num, num))
        a_den.upload(block(a_den, den))
        ctx.sync()
        ctx.set_timing(True)
        t0 = time.perf_counter()
        r = dm.ebw_update(a_num, a_den, None, None, 0x7)
        wall = time.perf_counter() - t0
        ctx.sync()
        k = kernel_ms(ctx, "k4_ebw_update")
        ctx.set_timing(False)
        if rep == 0:
            d = dm.download()
            same = bool(np.array_equal(d["weights"], h_w) and np.array_equal(d["inv_vars"], h_iv) and np.array_equal(d["means_invvars"], h_miv)
                        and all(r[x] == h_res[x] for x in ("floored", "failed", "skipped", "weights_skipped", "count")))
        else:
            ebw_ms.append(k[-1])
            ebw_wall.append(1e3 * wall)
        dm2 = khg.DeviceModel(ctx, go, gc, miv, iv, weights=w)
        ctx.sync()
        ctx.set_timing(True)
        dm2.mle_update(a_num, None, 0x7)
        ctx.sync()
        k = kernel_ms(ctx, "k4_mle_update")
        ctx.set_timing(False)
        if rep > 0:
            mle_ms.append(k[-1])
        for h in (a_num, a_den, dm, dm2):
            h.close()
    G, D = int(go[-1]), args.dim
    ebw_bytes = G * (48 * D + 16)
    out = {"shape": [args.pdfs, args.gauss, args.dim], "den_spread": args.den_spread, "host_form_s": round(host_s, 4), "device_equals_host_bitwise": same,
           "k4_ebw_update_ms": [round(x, 4) for x in ebw_ms], "ebw_update_call_ms": [round(x, 3) for x in ebw_wall],
           "k4_mle_update_ms": [round(x, 4) for x in mle_ms], "ebw_bytes": ebw_bytes,
           "ebw_GBps_at_median": round(ebw_bytes / (1e6 * float(np.median(ebw_ms))), 1), "mle_bytes": G * (32 * D + 8),
           "floored": r["floored"], "failed": r["failed"], "skipped": r["skipped"]}
    print(json.dumps(out))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
