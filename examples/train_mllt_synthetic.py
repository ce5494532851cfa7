#!/usr/bin/env python3
"""MLLT (semi-tied covariance) on the synthetic YES/NO task -- the flow of Kaldi's train_lda_mllt.sh, without the LDA, on this
project's device path:

  1. every feature vector passes through ONE fixed well-conditioned random matrix, so the dimensions are correlated and a
     diagonal-covariance model no longer fits;
  2. ML training of the monophone model on the mixed features (train_mono_synthetic.py's schedule);
  3. MLLT from the alignment: align -> ali-to-post on the device -> gmm-acc-mllt over all frames -> est-mllt;
  4. transform-feats in place with [M | 0], gmm-transform-means on the model, then more ML iterations on the transformed features;
  5. decoding of held-out utterances before and after.

Prints the per-frame likelihood (including log |det M|) and the WER before and after; exits 0 when the likelihood rose and the WER did
not.

Usage: python examples/train_mllt_synthetic.py [--utts 200] [--test-utts 30] [--iters 80] [--mllt-iters 4] [--mix 0.2]
"""
import argparse
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kaldi_hmm_gmm_amd as khg  # noqa: E402
import decode_synthetic as dx  # noqa: E402
import train_mono_synthetic as tr  # noqa: E402
from kaldi_hmm_gmm_amd import _gpu  # noqa: E402
from kaldi_hmm_gmm_amd.training_graph import TrainingGraphCompiler, equal_align, generate_hmm_topo  # noqa: E402


def mixing_matrix(dim, rng, strength):
    """a fixed well-conditioned matrix far enough from the identity that the mixed dimensions are visibly correlated"""
    return np.eye(dim) + strength * rng.standard_normal((dim, dim)) / np.sqrt(dim)


def align(am, tm, names, graphs, feats):
    cfg = khg.AlignConfig(beam=6.0, retry_beam=40.0, careful=False)
    return khg.gmm_align_compiled_batch(am, tm, names, graphs, feats, cfg, acoustic_scale=0.1, transition_scale=1.0, self_loop_scale=0.1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=200)
    ap.add_argument("--test-utts", type=int, default=30)
    ap.add_argument("--iters", type=int, default=80)
    ap.add_argument("--mllt-iters", type=int, default=4, help="ML iterations on the transformed features")
    ap.add_argument("--dim", type=int, default=23)
    ap.add_argument("--mix", type=float, default=0.2, help="strength of the mixing matrix I + mix N(0, 1) / sqrt(dim)")
    ap.add_argument("--seed", type=int, default=3)
    args = ap.parse_args()
    rng = np.random.default_rng(args.seed)
    clean = tr.make_data(args.utts + args.test_utts, args.dim, rng)
    R = mixing_matrix(args.dim, np.random.default_rng(args.seed + 100), args.mix)
    utts = [(n, w, np.ascontiguousarray(x.astype(np.float64) @ R.T, np.float32)) for n, w, x in clean]
    train_utts, test_utts = utts[: args.utts], utts[args.utts:]
    names, feats = [u[0] for u in train_utts], [u[2] for u in train_utts]

    # ---- 2. ML training on the mixed features ----
    topo = generate_hmm_topo(non_sil_phones=[tr.Y, tr.N], sil_phone=tr.SIL)
    tm, tree, am = khg.gmm_init_mono(topo, np.concatenate(feats[:10]))
    lexicon = {tr.YES: [(1.0, [tr.Y])], tr.NO: [(1.0, [tr.N])]}
    gcomp = TrainingGraphCompiler(tm, tree, lexicon, sil_phone=tr.SIL, sil_prob=0.5)
    graphs = gcomp.compile_graphs_from_text([u[1] for u in train_utts])
    ali = [equal_align(g, x.shape[0], rand_seed=3, num_retries=10)[1] for g, x in zip(graphs, feats)]
    targs = types.SimpleNamespace(iters=args.iters, out="", seed=args.seed)
    tr.train_resident(targs, train_utts, names, feats, tm, tree, am, graphs, ali, log=lambda *a: None)
    r0 = align(am, tm, names, graphs, feats)
    like_before = r0["tot_like"] / max(r0["frame_count"], 1)
    errs0, nref, _, _ = dx.decode(tm, tree, am, lexicon, test_utts, log=lambda *a: None)
    print(f"ML model on mixed features: {am.num_gauss} Gaussians, per-frame likelihood {like_before:.4f}, WER {100.0 * errs0 / max(nref, 1):.2f}%")

    # ---- 3. MLLT from the alignment, over every frame ----
    ctx = _gpu.default_context()
    go, gc, w, miv, iv = am.flat()
    dm = khg.DeviceModel(ctx, go, gc, miv, iv, w)
    dt = khg.DeviceTransitions(ctx, np.asarray(tm.transition_id_to_pdf_array(), np.int32))
    fo = np.concatenate([[0], np.cumsum([len(f) for f in feats])]).astype(np.int64)
    us = khg.UtteranceSet(ctx, None, fo, np.ascontiguousarray(np.concatenate(feats), np.float32))
    us.upload_ali(np.concatenate([np.asarray(a if a else [0] * len(f), np.int32) for a, f in zip(r0["alignment"], feats)]))
    posts = khg.DevicePosteriors.from_alignment(us)
    stats = khg.gmm_acc_mllt_batch(dm, dt, us, posts)
    posts.close()
    est = khg.est_mllt(stats)
    assert est["status"] == khg.MLLT_OK, est["status"]
    logdet = float(np.linalg.slogdet(est["M64"])[1])
    print(f"est-mllt: objf_impr per frame {est['objf_impr'] / est['count']:.4f} over {est['count']:.0f} frames, log |det M| {logdet:.4f}")

    # ---- 4. the features and the means through M, then more ML iterations ----
    one = np.zeros(len(feats), np.int32)
    khg.transform_feats_batch(us, one, est["W"][None])                     # in place on the device set ...
    khg.gmm_transform_means(est["M"], model=dm, am_gmm=am)                # ... the resident model and the host model: the same bits
    d = dm.download()
    assert np.asarray(d["means_invvars"]).tobytes() == np.asarray(am.flat()[3]).tobytes()
    mfeats = [khg.transform_feats(f, est["W"]) for f in feats]            # the host recipe below re-aligns on the same rows
    for h in (us, dm, dt, stats):
        h.close()
    r_mid = align(am, tm, names, graphs, mfeats)
    like_mid = r_mid["tot_like"] / max(r_mid["frame_count"], 1) + logdet
    tcfg = khg.MleTransitionUpdateConfig()
    for _ in range(args.mllt_iters):
        r = align(am, tm, names, graphs, mfeats)
        a = [x if x else old for x, old in zip(r["alignment"], r0["alignment"])]
        accs = khg.AccumAmDiagGmm()
        accs.init(am, khg.GmmUpdateFlags.kGmmAll)
        _, tacc = khg.gmm_acc_stats_ali_batch(am, accs, tm, mfeats, a)
        khg.gmm_est(am, accs, tm, tacc, tcfg, khg.MleDiagGmmOptions(), update_flags="mvwt", verbose=False)
    r1 = align(am, tm, names, graphs, mfeats)
    like_after = r1["tot_like"] / max(r1["frame_count"], 1) + logdet
    print(f"per-frame likelihood with log |det M|: before {like_before:.4f}, transformed features and means {like_mid:.4f}, "
          f"after {args.mllt_iters} more ML iterations {like_after:.4f}")

    # ---- 5. decoding on the transformed features ----
    ttest = [(n, w, khg.transform_feats(x, est["W"])) for n, w, x in test_utts]
    errs1, _, _, _ = dx.decode(tm, tree, am, lexicon, ttest, log=lambda *a: None)
    print(f"WER before {100.0 * errs0 / max(nref, 1):.2f}% ({errs0} / {nref}), after {100.0 * errs1 / max(nref, 1):.2f}% ({errs1} / {nref})")
    ok = like_after > like_before and errs1 <= errs0
    print(f"RESULT like_before={like_before:.6f} like_after={like_after:.6f} wer_before={errs0 / max(nref, 1):.6f} wer_after={errs1 / max(nref, 1):.6f}")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
