#!/usr/bin/env python3
"""LDA + MLLT on the synthetic YES/NO task -- the flow of Kaldi's train_lda_mllt.sh on this project's device path (DESIGN.md
sections 7n and 7m):

  1. 13-dimensional features whose single frames are noisy (--noise: the standard deviation of white noise added to every frame),
     so that a frame alone says little about its state and its neighbours help;
  2. ML training of the monophone model on the raw features (train_mono_synthetic.py's schedule), decoding of held-out utterances;
  3. align -> ali-to-post on the device -> acc-lda on +-4 spliced frames with silence weight 0 -> est-lda;
  4. splice-feats | transform-feats on the device into a new set on the projected rows; a model on the new features from the SAME
     alignment: flat start, acc-stats with the kept alignment, gmm-est; then a few ML iterations with realignment;
  5. MLLT on top (gmm-acc-mllt, est-mllt, gmm-transform-means); the two matrices compose into one final.mat;
  6. decoding of the held-out utterances through final.mat.

Prints the kept eigenvalues and the WER before and after; exits 0 when every held-out utterance decodes and the WER after is no
worse than before.

Usage: python examples/train_lda_mllt_synthetic.py [--utts 200] [--test-utts 30] [--iters 80] [--lda-iters 12] [--noise 3.0]
                                                   [--left 4] [--right 4] [--lda-dim 10]
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


def align(am, tm, names, graphs, feats, boost=None):
    cfg = khg.AlignConfig(beam=6.0, retry_beam=40.0, careful=False)
    if boost is not None:
        am = khg.gmm_boost_silence(am, tm, [tr.SIL], boost=boost)          # a boosted COPY aligns
    return khg.gmm_align_compiled_batch(am, tm, names, graphs, feats, cfg, acoustic_scale=0.1, transition_scale=1.0, self_loop_scale=0.1)


def ml_pass(am, tm, feats, ali, num_gauss, randn, first=False):
    accs = khg.AccumAmDiagGmm()
    accs.init(am, khg.GmmUpdateFlags.kGmmAll)
    _, tacc = khg.gmm_acc_stats_ali_batch(am, accs, tm, feats, ali)
    opts = khg.MleDiagGmmOptions()
    if first:
        opts.min_gaussian_occupancy = 3
    return khg.gmm_est(am, accs, tm, tacc, khg.MleTransitionUpdateConfig(), opts, mixup=num_gauss, perturb_factor=0.01, power=0.2,
                       min_count=20.0, update_flags="mvwt", verbose=False, randn=randn)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=200)
    ap.add_argument("--test-utts", type=int, default=30)
    ap.add_argument("--iters", type=int, default=80)
    ap.add_argument("--lda-iters", type=int, default=12, help="ML iterations on the projected features")
    ap.add_argument("--dim", type=int, default=13)
    ap.add_argument("--noise", type=float, default=3.0, help="standard deviation of the white noise added to every frame")
    ap.add_argument("--left", type=int, default=4)
    ap.add_argument("--right", type=int, default=4)
    ap.add_argument("--lda-dim", type=int, default=10)
    ap.add_argument("--seed", type=int, default=3)
    args = ap.parse_args()
    L, R = args.left, args.right
    rng = np.random.default_rng(args.seed)
    clean = tr.make_data(args.utts + args.test_utts, args.dim, rng)
    nrng = np.random.default_rng(args.seed + 100)
    utts = [(n, w, np.ascontiguousarray(x + args.noise * nrng.standard_normal(x.shape), np.float32)) for n, w, x in clean]
    train_utts, test_utts = utts[: args.utts], utts[args.utts:]
    names, feats = [u[0] for u in train_utts], [u[2] for u in train_utts]

    # ---- 2. ML training on the raw, noisy frames ----
    topo = generate_hmm_topo(non_sil_phones=[tr.Y, tr.N], sil_phone=tr.SIL)
    tm, tree, am = khg.gmm_init_mono(topo, np.concatenate(feats[:10]))
    lexicon = {tr.YES: [(1.0, [tr.Y])], tr.NO: [(1.0, [tr.N])]}
    gcomp = TrainingGraphCompiler(tm, tree, lexicon, sil_phone=tr.SIL, sil_prob=0.5)
    graphs = gcomp.compile_graphs_from_text([u[1] for u in train_utts])
    ali = [equal_align(g, x.shape[0], rand_seed=3, num_retries=10)[1] for g, x in zip(graphs, feats)]
    targs = types.SimpleNamespace(iters=args.iters, out="", seed=args.seed)
    tr.train_resident(targs, train_utts, names, feats, tm, tree, am, graphs, ali, log=lambda *a: None)
    errs0, nref, _, res0 = dx.decode(tm, tree, am, lexicon, test_utts, log=lambda *a: None)
    print(f"ML model on single frames (noise {args.noise}): {am.num_gauss} Gaussians, WER {100.0 * errs0 / max(nref, 1):.2f}% ({errs0} / {nref})")

    # ---- 3. LDA statistics from the alignment: ali-to-post on the device, silence weight 0 ----
    r0 = align(am, tm, names, graphs, feats)
    ali0 = [a if a else old for a, old in zip(r0["alignment"], ali)]
    ctx = _gpu.default_context()
    id2pdf = np.asarray(tm.transition_id_to_pdf_array(), np.int32)
    dt = khg.DeviceTransitions(ctx, id2pdf)
    fo = np.concatenate([[0], np.cumsum([len(f) for f in feats])]).astype(np.int64)
    us = khg.UtteranceSet(ctx, None, fo, np.ascontiguousarray(np.concatenate(feats), np.float32))
    us.upload_ali(np.concatenate([np.asarray(a, np.int32) for a in ali0]))
    posts = khg.DevicePosteriors.from_alignment(us)
    sil_tids = [t for t in range(1, len(id2pdf)) if tm.transition_id_to_phone(t) == tr.SIL]
    stats = khg.acc_lda_batch(dt, us, posts, left=L, right=R, silence_tids=sil_tids, silence_weight=0.0)
    posts.close()
    lda = khg.est_lda(stats, target_dim=args.lda_dim)
    assert lda["status"] == khg.LDA_OK, lda["status"]
    print(f"est-lda over {lda['count']:.0f} non-silence frames, {us.dim} x {L + R + 1} = {stats.dim_z} -> {args.lda_dim}; kept eigenvalues "
          + " ".join(f"{v:.3f}" for v in lda["eig"][: args.lda_dim]))

    # ---- 4. a new set on the projected rows; a model on them from the same alignment ----
    proj = khg.splice_transform_feats_batch(us, lda["M"], L, R)
    us2 = khg.UtteranceSet(ctx, None, fo, (proj.data_ptr(), proj), dim=args.lda_dim)
    rows = proj.cpu().numpy()
    pfeats = [np.ascontiguousarray(rows[fo[i]: fo[i + 1]]) for i in range(len(feats))]
    assert pfeats[0].tobytes() == khg.splice_transform_feats(feats[0], lda["M"], L, R).tobytes()
    tm2, tree2, am2 = khg.gmm_init_mono(topo, np.concatenate(pfeats[:10]))                # flat start
    randn = tr.seeded_randn(args.seed + 2)
    num_gauss, max_gauss = am2.num_pdfs, 4 * am2.num_pdfs
    inc = max(1, (max_gauss - num_gauss) // max(1, args.lda_iters // 2))
    ali2 = ali0
    for i in range(args.lda_iters):
        if i >= 2:
            r = align(am2, tm2, names, graphs, pfeats, boost=1.0)
            ali2 = [a if a else old for a, old in zip(r["alignment"], ali2)]
        ml_pass(am2, tm2, pfeats, ali2, num_gauss, randn, first=(i == 0))
        num_gauss = min(max_gauss, num_gauss + inc)
    r1 = align(am2, tm2, names, graphs, pfeats)
    ali2 = [a if a else old for a, old in zip(r1["alignment"], ali2)]

    # ---- 5. MLLT on top, on the resident projected set ----
    go, gc, w, miv, iv = am2.flat()
    dm2 = khg.DeviceModel(ctx, go, gc, miv, iv, w)
    dt2 = khg.DeviceTransitions(ctx, np.asarray(tm2.transition_id_to_pdf_array(), np.int32))
    us2.upload_ali(np.concatenate([np.asarray(a, np.int32) for a in ali2]))
    posts2 = khg.DevicePosteriors.from_alignment(us2)
    mstats = khg.gmm_acc_mllt_batch(dm2, dt2, us2, posts2)
    posts2.close()
    mllt = khg.est_mllt(mstats)
    assert mllt["status"] == khg.MLLT_OK, mllt["status"]
    khg.gmm_transform_means(mllt["M"], model=dm2, am_gmm=am2)
    final = khg.compose_with_lda(mllt["M"], lda["M"])                                     # one final.mat: [lda_dim, dim_z]
    print(f"est-mllt: objf_impr per frame {mllt['objf_impr'] / mllt['count']:.4f} over {mllt['count']:.0f} frames; final.mat {final.shape}")
    for h in (us, us2, dt, dt2, dm2, stats, mstats):
        h.close()
    ffeats = [khg.splice_transform_feats(f, final, L, R) for f in feats]
    for _ in range(2):
        r = align(am2, tm2, names, graphs, ffeats)
        ali2 = [a if a else old for a, old in zip(r["alignment"], ali2)]
        ml_pass(am2, tm2, ffeats, ali2, am2.num_gauss, randn)

    # ---- 6. decoding through final.mat ----
    ttest = [(n, w, khg.splice_transform_feats(x, final, L, R)) for n, w, x in test_utts]
    errs1, _, _, res1 = dx.decode(tm2, tree2, am2, lexicon, ttest, log=lambda *a: None)
    failed = sum(1 for r in res1 if not r["ok"])
    print(f"WER before {100.0 * errs0 / max(nref, 1):.2f}% ({errs0} / {nref}), after LDA + MLLT {100.0 * errs1 / max(nref, 1):.2f}% ({errs1} / {nref}), "
          f"{failed} utterances failed to decode")
    print(f"RESULT wer_before={errs0 / max(nref, 1):.6f} wer_after={errs1 / max(nref, 1):.6f} failed={failed} "
          f"eig={','.join(f'{v:.4f}' for v in lda['eig'][: args.lda_dim])}")
    return 0 if failed == 0 and errs1 <= errs0 else 1


if __name__ == "__main__":
    sys.exit(main())
