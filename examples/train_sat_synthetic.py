#!/usr/bin/env python3
"""Speaker adaptation with fMLLR on the synthetic YES/NO task -- the flow of Kaldi's tri3 / decode_fmllr.sh on this project's device
path:

  1. every synthetic speaker's features pass through that speaker's own fixed affine map (the generator below);
  2. ML training of the monophone model on the distorted features (train_mono_synthetic.py's schedule);
  3. per-speaker fMLLR from the alignment: align -> ali-to-post -> gmm-est-fmllr -> transform-feats;
  4. re-estimation of the model on the transformed features (speaker adaptive training);
  5. two-pass decoding of held-out utterances of held-out speakers: decode with the ML model -> lattice posteriors -> fMLLR ->
     transform-feats -> decode with the adapted model.

Prints the per-frame likelihood and the WER before and after adaptation; exits 0 when the likelihood rose and the WER did not.

Usage: python examples/train_sat_synthetic.py [--utts 200] [--test-utts 30] [--speakers 5] [--iters 80]
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
from kaldi_hmm_gmm_amd.training_graph import (TrainingGraphCompiler, TrainingGraphCompilerOptions, equal_align,  # noqa: E402
                                              generate_hmm_topo)


def speaker_maps(n_spk, dim, rng, strength=0.25):
    """one fixed affine map per synthetic speaker: x -> A x + b, A near the identity"""
    return [(np.eye(dim) + strength * rng.standard_normal((dim, dim)) / np.sqrt(dim), 2.0 * strength * rng.standard_normal(dim))
            for _ in range(n_spk)]


def distort(utts, utt2spk, maps):
    return [(n, w, np.ascontiguousarray(x.astype(np.float64) @ maps[s][0].T + maps[s][1], np.float32)) for (n, w, x), s in zip(utts, utt2spk)]


def device_objects(am, tm, feats):
    """the model, the transition table and a features-only utterance set on the default context"""
    ctx = _gpu.default_context()
    go, gc, w, miv, iv = am.flat()
    dm = khg.DeviceModel(ctx, go, gc, miv, iv)
    dt = khg.DeviceTransitions(ctx, np.asarray(tm.transition_id_to_pdf_array(), np.int32))
    fo = np.concatenate([[0], np.cumsum([len(f) for f in feats])]).astype(np.int64)
    us = khg.UtteranceSet(ctx, None, fo, np.ascontiguousarray(np.concatenate(feats), np.float32))
    return dm, dt, us


def align(am, tm, names, graphs, feats):
    cfg = khg.AlignConfig(beam=6.0, retry_beam=40.0, careful=False)
    return khg.gmm_align_compiled_batch(am, tm, names, graphs, feats, cfg, acoustic_scale=0.1, transition_scale=1.0, self_loop_scale=0.1)


def logdet_per_frame(W, utt2spk, feats):
    ld = [np.linalg.slogdet(w[:, :-1].astype(np.float64))[1] for w in W]
    frames = np.array([len(f) for f in feats], np.float64)
    return float(sum(ld[s] * t for s, t in zip(utt2spk, frames)) / frames.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=200)
    ap.add_argument("--test-utts", type=int, default=30)
    ap.add_argument("--speakers", type=int, default=5, help="training speakers; the test utterances belong to 3 further ones")
    ap.add_argument("--iters", type=int, default=80)
    ap.add_argument("--sat-iters", type=int, default=4)
    ap.add_argument("--dim", type=int, default=23)
    ap.add_argument("--seed", type=int, default=3)
    args = ap.parse_args()
    rng = np.random.default_rng(args.seed)
    n_test_spk = 3
    clean = tr.make_data(args.utts + args.test_utts, args.dim, rng)
    maps = speaker_maps(args.speakers + n_test_spk, args.dim, np.random.default_rng(args.seed + 100))
    u2s_all = np.concatenate([np.arange(args.utts) % args.speakers, args.speakers + np.arange(args.test_utts) % n_test_spk]).astype(np.int32)
    utts = distort(clean, u2s_all, maps)
    train_utts, test_utts = utts[: args.utts], utts[args.utts:]
    u2s_train, u2s_test = u2s_all[: args.utts], u2s_all[args.utts:] - args.speakers
    names, feats = [u[0] for u in train_utts], [u[2] for u in train_utts]

    # ---- 2. ML training on the distorted features ----
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
    print(f"ML model on {args.speakers} distorted speakers: {am.num_gauss} Gaussians, per-frame likelihood {like_before:.4f}")

    # ---- 3. per-speaker fMLLR from the alignment ----
    dm, dt, us = device_objects(am, tm, feats)
    # ali-to-post on the device: the set holds the alignment (a set that ran khg_align itself has it already; this host-level
    # recipe aligned through gmm_align_compiled_batch, so the ids are put back once) and the posteriors never exist on the host
    us.upload_ali(np.concatenate([np.asarray(a if a else [0] * len(f), np.int32) for a, f in zip(r0["alignment"], feats)]))
    posts = khg.DevicePosteriors.from_alignment(us)
    est = khg.gmm_est_fmllr_batch(dm, dt, us, posts, u2s_train, n_spk=args.speakers)
    posts.close()
    assert (est["status"] == khg.FMLLR_OK).all(), est["status"]
    print("fMLLR per training speaker: objf_impr per frame " + " ".join(f"{i / c:.3f}" for i, c in zip(est["objf_impr"], est["count"])))
    sat_feats = [khg.transform_feats(f, est["W"][s]) for f, s in zip(feats, u2s_train)]
    khg.transform_feats_batch(us, u2s_train, est["W"])                    # ... and in place on the device set: the same rows
    for h in (us, dm, dt):
        h.close()

    # ---- 5a. first pass on the held-out speakers with the ML model, and their transforms from its lattices ----
    errs0, nref, graph, _ = dx.decode(tm, tree, am, lexicon, test_utts, log=lambda *a: None)
    tfeats = [u[2] for u in test_utts]
    cfg = khg.LatticeFasterDecoderConfig(max_active=7000, beam=13.0, lattice_beam=6.0)
    gc2 = TrainingGraphCompiler(tm, tree, lexicon, sil_phone=tr.SIL, sil_prob=0.5, opts=TrainingGraphCompilerOptions(transition_scale=1.0, self_loop_scale=1.0))
    res, dl = khg.get_raw_lattice_faster_device_batch(am, tm, gc2.compile_word_loop_graph(), tfeats, cfg, 0.1)
    post = dl.posteriors(1.0, 0.1)
    dm, dt, us = device_objects(am, tm, tfeats)
    est2 = khg.gmm_est_fmllr_batch(dm, dt, us, post, u2s_test, n_spk=n_test_spk)
    adapted = [khg.transform_feats(f, est2["W"][s]) for f, s in zip(tfeats, u2s_test)]
    for h in (post, dl, us, dm, dt):
        h.close()

    # ---- 4. re-estimation on the transformed features ----
    sat_am = khg.AmDiagGmm()
    sat_am.copy_from_am_diag_gmm(am)                                      # `am` stays the first pass's model
    tcfg = khg.MleTransitionUpdateConfig()
    for i in range(args.sat_iters):
        r = align(sat_am, tm, names, graphs, sat_feats)
        a = [x if x else old for x, old in zip(r["alignment"], r0["alignment"])]
        accs = khg.AccumAmDiagGmm()
        accs.init(sat_am, khg.GmmUpdateFlags.kGmmAll)
        _, tacc = khg.gmm_acc_stats_ali_batch(sat_am, accs, tm, sat_feats, a)
        khg.gmm_est(sat_am, accs, tm, tacc, tcfg, khg.MleDiagGmmOptions(), update_flags="mvwt", verbose=False)
    r1 = align(sat_am, tm, names, graphs, sat_feats)
    like_after = r1["tot_like"] / max(r1["frame_count"], 1) + logdet_per_frame(est["W"], u2s_train, feats)
    print(f"adapted model on the transformed features: per-frame likelihood {like_after:.4f} (with log |det A|), before {like_before:.4f}")

    # ---- 5b. second pass: the adapted model on the transformed features ----
    errs1, _, _, _ = dx.decode(tm, tree, sat_am, lexicon, [(n, w, x) for (n, w, _), x in zip(test_utts, adapted)], log=lambda *a: None)
    print(f"first pass (ML model, distorted features): WER {100.0 * errs0 / max(nref, 1):.2f}% ({errs0} / {nref})")
    print(f"second pass (fMLLR per test speaker, status {est2['status'].tolist()}, adapted model): WER {100.0 * errs1 / max(nref, 1):.2f}% ({errs1} / {nref})")
    ok = like_after > like_before and errs1 <= errs0
    print(f"RESULT like_before={like_before:.6f} like_after={like_after:.6f} wer_before={errs0 / max(nref, 1):.6f} wer_after={errs1 / max(nref, 1):.6f}")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
