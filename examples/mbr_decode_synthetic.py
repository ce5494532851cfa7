#!/usr/bin/env python3
"""Minimum Bayes risk decoding and word confidences without leaving the device.

The task is the YES/NO task of score_lattices_synthetic.py (the two words sound alike, so the decode makes errors): a monophone model
trained on the training half, ONE lattice-faster decode of the held-out half on the shared word-loop graph, and then, on the lattices
the decode left in HBM,

    out = lattice_mbr_decode_batch(lats, 1.0, 1.0 / (LMWT * 0.1))      lattice-mbr-decode: the word sequence of least expected word
                                                                       error, a confidence per word, the confusion bins (sausages)

beside the MAP hypothesis (best_path at the same scales).  Printed: the MAP WER, the MBR WER, and the mean confidence of the MBR words
that are correct against those that are wrong (by the edit-distance alignment with the reference).  Every lattice is also decoded on
the host (Lattice.mbr) with the weights the device handed back, and compared: the two must be identical.

Usage: python examples/mbr_decode_synthetic.py [--utts 200] [--test-utts 100] [--iters 80] [--lattice-beam 8] [--lmwt 10]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_lm_rescore_synthetic as lmx  # noqa: E402
import kaldi_hmm_gmm_amd as khg  # noqa: E402
import train_mono_synthetic as tr  # noqa: E402
from kaldi_hmm_gmm_amd.training_graph import TrainingGraphCompiler, TrainingGraphCompilerOptions  # noqa: E402

ACOUSTIC_SCALE = 0.1          # of the decode: the lattices hold acoustic costs at this scale


def matched(ref, hyp):
    """which words of hyp the edit-distance alignment matches with an equal word of ref (diagonal first, as compute-wer)"""
    R, H = len(ref), len(hyp)
    d = np.zeros((H + 1, R + 1), np.int64)
    d[0, :], d[:, 0] = np.arange(R + 1), np.arange(H + 1)
    for i in range(1, H + 1):
        for j in range(1, R + 1):
            d[i, j] = min(d[i - 1, j - 1] + (hyp[i - 1] != ref[j - 1]), d[i - 1, j] + 1, d[i, j - 1] + 1)
    ok, i, j = [False] * H, H, R
    while i > 0 and j > 0:
        if d[i, j] == d[i - 1, j - 1] + (hyp[i - 1] != ref[j - 1]):
            ok[i - 1] = hyp[i - 1] == ref[j - 1]
            i, j = i - 1, j - 1
        elif d[i, j] == d[i - 1, j] + 1:
            i -= 1
        else:
            j -= 1
    return ok


def evaluate(tm, tree, am, lexicon, train_utts, test_utts, lattice_beam, lmwt):
    transcripts = [u[1] for u in train_utts]
    counts = np.bincount(np.concatenate(transcripts), minlength=3)[1:3].astype(np.float64)
    word_probs = {tr.YES: float(counts[0] / counts.sum()), tr.NO: float(counts[1] / counts.sum())}
    gc = TrainingGraphCompiler(tm, tree, lexicon, sil_phone=tr.SIL, sil_prob=0.5,
                               opts=TrainingGraphCompilerOptions(transition_scale=1.0, self_loop_scale=1.0))
    graph = gc.compile_word_loop_graph(word_probs)
    config = khg.LatticeFasterDecoderConfig(max_active=7000, beam=13.0, lattice_beam=lattice_beam)
    feats, refs = [u[2] for u in test_utts], [[int(w) for w in u[1]] for u in test_utts]
    U = len(feats)
    _, lats = khg.get_raw_lattice_faster_device_batch(am, tm, graph, feats, config, ACOUSTIC_SCALE)
    gs, as_ = 1.0, 1.0 / (lmwt * ACOUSTIC_SCALE)
    bp = lats.best_path(np.array([gs], np.float32), np.array([as_], np.float32))
    maps = [bp["words"][bp["words_off"][u]: bp["words_off"][u + 1]].tolist() if bp["status"][u] & 1 else [] for u in range(U)]
    out = khg.lattice_mbr_decode_batch(lats, gs, as_)
    conf_only = khg.lattice_mbr_decode_batch(lats, gs, as_, decode_mbr=False)
    mbrs = [o["words"].tolist() for o in out]
    map_wer, _ = khg.compute_wer(refs, maps)
    mbr_wer, _ = khg.compute_wer(refs, mbrs)
    good, bad, worst, agree = [], [], 0.0, True
    for u, L in enumerate(lats.download()):
        o = out[u]
        if not o["status"] & 1:
            continue
        for c, ok in zip(o["conf"], matched(refs[u], mbrs[u])):
            (good if ok else bad).append(float(c))
        bound = (L.num_states + L.num_arcs_total) * (2 * len(mbrs[u]) + 2) * 2.0 ** -52
        worst = max(worst, float(np.abs(o["gamma"].sum(axis=1) - 1.0).max()) / bound)
        h = L.mbr(gs, as_, arc_cond=o["arc_cond"], final_cond=o["final_cond"])
        agree = agree and h["status"] == o["status"] and h["iters"] == o["iters"] and h["words"].tolist() == mbrs[u] and \
            h["bayes_risk"] == o["bayes_risk"] and h["gamma"].tobytes() == o["gamma"].tobytes() and h["conf"].tobytes() == o["conf"].tobytes()
        agree = agree and conf_only[u]["words"].tolist() == maps[u] and conf_only[u]["iters"] == 0
    r = {"utts": U, "ref_words": sum(len(x) for x in refs), "states": int(lats.state_off[-1]), "arcs": int(lats.arc_off[-1]), "map_wer": map_wer,
         "mbr_wer": mbr_wer, "changed": sum(a != b for a, b in zip(maps, mbrs)), "iters": [o["iters"] for o in out],
         "risk": float(np.mean([o["bayes_risk"] for o in out if o["status"] & 1] or [0.0])), "conf_good": good, "conf_bad": bad,
         "gamma_sum_over_bound": worst, "host_agrees": bool(agree), "failed": sum(1 for o in out if not o["status"] & 1),
         "sausage": out[0]["sausage"] if out and out[0]["status"] & 1 else []}
    lats.close()
    return r


def report(r, lmwt):
    print(f"{r['utts']} held-out utterances, {r['ref_words']} reference words; lattices: {r['states']} states, {r['arcs']} arcs; LMWT {lmwt}")
    print(f"MAP WER {r['map_wer']:.2f}%   MBR WER {r['mbr_wer']:.2f}%   ({r['changed']} hypotheses changed; updates per utterance: "
          f"mean {np.mean(r['iters']):.2f}, most {max(r['iters'])}; mean Bayes risk {r['risk']:.3f}; {r['failed']} lattices without a path)")
    mg = float(np.mean(r["conf_good"])) if r["conf_good"] else float("nan")
    mb = float(np.mean(r["conf_bad"])) if r["conf_bad"] else float("nan")
    print(f"mean confidence: {mg:.3f} over {len(r['conf_good'])} correct words, {mb:.3f} over {len(r['conf_bad'])} wrong words")
    print("the bins of utterance 0: " + " | ".join(" ".join(f"{w}:{p:.2f}" for w, p in b[:3]) for b in r["sausage"][:9]))
    print(f"largest |sum of a bin - 1| / bound: {r['gamma_sum_over_bound']:.3g}; host and device {'identical' if r['host_agrees'] else 'DIFFERENT'}")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=200)
    ap.add_argument("--test-utts", type=int, default=100)
    ap.add_argument("--iters", type=int, default=80)
    ap.add_argument("--dim", type=int, default=23)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--p-switch", type=float, default=0.85)
    ap.add_argument("--diff-dims", type=int, default=4)
    ap.add_argument("--lattice-beam", type=float, default=8.0)
    ap.add_argument("--lmwt", type=int, default=10)
    args = ap.parse_args(argv)
    train_utts, test_utts = lmx.make_data(args.utts, args.test_utts, args.dim, np.random.default_rng(args.seed), args.p_switch, 0.0, args.diff_dims)
    tm, tree, am, lexicon = lmx.train(args, train_utts)
    r = evaluate(tm, tree, am, lexicon, train_utts, test_utts, args.lattice_beam, args.lmwt)
    report(r, args.lmwt)
    print(f"RESULT map_wer={r['map_wer'] / 100:.4f} mbr_wer={r['mbr_wer'] / 100:.4f} gamma_sum_over_bound={r['gamma_sum_over_bound']:.4g} "
          f"failed={r['failed']} host_agrees={int(r['host_agrees'])}")
    return 0 if r["host_agrees"] and r["gamma_sum_over_bound"] <= 1.0 else 1


if __name__ == "__main__":
    sys.exit(main())
