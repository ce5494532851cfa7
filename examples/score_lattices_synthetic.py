#!/usr/bin/env python3
"""Scoring a decode without leaving the device: the sweep of Kaldi's score.sh and lattice-oracle on the lattices one decode left in HBM.

The task is the YES/NO task of decode_lm_rescore_synthetic.py (the two words sound alike, so the decode makes errors): a monophone
model trained on the training half, ONE lattice-faster decode of the held-out half on the shared word-loop graph, and then

    table, best = score_lattices(lats, refs, lmwts=range(7, 18), penalties=(0.0, 0.5, 1.0), lattice_acoustic_scale=0.1)
                                                   lattice-scale | lattice-add-penalty | lattice-best-path | compute-wer at 33 points:
                                                   ONE call (khg_lattices_wer), only the counts come back
    oracle      = lats.oracle(refs)                lattice-oracle: the fewest errors any path of the lattice makes -- whether a bad
                                                   WER is the lattice's fault (beam too tight) or the scales' fault

The point (LMWT 10, penalty 0) is also formed the way the other examples score -- best_path, the words downloaded, compute_wer on the
host -- and compared, and the oracle of every lattice is formed on the host (Lattice.oracle) and compared.

Usage: python examples/score_lattices_synthetic.py [--utts 200] [--test-utts 100] [--iters 80] [--lattice-beam 8]
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

LMWTS = list(range(7, 18))
PENALTIES = (0.0, 0.5, 1.0)
ACOUSTIC_SCALE = 0.1          # of the decode: the lattices hold acoustic costs at this scale


def evaluate(tm, tree, am, lexicon, train_utts, test_utts, lattice_beam):
    transcripts = [u[1] for u in train_utts]
    counts = np.bincount(np.concatenate(transcripts), minlength=3)[1:3].astype(np.float64)
    word_probs = {tr.YES: float(counts[0] / counts.sum()), tr.NO: float(counts[1] / counts.sum())}
    gc = TrainingGraphCompiler(tm, tree, lexicon, sil_phone=tr.SIL, sil_prob=0.5,
                               opts=TrainingGraphCompilerOptions(transition_scale=1.0, self_loop_scale=1.0))
    graph = gc.compile_word_loop_graph(word_probs)
    config = khg.LatticeFasterDecoderConfig(max_active=7000, beam=13.0, lattice_beam=lattice_beam)
    feats, refs = [u[2] for u in test_utts], [u[1] for u in test_utts]
    U = len(feats)
    _, lats = khg.get_raw_lattice_faster_device_batch(am, tm, graph, feats, config, ACOUSTIC_SCALE)
    table, best = khg.score_lattices(lats, refs, LMWTS, PENALTIES, lattice_acoustic_scale=ACOUSTIC_SCALE)
    orc = lats.oracle(refs)
    nref = sum(len(r) for r in refs)
    # the way the other examples score, at (LMWT 10, penalty 0): the words come to the host
    bp = lats.best_path(np.ones(1, np.float32), np.ones(1, np.float32))
    hyps = [bp["words"][bp["words_off"][u]: bp["words_off"][u + 1]].tolist() if bp["status"][u] & 1 else [] for u in range(U)]
    wer10, tot10 = khg.compute_wer(refs, hyps)
    agree = tot10["errors"] == table[(10, 0.0)]["errors"] and tot10["insertions"] == table[(10, 0.0)]["insertions"]
    for u, L in enumerate(lats.download()):
        h = L.oracle(refs[u])
        agree = agree and h["counts"].tolist() == orc["counts"][u].tolist() and \
            h["words"].tolist() == orc["words"][orc["words_off"][u]: orc["words_off"][u + 1]].tolist()
    r = {"table": table, "best": best, "oracle": orc["counts"].astype(np.int64).sum(axis=0).tolist(), "ref_words": nref,
         "oracle_failed": int(sum(1 for s in orc["status"] if not s & 1)), "states": int(lats.state_off[-1]), "arcs": int(lats.arc_off[-1]),
         "host_agrees": bool(agree), "utts": U}
    lats.close()
    return r


def report(r):
    print(f"{r['utts']} held-out utterances, {r['ref_words']} reference words; lattices: {r['states']} states, {r['arcs']} arcs")
    print("WER % (insertions / deletions / substitutions)   penalty " + "".join(f"{p:>22.1f}" for p in PENALTIES))
    for w in LMWTS:
        row = [r["table"][(w, p)] for p in PENALTIES]
        print(f"LMWT {w:2d}                                                " +
              "".join(f"{x['wer']:8.2f} ({x['insertions']:3d}/{x['deletions']:3d}/{x['substitutions']:3d})" for x in row))
    b = r["table"][r["best"]]
    o = r["oracle"]
    print(f"best point: LMWT {r['best'][0]}, penalty {r['best'][1]}: WER {b['wer']:.2f}% ({b['errors']} / {r['ref_words']})")
    print(f"oracle: WER {100.0 * o[0] / r['ref_words']:.2f}% ({o[0]} / {r['ref_words']}: {o[1]} ins, {o[2]} del, {o[3]} sub), "
          f"{r['oracle_failed']} lattices without a path; host and device {'identical' if r['host_agrees'] else 'DIFFERENT'}")


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
    args = ap.parse_args(argv)
    train_utts, test_utts = lmx.make_data(args.utts, args.test_utts, args.dim, np.random.default_rng(args.seed), args.p_switch, 0.0, args.diff_dims)
    tm, tree, am, lexicon = lmx.train(args, train_utts)
    r = evaluate(tm, tree, am, lexicon, train_utts, test_utts, args.lattice_beam)
    report(r)
    print(f"RESULT best_wer={r['table'][r['best']]['errors'] / r['ref_words']:.4f} best_lmwt={r['best'][0]} best_penalty={r['best'][1]} "
          f"oracle_wer={r['oracle'][0] / r['ref_words']:.4f} host_agrees={int(r['host_agrees'])}")
    return 0 if r["host_agrees"] else 1


if __name__ == "__main__":
    sys.exit(main())
