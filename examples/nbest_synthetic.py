#!/usr/bin/env python3
"""N-best lists of the lattices a decode left on the device.

The task is the YES/NO task of determinize_synthetic.py: a monophone model trained on the training half, ONE lattice-faster decode of
the held-out half on the shared word-loop graph, and then, on the lattices the decode left in HBM,

    det, status, stats = lats.determinize(gs, as, lattice_beam)       one path per word sequence
    nb = det.nbest(10, gs, as)                                         the 10 cheapest of them: the 10 best distinct word sequences
    lists = khg.NbestList(nb.download())

which is lattice-to-nbest | nbest-to-linear, the form in which a recipe hands alternatives to anything that is not a WFST.  Here that
is a bigram NgramLm estimated from the training transcripts: every entry is rescored on the host (its total plus the LM's cost of its
words) and the cheapest is picked.  Printed: the WER of the 1-best, of the rescored pick, and of the best entry of each list (the
oracle of the list, which can only be better than the 1-best).  Every list is also made on the host (Lattice.nbest) and compared:
the two must be identical.

Usage: python examples/nbest_synthetic.py [--utts 200] [--test-utts 100] [--iters 80] [--lattice-beam 8] [--lmwt 10] [--n 10]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_lm_rescore_synthetic as lmx  # noqa: E402
import kaldi_hmm_gmm_amd as khg  # noqa: E402
import train_mono_synthetic as tr  # noqa: E402
from kaldi_hmm_gmm_amd.training_graph import TrainingGraphCompiler, TrainingGraphCompilerOptions  # noqa: E402

ACOUSTIC_SCALE = 0.1          # of the decode: the lattices hold acoustic costs at this scale


def evaluate(tm, tree, am, lexicon, train_utts, test_utts, lattice_beam, lmwt, n, state_factor=8):
    transcripts = [u[1] for u in train_utts]
    counts = np.bincount(np.concatenate(transcripts), minlength=3)[1:3].astype(np.float64)
    word_probs = {tr.YES: float(counts[0] / counts.sum()), tr.NO: float(counts[1] / counts.sum())}
    gc = TrainingGraphCompiler(tm, tree, lexicon, sil_phone=tr.SIL, sil_prob=0.5,
                               opts=TrainingGraphCompilerOptions(transition_scale=1.0, self_loop_scale=1.0))
    graph = gc.compile_word_loop_graph(word_probs)
    config = khg.LatticeFasterDecoderConfig(max_active=7000, beam=13.0, lattice_beam=lattice_beam, determinize_lattice=False)
    feats, refs = [u[2] for u in test_utts], [[int(w) for w in u[1]] for u in test_utts]
    U = len(feats)
    gs, as_ = 1.0, 1.0 / (lmwt * ACOUSTIC_SCALE)
    _, raw = khg.get_raw_lattice_faster_device_batch(am, tm, graph, feats, config, ACOUSTIC_SCALE)
    det, status, _ = raw.determinize(gs, as_, lattice_beam, config.det_opts.delta, state_factor)
    det.nbest(n, gs, as_).close()          # (the first call builds the handle's in-arc index)
    t0 = time.time()
    nb = det.nbest(n, gs, as_)
    lists = khg.NbestList(nb.download())
    t_dev = time.time() - t0
    # the host form on the downloaded lattices
    agree = True
    t0 = time.time()
    host = [L.nbest_with_status(n, gs, as_) for L in det.download()]
    t_host = time.time() - t0
    for u, (got, hst, _) in enumerate(host):
        agree = agree and hst == int(lists.status[u]) and [tuple(x) for x in got] == [tuple(x) for x in lists.entries(u)]
    # rescoring on the host with a bigram
    bigram = khg.estimate_ngram_lm(transcripts, 2, [tr.YES, tr.NO], 0.5)
    best, picked, oracle = [], [], []
    distinct = True
    for u in range(U):
        entries = lists.entries(u)
        if not entries:
            best.append([]); picked.append([]); oracle.append([])
            continue
        seqs = [tuple(e[0]) for e in entries]
        distinct = distinct and len(set(seqs)) == len(seqs)
        best.append(entries[0][0])
        picked.append(min(entries, key=lambda e: e[3] + bigram.score(e[0]))[0])
        oracle.append(min(entries, key=lambda e: int(khg.edit_distance_counts(np.array(refs[u], np.int32), np.array(e[0], np.int32))[0]))[0])
    r = {"utts": U, "ref_words": sum(len(x) for x in refs), "n": n, "entries": int(lists.counts.sum()), "full": int((lists.counts == n).sum()),
         "failed": int(sum(1 for s in lists.status if not s & 1)), "det_failed": int(sum(1 for s in status if not s & 1)),
         "host_agrees": bool(agree), "distinct": bool(distinct), "device_bytes": int(nb.device_bytes), "det_states": int(det.state_off[-1]), "det_arcs": int(det.arc_off[-1]),
         "call_ms": 1e3 * t_dev, "host_ms": 1e3 * t_host,
         "wer_best": khg.compute_wer(refs, best)[0], "wer_rescored": khg.compute_wer(refs, picked)[0], "wer_oracle": khg.compute_wer(refs, oracle)[0]}
    for h in (nb, det, raw):
        h.close()
    return r


def report(r, lattice_beam, lmwt):
    print(f"{r['utts']} held-out utterances, {r['ref_words']} reference words; lattice beam {lattice_beam}, LMWT {lmwt}")
    print(f"{r['n']}-best lists: {r['entries']} entries, {r['full']} lists full, {r['failed']} utterances without a list "
          f"({r['det_failed']} refused by determinize); {r['device_bytes']} bytes on the device")
    print(f"determinized lattices: {r['det_states']} states, {r['det_arcs']} arcs; nbest with its download {r['call_ms']:.2f} ms, download of the lattices "
          f"and a loop of Lattice.nbest {r['host_ms']:.2f} ms")
    print(f"WER of the 1-best {r['wer_best']:.2f}%, of the bigram-rescored pick {r['wer_rescored']:.2f}%, of the best entry of each list {r['wer_oracle']:.2f}%")
    print(f"word sequences of a list {'pairwise distinct' if r['distinct'] else 'NOT DISTINCT'}; host and device {'identical' if r['host_agrees'] else 'DIFFERENT'}")


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
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--state-factor", type=int, default=8)
    args = ap.parse_args(argv)
    train_utts, test_utts = lmx.make_data(args.utts, args.test_utts, args.dim, np.random.default_rng(args.seed), args.p_switch, 0.0, args.diff_dims)
    tm, tree, am, lexicon = lmx.train(args, train_utts)
    r = evaluate(tm, tree, am, lexicon, train_utts, test_utts, args.lattice_beam, args.lmwt, args.n, args.state_factor)
    report(r, args.lattice_beam, args.lmwt)
    print(f"RESULT wer_best={r['wer_best']:.4f} wer_rescored={r['wer_rescored']:.4f} wer_oracle={r['wer_oracle']:.4f} entries={r['entries']} "
          f"failed={r['failed']} distinct={int(r['distinct'])} host_agrees={int(r['host_agrees'])}")
    return 0 if r["host_agrees"] and r["distinct"] else 1


if __name__ == "__main__":
    sys.exit(main())
