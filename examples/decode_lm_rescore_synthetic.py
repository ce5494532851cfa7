#!/usr/bin/env python3
"""Two-pass decoding with a language model: decode once on the shared unigram word-loop graph, then rescore the lattices that stay on
the device with a bigram -- the shape of every Kaldi recipe (decode with a small LM, lattice-lmrescore with the real one).

The task is the synthetic YES/NO task of decode_synthetic.py with two changes.  The transcripts are drawn from a first-order Markov
chain over the two words (a word is followed by the other one with probability --p-switch, 0.85), so a bigram knows something the
unigram of the decoding graph does not.  And the two words sound alike: the means of the phones Y and N differ in the first
--diff-dims (4) of the 23 dimensions only, in training and in the held-out data, so the acoustic model alone confuses the words and
the unigram decode makes errors.  (--mix m instead moves every state of a held-out word's phone to (1 - m) * its own mean + m * the
other word's, under a model trained on the unmixed task; at --diff-dims 0 --mix 0 this is decode_synthetic.py's task, WER 0.)

    graph        = compile_word_loop_graph(word_probs)               H o C o L o G, G the unigram of the training transcripts
    _, lats      = get_raw_lattice_faster_device_batch(...)          ONE decode; the raw lattices stay in HBM
    no_lm, ...   = lats.lm_rescore(DeviceLm(NgramLm.unigram(word_probs)), -1)      the graph's unigram taken out
    rescored, .. = no_lm.lm_rescore(DeviceLm(estimate_ngram_lm(train, 2, words)), +1)  the bigram put in
    lats.best_path / rescored.best_path over the LM weights 7 .. 17  WER before and after, from that one decode

Every held-out hypothesis is also formed on the host (Lattice.lm_rescore twice, Lattice.best_path) and compared.

Usage: python examples/decode_lm_rescore_synthetic.py [--utts 200] [--test-utts 100] [--iters 80] [--diff-dims 4] [--mix 0]
"""
import argparse
import os
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_synthetic as dx  # noqa: E402
import kaldi_hmm_gmm_amd as khg  # noqa: E402
import train_mono_synthetic as tr  # noqa: E402
from kaldi_hmm_gmm_amd.training_graph import (TrainingGraphCompiler, TrainingGraphCompilerOptions, equal_align,  # noqa: E402
                                              generate_hmm_topo)

WEIGHTS = np.arange(7, 18)


def make_data(n_train, n_test, dim, rng, p_switch, mix, diff_dims=0):
    """tr.make_data with Markov-chain transcripts.  The held-out utterances (the last n_test) emit every state of a word's phone around
    (1 - mix) * its own mean + mix * the mean of the same state of the other word's phone.  diff_dims = k > 0: the two phones' means
    differ in the first k dimensions only, in training too."""
    nstate = {tr.SIL: 5, tr.Y: 3, tr.N: 3}
    base = {tr.SIL: 0, tr.Y: 5, tr.N: 8}
    means = (rng.standard_normal((11, dim)) * 2.5).astype(np.float32)
    if diff_dims:
        means[8:11, diff_dims:] = means[5:8, diff_dims:]
    mixed = means.copy()
    mixed[5:8] = (1.0 - mix) * means[5:8] + mix * means[8:11]
    mixed[8:11] = (1.0 - mix) * means[8:11] + mix * means[5:8]
    utts = []
    for u in range(n_train + n_test):
        words = [int(rng.integers(1, 3))]
        for _ in range(int(rng.integers(3, 9)) - 1):
            words.append(3 - words[-1] if rng.random() < p_switch else words[-1])
        phones = [tr.SIL] if rng.random() < 0.5 else []
        for w in words:
            phones.append(tr.Y if w == tr.YES else tr.N)
            if rng.random() < 0.5:
                phones.append(tr.SIL)
        mu = mixed if u >= n_train else means
        x = []
        for ph in phones:
            for s in range(nstate[ph]):
                d = int(rng.integers(3, 9))
                x.append(mu[base[ph] + s] + rng.standard_normal((d, dim)).astype(np.float32))
        utts.append((f"utt{u:04d}", words, np.concatenate(x).astype(np.float32)))
    return utts[:n_train], utts[n_train:]


def train(args, train_utts):
    """decode_synthetic.train on given utterances"""
    feats = [u[2] for u in train_utts]
    topo = generate_hmm_topo(non_sil_phones=[tr.Y, tr.N], sil_phone=tr.SIL)
    tm, tree, am = khg.gmm_init_mono(topo, np.concatenate(feats[:10]))
    lexicon = {tr.YES: [(1.0, [tr.Y])], tr.NO: [(1.0, [tr.N])]}
    gc = TrainingGraphCompiler(tm, tree, lexicon, sil_phone=tr.SIL, sil_prob=0.5)
    graphs = gc.compile_graphs_from_text([u[1] for u in train_utts])
    ali = [equal_align(g, x.shape[0], rand_seed=3, num_retries=10)[1] for g, x in zip(graphs, feats)]
    targs = types.SimpleNamespace(iters=args.iters, out="", seed=args.seed)
    rc = tr.train_resident(targs, train_utts, [u[0] for u in train_utts], feats, tm, tree, am, graphs, ali, log=lambda *a: None)
    print(f"trained on {len(train_utts)} utterances: {am.num_gauss} Gaussians, training alignments {'ok' if rc == 0 else 'INCOMPLETE'}")
    return tm, tree, am, lexicon


def _hyps(bp, U):
    """DeviceLattices.best_path's dict -> words[k][u]"""
    out = []
    for k in range(len(WEIGHTS)):
        row = []
        for u in range(U):
            o = k * U + u
            row.append(bp["words"][bp["words_off"][o]: bp["words_off"][o + 1]].tolist() if bp["status"][o] & 1 else [])
        out.append(row)
    return out


def _wer(hyps, test_utts):
    e = sum(dx.edit_distance(u[1], h) for u, h in zip(test_utts, hyps))
    return e, sum(len(u[1]) for u in test_utts)


def evaluate(tm, tree, am, lexicon, train_utts, test_utts, check_host=True):
    """-> dict: errors of the unigram decode and of the bigram-rescored lattices at every LM weight, the growth, host agreement"""
    transcripts = [u[1] for u in train_utts]
    counts = np.bincount(np.concatenate(transcripts), minlength=3)[1:3].astype(np.float64)
    word_probs = {tr.YES: float(counts[0] / counts.sum()), tr.NO: float(counts[1] / counts.sum())}
    gc = TrainingGraphCompiler(tm, tree, lexicon, sil_phone=tr.SIL, sil_prob=0.5,
                               opts=TrainingGraphCompilerOptions(transition_scale=1.0, self_loop_scale=1.0))
    graph = gc.compile_word_loop_graph(word_probs)
    config = khg.LatticeFasterDecoderConfig(max_active=7000, beam=13.0, lattice_beam=8.0)
    feats = [u[2] for u in test_utts]
    U = len(feats)
    _, lats = khg.get_raw_lattice_faster_device_batch(am, tm, graph, feats, config, 0.1)
    unigram = khg.NgramLm.unigram(word_probs)
    bigram = khg.estimate_ngram_lm(transcripts, 2, [tr.YES, tr.NO], 0.5)
    d_uni, d_bi = khg.DeviceLm(unigram), khg.DeviceLm(bigram)
    no_lm, st1, _ = lats.lm_rescore(d_uni, -1.0)
    rescored, st2, stats = no_lm.lm_rescore(d_bi, 1.0)
    # the lattices hold acoustic costs at scale 0.1 = LM weight 10: weight w re-weights them by 10 / w
    gs, as_ = np.ones(len(WEIGHTS), np.float32), (10.0 / WEIGHTS).astype(np.float32)
    before, after = _hyps(lats.best_path(gs, as_), U), _hyps(rescored.best_path(gs, as_), U)
    r = {"weights": WEIGHTS.tolist(), "before": [_wer(h, test_utts) for h in before], "after": [_wer(h, test_utts) for h in after],
         "stats": stats, "failed": int(sum(1 for s in st2 if not s & 1)), "states_in": int(lats.state_off[-1]), "graph_states": graph.num_states,
         "host_agrees": None}
    if check_host:
        agree = True
        for u, L in enumerate(lats.download()):
            H = L.lm_rescore(unigram, -1.0)[0].lm_rescore(bigram, 1.0)[0]
            for k in range(len(WEIGHTS)):
                b = H.best_path(float(gs[k]), float(as_[k]))
                agree = agree and (b["words"] if b["status"] & 1 else []) == after[k][u]
        r["host_agrees"] = agree
    for h in (rescored, no_lm, lats, d_uni, d_bi):
        h.close()
    return r


def report(r):
    nref = r["before"][0][1]
    print(f"decoded {r['states_in']} lattice states on a {r['graph_states']}-state word-loop graph; bigram rescoring: states "
          f"{r['stats']['in_states']} -> {r['stats']['out_states']}, arcs {r['stats']['in_arcs']} -> {r['stats']['out_arcs']}, "
          f"largest history set {r['stats']['max_hist']}, {r['failed']} utterances failed")
    for w, (eb, _), (ea, _) in zip(r["weights"], r["before"], r["after"]):
        print(f"LM weight {w:2d}: WER unigram {100.0 * eb / nref:6.2f}% ({eb} / {nref})   bigram-rescored {100.0 * ea / nref:6.2f}% ({ea} / {nref})")
    bb, ba = min(e for e, _ in r["before"]), min(e for e, _ in r["after"])
    print(f"best over the sweep: unigram {100.0 * bb / nref:.2f}%, bigram-rescored {100.0 * ba / nref:.2f}%; "
          f"host and device hypotheses {'identical' if r['host_agrees'] else 'DIFFERENT' if r['host_agrees'] is not None else 'not compared'}")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=200)
    ap.add_argument("--test-utts", type=int, default=100)
    ap.add_argument("--iters", type=int, default=80)
    ap.add_argument("--dim", type=int, default=23)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--p-switch", type=float, default=0.85)
    ap.add_argument("--mix", type=float, default=0.0)
    ap.add_argument("--diff-dims", type=int, default=4)
    args = ap.parse_args(argv)
    train_utts, test_utts = make_data(args.utts, args.test_utts, args.dim, np.random.default_rng(args.seed), args.p_switch, args.mix, args.diff_dims)
    tm, tree, am, lexicon = train(args, train_utts)
    r = evaluate(tm, tree, am, lexicon, train_utts, test_utts)
    report(r)
    k, nref = r["weights"].index(10), r["before"][0][1]
    print(f"RESULT wer_unigram={r['before'][k][0] / nref:.4f} wer_rescored={r['after'][k][0] / nref:.4f} "
          f"best_unigram={min(e for e, _ in r['before']) / nref:.4f} best_rescored={min(e for e, _ in r['after']) / nref:.4f} "
          f"host_agrees={int(bool(r['host_agrees']))}")
    return 0 if r["host_agrees"] and r["failed"] == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
