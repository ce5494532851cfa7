#!/usr/bin/env python3
"""Determinizing the lattices a decode left on the device.

The task is the YES/NO task of score_lattices_synthetic.py: a monophone model trained on the training half, ONE lattice-faster decode
of the held-out half on the shared word-loop graph, and then, on the raw lattices the decode left in HBM,

    det, status, stats = lats.determinize(1.0, 1.0, lattice_beam)      lattice-determinize-pruned: one path per word sequence,
                                                                       the cheapest, made of copies of the raw lattice's arcs

which is what get_lattice_faster_device_batch returns for a configuration with determinize_lattice=True.  Printed: states and arcs
before and after, what a bigram lm_rescore makes of both (the history split works on one path per sequence instead of one per
alignment), and the MBR hypotheses of both.  Every lattice is also determinized on the host (Lattice.determinize) and compared: the
two must be identical, and the best path of a determinized lattice must be the raw lattice's, words and weight.

Usage: python examples/determinize_synthetic.py [--utts 200] [--test-utts 100] [--iters 80] [--lattice-beam 8] [--lmwt 10] [--state-factor 8]
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
FIELDS = ("frame", "graph_state", "tot_cost", "extra_cost", "final_cost", "arc_begin", "ilabel", "olabel", "graph_cost", "acoustic_cost", "nextstate")


def _same(a, b):
    return a.start == b.start and all(np.asarray(getattr(a, f)).tobytes() == np.asarray(getattr(b, f)).tobytes() for f in FIELDS)


def evaluate(tm, tree, am, lexicon, train_utts, test_utts, lattice_beam, lmwt, state_factor=8):
    transcripts = [u[1] for u in train_utts]
    counts = np.bincount(np.concatenate(transcripts), minlength=3)[1:3].astype(np.float64)
    word_probs = {tr.YES: float(counts[0] / counts.sum()), tr.NO: float(counts[1] / counts.sum())}
    gc = TrainingGraphCompiler(tm, tree, lexicon, sil_phone=tr.SIL, sil_prob=0.5,
                               opts=TrainingGraphCompilerOptions(transition_scale=1.0, self_loop_scale=1.0))
    graph = gc.compile_word_loop_graph(word_probs)
    config = khg.LatticeFasterDecoderConfig(max_active=7000, beam=13.0, lattice_beam=lattice_beam, determinize_lattice=False)
    feats, refs = [u[2] for u in test_utts], [[int(w) for w in u[1]] for u in test_utts]
    U = len(feats)
    _, raw = khg.get_raw_lattice_faster_device_batch(am, tm, graph, feats, config, ACOUSTIC_SCALE)
    det, status, stats = raw.determinize(1.0, 1.0, lattice_beam, config.det_opts.delta, state_factor)
    # GetLattice: the same through the configuration
    config.determinize_lattice = True
    _, det2 = khg.get_lattice_faster_device_batch(am, tm, graph, feats, config, ACOUSTIC_SCALE, state_factor=state_factor)
    agree = True
    host_raw, got, got2 = raw.download(), det.download(), det2.download()
    for u, L in enumerate(host_raw):
        H, hst, _ = L.determinize(1.0, 1.0, lattice_beam, config.det_opts.delta, state_factor)
        agree = agree and hst == int(status[u]) and _same(H, got[u]) and _same(got2[u], got[u])
        if hst & 1:
            a, b = H.best_path(1.0, 1.0), L.best_path(1.0, 1.0)
            agree = agree and a["words"] == b["words"] and a["weight"] == b["weight"]
    # what follows in a recipe, on both
    bigram = khg.estimate_ngram_lm(transcripts, 2, [tr.YES, tr.NO], 0.5)
    dlm = khg.DeviceLm(bigram)
    gs, as_ = 1.0, 1.0 / (lmwt * ACOUSTIC_SCALE)
    r = {"utts": U, "ref_words": sum(len(x) for x in refs), "stats": stats, "failed": int(sum(1 for s in status if not s & 1)),
         "scratch": int(sum(1 for s in status if s & 4)),
         "host_agrees": bool(agree)}
    for name, lats in (("raw", raw), ("det", det)):
        res, _, lst = lats.lm_rescore(dlm, 1.0)
        bp = res.best_path(np.array([gs], np.float32), np.array([as_], np.float32))
        hyp = [bp["words"][bp["words_off"][u]: bp["words_off"][u + 1]].tolist() if bp["status"][u] & 1 else [] for u in range(U)]
        mbr = [o["words"].tolist() for o in khg.lattice_mbr_decode_batch(lats, gs, as_)]
        r[name] = {"states": int(lats.state_off[-1]), "arcs": int(lats.arc_off[-1]), "lm_states": int(lst["out_states"]), "lm_max_hist": int(lst["max_hist"]),
                   "lm_wer": khg.compute_wer(refs, hyp)[0], "mbr_wer": khg.compute_wer(refs, mbr)[0], "lm_hyp": hyp}
        res.close()
    r["lm_same_words"] = sum(a == b for a, b in zip(r["raw"]["lm_hyp"], r["det"]["lm_hyp"]))
    for h in (raw, det, det2, dlm):
        h.close()
    return r


def report(r, lattice_beam, lmwt):
    s = r["stats"]
    print(f"{r['utts']} held-out utterances, {r['ref_words']} reference words; lattice beam {lattice_beam}, LMWT {lmwt}")
    print(f"raw lattices: {r['raw']['states']} states, {r['raw']['arcs']} arcs; pruned: {s['pruned_states']} states; determinized states: {s['det_states']} "
          f"(largest subset {s['max_subset']}, largest closure {s['max_closure']})")
    print(f"determinized: {r['det']['states']} states, {r['det']['arcs']} arcs ({r['det']['states'] / max(r['raw']['states'], 1):.2f} of the raw states; "
          f"{r['failed']} lattices without a result, {r['scratch']} of them for scratch: a larger --state-factor takes them)")
    for name in ("raw", "det"):
        x = r[name]
        print(f"  {name}: bigram lm_rescore -> {x['lm_states']} states (largest history set {x['lm_max_hist']}), WER {x['lm_wer']:.2f}%; MBR WER {x['mbr_wer']:.2f}%")
    print(f"rescored best paths with the same words on both: {r['lm_same_words']} of {r['utts']}; host and device {'identical' if r['host_agrees'] else 'DIFFERENT'}")


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
    ap.add_argument("--state-factor", type=int, default=8)
    args = ap.parse_args(argv)
    train_utts, test_utts = lmx.make_data(args.utts, args.test_utts, args.dim, np.random.default_rng(args.seed), args.p_switch, 0.0, args.diff_dims)
    tm, tree, am, lexicon = lmx.train(args, train_utts)
    r = evaluate(tm, tree, am, lexicon, train_utts, test_utts, args.lattice_beam, args.lmwt, args.state_factor)
    report(r, args.lattice_beam, args.lmwt)
    print(f"RESULT states_raw={r['raw']['states']} states_det={r['det']['states']} lm_states_raw={r['raw']['lm_states']} lm_states_det={r['det']['lm_states']} "
          f"failed={r['failed']} host_agrees={int(r['host_agrees'])}")
    return 0 if r["host_agrees"] else 1


if __name__ == "__main__":
    sys.exit(main())
