#!/usr/bin/env python3
"""Decoding with the trained monophone model through the reference's lattice decoder calls -- egs/yesno/decode.py:143-179:

    config  = LatticeFasterDecoderConfig(max_active=7000, beam=13.0, lattice_beam=6.0)
    decoder = LatticeFasterDecoder(HCLG, config)
    ok, ali, words, like = decode_utterance_lattice_faster(decoder=decoder, decodable=decodable, trans_model=tm, utt=..., allow_partial=True)

on the synthetic YES/NO task of decode_synthetic.py: the same training (train_mono_synthetic.py's flat start, 80 passes), the same
unigram word-loop graph, then every held-out utterance through those three calls (K1 scores the frames, the lattice decoder kernel
searches and returns the raw lattice's best path), the batched decode_lattice_faster_batch beside them, and the WER.

--decoder simple runs the same through LatticeSimpleDecoderConfig(beam=13, lattice_beam=6) / LatticeSimpleDecoder /
decode_utterance_lattice_simple and decode_lattice_simple_batch.  The word loop is epsilon-free, on which the reference's
LatticeSimpleDecoder stops at InitDecoding ("no surviving tokens"), so that decoder gets a copy of it with a zero-weight
input-epsilon self-loop on every state: no path's weight changes.

--sweep 7:17 also keeps the batch's raw lattices on the device (get_raw_lattice_faster_device_batch: the word loop as compiled,
nothing added; with --decoder simple get_raw_lattice_simple_device_batch on the copy with self-loops) and prints the WER at every
integer language-model weight w in 7..17 (graph_scale 1, acoustic_scale 1 / w; the lattices hold costs at acoustic scale 0.1, i.e.
weight 10 is acoustic_scale 1.0 here) from that ONE decode: one DeviceLattices.best_path call, no lattice leaves the device.

Usage: python examples/decode_lattice_synthetic.py [--utts 200] [--iters 80] [--decoder faster|simple] [--sweep 7:17]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_synthetic as dx  # noqa: E402
import kaldi_hmm_gmm_amd as khg  # noqa: E402
from kaldi_hmm_gmm_amd.training_graph import TrainingGraphCompiler, TrainingGraphCompilerOptions  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=200)
    ap.add_argument("--test-utts", type=int, default=30)
    ap.add_argument("--iters", type=int, default=80)
    ap.add_argument("--dim", type=int, default=23)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--decoder", choices=("faster", "simple"), default="faster")
    ap.add_argument("--sweep", default=None, metavar="LO:HI", help="WER at every integer LM weight, from one decode")
    args = ap.parse_args()
    tm, tree, am, lexicon, test_utts = dx.train(args)
    # decode.py:112,135: transition_scale 1.0, self_loop_scale 1.0 go into the graph
    gc = TrainingGraphCompiler(tm, tree, lexicon, sil_phone=dx.tr.SIL, sil_prob=0.5,
                               opts=TrainingGraphCompilerOptions(transition_scale=1.0, self_loop_scale=1.0))
    graph = gc.compile_word_loop_graph()
    if args.decoder == "simple":
        graph = graph.copy()
        for s in range(graph.num_states):
            graph.add_arc(s, khg.StdArc(0, 0, 0.0, s))
        config = khg.LatticeSimpleDecoderConfig(beam=13.0, lattice_beam=6.0)
        decoder = khg.LatticeSimpleDecoder(graph, config)
        decode_one, decode_batch = khg.decode_utterance_lattice_simple, khg.decode_lattice_simple_batch
    else:
        config = khg.LatticeFasterDecoderConfig(max_active=7000, beam=13.0, lattice_beam=6.0)
        decoder = khg.LatticeFasterDecoder(graph, config)
        decode_one, decode_batch = khg.decode_utterance_lattice_faster, khg.decode_lattice_faster_batch
    errs = nref = failed = 0
    t0 = time.time()
    hyps = []
    for utt, ref_words, feats in test_utts:
        decodable = khg.DecodableAmDiagGmmScaled(am, tm, feats, 0.1)
        ok, ali, words, like = decode_one(decoder=decoder, decodable=decodable, trans_model=tm, utt=str(utt), allow_partial=True)
        failed += not ok
        hyps.append((ok, ali, words, like))
        errs += dx.edit_distance(ref_words, words if ok else [])
        nref += len(ref_words)
    t1 = time.time()
    batch = decode_batch(am, tm, graph, [u[2] for u in test_utts], config, 0.1, allow_partial=True)
    same = all((h[0], h[1], h[2], h[3]) == (b["succeeded"], b["alignment"], b["words"], b["like"]) for h, b in zip(hyps, batch))
    print(f"decoded {len(test_utts)} utterances on a {graph.num_states}-state word-loop graph with {config}: "
          f"WER {100.0 * errs / max(nref, 1):.2f}% ({errs} / {nref}), {failed} failed, {t1 - t0:.2f} s through the per-utterance calls; "
          f"batched decode {'identical' if same else 'DIFFERENT'}")
    print(f"{test_utts[0][0]}: words {hyps[0][2]} (truth {test_utts[0][1]}), like {hyps[0][3]:.4f}")
    if args.sweep:
        import numpy as np
        lo, hi = (int(x) for x in args.sweep.split(":"))
        ws = np.arange(lo, hi + 1)
        # the lattices were decoded at acoustic scale 0.1 = LM weight 10: weight w re-weights their acoustic costs by 10 / w
        raw_device_batch = khg.get_raw_lattice_simple_device_batch if args.decoder == "simple" else khg.get_raw_lattice_faster_device_batch
        _, lats = raw_device_batch(am, tm, graph, [u[2] for u in test_utts], config, 0.1)
        bp = lats.best_path(np.ones(len(ws), np.float32), (10.0 / ws).astype(np.float32))
        U = len(test_utts)
        for k, w in enumerate(ws):
            e = n = 0
            for u, (_, ref_words, _) in enumerate(test_utts):
                o = k * U + u
                hyp = bp["words"][bp["words_off"][o]: bp["words_off"][o + 1]].tolist() if bp["status"][o] & 1 else []
                e += dx.edit_distance(ref_words, hyp)
                n += len(ref_words)
            print(f"LM weight {w:2d}: WER {100.0 * e / max(n, 1):.2f}% ({e} / {n})")
        lats.close()
    return 0 if errs <= 0.05 * nref and same and (failed == 0 or args.decoder == "faster") else 1


if __name__ == "__main__":
    sys.exit(main())
