#!/usr/bin/env python3
"""Wall-clock time of a batched lattice decode (decode_lattice_faster_batch: K1 over every cell of the graphs' pdfs + the lattice
decoder kernel + transfers) beside the FasterDecoder batch (align_batch at FasterDecoderOptions(beam=13, max_active=7000)) on the
bench workload's model (tri5000x64: 5000 pdfs x 64 Gaussians, dim 40) and its linear training graphs, at decode.py's configuration
(max_active 7000, beam 13, lattice_beam 6, acoustic scale 0.1).  Prints one JSON line.

--decoder simple times decode_lattice_simple_batch (LatticeSimpleDecoderConfig(beam=13, lattice_beam=6)) instead, beside the faster
lattice decoder and the FasterDecoder batch on the same graphs.  All three then decode the graphs with a zero-weight input-epsilon
self-loop added on every state: no path's weight changes, and the simple decoder's ProcessNonemitting always has a token to queue
(the training graphs alone are epsilon-free, on which the reference stops at InitDecoding).

--check N (with --decoder simple) also decodes the first N utterances with their K1 scores returned and compares them, outside the
timing, with the plain-Python restatement of the reference (tests/lattice_simple_ref.py): succeeded, alignment, words, like.

Usage: python tools/decode_lattice_bench.py [--utts 100000] [--reps 2] [--decoder faster|simple] [--check N]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kaldi_hmm_gmm_amd as khg  # noqa: E402
from kaldi_hmm_gmm_amd import synth  # noqa: E402


def with_eps_self_loops(graphs, u):
    """Utterance u of a CSR graph set with a 0:0/0 self-loop after the arcs of every state."""
    so = graphs["state_off"]
    s0, s1 = int(so[u]), int(so[u + 1])
    ao = graphs["arc_off"]
    il, ol, w, ns, off = [], [], [], [], [0]
    for s in range(s0, s1):
        a0, a1 = int(ao[s]), int(ao[s + 1])
        il += list(graphs["ilabel"][a0:a1]) + [0]
        ol += list(graphs["olabel"][a0:a1]) + [0]
        w += list(graphs["weight"][a0:a1]) + [0.0]
        ns += list(graphs["nextstate"][a0:a1]) + [s - s0]
        off.append(len(il))
    return khg.StdVectorFst.from_csr(int(graphs["start"][u]), np.asarray(off, np.int64), np.asarray(il, np.int32), np.asarray(ol, np.int32),
                                     np.asarray(w, np.float32), np.asarray(ns, np.int32), np.asarray(graphs["final"][s0:s1], np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--decoder", choices=("faster", "simple"), default="faster")
    ap.add_argument("--check", type=int, default=0)
    args = ap.parse_args()
    m = synth.make_model(5000, 64, 40, seed=args.seed)
    am, tm = synth.host_objects(m)
    ut = synth.make_utts(m, args.utts, seed=args.seed + 1000)
    if args.decoder == "simple":
        fsts = [with_eps_self_loops(ut.graphs, u) for u in range(args.utts)]
    else:
        fsts = [synth.utt_fst(ut.graphs, u) for u in range(args.utts)]
    feats = [ut.feats[ut.frame_off[u]: ut.frame_off[u + 1]] for u in range(args.utts)]
    frames = int(ut.frame_off[-1])
    cfg = khg.LatticeFasterDecoderConfig(max_active=7000, beam=13.0, lattice_beam=6.0)
    lat_s, ali_s, res = [], [], None
    if args.decoder == "simple":
        scfg = khg.LatticeSimpleDecoderConfig(beam=13.0, lattice_beam=6.0)
        simple_s = []
        khg.decode_lattice_simple_batch(am, tm, fsts[:64], feats[:64], scfg, 0.1)          # warm-up
        for _ in range(args.reps):
            t0 = time.time()
            res = khg.decode_lattice_simple_batch(am, tm, fsts, feats, scfg, 0.1)
            simple_s.append(time.time() - t0)
    for _ in range(args.reps):
        t0 = time.time()
        fres = khg.decode_lattice_faster_batch(am, tm, fsts, feats, cfg, 0.1)
        lat_s.append(time.time() - t0)
        t0 = time.time()
        khg.align_batch(am, tm, fsts, feats, khg.AlignConfig(beam=13.0), 0.1,
                        decoder_opts=khg.FasterDecoderOptions(beam=13.0, max_active=7000))
        ali_s.append(time.time() - t0)
    if res is None:
        res = fres
    st = [r["status"] for r in res]
    out = {"decoder": args.decoder,"utterances": args.utts, "frames": frames, "lattice_s": min(lat_s), "lattice_frames_per_s": frames / min(lat_s),
           "faster_decoder_s": min(ali_s), "ratio": min(lat_s) / min(ali_s),
           "succeeded": sum(1 for s in st if s & 1), "partial": sum(1 for s in st if s & 2), "scratch": sum(1 for s in st if s & 4)}
    if args.decoder == "simple":
        out.update(simple_s=min(simple_s), simple_frames_per_s=frames / min(simple_s), simple_over_lattice_faster=min(simple_s) / min(lat_s),
                   simple_over_faster_decoder=min(simple_s) / min(ali_s),
                   same_best_paths_as_lattice_faster=sum(1 for a, b in zip(res, fres) if a["alignment"] == b["alignment"]))
        if args.check > 0:
            sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
            import lattice_simple_ref as ref
            n = min(args.check, args.utts)
            chk = khg.decode_lattice_simple_batch(am, tm, fsts[:n], feats[:n], scfg, 0.1, return_scores=True)
            match = 0
            for u, r in enumerate(chk):
                g = fsts[u].to_csr()
                want = ref.decode_utterance_lattice_simple(ref.Graph.from_dict(g), ref.Config(beam=13.0, lattice_beam=6.0),
                                                           ref.score_fn(r["loglikes"], r["pdfs"], m.id2pdf, 0.1), len(feats[u]))
                match += (r["succeeded"], r["alignment"], r["words"], r["like"]) == (want["succeeded"], want["alignment"], want["words"],
                                                                                      want["like"]) and (res[u]["alignment"] == r["alignment"])
            out.update(checked_against_restatement=n, restatement_matches=match)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
