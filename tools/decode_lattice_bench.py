#!/usr/bin/env python3
"""Wall-clock time of a batched lattice decode (decode_lattice_faster_batch: K1 over every cell of the graphs' pdfs + the lattice
decoder kernel + transfers) beside the FasterDecoder batch (align_batch at FasterDecoderOptions(beam=13, max_active=7000)) on the
bench workload's model (tri5000x64: 5000 pdfs x 64 Gaussians, dim 40) and its linear training graphs, at decode.py's configuration
(max_active 7000, beam 13, lattice_beam 6, acoustic scale 0.1).  Prints one JSON line.

Usage: python tools/decode_lattice_bench.py [--utts 100000] [--reps 2]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kaldi_hmm_gmm_amd as khg  # noqa: E402
from kaldi_hmm_gmm_amd import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    m = synth.make_model(5000, 64, 40, seed=args.seed)
    am, tm = synth.host_objects(m)
    ut = synth.make_utts(m, args.utts, seed=args.seed + 1000)
    fsts = [synth.utt_fst(ut.graphs, u) for u in range(args.utts)]
    feats = [ut.feats[ut.frame_off[u]: ut.frame_off[u + 1]] for u in range(args.utts)]
    frames = int(ut.frame_off[-1])
    cfg = khg.LatticeFasterDecoderConfig(max_active=7000, beam=13.0, lattice_beam=6.0)
    lat_s, ali_s, res = [], [], None
    for _ in range(args.reps):
        t0 = time.time()
        res = khg.decode_lattice_faster_batch(am, tm, fsts, feats, cfg, 0.1)
        lat_s.append(time.time() - t0)
        t0 = time.time()
        khg.align_batch(am, tm, fsts, feats, khg.AlignConfig(beam=13.0), 0.1,
                        decoder_opts=khg.FasterDecoderOptions(beam=13.0, max_active=7000))
        ali_s.append(time.time() - t0)
    st = [r["status"] for r in res]
    out = {"utterances": args.utts, "frames": frames, "lattice_s": min(lat_s), "lattice_frames_per_s": frames / min(lat_s),
           "faster_decoder_s": min(ali_s), "ratio": min(lat_s) / min(ali_s),
           "succeeded": sum(1 for s in st if s & 1), "partial": sum(1 for s in st if s & 2), "scratch": sum(1 for s in st if s & 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
