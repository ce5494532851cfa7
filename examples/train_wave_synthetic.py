#!/usr/bin/env python3
"""From waveforms to words on the synthetic YES/NO task, with only the samples going up to the device:

  1. synth.make_yesno_waves: int16 waveforms, every phone state its own pair of tones over noise, per-utterance gain and pitch;
  2. compute-mfcc-feats on the device (khg.compute_mfcc_feats_batch): 13 cepstra per 10 ms;
  3. the tensor is borrowed by an UtteranceSet; compute-cmvn-stats per utterance and apply-cmvn | add-deltas in one kernel (7p);
  4. flat start and ML training of the monophone model (train_mono_synthetic.py's schedule);
  5. decoding of held-out utterances.

Prints the WER and the per-frame training likelihood; exits 0 when the held-out WER is at most --max-wer.

Usage: python examples/train_wave_synthetic.py [--utts 150] [--test-utts 30] [--iters 80] [--max-wer 0.2]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kaldi_hmm_gmm_amd as khg  # noqa: E402
import decode_synthetic as dx  # noqa: E402
import train_cmvn_deltas_synthetic as cd  # noqa: E402
from kaldi_hmm_gmm_amd import _gpu, synth  # noqa: E402


def device_features(waves, opts):
    """wave -> mfcc -> per-utterance CMVN + deltas, all on the device; the 39-dimensional rows come down once, for the host recipe"""
    ctx = _gpu.default_context()
    fo, mfcc = khg.compute_mfcc_feats_batch(ctx, waves, opts)
    us = khg.UtteranceSet(ctx, None, fo, (mfcc.data_ptr(), mfcc), dim=mfcc.shape[1])
    stats = khg.compute_cmvn_stats_batch(us)
    r = khg.cmvn_compute(stats, norm_vars=True)
    assert (r["status"] == khg.CMVN_OK).all(), r["status"]
    t = khg.add_deltas_batch(us, cd.ORDER, cd.WINDOW, norm=r["norm"], status=r["status"])
    rows = t.cpu().numpy()
    stats.close()
    us.close()
    return [np.ascontiguousarray(rows[fo[i]:fo[i + 1]]) for i in range(len(waves))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=150)
    ap.add_argument("--test-utts", type=int, default=30)
    ap.add_argument("--iters", type=int, default=80)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--max-wer", type=float, default=0.2)
    args = ap.parse_args()
    opts = khg.FrontendOptions()
    utts = synth.make_yesno_waves(args.utts + args.test_utts, seed=args.seed, samp_freq=opts.samp_freq)
    feats = device_features([u[2] for u in utts], opts)
    one = khg.compute_mfcc_feats(utts[0][2], opts)                 # the host form of the first utterance: the same frames
    assert one.shape == (len(feats[0]), 13), (one.shape, feats[0].shape)
    train_utts, test_utts = utts[: args.utts], utts[args.utts:]
    tm, tree, am, lexicon, like = cd.train(args, train_utts, feats[: args.utts])
    errs, nref, _, _ = dx.decode(tm, tree, am, lexicon, [(n, w, f) for (n, w, _), f in zip(test_utts, feats[args.utts:])], log=lambda *a: None)
    wer = errs / max(nref, 1)
    secs = sum(len(u[2]) for u in utts) / opts.samp_freq
    print(f"{len(utts)} waveforms, {secs:.1f} s of audio -> {sum(len(f) for f in feats)} frames of dim {feats[0].shape[1]}; {am.num_gauss} Gaussians, "
          f"per-frame likelihood {like:.4f}; held-out WER {100.0 * wer:.2f}% ({errs} / {nref})")
    print(f"RESULT wer={wer:.6f} like={like:.6f}")
    return 0 if wer <= args.max_wer else 1


if __name__ == "__main__":
    sys.exit(main())
