#!/usr/bin/env python3
"""The first two stages of a Kaldi GMM recipe on the synthetic YES/NO task -- `apply-cmvn | add-deltas` in front of the monophone model,
on this project's device path:

  1. low-dimensional static features; every synthetic speaker's rows get that speaker's own offset and per-dimension gain;
  2. the model's features are made on the device from the resident static rows, twice:
       raw:   add-deltas                                  (UtteranceSet.add_deltas)
       cmvn:  compute-cmvn-stats per speaker -> the normaliser -> apply-cmvn | add-deltas in one kernel
     (the fused call is checked against apply-cmvn in place followed by add-deltas, on the bits);
  3. ML training of the monophone model on each, in the same schedule (train_mono_synthetic.py's);
  4. decoding of held-out utterances of held-out speakers both ways (their statistics come from their own utterances).

Prints the WER and the per-frame training likelihood of both; exits 0 when the normalised features decode no worse.

Usage: python examples/train_cmvn_deltas_synthetic.py [--utts 200] [--test-utts 30] [--speakers 5] [--iters 80] [--strength 1.0]
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
from kaldi_hmm_gmm_amd.training_graph import TrainingGraphCompiler, equal_align, generate_hmm_topo  # noqa: E402

ORDER, WINDOW = 2, 2


def speaker_channels(n_spk, dim, rng, strength):
    """one fixed channel per synthetic speaker: x -> gain * x + offset, per dimension"""
    return [(np.exp(0.3 * strength * rng.standard_normal(dim)), 3.0 * strength * rng.standard_normal(dim)) for _ in range(n_spk)]


def distort(utts, utt2spk, channels):
    return [(n, w, np.ascontiguousarray(x.astype(np.float64) * channels[s][0] + channels[s][1], np.float32)) for (n, w, x), s in zip(utts, utt2spk)]


def device_features(static, utt2spk, n_spk, cmvn):
    """the model's features from the static rows, on the device: add-deltas, with per-speaker CMVN fused in when `cmvn`"""
    ctx = _gpu.default_context()
    fo = np.concatenate([[0], np.cumsum([len(f) for f in static])]).astype(np.int64)
    us = khg.UtteranceSet(ctx, None, fo, np.ascontiguousarray(np.concatenate(static), np.float32))
    if cmvn:
        stats = khg.compute_cmvn_stats_batch(us, utt2spk, n_spk)
        r = khg.cmvn_compute(stats, norm_vars=True)
        assert (r["status"] == khg.CMVN_OK).all(), r["status"]
        t = khg.add_deltas_batch(us, ORDER, WINDOW, norm=r["norm"], utt2spk=utt2spk, status=r["status"])
        khg.apply_cmvn_batch(us, r["norm"], utt2spk, r["status"])          # the same in two calls: in place, then the deltas
        assert bool((khg.add_deltas_batch(us, ORDER, WINDOW) == t).all()), "fused and unfused differ"
        stats.close()
    else:
        t = khg.add_deltas_batch(us, ORDER, WINDOW)
    rows = t.cpu().numpy()
    us.close()
    return [np.ascontiguousarray(rows[fo[i]:fo[i + 1]]) for i in range(len(static))]


def train(args, utts, feats):
    """flat start and train_mono_synthetic.py's schedule on `feats` -> (tm, tree, am, lexicon, per-frame likelihood of the final alignment)"""
    names = [u[0] for u in utts]
    with_feats = [(n, w, f) for (n, w, _), f in zip(utts, feats)]
    topo = generate_hmm_topo(non_sil_phones=[tr.Y, tr.N], sil_phone=tr.SIL)
    tm, tree, am = khg.gmm_init_mono(topo, np.concatenate(feats[:10]))
    lexicon = {tr.YES: [(1.0, [tr.Y])], tr.NO: [(1.0, [tr.N])]}
    gcomp = TrainingGraphCompiler(tm, tree, lexicon, sil_phone=tr.SIL, sil_prob=0.5)
    graphs = gcomp.compile_graphs_from_text([u[1] for u in utts])
    ali = [equal_align(g, x.shape[0], rand_seed=3, num_retries=10)[1] for g, x in zip(graphs, feats)]
    targs = types.SimpleNamespace(iters=args.iters, out="", seed=args.seed)
    tr.train_resident(targs, with_feats, names, feats, tm, tree, am, graphs, ali, log=lambda *a: None)
    cfg = khg.AlignConfig(beam=6.0, retry_beam=40.0, careful=False)
    r = khg.gmm_align_compiled_batch(am, tm, names, graphs, feats, cfg, acoustic_scale=0.1, transition_scale=1.0, self_loop_scale=0.1)
    return tm, tree, am, lexicon, r["tot_like"] / max(r["frame_count"], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=200)
    ap.add_argument("--test-utts", type=int, default=30)
    ap.add_argument("--speakers", type=int, default=5, help="training speakers; the test utterances belong to 3 further ones")
    ap.add_argument("--iters", type=int, default=80)
    ap.add_argument("--dim", type=int, default=13)
    ap.add_argument("--strength", type=float, default=1.0, help="scale of the speakers' offsets (3 x) and log-gains (0.3 x)")
    ap.add_argument("--seed", type=int, default=3)
    args = ap.parse_args()
    rng = np.random.default_rng(args.seed)
    n_test_spk = 3
    clean = tr.make_data(args.utts + args.test_utts, args.dim, rng)
    channels = speaker_channels(args.speakers + n_test_spk, args.dim, np.random.default_rng(args.seed + 100), args.strength)
    u2s_all = np.concatenate([np.arange(args.utts) % args.speakers, args.speakers + np.arange(args.test_utts) % n_test_spk]).astype(np.int32)
    utts = distort(clean, u2s_all, channels)
    train_utts, test_utts = utts[: args.utts], utts[args.utts:]
    u2s_train, u2s_test = u2s_all[: args.utts], u2s_all[args.utts:] - args.speakers
    static, tstatic = [u[2] for u in train_utts], [u[2] for u in test_utts]

    result = {}
    for name, cmvn in (("raw", False), ("cmvn", True)):
        feats = device_features(static, u2s_train, args.speakers, cmvn)
        tm, tree, am, lexicon, like = train(args, train_utts, feats)
        tfeats = device_features(tstatic, u2s_test, n_test_spk, cmvn)
        errs, nref, _, _ = dx.decode(tm, tree, am, lexicon, [(n, w, f) for (n, w, _), f in zip(test_utts, tfeats)], log=lambda *a: None)
        result[name] = (errs / max(nref, 1), like)
        what = "apply-cmvn | add-deltas, per-speaker statistics" if cmvn else "add-deltas of the raw rows"
        print(f"{what}: dim {feats[0].shape[1]}, {am.num_gauss} Gaussians, per-frame likelihood {like:.4f}; held-out speakers: "
              f"WER {100.0 * errs / max(nref, 1):.2f}% ({errs} / {nref})")
    print(f"RESULT wer_raw={result['raw'][0]:.6f} wer_cmvn={result['cmvn'][0]:.6f} like_raw={result['raw'][1]:.6f} like_cmvn={result['cmvn'][1]:.6f}")
    return 0 if result["cmvn"][0] <= result["raw"][0] else 1


if __name__ == "__main__":
    sys.exit(main())
