#!/usr/bin/env python3
"""From a monophone to a context-dependent (triphone) system on a synthetic task -- the mono -> tri1 step of a Kaldi recipe on this
project's device path:

  1. a small task whose phone realisations depend on the class of the phone to the LEFT: every state mean is shifted by a vector that
     depends on whether the left neighbour is in {A, C}; a monophone model has to spend its Gaussians on the two variants;
  2. ML training of the monophone model (train_mono_synthetic.py's schedule, resident on the device);
  3. acc-tree-stats on the device from the monophone alignment (silence context-independent), build-tree on the host, gmm-init-model,
     convert-ali;
  4. training graphs on the new tree, ML training with mixing up from the converted alignment;
  5. decoding of held-out utterances on word-loop graphs of both systems.

Prints the leaves, the per-frame likelihood of the training alignments and the WER for mono against tri; exits 0 when every
transcript compiled and aligned on the triphone graphs and the tree has more leaves than the monophone system.

Usage: python examples/train_tri_synthetic.py [--utts 120] [--test-utts 30] [--iters 30] [--max-leaves 40] [--thresh 100] [--cluster-thresh -1]
"""
import argparse
import os
import pickle
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

SIL, A, B, C, D = 1, 2, 3, 4, 5
LEXICON = {1: [(1.0, [A, B])], 2: [(1.0, [B, A])], 3: [(1.0, [C, D, A])], 4: [(1.0, [D, C])]}
QUESTIONS = [[A, C], [B, D], [A], [B], [C], [D], [0, SIL]]


def make_data(n_utt, dim, rng, shift=2.0):
    """3..6 random words, silence around them with probability 0.3; a phone state emits 3..6 frames from its own Gaussian, whose mean
    moves by the phone's shift vector when the phone to the left is A or C"""
    nstate = {SIL: 5, A: 3, B: 3, C: 3, D: 3}
    base, k = {}, 0
    for ph in (SIL, A, B, C, D):
        base[ph] = k
        k += nstate[ph]
    means = (rng.standard_normal((k, dim)) * 2.5).astype(np.float32)
    shifts = {ph: (shift * rng.standard_normal(dim)).astype(np.float32) for ph in (A, B, C, D)}
    utts = []
    for u in range(n_utt):
        words = [int(w) for w in rng.integers(1, 5, size=int(rng.integers(3, 7)))]
        phones = [SIL] if rng.random() < 0.3 else []
        for w in words:
            phones.extend(LEXICON[w][0][1])
            if rng.random() < 0.3:
                phones.append(SIL)
        x = []
        for i, ph in enumerate(phones):
            left = phones[i - 1] if i > 0 else 0
            off = shifts[ph] if (ph != SIL and left in (A, C)) else 0.0
            for s in range(nstate[ph]):
                n = int(rng.integers(3, 7))
                x.append(means[base[ph] + s] + off + rng.standard_normal((n, dim)).astype(np.float32))
        utts.append((f"utt{u:04d}", words, np.concatenate(x).astype(np.float32)))
    return utts


def align(am, tm, names, graphs, feats):
    cfg = khg.AlignConfig(beam=6.0, retry_beam=40.0, careful=False)
    return khg.gmm_align_compiled_batch(am, tm, names, graphs, feats, cfg, acoustic_scale=0.1, transition_scale=1.0, self_loop_scale=0.1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=120)
    ap.add_argument("--test-utts", type=int, default=30)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--dim", type=int, default=13)
    ap.add_argument("--max-leaves", type=int, default=40)
    ap.add_argument("--thresh", type=float, default=100.0)
    ap.add_argument("--cluster-thresh", type=float, default=-1.0)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--out", default="", help="pickle the statistics, the tree and build-tree's figures here")
    args = ap.parse_args()
    rng = np.random.default_rng(args.seed)
    utts = make_data(args.utts + args.test_utts, args.dim, rng)
    train_utts, test_utts = utts[: args.utts], utts[args.utts:]
    names, feats, texts = [u[0] for u in train_utts], [u[2] for u in train_utts], [u[1] for u in train_utts]
    quiet = lambda *a: None  # noqa: E731

    # ---- 2. the monophone system ----
    topo = generate_hmm_topo(non_sil_phones=[A, B, C, D], sil_phone=SIL)
    tm, tree, am = khg.gmm_init_mono(topo, np.concatenate(feats[:10]))
    graphs = TrainingGraphCompiler(tm, tree, LEXICON, sil_phone=SIL, sil_prob=0.5).compile_graphs_from_text(texts)
    ali = [equal_align(g, x.shape[0], rand_seed=3, num_retries=10)[1] for g, x in zip(graphs, feats)]
    targs = types.SimpleNamespace(iters=args.iters, out="", seed=args.seed)
    tr.train_resident(targs, train_utts, names, feats, tm, tree, am, graphs, ali, log=quiet)
    r0 = align(am, tm, names, graphs, feats)
    like_mono = r0["tot_like"] / max(r0["frame_count"], 1)
    errs0, nref, _, _ = dx.decode(tm, tree, am, LEXICON, test_utts, log=quiet)
    print(f"mono: {tree.num_pdfs} pdfs, {am.num_gauss} Gaussians, per-frame likelihood {like_mono:.4f}, WER {100.0 * errs0 / max(nref, 1):.2f}%")

    # ---- 3. acc-tree-stats on the device, build-tree, gmm-init-model, convert-ali ----
    ctx = _gpu.default_context()
    keep = [i for i, a in enumerate(r0["alignment"]) if a]
    fo = np.concatenate([[0], np.cumsum([len(feats[i]) for i in keep])]).astype(np.int64)
    us = khg.UtteranceSet(ctx, None, fo, np.ascontiguousarray(np.concatenate([feats[i] for i in keep]), np.float32))
    us.upload_ali(np.concatenate([np.asarray(r0["alignment"][i], np.int32) for i in keep]))
    st = khg.acc_tree_stats(tm, us, N=3, P=1, ci_phones=[SIL])
    assert not np.asarray(st["status"]).any(), "an alignment of the monophone system does not split into phones"
    st.pop("stats").close()
    us.close()
    p2n = topo.get_phone_to_num_pdf_classes()
    sets = [[p] for p in (SIL, A, B, C, D)]
    tri_tree, info = khg.build_tree(st, QUESTIONS, sets, p2n, [True] * 5, [False, True, True, True, True], thresh=args.thresh,
                                    max_leaves=args.max_leaves, cluster_thresh=args.cluster_thresh, return_info=True)
    print(f"acc-tree-stats: {len(st['keys'])} events over {int(st['count'].sum())} frames; build-tree: {info['num_leaves']} leaves, "
          f"objf_impr {info['objf_impr']:.2f} ({info['objf_impr'] / st['count'].sum():.4f} per frame), {info['num_removed']} leaves merged")
    tri_am, tri_tm = khg.gmm_init_model(tri_tree, st, topo)
    tri_ali = [list(khg.convert_ali(tm, tri_tm, tri_tree, r0["alignment"][i])) if r0["alignment"][i] else [] for i in range(len(feats))]
    if args.out:
        with open(args.out, "wb") as fh:
            pickle.dump({"stats": {k: np.asarray(st[k]) for k in ("keys", "count", "x", "x2")}, "tree": tri_tree, "info": info}, fh)

    # ---- 4. triphone graphs and training ----
    failed_compile = 0
    tri_graphs = []
    gcomp = TrainingGraphCompiler(tri_tm, tri_tree, LEXICON, sil_phone=SIL, sil_prob=0.5)
    for t in texts:
        try:
            tri_graphs.append(gcomp.compile_graph_from_text(t))
        except khg.KhgError:
            failed_compile += 1
            tri_graphs.append(None)
    if failed_compile:
        print(f"RESULT failed_compile={failed_compile}")
        return 1
    tri_ali = [a if a else equal_align(g, x.shape[0], rand_seed=3, num_retries=10)[1] for a, g, x in zip(tri_ali, tri_graphs, feats)]
    rc = tr.train_resident(targs, train_utts, names, feats, tri_tm, tri_tree, tri_am, tri_graphs, tri_ali, log=quiet)
    r1 = align(tri_am, tri_tm, names, tri_graphs, feats)
    like_tri = r1["tot_like"] / max(r1["frame_count"], 1)

    # ---- 5. decoding ----
    errs1, _, graph, _ = dx.decode(tri_tm, tri_tree, tri_am, LEXICON, test_utts, log=quiet)
    print(f"tri:  {tri_tree.num_pdfs} pdfs, {tri_am.num_gauss} Gaussians, per-frame likelihood {like_tri:.4f}, WER {100.0 * errs1 / max(nref, 1):.2f}% "
          f"on a {graph.num_states}-state word-loop graph")
    print(f"RESULT failed_compile=0 failed_align={r1['num_error']} mono_pdfs={tree.num_pdfs} tri_pdfs={tri_tree.num_pdfs} max_leaves={args.max_leaves} "
          f"objf_impr={info['objf_impr']!r} like_mono={like_mono:.6f} like_tri={like_tri:.6f} wer_mono={errs0 / max(nref, 1):.6f} wer_tri={errs1 / max(nref, 1):.6f} "
          f"transcripts_ok={1 if rc == 0 else 0}")
    return 0 if (r1["num_error"] == 0 and tri_tree.num_pdfs > tree.num_pdfs) else 1


if __name__ == "__main__":
    sys.exit(main())
