#!/usr/bin/env python3
"""Discriminative (MMI-style) training of the monophone model on the synthetic YES/NO task of decode_lattice_synthetic.py.

The model is trained by maximum likelihood as today (decode_synthetic.train: flat start, 80 passes).  Then, for a few iterations:

  1. align the training utterances on their transcripts' graphs, acc_stats of the alignment            -> the numerator block;
  2. lattice-faster raw lattices on the shared word-loop graph (the HCLG of this task), posteriors of the lattices, acc_stats_post
                                                                                                         -> the denominator block;
  3. I-smoothing of the numerator block with itself: num.smooth_with_accum(tau, num)     (gmm-ismooth-stats);
  4. the Extended Baum-Welch update of means, variances and weights from the two blocks: DeviceModel.ebw_update
                                                                                  (gmm-est-gmm-ebw + gmm-est-weights-ebw).

Features, graphs, lattices, posteriors, both accumulator blocks and the model stay in HBM between the steps; what comes down per
iteration is the alignment's per-utterance likelihoods and the lattices' log Z.  Per iteration the script prints the MMI objective
F = sum_u (kappa like_u - logZ_u) -- like_u the per-frame-unscaled likelihood of the numerator alignment, logZ_u the total
likelihood of utterance u's lattice, both at acoustic scale kappa (the lattices are decoded at kappa, so their costs carry it and
the posteriors are taken at scales (1, 1)) -- and the update's floored / failed counts; at the end the WER on the held-out utterances
before and after.

--rescore: Kaldi's train_mmi.sh does not decode in every iteration.  The denominator lattices are decoded ONCE, before the first
iteration, with the ML model; every iteration then rescores them with the current model (gmm-rescore-lattice:
DeviceLattices.rescore at scale 1, only the (frame, pdf) cells the lattices name are evaluated; the decoding set needs no score
buffer) and takes the posteriors at scales (1, kappa).  The objective F then sums over a FIXED lattice: logZ_u is the total
likelihood of the paths the first decode kept, under the current model, not of a fresh decode.
--boost B: boosted MMI.  The lattices' graph costs are boosted once, right after the decode (lattice-boost-ali:
DeviceLattices.boost, b = B, the numerator alignment of the ML model as the reference, silence errors free); boosting changes graph
costs only, so it commutes with the rescoring.  logZ_u is then the boosted lattice's.

--criterion mpe|smbr (default mmi: everything above, unchanged): MPE / sMBR training (Kaldi's train_mpe.sh).  The lattices are
decoded once with the ML model; every iteration aligns the transcripts (the alignment is the reference and its acc_stats the ML
block), rescores the lattices with the current model, takes the signed posteriors of the expected frame accuracy
(DeviceLattices.mpe_posteriors at scales (1, kappa), ali_set = the aligned set: lattice-to-mpe-post / lattice-to-smbr-post), sends
the positive weights to the numerator block and the negated negative ones to the denominator block (UtteranceSet.acc_stats_post2:
gmm-acc-stats2), I-smooths the numerator block with the ML block (num.smooth_with_accum(tau, ml)) and runs the same EBW update.
Per iteration it prints the criterion: the mean over the utterances of avg_acc / T, the expected fraction of correct frames.

Usage: python examples/train_mmi_synthetic.py [--utts 200] [--mmi-utts 60] [--mmi-iters 4] [--tau 50] [--E 2.0] [--rescore] [--boost B]
                                              [--criterion mmi|mpe|smbr]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_synthetic as dx  # noqa: E402
import kaldi_hmm_gmm_amd as khg  # noqa: E402
from kaldi_hmm_gmm_amd.fst import concat_graphs  # noqa: E402
from kaldi_hmm_gmm_amd.training_graph import TrainingGraphCompiler, TrainingGraphCompilerOptions  # noqa: E402

LEXICON = {dx.tr.YES: [(1.0, [dx.tr.Y])], dx.tr.NO: [(1.0, [dx.tr.N])]}


class MmiState:
    """Everything one MMI run keeps on the device: the model, the utterances on their numerator graphs (us_ali) and on the shared
    decoding graph (us_dec), the two accumulator blocks."""

    def __init__(self, ctx, tm, am, graph, utts, kappa=0.1, tau=50.0, E=2.0, rescore=False, boost=0.0, criterion="mmi"):
        assert criterion in ("mmi", "mpe", "smbr")
        self.ctx, self.kappa, self.tau = ctx, float(kappa), float(tau)
        self.rescore, self.boost, self.lats0 = bool(rescore), float(boost), None
        self.criterion, self.ml = criterion, None
        self.tid2phone = np.asarray(tm.transition_id_to_phone_array(), np.int32)
        self.opts, self.weight_opts = khg.EbwOptions(E=E), khg.EbwWeightOptions()
        self.refs = [u[1] for u in utts]
        feats = [np.ascontiguousarray(u[2], np.float32) for u in utts]
        self.T = np.asarray([f.shape[0] for f in feats], np.int64)
        fo = np.concatenate([[0], np.cumsum(self.T)]).astype(np.int64)
        allf = np.ascontiguousarray(np.concatenate(feats), np.float32)
        go, gc, w, miv, iv = am.flat()
        id2pdf = np.asarray(tm.transition_id_to_pdf_array(), np.int32)
        self.dm = khg.DeviceModel(ctx, go, gc, miv, iv, weights=w)
        # numerator: the transcripts' training graphs, transition probabilities added on the device (train.py: 1.0 / 0.1)
        tree = khg.monophone_context_dependency(tm.topo.phones, tm.topo.get_phone_to_num_pdf_classes())
        comp = TrainingGraphCompiler(tm, tree, LEXICON, sil_phone=dx.tr.SIL, sil_prob=0.5)
        self.dt_ali = khg.DeviceTransitions(ctx, id2pdf)
        self.dt_ali.set_trans_cost(tm.scaled_trans_cost(1.0, 0.1))
        self.us_ali = khg.UtteranceSet(ctx, self.dt_ali, fo, allf, graphs=concat_graphs(comp.compile_graphs_from_text(self.refs)))
        # denominator: ONE decoding graph shared by every utterance; it carries its own transition probabilities
        self.dt_dec = khg.DeviceTransitions(ctx, id2pdf)
        self.dg = khg.DecodingGraph(graph, tm, ctx)
        self.us_dec = khg.UtteranceSet(ctx, self.dt_dec, fo, allf, graph=self.dg)
        self.num = khg.DeviceAccs(ctx, self.dm, self.dt_ali)
        self.den = khg.DeviceAccs(ctx, self.dm, self.dt_dec)
        if criterion != "mmi":
            self.tid2pdf = id2pdf
            self.ml = khg.DeviceAccs(ctx, self.dm, self.dt_ali)
        self.dec = dict(beam=13.0, max_active=7000, lattice_beam=6.0, acoustic_scale=self.kappa)

    def accumulate(self, check=True):
        """Steps 1 and 2 -> dict(F, n_ok, num_frames, den_weight (check=True: the posteriors' total weight, downloaded))."""
        self.num.zero()
        self.den.zero()
        self.us_ali.loglikes(self.dm, reachable_only=True)
        a = self.us_ali.align(self.dt_ali, beam=10.0, retry_beam=40.0, acoustic_scale=self.kappa)
        self.us_ali.acc_stats(self.dm, self.dt_ali, self.num)
        if self.rescore:
            if self.lats0 is None:
                self.lats0 = self.decode_once()
            lats = self.lats0.rescore(self.us_dec, self.dm, self.dt_dec, 1.0)       # unscaled costs: the scale goes into the posteriors
            post = lats.posteriors(1.0, self.kappa)
        else:
            self.us_dec.loglikes(self.dm)
            lats = self.us_dec.raw_lattices_faster_device(self.dt_dec, **self.dec)["lattices"]
            if self.boost:
                lats = self.boosted(lats)
            post = lats.posteriors(1.0, 1.0)
        self.us_dec.acc_stats_post(self.dm, self.dt_dec, post, self.den)
        ok_n = (np.asarray(a["status"]) & khg.ALIGN_ERROR) == 0
        ok_d = (np.asarray(post.status) & 1) != 0
        ok = ok_n & ok_d
        F = float(np.sum(self.kappa * np.asarray(a["like"], np.float64)[ok] - np.asarray(post.tot_like, np.float64)[ok]))
        info = dict(F=F, n_ok=int(ok.sum()), num_frames=float(self.T[ok_n].sum()), den_weight=float(self.T[ok_d].sum()))
        if check:
            info["den_weight"] = float(sum(w for p in post.download() for f in p for _, w in f))
        post.close()
        lats.close()
        return info

    def accumulate_mpe(self, check=True):
        """--criterion mpe|smbr: the reference alignment and the ML block, the rescored lattices' signed posteriors, the two blocks
        -> dict(crit (the mean avg_acc / T), n_ok, pos_weight, neg_weight (check=True: the posteriors' sums by sign, downloaded))."""
        self.num.zero()
        self.den.zero()
        self.ml.zero()
        self.us_ali.loglikes(self.dm, reachable_only=True)
        self.us_ali.align(self.dt_ali, beam=10.0, retry_beam=40.0, acoustic_scale=self.kappa)
        self.us_ali.acc_stats(self.dm, self.dt_ali, self.ml)
        if self.lats0 is None:
            self.lats0 = self.decode_once()
        lats = self.lats0.rescore(self.us_dec, self.dm, self.dt_dec, 1.0)
        post = lats.mpe_posteriors(self.tid2phone, np.asarray([dx.tr.SIL], np.int32), ali_set=self.us_ali,
                                   criterion="mpfe" if self.criterion == "mpe" else "smbr", tid2pdf=self.tid2pdf, one_silence_class=True,
                                   graph_scale=1.0, acoustic_scale=self.kappa)
        self.us_dec.acc_stats_post2(self.dm, self.dt_dec, post, self.num, self.den)
        ok = (np.asarray(post.status) & 1) != 0
        crit = float(np.mean(np.asarray(post.avg_acc, np.float64)[ok] / self.T[ok])) if ok.any() else 0.0
        info = dict(crit=crit, n_ok=int(ok.sum()))
        if check:
            w = [x for p in post.download() for f in p for _, x in f]
            info["pos_weight"], info["neg_weight"] = float(sum(x for x in w if x > 0)), float(-sum(x for x in w if x < 0))
        post.close()
        lats.close()
        return info

    def boosted(self, lats):
        """lattice-boost-ali with the numerator alignment this set holds as the reference; the input handle is closed"""
        out = lats.boost(self.tid2phone, np.asarray([dx.tr.SIL], np.int32), ali_set=self.us_ali, b=self.boost, max_silence_error=0.0)
        lats.close()
        return out

    def decode_once(self):
        """--rescore: the denominator lattices of the whole run, decoded with the current (ML) model, boosted if asked"""
        self.us_dec.loglikes(self.dm)
        lats = self.us_dec.raw_lattices_faster_device(self.dt_dec, **self.dec)["lattices"]
        return self.boosted(lats) if self.boost else lats

    def update(self):
        return self.dm.ebw_update(self.num, self.den, self.opts, self.weight_opts, 0x7)

    def wer(self, utts):
        """Best paths of the lattice decoder on the shared graph with the current device model -> (errors, reference words)."""
        feats = [np.ascontiguousarray(u[2], np.float32) for u in utts]
        fo = np.concatenate([[0], np.cumsum([f.shape[0] for f in feats])]).astype(np.int64)
        us = khg.UtteranceSet(self.ctx, self.dt_dec, fo, np.ascontiguousarray(np.concatenate(feats), np.float32), graph=self.dg)
        us.loglikes(self.dm)
        r = us.decode_lattice_faster(self.dt_dec, **self.dec)
        errs = nref = 0
        for u, (_, ref, _) in enumerate(utts):
            hyp = r["words"][r["words_off"][u]: r["words_off"][u + 1]].tolist() if int(r["status"][u]) & 1 else []
            errs += dx.edit_distance(ref, hyp)
            nref += len(ref)
        us.close()
        return errs, nref

    def close(self):
        for h in (self.lats0, self.ml, self.num, self.den, self.us_ali, self.us_dec, self.dg, self.dm, self.dt_ali, self.dt_dec):
            if h is not None:
                h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=200)
    ap.add_argument("--test-utts", type=int, default=30)
    ap.add_argument("--iters", type=int, default=80)
    ap.add_argument("--dim", type=int, default=23)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--mmi-utts", type=int, default=60)
    ap.add_argument("--mmi-iters", type=int, default=4)
    ap.add_argument("--tau", type=float, default=50.0, help="I-smoothing count per Gaussian")
    ap.add_argument("--E", type=float, default=2.0)
    ap.add_argument("--kappa", type=float, default=0.1, help="acoustic scale")
    ap.add_argument("--rescore", action="store_true", help="decode the denominator lattices once, rescore them in every iteration")
    ap.add_argument("--boost", type=float, default=0.0, help="boosted MMI: b of lattice-boost-ali (0: off)")
    ap.add_argument("--criterion", choices=("mmi", "mpe", "smbr"), default="mmi", help="mpe / smbr: signed posteriors, gmm-acc-stats2")
    args = ap.parse_args()
    tm, tree, am, lexicon, test_utts = dx.train(args)
    train_utts = dx.tr.make_data(args.utts + args.test_utts, args.dim, np.random.default_rng(args.seed))[: args.mmi_utts]    # the same draw as train()
    comp = TrainingGraphCompiler(tm, tree, lexicon, sil_phone=dx.tr.SIL, sil_prob=0.5,
                                 opts=TrainingGraphCompilerOptions(transition_scale=1.0, self_loop_scale=1.0))
    graph = comp.compile_word_loop_graph()
    st = MmiState(khg._gpu.default_context(), tm, am, graph, train_utts, kappa=args.kappa, tau=args.tau, E=args.E, rescore=args.rescore,
                  boost=args.boost, criterion=args.criterion)
    e0, n0 = st.wer(test_utts)
    print(f"ML model: WER {100.0 * e0 / max(n0, 1):.2f}% ({e0} / {n0}) on {len(test_utts)} held-out utterances")
    failed = 0
    if args.criterion != "mmi":
        for it in range(args.mmi_iters):
            info = st.accumulate_mpe(check=False)
            untouched = st.num.smooth_with_accum(st.tau, st.ml, st.dm)
            r = st.update()
            failed += r["failed"]
            print(f"{args.criterion} iteration {it}: mean avg_acc / T = {info['crit']:.6f} over {info['n_ok']} utterances; "
                  f"update: {r['floored']} Gaussians floored, {r['failed']} failed, {r['skipped']} skipped, {untouched} without ML counts")
        info = st.accumulate_mpe(check=False)
        print(f"after {args.mmi_iters} iterations: mean avg_acc / T = {info['crit']:.6f}")
        e1, n1 = st.wer(test_utts)
        print(f"{args.criterion} model: WER {100.0 * e1 / max(n1, 1):.2f}% ({e1} / {n1})")
        st.close()
        return 0 if failed == 0 and e1 <= max(e0, 0.05 * n1) else 1
    for it in range(args.mmi_iters):
        info = st.accumulate(check=False)
        untouched = st.num.smooth_with_accum(st.tau, st.num, st.dm)
        r = st.update()
        failed += r["failed"]
        print(f"MMI iteration {it}: F = {info['F']:.4f} over {info['n_ok']} utterances ({info['F'] / max(info['num_frames'], 1):.5f} per frame); "
              f"update: {r['floored']} Gaussians floored, {r['failed']} failed, {r['skipped']} skipped, {untouched} without numerator counts, "
              f"auxf improvement {r['auxf_impr_gauss']:.3f} (Gaussians) {r['auxf_impr_weights']:.3f} (weights)")
    info = st.accumulate(check=False)
    print(f"after {args.mmi_iters} iterations: F = {info['F']:.4f}")
    e1, n1 = st.wer(test_utts)
    print(f"MMI model: WER {100.0 * e1 / max(n1, 1):.2f}% ({e1} / {n1})")
    st.close()
    return 0 if failed == 0 and e1 <= max(e0, 0.05 * n1) else 1


if __name__ == "__main__":
    sys.exit(main())
