"""The host chain of MPE / sMBR training on the YES/NO task, without a GPU: what examples/train_mmi_synthetic.py --criterion mpe|smbr
does on the device, restated from the project's own yardsticks (tests/ebw_host_chain.py does the same for MMI) --

  once          the lattice-faster decoder's raw lattices on the word loop under the ML model (tests/lattice_faster_raw_ref.py);
  reference     the oracle's aligner on the transcripts' training graphs; the oracle's acc-stats of it are the ML block;
  posteriors    the lattices rescored with the current model (tests/lattice_rescore_ref.py, scale 1), then tests/lattice_mpe_ref.py at
                scales (1, kappa) with that alignment as the reference;
  statistics    the oracle's acc-stats once per entry (tests/acc_post_ref.py), the positive entries into the numerator block, the
                negated negative ones into the denominator block;
  update        tests/ebw_ref.py: smooth_with_accum of the numerator block with the ML block, then the Extended Baum-Welch update.

The criterion is the mean over the utterances of avg_acc / T.  DESIGN.md 7k records the run."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import acc_post_ref  # noqa: E402
import ebw_ref  # noqa: E402
import lattice_faster_raw_ref as rawf  # noqa: E402
import lattice_faster_ref as lref  # noqa: E402
import lattice_mpe_ref as mr  # noqa: E402
import lattice_rescore_ref as rr  # noqa: E402
from ebw_host_chain import HostChain  # noqa: E402
from oracle import oracle as orc  # noqa: E402


class MpeHostChain(HostChain):
    def __init__(self, khg, tm, am, graph, utts, criterion="smbr", silence_phones=(1,), kappa=0.1, tau=50.0, E=2.0):
        super().__init__(khg, tm, am, graph, utts, kappa=kappa, tau=tau, E=E)
        self.criterion = "mpfe" if criterion == "mpe" else criterion
        self.tid2phone = np.asarray(tm.transition_id_to_phone_array(), np.int32)
        self.sil = tuple(int(x) for x in silence_phones)
        om = orc.OModel(self.go, self.gc, self.miv, self.iv)
        self.lats = []
        for x in self.feats:
            ll = lref.score_fn(orc.loglikes_matrix(om, x, self.pdfs), self.pdfs, self.id2pdf, self.kappa)
            lat, res = rawf.rule_lattice(self.den_graph, self.cfg, ll, len(x))
            self.lats.append(lat if res["succeeded"] else None)

    def accumulate(self):
        """-> (mean avg_acc / T, utterances in it, numerator block, denominator block, ML block, (sum of positive weights, of negative))"""
        om = orc.OModel(self.go, self.gc, self.miv, self.iv)
        G, D = int(self.go[-1]), self.miv.shape[1]
        ml = orc.OAccs(G, D, self.num_tids)
        pos, neg, crit = [], [], []
        for x, og, lat in zip(self.feats, self.num_graphs, self.lats):
            a = orc.align_utterance(og, om, self.id2pdf, x, acoustic_scale=self.kappa, beam=10.0, retry_beam=40.0)
            ok_n = (a["status"] & 1) == 0
            if ok_n:
                orc.acc_stats_ali(om, self.id2pdf, x, a["ali"], ml)
            post = []
            if ok_n and lat is not None:
                ll = lref.score_fn(orc.loglikes_matrix(om, x, self.pdfs), self.pdfs, self.id2pdf, 1.0)
                r = mr.forward_backward_mpe(rr.rescore_from_ll(lat, ll, 1.0), self.tid2phone, self.id2pdf, self.sil, np.asarray(a["ali"], np.int32),
                                            self.criterion, True, 1.0, self.kappa)
                if r["status"] == mr.SUCCEEDED:
                    post = r["post"]
                    crit.append(r["avg"] / len(x))
            pos.append([[(t, w) for t, w in f if w > 0] for f in post])
            neg.append([[(t, -w) for t, w in f if w < 0] for f in post])
        num = acc_post_ref.oracle_post(om, self.id2pdf, G, D, self.num_tids, self.feats, pos)
        den = acc_post_ref.oracle_post(om, self.id2pdf, G, D, self.num_tids, self.feats, neg)
        blk = lambda d: (d["occ"], d["mean_acc"], d["var_acc"])  # noqa: E731
        return (float(np.mean(crit)) if crit else 0.0, len(crit), blk(num), blk(den), (ml.occ.copy(), ml.mean_acc.copy(), ml.var_acc.copy()),
                (num["frames_seq"], den["frames_seq"]))

    def update(self, num, den, ml):
        occ, mean, var, _ = ebw_ref.accs_smooth_with_accum(num[0], num[1], num[2], self.tau, ml[0], ml[1], ml[2])
        r = ebw_ref.ebw_update(self.go, self.w, self.miv, self.iv, (occ, mean, var), den, 0x7, E=self.E)
        self.w, self.miv, self.iv, self.gc = r["weights"], r["means_invvars"], r["inv_vars"], r["gconsts"]
        return r


def run(khg, tm, am, graph, utts, iters=3, **kw):
    """-> [c_0, ..., c_iters]: the criterion before every update and after the last"""
    hc = MpeHostChain(khg, tm, am, graph, utts, **kw)
    out = []
    for _ in range(iters):
        c, n, num, den, ml, _ = hc.accumulate()
        out.append(c)
        hc.update(num, den, ml)
    out.append(hc.accumulate()[0])
    return out


if __name__ == "__main__":          # the run DESIGN.md 7k records: python tests/mpe_host_chain.py
    import types
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import decode_synthetic as dx
    import kaldi_hmm_gmm_amd as khg_
    from kaldi_hmm_gmm_amd.training_graph import TrainingGraphCompiler, TrainingGraphCompilerOptions
    args = types.SimpleNamespace(utts=200, test_utts=30, iters=80, dim=23, seed=3)          # the `trained` fixture of the GPU tests
    tm_, tree, am_, lexicon, test_utts = dx.train(args, log=lambda *a: None)
    graph_ = TrainingGraphCompiler(tm_, tree, lexicon, sil_phone=dx.tr.SIL, sil_prob=0.5,
                                   opts=TrainingGraphCompilerOptions(transition_scale=1.0, self_loop_scale=1.0)).compile_word_loop_graph()
    for crit_ in ("mpe", "smbr"):
        print(crit_, ["%.17g" % c for c in run(khg_, tm_, am_, graph_, test_utts[:30], criterion=crit_, silence_phones=(dx.tr.SIL,))], flush=True)
