"""The host chain of one MMI iteration on the YES/NO task, without a GPU: what examples/train_mmi_synthetic.py (MmiState) does on
the device, restated from the project's own yardsticks --

  numerator     the oracle's aligner (orc.align_utterance) on the transcripts' training graphs, the oracle's acc-stats;
  denominator   the oracle's log-likelihoods, tests/lattice_faster_raw_ref.py (the lattice-faster decoder's raw lattice on the word
                loop), tests/lattice_post_ref.py (forward-backward, float64), the oracle's acc-stats once per entry
                (tests/acc_post_ref.py);
  update        tests/ebw_ref.py: smooth_with_accum of the numerator block with itself, then the Extended Baum-Welch update.

F = sum_u (kappa like_u - logZ_u) over the utterances that aligned and decoded.  tests/test_gpu_ebw.py uses iteration 0 of this
chain for the margin of its assertion on the device's F; DESIGN.md 7i records the whole run that chose E."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
import acc_post_ref  # noqa: E402
import ebw_ref  # noqa: E402
import lattice_faster_raw_ref as rawf  # noqa: E402
import lattice_faster_ref as lref  # noqa: E402
import lattice_post_ref as pref  # noqa: E402
from oracle import oracle as orc  # noqa: E402


class HostChain:
    def __init__(self, khg, tm, am, graph, utts, kappa=0.1, tau=50.0, E=2.0):
        import train_mmi_synthetic as mmi
        from kaldi_hmm_gmm_amd.fst import concat_graphs
        from kaldi_hmm_gmm_amd.training_graph import TrainingGraphCompiler
        self.kappa, self.tau, self.E = float(kappa), float(tau), float(E)
        self.feats = [np.ascontiguousarray(u[2], np.float32) for u in utts]
        go, gc, w, miv, iv = am.flat()
        self.go = np.asarray(go, np.int32)
        self.w, self.gc = np.array(w, np.float32), np.array(gc, np.float32)
        self.miv, self.iv = np.array(miv, np.float32), np.array(iv, np.float32)
        self.id2pdf = np.asarray(tm.transition_id_to_pdf_array(), np.int32)
        self.num_tids = len(self.id2pdf) - 1
        tree = khg.monophone_context_dependency(tm.topo.phones, tm.topo.get_phone_to_num_pdf_classes())
        comp = TrainingGraphCompiler(tm, tree, mmi.LEXICON, sil_phone=mmi.dx.tr.SIL, sil_prob=0.5)
        g = dict(concat_graphs(comp.compile_graphs_from_text([u[1] for u in utts])))
        cost = np.asarray(tm.scaled_trans_cost(1.0, 0.1), np.float32)
        g["weight"] = np.where(g["ilabel"] >= 1, g["weight"] + cost[np.maximum(g["ilabel"], 0)], g["weight"]).astype(np.float32)
        self.num_graphs = [orc.OGraph.from_set(g, u) for u in range(len(utts))]
        c = graph.to_csr()
        self.den_graph = lref.Graph(c["start"], c["arc_off"], c["ilabel"], c["olabel"], c["weight"], c["nextstate"], c["final"])
        self.cfg = lref.Config(beam=13.0, max_active=7000, lattice_beam=6.0)
        self.pdfs = np.arange(len(self.go) - 1, dtype=np.int32)

    def accumulate(self):
        """-> (F, number of utterances in it, numerator block, denominator block); a block = (occ, mean_acc, var_acc)"""
        om = orc.OModel(self.go, self.gc, self.miv, self.iv)
        G, D = int(self.go[-1]), self.miv.shape[1]
        num = orc.OAccs(G, D, self.num_tids)
        posts, F, n = [], 0.0, 0
        for x, og in zip(self.feats, self.num_graphs):
            a = orc.align_utterance(og, om, self.id2pdf, x, acoustic_scale=self.kappa, beam=10.0, retry_beam=40.0)
            ok_n = (a["status"] & 1) == 0
            if ok_n:
                orc.acc_stats_ali(om, self.id2pdf, x, a["ali"], num)
            ll = lref.score_fn(orc.loglikes_matrix(om, x, self.pdfs), self.pdfs, self.id2pdf, self.kappa)
            lat, res = rawf.rule_lattice(self.den_graph, self.cfg, ll, len(x))
            fb = pref.forward_backward(lat, 1.0, 1.0) if res["succeeded"] else {"status": pref.NO_PATH, "post": []}
            ok_d = fb["status"] == pref.SUCCEEDED
            posts.append(fb["post"] if ok_d else [])
            if ok_n and ok_d:
                F += self.kappa * float(a["like"]) - fb["tot"]
                n += 1
        den = acc_post_ref.oracle_post(om, self.id2pdf, G, D, self.num_tids, self.feats, posts)
        return F, n, (num.occ.copy(), num.mean_acc.copy(), num.var_acc.copy()), (den["occ"], den["mean_acc"], den["var_acc"])

    def update(self, num, den):
        occ, mean, var, _ = ebw_ref.accs_smooth_with_accum(num[0], num[1], num[2], self.tau, num[0], num[1], num[2])
        r = ebw_ref.ebw_update(self.go, self.w, self.miv, self.iv, (occ, mean, var), den, 0x7, E=self.E)
        self.w, self.miv, self.iv, self.gc = r["weights"], r["means_invvars"], r["inv_vars"], r["gconsts"]
        return r


def run(khg, tm, am, graph, utts, iters=3, **kw):
    """-> [F_0, ..., F_iters]: F before every update and after the last"""
    hc = HostChain(khg, tm, am, graph, utts, **kw)
    out = []
    for _ in range(iters):
        F, n, num, den = hc.accumulate()
        out.append(F)
        hc.update(num, den)
    out.append(hc.accumulate()[0])
    return out
