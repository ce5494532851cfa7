"""Cases of the MLLT tests (tests/test_mllt_cpu.py, tests/test_gpu_mllt.py): synthetic models of tests/helpers.py, features drawn from
them and mixed by a fixed well-conditioned matrix (so that a diagonal model no longer fits and MLLT has something to find),
posteriors, and the restatement's statistics -- computed once per case and shared read-only."""
import functools
import types

import numpy as np

import fmllr_cases as fcases
import mllt_ref as ref
from helpers import build
from oracle import oracle as orc

GSLICE = ref.GSLICE


def mixing(D, seed, strength=0.3):
    rng = np.random.default_rng(seed)
    return np.eye(D) + strength * rng.standard_normal((D, D)) / np.sqrt(D)


def offset_model(m, off):
    """the same model with every mean moved by `off` in every dimension -> (model namespace, gconsts)"""
    mu = ref.means(m) + np.float32(off)
    miv = (mu * m.inv_vars).astype(np.float32)
    gc = orc.model_gconsts(m.gauss_off, m.weights, m.inv_vars, miv)
    ns = types.SimpleNamespace(gauss_off=m.gauss_off, weights=m.weights, inv_vars=m.inv_vars, means_invvars=miv, id2pdf=m.id2pdf,
                               num_tids=m.num_tids, dim=m.dim)
    return ns, gc


def mixed_set(m, lens, seed, D):
    """frames drawn from the model's Gaussians, passed through y = R (x - mean) + mean: correlated, same location"""
    feats, pdfs = fcases.draw_set(m, lens, seed)
    R = mixing(D, seed + 100)
    centre = ref.means(m).astype(np.float64).mean(0)
    feats = [np.ascontiguousarray((f.astype(np.float64) - centre) @ R.T + centre, np.float32) for f in feats]
    return feats, pdfs


def host_am(m):
    """the model as a host AmDiagGmm"""
    import kaldi_hmm_gmm_amd as khg
    am = khg.AmDiagGmm()
    for p in range(len(m.gauss_off) - 1):
        a, b = int(m.gauss_off[p]), int(m.gauss_off[p + 1])
        g = khg.DiagGmm(b - a, m.inv_vars.shape[1])
        g.set_weights(m.weights[a:b]); g.set_invvars(m.inv_vars[a:b]); g._means_invvars = m.means_invvars[a:b].copy(); g.compute_gconsts()
        am.add_pdf(g)
    return am


def skewed_set(m, lens, seed, D, share=0.8):
    """mixed_set with `share` of the frames given to pdf 0 (silence in a real alignment): one bucket far above the average"""
    feats, pdfs = mixed_set(m, lens, seed, D)
    rng = np.random.default_rng(seed + 7)
    pdfs = [np.where(rng.random(len(p)) < share, 0, np.asarray(p)) for p in pdfs]
    return feats, pdfs


@functools.lru_cache(maxsize=None)
def estimate_case(D, G, T, off=0.0, seed=3):
    """a model of 3 pdfs x G Gaussians, T mixed frames in two utterances, unit posteriors from the alignment, and the restatement's
    statistics (float64 posteriors)"""
    m, gc, om, ut, _ = build(3, G, D, n_utt=1, seed=seed + D, max_phones=2)
    if off:
        m, gc = offset_model(m, off)
    feats, pdfs = mixed_set(m, [T // 2, T - T // 2], seed + 2, D)
    posts = fcases.ali_posts(m, pdfs, seed + 3)
    st = ref.acc_stats(m, gc, feats, posts, dtype=np.float64)
    for k in ("G", "S", "C", "c"):
        st[k].setflags(write=False)
    return dict(m=m, gc=gc, feats=feats, pdfs=pdfs, posts=posts, stats=st)
