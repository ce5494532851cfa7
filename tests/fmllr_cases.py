"""Cases of the fMLLR tests (tests/test_fmllr_cpu.py, tests/test_gpu_fmllr.py): synthetic models of tests/helpers.py, features drawn
from them (optionally through a known affine map per speaker), posteriors, and the restatement's statistics -- computed once per
case and shared read-only."""
import functools

import numpy as np

import acc_post_ref as apr
import fmllr_ref as ref
from helpers import build

SLICE = 1024          # frames of one work item of the Gram kernel (khg_fmllr_stats.hip.inc: FM_SLICE)


def draw_set(m, lens, seed, maps=None, utt2spk=None):
    """Utterances of the given lengths: every frame is drawn from one Gaussian of one pdf (the pdf that fits it).  maps[s] = (A, b):
    the frames of speaker s's utterances are passed through y = A x + b.  -> (feats list of float32 [T, D], frame_pdfs list)"""
    rng = np.random.default_rng(seed)
    D = m.means_invvars.shape[1]
    P = len(m.gauss_off) - 1
    mu = m.means_invvars.astype(np.float64) / m.inv_vars.astype(np.float64)
    sd = 1.0 / np.sqrt(m.inv_vars.astype(np.float64))
    feats, pdfs = [], []
    for u, T in enumerate(lens):
        p = rng.integers(0, P, size=T)
        g = np.array([rng.integers(m.gauss_off[q], m.gauss_off[q + 1]) for q in p], np.int64) if T else np.zeros(0, np.int64)
        x = mu[g] + sd[g] * rng.standard_normal((T, D))
        if maps is not None and utt2spk is not None and utt2spk[u] >= 0:
            A, b = maps[int(utt2spk[u])]
            x = x @ A.T + b
        feats.append(np.ascontiguousarray(x, np.float32))
        pdfs.append([int(q) for q in p])
    return feats, pdfs


def speaker_maps(n_spk, D, seed, strength=0.15):
    rng = np.random.default_rng(seed)
    return [(np.eye(D) + strength * rng.standard_normal((D, D)) / np.sqrt(D), strength * rng.standard_normal(D)) for _ in range(n_spk)]


def ali_posts(m, pdfs, seed):
    """one entry of weight 1 per frame: an id of the frame's own pdf (ali-to-post of an alignment)"""
    rng = np.random.default_rng(seed)
    id2pdf = np.asarray(m.id2pdf)
    own = {p: np.nonzero(id2pdf[1:] == p)[0] + 1 for p in range(len(m.gauss_off) - 1)}
    return [[[(int(rng.choice(own[p])), 1.0)] for p in fp] for fp in pdfs]


def freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def estimate_case(P, G, D, T, n_spk=2, seed=3):
    """a model, n_spk speakers of T frames each (two utterances per speaker, interleaved) distorted by a known map each, unit
    posteriors from the alignment, and the restatement's float32-rule statistics"""
    m, gc, om, ut, _ = build(P, G, D, n_utt=1, seed=seed, max_phones=2)
    utt2spk = np.array([s for _ in range(2) for s in range(n_spk)], np.int32)
    lens = [T // 2 if i < n_spk else T - T // 2 for i in range(2 * n_spk)]
    maps = speaker_maps(n_spk, D, seed + 1)
    feats, pdfs = draw_set(m, lens, seed + 2, maps, utt2spk)
    posts = ali_posts(m, pdfs, seed + 3)
    beta, K, Gs = freeze(*ref.acc_stats(m, gc, feats, posts, utt2spk, n_spk, dtype=np.float32))
    return dict(m=m, gc=gc, feats=feats, pdfs=pdfs, posts=posts, utt2spk=utt2spk, maps=maps, beta=beta, K=K, G=Gs, n_spk=n_spk)


@functools.lru_cache(maxsize=None)
def one_gaussian_converged(D=4, T=60, seed=5):
    """The tie: ONE Gaussian whose mean and variance are the data's own (a converged model).  Then e2 -> 0 in the row update and its
    two roots mirror each other: their auxiliary values agree to ~1e-15, and which one wins is decided by the rounding of log."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T, D)).astype(np.float32).astype(np.float64)
    mu, var = x.mean(0), x.var(0)
    xp = np.concatenate([x, np.ones((T, 1))], 1)
    il, jl = np.tril_indices(D + 1)
    K = np.stack([(mu[d] / var[d]) * xp.sum(0) for d in range(D)])
    G = np.stack([((xp.T @ xp) / var[d])[il, jl] for d in range(D)])
    return float(T), K, G


def tiny_case():
    """three pdfs' worth of frames, multi-entry posteriors, for the definition check"""
    m, gc, om, ut, _ = build(4, 3, 3, n_utt=1, seed=9, max_phones=2)
    utt2spk = np.array([0, 1, 0, -1], np.int32)
    feats, pdfs = draw_set(m, [7, 5, 4, 6], 21)
    posts = apr.random_posts(pdfs, m.id2pdf, seed=4)
    return m, gc, feats, posts, utt2spk
