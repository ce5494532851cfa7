"""gmm-acc-stats2 without a GPU: the sign split of tests/acc_post2_ref.py and its yardstick (the yardstick of
khg_acc_stats_post once per sign) against a plain float64 evaluation, the exported names, and what the C entry refuses before it
touches a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import acc_post2_ref as ref2
import acc_post_ref as ref
from helpers import build, utt_feats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECIAL = [-0.7, 1e-30, 0.0, 3.5]


def _posts(ut, m, seed):
    posts = ref.random_posts(ref.utt_pdfs(ut), m.id2pdf, seed=seed)
    return [[[(t, SPECIAL[(u + i + k) % 7] if (u + i + k) % 7 < 4 else w) for k, (t, w) in enumerate(f)] for i, f in enumerate(p)]
            for u, p in enumerate(posts)]


@pytest.mark.parametrize("scale", [1.0, -0.5])
def test_the_sign_split(scale):
    m, gc, om, ut, _ = build(12, 8, 13, n_utt=3, seed=2, ragged=True, max_phones=3)
    posts = _posts(ut, m, 8)
    pos, neg = ref2.split_posts(posts, scale)
    flat = lambda ps: [(u, i, t, w) for u, p in enumerate(ps) for i, f in enumerate(p) for t, w in f]  # noqa: E731
    all_, p_, n_ = flat(posts), flat(pos), flat(neg)
    assert [len(p) for p in pos] == [len(p) for p in posts] == [len(p) for p in neg]          # frames are kept
    assert not set(p_) & set(n_) and set(p_) | set(n_) <= set(all_)
    left = set(all_) - set(p_) - set(n_)
    # what belongs to neither: the zeros, and 1e-30 * -0.5 stays a float (5e-31) while nothing here underflows
    assert {w for *_, w in left} == {0.0}
    for *_, w in p_:
        assert np.float32(scale) * w > 0
    for *_, w in n_:
        assert np.float32(scale) * w < 0
    assert sum(1 for *_, w in p_ if abs(w) == 1e-30) + sum(1 for *_, w in n_ if abs(w) == 1e-30) == sum(1 for *_, w in all_ if w == 1e-30) > 0
    # an entry whose product underflows a float belongs to neither block
    tiny = [[[(1, 1e-60), (2, -1e-60), (3, 0.25)]]]
    pos, neg = ref2.split_posts(tiny, 1.0)
    assert pos == [[[(3, 0.25)]]] and neg == [[[]]]


@pytest.mark.parametrize("P,G,D,scale", [(12, 8, 13, 1.0), (9, 20, 40, -0.5)])
def test_yardstick_once_per_sign_against_float64(P, G, D, scale):
    m, gc, om, ut, _ = build(P, G, D, n_utt=3, seed=2, ragged=True, max_phones=3)
    feats = [utt_feats(ut, u) for u in range(3)]
    posts = _posts(ut, m, 8)
    num, den = ref2.oracle_post2(om, m.id2pdf, int(m.gauss_off[-1]), D, m.num_tids, feats, posts, scale)
    e_num, e_den = ref2.exact_post2(m, gc, feats, posts, scale)
    for got, exact, what in ((num, e_num, "num"), (den, e_den, "den")):
        ref.assert_stats(got, exact, what)
        assert (got["occ"] >= 0).all() and (got["trans_acc"] >= 0).all() and got["total_frames"] > 0, what
        assert np.abs(got["trans_acc"] - exact["trans_acc"]).max() <= 1e-12 * got["sum_abs_w"]
    # the two blocks together are the one block of khg_acc_stats_post: num - den
    one = ref.oracle_post(om, m.id2pdf, int(m.gauss_off[-1]), D, m.num_tids, feats, posts, scale)
    for k in ("occ", "mean_acc", "var_acc", "trans_acc"):
        assert np.abs((num[k] - den[k]) - one[k]).max() <= 1e-9 * max(1.0, np.abs(num[k]).max() + np.abs(den[k]).max()), k
    w = [float(ref.entry_weight(scale, x)) for p in posts for f in p for _, x in f]
    assert abs(num["total_frames"] - sum(x for x in w if x > 0)) <= 1e-12 * num["sum_abs_w"]
    assert abs(den["total_frames"] + sum(x for x in w if x < 0)) <= 1e-12 * den["sum_abs_w"]


def test_the_names_exist():
    with open(os.path.join(ROOT, "include", "khg_hip.h")) as fh:
        text = fh.read()
    from kaldi_hmm_gmm_amd import _lib
    so = os.path.join(ROOT, "kaldi_hmm_gmm_amd", "libkhg_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    for name in ("khg_acc_stats_post2", "khg_acc_stats_post"):
        assert re.search(r"\bint %s\(" % name, text), name
        assert name in _lib.SIGNATURES and getattr(_lib.lib, name) is not None, name
        assert re.search(r" T %s$" % name, out, re.M), name
    import kaldi_hmm_gmm_amd as khg
    assert hasattr(khg.UtteranceSet, "acc_stats_post2")
    for n in ("gmm_acc_stats2", "gmm_acc_stats2_batch", "lattice_to_mpe_post", "lattice_to_smbr_post", "lattice_to_mpe_post_batch",
              "lattice_to_smbr_post_batch"):
        assert callable(getattr(khg, n)), n


def test_host_refusals():
    """NULL handles are KHG_E_ARG (-1) before any device is touched, and the message names the call"""
    from kaldi_hmm_gmm_amd import _lib
    last = lambda: _lib.lib.khg_last_error().decode()  # noqa: E731
    assert _lib.lib.khg_acc_stats_post2(None, None, None, None, None, 1.0, None, None) == -1
    assert "khg_acc_stats_post2:" in last()
    assert _lib.lib.khg_acc_stats_post(None, None, None, None, None, 1.0, None) == -1
    assert "khg_acc_stats_post:" in last()
    out = C.c_void_p()
    assert _lib.lib.khg_lattices_mpe_posteriors(None, None, 0, None, None, 0, None, None, None, None, 0, 1, 1.0, 1.0, None, None, None, C.byref(out)) == -1
    assert "khg_lattices_mpe_posteriors:" in last()
