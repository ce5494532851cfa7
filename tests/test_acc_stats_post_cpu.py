"""gmm-acc-stats without a GPU: the Posterior helpers, khg_posteriors_validate (host only), the yardstick of
tests/test_gpu_acc_stats_post.py against a plain float64 evaluation of the rule, and the inputs of its bucket-edge test."""
import numpy as np
import pytest

import acc_post_ref as ref
from helpers import build, utt_feats
from kaldi_hmm_gmm_amd import _kaldi_hmm_gmm_amd as ext
from kaldi_hmm_gmm_amd import ali_to_post, arrays_to_posts, posts_to_arrays


def test_ali_to_post_and_array_round_trip():
    assert ali_to_post([3, 3, 4]) == [[(3, 1.0)], [(3, 1.0)], [(4, 1.0)]]
    id2pdf = np.concatenate([[0], np.arange(20) // 2]).astype(np.int32)
    rng = np.random.default_rng(0)
    posts = ref.random_posts([rng.integers(0, 10, size=T) for T in (7, 0, 12, 1)], id2pdf, seed=3) + [[]]
    fo, eb, tid, w = posts_to_arrays(posts)
    assert fo.tolist() == [0, 7, 7, 19, 20, 20] and eb[0] == 0 and eb[-1] == len(tid) == len(w) and len(eb) == 21
    assert fo.dtype == eb.dtype == np.int64 and tid.dtype == np.int32 and w.dtype == np.float64
    assert arrays_to_posts(fo, eb, tid, w) == posts
    assert any(len(f) == 0 for p in posts for f in p) and max(len(f) for p in posts for f in p) == 5
    for p in posts:
        for f in p:
            assert len({t for t, _ in f}) == len(f) and all(x > 0 for _, x in f)
    norm = ref.random_posts([rng.integers(0, 10, size=30)], id2pdf, seed=4, normalise=True)
    assert all(abs(sum(x for _, x in f) - 1.0) < 1e-12 for f in norm[0] if f)


def test_validate():
    id2pdf = np.concatenate([[0], np.arange(12) // 2]).astype(np.int32)
    fo, eb, tid, w = posts_to_arrays(ref.random_posts([np.arange(9) % 6, [], np.arange(14) % 6], id2pdf, seed=1))
    ext.posteriors_validate(fo, eb, tid, w)
    ext.posteriors_validate(fo, eb, tid, -w)              # a weight of any sign

    def refused(fo=fo, eb=eb, tid=tid, w=w):
        with pytest.raises(Exception) as e:
            ext.posteriors_validate(fo, eb, tid, w)
        return str(e.value)

    bad = fo.copy(); bad[1], bad[2] = 12, 9              # non-monotone utterance offsets
    assert "frame_off" in refused(fo=bad)
    bad = eb.copy(); bad[3], bad[4] = bad[4] + 1, bad[3]  # non-monotone entry offsets
    assert "entry_begin" in refused(eb=bad)
    bad = eb.copy(); bad[-1] -= 1                         # not ending at the count
    assert "entry_begin" in refused(eb=bad)
    assert "entry_begin" in refused(tid=tid[:-1], w=w[:-1])
    bad = tid.copy(); bad[5] = 0
    assert "transition-id" in refused(tid=bad)
    for v in (np.nan, np.inf, -np.inf):
        bad = w.copy(); bad[2] = v
        assert "finite" in refused(w=bad)


@pytest.mark.parametrize("P,G,D,scale", [(12, 8, 13, 1.0), (9, 20, 40, -0.5)])
def test_yardstick_against_float64(P, G, D, scale):
    m, gc, om, ut, _ = build(P, G, D, n_utt=3, seed=2, ragged=True, max_phones=3)
    feats = [utt_feats(ut, u) for u in range(3)]
    posts = ref.random_posts(ref.utt_pdfs(ut), m.id2pdf, seed=8)
    want = ref.oracle_post(om, m.id2pdf, int(m.gauss_off[-1]), D, m.num_tids, feats, posts, scale)
    exact = ref.exact_post(m, gc, feats, posts, scale)
    ref.assert_stats(want, exact, "oracle loop against float64")
    assert np.abs(want["trans_acc"] - exact["trans_acc"]).max() <= 1e-12 * want["sum_abs_w"]
    assert abs(want["total_frames"] - exact["total_frames"]) <= 1e-12 * want["sum_abs_w"]


def test_oracle_meets_the_float64_bound_on_uniform_ids():
    """ordinary weights on ids of any pdf: the oracle's fp32 chain within the bound derived in tests/acc_post_ref.py -- and not
    within the K3 tolerances, which is why the device is held to float64 there"""
    m, gc, om, ut, _ = build(30, 64, 40, n_utt=12, seed=7, max_phones=3)
    feats = [utt_feats(ut, u) for u in range(12)]
    posts = ref.uniform_posts([len(f) for f in feats], m.num_tids, seed=5)
    want = ref.oracle_post(om, m.id2pdf, int(m.gauss_off[-1]), 40, m.num_tids, feats, posts)
    exact = ref.exact_post(m, gc, feats, posts, bounds=True)
    worst = ref.assert_within_bounds(want, exact, "oracle")
    print("oracle against float64: largest error / bound %.3g" % worst)
    assert worst > 1e-3           # the bound is not vacuous: the fp32 chain uses a visible part of it
    with pytest.raises(AssertionError):
        ref.assert_stats(want, exact)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 128, 129])
def test_bucket_edge_inputs(n):
    m = ref.edge_model()[0]
    posts = ref.bucket_edge_posts(n)
    cnt = ref.entries_per_pdf(posts, m.id2pdf, 4)
    assert len(posts) == 1 and len(posts[0]) == ref.EDGE_T
    assert cnt[0] == n and cnt[1] == 0 and cnt[2] >= 3000 and cnt[3] == 61 and cnt.sum() == n + 3061
    pdf_of_frame = ref.EDGE_PDF[ref.edge_order()]
    assert all(m.id2pdf[t] == pdf_of_frame[i] for i, f in enumerate(posts[0]) for t, _ in f)
