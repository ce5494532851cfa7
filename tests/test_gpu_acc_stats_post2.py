"""khg_acc_stats_post2 (gmm-acc-stats2 from signed posteriors resident on the device) through
UtteranceSet.acc_stats_post2, against the yardstick of khg_acc_stats_post called once per sign (tests/acc_post2_ref.py).

Tolerances are section 7h's (tests/acc_post_ref.py: assert_stats): occ rtol 2e-5 / atol 1e-6, mean_acc / var_acc rtol 2e-5 / atol
2e-6 x the largest magnitude, total_log_like rel 2e-6, trans_acc and total_frames within 1e-12 * sum|w|.  Two device runs that differ
only in the order of their fp64 additions: 1e-11 * max|.| per array.

The MPE / sMBR loop on the YES/NO task asserts the equalities.  Whether it also asserts a rise of the criterion (the mean avg_acc / T)
is decided as 7i decided it: only where the host chain's rise over three iterations (tests/mpe_host_chain.py) exceeds ten times the
host / device difference at iteration 0.  sMBR: the host chain gives 0.99980741981310561, 0.9998132619567095, 0.99981290243308274 and
0.99981375203825817 after the third update, a rise of 6.33e-6 where the device's c_0 lies 3.6e-12 from the host's: the rise is
asserted, with the host's c_0 carried as a constant as 7i's test carries F_0.  MPFE: the task saturates -- every path of these
lattices has the reference's phone on every frame, the criterion is 1 to 5e-15 on the host and on the device and the signed weights
are rounding noise (1e-13 in total) -- so only the equalities are asserted there."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import acc_post2_ref as ref2  # noqa: E402
import acc_post_ref as ref  # noqa: E402
import ebw_cases  # noqa: E402
from helpers import build, utt_feats  # noqa: E402
from test_gpu_lattice_faster_raw import trained  # noqa: E402,F401

pytestmark = pytest.mark.gpu

KEYS = ("occ", "mean_acc", "var_acc", "trans_acc")
SPECIAL = [-0.7, 1e-30, 0.0, 3.5]
GC_ULPS = 4
C0_HOST_SMBR = 0.99980741981310561      # tests/mpe_host_chain.py, iteration 0, on the set of test_mpe_loop_on_the_yes_no_task


def _device(ctx, m, gc, frame_off, feats):
    from kaldi_hmm_gmm_amd import DeviceAccs, DeviceModel, DeviceTransitions, UtteranceSet
    dm = DeviceModel(ctx, m.gauss_off, gc, m.means_invvars, m.inv_vars)
    tm = DeviceTransitions(ctx, m.id2pdf)
    us = UtteranceSet(ctx, None, np.asarray(frame_off, np.int64), np.ascontiguousarray(feats, np.float32))
    return dm, tm, us, DeviceAccs(ctx, dm, tm), DeviceAccs(ctx, dm, tm)


def _run2(ctx, us, dm, tm, num, den, posts, scale=1.0):
    from kaldi_hmm_gmm_amd import DevicePosteriors
    post = DevicePosteriors.from_posteriors(ctx, posts)
    us.acc_stats_post2(dm, tm, post, num, den, scale=scale)
    got = num.download(), den.download()
    post.close()
    return got


def _zero(block):
    return all(not np.asarray(block[k]).any() for k in KEYS) and block["total_frames"] == 0.0 and block["total_log_like"] == 0.0


@functools.lru_cache(maxsize=None)
def _weights_case(P, G, D, scale):
    """weights -0.7 / 1e-30 / 0 / 3.5 on entries of the frame's own pdf (tests/acc_post_ref.py says why the others keep their small
    weights; here every second one of those is negative); the yardstick once per sign, computed once per shape"""
    m, gc, om, ut, _ = build(P, G, D, n_utt=12, seed=7, ragged=(D % 2 == 1), max_phones=3)
    posts = ref.random_posts(ref.utt_pdfs(ut), m.id2pdf, seed=P + G + D)
    pdfs = ref.utt_pdfs(ut)
    posts = [[[(t, SPECIAL[(u + i + k) % 7] if (u + i + k) % 7 < 4 and m.id2pdf[t] == pdfs[u][i] else (w if (i + k) % 2 else -w)) for k, (t, w) in enumerate(f)]
              for i, f in enumerate(p)] for u, p in enumerate(posts)]
    flat = [w for p in posts for f in p for _, w in f]
    assert all(flat.count(s) > 3 for s in SPECIAL)
    feats = [utt_feats(ut, u) for u in range(12)]
    num, den = ref2.oracle_post2(om, m.id2pdf, int(m.gauss_off[-1]), D, m.num_tids, feats, posts, scale)
    return m, gc, ut, posts, num, den


@pytest.mark.parametrize("form", [0, 2])
@pytest.mark.parametrize("P,G,D", [(6, 7, 40), (3, 100, 77)])
def test_weights_of_both_signs(ctx, opt, P, G, D, form):
    if form:
        opt("k3_form", form)
    scale = -0.5
    m, gc, ut, posts, w_num, w_den = _weights_case(P, G, D, scale)
    dm, tm, us, num, den = _device(ctx, m, gc, ut.frame_off, ut.feats)
    g_num, g_den = _run2(ctx, us, dm, tm, num, den, posts, scale=scale)
    ref.assert_stats(g_num, w_num, ("num", P, G, D, form))
    ref.assert_stats(g_den, w_den, ("den", P, G, D, form))
    for g in (g_num, g_den):
        assert (g["occ"] >= 0).all() and (g["trans_acc"] >= 0).all() and g["total_frames"] > 0
    # the two blocks are what khg_acc_stats_post puts into one: num - den
    from kaldi_hmm_gmm_amd import DeviceAccs, DevicePosteriors
    one = DeviceAccs(ctx, dm, tm)
    post = DevicePosteriors.from_posteriors(ctx, posts)
    us.acc_stats_post(dm, tm, post, one, scale=scale)
    g_one = one.download()
    post.close()
    for k in KEYS:
        assert np.abs((g_num[k] - g_den[k]) - g_one[k]).max() <= 1e-11 * (np.abs(g_num[k]).max() + np.abs(g_den[k]).max()), k
    # once more into the same blocks: twice the statistics (the set's buffers are found as the call left them)
    t_num, t_den = _run2(ctx, us, dm, tm, num, den, posts, scale=scale)
    for k in KEYS:
        assert np.abs(t_num[k] - 2.0 * g_num[k]).max() <= 1e-11 * np.abs(t_num[k]).max() and np.abs(t_den[k] - 2.0 * g_den[k]).max() <= 1e-11 * np.abs(t_den[k]).max(), k


@pytest.mark.parametrize("P,G,D", [(6, 7, 40), (3, 100, 77)])
def test_all_positive_is_acc_stats_post_and_den_stays_zero(ctx, P, G, D):
    from kaldi_hmm_gmm_amd import DeviceAccs, DevicePosteriors
    m, gc, om, ut, _ = build(P, G, D, n_utt=12, seed=7, ragged=(D % 2 == 1), max_phones=3)
    posts = ref.random_posts(ref.utt_pdfs(ut), m.id2pdf, seed=3)
    dm, tm, us, num, den = _device(ctx, m, gc, ut.frame_off, ut.feats)
    g_num, g_den = _run2(ctx, us, dm, tm, num, den, posts)
    one = DeviceAccs(ctx, dm, tm)
    post = DevicePosteriors.from_posteriors(ctx, posts)
    us.acc_stats_post(dm, tm, post, one)
    g_one = one.download()
    for k in ("occ", "mean_acc", "var_acc"):
        assert np.abs(g_num[k] - g_one[k]).max() <= 1e-11 * np.abs(g_one[k]).max(), k
    bound = 1e-12 * sum(abs(w) for p in posts for f in p for _, w in f)
    assert np.abs(g_num["trans_acc"] - g_one["trans_acc"]).max() <= bound and abs(g_num["total_frames"] - g_one["total_frames"]) <= bound
    assert abs(g_num["total_log_like"] - g_one["total_log_like"]) <= 1e-11 * abs(g_one["total_log_like"])
    assert _zero(g_den)
    # ... and under a negative scale everything goes to den, num stays zero
    num.zero()
    g_num, g_den = _run2(ctx, us, dm, tm, num, den, posts, scale=-1.0)
    assert _zero(g_num)
    for k in ("occ", "mean_acc", "var_acc"):
        assert np.abs(g_den[k] - g_one[k]).max() <= 1e-11 * np.abs(g_one[k]).max(), k
    post.close()


@functools.lru_cache(maxsize=None)
def _edge_case(n):
    """tests/acc_post_ref.py's bucket-edge construction (pdf 0 holds n entries) with the third entry of every pdf-2 frame negated: under
    scale 1 the numerator's pdf-0 bucket holds n entries, under scale -1 the denominator's"""
    m, gc, om, x = ref.edge_model()
    posts = [[[(t, -w if len(f) == 3 and k == 2 else w) for k, (t, w) in enumerate(f)] for f in p] for p in ref.bucket_edge_posts(n)]
    want = {s: ref2.oracle_post2(om, m.id2pdf, int(m.gauss_off[-1]), 40, m.num_tids, [x], posts, s) for s in (1.0, -1.0)}
    return posts, want


@pytest.mark.parametrize("scale", [1.0, -1.0])
@pytest.mark.parametrize("n", [1, 64, 65, 129])
def test_bucket_edges(ctx, n, scale):
    m, gc, om, x = ref.edge_model()
    posts, want = _edge_case(n)
    dm, tm, us, num, den = _device(ctx, m, gc, [0, len(x)], x)
    g_num, g_den = _run2(ctx, us, dm, tm, num, den, posts, scale=scale)
    ref.assert_stats(g_num, want[scale][0], ("edge num", n, scale))
    ref.assert_stats(g_den, want[scale][1], ("edge den", n, scale))
    a, b = int(m.gauss_off[0]), int(m.gauss_off[1])
    holder, other = (g_num, g_den) if scale > 0 else (g_den, g_num)
    assert holder["occ"][a:b].sum() > 0
    assert not other["occ"][a:b].any()                 # pdf 0 has entries of one sign only


def test_refusals(ctx):
    from kaldi_hmm_gmm_amd import DeviceAccs, DeviceModel, DevicePosteriors
    m, gc, ut, posts, _, _ = _weights_case(6, 7, 40, -0.5)
    dm, tm, us, num, den = _device(ctx, m, gc, ut.frame_off, ut.feats)
    before = _run2(ctx, us, dm, tm, num, den, posts)

    def refused(posts_, scale=1.0, model=dm, a=num, b=den, close=False, match=None):
        post = DevicePosteriors.from_posteriors(ctx, posts_)
        if close:
            post.close()
        with pytest.raises(Exception, match=match):
            us.acc_stats_post2(model, tm, post, a, b, scale=scale)
        post.close()
        for blk, was in zip((num.download(), den.download()), before):
            assert all(blk[k].tobytes() == was[k].tobytes() for k in KEYS) and blk["total_frames"] == was["total_frames"]

    refused(posts, a=num, b=num, match="same block")
    refused(posts, a=den, b=den, match="same block")
    short = [list(p) for p in posts]
    short[4] = short[4][:-1]
    refused(short, match="utterance 4")
    refused(posts[:-1])                              # another n_utt
    big = [list(p) for p in posts]
    big[2] = [list(f) for f in big[2]]
    big[2][1] = big[2][1] + [(m.num_tids + 1, -0.5)]
    refused(big)                                     # an id above num_tids
    refused(posts, scale=float("nan"), match="finite")
    refused(posts, close=True)                       # a closed handle
    m2, gc2, *_ = build(6, 7, 39, n_utt=1, seed=7, ragged=True, max_phones=2)
    dm2 = DeviceModel(ctx, m2.gauss_off, gc2, m2.means_invvars, m2.inv_vars)
    refused(posts, model=dm2, match="dimensions")
    other = DeviceAccs(ctx, dm2, tm)
    refused(posts, b=other, match="dimensions")      # a denominator block of another layout


@pytest.mark.parametrize("criterion", ["mpe", "smbr"])
def test_mpe_loop_on_the_yes_no_task(ctx, trained, criterion):  # noqa: F811
    """Three iterations of align (the reference and the ML block), rescore, mpe_posteriors(ali_set), acc_stats_post2,
    num.smooth_with_accum(tau, ml), ebw_update on 30 utterances: each iteration's device parameters are bit-equal to the host EBW form
    applied to the downloaded blocks, the occupancies of both blocks are non-negative, and the transition totals of the two blocks
    are the sums of the positive and of the negative weights.  sMBR also rises (the module's text has the decision)."""
    from kaldi_hmm_gmm_amd import mle as khg_mle
    khg_, dx, tm, am, graph, test_utts = trained
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_mmi_synthetic as mmi
    st = mmi.MmiState(ctx, tm, am, graph, test_utts[:30], kappa=0.1, criterion=criterion)
    crit = []
    for it in range(3):
        info = st.accumulate_mpe()
        num, den = st.num.download(), st.den.download()
        assert info["n_ok"] > 0 and info["pos_weight"] >= 0 and info["neg_weight"] >= 0
        assert (num["occ"] >= 0).all() and (den["occ"] >= 0).all()
        # a weight is rounded to float once (2^-24 relative) before it is counted
        for blk, tot in ((num, info["pos_weight"]), (den, info["neg_weight"])):
            assert abs(blk["trans_acc"].sum() - tot) <= 2.0 ** -23 * tot and abs(blk["total_frames"] - tot) <= 2.0 ** -23 * tot
            assert abs(blk["occ"].sum() - tot) <= 2e-5 * tot
        st.num.smooth_with_accum(st.tau, st.ml, st.dm, count=False)
        sm = st.num.download()
        before = st.dm.download()
        r = st.update()
        d = st.dm.download()
        h_w, h_gc, h_miv, h_iv, h_res = khg_mle._flat_ebw_update(
            st.opts, st.weight_opts, before["gauss_off"], (sm["occ"], sm["mean_acc"], sm["var_acc"]), (den["occ"], den["mean_acc"], den["var_acc"]), 0x7,
            before["weights"], before["means_invvars"], before["inv_vars"])
        np.testing.assert_array_equal(d["weights"], h_w)
        np.testing.assert_array_equal(d["inv_vars"], h_iv)
        np.testing.assert_array_equal(d["means_invvars"], h_miv)
        assert ebw_cases.ulps32(d["gconsts"], h_gc).max() <= GC_ULPS
        for k in ("floored", "failed", "skipped", "weights_skipped", "count"):
            assert r[k] == h_res[k], (k, r[k], h_res[k])
        assert r["failed"] == 0 and all(np.isfinite(d[k]).all() for k in ("weights", "gconsts", "means_invvars", "inv_vars"))
        crit.append(info["crit"])
        print("%s iteration %d: mean avg_acc / T = %.17g over %d utterances; weight +%.6f -%.6f; floored %d failed %d skipped %d"
              % (criterion, it, info["crit"], info["n_ok"], info["pos_weight"], info["neg_weight"], r["floored"], r["failed"], r["skipped"]))
    crit.append(st.accumulate_mpe(check=False)["crit"])
    print("%s criterion per iteration: %s" % (criterion, ["%.17g" % c for c in crit]))
    assert all(np.isfinite(crit)) and all(c > 0.0 for c in crit)
    if criterion == "smbr":
        margin = 10.0 * abs(C0_HOST_SMBR - crit[0])
        print("smbr c_0 host %.17g device %.17g margin %.3g rise %.3g" % (C0_HOST_SMBR, crit[0], margin, crit[-1] - crit[0]))
        assert crit[-1] > crit[0] + margin, (crit, margin)
    st.close()
