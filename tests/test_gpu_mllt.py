"""MLLT on the device: khg_acc_mllt_stats_post through UtteranceSet.acc_mllt_stats_post against the float64
restatement of tests/mllt_ref.py, the bits of the statistics across runs / calls / chunk sizes, gmm-transform-means on the handle
against the host form, and est-mllt end to end.

Tolerances: the project's own for K3's statistics, applied to each uncancelled term -- beta as occ (rtol 2e-5, atol 1e-6), G[d] rtol
2e-5 and atol 2e-6 x (the largest magnitude of the shifted S[d] + the largest magnitude of the shifted C[d])."""
import functools
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import acc_post_ref as apr  # noqa: E402
import fmllr_cases as fcases  # noqa: E402
import mllt_cases as cases  # noqa: E402
import mllt_ref as ref  # noqa: E402
from helpers import build  # noqa: E402
from test_gpu_lattice_faster_raw import trained  # noqa: E402,F401

pytestmark = pytest.mark.gpu
SLICE = fcases.SLICE


def _device(ctx, m, gc, feats):
    from kaldi_hmm_gmm_amd import DeviceModel, DeviceTransitions, UtteranceSet
    dm = DeviceModel(ctx, m.gauss_off, gc, m.means_invvars, m.inv_vars, m.weights)
    tm = DeviceTransitions(ctx, m.id2pdf)
    fo = np.concatenate([[0], np.cumsum([len(f) for f in feats])]).astype(np.int64)
    D = m.means_invvars.shape[1]
    x = np.ascontiguousarray(np.concatenate(feats), np.float32) if fo[-1] else np.zeros((0, D), np.float32)
    return dm, tm, UtteranceSet(ctx, None, fo, x)


def _acc(ctx, dev, posts, scale=1.0, chunk=None, stats=None, download=True):
    from kaldi_hmm_gmm_amd import DeviceMlltStats, DevicePosteriors
    dm, tm, us = dev
    if stats is None:
        stats = DeviceMlltStats(ctx, us.dim)
    if chunk is not None:
        stats.set_chunk_frames(chunk)
    post = DevicePosteriors.from_posteriors(ctx, posts)
    us.acc_mllt_stats_post(dm, tm, post, stats, scale=scale)
    got = stats.download() if download else None
    post.close()
    return got, stats


def _assert_stats(got, want, what):
    np.testing.assert_allclose(got["beta"], want["beta"], rtol=2e-5, atol=1e-6, err_msg=str(what))
    worst = 0.0
    for d in range(want["G"].shape[0]):
        atol = 2e-6 * (np.abs(want["S"][d]).max() + np.abs(want["C"][d]).max())
        worst = max(worst, float((np.abs(got["G"][d] - want["G"][d]) / (atol + 2e-5 * np.abs(want["G"][d]))).max()))
    print("%s: beta %.6f (want %.6f), largest error / tolerance of G %.3g" % (what, got["beta"], want["beta"], worst))
    for d in range(want["G"].shape[0]):
        atol = 2e-6 * (np.abs(want["S"][d]).max() + np.abs(want["C"][d]).max())
        np.testing.assert_allclose(got["G"][d], want["G"][d], rtol=2e-5, atol=atol, err_msg="%s G[%d]" % (what, d))


def _same_bits(a, b, what):
    assert np.float64(a["beta"]).tobytes() == np.float64(b["beta"]).tobytes(), (what, a["beta"], b["beta"])
    assert a["G"].tobytes() == b["G"].tobytes(), (what, np.abs(a["G"] - b["G"]).max())


# ---- statistics against the float64 restatement -------------------------------------------------------------------------------------
SHAPES = [(6, 1, 13), (6, 7, 40), (4, 65, 40), (3, 2, 1), (3, 4, 80), (3, 100, 80)]       # the last: a pdf staged in two tiles of Gaussians
LENS = [23, 40, 17, 31, 1, 25, 64, 19, 30, 65]


@functools.lru_cache(maxsize=None)
def _shape_case(P, G, D, off=0.0):
    m, gc, om, ut, _ = build(P, G, D, n_utt=1, seed=P + G + D, max_phones=2)
    if off:
        m, gc = cases.offset_model(m, off)
    feats, pdfs = cases.mixed_set(m, LENS, G + D, D)
    posts = apr.random_posts(pdfs, m.id2pdf, seed=P + D)        # 0 .. 5 entries per frame, two ids of one pdf on a frame among them
    posts[8] = []                                               # an utterance without frames in the handle
    assert any(len(f) == 0 for p in posts for f in p) and any(len(f) == 5 for p in posts for f in p)
    assert any(len({int(m.id2pdf[t]) for t, _ in f}) < len(f) for p in posts for f in p)
    want = ref.acc_stats(m, gc, feats, posts, dtype=np.float64)
    return m, gc, feats, pdfs, posts, want


@pytest.mark.parametrize("P,G,D", SHAPES)
def test_statistics_against_the_restatement(ctx, P, G, D):
    m, gc, feats, pdfs, posts, want = _shape_case(P, G, D)
    dev = _device(ctx, m, gc, feats)
    got, stats = _acc(ctx, dev, posts)
    _assert_stats(got, want, (P, G, D))
    assert want["beta"] > 0
    twice, _ = _acc(ctx, dev, posts, stats=stats)               # a second call adds: twice the statistics, exactly (x + x)
    assert twice["beta"] == 2.0 * got["beta"] and (twice["G"] == 2.0 * got["G"]).all()


def test_features_and_means_offset_by_50(ctx):
    m, gc, feats, pdfs, posts, want = _shape_case(6, 7, 40, 50.0)
    assert np.abs(np.concatenate(feats)).mean() > 40 and np.abs(want["c"]).min() > 40
    got, _ = _acc(ctx, _device(ctx, m, gc, feats), posts)
    _assert_stats(got, want, "offset 50")


@pytest.mark.parametrize("scale", [1.0, -0.5])
def test_negative_zero_and_tiny_weights(ctx, scale):
    m, gc, feats, pdfs, posts, _ = _shape_case(6, 7, 40)
    special = [-0.7, 1e-30, 0.0, 3.5]
    # (on entries of the frame's own pdf, as tests/test_gpu_acc_stats_post.py: the others keep their small weights)
    posts = [[[(t, special[(u + i + k) % 7] if (u + i + k) % 7 < 4 and m.id2pdf[t] == pdfs[u][i] else w) for k, (t, w) in enumerate(f)]
              for i, f in enumerate(p)] for u, p in enumerate(posts)]
    flat = [w for p in posts for f in p for _, w in f]
    assert all(flat.count(s) > 5 for s in special)
    want = ref.acc_stats(m, gc, feats, posts, scale=scale, dtype=np.float64)
    got, _ = _acc(ctx, _device(ctx, m, gc, feats), posts, scale=scale)
    _assert_stats(got, want, ("weights", scale))


def _split(T):
    """T frames over three utterances (one when T < 3)"""
    return [T] if T < 3 else [T // 3, T // 2 - T // 3, T - T // 2]


@functools.lru_cache(maxsize=None)
def _frames_case(T):
    m, gc, om, ut, _ = build(6, 1, 13, n_utt=1, seed=2, max_phones=2)
    feats, pdfs = cases.mixed_set(m, _split(T), 31 + T, 13)
    posts = fcases.ali_posts(m, pdfs, seed=8)
    return m, gc, feats, posts, ref.acc_stats(m, gc, feats, posts, dtype=np.float64)


@pytest.mark.parametrize("T", [1, SLICE - 1, SLICE, SLICE + 1, 3 * SLICE + 5])
def test_frame_counts_around_the_slice(ctx, T):
    m, gc, feats, posts, want = _frames_case(T)
    got, _ = _acc(ctx, _device(ctx, m, gc, feats), posts)
    assert int(round(got["beta"])) == T
    _assert_stats(got, want, "%d frames" % T)


# (K3's any-size form, which makes occ_g / m_g here, stages a pdf's posteriors in LDS: pdfs of up to 595 Gaussians at D <= 40)
GAUSS_COUNTS = {1: [1], 1023: [500, 23, 500], 1024: [500, 24, 500], 1025: [1, 512, 512], 2053: [500, 53, 500, 500, 500]}


@functools.lru_cache(maxsize=None)
def _gauss_case(total):
    from kaldi_hmm_gmm_amd import synth
    from oracle import oracle as orc
    counts = GAUSS_COUNTS[total]
    m = synth.make_model(len(counts), 1, 13, seed=20230414 + total, gauss_counts=counts)
    assert int(m.gauss_off[-1]) == total
    gc = orc.model_gconsts(m.gauss_off, m.weights, m.inv_vars, m.means_invvars)
    feats, pdfs = cases.mixed_set(m, [90, 1, 110], 5 + total, 13)
    posts = fcases.ali_posts(m, pdfs, seed=total)
    return m, gc, feats, posts, ref.acc_stats(m, gc, feats, posts, dtype=np.float64)


@pytest.mark.parametrize("total", sorted(GAUSS_COUNTS))
def test_gaussian_counts_around_the_slice(ctx, total):
    """models of 1, 1023, 1024, 1025 and 2053 Gaussians with uneven pdfs: the Gaussian side's 1024-Gaussian slice edges are crossed"""
    m, gc, feats, posts, want = _gauss_case(total)
    got, _ = _acc(ctx, _device(ctx, m, gc, feats), posts)
    _assert_stats(got, want, "%d Gaussians" % total)


# ---- bits -----------------------------------------------------------------------------------------------------------------------
LONG_LENS = [1, SLICE - 1, SLICE, 700, SLICE + 1, 2 * SLICE, SLICE + 5 - 700]


@functools.lru_cache(maxsize=None)
def _long_case():
    m, gc, om, ut, _ = build(6, 3, 13, n_utt=1, seed=2, max_phones=2)
    feats, pdfs = cases.mixed_set(m, LONG_LENS, 31, 13)
    return m, gc, feats, fcases.ali_posts(m, pdfs, seed=8)


def test_bits_from_run_to_run_chunks_and_order(ctx):
    m, gc, feats, posts = _long_case()
    dev = _device(ctx, m, gc, feats)
    whole, s1 = _acc(ctx, dev, posts)
    again, _ = _acc(ctx, dev, posts)
    _same_bits(whole, again, "two runs")
    assert s1.num_chunks() == 1
    many, s2 = _acc(ctx, dev, posts, chunk=SLICE)                    # the scratch bound forced low: chunks of one slice
    assert s2.num_chunks() >= 2
    _same_bits(whole, many, "chunks")
    # the utterances permuted: another frame order, other sums, the same statistics within fp64 rounding of the uncancelled terms ...
    perm = [3, 0, 6, 2, 5, 1, 4]
    moved, _ = _acc(ctx, _device(ctx, m, gc, [feats[u] for u in perm]), [posts[u] for u in perm])
    np.testing.assert_allclose(moved["G"], whole["G"], rtol=0, atol=1e-9 * np.abs(whole["G"]).max())
    # ... and permuted back, in a fresh set: the same bits
    inv = np.argsort(perm)
    back, _ = _acc(ctx, _device(ctx, m, gc, [feats[perm[i]] for i in inv]), [posts[perm[i]] for i in inv])
    _same_bits(whole, back, "permuted back")


# One pdf with most of the entries, as silence in a real alignment.  khg_acc_stats_post on its own cuts a bucket of more than twice
# max(512, 2 x the average bucket) entries into three or more work items, whose closing fp64 atomics land in whatever order the items
# finish; the MLLT call must not.  30 pdfs, 12000 frames, 80 % of them on pdf 0: the average bucket is 400, pdf 0's is
# ~9700, twelve items' worth.  Narrow pdfs go through K3's chunk-per-block MFMA form, a 300-Gaussian pdf through its VALU form, which
# flushes after every chunk.
SKEW_LENS = [5000, 1, 4000, 2999]


@functools.lru_cache(maxsize=None)
def _skew_case(wide):
    from kaldi_hmm_gmm_amd import synth
    from oracle import oracle as orc
    if wide:
        m = synth.make_model(30, 1, 13, seed=20230415, gauss_counts=[300] + [2] * 29)
        gc = orc.model_gconsts(m.gauss_off, m.weights, m.inv_vars, m.means_invvars)
    else:
        m, gc, om, ut, _ = build(30, 3, 13, n_utt=1, seed=4, max_phones=2)
    feats, pdfs = cases.skewed_set(m, SKEW_LENS, 77, 13)
    n0, N = sum(int((p == 0).sum()) for p in pdfs), sum(SKEW_LENS)
    assert n0 > 4 * 2 * max(512, 2 * (N // 30)) and n0 > 16 * (N // 30)      # well over four times the average, and over four K3 targets
    return m, gc, feats, fcases.ali_posts(m, pdfs, seed=9)


@pytest.mark.parametrize("wide", [False, True])
def test_bits_with_one_pdf_far_above_the_average_bucket(ctx, wide):
    m, gc, feats, posts = _skew_case(wide)
    dev = _device(ctx, m, gc, feats)
    first, s1 = _acc(ctx, dev, posts)
    assert int(round(first["beta"])) == sum(SKEW_LENS)
    for run in range(3):
        _same_bits(first, _acc(ctx, dev, posts)[0], "skewed, run %d" % run)
    _same_bits(first, _acc(ctx, dev, posts, chunk=SLICE)[0], "skewed, chunks of one slice")
    if not wide:                                                     # (the restatement walks Gaussians in Python: the narrow model only)
        _assert_stats(first, ref.acc_stats(m, gc, feats, posts, dtype=np.float64), "skewed")


def test_a_pdf_too_wide_for_the_statistics_pass_is_refused_up_front(ctx):
    """khg_acc_stats_post's any-size form ends at 595 Gaussians per pdf (D <= 40); the MLLT call says so before it launches anything"""
    from kaldi_hmm_gmm_amd import DevicePosteriors, synth
    from oracle import oracle as orc
    m = synth.make_model(2, 1, 13, seed=3, gauss_counts=[600, 2])
    gc = orc.model_gconsts(m.gauss_off, m.weights, m.inv_vars, m.means_invvars)
    feats, pdfs = fcases.draw_set(m, [20, 9], seed=1)
    dm, tm, us = dev = _device(ctx, m, gc, feats)
    from kaldi_hmm_gmm_amd import DeviceMlltStats
    stats = DeviceMlltStats(ctx, 13)
    seeded = {"beta": 3.0, "G": np.arange(13 * 91, dtype=np.float64).reshape(13, 91)}
    stats.upload(seeded["beta"], seeded["G"])
    post = DevicePosteriors.from_posteriors(ctx, fcases.ali_posts(m, pdfs, seed=2))
    with pytest.raises(Exception, match="600 Gaussians"):
        us.acc_mllt_stats_post(dm, tm, post, stats)
    post.close()
    _same_bits(stats.download(), seeded, "refused: too wide")


def test_bits_two_calls_equal_the_sum_of_two_handles(ctx):
    m, gc, feats, posts = _long_case()
    dev = _device(ctx, m, gc, feats)
    first = [p if u < 4 else [] for u, p in enumerate(posts)]
    second = [p if u >= 4 else [] for u, p in enumerate(posts)]
    _, both = _acc(ctx, dev, first, download=False)
    two_calls, _ = _acc(ctx, dev, second, stats=both)
    _, a = _acc(ctx, dev, first, download=False)
    _, b = _acc(ctx, dev, second, download=False)
    a.add(1.0, b)
    _same_bits(two_calls, a.download(), "two calls against add")
    c = type(a)(ctx, 13)                                             # upload(download()) round-trips; zero() clears
    d = a.download()
    c.upload(d["beta"], d["G"])
    _same_bits(c.download(), d, "upload")
    c.zero()
    z = c.download()
    assert z["beta"] == 0.0 and not z["G"].any()
    with pytest.raises(Exception, match="same handle"):
        a.add(1.0, a)


def test_refusals_leave_the_bits(ctx):
    from kaldi_hmm_gmm_amd import DeviceMlltStats, DevicePosteriors
    m, gc, feats, pdfs, posts, _ = _shape_case(6, 1, 13)
    dev = _device(ctx, m, gc, feats)
    dm, tm, us = dev
    before, stats = _acc(ctx, dev, posts)

    def refused(posts_=posts, scale=1.0, st=stats, match=None):
        post = DevicePosteriors.from_posteriors(ctx, posts_)
        with pytest.raises(Exception, match=match):
            us.acc_mllt_stats_post(dm, tm, post, st, scale=scale)
        post.close()
        _same_bits(stats.download(), before, "refused")

    refused(st=DeviceMlltStats(ctx, 12), match="dimension")
    short = [list(p) for p in posts]
    short[3] = short[3][:-1]
    refused(posts_=short, match="utterance 3")
    refused(posts_=posts[:-1])
    refused(scale=float("inf"), match="finite")
    big = [list(p) for p in posts]
    big[2] = [list(f) for f in big[2]]
    big[2][1] = big[2][1] + [(m.num_tids + 1, 0.5)]
    refused(posts_=big, match="transition-id")
    with pytest.raises(Exception):
        DeviceMlltStats(ctx, 81)
    again, _ = _acc(ctx, dev, posts, stats=stats)                    # and the handle still accumulates
    assert again["beta"] == 2.0 * before["beta"]


# ---- gmm-transform-means ------------------------------------------------------------------------------------------------------------
def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max()


@pytest.mark.parametrize("D", [1, 13, 40, 80])
def test_transform_means_against_the_host_form(ctx, D):
    import kaldi_hmm_gmm_amd as khg
    m, gc, om, ut, _ = build(5, 7, D, n_utt=1, seed=D, max_phones=2, ragged=True)
    M = (np.eye(D) + 0.3 * np.random.default_rng(D).standard_normal((D, D)) / np.sqrt(D)).astype(np.float32)
    feats, _ = fcases.draw_set(m, [65, 1, 130], seed=D)
    dm, tm, us = _device(ctx, m, gc, feats)
    am = cases.host_am(m)
    khg.gmm_transform_means(M, model=dm, am_gmm=am)
    d = dm.download()
    go, hgc, hw, hmiv, hiv = am.flat()
    assert np.asarray(d["weights"]).tobytes() == np.asarray(hw).tobytes() == m.weights.tobytes()
    assert np.asarray(d["inv_vars"]).tobytes() == np.asarray(hiv).tobytes() == m.inv_vars.tobytes()
    assert np.asarray(d["means_invvars"]).tobytes() == np.asarray(hmiv).tobytes() == ref.transform_means(m.means_invvars, m.inv_vars, M).tobytes()
    assert np.asarray(d["means_invvars"]).tobytes() != m.means_invvars.tobytes()
    assert _ulps(d["gconsts"], hgc) <= 4                               # logf on the device and in glibc
    # the transformed model on the transformed rows: the handle rewritten in place scores as a fresh upload of the same parameters
    pdfs = np.arange(5, dtype=np.int32)
    W = np.concatenate([M, np.zeros((D, 1), np.float32)], 1)
    khg.transform_feats_batch(us, np.zeros(3, np.int32), W[None])
    us.set_pdf_list(pdfs)
    us.loglikes(dm)

    def lls(u):
        return np.concatenate([np.ravel(a) for a in u.download_loglikes()])
    m2 = types.SimpleNamespace(gauss_off=m.gauss_off, means_invvars=np.asarray(d["means_invvars"]), inv_vars=m.inv_vars, weights=m.weights, id2pdf=m.id2pdf)
    _, _, us2 = dev2 = _device(ctx, m2, np.asarray(d["gconsts"]), [khg.transform_feats(f, W) for f in feats])
    us2.set_pdf_list(pdfs)
    us2.loglikes(dev2[0])
    assert lls(us).tobytes() == lls(us2).tobytes()
    with pytest.raises(Exception):
        dm.transform_means(M[:, :-1] if D > 1 else np.zeros((2, 2), np.float32))
    bare = khg.DeviceModel(ctx, m.gauss_off, gc, m.means_invvars, m.inv_vars)
    with pytest.raises(Exception, match="weights"):
        bare.transform_means(M)


# ---- end to end on the trained YES / NO model ----------------------------------------------------------------------------------------
def test_trained_model_mixed_features_end_to_end(trained):
    """The test utterances mixed by one fixed matrix; decode -> lattice posteriors -> gmm-acc-mllt -> est-mllt.  The statistics are held
    to the restatement; the status is OK and objf_impr > 0; the gain in the posterior-weighted likelihood of the transformed
    features under the transformed means plus sum(w) log |det M| is at least objf_impr (EM), slack 1e-6 of the gain (the likelihoods
    here are float64)."""
    khg, dx, tmh, am, graph, test_utts = trained
    from kaldi_hmm_gmm_amd import DeviceModel, DeviceTransitions, UtteranceSet, _gpu
    dctx = _gpu.default_context()
    raw = [np.ascontiguousarray(u[2], np.float32) for u in test_utts]
    D = raw[0].shape[1]
    R = cases.mixing(D, seed=17, strength=0.2)
    feats = [np.ascontiguousarray(f.astype(np.float64) @ R.T, np.float32) for f in raw]
    cfg = khg.LatticeFasterDecoderConfig(max_active=7000, beam=13.0, lattice_beam=6.0)
    res, dl = khg.get_raw_lattice_faster_device_batch(am, tmh, graph, feats, cfg, 0.1)
    P = dl.posteriors(1.0, 0.1)
    posts = P.download()
    go, gc, w, miv, iv = am.flat()
    id2pdf = np.asarray(tmh.transition_id_to_pdf_array(), np.int32)
    m = types.SimpleNamespace(gauss_off=np.asarray(go, np.int32), means_invvars=np.asarray(miv, np.float32), inv_vars=np.asarray(iv, np.float32),
                              weights=np.asarray(w, np.float32), id2pdf=id2pdf)
    gc = np.asarray(gc, np.float32)
    dm, dt = DeviceModel(dctx, go, gc, miv, iv, w), DeviceTransitions(dctx, id2pdf)
    fo = np.concatenate([[0], np.cumsum([len(f) for f in feats])]).astype(np.int64)
    us = UtteranceSet(dctx, None, fo, np.ascontiguousarray(np.concatenate(feats)))
    r = khg.gmm_acc_mllt(dm, dt, us, P)
    _assert_stats(r, ref.acc_stats(m, gc, feats, posts, dtype=np.float64), "trained")
    est = khg.est_mllt(r["stats"])
    assert est["status"] == khg.MLLT_OK and est["objf_impr"] > 0 and est["count"] == r["beta"]
    M = est["M"].astype(np.float64)
    logdet = np.linalg.slogdet(M)[1]
    mu, iv64, w64 = ref.means(m).astype(np.float64), m.inv_vars.astype(np.float64), m.weights.astype(np.float64)
    gain = 0.0
    for u, post in enumerate(posts):
        x = feats[u].astype(np.float64)
        y = x @ M.T
        for t, f in enumerate(post):
            for tid, wt in f:
                p = int(id2pdf[tid])
                g0, g1 = int(go[p]), int(go[p + 1])
                gain += wt * (ref.loglike64(w64[g0:g1], mu[g0:g1] @ M.T, iv64[g0:g1], y[t:t + 1])[0]
                              - ref.loglike64(w64[g0:g1], mu[g0:g1], iv64[g0:g1], x[t:t + 1])[0] + logdet)
    print("likelihood gain %.4f, objf_impr %.4f over %.1f frames" % (gain, est["objf_impr"], est["count"]))
    assert gain >= est["objf_impr"] - 1e-6 * abs(gain)
    # gmm-transform-means and transform-feats go through on the trained handles
    khg.gmm_transform_means(est["M"], model=dm)
    khg.transform_feats_batch(us, np.zeros(len(feats), np.int32), est["W"][None])
    P.close(); dl.close(); us.close()
