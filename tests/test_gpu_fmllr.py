"""fMLLR on the device: khg_acc_fmllr_stats_post through UtteranceSet.acc_fmllr_stats_post against the float64
restatement of tests/fmllr_ref.py, the bits of the statistics across batches / runs / calls / chunk sizes, transform-feats against the
fmaf chain, and gmm-est-fmllr end to end.

Tolerances: the project's own for K3's statistics -- beta as occ (rtol 2e-5, atol 1e-6), K and G rtol 2e-5 and atol 2e-6 x the
largest magnitude of the speaker's block."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import acc_post_ref as apr  # noqa: E402
import fmllr_cases as cases  # noqa: E402
import fmllr_ref as ref  # noqa: E402
from helpers import build  # noqa: E402
from test_gpu_lattice_faster_raw import trained  # noqa: E402,F401

pytestmark = pytest.mark.gpu
SLICE = cases.SLICE


def _device(ctx, m, gc, feats):
    from kaldi_hmm_gmm_amd import DeviceModel, DeviceTransitions, UtteranceSet
    dm = DeviceModel(ctx, m.gauss_off, gc, m.means_invvars, m.inv_vars)
    tm = DeviceTransitions(ctx, m.id2pdf)
    fo = np.concatenate([[0], np.cumsum([len(f) for f in feats])]).astype(np.int64)
    D = m.means_invvars.shape[1]
    x = np.ascontiguousarray(np.concatenate(feats), np.float32) if fo[-1] else np.zeros((0, D), np.float32)
    return dm, tm, UtteranceSet(ctx, None, fo, x)


def _acc(ctx, dev, posts, utt2spk, n_spk, scale=1.0, chunk=None, stats=None, download=True):
    from kaldi_hmm_gmm_amd import DeviceFmllrStats, DevicePosteriors
    dm, tm, us = dev
    if stats is None:
        stats = DeviceFmllrStats(ctx, n_spk, us.dim)
    if chunk is not None:
        stats.set_chunk_frames(chunk)
    post = DevicePosteriors.from_posteriors(ctx, posts)
    us.acc_fmllr_stats_post(dm, tm, post, np.asarray(utt2spk, np.int32), stats, scale=scale)
    got = stats.download() if download else None
    post.close()
    return got, stats


def _assert_stats(got, want, what):
    beta, K, G = want
    np.testing.assert_allclose(got["beta"], beta, rtol=2e-5, atol=1e-6, err_msg=str(what))
    for s in range(len(beta)):
        for name, w in (("K", K[s]), ("G", G[s])):
            np.testing.assert_allclose(got[name][s], w, rtol=2e-5, atol=2e-6 * max(np.abs(w).max(), 1e-30), err_msg="%s %s speaker %d" % (what, name, s))


def _same_bits(a, b, what, speakers=None):
    for k in ("beta", "K", "G"):
        x, y = (a[k], b[k]) if speakers is None else (a[k][speakers[0]], b[k][speakers[1]])
        assert x.tobytes() == y.tobytes(), (what, k, np.abs(x - y).max())


# ---- statistics against the float64 restatement -------------------------------------------------------------------------------------
SHAPES = [(6, 1, 13), (6, 7, 40), (4, 65, 40), (3, 100, 39), (3, 2, 1), (3, 4, 80), (3, 100, 80)]       # the last: a pdf staged in two tiles of Gaussians
# utterance -> speaker: three speakers interleaved, utterance 5 belongs to nobody, speaker 3 has no utterance, speaker 4's only
# utterance has no frames in the handle (what a failed utterance leaves)
U2S = np.array([0, 1, 2, 0, 1, -1, 2, 0, 4, 1], np.int32)
LENS = [23, 40, 17, 31, 1, 25, 64, 19, 30, 65]
N_SPK = 5


@functools.lru_cache(maxsize=None)
def _shape_case(P, G, D):
    m, gc, om, ut, _ = build(P, G, D, n_utt=1, seed=P + G + D, max_phones=2)
    feats, pdfs = cases.draw_set(m, LENS, seed=G + D)
    posts = apr.random_posts(pdfs, m.id2pdf, seed=P + D)        # 0 .. 5 entries per frame, two ids of one pdf on a frame among them
    posts[8] = []
    assert any(len(f) == 0 for p in posts for f in p) and any(len(f) == 5 for p in posts for f in p)
    assert any(len({int(m.id2pdf[t]) for t, _ in f}) < len(f) for p in posts for f in p)
    want = cases.freeze(*ref.acc_stats(m, gc, feats, posts, U2S, N_SPK, dtype=np.float64))
    return m, gc, feats, pdfs, posts, want


@pytest.mark.parametrize("P,G,D", SHAPES)
def test_statistics_against_the_restatement(ctx, P, G, D):
    m, gc, feats, pdfs, posts, want = _shape_case(P, G, D)
    dev = _device(ctx, m, gc, feats)
    got, stats = _acc(ctx, dev, posts, U2S, N_SPK)
    _assert_stats(got, want, (P, G, D))
    for s in (3, 4):                                             # no utterance / no frames in the handle: untouched
        assert got["beta"][s] == 0 and not got["K"][s].any() and not got["G"][s].any()
    assert want[0][:3].min() > 0
    # a second call adds: twice the statistics, exactly (x + x)
    twice, _ = _acc(ctx, dev, posts, U2S, N_SPK, stats=stats)
    for k in ("beta", "K", "G"):
        assert (twice[k] == 2.0 * got[k]).all(), k


# frames per speaker: 1, one slice - 1, one slice, one slice + 1, three slices + 5 (the last over three utterances)
LONG_LENS = [1, SLICE - 1, SLICE, 700, SLICE + 1, 2 * SLICE, SLICE + 5 - 700]
LONG_U2S = np.array([0, 1, 2, 4, 3, 4, 4], np.int32)


@functools.lru_cache(maxsize=None)
def _long_case():
    m, gc, om, ut, _ = build(6, 1, 13, n_utt=1, seed=2, max_phones=2)
    feats, pdfs = cases.draw_set(m, LONG_LENS, seed=31)
    posts = cases.ali_posts(m, pdfs, seed=8)
    want = cases.freeze(*ref.acc_stats(m, gc, feats, posts, LONG_U2S, 5, dtype=np.float64))
    return m, gc, feats, posts, want


def test_frame_counts_around_the_slice(ctx):
    m, gc, feats, posts, want = _long_case()
    got, stats = _acc(ctx, _device(ctx, m, gc, feats), posts, LONG_U2S, 5)
    assert [int(round(b)) for b in got["beta"]] == [1, SLICE - 1, SLICE, SLICE + 1, 3 * SLICE + 5]
    _assert_stats(got, want, "long")


@pytest.mark.parametrize("scale", [1.0, -0.5])
def test_negative_and_zero_weights(ctx, scale):
    m, gc, feats, pdfs, posts, _ = _shape_case(6, 7, 40)
    special = [-0.7, 1e-30, 0.0, 3.5]
    # (on entries of the frame's own pdf, as tests/test_gpu_acc_stats_post.py: the others keep their small weights)
    posts = [[[(t, special[(u + i + k) % 7] if (u + i + k) % 7 < 4 and m.id2pdf[t] == pdfs[u][i] else w) for k, (t, w) in enumerate(f)]
              for i, f in enumerate(p)] for u, p in enumerate(posts)]
    flat = [w for p in posts for f in p for _, w in f]
    assert all(flat.count(s) > 5 for s in special)
    want = ref.acc_stats(m, gc, feats, posts, U2S, N_SPK, scale=scale, dtype=np.float64)
    got, _ = _acc(ctx, _device(ctx, m, gc, feats), posts, U2S, N_SPK, scale=scale)
    _assert_stats(got, want, ("weights", scale))


# ---- bits -----------------------------------------------------------------------------------------------------------------------
def test_bits_alone_in_a_batch_and_from_run_to_run(ctx):
    m, gc, feats, posts, _ = _long_case()
    dev = _device(ctx, m, gc, feats)
    whole, _ = _acc(ctx, dev, posts, LONG_U2S, 5)
    again, _ = _acc(ctx, dev, posts, LONG_U2S, 5)
    _same_bits(whole, again, "two runs")
    # speaker 4 alone (every other utterance belongs to nobody), and alone in a set of its own utterances, as speaker 0
    alone, _ = _acc(ctx, dev, posts, np.where(LONG_U2S == 4, 4, -1), 5)
    _same_bits(alone, whole, "alone in the call", speakers=(4, 4))
    own = [u for u in range(len(LONG_U2S)) if LONG_U2S[u] == 4]
    dev2 = _device(ctx, m, gc, [feats[u] for u in own])
    solo, _ = _acc(ctx, dev2, [posts[u] for u in own], np.zeros(len(own), np.int32), 1)
    _same_bits(solo, whole, "alone in a set", speakers=(0, 4))
    # ... and in a batch of three, under other numbers
    three, _ = _acc(ctx, dev, posts, np.array([-1, 2, -1, 0, 1, 0, 0], np.int32), 3)
    _same_bits(three, whole, "a batch of three", speakers=(0, 4))
    _same_bits(three, whole, "a batch of three", speakers=(2, 1))


def test_bits_two_calls_equal_the_sum_of_two_handles(ctx):
    m, gc, feats, posts, _ = _long_case()
    dev = _device(ctx, m, gc, feats)
    first = [p if u < 4 else [] for u, p in enumerate(posts)]
    second = [p if u >= 4 else [] for u, p in enumerate(posts)]
    _, both = _acc(ctx, dev, first, LONG_U2S, 5, download=False)
    two_calls, _ = _acc(ctx, dev, second, LONG_U2S, 5, stats=both)
    _, a = _acc(ctx, dev, first, LONG_U2S, 5, download=False)
    _, b = _acc(ctx, dev, second, LONG_U2S, 5, download=False)
    a.add(1.0, b)
    _same_bits(two_calls, a.download(), "two calls against add")
    # upload(download()) round-trips
    c = type(a)(ctx, 5, 13)
    d = a.download()
    c.upload(d["beta"], d["K"], d["G"])
    _same_bits(c.download(), d, "upload")
    with pytest.raises(Exception, match="same handle"):
        a.add(1.0, a)


def test_bits_do_not_depend_on_the_chunk(ctx):
    m, gc, feats, posts, _ = _long_case()
    dev = _device(ctx, m, gc, feats)
    one, s1 = _acc(ctx, dev, posts, LONG_U2S, 5)
    assert s1.num_chunks() == 1
    many, s2 = _acc(ctx, dev, posts, LONG_U2S, 5, chunk=SLICE)       # the scratch bound forced low: two slices per chunk
    assert s2.num_chunks() >= 2
    _same_bits(one, many, "chunks")


# ---- estimate -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,G,D,T,iters", [(5, 3, 5, 400, 40), (3, 7, 13, 800, 40), (3, 7, 40, 1500, 3), (3, 2, 64, 400, 1)])
def test_device_estimate_equals_the_host_form_on_the_bits(ctx, P, G, D, T, iters):
    """khg_fmllr_stats_estimate against khg_fmllr_compute on the downloaded statistics: W (narrowed: the device form gives floats),
    statuses and counts on the bits, objf_impr to the rounding of log.  Condition: the restatement's smallest relative gap of the
    two roots over all row updates is >= 1e-6 (tests/test_fmllr_cpu.py), computed here by the restatement on the downloaded
    statistics.  D <= 40 keeps A^T and its inverse in LDS, D = 64 in HBM scratch."""
    import kaldi_hmm_gmm_amd as khg
    c = cases.estimate_case(P, G, D, T)
    dev = _device(ctx, c["m"], c["gc"], c["feats"])
    # one more speaker than the case has: no utterance, beta = 0, LOW_COUNT
    got, stats = _acc(ctx, dev, c["posts"], c["utt2spk"], c["n_spk"] + 1)
    host = khg.fmllr_compute(got["beta"], got["K"], got["G"], min_count=50.0, num_iters=iters)
    devr = stats.estimate(min_count=50.0, num_iters=iters)
    for s in range(c["n_spk"]):
        assert ref.estimate(got["beta"][s], got["K"][s], got["G"][s], min_count=50.0, num_iters=iters)["gap"] >= 1e-6
    assert (host["status"] == [0] * c["n_spk"] + [khg.FMLLR_LOW_COUNT]).all()
    assert (devr["status"] == host["status"]).all() and devr["count"].tobytes() == host["count"].tobytes()
    assert devr["W"].tobytes() == host["W"].tobytes()
    np.testing.assert_allclose(devr["objf_impr"], host["objf_impr"], rtol=1e-10, atol=1e-8)
    # the transforms resident in a caller's buffer: the same floats
    import torch
    Wd = torch.zeros(host["W"].shape, dtype=torch.float32, device="cuda:%d" % ctx.device)
    stats.estimate(min_count=50.0, num_iters=iters, W_d=Wd.data_ptr())
    assert Wd.cpu().numpy().tobytes() == host["W"].tobytes()


def test_device_estimate_singular(ctx):
    """fewer frames than D + 1 with a count above min_count: integer data keep the elimination exact, the fourth pivot is 0"""
    import kaldi_hmm_gmm_amd as khg
    D = 5
    xs = np.array([[1, 2, 0, 1, 2, 1], [2, 1, 1, 0, 1, 1], [0, 1, 2, 2, 1, 1]], np.float64)
    il, jl = np.tril_indices(D + 1)
    G1 = np.stack([(xs.T @ xs)[il, jl]] * D)[None]
    st = khg.DeviceFmllrStats(ctx, 1, D)
    st.upload(np.array([600.0]), np.ones((1, D, D + 1)), G1)
    r = st.estimate()
    ident = np.concatenate([np.eye(D), np.zeros((D, 1))], 1).astype(np.float32)
    assert r["status"][0] == khg.FMLLR_SINGULAR and (r["W"][0] == ident).all() and r["count"][0] == 600.0 and r["objf_impr"][0] == 0.0


# ---- from_alignment -------------------------------------------------------------------------------------------------------------
def test_from_alignment_against_ali_to_post(ctx):
    """DevicePosteriors.from_alignment on a set whose resident alignment has a failed utterance (ids 0, as khg_align leaves one):
    the download equals ali-to-post through from_arrays with no frames for that utterance, and so do the statistics"""
    from kaldi_hmm_gmm_amd import DevicePosteriors, DeviceFmllrStats
    m, gc, feats, pdfs, posts, _ = _shape_case(6, 7, 40)
    dm, tm, us = dev = _device(ctx, m, gc, feats)
    ali = [np.array([f[0][0] if f else 1 for f in p], np.int32) for p in cases.ali_posts(m, pdfs, seed=3)]
    ali[4] = np.zeros_like(ali[4])                                   # a failed utterance
    ali[6] = np.zeros_like(ali[6])
    with pytest.raises(Exception, match="alignment"):
        DevicePosteriors.from_alignment(us)                          # nothing resident yet
    us.upload_ali(np.concatenate(ali))
    P = DevicePosteriors.from_alignment(us)
    want_posts = [[] if u in (4, 6) else [[(int(t), 1.0)] for t in a] for u, a in enumerate(ali)]
    Q = DevicePosteriors.from_posteriors(ctx, want_posts)
    assert P.download() == Q.download() == want_posts
    assert (np.asarray(P.frame_off) == np.asarray(Q.frame_off)).all() and list(P.status) == list(Q.status)
    a, b = DeviceFmllrStats(ctx, N_SPK, 40), DeviceFmllrStats(ctx, N_SPK, 40)
    us.acc_fmllr_stats_post(dm, tm, P, U2S, a)
    us.acc_fmllr_stats_post(dm, tm, Q, U2S, b)
    _same_bits(a.download(), b.download(), "from_alignment")
    _assert_stats(a.download(), ref.acc_stats(m, gc, feats, want_posts, U2S, N_SPK, dtype=np.float64), "from_alignment")
    P.close(); Q.close()


# ---- transform ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 13, 40, 80])
def test_transform_against_the_fmaf_chain(ctx, D):
    import torch
    import kaldi_hmm_gmm_amd as khg
    rng = np.random.default_rng(D)
    lens = [65, 1, 64, 130, 7]
    u2s = np.array([1, 0, -1, 2, 1], np.int32)
    feats = [rng.standard_normal((T, D)).astype(np.float32) for T in lens]
    W = rng.standard_normal((3, D, D + 1)).astype(np.float32)
    want = np.concatenate([f if s < 0 else khg.transform_feats(f, W[s]) for f, s in zip(feats, u2s)])
    fo = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    x = np.ascontiguousarray(np.concatenate(feats))
    us = khg.UtteranceSet(ctx, None, fo, x)
    out = torch.zeros((int(fo[-1]), D), dtype=torch.float32, device="cuda:%d" % ctx.device)
    khg.transform_feats_batch(us, u2s, W, out=out.data_ptr())
    assert out.cpu().numpy().tobytes() == want.tobytes()
    # W resident on the device, rows in place on borrowed device features
    xd = torch.from_numpy(x).to(out.device)
    Wd = torch.from_numpy(W).to(out.device)
    us2 = khg.UtteranceSet(ctx, None, fo, (xd.data_ptr(), xd), dim=D)
    khg.transform_feats_batch(us2, u2s, Wd.data_ptr(), n_spk=3)
    assert xd.cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(Exception):
        khg.transform_feats_batch(us, np.array([1, 0, 3, 2, 1], np.int32), W)          # a speaker the transforms lack


def test_loglikes_after_the_in_place_transform(ctx):
    import kaldi_hmm_gmm_amd as khg
    c = cases.estimate_case(5, 3, 5, 400)
    m, gc = c["m"], c["gc"]
    W = np.stack([np.concatenate([np.linalg.inv(A), -(np.linalg.inv(A) @ b)[:, None]], 1) for A, b in c["maps"]]).astype(np.float32)
    dm, tm, us = _device(ctx, m, gc, c["feats"])
    pdfs = np.arange(5, dtype=np.int32)
    us.set_pdf_list(pdfs)
    us.loglikes(dm)
    def lls(u):
        return np.concatenate([np.ravel(a) for a in u.download_loglikes()])
    before = lls(us)
    khg.transform_feats_batch(us, c["utt2spk"], W)
    us.loglikes(dm)
    after = lls(us)
    fresh_feats = [khg.transform_feats(f, W[s]) for f, s in zip(c["feats"], c["utt2spk"])]
    _, _, us2 = _device(ctx, m, gc, fresh_feats)
    us2.set_pdf_list(pdfs)
    us2.loglikes(dm)
    assert after.tobytes() == lls(us2).tobytes() and after.tobytes() != before.tobytes()


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    from kaldi_hmm_gmm_amd import DeviceFmllrStats, DevicePosteriors
    m, gc, feats, pdfs, posts, _ = _shape_case(6, 1, 13)
    dev = _device(ctx, m, gc, feats)
    dm, tm, us = dev
    before, stats = _acc(ctx, dev, posts, U2S, N_SPK)

    def refused(posts_=posts, u2s=U2S, scale=1.0, st=stats, match=None):
        post = DevicePosteriors.from_posteriors(ctx, posts_)
        with pytest.raises(Exception, match=match):
            us.acc_fmllr_stats_post(dm, tm, post, np.asarray(u2s, np.int32), st, scale=scale)
        post.close()
        _same_bits(stats.download(), before, "refused")

    refused(u2s=np.where(U2S == 2, N_SPK, U2S), match="speaker")           # a speaker the statistics lack
    refused(st=DeviceFmllrStats(ctx, N_SPK, 12), match="dimension")
    short = [list(p) for p in posts]
    short[3] = short[3][:-1]
    refused(posts_=short, match="utterance 3")
    refused(posts_=posts[:-1], u2s=U2S[:-1])
    refused(scale=float("inf"), match="finite")
    big = [list(p) for p in posts]
    big[2] = [list(f) for f in big[2]]
    big[2][1] = big[2][1] + [(m.num_tids + 1, 0.5)]
    refused(posts_=big, match="transition-id")
    with pytest.raises(Exception):
        DeviceFmllrStats(ctx, 1, 81)


# ---- end to end on the trained YES / NO model -------------------------------------------------------------------------------------
def test_trained_model_lattice_posteriors_end_to_end(trained):
    """Per-speaker distortion of the test utterances; decode -> lattice posteriors -> fMLLR -> transform.  The handle is the one
    posteriors() makes of decoded lattices.  The statistics are held to the restatement; every distorted speaker is estimated (OK);
    the gain in the posterior-weighted likelihood on the transformed features plus sum(w) log |det A| is at least objf_impr (EM),
    with a slack of 2e-5 per frame (twice the absolute part of K1's per-cell tolerance; the likelihoods here are float64)."""
    khg, dx, tmh, am, graph, test_utts = trained
    from kaldi_hmm_gmm_amd import DeviceModel, DeviceTransitions, UtteranceSet, _gpu
    import types
    dctx = _gpu.default_context()
    n_spk = 3
    raw = [np.ascontiguousarray(u[2], np.float32) for u in test_utts]
    D = raw[0].shape[1]
    u2s = np.arange(len(raw), dtype=np.int32) % n_spk
    maps = cases.speaker_maps(n_spk, D, seed=17, strength=0.1)
    feats = [np.ascontiguousarray(f.astype(np.float64) @ maps[s][0].T + maps[s][1], np.float32) for f, s in zip(raw, u2s)]
    cfg = khg.LatticeFasterDecoderConfig(max_active=7000, beam=13.0, lattice_beam=6.0)
    res, dl = khg.get_raw_lattice_faster_device_batch(am, tmh, graph, feats, cfg, 0.1)
    P = dl.posteriors(1.0, 0.1)
    posts = P.download()
    go, gc, w, miv, iv = am.flat()
    id2pdf = np.asarray(tmh.transition_id_to_pdf_array(), np.int32)
    m = types.SimpleNamespace(gauss_off=np.asarray(go, np.int32), means_invvars=np.asarray(miv, np.float32), inv_vars=np.asarray(iv, np.float32), id2pdf=id2pdf)
    gc = np.asarray(gc, np.float32)
    dm, dt = DeviceModel(dctx, go, gc, miv, iv), DeviceTransitions(dctx, id2pdf)
    fo = np.concatenate([[0], np.cumsum([len(f) for f in feats])]).astype(np.int64)
    us = UtteranceSet(dctx, None, fo, np.ascontiguousarray(np.concatenate(feats)))
    r = khg.gmm_est_fmllr_batch(dm, dt, us, P, u2s, n_spk=n_spk, min_count=100.0)
    got = r["stats"].download()
    want = ref.acc_stats(m, gc, feats, posts, u2s, n_spk, dtype=np.float64)
    _assert_stats(got, want, "trained")
    assert (r["status"] == khg.FMLLR_OK).all() and (r["objf_impr"] > 0).all()
    for s in range(n_spk):
        W = r["W"][s].astype(np.float64)
        logdet = np.linalg.slogdet(W[:, :D])[1]
        gain, frames = 0.0, 0
        for u in np.nonzero(u2s == s)[0]:
            x = feats[u].astype(np.float64)
            y = x @ W[:, :D].T + W[:, D]
            frames += len(posts[u])
            for t, f in enumerate(posts[u]):
                for tid, wt in f:
                    p = int(id2pdf[tid])
                    gain += wt * (ref.loglike(m, gc, y[t:t + 1], p)[0] - ref.loglike(m, gc, x[t:t + 1], p)[0] + logdet)
        print("speaker %d: likelihood gain %.3f, objf_impr %.3f over %d frames" % (s, gain, r["objf_impr"][s], frames))
        assert gain >= r["objf_impr"][s] - 2e-5 * frames
    # the transform in place: the set's rows are the host chain's
    khg.transform_feats_batch(us, u2s, r["W"])
    P.close(); dl.close(); us.close()
