"""LDA on the device: khg_acc_lda_stats_post through UtteranceSet.acc_lda_stats_post against the restatement of
tests/lda_ref.py, the bits of the statistics across runs / calls / chunk sizes, the fused splice-and-project against the host form
on the bits, and acc-lda -> est-lda end to end.

The bound of the statistics is derived, not measured: any order of an n-term fp64 sum of once-rounded products errs by at most
n 2^-52 sum |terms| per element.  The restatement returns sum |terms| and n (the entries of the class for zero_acc / first_acc, all
the entries for total_second_acc) and adds its own terms in extended precision, so that its rounding stays out of the bound."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lda_ref as ref  # noqa: E402
from helpers import build  # noqa: E402
from test_gpu_lattice_faster_raw import trained  # noqa: E402,F401

pytestmark = pytest.mark.gpu
SLICE = 1024
U52 = 2.0 ** -52


def _id2pdf(C):
    """two transition-ids per class: a frame can carry two ids of one pdf"""
    return np.concatenate([[0], np.repeat(np.arange(C), 2)]).astype(np.int32)


def _posts(lens, id2pdf, seed, skip_class=None, max_entries=5, drop_utt=None, min_entries=0):
    """per frame min_entries .. max_entries entries with distinct ids (none of skip_class), weights in (0.05, 1)"""
    rng = np.random.default_rng(seed)
    ids = np.array([t for t in range(1, len(id2pdf)) if id2pdf[t] != skip_class])
    posts = []
    for u, T in enumerate(lens):
        post = []
        for _ in range(T):
            k = int(rng.integers(min_entries, max_entries + 1))
            pick = rng.choice(ids, size=min(k, len(ids)), replace=False)
            post.append([(int(t), float(w)) for t, w in zip(pick, rng.uniform(0.05, 1.0, size=len(pick)))])
        posts.append([] if u == drop_utt else post)
    return posts


def _feats(lens, D, seed):
    rng = np.random.default_rng(seed)
    return [np.ascontiguousarray(rng.standard_normal((T, D)) * 1.5 + 0.7, np.float32) for T in lens]


def _device(ctx, feats, id2pdf):
    from kaldi_hmm_gmm_amd import DeviceTransitions, UtteranceSet
    tm = DeviceTransitions(ctx, id2pdf)
    fo = np.concatenate([[0], np.cumsum([len(f) for f in feats])]).astype(np.int64)
    return tm, UtteranceSet(ctx, None, fo, np.ascontiguousarray(np.concatenate(feats), np.float32))


def _acc(ctx, dev, posts, C, L, R, scale=1.0, chunk=None, stats=None, download=True):
    from kaldi_hmm_gmm_amd import DeviceLdaStats, DevicePosteriors
    tm, us = dev
    if stats is None:
        stats = DeviceLdaStats(ctx, C, us.dim, L, R)
    if chunk is not None:
        stats.set_chunk_frames(chunk)
    post = DevicePosteriors.from_posteriors(ctx, posts)
    us.acc_lda_stats_post(tm, post, stats, scale=scale)
    got = stats.download() if download else None
    post.close()
    return got, stats


def _assert_within_bound(got, want, what):
    n = want["n_cls"].astype(np.float64)
    Dz = want["first"].shape[1]
    b0, b1, b2 = n * U52 * want["abs_zero"], n[:, None] * U52 * want["abs_first"], want["n_second"] * U52 * want["abs_second"]
    e0, e1 = np.abs(got["zero_acc"] - want["zero"]), np.abs(got["first_acc"] - want["first"])
    e2 = np.abs(ref.unpacked(got["total_second_acc"], Dz) - want["second"])
    worst = max(float((e / np.maximum(b, 1e-300)).max()) for e, b in ((e0, b0), (e1, b1), (e2, b2)))
    print("%s: %d entries, largest error / bound %.3g" % (what, want["n_second"], worst))
    assert (e0 <= b0).all() and (e1 <= b1).all() and (e2 <= b2).all(), what
    assert got["total_second_acc"].shape == (Dz * (Dz + 1) // 2,)


def _same_bits(a, b, what):
    for k in ("zero_acc", "first_acc", "total_second_acc"):
        assert a[k].tobytes() == b[k].tobytes(), (what, k, np.abs(a[k] - b[k]).max())


# ---- statistics against the restatement ---------------------------------------------------------------------------------------------
SHAPES = [(6, 1, 0, 0), (6, 5, 1, 1), (6, 1, 8, 7), (6, 17, 0, 0), (14, 13, 4, 4), (4, 40, 4, 4)]     # C, D, L, R: Dz = 1, 15, 16, 17, 117, 360


@functools.lru_cache(maxsize=None)
def _shape_case(C, D, L, R):
    """utterances of 1, 2, L, L + R + 1, 64 and 65 frames, a one-frame utterance first and last (a clamp that slips reads outside the
    buffer's ends, which the numbers catch); frames of 0 .. 5 entries, two ids of one pdf on a frame, class C - 2 without entries,
    utterance 5 without frames in the handle"""
    lens = [1] + [T for T in (2, L, L + R + 1, 64, 23, 65) if T > 0] + [1]
    assert sum(lens) <= 300
    id2pdf = _id2pdf(C)
    feats = _feats(lens, D, seed=C + D + L)
    posts = _posts(lens, id2pdf, seed=D + R, skip_class=C - 2, drop_utt=5)
    assert any(len(f) == 0 for p in posts for f in p) and any(len(f) == 5 for p in posts for f in p)
    assert any(len({int(id2pdf[t]) for t, _ in f}) < len(f) for p in posts for f in p)
    want = ref.definition_stats(feats, posts, id2pdf, C, L, R)
    assert want["n_cls"][C - 2] == 0 and (np.delete(want["n_cls"], C - 2) > 0).all()
    return id2pdf, feats, posts, want


@pytest.mark.parametrize("C,D,L,R", SHAPES)
def test_statistics_against_the_definition(ctx, C, D, L, R):
    id2pdf, feats, posts, want = _shape_case(C, D, L, R)
    dev = _device(ctx, feats, id2pdf)
    got, stats = _acc(ctx, dev, posts, C, L, R)
    _assert_within_bound(got, want, (C, D, L, R))
    assert got["zero_acc"][C - 2] == 0.0 and not got["first_acc"][C - 2].any()      # the class without entries
    twice, _ = _acc(ctx, dev, posts, C, L, R, stats=stats)      # a second call adds: twice the statistics, exactly (x + x)
    for k in got:
        assert (twice[k] == 2.0 * got[k]).all(), k
    stats.upload(got["zero_acc"], got["first_acc"], got["total_second_acc"])
    _same_bits(stats.download(), got, "upload(download())")


@pytest.mark.parametrize("scale", [1.0, -0.5])
def test_negative_zero_and_tiny_weights(ctx, scale):
    C, D, L, R = 6, 5, 1, 1
    id2pdf, feats, posts, _ = _shape_case(C, D, L, R)
    special = [-0.7, 1e-30, 0.0, 3.5]
    posts = [[[(t, special[(u + i + k) % 7] if (u + i + k) % 7 < 4 else w) for k, (t, w) in enumerate(f)] for i, f in enumerate(p)]
             for u, p in enumerate(posts)]
    flat = [w for p in posts for f in p for _, w in f]
    assert all(flat.count(s) > 5 for s in special)
    want = ref.definition_stats(feats, posts, id2pdf, C, L, R, scale=scale)
    got, _ = _acc(ctx, _device(ctx, feats, id2pdf), posts, C, L, R, scale=scale)
    _assert_within_bound(got, want, ("weights", scale))


def _split(T):
    """T frames over three utterances (one when T < 3): the slice edges at 1024, 2048 and 3072 fall inside utterances"""
    return [T] if T < 3 else [T // 3, T // 2 - T // 3, T - T // 2]


@functools.lru_cache(maxsize=None)
def _frames_case(T):
    C, D, L, R = 3, 5, 1, 1                                     # three classes: at 3077 frames a class has more than one slice of entries
    lens = _split(T)
    edges = np.cumsum(lens)[:-1]
    assert not any(e % SLICE == 0 for e in edges)
    id2pdf = _id2pdf(C)
    feats = _feats(lens, D, seed=T)
    posts = _posts(lens, id2pdf, seed=T + 1, max_entries=2, min_entries=1)
    return C, L, R, id2pdf, feats, posts, ref.definition_stats(feats, posts, id2pdf, C, L, R)


@pytest.mark.parametrize("T", [1, SLICE - 1, SLICE, SLICE + 1, 3 * SLICE + 5])
def test_frame_counts_around_the_slice(ctx, T):
    C, L, R, id2pdf, feats, posts, want = _frames_case(T)
    got, stats = _acc(ctx, _device(ctx, feats, id2pdf), posts, C, L, R)
    _assert_within_bound(got, want, "%d frames" % T)
    assert stats.num_chunks() == 1


def test_bits_across_runs_chunks_and_calls(ctx):
    from kaldi_hmm_gmm_amd import DeviceLdaStats
    T = 3 * SLICE + 5
    C, L, R, id2pdf, feats, posts, want = _frames_case(T)
    dev = _device(ctx, feats, id2pdf)
    first, _ = _acc(ctx, dev, posts, C, L, R)
    for run in range(3):                                        # equal bits over four runs
        again, _ = _acc(ctx, dev, posts, C, L, R)
        _same_bits(again, first, "run %d" % (run + 2))
    small, st = _acc(ctx, dev, posts, C, L, R, chunk=SLICE)     # a chunk of one slice against the default
    assert st.num_chunks() == 4
    _same_bits(small, first, "chunk of one slice")
    # two calls into one handle equal the add of two handles
    posts2 = _posts([len(f) for f in feats], id2pdf, seed=77, max_entries=3)
    both, st_both = _acc(ctx, dev, posts, C, L, R, download=False)
    both, _ = _acc(ctx, dev, posts2, C, L, R, stats=st_both)
    _, a = _acc(ctx, dev, posts, C, L, R, download=False)
    _, b = _acc(ctx, dev, posts2, C, L, R, download=False)
    a.add(1.0, b)
    _same_bits(a.download(), both, "two calls against add")
    a.zero()
    assert not any(v.any() for v in a.download().values())
    with pytest.raises(Exception):
        a.add(1.0, DeviceLdaStats(ctx, C, 5, 2, 1))             # another context width


def test_refusals_leave_the_handles_bits(ctx):
    from kaldi_hmm_gmm_amd import DeviceLdaStats, DevicePosteriors, DeviceTransitions, LDA_MAX_SPLICED_DIM
    C, D, L, R = 6, 5, 1, 1
    id2pdf, feats, posts, _ = _shape_case(C, D, L, R)
    dev = _device(ctx, feats, id2pdf)
    tm, us = dev
    before, stats = _acc(ctx, dev, posts, C, L, R)
    post = DevicePosteriors.from_posteriors(ctx, posts)
    with pytest.raises(Exception):
        us.acc_lda_stats_post(tm, post, stats, scale=float("nan"))
    with pytest.raises(Exception, match="classes"):
        us.acc_lda_stats_post(tm, post, DeviceLdaStats(ctx, C + 1, D, L, R))
    with pytest.raises(Exception, match="dimension"):
        us.acc_lda_stats_post(tm, post, DeviceLdaStats(ctx, C, D + 1, L, R))
    with pytest.raises(Exception):
        us.acc_lda_stats_post(DeviceTransitions(ctx, _id2pdf(2)), post, stats)        # ids the transition model lacks
    short = DevicePosteriors.from_posteriors(ctx, posts[:-1])
    with pytest.raises(Exception, match="utterances"):
        us.acc_lda_stats_post(tm, short, stats)
    wrong = [p[:-1] if len(p) > 1 else p for p in posts]
    bad = DevicePosteriors.from_posteriors(ctx, wrong)
    with pytest.raises(Exception, match="frames"):
        us.acc_lda_stats_post(tm, bad, stats)
    _same_bits(stats.download(), before, "after the refusals")
    with pytest.raises(Exception, match="KHG_LDA_MAX_SPLICED_DIM"):
        DeviceLdaStats(ctx, C, 40, LDA_MAX_SPLICED_DIM // 40, 0)
    for h in (post, short, bad):
        h.close()


# ---- splice-feats | transform-feats -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,L,R,out_dim", [(1, 0, 0, 1), (13, 4, 4, 40), (40, 4, 4, 40)])
def test_splice_transform_equals_the_host_form_on_the_bits(ctx, D, L, R, out_dim):
    import kaldi_hmm_gmm_amd as khg
    lens = [1] + [T for T in (2, L, L + R + 1, 64, 65, 130) if T > 0] + [1]
    feats = _feats(lens, D, seed=D + L)
    _, us = _device(ctx, feats, _id2pdf(2))
    Dz = D * (L + R + 1)
    rng = np.random.default_rng(out_dim + D)
    for offset in (False, True):
        M = (rng.standard_normal((out_dim, Dz + (1 if offset else 0))) / np.sqrt(Dz)).astype(np.float32)
        want = np.concatenate([khg.splice_transform_feats(f, M, L, R) for f in feats])
        out = khg.splice_transform_feats_batch(us, M, L, R)
        assert tuple(out.shape) == want.shape and out.cpu().numpy().tobytes() == want.tobytes(), offset
    want = np.concatenate([khg.splice_feats(f, L, R) for f in feats])
    out = khg.splice_transform_feats_batch(us, None, L, R)
    assert out.cpu().numpy().tobytes() == want.tobytes()        # pure splice: every byte
    assert want.tobytes() == np.concatenate([ref.splice(f, L, R) for f in feats]).tobytes()
    import torch
    mine = torch.zeros((int(sum(lens)), Dz), dtype=torch.float32, device=out.device)
    assert khg.splice_transform_feats_batch(us, None, L, R, out=mine) is mine and mine.cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(Exception):
        khg.splice_transform_feats_batch(us, np.zeros((out_dim, Dz + 2), np.float32), L, R)


def test_transform_limits_name_themselves(ctx):
    import kaldi_hmm_gmm_amd as khg
    _, us = _device(ctx, _feats([3], 40, seed=1), _id2pdf(2))
    with pytest.raises(Exception, match="KHG_LDA_MAX_SPLICED_DIM"):
        khg.splice_transform_feats_batch(us, None, 7, 6)                               # 40 x 14 = 560
    with pytest.raises(Exception, match="LDS"):
        khg.splice_transform_feats_batch(us, np.zeros((120, 360), np.float32), 4, 4)   # 120 x 361 floats of matrix


def test_loglikes_of_a_set_on_the_projected_tensor(ctx):
    """a set built on the returned tensor scores as a set built from the host-projected rows, on the bits"""
    import kaldi_hmm_gmm_amd as khg
    m, gc, om, ut, _ = build(5, 3, 8, n_utt=1, seed=4, max_phones=2)
    lens = [1, 9, 64, 65, 30]
    feats = _feats(lens, 3, seed=12)
    L, R = 2, 1
    rng = np.random.default_rng(3)
    M = (rng.standard_normal((8, 3 * (L + R + 1) + 1)) * 0.5).astype(np.float32)
    tm, us = _device(ctx, feats, m.id2pdf)
    t = khg.splice_transform_feats_batch(us, M, L, R)
    dm = khg.DeviceModel(ctx, m.gauss_off, gc, m.means_invvars, m.inv_vars, m.weights)
    fo = np.asarray(us.frame_off)
    on_tensor = khg.UtteranceSet(ctx, None, fo, (t.data_ptr(), t), dim=8)
    host_rows = np.ascontiguousarray(np.concatenate([khg.splice_transform_feats(f, M, L, R) for f in feats]))
    on_host = khg.UtteranceSet(ctx, None, fo, host_rows)
    pdfs = np.arange(5, dtype=np.int32)

    def lls(u):
        u.set_pdf_list(pdfs)
        u.loglikes(dm)
        return np.concatenate([np.ravel(a) for a in u.download_loglikes()])
    a, b = lls(on_tensor), lls(on_host)
    assert a.tobytes() == b.tobytes() and np.isfinite(a).all()


# ---- end to end on the trained YES / NO model ----------------------------------------------------------------------------------------
def test_trained_model_end_to_end(trained):
    """decode -> lattice posteriors -> acc-lda on +-2 frames -> est-lda: the statistics are held to the definition, the status is OK, the
    eigenvalues descend, and M_full whitens Wc and diagonalises Bc of the DOWNLOADED statistics within the cap Dz 2^-40 max(1,
    lambda_max) (the condition of tests/test_lda_cpu.py); the projected rows come back finite and equal the host form."""
    khg, dx, tmh, am, graph, test_utts = trained
    from kaldi_hmm_gmm_amd import DeviceTransitions, UtteranceSet, _gpu
    dctx = _gpu.default_context()
    feats = [np.ascontiguousarray(u[2], np.float32) for u in test_utts]
    D, L, R = feats[0].shape[1], 2, 2
    Dz = D * (L + R + 1)
    cfg = khg.LatticeFasterDecoderConfig(max_active=7000, beam=13.0, lattice_beam=6.0)
    res, dl = khg.get_raw_lattice_faster_device_batch(am, tmh, graph, feats, cfg, 0.1)
    P = dl.posteriors(1.0, 0.1)
    posts = P.download()
    id2pdf = np.asarray(tmh.transition_id_to_pdf_array(), np.int32)
    C = int(id2pdf[1:].max()) + 1
    dt = DeviceTransitions(dctx, id2pdf)
    fo = np.concatenate([[0], np.cumsum([len(f) for f in feats])]).astype(np.int64)
    us = UtteranceSet(dctx, None, fo, np.ascontiguousarray(np.concatenate(feats)))
    r = khg.acc_lda(dt, us, P, left=L, right=R)
    assert r["stats"].num_classes == C and r["stats"].dim_z == Dz
    _assert_within_bound(r, ref.definition_stats(feats, posts, id2pdf, C, L, R), "trained")
    td = min(C - 1, 10)
    est = khg.est_lda(r["stats"], target_dim=td)
    assert est["status"] == khg.LDA_OK and est["count"] == r["zero_acc"].sum() and (np.diff(est["eig"]) <= 0).all()
    N, mu, Tc, Bc, Wc = ref.scatter(r["zero_acc"], r["first_acc"], r["total_second_acc"])
    Mf, lam = est["M_full"], est["eig"]
    cap = Dz * 2.0 ** -40 * max(1.0, lam[0])
    d_w, d_b = np.abs(Mf @ Wc @ Mf.T - np.eye(Dz)).max(), np.abs(Mf @ Bc @ Mf.T - np.diag(lam)).max()
    print("kept eigenvalues %s; residuals W %.3g B %.3g, cap %.3g" % (np.round(lam[:td], 4), d_w, d_b, cap))
    assert d_w <= cap and d_b <= cap and lam[td - 1] > 0
    # silence weighting goes through weight_silence_post: with every id silenced at weight 0 nothing is left
    none = khg.acc_lda(dt, us, P, left=L, right=R, silence_tids=range(1, len(id2pdf)), silence_weight=0.0)
    assert not none["zero_acc"].any() and not none["total_second_acc"].any()
    t = khg.splice_transform_feats_batch(us, est["M"], L, R)
    want = np.concatenate([khg.splice_transform_feats(f, est["M"], L, R) for f in feats])
    assert t.cpu().numpy().tobytes() == want.tobytes() and np.isfinite(want).all()
    for h in (P, us, dt, r["stats"], none["stats"]):
        h.close()
