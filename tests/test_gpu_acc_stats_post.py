"""khg_acc_stats_post (gmm-acc-stats from posteriors resident on the device) through
UtteranceSet.acc_stats_post, against the oracle loop of tests/acc_post_ref.py: one orc.acc_stats_ali call per entry.

Tolerances: the project's own for K3 (occ rtol 2e-5 / atol 1e-6, mean_acc / var_acc rtol 2e-5 / atol 2e-6 x the largest magnitude,
total_log_like rel 2e-6); trans_acc and total_frames within 1e-12 * sum|w| (the re-association of at most 10^4 widened floats:
10^4 * 2^-53 = 1.1e-12).  Two device runs that differ only in the order of their fp64 additions: 1e-11 * max|.| per array."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import acc_post_ref as ref  # noqa: E402
from helpers import build, utt_feats  # noqa: E402
from test_gpu_lattice_faster_raw import _feats, _fst, _slice_bytes, setup, trained  # noqa: E402,F401

pytestmark = pytest.mark.gpu

KEYS = ("occ", "mean_acc", "var_acc", "trans_acc")


def _device(ctx, m, gc, frame_off, feats):
    from kaldi_hmm_gmm_amd import DeviceAccs, DeviceModel, DeviceTransitions, UtteranceSet
    dm = DeviceModel(ctx, m.gauss_off, gc, m.means_invvars, m.inv_vars)
    tm = DeviceTransitions(ctx, m.id2pdf)
    us = UtteranceSet(ctx, None, np.asarray(frame_off, np.int64), np.ascontiguousarray(feats, np.float32))
    return dm, tm, us, DeviceAccs(ctx, dm, tm)


def _form(opt, form):
    if form:
        opt("k3_form", form)


def _run(ctx, us, dm, tm, accs, posts, scale=1.0):
    from kaldi_hmm_gmm_amd import DevicePosteriors
    post = DevicePosteriors.from_posteriors(ctx, posts)
    us.acc_stats_post(dm, tm, post, accs, scale=scale)
    got = accs.download()
    post.close()
    return got


def _close_runs(a, b, what):
    """two device runs that differ only in the order of fp64 additions"""
    for k in ("occ", "mean_acc", "var_acc"):
        assert np.abs(a[k] - b[k]).max() <= 1e-11 * np.abs(b[k]).max(), (what, k, np.abs(a[k] - b[k]).max())
    assert abs(a["total_log_like"] - b["total_log_like"]) <= 1e-11 * abs(b["total_log_like"]), what


# ---- 5.1 against the oracle, every form ---------------------------------------------------------------------------------------
SHAPES = [(30, 8, 39, True), (30, 64, 40, False), (30, 40, 13, True), (12, 128, 80, False), (10, 100, 77, True), (6, 130, 40, False),
          (6, 300, 40, False), (8, 20, 83, True)]


@functools.lru_cache(maxsize=None)
def _case(P, G, D, ragged):
    """the set, its posteriors and the oracle's statistics: computed once per shape, shared by the forms"""
    m, gc, om, ut, _ = build(P, G, D, n_utt=12, seed=7, ragged=ragged, max_phones=3)
    feats = [utt_feats(ut, u) for u in range(12)]
    posts = ref.random_posts(ref.utt_pdfs(ut), m.id2pdf, seed=P + G + D, normalise=(D % 2 == 0))
    want = ref.oracle_post(om, m.id2pdf, int(m.gauss_off[-1]), D, m.num_tids, feats, posts)
    for v in want.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return m, gc, om, ut, posts, want


@pytest.mark.parametrize("form", [0, 1, 2])
@pytest.mark.parametrize("P,G,D,ragged", SHAPES)
def test_against_oracle(ctx, opt, P, G, D, ragged, form):
    _form(opt, form)
    m, gc, om, ut, posts, want = _case(P, G, D, ragged)
    dm, tm, us, accs = _device(ctx, m, gc, ut.frame_off, ut.feats)
    got = _run(ctx, us, dm, tm, accs, posts)
    ref.assert_stats(got, want, (P, G, D, form))


# ---- 5.2 bucket edges ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _edge_want(n):
    m, gc, om, x = ref.edge_model()
    posts = ref.bucket_edge_posts(n)
    return posts, ref.oracle_post(om, m.id2pdf, int(m.gauss_off[-1]), 40, m.num_tids, [x], posts)


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("n,ny", [(1, 0), (63, 0), (64, 0), (65, 0), (128, 0), (129, 0), (65, 3)])
def test_bucket_edges(ctx, opt, n, ny, form):
    """pdf 0 holds n entries (the edges of K3_CHUNK = 64), pdf 1 none, pdf 2 3000 (three times the average), pdf 3 the rest"""
    _form(opt, form)
    if ny:
        opt("k3_ny", ny)
    m, gc, om, x = ref.edge_model()
    posts, want = _edge_want(n)
    dm, tm, us, accs = _device(ctx, m, gc, [0, len(x)], x)
    got = _run(ctx, us, dm, tm, accs, posts)
    a, b = int(m.gauss_off[1]), int(m.gauss_off[2])
    assert not got["occ"][a:b].any() and not got["mean_acc"][a:b].any()
    ref.assert_stats(got, want, ("edge", n, ny, form))


# ---- 5.3 unit posteriors are the alignment ------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("P,G,D,ragged", [(30, 64, 40, False), (10, 100, 77, True)])
def test_unit_posteriors_are_the_alignment(ctx, opt, P, G, D, ragged, form):
    """acc_stats_post(ali_to_post(ali)) against acc_stats(ali) in the SAME fp32 form: the two differ only in the order of the fp64
    additions.  Under k3_form = 1 alone an alignment pass takes the fp16 form k3_accumulate_block16 where its domain holds, which
    posteriors never run, so k3_phase_a = 1 holds the alignment pass to the fp32 / fp64 MFMA form."""
    from kaldi_hmm_gmm_amd import DeviceAccs, ali_to_post
    _form(opt, form)
    if form == 1:
        opt("k3_phase_a", 1)
    m, gc, om, ut, _, _ = _case(P, G, D, ragged)
    dm, tm, us, accs = _device(ctx, m, gc, ut.frame_off, ut.feats)
    posts = [ali_to_post(ut.ref_ali[ut.frame_off[u]: ut.frame_off[u + 1]]) for u in range(12)]
    got = _run(ctx, us, dm, tm, accs, posts)
    accs2 = DeviceAccs(ctx, dm, tm)
    us.upload_ali(ut.ref_ali)
    us.acc_stats(dm, tm, accs2, weight=1.0)
    want = accs2.download()
    assert np.array_equal(got["trans_acc"], want["trans_acc"]) and got["total_frames"] == want["total_frames"] == ut.frame_off[-1]
    _close_runs(got, want, (P, G, D, form))
    # ... and the alignment path finds its own buffers as it left them: once more, bit for bit
    accs2.zero()
    us.acc_stats(dm, tm, accs2, weight=1.0)
    again = accs2.download()
    assert all(np.array_equal(again[k], want[k]) for k in KEYS)


# ---- 5.4 weights --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _weights_case(scale):
    m, gc, om, ut, posts, _ = _case(30, 64, 40, False)
    special = [-0.7, 1e-30, 0.0, 3.5]
    # (on entries of the frame's own pdf: tests/acc_post_ref.py says why the others keep their small weights)
    pdfs = ref.utt_pdfs(ut)
    posts = [[[(t, special[(u + i + k) % 7] if (u + i + k) % 7 < 4 and m.id2pdf[t] == pdfs[u][i] else w) for k, (t, w) in enumerate(f)]
              for i, f in enumerate(p)] for u, p in enumerate(posts)]
    flat = [w for p in posts for f in p for _, w in f]
    assert all(flat.count(s) > 10 for s in special)
    feats = [utt_feats(ut, u) for u in range(12)]
    return m, gc, ut, posts, ref.oracle_post(om, m.id2pdf, int(m.gauss_off[-1]), 40, m.num_tids, feats, posts, scale)


@pytest.mark.parametrize("form", [0, 2])
@pytest.mark.parametrize("scale", [1.0, -0.5])
def test_weights(ctx, opt, scale, form):
    _form(opt, form)
    m, gc, ut, posts, want = _weights_case(scale)
    dm, tm, us, accs = _device(ctx, m, gc, ut.frame_off, ut.feats)
    got = _run(ctx, us, dm, tm, accs, posts, scale=scale)
    ref.assert_stats(got, want, ("weights", scale, form))


# ---- ordinary weights on ids of any pdf: held to float64 (tests/acc_post_ref.py derives the bound) ---------------------------------
@functools.lru_cache(maxsize=None)
def _uniform_case(P, G, D, ragged):
    m, gc, om, ut, _, _ = _case(P, G, D, ragged)
    feats = [utt_feats(ut, u) for u in range(12)]
    posts = ref.uniform_posts([len(f) for f in feats], m.num_tids, seed=5)
    return m, gc, ut, posts, ref.exact_post(m, gc, feats, posts, bounds=True)


@pytest.mark.parametrize("form", [0, 2])
@pytest.mark.parametrize("P,G,D,ragged", [(30, 64, 40, False), (10, 100, 77, True)])
def test_uniform_ids_against_float64(ctx, opt, P, G, D, ragged, form):
    """the case of a lattice posterior -- an ordinary weight on a frame under a pdf that does not fit it -- where the oracle's fp32
    chain is no yardstick at the K3 tolerances: the device within the derived fp32 bound of float64, as the oracle is"""
    _form(opt, form)
    m, gc, ut, posts, exact = _uniform_case(P, G, D, ragged)
    dm, tm, us, accs = _device(ctx, m, gc, ut.frame_off, ut.feats)
    got = _run(ctx, us, dm, tm, accs, posts)
    worst = ref.assert_within_bounds(got, exact, (P, G, D, form))
    print("device against float64: largest error / bound %.3g" % worst)
    assert abs(got["total_log_like"] - exact["total_log_like"]) <= 2e-6 * abs(exact["total_log_like"])
    assert np.abs(got["trans_acc"] - exact["trans_acc"]).max() <= 1e-12 * exact["total_frames"]


def test_weight_beyond_float_raises_the_error_word(ctx):
    """|scale * w64| above FLT_MAX: the entry is dropped on the device and the next synchronising call raises; the block stays finite"""
    m, gc, om, ut, posts, _ = _case(30, 8, 39, True)
    dm, tm, us, accs = _device(ctx, m, gc, ut.frame_off, ut.feats)
    huge = [list(p) for p in posts]
    huge[0] = [list(f) for f in huge[0]]
    huge[0][0] = [(1, 1e300)]
    from kaldi_hmm_gmm_amd import DevicePosteriors
    post = DevicePosteriors.from_posteriors(ctx, huge)
    us.acc_stats_post(dm, tm, post, accs)
    with pytest.raises(Exception, match="overflow"):
        accs.download()
    got = accs.download()                       # (the word is cleared by the call that reported it)
    assert all(np.isfinite(got[k]).all() for k in KEYS) and np.isfinite(got["total_frames"])
    post.close()


# ---- the script level: gmm_acc_stats_batch through AccumAmDiagGmm's device-resident block -----------------------------------------
def test_gmm_acc_stats_batch_against_oracle(ctx):
    import kaldi_hmm_gmm_amd as khg
    from kaldi_hmm_gmm_amd import _gpu, synth
    _gpu.set_default_context(ctx)
    m, gc, om, ut, posts, want = _case(30, 8, 39, True)
    am, tmh = synth.host_objects(m)
    assert tmh.num_transition_ids == m.num_tids
    gmm_accs = khg.AccumAmDiagGmm()
    gmm_accs.init(model=am, flags=khg.GmmUpdateFlags.kGmmAll)
    feats = [utt_feats(ut, u) for u in range(12)]
    ll, tacc = khg.gmm_acc_stats_batch(am, gmm_accs, tmh, feats[:6], posts[:6])
    for f, p in zip(feats[6:], posts[6:]):       # ... and one utterance at a time, the transition statistics carried along
        ll1, tacc = khg.gmm_acc_stats(am_gmm=am, gmm_accs=gmm_accs, transition_model=tmh, feats=f, post=p, transition_accs=tacc)
        ll += ll1
    assert gmm_accs._has_device_stats
    got = {"occ": np.concatenate([np.asarray(gmm_accs.get_acc(p).occupancy) for p in range(m.num_pdfs)]),
           "mean_acc": np.concatenate([np.asarray(gmm_accs.get_acc(p).mean_accumulator) for p in range(m.num_pdfs)]),
           "var_acc": np.concatenate([np.asarray(gmm_accs.get_acc(p).variance_accumulator) for p in range(m.num_pdfs)]),
           "trans_acc": np.asarray(tacc, np.float64), "total_frames": float(gmm_accs._total_frames), "total_log_like": float(gmm_accs._total_log_like)}
    ref.assert_stats(got, want, "gmm_acc_stats_batch")
    assert abs(ll - want["total_log_like"]) <= 2e-6 * abs(want["total_log_like"])      # the calls' own log-likes: weighted, as the block's


# ---- 5.5 empty utterances, additivity, batch independence ---------------------------------------------------------------------
def test_empty_utterances_and_additivity(ctx):
    from kaldi_hmm_gmm_amd import DeviceAccs, UtteranceSet
    U, empty = 65, (0, 63, 64)
    m, gc, om, ut, _ = build(9, 16, 40, n_utt=U, seed=11, max_phones=2)
    T = np.diff(ut.frame_off)
    posts = ref.random_posts(ref.utt_pdfs(ut), m.id2pdf, seed=19)
    for u in empty:
        posts[u] = []
    dm, tm, us, accs = _device(ctx, m, gc, ut.frame_off, ut.feats)
    whole = _run(ctx, us, dm, tm, accs, posts)
    # the same handle into the same block again: twice the statistics
    accs2 = DeviceAccs(ctx, dm, tm)
    twice = _run(ctx, us, dm, tm, accs2, posts)
    twice = _run(ctx, us, dm, tm, accs2, posts)
    for k in KEYS:
        assert np.abs(twice[k] - 2.0 * whole[k]).max() <= 1e-11 * np.abs(twice[k]).max(), k
    # ... and the sum of one-utterance handles on one-utterance sets
    accs3 = DeviceAccs(ctx, dm, tm)
    for u in range(U):
        if u in empty:
            continue
        one = UtteranceSet(ctx, None, np.array([0, T[u]], np.int64), np.ascontiguousarray(utt_feats(ut, u)))
        parts = _run(ctx, one, dm, tm, accs3, [posts[u]])
        one.close()
    _close_runs(whole, parts, "one-utterance handles")
    bound = 1e-12 * sum(abs(w) for p in posts for f in p for _, w in f)
    assert np.abs(whole["trans_acc"] - parts["trans_acc"]).max() <= bound and abs(whole["total_frames"] - parts["total_frames"]) <= bound


# ---- 5.6 refusals -------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    from kaldi_hmm_gmm_amd import DeviceAccs, DeviceModel, DevicePosteriors
    m, gc, om, ut, posts, _ = _case(30, 8, 39, True)
    dm, tm, us, accs = _device(ctx, m, gc, ut.frame_off, ut.feats)
    before = _run(ctx, us, dm, tm, accs, posts)

    def refused(posts_, scale=1.0, model=dm, accs_=accs, close=False):
        post = DevicePosteriors.from_posteriors(ctx, posts_)
        if close:
            post.close()
        with pytest.raises(Exception):
            us.acc_stats_post(model, tm, post, accs_, scale=scale)
        post.close()
        after = accs.download()
        assert all(after[k].tobytes() == before[k].tobytes() for k in KEYS) and after["total_frames"] == before["total_frames"] \
            and after["total_log_like"] == before["total_log_like"]

    short = [list(p) for p in posts]
    short[4] = short[4][:-1]                         # one frame fewer than the set has for utterance 4
    named = DevicePosteriors.from_posteriors(ctx, short)
    with pytest.raises(Exception, match="utterance 4"):
        us.acc_stats_post(dm, tm, named, accs)
    named.close()
    refused(short)
    refused(posts[:-1])                              # another n_utt
    big = [list(p) for p in posts]
    big[2] = [list(f) for f in big[2]]
    big[2][1] = big[2][1] + [(m.num_tids + 1, 0.5)]
    refused(big)                                     # an id above num_tids
    refused(posts, scale=float("nan"))
    refused(posts, close=True)                       # a closed handle
    m2, gc2, *_ = build(30, 8, 40, n_utt=1, seed=7, ragged=True, max_phones=2)
    dm2 = DeviceModel(ctx, m2.gauss_off, gc2, m2.means_invvars, m2.inv_vars)
    refused(posts, model=dm2)                        # a model of another dimension


# ---- 5.7 end to end on real lattices ------------------------------------------------------------------------------------------
def _lattice_posts_to_stats(khg, am, tm, dl, feats, what):
    """posteriors(1.0, 0.1) of the device lattices -> acc_stats_post on a set of the same utterances, against the oracle loop over
    post.download(); -> the statistics"""
    from kaldi_hmm_gmm_amd import DeviceAccs, DeviceModel, DeviceTransitions, UtteranceSet, _gpu
    from oracle import oracle as orc
    dctx = _gpu.default_context()                   # the batch calls' context: the lattices live there
    go, gc, w, miv, iv = am.flat()
    id2pdf = np.asarray(tm.transition_id_to_pdf_array(), np.int32)
    P = dl.posteriors(1.0, 0.1)
    posts = P.download()
    ok = [(int(s) & 1) != 0 for s in P.status]
    assert any(ok) and all(len(p) == (len(f) if o else 0) for p, f, o in zip(posts, feats, ok))
    D = feats[0].shape[1]
    dm = DeviceModel(dctx, go, gc, miv, iv)
    dt = DeviceTransitions(dctx, id2pdf)
    fo = np.concatenate([[0], np.cumsum([len(f) for f in feats])]).astype(np.int64)
    us = UtteranceSet(dctx, None, fo, np.ascontiguousarray(np.concatenate(feats), np.float32))
    accs = DeviceAccs(dctx, dm, dt)
    us.acc_stats_post(dm, dt, P, accs)
    got = accs.download()
    om = orc.OModel(np.asarray(go, np.int32), np.asarray(gc, np.float32), np.asarray(miv, np.float32), np.asarray(iv, np.float32))
    want = ref.oracle_post(om, id2pdf, int(go[-1]), D, len(id2pdf) - 1, feats, posts)
    ref.assert_stats(got, want, what)
    nfr = sum(len(f) for f, o in zip(feats, ok) if o)
    assert abs(got["total_frames"] - nfr) <= 1e-9 * nfr, (got["total_frames"], nfr)      # every frame's posteriors sum to one
    merged = sum(len(f) - len({int(id2pdf[t]) for t, _ in f}) for p in posts for f in p)
    print("%s: %d entries on %d frames; post-to-pdf-post would merge %d of them" % (what, sum(len(f) for p in posts for f in p), nfr, merged))
    P.close(); us.close(); accs.close(); dm.close(); dt.close()
    return got


def test_trained_word_loop_lattices(trained):
    khg, dx, tm, am, graph, test_utts = trained
    khg._gpu.default_context()
    feats = [np.ascontiguousarray(u[2], np.float32) for u in test_utts]
    cfg = khg.LatticeFasterDecoderConfig(max_active=7000, beam=13.0, lattice_beam=6.0)
    res, dl = khg.get_raw_lattice_faster_device_batch(am, tm, graph, feats, cfg, 0.1)
    assert all(r["status"] == 1 for r in res)
    _lattice_posts_to_stats(khg, am, tm, dl, feats, "word loop")
    dl.close()


def test_two_chunk_handle(setup):
    """the two-chunk construction of tests/test_gpu_lattice_post.py: test_two_chunks -- more than one chunk through the flatten pass"""
    import test_shared_graph_cpu as sg
    khg, synth, m, am, tm, ut = setup
    khg._gpu.default_context()
    g = sg.word_loop_graph(np.random.default_rng(sg.BIG_W), m.num_tids, sg.BIG_W, sg.BIG_CHAIN)
    S, A = len(g["final"]), len(g["ilabel"])
    lens3 = [12, 11, 13]
    hb = max(1000, int(np.float32(S) * np.float32(2.0))) + 1
    U = int((4 << 30) // min(_slice_bytes(T, S, A, hb) for T in lens3)) + 9
    feats = _feats(ut, U, [lens3[u % 3] for u in range(U)])
    dg = khg.DecodingGraph(_fst(khg, g), tm)
    cfg = khg.LatticeFasterDecoderConfig(beam=8.0, max_active=100, min_active=0, lattice_beam=4.0)
    res, dl = khg.get_raw_lattice_faster_device_batch(am, tm, dg, feats, cfg, 0.1)
    assert dl.num_chunks >= 2
    _lattice_posts_to_stats(khg, am, tm, dl, feats, "two chunks")
    dl.close(); dg.close()
