"""fMLLR without a GPU: the restatement of tests/fmllr_ref.py against the definition, the properties of the
row update, and the host form khg_fmllr_compute against the restatement on the bits.

Condition of every bit comparison: by the restatement alone, the smallest relative gap |f1 - f2| / (|f1| + |f2|) between the two
roots' auxiliary values over all row updates of the case is >= 1e-6, so no rounding of log (a few 1e-16) can pick the other root.
The random multi-Gaussian cases here give >= 1e-3.  The converged one-Gaussian case ties to ~1e-15 and is compared by Q(W) only."""
import ctypes
from fractions import Fraction
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fmllr_cases as cases  # noqa: E402
import fmllr_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_COUNT = 50.0
CASES = [(5, 3, 5, 400), (3, 7, 13, 800)]        # P, G, D, T (the third shape of the issue, 4 / 1 / 60, is the tie case below)


def _compute(beta, K, G, **kw):
    import kaldi_hmm_gmm_amd as khg
    return khg.fmllr_compute(np.ascontiguousarray(beta, np.float64), np.ascontiguousarray(K), np.ascontiguousarray(G), **kw)


def test_restatement_against_the_definition():
    m, gc, feats, posts, utt2spk = cases.tiny_case()
    want = ref.definition_stats(m, gc, feats, posts, utt2spk, 2)
    got64 = ref.acc_stats(m, gc, feats, posts, utt2spk, 2, dtype=np.float64)
    got32 = ref.acc_stats(m, gc, feats, posts, utt2spk, 2, dtype=np.float32)
    assert want[0].min() > 0
    for g, w in zip(got64, want):
        np.testing.assert_allclose(g, w, rtol=1e-10, atol=1e-12 * np.abs(w).max())
    # the float32 rule: the project's tolerances for K3's statistics
    np.testing.assert_allclose(got32[0], want[0], rtol=2e-5, atol=1e-6)
    for g, w in zip(got32[1:], want[1:]):
        np.testing.assert_allclose(g, w, rtol=2e-5, atol=2e-6 * np.abs(w).max())


def test_repeated_entry_is_one_entry_of_doubled_weight():
    m, gc, feats, posts, utt2spk = cases.tiny_case()
    twice = [[[e for e in f for _ in range(2)] for f in p] for p in posts]
    doubled = [[[(t, 2.0 * w) for t, w in f] for f in p] for p in posts]
    a = ref.acc_stats(m, gc, feats, twice, utt2spk, 2, dtype=np.float32)
    b = ref.acc_stats(m, gc, feats, doubled, utt2spk, 2, dtype=np.float32)
    for x, y in zip(a, b):                      # x + x is exact; only the entries' order of addition into the frame's sums differs
        np.testing.assert_allclose(x, y, rtol=1e-6, atol=1e-6 * np.abs(y).max())


@pytest.mark.parametrize("P,G,D,T", CASES)
def test_q_never_falls_across_a_row_update(P, G, D, T):
    c = cases.estimate_case(P, G, D, T)
    for s in range(c["n_spk"]):
        r = ref.estimate(c["beta"][s], c["K"][s], c["G"][s], min_count=MIN_COUNT, num_iters=3, trace=True)
        assert r["status"] == ref.OK
        W0 = np.concatenate([np.eye(D), np.zeros((D, 1))], 1)
        q = [ref.auxf(c["beta"][s], c["K"][s], c["G"][s], W0)] + r["q"]
        for a, b in zip(q, q[1:]):
            assert b >= a - 1e-9 * abs(a), (a, b)
        assert q[-1] > q[0]


@pytest.mark.parametrize("P,G,D,T", CASES)
def test_true_likelihood_gain_is_at_least_the_q_gain(P, G, D, T):
    """EM: on data distorted by a known affine map, sum_t [ll(W x+) + log |det A| - ll(x)] >= Q(W) - Q([I | 0]).  The inequality is
    between exact quantities, so both sides come from float64 here: the statistics are the restatement's with dtype float64 (the
    posteriors the bound is built on are then the ones ll itself has), and the slack is rounding only, 1e-9 of the gain."""
    c = cases.estimate_case(P, G, D, T)
    m, gc = c["m"], c["gc"]
    beta, K, Gs = ref.acc_stats(m, gc, c["feats"], c["posts"], c["utt2spk"], c["n_spk"], dtype=np.float64)
    for s in range(c["n_spk"]):
        r = ref.estimate(beta[s], K[s], Gs[s], min_count=MIN_COUNT, num_iters=10)
        W = r["W"]
        logdet = np.linalg.slogdet(W[:, :D])[1]
        gain = 0.0
        for u in np.nonzero(c["utt2spk"] == s)[0]:
            x = c["feats"][u].astype(np.float64)
            y = x @ W[:, :D].T + W[:, D]
            for p in set(c["pdfs"][u]):
                sel = np.array(c["pdfs"][u]) == p
                gain += (ref.loglike(m, gc, y[sel], p) - ref.loglike(m, gc, x[sel], p)).sum() + sel.sum() * logdet
        assert r["objf_impr"] > 0
        assert gain >= r["objf_impr"] - 1e-9 * abs(gain), (gain, r["objf_impr"])


@pytest.mark.parametrize("P,G,D,T", CASES)
def test_host_form_equals_the_restatement_on_the_bits(P, G, D, T):
    c = cases.estimate_case(P, G, D, T)
    iters = 40 if D <= 5 else 6
    got = _compute(c["beta"], c["K"], c["G"], min_count=MIN_COUNT, num_iters=iters)
    for s in range(c["n_spk"]):
        r = ref.estimate(c["beta"][s], c["K"][s], c["G"][s], min_count=MIN_COUNT, num_iters=iters)
        print("speaker %d: smallest relative gap of the roots %.3g, objf_impr %.6f" % (s, r["gap"], r["objf_impr"]))
        assert r["gap"] >= 1e-6                                         # the condition of the bit comparison
        assert got["status"][s] == r["status"] == ref.OK and got["count"][s] == c["beta"][s]
        assert got["W64"][s].tobytes() == r["W"].tobytes()
        assert got["W"][s].tobytes() == r["W"].astype(np.float32).tobytes()
        assert abs(got["objf_impr"][s] - r["objf_impr"]) <= 1e-12 * abs(r["objf_impr"]) + 1e-9


def test_converged_one_gaussian_model_ties():
    """The tie of the two roots: compared by Q(W) only"""
    beta, K, G = cases.one_gaussian_converged()
    r = ref.estimate(beta, K, G, min_count=MIN_COUNT, num_iters=5)
    assert r["gap"] < 1e-9, r["gap"]                                    # this IS the tie
    got = _compute(np.array([beta]), K[None], G[None], min_count=MIN_COUNT, num_iters=5)
    assert got["status"][0] == ref.OK
    q_host = ref.auxf(beta, K, G, got["W64"][0])
    q_ref = ref.auxf(beta, K, G, r["W"])
    assert abs(q_host - q_ref) <= 1e-9 * abs(q_ref)
    assert abs(got["objf_impr"][0] - r["objf_impr"]) <= 1e-9 * abs(q_ref)


def test_low_count_and_singular():
    c = cases.estimate_case(5, 3, 5, 400)
    D = 5
    ident = np.concatenate([np.eye(D), np.zeros((D, 1))], 1)
    got = _compute(c["beta"], c["K"], c["G"], min_count=1e6)
    assert (got["status"] == ref.LOW_COUNT).all() and all((w == ident).all() for w in got["W64"]) and (got["objf_impr"] == 0).all()
    assert ref.estimate(c["beta"][0], c["K"][0], c["G"][0], min_count=1e6)["status"] == ref.LOW_COUNT
    # fewer frames than D + 1: every G[d] = sum of 3 outer products has rank 3 < 6.  Integer-valued x+ and unit a_t keep the
    # elimination exact, so the fourth pivot is exactly 0.
    xs = np.array([[1, 2, 0, 1, 2, 1], [2, 1, 1, 0, 1, 1], [0, 1, 2, 2, 1, 1]], np.float64)
    il, jl = np.tril_indices(D + 1)
    G1 = np.stack([(xs.T @ xs)[il, jl]] * D)
    K1 = np.ones((D, D + 1))
    got = _compute(np.array([600.0]), K1[None], G1[None])
    assert got["status"][0] == ref.SINGULAR and (got["W64"][0] == ident).all() and got["count"][0] == 600.0
    assert ref.estimate(600.0, K1, G1)["status"] == ref.SINGULAR


def test_refusals():
    import kaldi_hmm_gmm_amd as khg
    from kaldi_hmm_gmm_amd import _lib
    c = cases.estimate_case(5, 3, 5, 400)
    with pytest.raises(Exception):
        khg.fmllr_compute(c["beta"], c["K"][:, :, :-1], c["G"])              # K of another shape
    with pytest.raises(Exception):
        _compute(c["beta"], c["K"], c["G"], num_iters=-1)
    with pytest.raises(Exception):
        _compute(c["beta"], c["K"], c["G"], min_count=float("nan"))
    lib = _lib.lib
    f64 = ctypes.POINTER(ctypes.c_double)
    b = c["beta"].copy()
    k, g = np.ascontiguousarray(c["K"]), np.ascontiguousarray(c["G"])
    args = [b.ctypes.data_as(f64), k.ctypes.data_as(f64), g.ctypes.data_as(f64)]
    assert lib.khg_fmllr_compute(None, 2, 5, *args, None, None, None, None, None) == -1          # nowhere to put W
    assert lib.khg_fmllr_compute(None, 2, 81, *args, None, None, None, None, None) == -1     # above KHG_FMLLR_MAX_DIM
    assert b"khg_fmllr_compute" in lib.khg_last_error()
    # the device entry points refuse a dead context before anything else
    assert lib.khg_fmllr_stats_create(None, 1, 5, ctypes.byref(ctypes.c_void_p())) == -1
    assert lib.khg_utts_transform_feats(None, None, 1, None, None, None, None) == -1
    assert lib.khg_acc_fmllr_stats_post(None, None, None, None, None, 1.0, None, None) == -1


def test_weight_silence_post():
    import kaldi_hmm_gmm_amd as khg
    from kaldi_hmm_gmm_amd import fmllr
    posts = [[[(1, 0.5), (4, 0.5)], [(2, 1.0)]], [], [[(4, 0.25), (3, 0.75)]]]
    fo, eb, tid, w = khg.posts_to_arrays(posts)
    fo2, eb2, tid2, w2 = fmllr.weight_silence_post(fo, eb, tid, w, silence_tids=[1, 2, 99], silence_weight=0.1)
    assert fo2 is fo and eb2 is eb and tid2 is tid and w2 is not w
    assert w2.tolist() == [0.5 * 0.1, 0.5, 1.0 * 0.1, 0.25, 0.75] and w.tolist() == [0.5, 0.5, 1.0, 0.25, 0.75]
    assert fmllr.weight_silence_post(fo, eb, tid[:0], w[:0], [1], 0.0)[3].size == 0

    class NotPosteriors:                    # silence weighting of a resident handle is refused before anything touches the device
        pass
    real = fmllr.DevicePosteriors
    try:
        fmllr.DevicePosteriors = NotPosteriors
        utts = type("U", (), {"ctx": None, "dim": 3, "n_utt": 1})()
        with pytest.raises(ValueError, match="silence weighting"):
            khg.gmm_est_fmllr_batch(None, None, utts, NotPosteriors(), [0], silence_tids=[1])
    finally:
        fmllr.DevicePosteriors = real


def test_new_symbols_are_exported():
    from kaldi_hmm_gmm_amd import _lib
    import kaldi_hmm_gmm_amd as khg
    with open(os.path.join(ROOT, "include", "khg_hip.h")) as fh:
        header = fh.read()
    for name in ("khg_fmllr_stats_create", "khg_fmllr_stats_destroy", "khg_fmllr_stats_zero", "khg_fmllr_stats_download", "khg_fmllr_stats_upload",
                 "khg_fmllr_stats_add", "khg_fmllr_stats_set_chunk_frames", "khg_fmllr_stats_num_chunks", "khg_acc_fmllr_stats_post",
                 "khg_fmllr_compute", "khg_utts_transform_feats", "khg_fmllr_stats_estimate", "khg_posteriors_from_ali"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.SIGNATURES and getattr(_lib.lib, name) is not None, name
    assert "khg_fmllr_options_default" in _lib.SIGNATURES
    o = _lib.FmllrOptionsC()
    _lib.lib.khg_fmllr_options_default(ctypes.byref(o))
    assert o.min_count == 500.0 and o.num_iters == 40
    for name in ("DeviceFmllrStats", "fmllr_compute", "gmm_est_fmllr", "gmm_est_fmllr_batch", "transform_feats", "transform_feats_batch",
                 "compose_transforms", "utt2spk_ids", "spk2utt", "FMLLR_OK", "FMLLR_LOW_COUNT", "FMLLR_SINGULAR"):
        assert hasattr(khg, name), name
    assert hasattr(khg.UtteranceSet, "acc_fmllr_stats_post") and hasattr(khg.UtteranceSet, "transform_feats")
    assert hasattr(khg.DevicePosteriors, "from_alignment") and hasattr(khg.DeviceFmllrStats, "estimate")


def _round32(v):
    """the float32 nearest to the exact rational v (no tie occurs in the test's data)"""
    c = np.float32(float(v))
    cands = [float(np.nextafter(c, np.float32(-np.inf))), float(c), float(np.nextafter(c, np.float32(np.inf)))]
    return min(cands, key=lambda f: abs(v - Fraction(f)))


def test_compose_transforms_and_speaker_maps():
    import kaldi_hmm_gmm_amd as khg
    rng = np.random.default_rng(2)
    D = 6
    a = rng.standard_normal((D, D + 1)).astype(np.float32)
    b = rng.standard_normal((D, D + 1)).astype(np.float32)
    x = rng.standard_normal((9, D)).astype(np.float32)
    ab = khg.compose_transforms(a, b)
    want = khg.transform_feats(khg.transform_feats(x, b), a)
    np.testing.assert_allclose(khg.transform_feats(x, ab), want, rtol=1e-5, atol=1e-5)
    both = khg.compose_transforms(np.stack([a, b]), np.stack([b, a]))
    assert both.shape == (2, D, D + 1) and (both[0] == ab).all()
    # the host transform is the fmaf chain: against exact rational arithmetic rounded once per step
    y = khg.transform_feats(x[:2], a)
    for r in range(2):
        for d in range(D):
            acc = Fraction(float(a[d, D]))
            for j in range(D):
                acc = Fraction(_round32(Fraction(float(a[d, j])) * Fraction(float(x[r, j])) + acc))
            assert float(acc) == float(y[r, d])
    ids, names = khg.utt2spk_ids(["u1", "u2", "u3", "u4"], {"u1": "B", "u2": "A", "u3": "B"})
    assert ids.tolist() == [0, 1, 0, -1] and names == ["B", "A"] and khg.spk2utt(ids) == [[0, 2], [1]]
