"""MLLT without a GPU: the restatement's computed form (tests/mllt_ref.py) against the definition, the properties
of the row update, the host form khg_mllt_compute against the restatement on the bits, and the host gmm-transform-means against
exact rational arithmetic."""
import ctypes
from fractions import Fraction
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mllt_cases as cases  # noqa: E402
import mllt_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(1, 1, 60), (5, 3, 400), (13, 7, 800)]        # D, G, T


def _compute(beta, G, **kw):
    import kaldi_hmm_gmm_amd as khg
    return khg.mllt_compute(float(beta), np.ascontiguousarray(G, np.float64), **kw)


@pytest.mark.parametrize("off", [0.0, 50.0])
@pytest.mark.parametrize("D,G,T", CASES)
def test_computed_form_against_the_definition(D, G, T, off):
    """rtol 1e-9 plus, per d, atol 1e-9 x the largest magnitude among the shifted terms S[d] and C[d]; also with features and means
    offset by +50 in every dimension, where the terms it is measured against are still the shifted ones.  The bound holds because
    the frame side subtracts the shift in fp64, where the difference of two floats is exact: a float subtraction leaves ~1e-8 of
    max |S|."""
    c = cases.estimate_case(D, G, T, off)
    st = c["stats"]
    beta, Gd = ref.definition_stats(c["m"], c["gc"], c["feats"], c["posts"])
    assert beta > 0 and abs(st["beta"] - beta) <= 1e-9 * beta
    worst = 0.0
    for d in range(D):
        atol = 1e-9 * max(np.abs(st["S"][d]).max(), np.abs(st["C"][d]).max())
        worst = max(worst, float((np.abs(st["G"][d] - Gd[d]) / (atol + 1e-9 * np.abs(Gd[d]))).max()))
        np.testing.assert_allclose(st["G"][d], Gd[d], rtol=1e-9, atol=atol, err_msg="d = %d" % d)
    print("largest error / tolerance %.3g; max |S| / max |G| %.3g" % (worst, np.abs(st["S"]).max() / np.abs(Gd).max()))
    if off:
        # the same sums without the shift: the uncancelled terms the subtraction then has to survive
        raw = ref.acc_stats(c["m"], c["gc"], c["feats"], c["posts"], dtype=np.float64, use_shift=False)
        print("without the shift max |S| is %.3g x the shifted one" % (np.abs(raw["S"]).max() / np.abs(st["S"]).max()))
        assert np.abs(raw["S"]).max() > 4 * np.abs(st["S"]).max()


@pytest.mark.parametrize("D,G,T", CASES)
def test_host_form_equals_the_restatement_on_the_bits(D, G, T):
    """at the default 200 sweeps, and after 1 and 7"""
    st = cases.estimate_case(D, G, T)["stats"]
    for iters in (1, 7):
        assert _compute(st["beta"], st["G"], num_iters=iters)["M64"].tobytes() == ref.estimate(st["beta"], st["G"], num_iters=iters)["M"].tobytes()
    got = _compute(st["beta"], st["G"])
    r = ref.estimate(st["beta"], st["G"])
    assert got["status"] == r["status"] == ref.OK and got["count"] == st["beta"]
    assert got["M64"].tobytes() == r["M"].tobytes()
    assert got["M"].tobytes() == r["M"].astype(np.float32).tobytes()
    assert abs(got["objf_impr"] - r["objf_impr"]) <= 1e-12 * abs(r["objf_impr"]) + 1e-9      # the rounding of log
    assert r["objf_impr"] > 0


@pytest.mark.parametrize("D,G,T", CASES)
def test_q_never_falls_across_a_row_update(D, G, T):
    st = cases.estimate_case(D, G, T)["stats"]
    """every row update of the default 200 sweeps"""
    r = ref.estimate(st["beta"], st["G"], trace=True)
    q = [ref.auxf(st["beta"], st["G"], np.eye(D))] + r["q"]
    assert len(q) == 1 + 200 * D
    for a, b in zip(q, q[1:]):
        assert b >= a - 1e-9 * abs(a), (a, b)
    assert q[-1] > q[0]


@pytest.mark.parametrize("D,G,T", CASES)
def test_200_sweeps_are_no_worse_than_20(D, G, T):
    st = cases.estimate_case(D, G, T)["stats"]
    a, b = _compute(st["beta"], st["G"], num_iters=20), _compute(st["beta"], st["G"], num_iters=200)
    qa, qb = ref.auxf(st["beta"], st["G"], a["M64"]), ref.auxf(st["beta"], st["G"], b["M64"])
    assert qb >= qa and b["objf_impr"] >= a["objf_impr"]


def test_one_dimension_is_the_closed_form():
    st = cases.estimate_case(1, 1, 60)["stats"]
    want = math.sqrt(st["beta"] / st["G"][0, 0])
    for iters in (1, 200):
        got = _compute(st["beta"], st["G"], num_iters=iters)["M64"][0, 0]
        assert abs(got - want) <= math.ulp(want), (got, want)
    assert _compute(10.0, np.array([[2.5]]), num_iters=1)["M64"][0, 0] == 2.0


@pytest.mark.parametrize("D,G,T", CASES)
def test_true_likelihood_gain_is_at_least_the_q_gain(D, G, T):
    """EM: sum_t [ll(M x; means M mu) + log |det M| - ll(x)] >= Q(M) - Q(I).  The inequality is between exact quantities, so both
    sides are float64 (the statistics are the restatement's with float64 posteriors), slack 1e-9 of the gain."""
    c = cases.estimate_case(D, G, T)
    m, st = c["m"], c["stats"]
    r = ref.estimate(st["beta"], st["G"], num_iters=20)
    M = r["M"]
    logdet = np.linalg.slogdet(M)[1]
    mu, iv, w = ref.means(m).astype(np.float64), m.inv_vars.astype(np.float64), m.weights.astype(np.float64)
    gain = 0.0
    for u, x in enumerate(c["feats"]):
        x = x.astype(np.float64)
        pd = np.array(c["pdfs"][u])
        for p in set(c["pdfs"][u]):
            g0, g1 = int(m.gauss_off[p]), int(m.gauss_off[p + 1])
            sel = pd == p
            gain += (ref.loglike64(w[g0:g1], mu[g0:g1] @ M.T, iv[g0:g1], x[sel] @ M.T) - ref.loglike64(w[g0:g1], mu[g0:g1], iv[g0:g1], x[sel])).sum()
            gain += sel.sum() * logdet
    print("gain %.6f objf_impr %.6f" % (gain, r["objf_impr"]))
    assert r["objf_impr"] > 0 and gain >= r["objf_impr"] - 1e-9 * abs(gain)


def test_singular_and_refusals():
    import kaldi_hmm_gmm_amd as khg
    from kaldi_hmm_gmm_amd import _lib
    # fewer than D frames of integer data: every G[d] = sum of 3 outer products has rank 3 < 5, the elimination stays exact and the
    # fourth pivot is exactly 0
    D = 5
    xs = np.array([[1, 2, 0, 1, 2], [2, 1, 1, 0, 1], [0, 1, 2, 2, 1]], np.float64)
    il, jl = np.tril_indices(D)
    G1 = np.stack([(xs.T @ xs)[il, jl]] * D)
    got = _compute(3.0, G1)
    assert got["status"] == khg.MLLT_SINGULAR == ref.SINGULAR and (got["M64"] == np.eye(D)).all() and (got["M"] == np.eye(D)).all()
    assert got["count"] == 3.0 and got["objf_impr"] == 0.0
    assert ref.estimate(3.0, G1)["status"] == ref.SINGULAR
    st = cases.estimate_case(5, 3, 400)["stats"]
    assert _compute(0.0, st["G"])["status"] == khg.MLLT_SINGULAR and ref.estimate(0.0, st["G"])["status"] == ref.SINGULAR
    with pytest.raises(Exception):
        _compute(st["beta"], st["G"], num_iters=-1)
    with pytest.raises(Exception):
        _compute(st["beta"], st["G"][:, :-1])                          # G of another shape
    lib = _lib.lib
    f64 = ctypes.POINTER(ctypes.c_double)
    g = np.ascontiguousarray(st["G"])
    M = np.zeros((5, 5), np.float32)
    pM = M.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    assert lib.khg_mllt_compute(None, 5, st["beta"], g.ctypes.data_as(f64), None, None, None, None, None) == -1      # nowhere to put M
    assert b"khg_mllt_compute" in lib.khg_last_error()
    assert lib.khg_mllt_compute(None, 81, st["beta"], g.ctypes.data_as(f64), pM, None, None, None, None) == -4       # above KHG_MLLT_MAX_DIM
    o = _lib.MlltOptionsC(-1)
    assert lib.khg_mllt_compute(ctypes.byref(o), 5, st["beta"], g.ctypes.data_as(f64), pM, None, None, None, None) == -1
    assert lib.khg_mllt_compute(None, 5, st["beta"], g.ctypes.data_as(f64), pM, None, None, None, None) == 0 and M.any()
    # the device entry points refuse a dead context before anything else
    assert lib.khg_mllt_stats_create(None, 5, ctypes.byref(ctypes.c_void_p())) == -1
    assert lib.khg_acc_mllt_stats_post(None, None, None, None, None, 1.0, None) == -1
    assert lib.khg_model_transform_means(None, None, None) == -1


def test_new_symbols_are_exported():
    from kaldi_hmm_gmm_amd import _lib
    import kaldi_hmm_gmm_amd as khg
    with open(os.path.join(ROOT, "include", "khg_hip.h")) as fh:
        header = fh.read()
    for name in ("khg_mllt_stats_create", "khg_mllt_stats_destroy", "khg_mllt_stats_zero", "khg_mllt_stats_download", "khg_mllt_stats_upload",
                 "khg_mllt_stats_add", "khg_mllt_stats_set_chunk_frames", "khg_mllt_stats_num_chunks", "khg_acc_mllt_stats_post",
                 "khg_mllt_compute", "khg_model_transform_means"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.SIGNATURES and getattr(_lib.lib, name) is not None, name
    assert "#define KHG_MLLT_MAX_DIM 80" in header
    o = _lib.MlltOptionsC()
    _lib.lib.khg_mllt_options_default(ctypes.byref(o))
    assert o.num_iters == 200
    for name in ("DeviceMlltStats", "mllt_compute", "gmm_acc_mllt", "gmm_acc_mllt_batch", "est_mllt", "gmm_transform_means", "MLLT_OK",
                 "MLLT_SINGULAR", "MLLT_MAX_DIM"):
        assert hasattr(khg, name), name
    assert hasattr(khg.UtteranceSet, "acc_mllt_stats_post") and hasattr(khg.DeviceModel, "transform_means")
    assert hasattr(khg.AmDiagGmm, "transform_means") and hasattr(khg.DiagGmm, "transform_means")
    for meth in ("download", "upload", "add", "zero", "set_chunk_frames"):
        assert hasattr(khg.DeviceMlltStats, meth), meth


def _round32(v):
    """the float32 nearest to the exact rational v (no tie occurs in the test's data)"""
    c = np.float32(float(v))
    cands = [float(np.nextafter(c, np.float32(-np.inf))), float(c), float(np.nextafter(c, np.float32(np.inf)))]
    return min(cands, key=lambda f: abs(v - Fraction(f)))


def test_host_transform_means_is_the_fmaf_chain():
    """means_invvars against exact rational arithmetic rounded once per step; weights and inv_vars keep their bits; est_mllt's W"""
    import kaldi_hmm_gmm_amd as khg
    m = cases.estimate_case(5, 3, 400)["m"]
    D = 5
    M = np.random.default_rng(1).standard_normal((D, D)).astype(np.float32)
    am = cases.host_am(m)
    go, gc0, w0, miv0, iv0 = am.flat()
    khg.gmm_transform_means(M, am_gmm=am)
    go, gc1, w1, miv1, iv1 = am.flat()
    assert np.asarray(w1).tobytes() == np.asarray(w0).tobytes() and np.asarray(iv1).tobytes() == np.asarray(iv0).tobytes()
    assert np.asarray(miv1).tobytes() == ref.transform_means(miv0, iv0, M).tobytes()
    assert np.asarray(gc1).tobytes() != np.asarray(gc0).tobytes()
    miv0, iv0, miv1 = np.asarray(miv0), np.asarray(iv0), np.asarray(miv1)
    for g in range(4):
        mu = [Fraction(_round32(Fraction(float(miv0[g, j])) / Fraction(float(iv0[g, j])))) for j in range(D)]
        for d in range(D):
            acc = Fraction(0)
            for j in range(D):
                acc = Fraction(_round32(Fraction(float(M[d, j])) * mu[j] + acc))
            assert _round32(acc * Fraction(float(iv0[g, d]))) == float(miv1[g, d]), (g, d)
    # one pdf alone gives the same rows
    one = cases.host_am(m).get_pdf(1)
    one.transform_means(M)
    a, b = int(m.gauss_off[1]), int(m.gauss_off[2])
    assert np.asarray(one._means_invvars).tobytes() == miv1[a:b].tobytes()
    with pytest.raises(Exception):
        am.transform_means(M[:, :-1])
    with pytest.raises(ValueError, match="dim, dim"):               # an affine transform is refused, its offset not dropped
        khg.gmm_transform_means(np.concatenate([M, np.ones((D, 1), np.float32)], 1), am_gmm=am)
    assert np.asarray(am.flat()[3]).tobytes() == miv1.tobytes()
    # est_mllt: W = [M | 0], and with prev= the composition that applies prev first
    st = cases.estimate_case(5, 3, 400)["stats"]
    r = khg.est_mllt({"beta": st["beta"], "G": st["G"]}, num_iters=5)
    assert r["status"] == khg.MLLT_OK and r["count"] == st["beta"] and (r["W"][:, :D] == r["M"]).all() and not r["W"][:, D].any()
    prev = np.concatenate([M, np.ones((D, 1), np.float32)], 1)
    r2 = khg.est_mllt({"beta": st["beta"], "G": st["G"]}, num_iters=5, prev=prev)
    assert r2["W"].tobytes() == khg.compose_transforms(r["W"], prev).tobytes()


def test_identity_leaves_the_means_within_one_ulp():
    """M = I: y = mu exactly (fmaf(1, mu, 0) and fmaf(0, ., y) are exact), but the round trip (miv / iv) * iv is two roundings and is
    NOT exact: within one float ulp, and not always equal"""
    m = cases.estimate_case(13, 7, 800)["m"]
    am = cases.host_am(m)
    _, _, _, miv0, _ = am.flat()
    am.transform_means(np.eye(13, dtype=np.float32))
    _, _, _, miv1, _ = am.flat()
    miv0, miv1 = np.asarray(miv0), np.asarray(miv1)
    assert (np.abs(miv1 - miv0) <= np.spacing(np.abs(miv0))).all()
