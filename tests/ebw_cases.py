"""Fabricated numerator / denominator blocks for the Extended Baum-Welch tests (CPU and GPU), built so that every branch of the rule
in DESIGN.md 7i occurs, and the reference results (tests/ebw_ref.py) computed once per (shape, flags, E) and shared.

Branch of Gaussian g by its index k inside its pdf (pdfs with fewer Gaussians see fewer branches; the tests assert the union):
  k % 9 == 1   denominator second-order statistics 30 x the model variance at occ_n == occ_d: a variance is negative at the first
               D = E occ_d / 2, so the search needs iter > 0;
  k % 9 == 3   occ_n = 0 with a large occ_d: D + occ <= 0 at E = 2; its weight also ends on the floor;
  k % 9 == 5   occ_n = occ_d = 0: skipped;
  k == min(7, Gmax - 1)   x2 so negative that 1.1^100 cannot repair it: the loop is exhausted (failed);
and every pdf with p % 5 == 4 has numerator counts that sum below min_num_count_weight_update.
"""
import numpy as np

from kaldi_hmm_gmm_amd import synth

import ebw_ref

SHAPES = [(23, 7, 13, False), (40, 12, 40, True), (6, 70, 80, True), (3, 1, 1, False)]
FLAGS = {"m": 1, "v": 2, "mv": 3, "w": 4, "mvw": 7}

_cache = {}


def fabricate(shape):
    """-> (model, num, den) with num / den = (occ[G], x[G, D], x2[G, D]) fp64."""
    key = ("fab",) + tuple(shape)
    if key in _cache:
        return _cache[key]
    P, Gmax, D, ragged = shape
    m = synth.make_model(P, Gmax, D, seed=31 + P, ragged=ragged)
    rng = np.random.default_rng(170 + P)
    G = int(m.gauss_off[-1])
    mean = m.means.astype(np.float64)
    var = m.vars.astype(np.float64)
    occ_n = rng.uniform(0.5, 2.0, G) * 40.0
    occ_d = rng.uniform(0.2, 1.2, G) * 40.0
    mu_n = mean + 0.3 * rng.standard_normal((G, D))
    mu_d = mean + 0.5 * rng.standard_normal((G, D))
    var_n = var * rng.uniform(0.7, 1.4, (G, D))
    var_d = var * rng.uniform(0.7, 1.6, (G, D))
    x2_extra = np.zeros((G, D))
    for p in range(P):
        a, b = int(m.gauss_off[p]), int(m.gauss_off[p + 1])
        for g in range(a, b):
            k = g - a if Gmax > 1 else p          # one Gaussian per pdf: the pdf index picks the branch
            if k % 9 == 1:
                occ_d[g] = occ_n[g]
                var_d[g] = 30.0 * var[g]
            elif k % 9 == 3:
                occ_n[g] = 0.0
                occ_d[g] = 60.0
            elif k % 9 == 5 or (Gmax == 1 and k == 2):
                occ_n[g] = 0.0
                occ_d[g] = 0.0
            elif Gmax > 1 and k == min(7, Gmax - 1):
                x2_extra[g] = 1e7 * var[g] * occ_d[g]
        if p % 5 == 4 and Gmax > 1:
            occ_n[a:b] = 0.5 / (b - a) * rng.uniform(0.5, 1.0, b - a)
    num = (occ_n, occ_n[:, None] * mu_n, occ_n[:, None] * (var_n + mu_n * mu_n))
    den = (occ_d, occ_d[:, None] * mu_d, occ_d[:, None] * (var_d + mu_d * mu_d) + x2_extra)
    _cache[key] = (m, num, den)
    return _cache[key]


def reference(shape, flags, E=2.0):
    """tests/ebw_ref.py on the fabricated blocks of `shape`, once."""
    key = ("ref",) + tuple(shape) + (flags, E)
    if key not in _cache:
        m, num, den = fabricate(shape)
        _cache[key] = ebw_ref.ebw_update(m.gauss_off, m.weights, m.means_invvars, m.inv_vars, num, den, FLAGS[flags], E=E)
    return _cache[key]


def ulps32(a, b):
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32))


def diag_bound(n_terms, abs_terms):
    """What a one-ulp log and a reordered fp64 sum can move a diagnostic by: n_terms 2^-50 sum |term|."""
    return float(n_terms) * 2.0 ** -50 * float(abs_terms)


def check_against_reference(got_w, got_gc, got_miv, got_iv, res, ref, gc_ulps=4):
    """Parameters and counters bit-equal to the restatement, gconsts within gc_ulps, diagnostics within diag_bound.
    -> the worst observed fraction of the diagnostics' bound."""
    np.testing.assert_array_equal(got_w, ref["weights"], err_msg="weights")
    np.testing.assert_array_equal(got_iv, ref["inv_vars"], err_msg="inv_vars")
    np.testing.assert_array_equal(got_miv, ref["means_invvars"], err_msg="means_invvars")
    for k in ("floored", "failed", "skipped", "weights_skipped"):
        assert res[k] == ref[k], (k, res[k], ref[k])
    assert res["count"] == float(ref["count"])
    assert np.isfinite(np.asarray(got_gc)).all() and np.isfinite(ref["gconsts"]).all()
    u = ulps32(got_gc, ref["gconsts"])
    assert u.max() <= gc_ulps, u.max()
    worst = 0.0
    for name, n, ab in (("auxf_impr_gauss", ref["n_gauss"], ref["abs_gauss"]), ("auxf_impr_weights", ref["n_weights"], ref["abs_weights"])):
        err = abs(res[name] - float(ref[name]))
        bound = diag_bound(n, ab)
        print("%s: got %.17g want %.17g |err| %.3g bound %.3g" % (name, res[name], float(ref[name]), err, bound))
        assert err <= bound, (name, err, bound)
        if bound > 0:
            worst = max(worst, err / bound)
    return worst
