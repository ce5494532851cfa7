"""The Extended Baum-Welch update without a GPU: the restatement tests/ebw_ref.py checked against itself through
invariants, the host C++ form (khg_ebw_am_diag_gmm_update) against the restatement, the host classes, and the three accumulator
operations against numpy.

Stated tolerances: weights / inv_vars / means_invvars and every counter are BIT-EQUAL between the host form and the restatement; gconsts
go through logf (GC_ULPS = 4, as for the ML update); the two diagnostics within n_terms 2^-50 sum |term| (a one-ulp log and a
reordered fp64 sum).  Observed on this suite: both diagnostics of the host form are bit-equal to the restatement's (the same libm log,
the same order): 0 of the bound."""
import math

import numpy as np
import pytest

import kaldi_hmm_gmm_amd as khg
from kaldi_hmm_gmm_amd import mle as khg_mle

import ebw_cases
import ebw_ref
from ebw_cases import FLAGS, SHAPES

GC_ULPS = 4
F64 = np.float64


def _host(shape, flags, E=2.0):
    m, num, den = ebw_cases.fabricate(shape)
    return khg_mle._flat_ebw_update(khg.EbwOptions(E=E), khg.EbwWeightOptions(), m.gauss_off, num, den, FLAGS[flags], m.weights, m.means_invvars,
                                    m.inv_vars)


@pytest.mark.parametrize("flags", list(FLAGS))
@pytest.mark.parametrize("shape", SHAPES)
def test_host_form_vs_restatement(shape, flags):
    ref = ebw_cases.reference(shape, flags)
    w, gc, miv, iv, res = _host(shape, flags)
    ebw_cases.check_against_reference(w, gc, miv, iv, res, ref, GC_ULPS)
    m, _, _ = ebw_cases.fabricate(shape)
    if not FLAGS[flags] & 4:
        np.testing.assert_array_equal(w, m.weights)
    if not FLAGS[flags] & 2:
        np.testing.assert_array_equal(iv, m.inv_vars)
    if not FLAGS[flags] & 3:
        np.testing.assert_array_equal(miv, m.means_invvars)


@pytest.mark.parametrize("shape", SHAPES[:3])
def test_every_branch_occurs(shape):
    """The fabricated blocks reach every branch of the rule (asserted on the restatement's own records)."""
    ref = ebw_cases.reference(shape, "mvw")
    g = ref["gauss"]
    ok = [o for o in g if o["status"] == "ok"]
    assert any(o["iters"] == 0 for o in ok), "first-try success"
    assert any(o["iters"] > 0 for o in ok) and ref["floored"] > 0, "iter > 0"
    assert any(o.get("branch_neg") for o in ok), "D + occ <= 0 at E = 2 (occ_n = 0)"
    assert ref["skipped"] > 0 and ref["failed"] > 0
    assert ref["weights_skipped"] > 0 and ref["weights_skipped"] < shape[0]
    assert any(p["status"] == "ok" and p["floored"] > 0 for p in ref["pdfs"]), "a weight on the floor"
    # E = 0.5: D = occ_d / 4 < occ_d - occ_n for Gaussians whose numerator count is positive
    ref05 = ebw_cases.reference(shape, "mv", E=0.5)
    num_occ = ebw_cases.fabricate(shape)[1][0]
    assert any(o.get("branch_neg") and o["status"] == "ok" and num_occ[i] > 0 for i, o in enumerate(ref05["gauss"])), "D + occ <= 0 at E = 0.5"
    w, gc, miv, iv, res = _host(shape, "mv", E=0.5)
    ebw_cases.check_against_reference(w, gc, miv, iv, res, ref05, GC_ULPS)
    # the skipped and the failed Gaussians keep their bits
    m, _, _ = ebw_cases.fabricate(shape)
    for i, o in enumerate(g):
        if o["status"] != "ok":
            np.testing.assert_array_equal(ref["inv_vars"][i], m.inv_vars[i])
            np.testing.assert_array_equal(ref["means_invvars"][i], m.means_invvars[i])


def test_one_gaussian_one_dimension_model():
    ref = ebw_cases.reference(SHAPES[3], "mvw")
    assert ref["skipped"] == 1 and ref["floored"] >= 1 and ref["failed"] == 0 and ref["gauss"][1]["iters"] > 0


# ---- the restatement against itself ---------------------------------------------------------------------------------------------
def _one(rng, D):
    mu = rng.standard_normal(D) * 2
    var = rng.uniform(0.5, 2.0, D)
    iv = (1 / var).astype(np.float32)
    miv = (mu * iv).astype(np.float32)
    return miv, iv


def test_zero_denominator_is_the_ml_update():
    """den = 0, tau = 0: D = 0 succeeds at once and the committed values are the closed-form ML mean and variance."""
    rng = np.random.default_rng(3)
    D = 9
    for _ in range(20):
        miv, iv = _one(rng, D)
        occ = rng.uniform(5, 50)
        m_ml = rng.standard_normal(D)
        v_ml = rng.uniform(0.3, 2.0, D)
        x, x2 = occ * m_ml, occ * (v_ml + m_ml * m_ml)
        o = ebw_ref.ebw_gauss(3, 2.0, 0.0, occ, x, x2, 0.0, np.zeros(D), np.zeros(D), miv, iv)
        assert o["status"] == "ok" and o["iters"] == 0 and o["D_committed"] == 0.0
        np.testing.assert_allclose(np.asarray(o["mu_new"]), x / occ, rtol=1e-12, atol=0)
        np.testing.assert_allclose(np.asarray(o["var_new"]), x2 / occ - (x / occ) ** 2, rtol=1e-12, atol=1e-12 * np.abs(x2 / occ).max())


@pytest.mark.parametrize("flags", ["m", "v", "mv"])
def test_auxf_improvement_is_never_negative(flags):
    """The committed values maximise Q on the smoothed statistics, so Q(new) - Q(old) >= 0 to rounding, for every Gaussian of every
    fabricated block."""
    n = 0
    for shape in SHAPES:
        for o in ebw_cases.reference(shape, flags)["gauss"]:
            if o["status"] == "ok":
                assert float(o["impr"]) >= -1e-9 * float(o["abs_terms"]), (shape, float(o["impr"]), float(o["abs_terms"]))
                n += 1
    assert n > 100


def test_zero_numerator_moves_means_away_from_the_denominator():
    rng = np.random.default_rng(5)
    D = 7
    for _ in range(20):
        miv, iv = _one(rng, D)
        mu, var = ebw_ref.normal_form(miv, iv)
        occ_d = rng.uniform(5, 50)
        m_d = np.asarray(mu) + rng.standard_normal(D)
        x_d, x2_d = occ_d * m_d, occ_d * (np.asarray(var) + m_d * m_d)
        o = ebw_ref.ebw_gauss(3, 2.0, 0.0, 0.0, np.zeros(D), np.zeros(D), occ_d, x_d, x2_d, miv, iv)
        assert o["status"] == "ok" and o["branch_neg"]
        step = np.asarray(o["mu_new"]) - np.asarray(mu)
        pull = x_d / occ_d - np.asarray(mu)
        assert (np.sign(step) == -np.sign(pull)).all()


def test_search_brackets_the_first_feasible_constant():
    """iter > 0: try fails at the last rejected D and succeeds at the accepted one (and at the committed, doubled one)."""
    n = 0
    for shape in SHAPES[:2]:
        m, num, den = ebw_cases.fabricate(shape)
        for g, o in enumerate(ebw_cases.reference(shape, "mv")["gauss"]):
            if o["status"] != "ok" or o["iters"] == 0:
                continue
            mu, var = ebw_ref.normal_form(m.means_invvars[g], m.inv_vars[g])
            occ = F64(num[0][g]) - F64(den[0][g])
            x = [F64(a) - F64(b) for a, b in zip(num[1][g], den[1][g])]
            x2 = [F64(a) - F64(b) for a, b in zip(num[2][g], den[2][g])]
            assert not ebw_ref.try_d(o["D_rejected"], 3, occ, x, x2, mu, var)[0]
            assert ebw_ref.try_d(o["D_accepted"], 3, occ, x, x2, mu, var)[0]
            assert ebw_ref.try_d(o["D_committed"], 3, occ, x, x2, mu, var)[0]
            assert o["D_accepted"] == F64(1.1) * o["D_rejected"]
            n += 1
    assert n >= 5


def test_weights_are_normalised_and_floored():
    n = 0
    for shape in SHAPES[:3]:
        for p in ebw_cases.reference(shape, "w")["pdfs"]:
            if p["status"] != "ok":
                continue
            w = np.asarray(p["w_new"], np.float64)
            assert abs(math.fsum(w) - 1.0) <= 1e-12
            assert (w >= ebw_ref.W_MIN_WEIGHT / float(p["last_sum"])).all()
            n += 1
    assert n > 20


# ---- the host classes -----------------------------------------------------------------------------------------------------------
def test_host_classes_match_the_flat_form():
    shape = SHAPES[0]
    m, num, den = ebw_cases.fabricate(shape)
    from kaldi_hmm_gmm_amd import synth
    am, _ = synth.host_objects(m)
    accs = []
    for blk in (num, den):
        a = khg.AccumAmDiagGmm()
        a.init(am, khg.GmmUpdateFlags.kGmmAll)
        for p in range(am.num_pdfs):
            lo, hi = int(m.gauss_off[p]), int(m.gauss_off[p + 1])
            a._accs[p].occupancy[:] = blk[0][lo:hi]
            a._accs[p].mean_accumulator[:] = blk[1][lo:hi]
            a._accs[p].variance_accumulator[:] = blk[2][lo:hi]
        accs.append(a)
    ref_mv = ebw_cases.reference(shape, "mv")
    ref_w = ebw_cases.reference(shape, "w")
    # whole model: gmm_est_gmm_ebw then gmm_est_weights_ebw
    am2 = khg.AmDiagGmm(); am2.copy_from_am_diag_gmm(am)
    r = khg.gmm_est_gmm_ebw(am2, accs[0], accs[1], khg.EbwOptions(), update_flags="mv", verbose=False)
    assert (r["floored"], r["failed"], r["skipped"]) == (ref_mv["floored"], ref_mv["failed"], ref_mv["skipped"])
    r = khg.gmm_est_weights_ebw(am2, accs[0], accs[1], verbose=False)
    assert r["weights_skipped"] == ref_w["weights_skipped"]
    go, gc, w, miv, iv = am2.flat()
    np.testing.assert_array_equal(w, ref_w["weights"])
    np.testing.assert_array_equal(miv, ref_mv["means_invvars"])
    np.testing.assert_array_equal(iv, ref_mv["inv_vars"])
    # one pdf through the per-pdf functions
    g = khg.DiagGmm(gmm=am.get_pdf(3))
    r = khg.update_ebw_diag_gmm(accs[0].get_acc(3), accs[1].get_acc(3), 3, khg.EbwOptions(), g)
    khg.update_ebw_weights_diag_gmm(accs[0].get_acc(3), accs[1].get_acc(3), khg.EbwWeightOptions(), g)
    lo, hi = int(m.gauss_off[3]), int(m.gauss_off[4])
    np.testing.assert_array_equal(g.inv_vars, ref_mv["inv_vars"][lo:hi])
    np.testing.assert_array_equal(g.weights, ref_w["weights"][lo:hi])
    cnt = F64(0.0)
    for v in num[0][lo:hi]:
        cnt = cnt + F64(v)
    assert g.valid_gconsts and r["count"] == float(cnt)
    with pytest.raises(khg.KhgError, match="not finite"):
        khg.update_ebw_diag_gmm(accs[0].get_acc(3), accs[1].get_acc(3), 3, khg.EbwOptions(E=float("nan")), g)
    with pytest.raises(khg.KhgError):
        khg.update_ebw_diag_gmm(accs[0].get_acc(3), accs[1].get_acc(2), 3, khg.EbwOptions(), khg.DiagGmm(nmix=2, dim=m.dim))


# ---- the accumulator operations -------------------------------------------------------------------------------------------------
def test_accumulator_operations_vs_numpy():
    """The restatement's add / scale / smooth_with_accum == the host classes' (AccumDiagGmm::Add / Scale / SmoothWithAccum) bit for bit,
    and gmm_sum_accs / gmm_ismooth_stats over whole accumulators."""
    shape = SHAPES[0]
    m, num, den = ebw_cases.fabricate(shape)
    from kaldi_hmm_gmm_amd import synth
    am, _ = synth.host_objects(m)

    def accs_of(blk):
        a = khg.AccumAmDiagGmm()
        a.init(am, khg.GmmUpdateFlags.kGmmAll)
        for p in range(am.num_pdfs):
            lo, hi = int(m.gauss_off[p]), int(m.gauss_off[p + 1])
            a._accs[p].occupancy[:] = blk[0][lo:hi]
            a._accs[p].mean_accumulator[:] = blk[1][lo:hi]
            a._accs[p].variance_accumulator[:] = blk[2][lo:hi]
        return a

    def flat(a):
        return (np.concatenate([a.get_acc(p).occupancy for p in range(a.num_accs)]),
                np.concatenate([a.get_acc(p).mean_accumulator for p in range(a.num_accs)]),
                np.concatenate([a.get_acc(p).variance_accumulator for p in range(a.num_accs)]))

    a, b = accs_of(num), accs_of(den)
    tot, tacc = khg.gmm_sum_accs([a, b], [np.arange(5.0), np.ones(5)])
    assert tot is a and np.array_equal(tacc, np.arange(5.0) + 1)
    for got, x, y in zip(flat(a), num, den):
        np.testing.assert_array_equal(got, ebw_ref.accs_add(np.asarray(x), 1.0, np.asarray(y)))
    a = accs_of(num)
    a.add(-0.3, b)
    for got, x, y in zip(flat(a), num, den):
        np.testing.assert_array_equal(got, ebw_ref.accs_add(np.asarray(x), -0.3, np.asarray(y)))
    a = accs_of(num)
    a.scale(0.7)
    for got, x in zip(flat(a), num):
        np.testing.assert_array_equal(got, ebw_ref.accs_scale(np.asarray(x), 0.7))
    # smoothing: from another block (zero-occupancy sources are left alone) and from itself
    a = accs_of(num)
    khg.gmm_ismooth_stats(a, 25.0, b)
    occ, mean, var, untouched = ebw_ref.accs_smooth_with_accum(num[0], num[1], num[2], 25.0, den[0], den[1], den[2])
    assert untouched == int((den[0] == 0).sum()) > 0
    for got, want in zip(flat(a), (occ, mean, var)):
        np.testing.assert_array_equal(got, want)
    a = accs_of(num)
    khg.gmm_ismooth_stats(a, 10.0)
    occ, mean, var, untouched = ebw_ref.accs_smooth_with_accum(num[0], num[1], num[2], 10.0, num[0], num[1], num[2])
    for got, want in zip(flat(a), (occ, mean, var)):
        np.testing.assert_array_equal(got, want)
    nz = num[0] != 0
    np.testing.assert_allclose(mean[nz] / occ[nz, None], num[1][nz] / num[0][nz, None], rtol=1e-12)    # the means do not move
