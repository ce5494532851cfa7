"""LDA without a GPU: the host estimate khg_lda_compute against the numpy restatement (tests/lda_ref.py) and its
own invariants, the statuses and refusals, the exported names, and the host forms of splice-feats / transform-feats / compose.

Tolerances of the estimate.  On the four cases below the host form's deviation and the restatement's own residuals were measured
(DESIGN.md 7n has the table); TOL holds 10 x the larger of the two per case and quantity, and every one of them is checked to lie
under the cap Dz 2^-40 max(1, lambda_max), beyond which the solver would not have converged.  Where both measured values were exactly
zero ((2, 1): every operation is exact or rounds alike), 10 ulps of 1 stand in: what evaluating the residual itself resolves."""
import ctypes
from fractions import Fraction
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lda_cases as cases  # noqa: E402
import lda_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = cases.ESTIMATE_CASES
# measured (host deviation, restatement's residual) -> 10 x the larger:   eig: |eig - eigvalsh(P)|;  W: |M Wc M^T - I|;  B: |M Bc M^T - diag|
TOL = {
    (2, 1): dict(eig=2.3e-15, W=2.3e-15, B=2.3e-15),          # (0, 0), (2.2e-16, 2.2e-16), (0, 0)
    (3, 5): dict(eig=6.8e-13, W=2.0e-14, B=7.2e-14),          # (6.8e-14, -), (2.0e-15, 4.6e-16), (7.1e-15, 6.3e-15)
    (7, 17): dict(eig=3.6e-14, W=5.6e-14, B=6.1e-13),         # (3.6e-15, -), (5.6e-15, 1.1e-15), (6.0e-14, 7.1e-15)
    (12, 117): dict(eig=1.5e-12, W=3.6e-13, B=1.6e-11),       # (1.4e-13, -), (3.5e-14, 2.8e-15), (1.5e-12, 4.3e-14)
}
GAP = 1e-3


def _compute(c, **kw):
    import kaldi_hmm_gmm_amd as khg
    return khg.lda_compute(c["zero"], c["first"], c["packed"], **kw)


def _separated(lam):
    """rows whose eigenvalue is at least GAP lambda_max away from both neighbours, and that distance"""
    n, lmax = len(lam), lam[0]
    out = {}
    for i in range(n):
        g = min(lam[i - 1] - lam[i] if i else np.inf, lam[i] - lam[i + 1] if i + 1 < n else np.inf)
        if g >= GAP * lmax:
            out[i] = g
    return out


def _projector(M):
    q = np.linalg.qr(np.asarray(M, np.float64).T)[0]
    return q @ q.T


@pytest.mark.parametrize("C,Dz,td", CASES)
def test_host_estimate_against_the_restatement(C, Dz, td):
    """eigenvalues, the two residuals, the order, the separated rows after the canonical sign, the projector onto the kept rows"""
    import kaldi_hmm_gmm_amd as khg
    c = cases.estimate_case(C, Dz)
    r = ref.estimate(c["zero"], c["first"], c["second"], td)
    Wc, Bc, lam = r["Wc"], r["Bc"], r["eig"]
    assert np.linalg.cond(Wc) <= 1e4                           # the restatement itself stays inside the tolerances
    g = _compute(c, target_dim=td)
    assert g["status"] == khg.LDA_OK == ref.OK and g["count"] == c["zero"].sum()
    assert g["M"].shape == (td, Dz) and g["M"].dtype == np.float32 and g["M"].tobytes() == g["M64"].astype(np.float32).tobytes()
    assert g["M64"].tobytes() == g["M_full"][:td].tobytes()
    tol, cap = TOL[(C, Dz)], Dz * 2.0 ** -40 * max(1.0, lam[0])
    assert max(tol.values()) <= cap
    Mf, eig = g["M_full"], g["eig"]
    d_eig = np.abs(eig - np.linalg.eigvalsh(r["P"])[::-1]).max()
    d_w = np.abs(Mf @ Wc @ Mf.T - np.eye(Dz)).max()
    d_b = np.abs(Mf @ Bc @ Mf.T - np.diag(eig)).max()
    n_w = np.abs(r["M_full"] @ Wc @ r["M_full"].T - np.eye(Dz)).max()
    n_b = np.abs(r["M_full"] @ Bc @ r["M_full"].T - np.diag(lam)).max()
    print("(%d, %d): eig %.3g; host residuals W %.3g B %.3g; restatement's W %.3g B %.3g; cap %.3g" % (C, Dz, d_eig, d_w, d_b, n_w, n_b, cap))
    assert d_eig <= tol["eig"] and d_w <= tol["W"] and d_b <= tol["B"]
    assert (np.diff(eig) <= 0).all()
    sep = _separated(lam)
    assert len([i for i in sep if i < td]) >= td - 1
    # a row with an isolated eigenvalue is determined up to (backward error of the two decompositions) / gap, relative to its length
    for i, gap in sep.items():
        bound = 4 * tol["B"] / gap * max(1.0, np.linalg.norm(r["M_full"][i]))
        assert np.abs(Mf[i] - r["M_full"][i]).max() <= bound, (i, gap)
        j = int(np.argmax(np.abs(Mf[i])))
        assert Mf[i, j] > 0                                    # the canonical sign
    if td < Dz:
        gap = lam[td - 1] - lam[td]
        assert gap >= GAP * lam[0]
        assert np.abs(_projector(g["M64"]) - _projector(r["M"])).max() <= 4 * tol["B"] / gap


@pytest.mark.parametrize("C,Dz,td", CASES)
def test_within_class_factor_and_remove_offset(C, Dz, td):
    c = cases.estimate_case(C, Dz)
    r = ref.estimate(c["zero"], c["first"], c["second"], td)
    tol = TOL[(C, Dz)]
    g = _compute(c, target_dim=td, within_class_factor=0.5)
    Mf, lam = g["M_full"], g["eig"]
    var = np.diag(Mf @ r["Wc"] @ Mf.T)
    assert np.abs(var - (0.5 + lam) / (1.0 + lam)).max() <= tol["W"]
    assert g["eig"].tobytes() == _compute(c, target_dim=td)["eig"].tobytes()
    g = _compute(c, target_dim=td, remove_offset=True)
    assert g["M"].shape == (td, Dz + 1) and g["M64"][:, :Dz].tobytes() == _compute(c, target_dim=td)["M64"].tobytes()
    mu1 = np.concatenate([r["mu"], [1.0]])
    bound = (Dz + 2) * 2.0 ** -52 * (np.abs(g["M64"]) @ np.abs(mu1))      # the rounding of a (Dz + 1)-term dot product, twice
    assert (np.abs(g["M64"] @ mu1) <= bound + 1e-300).all()
    assert g["M"].tobytes() == g["M64"].astype(np.float32).tobytes()


def test_singular_statuses():
    import kaldi_hmm_gmm_amd as khg
    c = cases.estimate_case(3, 5)
    g = khg.lda_compute(np.zeros(3), c["first"], c["packed"], target_dim=2, remove_offset=True)          # N = 0
    assert g["status"] == khg.LDA_SINGULAR == ref.SINGULAR and g["count"] == 0.0
    assert (g["M64"] == np.eye(2, 6)).all() and (g["M"] == np.eye(2, 6)).all() and (g["M_full"] == np.eye(5)).all() and not g["eig"].any()
    assert ref.estimate(np.zeros(3), c["first"], c["second"], 2)["status"] == ref.SINGULAR
    # fewer frames than Dz of integer data: Wc has rank <= 3 < 5 and its elimination stays exact (every value is a small dyadic
    # rational: N = 4), so a pivot is exactly 0
    xs = np.array([[1, 2, 0, 1, 2], [3, 2, 0, 1, 2], [0, 1, 2, 2, 1], [2, 1, 4, 2, 1]], np.float64)
    cls = np.array([0, 0, 1, 1])
    zero = np.array([2.0, 2.0])
    first = np.stack([xs[cls == k].sum(0) for k in range(2)])
    g = khg.lda_compute(zero, first, ref.packed(xs.T @ xs), target_dim=3)
    assert g["status"] == khg.LDA_SINGULAR and (g["M64"] == np.eye(3, 5)).all() and g["count"] == 4.0


def test_refusals_exports_and_constants():
    import kaldi_hmm_gmm_amd as khg
    from kaldi_hmm_gmm_amd import _lib
    c = cases.estimate_case(3, 5)
    for kw in (dict(target_dim=0), dict(target_dim=6), dict(target_dim=2, within_class_factor=float("nan")), dict(target_dim=2, within_class_factor=float("inf"))):
        with pytest.raises(Exception):
            _compute(c, **kw)
    with pytest.raises(Exception):
        khg.lda_compute(c["zero"], c["first"], c["packed"][:-1], target_dim=2)
    lib = _lib.lib
    f64, f32 = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_float)
    z, f, s = (np.ascontiguousarray(c[k]).ctypes.data_as(f64) for k in ("zero", "first", "packed"))
    M = np.zeros((2, 5), np.float32)
    pM = M.ctypes.data_as(f32)
    o = _lib.LdaOptionsC()
    lib.khg_lda_options_default(ctypes.byref(o))
    assert (o.target_dim, o.remove_offset, o.within_class_factor) == (40, 0, 1.0)
    o.target_dim = 2
    assert lib.khg_lda_compute(ctypes.byref(o), 3, 5, z, f, s, None, None, None, None, None, None) == -1         # nowhere to put M
    assert b"khg_lda_compute" in lib.khg_last_error()
    assert lib.khg_lda_compute(None, 3, 5, z, f, s, pM, None, None, None, None, None) == -1                      # the default target_dim 40 > 5
    o.within_class_factor = float("nan")
    assert lib.khg_lda_compute(ctypes.byref(o), 3, 5, z, f, s, pM, None, None, None, None, None) == -1
    o.within_class_factor = 1.0
    assert lib.khg_lda_compute(ctypes.byref(o), 3, khg.LDA_MAX_SPLICED_DIM + 1, z, f, s, pM, None, None, None, None, None) == -4
    assert lib.khg_lda_compute(ctypes.byref(o), 3, 5, z, f, s, pM, None, None, None, None, None) == 0 and M.any()
    # the device entry points refuse a dead context before anything else
    assert lib.khg_lda_stats_create(None, 3, 5, 4, 4, ctypes.byref(ctypes.c_void_p())) == -1
    assert lib.khg_acc_lda_stats_post(None, None, None, None, 1.0, None) == -1
    assert lib.khg_utts_splice_transform_feats(None, None, 4, 4, 40, 0, None, None) == -1
    with open(os.path.join(ROOT, "include", "khg_hip.h")) as fh:
        header = fh.read()
    for name in ("khg_lda_stats_create", "khg_lda_stats_destroy", "khg_lda_stats_zero", "khg_lda_stats_download", "khg_lda_stats_upload",
                 "khg_lda_stats_add", "khg_lda_stats_set_chunk_frames", "khg_lda_stats_num_chunks", "khg_acc_lda_stats_post", "khg_lda_compute",
                 "khg_utts_splice_transform_feats"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None, name
    m = re.search(r"#define KHG_LDA_MAX_SPLICED_DIM (\d+)", header)
    assert m and int(m.group(1)) == khg.LDA_MAX_SPLICED_DIM >= 360
    assert (khg.LDA_OK, khg.LDA_SINGULAR) == (0, 1)
    for name in ("DeviceLdaStats", "lda_compute", "acc_lda", "acc_lda_batch", "est_lda", "splice_feats", "splice_transform_feats",
                 "splice_transform_feats_batch", "compose_with_lda", "LDA_OK", "LDA_SINGULAR", "LDA_MAX_SPLICED_DIM"):
        assert hasattr(khg, name), name
    from kaldi_hmm_gmm_amd import device
    assert device.LDA_MAX_SPLICED_DIM == khg.LDA_MAX_SPLICED_DIM and device.DeviceLdaStats is khg.DeviceLdaStats
    assert hasattr(khg.UtteranceSet, "acc_lda_stats_post") and hasattr(khg.UtteranceSet, "splice_transform_feats")
    for meth in ("download", "upload", "add", "zero", "set_chunk_frames", "num_chunks"):
        assert hasattr(khg.DeviceLdaStats, meth), meth
    r = khg.est_lda(dict(zero_acc=c["zero"], first_acc=c["first"], total_second_acc=c["packed"]), target_dim=2)
    assert r["status"] == khg.LDA_OK and r["M"].tobytes() == _compute(c, target_dim=2)["M"].tobytes()


@pytest.mark.parametrize("L,R", [(4, 4), (3, 1), (0, 0)])
def test_host_splice_feats_is_the_definition(L, R):
    import kaldi_hmm_gmm_amd as khg
    rng = np.random.default_rng(L + 10 * R)
    for T in sorted({1, 2, L, L + R + 1}):
        x = rng.standard_normal((T, 3)).astype(np.float32)
        z = khg.splice_feats(x, L, R)
        assert z.dtype == np.float32 and z.shape == (T, 3 * (L + R + 1)) and z.tobytes() == ref.splice(x, L, R).tobytes(), T
        assert khg.splice_transform_feats(x, None, L, R).tobytes() == z.tobytes()


def _round32(v):
    """the float32 nearest to the exact rational v (no tie occurs in the test's data)"""
    c = np.float32(float(v))
    cands = [float(np.nextafter(c, np.float32(-np.inf))), float(c), float(np.nextafter(c, np.float32(np.inf)))]
    return min(cands, key=lambda f: abs(v - Fraction(f)))


@pytest.mark.parametrize("offset", [False, True])
def test_host_splice_transform_is_the_fmaf_chain(offset):
    """against exact rational arithmetic rounded to float once per step, on the bits"""
    import kaldi_hmm_gmm_amd as khg
    rng = np.random.default_rng(5)
    L, R, D, out_dim, T = 2, 1, 3, 4, 5
    x = rng.standard_normal((T, D)).astype(np.float32)
    Dz = D * (L + R + 1)
    M = rng.standard_normal((out_dim, Dz + (1 if offset else 0))).astype(np.float32)
    y = khg.splice_transform_feats(x, M, L, R)
    assert y.dtype == np.float32 and y.shape == (T, out_dim)
    z = ref.splice(x, L, R)
    for t in range(T):
        for r in range(out_dim):
            acc = Fraction(float(M[r, Dz])) if offset else Fraction(0)
            for c in range(Dz):
                acc = Fraction(_round32(Fraction(float(M[r, c])) * Fraction(float(z[t, c])) + acc))
            assert float(acc) == float(y[t, r]), (t, r)
    with pytest.raises(ValueError):
        khg.splice_transform_feats(x, M[:, :-2], L, R)


def test_compose_with_lda_is_the_matrix_product():
    import kaldi_hmm_gmm_amd as khg
    rng = np.random.default_rng(9)
    d, Dz = 4, 10
    A, b = rng.standard_normal((d, d)).astype(np.float32), rng.standard_normal(d).astype(np.float32)
    Lm, lo = rng.standard_normal((d, Dz)).astype(np.float32), rng.standard_normal(d).astype(np.float32)
    A64, L64 = A.astype(np.float64), Lm.astype(np.float64)
    got = khg.compose_with_lda(A, Lm)
    assert got.dtype == np.float32 and got.tobytes() == (A64 @ L64).astype(np.float32).tobytes()
    Ab, Lo = np.concatenate([A, b[:, None]], 1), np.concatenate([Lm, lo[:, None]], 1)
    want = np.concatenate([A64 @ L64, (b.astype(np.float64))[:, None]], 1)
    assert khg.compose_with_lda(Ab, Lm).tobytes() == want.astype(np.float32).tobytes()
    want = np.concatenate([A64 @ L64, (A64 @ lo.astype(np.float64))[:, None]], 1)
    assert khg.compose_with_lda(A, Lo, lda_has_offset=True).tobytes() == want.astype(np.float32).tobytes()
    want = np.concatenate([A64 @ L64, (A64 @ lo.astype(np.float64) + b.astype(np.float64))[:, None]], 1)
    assert khg.compose_with_lda(Ab, Lo, lda_has_offset=True).tobytes() == want.astype(np.float32).tobytes()
    # applying the composition is applying the two in turn (float64 on both sides)
    z = rng.standard_normal(Dz)
    one = khg.compose_with_lda(Ab, Lo, lda_has_offset=True).astype(np.float64)
    two = A64 @ (L64 @ z + lo) + b
    np.testing.assert_allclose(one[:, :Dz] @ z + one[:, Dz], two, rtol=1e-5, atol=1e-5)
    with pytest.raises(ValueError):
        khg.compose_with_lda(A[:, :-1], Lm)
