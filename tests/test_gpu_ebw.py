"""K4, discriminative form: the Extended Baum-Welch update on the device (khg_model_ebw_update) against the host form
(khg_ebw_am_diag_gmm_update) and the restatement (tests/ebw_ref.py), and the three block operations (khg_accs_add / _scale /
_smooth_with_accum) against numpy.

Stated tolerances: weights / inv_vars / means_invvars / every counter BIT-EQUAL to the host form; gconsts through logf, <= GC_ULPS = 4
float ulps (as for the ML update); the two diagnostics within n_terms 2^-50 sum |term| (a one-ulp log, a reordered fp64 sum); the
block operations bit-equal to numpy (one fp64 operation per element, contraction off)."""
import os
import sys

import numpy as np
import pytest

import kaldi_hmm_gmm_amd as khg
from kaldi_hmm_gmm_amd import Context, DeviceAccs, DeviceModel, DeviceTransitions, UtteranceSet
from kaldi_hmm_gmm_amd import mle as khg_mle
from oracle import oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ebw_cases  # noqa: E402
import ebw_ref  # noqa: E402
from ebw_cases import FLAGS  # noqa: E402
from helpers import build  # noqa: E402
from test_gpu_lattice_faster_raw import trained  # noqa: E402,F401

pytestmark = pytest.mark.gpu

GC_ULPS = 4
# beside the CPU shapes: 256 Gaussians in a pdf (64 per wave), and a dimension that takes the four-elements-per-lane kernel with a ragged
# last element (150 = 2 * 64 + 22); dim 80 = 64 + 16 above takes the two-element one
SHAPES = ebw_cases.SHAPES + [(3, 256, 40, False), (4, 8, 150, False)]


def _block(accs, blk):
    buf = np.zeros(accs.size, np.float64)
    G, D = accs.sumG, accs.dim
    buf[:G] = blk[0]
    buf[G: G + G * D] = np.asarray(blk[1]).reshape(-1)
    buf[G + G * D: G + 2 * G * D] = np.asarray(blk[2]).reshape(-1)
    return buf


def _device_update(ctx, shape, flags, E=2.0):
    m, num, den = ebw_cases.fabricate(shape)
    gc = orc.model_gconsts(m.gauss_off, m.weights, m.inv_vars, m.means_invvars)
    dm = DeviceModel(ctx, m.gauss_off, gc, m.means_invvars, m.inv_vars, weights=m.weights)
    tm = DeviceTransitions(ctx, m.id2pdf)
    a_num, a_den = DeviceAccs(ctx, dm, tm), DeviceAccs(ctx, dm, tm)
    a_num.upload(_block(a_num, num))
    a_den.upload(_block(a_den, den))
    r = dm.ebw_update(a_num, a_den, khg.EbwOptions(E=E), khg.EbwWeightOptions(), FLAGS[flags])
    return m, dm, tm, r


@pytest.mark.parametrize("flags", list(FLAGS))
@pytest.mark.parametrize("shape", SHAPES)
def test_device_vs_host_form(ctx, shape, flags):
    m, num, den = ebw_cases.fabricate(shape)
    h_w, h_gc, h_miv, h_iv, h_res = khg_mle._flat_ebw_update(khg.EbwOptions(), khg.EbwWeightOptions(), m.gauss_off, num, den, FLAGS[flags],
                                                             m.weights, m.means_invvars, m.inv_vars)
    _, dm, _, r = _device_update(ctx, shape, flags)
    d = dm.download()
    assert np.array_equal(d["gauss_off"], m.gauss_off)
    for name, got, want in (("weights", d["weights"], h_w), ("inv_vars", d["inv_vars"], h_iv), ("means_invvars", d["means_invvars"], h_miv)):
        np.testing.assert_array_equal(got, want, err_msg=name)
    for k in ("floored", "failed", "skipped", "weights_skipped", "count"):
        assert r[k] == h_res[k], (k, r[k], h_res[k])
    assert ebw_cases.ulps32(d["gconsts"], h_gc).max() <= GC_ULPS
    ref = ebw_cases.reference(shape, flags)
    worst = ebw_cases.check_against_reference(d["weights"], d["gconsts"], d["means_invvars"], d["inv_vars"], r, ref, GC_ULPS)
    print("worst fraction of the diagnostics' bound: %.3g" % worst)
    if shape[1] > 1 and FLAGS[flags] & 3:
        assert r["skipped"] > 0
        if FLAGS[flags] & 2:                  # without v every try succeeds: nothing is floored, nothing fails
            assert r["floored"] > 0 and r["failed"] > 0
        else:
            assert r["floored"] == 0 and r["failed"] == 0


def test_device_vs_host_form_other_E(ctx):
    """E = 0.5: the D + occ <= 0 branch with a positive numerator count."""
    shape = ebw_cases.SHAPES[1]
    ref = ebw_cases.reference(shape, "mv", E=0.5)
    _, dm, _, r = _device_update(ctx, shape, "mv", E=0.5)
    d = dm.download()
    ebw_cases.check_against_reference(d["weights"], d["gconsts"], d["means_invvars"], d["inv_vars"], r, ref, GC_ULPS)


def test_updated_handle_is_repacked_for_k1_k3(ctx):
    """After the update the handle behaves exactly like a model created from the downloaded parameters: K1 log-likes and K3
    statistics through the updated handle == through a fresh handle (what test_device_m_step_model_is_repacked_for_k1_k3 checks for K4)."""
    m, gc, om, ut, cost = build(30, 9, 20, 12, seed=4, ragged=True, max_phones=5)
    rng = np.random.default_rng(3)
    G, D = int(m.gauss_off[-1]), m.dim
    mean, var = m.means.astype(np.float64), m.vars.astype(np.float64)
    blocks = []
    for spread in (0.3, 0.6):
        occ = rng.uniform(5.0, 60.0, G)
        mu = mean + spread * rng.standard_normal((G, D))
        blocks.append((occ, occ[:, None] * mu, occ[:, None] * (var * rng.uniform(0.7, 1.5, (G, D)) + mu * mu)))
    dm = DeviceModel(ctx, m.gauss_off, gc, m.means_invvars, m.inv_vars, weights=m.weights)
    tm = DeviceTransitions(ctx, m.id2pdf)
    tm.set_trans_cost(cost)
    a_num, a_den = DeviceAccs(ctx, dm, tm), DeviceAccs(ctx, dm, tm)
    a_num.upload(_block(a_num, blocks[0]))
    a_den.upload(_block(a_den, blocks[1]))
    r = khg_mle.ebw_am_diag_gmm_update_device(None, None, a_num, a_den, 0x7, dm)
    assert r["failed"] == 0 and r["count"] > 0
    d = dm.download()
    assert np.array_equal(d["gauss_off"], m.gauss_off) and not np.array_equal(d["inv_vars"], m.inv_vars)
    fresh = DeviceModel(ctx, d["gauss_off"], d["gconsts"], d["means_invvars"], d["inv_vars"])
    us = UtteranceSet(ctx, tm, ut.frame_off, ut.feats, graphs=ut.graphs)
    us.loglikes(dm)
    ll_a = us.download_loglikes()
    us.loglikes(fresh)
    ll_b = us.download_loglikes()
    for x, y in zip(ll_a, ll_b):
        np.testing.assert_array_equal(x, y)
    us.upload_ali(ut.ref_ali)
    accs_a, accs_b = DeviceAccs(ctx, dm, tm), DeviceAccs(ctx, fresh, tm)
    us.acc_stats(dm, tm, accs_a)
    us.acc_stats(fresh, tm, accs_b)
    sa, sb = accs_a.download(), accs_b.download()
    np.testing.assert_allclose(sa["occ"], sb["occ"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(sa["mean_acc"], sb["mean_acc"], rtol=1e-9, atol=1e-9)
    # the statistics an alignment leaves, minus themselves, are all zeros
    accs_a.add(-1.0, accs_a)
    z = accs_a.download_range(0, accs_a.size)
    assert sa["occ"].sum() > 0 and not z.any()


def test_block_operations_vs_numpy(ctx):
    shape = ebw_cases.SHAPES[1]
    m, num, den = ebw_cases.fabricate(shape)
    gc = orc.model_gconsts(m.gauss_off, m.weights, m.inv_vars, m.means_invvars)
    dm = DeviceModel(ctx, m.gauss_off, gc, m.means_invvars, m.inv_vars)
    tm = DeviceTransitions(ctx, m.id2pdf)
    rng = np.random.default_rng(8)
    a, b = DeviceAccs(ctx, dm, tm), DeviceAccs(ctx, dm, tm)
    G, D = a.sumG, a.dim
    ba, bb = _block(a, num), _block(b, den)
    ba[G + 2 * G * D:] = rng.uniform(0.0, 50.0, a.size - (G + 2 * G * D))      # transition counts and scalars take part in add / scale
    bb[G + 2 * G * D:] = rng.uniform(0.0, 50.0, a.size - (G + 2 * G * D))
    assert (den[0] == 0).sum() > 0
    for scale in (1.0, -0.3):
        a.upload(ba); b.upload(bb)
        a.add(scale, b)
        np.testing.assert_array_equal(a.download_range(0, a.size), ebw_ref.accs_add(ba, scale, bb))
        np.testing.assert_array_equal(b.download_range(0, b.size), bb)
    a.upload(ba)
    a.scale(0.7)
    np.testing.assert_array_equal(a.download_range(0, a.size), ebw_ref.accs_scale(ba, 0.7))

    def parts(buf):
        return buf[:G], buf[G: G + G * D].reshape(G, D), buf[G + G * D: G + 2 * G * D].reshape(G, D), buf[G + 2 * G * D:]

    # smoothing from another block: Gaussians whose source count is zero are untouched and counted
    a.upload(ba); b.upload(bb)
    untouched = a.smooth_with_accum(25.0, b, dm)
    occ, mean, var, n0 = ebw_ref.accs_smooth_with_accum(*parts(ba)[:3], 25.0, *parts(bb)[:3])
    got = parts(a.download_range(0, a.size))
    assert untouched == n0 == int((den[0] == 0).sum())
    np.testing.assert_array_equal(got[0], occ)
    np.testing.assert_array_equal(got[1], mean)
    np.testing.assert_array_equal(got[2], var)
    np.testing.assert_array_equal(got[3], parts(ba)[3])                         # transition counts and scalars are not smoothed
    # ... and from itself (the I-smoothing of the numerator block), without asking for the count
    a.upload(ba)
    assert a.smooth_with_accum(10.0, a, dm, count=False) is None
    occ, mean, var, n0 = ebw_ref.accs_smooth_with_accum(*parts(ba)[:3], 10.0, *parts(ba)[:3])
    got = parts(a.download_range(0, a.size))
    np.testing.assert_array_equal(got[0], occ)
    np.testing.assert_array_equal(got[1], mean)
    np.testing.assert_array_equal(got[2], var)


def test_refusals(ctx):
    m, gc, om, ut, cost = build(12, 4, 8, 2, seed=2, max_phones=3)
    m2, gc2, *_ = build(12, 5, 8, 2, seed=2, max_phones=3)
    dm = DeviceModel(ctx, m.gauss_off, gc, m.means_invvars, m.inv_vars, weights=m.weights)
    dm2 = DeviceModel(ctx, m2.gauss_off, gc2, m2.means_invvars, m2.inv_vars, weights=m2.weights)
    tm = DeviceTransitions(ctx, m.id2pdf)
    a, b, c = DeviceAccs(ctx, dm, tm), DeviceAccs(ctx, dm, tm), DeviceAccs(ctx, dm2, tm)
    buf = np.random.default_rng(1).uniform(1.0, 2.0, a.size)
    a.upload(buf); b.upload(buf)
    before = dm.download()

    def refused(fn, *args, **kw):
        with pytest.raises(khg.KhgError):
            fn(*args, **kw)
        np.testing.assert_array_equal(a.download_range(0, a.size), buf)
        np.testing.assert_array_equal(dm.download()["means_invvars"], before["means_invvars"])

    refused(a.add, 1.0, c)                                   # another layout
    refused(a.smooth_with_accum, 1.0, c, dm)
    refused(a.smooth_with_accum, 1.0, b, dm2)                # a model of another layout
    refused(dm.ebw_update, a, c)
    refused(dm.ebw_update, c, a)
    for bad in (float("nan"), float("inf")):
        refused(a.add, bad, b)
        refused(a.scale, bad)
        refused(a.smooth_with_accum, bad, b, dm)
        refused(dm.ebw_update, a, b, khg.EbwOptions(E=bad))
        refused(dm.ebw_update, a, b, khg.EbwOptions(tau=bad))
        refused(dm.ebw_update, a, b, None, khg.EbwWeightOptions(tau=bad))
    other = Context(0)                                       # another context's block
    try:
        dmo = DeviceModel(other, m.gauss_off, gc, m.means_invvars, m.inv_vars, weights=m.weights)
        tmo = DeviceTransitions(other, m.id2pdf)
        o = DeviceAccs(other, dmo, tmo)
        o.upload(buf)
        refused(a.add, 1.0, o)
        refused(a.smooth_with_accum, 1.0, o, dm)
        refused(dm.ebw_update, a, o)
        refused(dm.ebw_update, o, a)
        o.close(); dmo.close(); tmo.close()
    finally:
        other.close()
    dm.ebw_update(a, b)                                      # and the same calls with proper arguments go through
    a.add(1.0, b)


F0_HOST = -69.91591201243091     # tests/ebw_host_chain.py, iteration 0, on the set of the test below (see its text)


def test_mmi_on_the_yes_no_task(ctx, trained):  # noqa: F811
    """Three iterations of align -> acc_stats (numerator), lattice-faster raw lattices on the shared word loop -> posteriors ->
    acc_stats_post (denominator), smooth_with_accum, ebw_update on 30 utterances: each iteration's device parameters are bit-equal to
    the host form applied to the downloaded blocks, the denominator counts equal the posteriors' weight, nothing fails and every
    parameter stays finite -- and the MMI objective F = sum_u (kappa like_u - logZ_u) rises: F_2 > F_0 by more than ten times
    |F_0(host) - F_0(device)|.  The host chain (tests/ebw_host_chain.py: the oracle's aligner and acc-stats, the restatements of the
    lattice-faster decoder and of forward-backward, tests/ebw_ref.py) was run without a GPU on this seeded set (the `trained` fixture's
    30 held-out utterances, kappa = 0.1, tau = 50) to choose E: at E = 2 it gives F = -69.91591, -69.89779, -69.87591 (and -69.86275
    after the third update), a rise of 0.0400 where the device's F_0 lies 3.4e-4 from the host's (11.6 s per pass in Python, so the
    test carries the host's F_0 instead of recomputing it; E = 1 rises by 0.056 on the device)."""
    khg_, dx, tm, am, graph, test_utts = trained
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    import train_mmi_synthetic as mmi
    utts = test_utts[:30]
    st = mmi.MmiState(ctx, tm, am, graph, utts, kappa=0.1)
    F = []
    for it in range(3):
        info = st.accumulate()
        num, den = st.num.download(), st.den.download()
        # the denominator block holds exactly the posteriors' weight: one unit per frame of every decoded utterance
        assert abs(den["occ"].sum() - info["den_weight"]) <= 2e-5 * info["den_weight"]
        assert abs(num["occ"].sum() - info["num_frames"]) <= 2e-5 * info["num_frames"]
        st.num.smooth_with_accum(st.tau, st.num, st.dm, count=False)
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
        assert r["failed"] == 0
        assert all(np.isfinite(d[k]).all() for k in ("weights", "gconsts", "means_invvars", "inv_vars"))
        F.append(info["F"])
        print("iteration %d: F = %.4f over %d utterances, floored %d failed %d skipped %d" % (it, info["F"], info["n_ok"], r["floored"], r["failed"], r["skipped"]))
    assert all(np.isfinite(F))
    margin = 10.0 * abs(F0_HOST - F[0])
    print("F_0 host %.5f device %.5f margin %.5f rise %.5f" % (F0_HOST, F[0], margin, F[-1] - F[0]))
    assert F[-1] > F[0] + margin, (F, margin)
    st.close()
