"""CMVN and add-deltas without a GPU: the coefficient tables against their recorded bit patterns and the
restatement, the C++ normaliser (khg_cmvn_compute) against the restatement on the bits, and the properties of the host add_deltas."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import feat_cases as cases  # noqa: E402
import feat_ref as ref  # noqa: E402


def _hex(a):
    return " ".join("%08x" % v for v in np.asarray(a, np.float32).view(np.uint32))


def test_delta_scales_bit_patterns():
    import kaldi_hmm_gmm_amd as khg
    s = khg.delta_scales(2, 2)
    assert _hex(s[0]) == "3f800000"
    assert _hex(s[1]) == "be4ccccd bdcccccd 00000000 3dcccccd 3e4ccccd"
    assert _hex(s[2]) == "3d23d70b 3d23d70b 3c23d70b bd23d70b bdcccccd bd23d70b 3c23d70b 3d23d70b 3d23d70b"
    assert _hex(khg.delta_scales(1, 2)[1]) == _hex(s[1])
    assert s[2][0] != np.float32(0.04)                          # built in float by the recurrence, not rounded from the real value
    w1 = khg.delta_scales(2, 1)[2]
    assert w1.tobytes() == np.array([0.25, 0.0, -0.5, 0.0, 0.25], np.float32).tobytes()


@pytest.mark.parametrize("order", [0, 1, 2, 3])
@pytest.mark.parametrize("window", [1, 2, 3, 4])
def test_delta_scales_equal_the_restatement(order, window):
    import kaldi_hmm_gmm_amd as khg
    got, want = khg.delta_scales(order, window), ref.delta_scales(order, window)
    assert len(got) == order + 1
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.float32 and g.shape == (2 * i * window + 1,) and g.tobytes() == w.tobytes(), (order, window, i)


def test_delta_scales_refusals():
    import kaldi_hmm_gmm_amd as khg
    for order, window in ((-1, 2), (2, 0)):
        with pytest.raises(Exception):
            khg.delta_scales(order, window)
    from kaldi_hmm_gmm_amd import _lib
    buf = np.zeros(4, np.float32)
    assert _lib.lib.khg_delta_scales(-1, 2, _lib.ptr(buf, _lib.C.c_float)) != 0
    assert _lib.lib.khg_delta_scales(1, 0, _lib.ptr(buf, _lib.C.c_float)) != 0


@pytest.mark.parametrize("norm_means", [False, True])
@pytest.mark.parametrize("norm_vars", [False, True])
@pytest.mark.parametrize("reverse", [False, True])
def test_cmvn_compute_equals_the_restatement_on_the_bits(norm_means, norm_vars, reverse):
    import kaldi_hmm_gmm_amd as khg
    st = cases.compute_inputs()
    got = khg.cmvn_compute(st, norm_means=norm_means, norm_vars=norm_vars, reverse=reverse)
    norm, status = ref.cmvn_compute(st, norm_means, norm_vars, reverse)
    assert got["norm"].dtype == np.float32 and got["norm"].shape == (4, 2, 5)
    assert got["norm"].tobytes() == norm.tobytes() and (got["status"] == status).all()
    assert list(got["status"]) == [khg.CMVN_OK, khg.CMVN_OK, khg.CMVN_NO_DATA, khg.CMVN_NONFINITE]
    for s in (2, 3):                                            # a speaker that is not OK: offset 0, scale 1
        assert not got["norm"][s, 0].any() and (got["norm"][s, 1] == 1.0).all()
    if norm_vars:                                               # the constant columns sit on the floor 1e-20
        floor = np.float32(1e-10) if reverse else np.float32(1.0 / np.sqrt(1e-20))
        assert got["norm"][0, 1, 2] == floor and (got["norm"][1, 1] == floor).all()
    else:
        assert (got["norm"][:, 1] == 1.0).all()
    if not norm_means:
        assert not got["norm"][:, 0].any()
    one = khg.cmvn_compute(st[0], norm_means=norm_means, norm_vars=norm_vars, reverse=reverse)
    assert one["norm"].tobytes() == norm[0].tobytes() and one["status"] == khg.CMVN_OK


def test_cmvn_normalises_and_reverses():
    import kaldi_hmm_gmm_amd as khg
    x = cases.float_feats([400], 6, seed=3)[0] * np.arange(1, 7, dtype=np.float32) + 3.0
    st = khg.compute_cmvn_stats(x)
    assert st.shape == (2, 7) and st[0, 6] == 400 and st[1, 6] == 0
    fwd = khg.cmvn_compute(st, norm_vars=True)
    y = khg.apply_cmvn(x, fwd["norm"])
    assert np.abs(y.mean(0)).max() < 1e-5 and np.abs(y.std(0) - 1).max() < 1e-5
    back = khg.apply_cmvn(y, khg.cmvn_compute(st, norm_vars=True, reverse=True)["norm"])
    assert np.abs(back - x).max() < 1e-4 * np.abs(x).max()
    assert khg.apply_cmvn(x, None).tobytes() == x.tobytes()
    # two roundings: the float product first, then the float sum
    n = fwd["norm"]
    want = np.array([[np.float32(np.float32(v * s) + o) for v, s, o in zip(row, n[1], n[0])] for row in x], np.float32)
    assert y.tobytes() == want.tobytes()


def test_add_deltas_of_a_ramp():
    """x[t] = a t + b with exactly representable values: away from the edges the delta block is a sum_j j scales[1][j] = a and the
    delta-delta block a sum_j j scales[2][j] + x[t] sum_j scales[2][j] = 0, each to the float rounding of the coefficient sums"""
    import kaldi_hmm_gmm_amd as khg
    a, b = np.array([2.0, -0.5, 0.25], np.float32), np.array([1.0, 8.0, -3.0], np.float32)
    T, order, window = 40, 2, 2
    x = (np.arange(T, dtype=np.float32)[:, None] * a[None, :] + b[None, :]).astype(np.float32)
    y = khg.add_deltas(x, order, window)
    assert y.shape == (T, 9) and y.dtype == np.float32 and y[:, :3].tobytes() == x.tobytes()
    H = order * window
    inner = slice(H, T - H)
    # a chain has at most 2 H + 1 = 9 steps; its partial sums stay below S = sum |scales| max |x| <= 0.6 max |x|; a step rounds once
    # (2^-24 S) and its coefficient is within 3 ulps of the real one (3 2^-24 S)
    tol = 9 * 4 * 2.0 ** -24 * 0.6 * np.abs(x).max()
    assert np.abs(y[inner, 3:6] - a[None, :]).max() <= tol
    assert np.abs(y[inner, 6:9]).max() <= tol
    assert np.abs(y[0, 3:6]).max() < np.abs(a).max()            # the clamped edge: the first frame is repeated, the slope is damped


def test_add_deltas_of_one_frame():
    import kaldi_hmm_gmm_amd as khg
    x = np.array([[1.5, -2.0, 3.25]], np.float32)
    for order, window in ((2, 2), (3, 1), (1, 4)):
        y = khg.add_deltas(x, order, window)
        scales = ref.delta_scales(order, window)
        for i, s in enumerate(scales):
            want = np.zeros(3, np.float64)
            for c in s:                                         # the chain of T = 1: every tap reads x[0]
                if c != 0:
                    want = np.float32(np.float64(c) * x[0].astype(np.float64) + want).astype(np.float64)      # exact product, one rounding
            assert y[0, 3 * i:3 * i + 3].tobytes() == want.astype(np.float32).tobytes(), (order, window, i)
            # x[0] sum scales[i]: one rounding of at most 2^-24 max |x| per step (sum |scales| <= 1), one more for the float product
            tol = (len(s) + 1) * 2.0 ** -24 * np.abs(x).max()
            assert np.abs(y[0, 3 * i:3 * i + 3] - x[0] * np.float32(s.astype(np.float64).sum())).max() <= tol
    assert khg.add_deltas(np.zeros((0, 3), np.float32), 2, 2).shape == (0, 9)


def test_add_deltas_with_a_normaliser_is_the_pipeline():
    import kaldi_hmm_gmm_amd as khg
    x = cases.float_feats([30], 4, seed=9)[0]
    norm = khg.cmvn_compute(khg.compute_cmvn_stats(x), norm_vars=True)["norm"]
    assert khg.add_deltas(x, 2, 2, norm=norm).tobytes() == khg.add_deltas(khg.apply_cmvn(x, norm), 2, 2).tobytes()


def test_symbols_exported_and_declared():
    from kaldi_hmm_gmm_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = os.path.join(root, "kaldi_hmm_gmm_amd", "libkhg_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    header = open(os.path.join(root, "include", "khg_hip.h")).read()
    for name in ("khg_cmvn_stats_create", "khg_cmvn_stats_destroy", "khg_cmvn_stats_zero", "khg_cmvn_stats_download", "khg_cmvn_stats_upload",
                 "khg_cmvn_stats_add", "khg_cmvn_stats_set_chunk_frames", "khg_cmvn_stats_num_chunks", "khg_acc_cmvn_stats", "khg_cmvn_compute",
                 "khg_delta_scales", "khg_utts_apply_cmvn", "khg_utts_add_deltas"):
        assert (" T " + name + "\n") in out and name in _lib.SIGNATURES and ("int " + name + "(") in header, name
    assert "#define KHG_FEAT_TILE_LDS_BYTES" in header
    # the entry points refuse a null context before touching anything
    assert _lib.lib.khg_acc_cmvn_stats(None, None, None, None) != 0
    assert _lib.lib.khg_utts_apply_cmvn(None, None, 1, None, None, None, None) != 0
    assert _lib.lib.khg_utts_add_deltas(None, None, 2, 2, 0, None, None, None, None) != 0
