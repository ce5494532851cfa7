"""CMVN and add-deltas on the device: khg_acc_cmvn_stats through UtteranceSet.acc_cmvn_stats against exact
integer sums and the restatement of tests/feat_ref.py, the bits of the statistics across runs / companions / chunk sizes, and the
tile kernel (khg_utts_apply_cmvn, khg_utts_add_deltas) against the host forms on the bits.

The bound of the float statistics is derived, not measured: any order of an n-term fp64 sum of exact terms errs by at most
n 2^-52 sum |terms| per element; the restatement adds its terms by math.fsum, so that its own rounding stays out of the bound."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import feat_cases as cases  # noqa: E402
from helpers import build  # noqa: E402

pytestmark = pytest.mark.gpu
U52 = 2.0 ** -52


def _set(ctx, feats):
    from kaldi_hmm_gmm_amd import UtteranceSet
    fo = np.concatenate([[0], np.cumsum([len(f) for f in feats])]).astype(np.int64)
    return UtteranceSet(ctx, None, fo, np.ascontiguousarray(np.concatenate(feats), np.float32))


def _set_on_tensor(ctx, feats):
    """a set that borrows a torch tensor: in-place rewrites can be read back"""
    import torch
    from kaldi_hmm_gmm_amd import UtteranceSet
    fo = np.concatenate([[0], np.cumsum([len(f) for f in feats])]).astype(np.int64)
    t = torch.from_numpy(np.ascontiguousarray(np.concatenate(feats), np.float32)).to("cuda:%d" % ctx.device)
    torch.cuda.synchronize()
    return UtteranceSet(ctx, None, fo, (t.data_ptr(), t), dim=feats[0].shape[1]), t


def _acc(ctx, feats, u2s, S, chunk=None, stats=None):
    from kaldi_hmm_gmm_amd import DeviceCmvnStats
    us = _set(ctx, feats)
    if stats is None:
        stats = DeviceCmvnStats(ctx, S, us.dim)
    if chunk is not None:
        stats.set_chunk_frames(chunk)
    us.acc_cmvn_stats(np.ascontiguousarray(u2s, np.int32), stats)
    return stats.download(), stats


# ---- statistics ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", cases.STATS_DIMS)
def test_statistics_of_integers_are_exact(ctx, D):
    lens, u2s, S, feats, _ = cases.stats_case(D, "int")
    got, stats = _acc(ctx, feats, u2s, S)
    want = cases.int_sums(feats, u2s, S)
    assert got.shape == (S, 2, D + 1) and got.dtype == np.float64
    assert (got == want).all(), np.argwhere(got != want)[:5]
    assert not got[5].any() and not got[6].any()                # a speaker without utterances, one whose utterance has no frames
    assert list(got[:5, 0, D]) == [1, 1023, 1024, 1025, 1200] and stats.num_chunks() == 1
    # a second call doubles an exactly representable handle; add and zero as documented
    twice, _ = _acc(ctx, feats, u2s, S, stats=stats)
    assert (twice == 2.0 * want).all()
    from kaldi_hmm_gmm_amd import DeviceCmvnStats
    other = DeviceCmvnStats(ctx, S, D)
    other.upload(want)
    assert other.download().tobytes() == want.tobytes()
    stats.add(-0.5, other)
    assert (stats.download() == 1.5 * want).all()
    stats.zero()
    assert not stats.download().any()
    with pytest.raises(Exception, match="differ"):
        stats.add(1.0, DeviceCmvnStats(ctx, S + 1, D))
    with pytest.raises(Exception):
        stats.add(float("nan"), other)


@pytest.mark.parametrize("D", cases.STATS_DIMS)
def test_statistics_of_floats_within_the_bound(ctx, D):
    lens, u2s, S, feats, want = cases.stats_case(D, "float")
    got, _ = _acc(ctx, feats, u2s, S)
    err, bound = np.abs(got - want["stats"]), want["n"][:, None, None] * U52 * want["abs"]
    print("D = %d: largest error / bound %.3g" % (D, float((err / np.maximum(bound, 1e-300)).max())))
    assert (err <= bound).all()
    assert (got[:, 0, D] == want["n"]).all() and not got[:, 1, D].any()


def test_per_utterance_mode(ctx):
    """n_spk = n_utt = 300: one slice per speaker, utterances of 0 .. 6 frames"""
    D, n = 13, 300
    rng = np.random.default_rng(1)
    lens = [int(t) for t in rng.integers(0, 7, size=n)]
    feats = cases.int_feats(lens, D, 3)
    u2s = np.arange(n, dtype=np.int32)
    got, _ = _acc(ctx, feats, u2s, n)
    assert (got == cases.int_sums(feats, u2s, n)).all()


def test_statistics_have_the_same_bits(ctx):
    D = 13
    lens, u2s, S, feats, _ = cases.stats_case(D, "float")
    first, _ = _acc(ctx, feats, u2s, S)
    again, _ = _acc(ctx, feats, u2s, S)
    assert again.tobytes() == first.tobytes()                   # two runs
    small, st = _acc(ctx, feats, u2s, S, chunk=cases.SLICE)     # a chunk of one slice against the default
    assert st.num_chunks() > 1 and small.tobytes() == first.tobytes()
    # speaker 4 alone in a set, its utterances in the same order, against speaker 4 among the others
    mine = [i for i, s in enumerate(u2s) if s == 4]
    alone, _ = _acc(ctx, [feats[i] for i in mine], np.zeros(len(mine), np.int32), 1)
    assert alone[0].tobytes() == first[4].tobytes()
    # ... and under another speaker number, with everything else unassigned
    moved = np.where(u2s == 4, 2, -1).astype(np.int32)
    got, _ = _acc(ctx, feats, moved, S)
    assert got[2].tobytes() == first[4].tobytes() and not np.delete(got, 2, axis=0).any()


def test_statistics_refusals_leave_the_handles_bits(ctx):
    from kaldi_hmm_gmm_amd import DeviceCmvnStats
    D = 13
    lens, u2s, S, feats, _ = cases.stats_case(D, "float")
    before, stats = _acc(ctx, feats, u2s, S)
    us = _set(ctx, feats)
    bad = u2s.copy()
    bad[3] = S
    with pytest.raises(Exception, match="speaker"):
        us.acc_cmvn_stats(bad, stats)
    with pytest.raises(Exception, match="dimension"):
        us.acc_cmvn_stats(u2s, DeviceCmvnStats(ctx, S, D + 1))
    with pytest.raises(Exception):
        us.acc_cmvn_stats(u2s[:-1], stats)
    assert stats.download().tobytes() == before.tobytes()


# ---- apply-cmvn and add-deltas -------------------------------------------------------------------------------------------------------
def _norms(feats, mine, norm_vars, reverse=False):
    """per-utterance normalisers of the test utterances from their own host statistics; the 1e30 neighbours get speaker -1"""
    import kaldi_hmm_gmm_amd as khg
    u2s = np.full(len(feats), -1, np.int32)
    st = np.zeros((len(mine), 2, feats[0].shape[1] + 1))
    for k, i in enumerate(mine):
        u2s[i] = k
        st[k] = khg.compute_cmvn_stats(feats[i])
    r = khg.cmvn_compute(st, norm_vars=norm_vars, reverse=reverse)
    return u2s, r["norm"], r["status"]


def _host(feats, u2s, norm, status, fn):
    return np.concatenate([fn(f, norm[s] if s >= 0 and (status is None or status[s] == 0) else None) for f, s in zip(feats, u2s)])


@pytest.mark.parametrize("D", cases.TILE_DIMS)
@pytest.mark.parametrize("norm_vars,reverse", [(False, False), (True, False), (True, True)])
def test_apply_cmvn_equals_the_host_form_on_the_bits(ctx, D, norm_vars, reverse):
    import kaldi_hmm_gmm_amd as khg
    lens, feats, mine = cases.tile_set(D)
    u2s, norm, status = _norms(feats, mine, norm_vars, reverse)
    feats[mine[3]][1, 0] = -0.0
    u2s[mine[3]] = -1                                           # a test utterance without a speaker, holding a -0.0
    feats[mine[4]][2, 0] = -0.0
    status = status.copy()
    status[4] = khg.CMVN_NO_DATA                                # ... and one of a speaker that is not OK
    want = _host(feats, u2s, norm, status, khg.apply_cmvn)
    us, t = _set_on_tensor(ctx, feats)
    before = t.cpu().numpy().copy()
    out = khg.apply_cmvn_batch(us, norm, u2s, status, in_place=False)
    assert out.cpu().numpy().tobytes() == want.tobytes() and t.cpu().numpy().tobytes() == before.tobytes()
    assert khg.apply_cmvn_batch(us, norm, u2s, status) is None
    got = t.cpu().numpy()
    assert got.tobytes() == want.tobytes()
    fo = np.asarray(us.frame_off)
    for i in (mine[3], mine[4]):                                # kept byte for byte, the sign of the zero included
        assert got[fo[i]:fo[i + 1]].tobytes() == feats[i].tobytes() and np.signbit(got[fo[i]:fo[i + 1]]).any()
    assert (got[fo[mine[0] - 1]:fo[mine[0]]] == np.float32(1e30)).all()
    with pytest.raises(Exception, match="speaker"):
        us.apply_cmvn(np.full(len(feats), len(norm), np.int32), norm)
    with pytest.raises(Exception):
        us.apply_cmvn(u2s, norm[:, :, :-1] if D > 1 else norm[:, :1])


def test_loglikes_see_the_rows_rewritten_in_place(ctx):
    """features_changed at work: the default K1 keeps planes packed from the rows; after the in-place call it scores the new rows"""
    import kaldi_hmm_gmm_amd as khg
    D = 13
    m, gc, om, ut, _ = build(5, 3, D, n_utt=1, seed=4, max_phones=2)
    feats = cases.float_feats([2, 9, 64, 65, 30], D, seed=12)
    dm = khg.DeviceModel(ctx, m.gauss_off, gc, m.means_invvars, m.inv_vars, m.weights)
    pdfs = np.arange(5, dtype=np.int32)

    def lls(u):
        u.set_pdf_list(pdfs)
        u.loglikes(dm)
        return np.concatenate([np.ravel(a) for a in u.download_loglikes()])
    us, _t = _set_on_tensor(ctx, feats)
    old = lls(us)
    u2s = np.arange(len(feats), dtype=np.int32)
    norm = khg.cmvn_compute(np.stack([khg.compute_cmvn_stats(f) for f in feats]), norm_vars=True)["norm"]
    khg.apply_cmvn_batch(us, norm, u2s)
    new = lls(us)
    fresh = lls(_set(ctx, [khg.apply_cmvn(f, n) for f, n in zip(feats, norm)]))
    assert new.tobytes() == fresh.tobytes() and new.tobytes() != old.tobytes() and np.isfinite(new).all()


@pytest.mark.parametrize("D", cases.TILE_DIMS)
@pytest.mark.parametrize("order,window", [(0, 1), (1, 1), (1, 4), (2, 2), (2, 4), (3, 1), (3, 2), (3, 4)])
def test_add_deltas_equals_the_host_form_on_the_bits(ctx, D, order, window):
    import kaldi_hmm_gmm_amd as khg
    lens, feats, mine = cases.tile_set(D, seed=order + window)
    us = _set(ctx, feats)
    want = np.concatenate([khg.add_deltas(f, order, window) for f in feats])
    out = khg.add_deltas_batch(us, order, window)
    got = out.cpu().numpy()
    assert got.shape == (sum(lens), D * (order + 1))
    fo = np.asarray(us.frame_off)
    for i in mine:                                              # a neighbour's 1e30 in any tap would show
        assert np.abs(got[fo[i]:fo[i + 1]]).max() < 1e3
    assert got.tobytes() == want.tobytes()
    if order == 0:
        assert np.array_equal(got, np.concatenate(feats))
    # fused against unfused, both against the host pipeline
    u2s, norm, status = _norms(feats, mine, norm_vars=True)
    fused = khg.add_deltas_batch(us, order, window, norm=norm, utt2spk=u2s, status=status)
    mid = khg.apply_cmvn_batch(us, norm, u2s, status, in_place=False)
    us2 = khg.UtteranceSet(ctx, None, fo, (mid.data_ptr(), mid), dim=D)
    unfused = khg.add_deltas_batch(us2, order, window)
    host = np.concatenate([khg.add_deltas(f, order, window, norm=norm[s] if s >= 0 else None) for f, s in zip(feats, u2s)])
    assert fused.cpu().numpy().tobytes() == host.tobytes() and unfused.cpu().numpy().tobytes() == host.tobytes()


def test_zero_coefficients_are_skipped(ctx):
    """window 1, order 2: [0.25, 0, -0.5, 0, 0.25].  A row of +inf at frame t0 meets only the zero taps at frames t0 - 1 and t0 + 1
    of the delta-delta block: skipped, the values there are finite (0 * inf would be NaN)"""
    import kaldi_hmm_gmm_amd as khg
    D, T, t0 = 3, 12, 6
    x = cases.float_feats([T], D, seed=2)[0]
    x[t0] = np.inf
    us = _set(ctx, [x])
    got = khg.add_deltas_batch(us, 2, 1).cpu().numpy()
    want = khg.add_deltas(x, 2, 1)
    assert np.isfinite(got[[t0 - 1, t0 + 1], 2 * D:]).all() and not np.isfinite(got[t0, 2 * D:]).any()
    fin = np.isfinite(want)
    assert (np.isfinite(got) == fin).all() and got[fin].tobytes() == want[fin].tobytes()


def test_a_set_on_the_output_aligns(ctx):
    """a new UtteranceSet borrows the returned tensor: dim D (order + 1), and a model of that dimension aligns on it"""
    import kaldi_hmm_gmm_amd as khg
    from kaldi_hmm_gmm_amd import DeviceModel, DeviceTransitions, UtteranceSet
    D = 13
    m, gc, om, ut, cost = build(6, 2, 3 * D, n_utt=3, seed=5, max_phones=3)
    fo = np.asarray(ut.frame_off, np.int64)
    static = [np.ascontiguousarray(ut.feats[fo[i]:fo[i + 1], :D], np.float32) for i in range(3)]
    us = _set(ctx, static)
    t = khg.add_deltas_batch(us, 2, 2)
    tm = DeviceTransitions(ctx, m.id2pdf)
    tm.set_trans_cost(cost)
    on = UtteranceSet(ctx, tm, fo, (t.data_ptr(), t), dim=3 * D, graphs=ut.graphs)
    assert on.dim == 3 * D and on.n_utt == 3
    dm = DeviceModel(ctx, m.gauss_off, gc, m.means_invvars, m.inv_vars)
    on.loglikes(dm)
    res = on.align(tm, acoustic_scale=0.1)
    assert len(res["ali"]) == fo[-1] and (np.asarray(res["status"]) & 1 == 0).all() and (res["ali"] > 0).all()


def test_limits_and_refusals(ctx):
    import kaldi_hmm_gmm_amd as khg
    import torch
    us = _set(ctx, cases.float_feats([5, 3], 128, seed=1))
    ok = khg.add_deltas_batch(us, 3, 4)                         # dim 128, order 3, window 4 is inside the limit
    assert tuple(ok.shape) == (8, 512)
    with pytest.raises(Exception, match="KHG_FEAT_TILE_LDS_BYTES"):
        khg.add_deltas_batch(us, 8, 8)                          # (64 + 128) rows of 128 floats: 96 KiB
    out = torch.zeros((8, 128 * 3), dtype=torch.float32, device=ok.device)
    for order, window in ((-1, 2), (2, 0)):
        with pytest.raises(Exception):
            us.add_deltas(order, window, out.data_ptr())
    norm = np.zeros((2, 2, 128), np.float32)
    with pytest.raises(Exception, match="speaker"):
        us.add_deltas(2, 2, out.data_ptr(), norm, np.array([0, 2], np.int32))
    with pytest.raises(Exception):
        khg.add_deltas_batch(us, 2, 2, out=out[:, :-1])
    assert not out.cpu().numpy().any()                          # nothing was launched
