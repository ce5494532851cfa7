"""acc-tree-stats on the device: khg_acc_tree_stats through UtteranceSet.acc_tree_stats against the restatement of
tests/tree_ref.py.  Alignments are uploaded (khg_ali_upload): no aligner is involved.

Keys and counts must be equal.  The bound of x / x2 is derived, not measured: the float rows are widened to double and their squares
are exact, so a key's sum of n terms, in any order, errs by at most n 2^-53 sum |term| per element (each add rounds once)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tree_cases as cases  # noqa: E402
import tree_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
U53 = 2.0 ** -53
SIL = 1


def _upload(ctx, alis, feats):
    from kaldi_hmm_gmm_amd import UtteranceSet
    fo = np.concatenate([[0], np.cumsum([len(a) for a in alis])]).astype(np.int64)
    dim = feats[0].shape[1]
    us = UtteranceSet(ctx, None, fo, np.ascontiguousarray(np.concatenate(feats) if fo[-1] else np.zeros((0, dim)), np.float32).reshape(-1, dim))
    us.upload_ali(np.ascontiguousarray(np.concatenate(alis) if fo[-1] else np.zeros(0), np.int32))
    return us


def _acc(ctx, tm, alis, feats, N, P, ci=(), stats=None):
    from kaldi_hmm_gmm_amd import DeviceTreeStats
    us = _upload(ctx, alis, feats)
    if stats is None:
        stats = DeviceTreeStats(ctx, feats[0].shape[1], N, P)
    status = us.acc_tree_stats(ctx, tm, stats, ci)
    return stats, np.asarray(status)


def _want(tm, alis, feats, N, P, ci=()):
    import kaldi_hmm_gmm_amd as khg
    phone, pdf_class, flags = khg.tid_tables(tm)
    return ref.acc_tree_stats(alis, feats, phone.tolist(), pdf_class.tolist(), flags.tolist(), N, P, ci)


def _check(got, want, what):
    keys = [tuple(int(v) for v in k) for k in got["keys"]]
    assert keys == sorted(want), what + ": keys"
    assert keys == sorted(keys) and len(set(keys)) == len(keys), what + ": order"
    worst = 0.0
    for i, k in enumerate(keys):
        w = want[k]
        assert got["count"][i] == w["n"], (what, k)
        for name, aname in (("x", "ax"), ("x2", "ax2")):
            err = np.abs(got[name][i] - np.asarray(w[name]))
            bound = w["n"] * U53 * np.asarray(w[aname])
            worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
            assert (err <= bound).all(), (what, k, name, err, bound)
    print(what, "keys", len(keys), "largest error / bound", worst)


def _utts(tm, mono, phone_seqs, seed, **kw):
    rng = np.random.default_rng(seed)
    return [cases.utterance(tm, mono, p, rng, **kw) if len(p) else np.zeros(0, np.int32) for p in phone_seqs]


SEQS = [[SIL, 2, 3, SIL], [4], [], [2, 2, 5, 3, SIL, 4, 2], [SIL], [5, SIL, SIL, 3], [3, 4]]


@pytest.fixture(scope="module")
def model():
    return cases.make_model([2, 3, 4, 5], SIL)


@pytest.mark.parametrize("N,P", [(1, 0), (2, 1), (3, 1), (3, 0), (3, 2), (2, 0)])
@pytest.mark.parametrize("dim", [1, 13, 40])
def test_equals_restatement(ctx, model, N, P, dim):
    tm, topo, mono = model
    alis = _utts(tm, mono, SEQS, 100 + dim)
    feats = cases.features([len(a) for a in alis], dim, 7)
    for ci in ((), (SIL,)):
        stats, status = _acc(ctx, tm, alis, feats, N, P, ci)
        assert (status == 0).all()
        want, wstatus = _want(tm, alis, feats, N, P, ci)
        assert wstatus == [0] * len(alis)
        _check(stats.download(), want, "N=%d P=%d dim=%d ci=%s" % (N, P, dim, ci))
        assert stats.num_keys() == len(want)


def test_one_frame_per_segment_and_silence_forward_arcs(ctx):
    """one-state phones without self-loops taken: every frame is a segment; the five-state silence taking different forward arcs"""
    tm1, _, mono1 = cases.make_model([2, 3, 4], SIL, non_sil_states=1, sil_states=1)
    alis = _utts(tm1, mono1, [[2, 3, 4, 2, SIL, 3], [4], [3, 3, 3]], 5, loops=0)
    assert [len(a) for a in alis] == [6, 1, 3]
    feats = cases.features([len(a) for a in alis], 13, 9)
    stats, status = _acc(ctx, tm1, alis, feats, 3, 1)
    assert (status == 0).all()
    _check(stats.download(), _want(tm1, alis, feats, 3, 1)[0], "one frame per segment")
    tm, _, mono = cases.make_model([2, 3], SIL)
    rng = np.random.default_rng(11)
    sil_paths = {tuple(cases.phone_alignment(tm, mono, SIL, rng, max_loops=2)) for _ in range(40)}
    fwd = {tuple(t for t in p if not tm.is_self_loop(t)) for p in sil_paths}
    assert len(fwd) >= 3, "the silence walks must differ in their forward arcs"
    alis = [np.asarray(list(p) + cases.phone_alignment(tm, mono, 2, rng) + list(q), np.int32) for p, q in zip(sorted(sil_paths)[:6], sorted(sil_paths)[6:12])]
    feats = cases.features([len(a) for a in alis], 13, 10)
    stats, status = _acc(ctx, tm, alis, feats, 3, 1, (SIL,))
    assert (status == 0).all()
    _check(stats.download(), _want(tm, alis, feats, 3, 1, (SIL,))[0], "silence forward arcs")


def _long_key_case(tm, mono, dim=13):
    """about 2 500 frames of one key (silence alone, context-independent: window 0 SIL 0 at one pdf-class via long self-loop runs) over
    several utterances, next to keys of one entry"""
    rng = np.random.default_rng(21)
    alis = []
    for n, nxt in ((900, 2), (1, 3), (700, 4), (950, 5)):
        a = cases.phone_alignment(tm, mono, SIL, rng, loops=0)
        sl = tm.self_loop_of(tm.transition_id_to_transition_state(a[-1]))
        alis.append(np.asarray(a + [sl] * n + cases.phone_alignment(tm, mono, nxt, rng, loops=0), np.int32))
    return alis, cases.features([len(a) for a in alis], dim, 22)


def test_long_key_crosses_the_slice(ctx, model):
    tm, topo, mono = model
    alis, feats = _long_key_case(tm, mono)
    want, _ = _want(tm, alis, feats, 3, 1, (SIL,))
    counts = sorted(w["n"] for w in want.values())
    assert counts[-1] > 2 * 1024 + 400 and counts[0] == 1
    stats, status = _acc(ctx, tm, alis, feats, 3, 1, (SIL,))
    assert (status == 0).all()
    got = stats.download()
    _check(got, want, "long key")
    again, _ = _acc(ctx, tm, alis, feats, 3, 1, (SIL,))
    g2 = again.download()
    for k in ("keys", "count", "x", "x2"):
        assert np.array_equal(got[k], g2[k]), "two runs: " + k


def test_invalid_alignments_are_skipped_bit_for_bit(ctx, model):
    tm, topo, mono = model
    alis = _utts(tm, mono, SEQS, 31)
    feats = cases.features([len(a) for a in alis], 13, 32)
    clean, _ = _acc(ctx, tm, alis, feats, 3, 1, (SIL,))
    rng = np.random.default_rng(33)
    good = cases.utterance(tm, mono, [2, 3, 4], rng)
    mid = good[:max(i for i in range(len(good)) if tm.is_final(int(good[i])))]        # cut before the last final id: ends mid-phone
    a3 = cases.phone_alignment(tm, mono, 3, rng, loops=1)
    a4 = cases.phone_alignment(tm, mono, 4, rng, loops=1)
    mixed = np.asarray(a3[:2] + a4[2:], np.int32)             # phone 3's first state, then phone 4's ids inside the same segment
    failed = np.zeros(7, np.int32)                            # what a failed khg_align leaves
    bad = [mid, mixed, failed]
    allu = alis[:2] + [bad[0]] + alis[2:4] + [bad[1]] + alis[4:] + [bad[2]]
    allf = feats[:2] + cases.features([len(bad[0])], 13, 34) + feats[2:4] + cases.features([len(bad[1])], 13, 35) + feats[4:] + cases.features([7], 13, 36)
    stats, status = _acc(ctx, tm, allu, allf, 3, 1, (SIL,))
    want, wstatus = _want(tm, allu, allf, 3, 1, (SIL,))
    assert status.tolist() == wstatus
    assert status[2] & ref.OPEN_END and status[5] & ref.MIXED_PHONES and status[len(allu) - 1] & ref.NO_ALI
    assert sorted(np.nonzero(status)[0].tolist()) == [2, 5, len(allu) - 1]
    a, b = clean.download(), stats.download()
    for k in ("keys", "count", "x", "x2"):
        assert np.array_equal(a[k], b[k]), k


def test_larger_batch_with_disjoint_phones_keeps_the_bits(ctx):
    tm, topo, mono = cases.make_model([2, 3, 4, 5, 6, 7], SIL)
    alis = _utts(tm, mono, [[2, 3, 2], [3], [2, 2, 3, 3, 2]], 41)
    feats = cases.features([len(a) for a in alis], 13, 42)
    small, _ = _acc(ctx, tm, alis, feats, 3, 1)
    other = _utts(tm, mono, [[5, 6, 7, 5], [6], [7, 7, 5, 6], [5, 5]], 43)
    of = cases.features([len(a) for a in other], 13, 44)
    big, status = _acc(ctx, tm, [other[0], alis[0], other[1], other[2], alis[1], alis[2], other[3]], [of[0], feats[0], of[1], of[2], feats[1], feats[2], of[3]], 3, 1)
    assert (status == 0).all()
    a, b = small.download(), big.download()
    assert len(b["keys"]) > len(a["keys"])
    where = {tuple(k): i for i, k in enumerate(b["keys"].tolist())}
    for i, k in enumerate(a["keys"].tolist()):
        j = where[tuple(k)]
        assert a["count"][i] == b["count"][j] and np.array_equal(a["x"][i], b["x"][j]) and np.array_equal(a["x2"][i], b["x2"][j]), k


def test_two_sets_into_one_handle_equal_add_of_two_handles(ctx, model):
    from kaldi_hmm_gmm_amd import DeviceTreeStats
    tm, topo, mono = model
    a1 = _utts(tm, mono, [[SIL, 2, 3, SIL], [4, 5], [2]], 51)
    a2 = _utts(tm, mono, [[SIL, 2, 3, SIL, 5], [3, 3], [4, 5, 2]], 52)       # overlapping and new keys
    f1, f2 = cases.features([len(a) for a in a1], 13, 53), cases.features([len(a) for a in a2], 13, 54)
    both, _ = _acc(ctx, tm, a1, f1, 3, 1, (SIL,))
    _acc(ctx, tm, a2, f2, 3, 1, (SIL,), stats=both)
    h1, _ = _acc(ctx, tm, a1, f1, 3, 1, (SIL,))
    h2, _ = _acc(ctx, tm, a2, f2, 3, 1, (SIL,))
    k1, k2 = {tuple(k) for k in h1.download()["keys"].tolist()}, {tuple(k) for k in h2.download()["keys"].tolist()}
    assert k1 & k2 and k1 - k2 and k2 - k1
    h1.add(1.0, h2)
    a, b = both.download(), h1.download()
    for k in ("keys", "count", "x", "x2"):
        assert np.array_equal(a[k], b[k]), k
    _check(a, _want(tm, a1 + a2, f1 + f2, 3, 1, (SIL,))[0], "two calls")
    # disjoint keys: another phone inventory in the second handle
    d1 = _utts(tm, mono, [[2, 2], [2]], 55)
    d2 = _utts(tm, mono, [[4, 5], [5]], 56)
    g1, g2 = cases.features([len(a) for a in d1], 13, 57), cases.features([len(a) for a in d2], 13, 58)
    s1, _ = _acc(ctx, tm, d1, g1, 3, 1)
    s2, _ = _acc(ctx, tm, d2, g2, 3, 1)
    s1.add(1.0, s2)
    _check(s1.download(), _want(tm, d1 + d2, g1 + g2, 3, 1)[0], "disjoint add")
    with pytest.raises(Exception):
        s1.add(1.0, DeviceTreeStats(ctx, 13, 2, 1))
    with pytest.raises(Exception):
        s1.add(1.0, s1)


def test_download_upload_round_trip_and_refusals(ctx, model):
    from kaldi_hmm_gmm_amd import DeviceTreeStats, KhgError
    tm, topo, mono = model
    alis = _utts(tm, mono, SEQS, 61)
    feats = cases.features([len(a) for a in alis], 13, 62)
    stats, _ = _acc(ctx, tm, alis, feats, 3, 1)
    a = stats.download()
    other = DeviceTreeStats(ctx, 13, 3, 1)
    other.upload(a["keys"], a["count"], a["x"], a["x2"])
    b = other.download()
    for k in ("keys", "count", "x", "x2"):
        assert np.array_equal(a[k], b[k]), k
    other.zero()
    assert other.num_keys() == 0 and other.download()["keys"].shape == (0, 4)
    with pytest.raises(KhgError, match="ascend"):
        other.upload(a["keys"][::-1].copy(), a["count"], a["x"], a["x2"])
    with pytest.raises(KhgError, match="N = 4"):
        DeviceTreeStats(ctx, 13, 4, 1)
    with pytest.raises(KhgError):
        DeviceTreeStats(ctx, 13, 3, 3)
    us = _upload(ctx, alis, feats)
    phone, pdf_class, flags = __import__("kaldi_hmm_gmm_amd").tid_tables(tm)
    none = np.zeros(0, np.int32)
    before = stats.download()
    big = phone.copy(); big[3] = 70000
    with pytest.raises(KhgError, match="70000"):
        us._acc_tree_stats(big, pdf_class, flags, none, stats)
    pc = pdf_class.copy(); pc[3] = 300
    with pytest.raises(KhgError, match="300"):
        us._acc_tree_stats(phone, pc, flags, none, stats)
    with pytest.raises(KhgError, match="dimension"):
        us._acc_tree_stats(phone, pdf_class, flags, none, DeviceTreeStats(ctx, 12, 3, 1))
    after = stats.download()
    for k in ("keys", "count", "x", "x2"):
        assert np.array_equal(before[k], after[k]), k
