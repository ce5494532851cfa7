"""The tail of K2's exact DP (KHG_OPT_K2_TAIL, csrc/khg_k2_viterbi.hip.inc: the trace-back on packed source words, the replay's fp64
cost chain as a wave scan where that is exact) on the batches of tests/k2_tail_cases.py: every output is byte for byte what the loops
it replaced give (option k2_tail = 1), the answers are the oracle's FasterDecoder's, and the number of replay batches that took the
scan and the serial loop, per utterance (UtteranceSet.k2_tail under option k2_prof), is what the numpy restatement of the rule
predicts for the path's addends -- so each branch is known to have run where the case means it to.  The properties of the batches:
tests/test_k2_tail_cpu.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import k2_dp_cases as kc  # noqa: E402
import k2_tail_cases as tc  # noqa: E402

pytestmark = pytest.mark.gpu

EXACT_DP, FALLBACK = 4, 8
KEYS = ("ali", "like", "words", "words_off", "status")


def _device(ctx, c):
    from kaldi_hmm_gmm_amd import DeviceTransitions, UtteranceSet
    tm = DeviceTransitions(ctx, kc.ID2PDF)
    us = UtteranceSet(ctx, tm, c.frame_off, np.zeros((int(c.frame_off[-1]), 2), np.float32), graphs=kc.concat(c.graphs))
    poff, pdfs = us.pdf_lists()
    for u, p in enumerate(c.pdfs):
        assert np.array_equal(pdfs[poff[u]: poff[u + 1]], p), u
    us.upload_loglikes(c.mats)
    return tm, us


def _against_oracle(c, res, u):
    """the comparison of tests/test_gpu_k2_dp_forms.py"""
    want = kc.oracle_align(c, u, **c.cfg)
    assert not want["status"] & 2
    a = res["ali"][c.frame_off[u]: c.frame_off[u + 1]]
    w = res["words"][res["words_off"][u]: res["words_off"][u + 1]]
    lk, st = float(res["like"][u]), int(res["status"][u])
    what = (c.name, u, len(c.graphs[u]["final"]), c.T[u])
    assert (st & 3) == (want["status"] & 1), (what, st)
    if want["status"] & 1:
        assert (a == 0).all() and not st & EXACT_DP, what
        return
    assert bool(st & EXACT_DP) != bool(st & FALLBACK), (what, st)
    assert np.array_equal(a, want["ali"]) and np.array_equal(w, want["words"]), what
    assert lk == pytest.approx(want["like"], rel=1e-6, abs=1e-4), what


def _run(ctx, opt, c, ladder, deg=2):
    tm, us = _device(ctx, c)
    plan = us.k2_plan(ctx)
    assert (plan["KS"], plan["DEG"], plan["FAST"], plan["GMEM"]) == (1, deg, True, False), plan
    assert us.k2_ladder(ctx) == ladder, c.name
    opt("k2_prof", 1)
    opt("k2_tail", 0)
    new = us.align(tm, acoustic_scale=c.scale, **c.cfg)
    got = np.asarray(us.k2_tail()).reshape(-1, 2)
    opt("k2_tail", 1)
    old = us.align(tm, acoustic_scale=c.scale, **c.cfg)
    got_old = np.asarray(us.k2_tail()).reshape(-1, 2)
    opt("k2_tail", 0)
    opt("k2_prof", 0)
    for k in KEYS:
        assert np.asarray(new[k]).dtype == np.asarray(old[k]).dtype and np.asarray(new[k]).tobytes() == np.asarray(old[k]).tobytes(), (c.name, k)
    for u in range(len(c.T)):
        _against_oracle(c, new, u)
    want = np.array([tc.expected_batches(c, u) for u in range(len(c.T))])
    print(c.name, "replay batches scanned / serial:", want.sum(0).tolist(), "kernel:", got.sum(0).tolist())
    assert np.array_equal(got, want), (c.name, [(u, got[u].tolist(), want[u].tolist()) for u in range(len(want)) if (got[u] != want[u]).any()])
    assert (got_old[:, 0] == 0).all() and np.array_equal(got_old[:, 1], want.sum(1)), "option off: every batch in the serial loop"
    us.close(); tm.close()
    return new


@pytest.mark.parametrize("permuted", [False, True], ids=["ladder", "general"])
@pytest.mark.parametrize("table", tc.TABLES)
def test_tail(ctx, opt, table, permuted):
    c = tc.case(table, permuted)
    res = _run(ctx, opt, c, ladder=not permuted)
    st = np.asarray(res["status"])
    assert not (st & 3).any()
    tie = np.array([r.path_tie or r.final_tie for r in c.ref])
    assert not (st[tie] & EXACT_DP).any() and (st[tie] & FALLBACK).all(), "a tie on the path or at the end goes to the order-faithful decoder"
    if table == "ties":
        assert tie.sum() >= 5
    want = [r.certified(**c.cfg) for r in c.ref]           # the certificate bit is the restatement's (tests/k2_dp_ref.py)
    assert [bool(x & EXACT_DP) for x in st] == want, (c.name, st.tolist(), want)


def test_in_degree_three(ctx, opt):
    _run(ctx, opt, tc.case("random", False, "deg3"), ladder=False, deg=3)
    _run(ctx, opt, tc.case("tiny", False, "deg3"), ladder=False, deg=3)


def test_more_than_256_states_keeps_the_general_trace_back(ctx, opt):
    """not on the eight-layers-per-step path: its trace-back is unchanged, the replay is the new one"""
    _run(ctx, opt, tc.case("random", False, "wide"), ladder=False)
    _run(ctx, opt, tc.case("tiny", False, "wide"), ladder=False)
