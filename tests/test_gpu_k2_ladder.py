"""The ladder form of K2's exact DP (k2_viterbi_dp<1, 2, true, false, SC, true>: costs move between lanes in registers, the waves of
an utterance run one group of eight layers apart, one workgroup barrier per group) on the inputs of tests/k2_ladder_cases.py: the
getter names it exactly where the batch's graphs are in chain order, every output is byte for byte what the general body (option
k2_ladder = 1) gives, the answers are the oracle's FasterDecoder's at a wide beam and at a beam that splits the batch, and the
certificate bit is the restatement's (tests/k2_dp_ref.py) -- which pins layer_best / layer_cnt, the certificate's only inputs."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import k2_dp_cases as kc  # noqa: E402
import k2_ladder_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu

EXACT_DP, FALLBACK = 4, 8
KEYS = ("ali", "words", "words_off", "like", "status")


def _device(ctx, c):
    from kaldi_hmm_gmm_amd import DeviceTransitions, UtteranceSet
    tm = DeviceTransitions(ctx, kc.ID2PDF)
    us = UtteranceSet(ctx, tm, c.frame_off, np.zeros((int(c.frame_off[-1]), 2), np.float32), graphs=kc.concat(c.graphs))
    poff, pdfs = us.pdf_lists()
    for u, p in enumerate(c.pdfs):
        assert np.array_equal(pdfs[poff[u]: poff[u + 1]], p), u
    us.upload_loglikes(c.mats)
    return tm, us


def _same_bytes(x, y, what):
    for k in KEYS:
        assert np.asarray(x[k]).dtype == np.asarray(y[k]).dtype and np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes(), (what, k)


def _utt(c, res, u):
    return (res["ali"][c.frame_off[u]: c.frame_off[u + 1]], res["words"][res["words_off"][u]: res["words_off"][u + 1]],
            float(res["like"][u]), int(res["status"][u]))


def _against_oracle(c, res, u, kw):
    want = kc.oracle_align(c, u, **kw)
    assert not want["status"] & 2
    a, w, lk, st = _utt(c, res, u)
    what = (c.name, u, len(c.graphs[u]["final"]), c.T[u], kw)
    assert (st & 3) == (want["status"] & 1), (what, st)
    if want["status"] & 1:
        assert (a == 0).all() and not st & EXACT_DP, what
        return
    assert bool(st & EXACT_DP) != bool(st & FALLBACK), (what, st)
    assert np.array_equal(a, want["ali"]) and np.array_equal(w, want["words"]), what
    assert lk == pytest.approx(want["like"], rel=1e-6, abs=1e-4), what


def _both(ctx, opt, c, us, tm):
    """-> results per configuration with the ladder option on; asserts the getter, the unchanged plan and byte equality with the
    option off"""
    opt("k2_ladder", 0)
    plan = us.k2_plan(ctx)
    assert (plan["KS"], plan["DEG"], plan["FAST"], plan["SC"], plan["GMEM"]) == c.plan[:3] + (c.plan[3], False)
    assert us.k2_ladder(ctx) == c.ladder, c.name
    on = [us.align(tm, acoustic_scale=c.scale, **kw) for kw in c.cfgs]
    opt("k2_ladder", 1)
    assert us.k2_plan(ctx) == plan and not us.k2_ladder(ctx)
    off = [us.align(tm, acoustic_scale=c.scale, **kw) for kw in c.cfgs]
    opt("k2_ladder", 0)
    for kw, x, y in zip(c.cfgs, on, off):
        _same_bytes(x, y, (c.name, kw))
    return on


def _certificates(c, on):
    for kw, res in zip(c.cfgs, on):
        want = [r.certified(**kw) for r in c.ref]
        got = [bool(int(res["status"][u]) & EXACT_DP) for u in range(len(c.ref))]
        print(c.name, kw, "EXACT_DP on %d of %d utterances, the restatement certifies %d" % (sum(got), len(got), sum(want)))
        assert got == want, (c.name, kw, [u for u in range(len(got)) if got[u] != want[u]])
    return want


@pytest.mark.parametrize("name", ["sizes", "sizes_rows", "mixed"])
def test_ladder_form(ctx, opt, name):
    c = lc.case(name)
    tm, us = _device(ctx, c)
    on = _both(ctx, opt, c, us, tm)
    for kw, res in zip(c.cfgs[:2], on):                    # a wide beam; a beam that splits the batch
        for u in range(len(c.graphs)):
            _against_oracle(c, res, u, kw)
    _certificates(c, on)
    last = [r.certified(**c.cfgs[1]) for r in c.ref if r.ok]
    assert any(last) and not all(last), "the narrow beam must split the batch"
    assert all((int(on[0]["status"][u]) & 3) == 1 for u, r in enumerate(c.ref) if not r.ok)
    us.close(); tm.close()


@pytest.mark.parametrize("name", ["constant", "boundary_tie"])
def test_ties_go_to_the_order_faithful_decoder(ctx, opt, name):
    """constant: every merge is a tie; boundary_tie: the only tie sits on state 64's cell, whose forward arc's source is lane 63 of
    the wave below.  A tie on the path is never certified -- with the ladder form exactly as without it"""
    c = lc.case(name)
    tm, us = _device(ctx, c)
    on = _both(ctx, opt, c, us, tm)
    for kw, res in zip(c.cfgs, on):
        st = np.asarray(res["status"])
        assert not (st & EXACT_DP).any() and (st & FALLBACK).all() and not (st & 3).any(), (name, kw, st)
        for u in range(len(c.graphs)):
            _against_oracle(c, res, u, kw)
    _certificates(c, on)
    us.close(); tm.close()


def test_permuted_states_take_the_general_body(ctx, opt):
    """the graphs of "sizes" renumbered: `ladder` is false, the plan is the same, the alignments are those of the chain-ordered run"""
    c, b = lc.case("permuted"), lc.case("sizes")
    tm, us = _device(ctx, c)
    on = _both(ctx, opt, c, us, tm)
    tmb, usb = _device(ctx, b)
    assert usb.k2_ladder(ctx) and usb.k2_plan(ctx)["nthr"] == us.k2_plan(ctx)["nthr"] == 256
    for kw, res in zip(c.cfgs[:1], on):                    # (the wide beam: nothing is pruned, the numbering cannot matter)
        base = usb.align(tmb, acoustic_scale=b.scale, **kw)
        for u, k in enumerate(c.of):
            a, w, lk, st = _utt(c, res, u)
            a2, w2, lk2, st2 = _utt(b, base, k)
            assert np.array_equal(a, a2) and np.array_equal(w, w2) and lk == lk2 and (st & 3) == (st2 & 3), (u, k, kw)
    for u in range(len(c.graphs)):
        _against_oracle(c, on[1], u, c.cfgs[1])
    _certificates(c, on)
    us.close(); tm.close(); usb.close(); tmb.close()


def test_in_degree_three_keeps_its_plan(ctx, opt):
    c = lc.case("indeg3")
    tm, us = _device(ctx, c)
    on = _both(ctx, opt, c, us, tm)
    for u in range(len(c.graphs)):
        _against_oracle(c, on[0], u, c.cfgs[0])
    _certificates(c, on)
    us.close(); tm.close()


def test_getter_refuses_a_set_without_graphs(ctx):
    from kaldi_hmm_gmm_amd import UtteranceSet
    us = UtteranceSet(ctx, None, np.array([0, 5], np.int64), np.zeros((5, 2), np.float32))
    for fn in (us.k2_plan, us.k2_ladder):
        with pytest.raises(Exception, match="no decoding graphs"):
            fn(ctx)
    us.close()
