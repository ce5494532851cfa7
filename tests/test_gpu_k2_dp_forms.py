"""Every instantiation of the exact-DP aligner kernel (k2_viterbi_dp<KS, DEG, FAST, GMEM, SC>, csrc/khg_k2_viterbi.hip.inc) on inputs
built for it (tests/k2_dp_cases.py; their properties are shown on the CPU by tests/test_k2_dp_cases_cpu.py): the form that runs is the
one the case names (UtteranceSet.k2_plan), its answers are the oracle's FasterDecoder's at a wide beam, at a beam that splits the
batch and with min_active in play, and its certificate bit (KHG_ALIGN_EXACT_DP) is the restatement's certified(...) -- both are
fixed arithmetic, so on every utterance: a certificate too lax would hand out a path the reference prunes, one too strict would
send everything to the order-faithful decoders unnoticed.  The HBM-scratch form keeps its own test
(tests/test_gpu_shared_graph.py).  These batches send what they do not certify to the chain decoder at out-degree 2 and 3;
test_chain_decoder_at_out_degree runs it at 1 and 4."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import k2_dp_cases as kc  # noqa: E402

pytestmark = pytest.mark.gpu

EXACT_DP, FALLBACK = 4, 8


def _device(ctx, c):
    from kaldi_hmm_gmm_amd import DeviceTransitions, UtteranceSet
    tm = DeviceTransitions(ctx, kc.ID2PDF)
    us = UtteranceSet(ctx, tm, c.frame_off, np.zeros((int(c.frame_off[-1]), 2), np.float32), graphs=kc.concat(c.graphs))
    poff, pdfs = us.pdf_lists()
    for u, p in enumerate(c.pdfs):                         # the rows of the score matrices are the set's own pdf lists
        assert np.array_equal(pdfs[poff[u]: poff[u + 1]], p), u
    us.upload_loglikes(c.mats)
    return tm, us


def _utt(c, res, u):
    return (res["ali"][c.frame_off[u]: c.frame_off[u + 1]], res["words"][res["words_off"][u]: res["words_off"][u + 1]],
            float(res["like"][u]), int(res["status"][u]))


def _against(c, res, u, ok, ali, words, like, what):
    a, w, lk, st = _utt(c, res, u)
    assert (st & 3) == (0 if ok else 1), (what, st)
    if not ok:
        assert (a == 0).all() and not st & EXACT_DP, what
        return
    assert bool(st & EXACT_DP) != bool(st & FALLBACK), (what, st)
    assert np.array_equal(a, ali), what
    assert np.array_equal(w, words), what
    assert lk == pytest.approx(like, rel=1e-6, abs=1e-4), what


def _against_oracle(c, res, u, kw):
    want = kc.oracle_align(c, u, **kw)
    assert not want["status"] & 2
    _against(c, res, u, not want["status"] & 1, want["ali"], want["words"], want["like"], (c.name, u, kw, "oracle"))


def _same_bytes(x, y, what):
    for k in ("ali", "words", "words_off", "like", "status"):
        assert np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes(), (what, k)


@pytest.mark.parametrize("name", kc.ALL)
def test_form(ctx, opt, name):
    c = kc.case(name)
    tm, us = _device(ctx, c)
    U = len(c.graphs)
    big = [len(g["final"]) > 300 for g in c.graphs]
    tie_free = name in kc.TIE_FREE
    fast = c.plan[2]
    # ---- the plan: the form this case is named after
    opt("k2_ks", c.k2_ks)
    plan = us.k2_plan(ctx)
    print(name, "plan", plan)
    KS, DEG, FAST, SC = c.plan
    assert (plan["KS"], plan["DEG"], plan["FAST"], plan["SC"], plan["GMEM"]) == (KS, DEG, FAST, SC, False)
    assert plan["nthr"] == c.expected_nthr() and 0 < plan["lds_bytes"] <= 160 * 1024
    f = kc.batch_facts(c)
    chain = not f["eps"] and f["S"] <= 1000 and f["outdeg"] <= 4          # (its tables fit at these sizes: 257 states, out-degree <= 3)
    assert plan["faithful_form"] == 4 if chain else plan["faithful_form"] in (2, 3)
    record = {"form": name, "plan": plan, "utterances": U, "certified": []}
    results = []
    for ki, kw in enumerate(c.cfgs):
        res = us.align(tm, acoustic_scale=c.scale, **kw)
        results.append(res)
        want_cert = [r.certified(**kw) for r in c.ref]
        got_cert = [bool(int(res["status"][u]) & EXACT_DP) for u in range(U)]
        record["certified"].append({"config": kw, "kernel": sum(got_cert), "restatement": sum(want_cert) if name != "generic_eps" else None})
        print(name, kw, "EXACT_DP on %d of %d utterances, the restatement certifies %d" % (sum(got_cert), U, sum(want_cert)))
        for u, r in enumerate(c.ref):
            what = (name, u, kw)
            # ---- results: the oracle's FasterDecoder; the restatement on the graphs of > 1024 states at beam 200
            if big[u] and ki == 0:
                _against(c, res, u, r.ok, r.ali, r.words, r.like, what + ("restatement",))
            else:
                _against_oracle(c, res, u, kw)
            if r.ok and want_cert[u] and name != "generic_eps":
                _against(c, res, u, True, r.ali, r.words, r.like, what + ("restatement, certified",))
            # ---- the certificate bit
            if tie_free or fast:
                assert got_cert[u] == want_cert[u], what + (got_cert[u], want_cert[u], r.required_beam if r.ok else None)
            elif got_cert[u]:
                assert not r.any_tie, what                  # generic form with ties: EXACT_DP implies no tie anywhere
        if tie_free and ki == 0:
            assert all(got_cert[u] for u, r in enumerate(c.ref) if r.ok), "beam 200 must certify every utterance that reaches a final state"
    # ---- max_active set: nothing is certified, the order-faithful decoders decide, same answers
    kw = dict(beam=200.0, max_active=1000)
    res = us.align(tm, acoustic_scale=c.scale, **kw)
    assert not (res["status"] & EXACT_DP).any()
    for u in range(U):
        _against_oracle(c, res, u, kw)
    # ---- launch order: utterances in index order instead of longest first
    opt("k2_inorder", 1)
    _same_bytes(us.align(tm, acoustic_scale=c.scale, **c.cfgs[1]), results[1], "k2_inorder")
    opt("k2_inorder", 0)
    # ---- a forced KS against the form the dispatch picks by itself on the same batch
    if c.k2_ks:
        opt("k2_ks", 0)
        auto = us.k2_plan(ctx)
        assert (auto["KS"], auto["DEG"], auto["SC"]) == (1, 2 if f["indeg"] <= 2 else 3, f["same_row"]) and auto["nthr"] == 320
        for kw, forced in zip(c.cfgs, results):
            _same_bytes(us.align(tm, acoustic_scale=c.scale, **kw), forced, ("k2_ks", c.k2_ks, kw))
    print("k2_dp_form_record " + json.dumps(record))
    us.close(); tm.close()


@pytest.mark.parametrize("odeg", [1, 4])
def test_chain_decoder_at_out_degree(ctx, opt, odeg):
    """k2_viterbi_faithful_chain<1> and <4>, the two rows of the kernel table (k2_insts, csrc/khg_k2.hip) that no batch of test_form
    reaches (theirs have out-degree 2, 3 or 6): with max_active set nothing is certified and the chain decoder decides every
    utterance -- the oracle's FasterDecoder's answers, and byte for byte the one-lane emulation's (k2_serial = 1).  The plan says
    "chain" and the batch has the out-degree; WHICH instantiation ran is not observable from here: that the table's row for ODEG
    points at chain<ODEG> rests on the kernel trace of these two tests (profiles/k2_table_ab.txt, part 4)."""
    c = kc.chain_case(odeg)
    tm, us = _device(ctx, c)
    f = kc.batch_facts(c)
    assert len(c.T) == 3 and all(8 <= t <= 30 for t in c.T) and not f["eps"] and f["S"] <= 20 and f["outdeg"] == odeg
    for kw in (dict(beam=200.0, max_active=1000), dict(beam=4.0, max_active=1000, min_active=0)):
        opt("k2_serial", 0)
        assert us.k2_plan(ctx)["faithful_form"] == 4
        res = us.align(tm, acoustic_scale=c.scale, **kw)
        assert not (res["status"] & EXACT_DP).any()
        for u in range(3):
            _against_oracle(c, res, u, kw)
        opt("k2_serial", 1)
        assert us.k2_plan(ctx)["faithful_form"] == 0
        _same_bytes(us.align(tm, acoustic_scale=c.scale, **kw), res, ("one-lane emulation", odeg, kw))
    us.close(); tm.close()
