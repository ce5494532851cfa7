"""What tests/test_gpu_k2_dp_forms.py rests on, shown without a GPU: the batches of tests/k2_dp_cases.py have the facts that select
the instantiation of k2_viterbi_dp they are named after, the tie-free ones are free of ties, the narrow beam splits every batch,
the tie batches have their ties on the path -- and the restatement (tests/k2_dp_ref.py) is the oracle's FasterDecoder wherever it
claims to be: the same path at beam 200, and the same answer at the narrow beams wherever its certificate holds."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import k2_dp_cases as kc  # noqa: E402
import k2_dp_ref as ref  # noqa: E402


def test_k2_plan_entry_point():
    name = "khg_utts_k2_plan"
    with open(os.path.join(ROOT, "include", "khg_hip.h")) as fh:
        header = fh.read()
    from kaldi_hmm_gmm_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "kaldi_hmm_gmm_amd", "libkhg_hip.so")], capture_output=True, text=True,
                         check=True).stdout
    assert re.search(r"\bint %s\(" % name, header) and name in _lib.SIGNATURES and re.search(r" T %s$" % name, out, re.M)
    assert getattr(_lib.lib, name) is not None
    import kaldi_hmm_gmm_amd as khg
    assert hasattr(khg.UtteranceSet, "k2_plan")


def test_step_down_is_the_float_below_the_rounded_minimum():
    for x in (0.0, 1.0, -1.0, 3.3, -3.3, 1e-30, 16777217.0):
        f = np.float32(x)
        d = ref.step_down(x)
        assert d < float(f) and np.float32(d) == d and np.nextafter(np.float32(d), np.float32(np.inf)) == f
    assert ref.step_down(0.0) == -float(np.float32(1.401298464324817e-45))


@pytest.mark.parametrize("name", kc.ALL)
def test_batch_facts_select_the_form(name):
    """the dispatch of csrc/khg_k2.hip (k2_plan) in words: what each form needs of the batch's largest graph, largest in-degree,
    epsilon arcs and score rows"""
    c = kc.case(name)
    f = kc.batch_facts(c)
    KS, DEG, FAST, SC = c.plan
    print(name, f, "utterances", len(c.graphs), "frames", int(c.frame_off[-1]))
    assert FAST == (not f["eps"] and f["indeg"] <= 6)
    if name == "generic_eps":
        assert f["eps"] and f["indeg"] > 6
    elif name == "generic_deg7":
        assert f["indeg"] == 7 and not f["eps"]
    elif DEG == 6:
        assert 4 <= f["indeg"] <= 6 and f["S"] <= 1024
    elif DEG == 3 and c.k2_ks == 3:
        assert f["indeg"] == 2                                         # the three-slot form is FORCED onto in-degree 2
    elif DEG == 3:
        assert f["indeg"] == 3
    else:
        assert f["indeg"] == 2
    if FAST and DEG != 6 and c.k2_ks != 3 and not (KS > 1 and DEG == 3):
        assert SC == f["same_row"]
    if name in kc.NATURAL:
        assert c.k2_ks == 0 and (1024 < f["S"] <= 2048 if KS == 2 else 2048 < f["S"] <= 4096)
        assert KS == 2 or f["inarcs"] <= 2.2 * f["S"]                # (more in-arcs: the DP's tables leave LDS, the HBM-scratch form runs)
    elif FAST:
        assert f["S"] == 257 and c.k2_ks == (KS if KS > 1 else c.k2_ks) and f["S"] <= 1024 * KS
        sizes = {len(g["final"]) for g in c.graphs}
        assert set(kc.SIZES) <= sizes and (KS == 1 or {64 * KS - 1, 64 * KS, 64 * KS + 1} <= sizes)
        assert c.expected_nthr() == {1: 320, 2: 192, 4: 128}[KS]
    assert {2, 65} <= {len(g["final"]) for g in c.graphs} and any(g["start"] != 0 for g in c.graphs)
    if name != "generic_eps":
        # lengths: the shortest path, one below it (no final state: ERROR), and the lengths around the 8-layer and 32-layer folds
        bad = [u for u, r in enumerate(c.ref) if not r.ok]
        if name in kc.FORMS:
            assert len(bad) == 1 and c.T[bad[0]] == kc.shortest(65, c.hop) - 1
            for S in kc.SIZES:
                sp = kc.shortest(S, c.hop)
                Ts = {t for g, t in zip(c.graphs, c.T) if len(g["final"]) == S}
                assert sp in Ts and {t for t in kc.LENGTHS if t >= sp} <= Ts, (S, Ts)
        else:
            assert not bad


@pytest.mark.parametrize("name", kc.TIE_FREE)
def test_tie_free_batches_have_no_tie_and_beam_200_certifies_them(name):
    c = kc.case(name)
    assert not any(r.any_tie or r.final_tie for r in c.ref)
    assert all(r.certified(200.0) for r in c.ref if r.ok)
    assert not any(r.certified(200.0, max_active=1000) for r in c.ref)


@pytest.mark.parametrize("name", kc.TIE_FREE)
def test_the_median_beam_splits_the_batch(name):
    c = kc.case(name)
    n = len(c.ref)
    for kw in c.cfgs[1:]:
        yes = sum(r.certified(**kw) for r in c.ref)
        print(name, kw, "certified", yes, "of", n)
        assert 4 * yes >= n and 4 * (n - yes) >= n, (kw, yes, n)
    assert c.cfgs[2]["min_active"] == c.median_live > 0


@pytest.mark.parametrize("name", ["tie_1_3", "tie_1_6"])
def test_tie_batches_have_ties_on_the_path(name):
    c = kc.case(name)
    n = sum(r.ok and r.path_tie for r in c.ref)
    print(name, "on-path ties in", n, "of", len(c.ref))
    assert 4 * n >= len(c.ref)
    assert {3: 3, 6: 6}[c.plan[1]] == kc.batch_facts(c)["indeg"]


def _same(r, want, what):
    assert (want["status"] & 1) == (0 if r.ok else 1), what
    if r.ok:
        assert np.array_equal(r.ali, want["ali"]) and np.array_equal(r.words, want["words"]), what
        assert r.like == pytest.approx(want["like"], rel=1e-6, abs=1e-4), what


@pytest.mark.parametrize("name", kc.ALL)
def test_restatement_against_the_oracle(name):
    """beam 200: the restatement's path is the oracle's (small cases; with ties only where the restatement saw none on its path);
    narrow beams: wherever certified(...) holds the oracle's FasterDecoder at that beam returns the restatement's answer -- the
    certificate is sound against the reference's decoder."""
    c = kc.case(name)
    checked = [0, 0]
    for u, r in enumerate(c.ref):
        small = len(c.graphs[u]["final"]) <= 300
        if small and not ((r.path_tie or r.final_tie) and r.ok):
            want = kc.oracle_align(c, u, beam=200.0)
            assert want["status"] & 3 == (0 if r.ok else 1)
            _same(r, want, (name, u))
            checked[0] += 1
        for kw in c.cfgs[1:]:
            if r.certified(**kw):
                want = kc.oracle_align(c, u, **kw)
                assert want["status"] == 0, (name, u, kw)
                _same(r, want, (name, u, kw))
                checked[1] += 1
    print(name, "paths compared at beam 200: %d, certified answers compared at narrow beams: %d" % tuple(checked))
    assert checked[0] >= 3 and checked[1] >= 3


@pytest.mark.parametrize("odeg", [1, 4])
def test_chain_cases_have_the_out_degree_they_are_named_after(odeg):
    """the batches of test_chain_decoder_at_out_degree (tests/test_gpu_k2_dp_forms.py): what selects k2_viterbi_faithful_chain<odeg>,
    and every utterance reaches a final state -- the restatement's path is the oracle's with max_active set as that test sets it"""
    c = kc.chain_case(odeg)
    f = kc.batch_facts(c)
    assert len(c.T) == 3 and all(8 <= t <= 30 for t in c.T) and not f["eps"] and f["S"] <= 20 and f["outdeg"] == odeg
    assert len({int(np.diff(g["arc_off"]).max()) for g in c.graphs}) == 1        # every graph of the batch, not only the largest
    for u, r in enumerate(c.ref):
        want = kc.oracle_align(c, u, beam=200.0, max_active=1000)
        assert r.ok and want["status"] & 3 == 0
        if not (r.path_tie or r.final_tie):
            _same(r, want, (odeg, u))
