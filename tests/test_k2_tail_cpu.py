"""The tail of K2's exact DP without a device (KHG_OPT_K2_TAIL, csrc/khg_k2_viterbi.hip.inc): the rule under which the replay's fp64
cost chain runs as a wave scan (restated in tests/k2_tail_cases.py) does what the kernel's comment claims -- on addend lists that
satisfy it the serial chain, a Hillis-Steele scan and the kernel's own scan order agree bit for bit -- and it refuses every list built
to break one of its clauses, one of which really does make scan and chain differ.  Also: the option and its getter are declared,
exported, bound and in the environment table, and the batches of tests/test_gpu_k2_tail.py are what that test takes them for."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import k2_tail_cases as tc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
KHG_E_ARG = -1


def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def _lists():
    """seeded addend lists (w, ac) that satisfy the rule: random floats, grids, mixed signs, zeros of both signs, a wide exponent range"""
    rng = np.random.default_rng(5150)
    out = []
    for n in (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64):
        out.append((rng.random(n).astype(F32), (-3.0 * rng.random(n)).astype(F32) * F32(0.7)))
        out.append(((rng.integers(-512, 512, n) / 1024.0).astype(F32), (rng.integers(-4096, 4096, n) / 1024.0).astype(F32)))
        out.append((np.where(rng.random(n) < 0.5, 0.0, -0.0).astype(F32), np.where(rng.random(n) < 0.5, 0.0, -0.0).astype(F32)))
        out.append(((rng.random(n) * 2.0 ** rng.integers(-12, 4, n)).astype(F32), (-rng.random(n) * 2.0 ** rng.integers(-12, 4, n)).astype(F32)))
    return out


def test_scan_equals_serial_chain_where_the_rule_holds():
    for w, ac in _lists():
        assert tc.exact_ok(np.concatenate([w, ac])), (len(w), w[:4], ac[:4])
        for cost in (0.0, 1234.5):                         # a first batch, and a later one whose incoming cost is on the grid (a multiple of 0.5)
            if cost and not tc.exact_ok(np.concatenate([w, ac, [F32(cost)]])):
                continue
            want = tc.serial_chain(w, ac, cost)
            d = w.astype(np.float64) + ac.astype(np.float64)
            d[0] = cost + d[0]
            assert np.array_equal(_bits(tc.hillis_steele(d)), _bits(want)), len(w)
            assert np.array_equal(_bits(tc.scanned_chain(w, ac, cost)), _bits(want)), len(w)


def test_long_utterance_batch_by_batch():
    """300 entries in batches of 64, the cost carried from batch to batch as the kernel carries it"""
    rng = np.random.default_rng(77)
    w, ac = rng.random(300).astype(F32), (8.0 * rng.random(300)).astype(F32) * F32(0.1)
    assert tc.batch_plan(w, ac) == (5, 0)
    want, cost, got = tc.serial_chain(w, ac), 0.0, []
    for b in range(0, 300, 64):
        ca = tc.scanned_chain(w[b: b + 64], ac[b: b + 64], cost)
        got.append(ca)
        cost = ca[-1]
    assert np.array_equal(_bits(np.concatenate(got)), _bits(want))


def test_the_rule_refuses_what_breaks_a_clause():
    ok_w, ok_ac = np.full(64, 0.5, F32), np.full(64, 1.25, F32)
    assert tc.exact_ok(np.concatenate([ok_w, ok_ac]))
    for bad, why in ((1e-30, "one tiny addend: the sum passes 2^52 q"), (2.0 ** -101, "below 2^-100"), (1e-40, "a subnormal"),
                     (np.nan, "NaN"), (np.inf, "inf"), (-np.inf, "-inf"), (3e8, "the sum passes 2^52 q = 2^28")):
        ac = ok_ac.copy()
        ac[40] = F32(bad)
        assert not tc.exact_ok(np.concatenate([ok_w, ac])), why
    assert not tc.exact_ok(np.full(10, 1e-35, F32)), "all tiny: only the 2^-100 clause refuses"
    assert tc.exact_ok(np.full(10, 2.0 ** -100, F32))
    # the bound itself: q = 2^-24 for an addend of exponent -1; 2^52 q = 2^28
    assert tc.exact_ok(np.array([0.5, 2.0 ** 27], F32)) and not tc.exact_ok(np.array([0.5, 2.0 ** 28], F32))


def test_sticky_fallback_counts():
    w = np.full(200, 0.25, F32)
    ac = np.full(200, 1.0, F32)
    assert tc.batch_plan(w, ac) == (4, 0)
    ac[70] = F32(1e-30)                                    # in the second batch: scanned before it, serial from it on
    assert tc.batch_plan(w, ac) == (1, 3)
    ac[70] = F32(np.nan)
    assert tc.batch_plan(w, ac) == (1, 3)
    assert tc.batch_plan(w, np.full(200, 1e7, F32)) == (0, 4)
    assert tc.batch_plan(w[:0], ac[:0]) == (0, 0)


def test_scan_and_chain_really_differ_outside_the_rule():
    """1e16 then ones: the chain loses every 1 (half an ulp, ties to even), the scan adds them in pairs first"""
    w, ac = np.zeros(8, F32), np.ones(8, F32)
    w[0] = F32(1e16)
    assert not tc.exact_ok(np.concatenate([w, ac]))
    want, got = tc.serial_chain(w, ac), tc.scanned_chain(w, ac)
    assert not np.array_equal(_bits(want), _bits(got)), (want, got)


def test_option_and_getter_are_declared_everywhere():
    import kaldi_hmm_gmm_amd as khg
    from kaldi_hmm_gmm_amd import _lib
    with open(os.path.join(ROOT, "include", "khg_hip.h")) as fh:
        h = fh.read()
    opt = int(re.search(r"#define KHG_OPT_K2_TAIL (\d+)", h).group(1))
    assert opt < int(re.search(r"#define KHG_OPT_COUNT (\d+)", h).group(1)) and "KHG_K2_TAIL=on|off" in h
    assert "int khg_utts_k2_tail(" in h and hasattr(_lib.lib, "khg_utts_k2_tail") and hasattr(khg.UtteranceSet, "k2_tail")
    with open(os.path.join(ROOT, "kaldi_hmm_gmm_amd", "csrc", "khg_pybind.cpp")) as fh:
        names = re.findall(r'"(\w+)"', re.search(r"names\[KHG_OPT_COUNT\] = \{(.*?)\};", fh.read(), re.S).group(1))
    assert names[opt] == "k2_tail"
    o, v = C.c_int(-1), C.c_int(-1)
    for text, want in (("on", 0), ("off", 1), ("0", 0), ("1", 1)):
        assert _lib.lib.khg_option_from_env(b"KHG_K2_TAIL", text.encode(), C.byref(o), C.byref(v)) == 0
        assert (o.value, v.value) == (opt, want)
    assert _lib.lib.khg_option_from_env(b"KHG_K2_TAIL", b"maybe", C.byref(o), C.byref(v)) == KHG_E_ARG
    assert _lib.lib.khg_option_check(opt, 1) == 0 and _lib.lib.khg_option_check(opt, 2) == KHG_E_ARG
    out = (C.c_int32 * 2)(7, 7)
    assert _lib.lib.khg_utts_k2_tail(None, out, 2) == KHG_E_ARG and b"khg_utts_k2_tail" in _lib.lib.khg_last_error()
    assert list(out) == [7, 7]


@pytest.mark.parametrize("table", tc.TABLES)
def test_gpu_batches_are_what_they_are_taken_for(table):
    """the ladder fact of the chain batches and of their renumbered copies; which branch of the replay each score table reaches"""
    import k2_ladder_cases as lc
    c, p = tc.case(table), tc.case(table, True)
    assert len(c.graphs) <= 66 and all(lc.is_ladder(g) for g in c.graphs) and not all(lc.is_ladder(g) for g in p.graphs)
    assert all(r.ok for r in c.ref) and all(r.ok for r in p.ref)
    plans = [tc.expected_batches(c, u) for u in range(len(c.T))]
    assert plans == [tc.expected_batches(p, u) for u in range(len(p.T))], "renumbering the states changes no addend"
    assert all(a + b == -(-t // 64) for (a, b), t in zip(plans, c.T))
    if table in ("grid", "positive", "random", "zeros", "ties"):
        assert all(b == 0 for _, b in plans), table
    elif table in ("huge", "alltiny"):
        assert all(a == 0 for a, _ in plans), table
    else:                                                  # tiny: the frame in the middle decides
        assert all((a, b) == ((t // 2) // 64, -(-t // 64) - (t // 2) // 64) for (a, b), t in zip(plans, c.T)), plans
        assert any(a > 0 and b > 0 for a, b in plans)
    tie = [r.path_tie or r.final_tie for r in c.ref]
    if table == "ties":                                    # (a chain crossed in S - 1 frames, or two states without a loop on the first, leave one path)
        assert sum(tie) >= 5
    if table == "grid":
        assert sorted({(len(g["final"]), t) for g, t in zip(c.graphs, c.T)} - {(129, 133), (256, 260)}) == sorted((s, t) for s in tc.S_EDGES for t in tc.T_EDGES)
        assert max(int(r.states.max()) for r in c.ref) == 255, "a path through the fourth state slot of the trace-back"


def test_other_kinds():
    d3, wide = tc.case("random", False, "deg3"), tc.case("random", False, "wide")
    import k2_dp_ref as ref
    assert max(ref.graph_facts(g, tc.kc.ID2PDF)["indeg"] for g in d3.graphs) == 3 and max(len(g["final"]) for g in d3.graphs) <= 256
    assert max(len(g["final"]) for g in wide.graphs) > 256
    assert all(r.ok for r in d3.ref) and all(r.ok for r in wide.ref)
