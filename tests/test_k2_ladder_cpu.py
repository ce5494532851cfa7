"""The ladder form of K2's exact DP without a device: its getter (khg_utts_k2_ladder) is declared, exported, bound and refuses bad
arguments; its option (KHG_OPT_K2_LADDER) is in the header, the Python names and the environment table; and the chain graphs of
tests/test_gpu_k2_ladder.py have the property the host fact looks for while their permuted copies do not."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import k2_ladder_cases as lc  # noqa: E402

KHG_E_ARG = -1


def _header():
    with open(os.path.join(ROOT, "include", "khg_hip.h")) as fh:
        return fh.read()


def test_k2_ladder_entry_point():
    name = "khg_utts_k2_ladder"
    from kaldi_hmm_gmm_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "kaldi_hmm_gmm_amd", "libkhg_hip.so")], capture_output=True, text=True,
                         check=True).stdout
    assert re.search(r"\bint %s\(" % name, _header()) and name in _lib.SIGNATURES and re.search(r" T %s$" % name, out, re.M)
    assert getattr(_lib.lib, name) is not None
    import kaldi_hmm_gmm_amd as khg
    assert hasattr(khg.UtteranceSet, "k2_ladder")


def test_k2_ladder_getter_refuses_bad_arguments():
    """no context, no set, no result: KHG_E_ARG, as khg_utts_k2_plan answers them (a set without graphs needs a device to exist:
    tests/test_gpu_k2_ladder.py::test_getter_refuses_a_set_without_graphs)"""
    from kaldi_hmm_gmm_amd import _lib
    out = C.c_int32(7)
    assert _lib.lib.khg_utts_k2_ladder(None, None, None) == KHG_E_ARG
    assert b"khg_utts_k2_ladder" in _lib.lib.khg_last_error()
    assert _lib.lib.khg_utts_k2_ladder(None, None, C.cast(C.byref(out), C.POINTER(C.c_int32))) == KHG_E_ARG and out.value == 7
    plan = (C.c_int32 * 8)()
    assert _lib.lib.khg_utts_k2_plan(None, None, plan) == KHG_E_ARG
    with open(os.path.join(ROOT, "kaldi_hmm_gmm_amd", "csrc", "khg_k2.hip")) as fh:
        src = fh.read()
    for fn in ("khg_utts_k2_plan", "khg_utts_k2_ladder"):
        assert '"%s: the utterance set has no decoding graphs"' % fn in src


def test_option_is_declared_named_and_seeded():
    h = _header()
    opt = int(re.search(r"#define KHG_OPT_K2_LADDER (\d+)", h).group(1))
    assert opt < int(re.search(r"#define KHG_OPT_COUNT (\d+)", h).group(1)) and "KHG_K2_LADDER=on|off" in h
    with open(os.path.join(ROOT, "kaldi_hmm_gmm_amd", "csrc", "khg_pybind.cpp")) as fh:
        names = re.findall(r'"(\w+)"', re.search(r"names\[KHG_OPT_COUNT\] = \{(.*?)\};", fh.read(), re.S).group(1))
    assert names[opt] == "k2_ladder"
    from kaldi_hmm_gmm_amd import _lib
    assert _lib.lib.khg_option_check(opt, 0) == 0 and _lib.lib.khg_option_check(opt, 1) == 0
    assert _lib.lib.khg_option_check(opt, 2) == KHG_E_ARG and _lib.lib.khg_option_check(opt, -1) == KHG_E_ARG
    for text, want in (("on", 0), ("off", 1), ("0", 0), ("1", 1)):
        o, v = C.c_int(-1), C.c_int(-1)
        assert _lib.lib.khg_option_from_env(b"KHG_K2_LADDER", text.encode(), C.byref(o), C.byref(v)) == 0
        assert (o.value, v.value) == (opt, want)
    o, v = C.c_int(-1), C.c_int(-1)
    assert _lib.lib.khg_option_from_env(b"KHG_K2_LADDER", b"maybe", C.byref(o), C.byref(v)) == KHG_E_ARG


def test_cases_are_what_they_are_named():
    """chain graphs are ladders, their permuted copies and the in-degree-3 graph are not; the boundary-tie case has its only tie on
    state 64's cell of the best path; the constant-score case ties everywhere"""
    for name in lc.ALL:
        c = lc.case(name)
        assert [lc.is_ladder(g) for g in c.graphs] == [c.ladder] * len(c.graphs), name
        assert len(c.graphs) == len(c.T) == len(c.mats) == len(c.ref)
    c = lc.case("sizes")
    assert sorted({len(g["final"]) for g in c.graphs}) == list(lc.SIZES)
    for S in lc.SIZES:
        ts = sorted(t for g, t in zip(c.graphs, c.T) if len(g["final"]) == S)
        assert ts == sorted({max(0, S - 2), S - 1, S, S + 6, S + 7, S + 8, S + 9, S + 33}), S
    for g, t, r in zip(c.graphs, c.T, c.ref):
        assert r.ok == (t >= len(g["final"]) - 1)
    assert sorted({len(g["final"]) for g in lc.case("mixed").graphs}) == [40, 70, 200]
    b = lc.case("boundary_tie")
    for r in b.ref:
        assert r.ok and r.path_tie and not r.final_tie
        t, s = np.nonzero(r.tie)
        assert set(s.tolist()) == {64} and t.min() == 65
    for r in lc.case("constant").ref:
        assert r.ok and r.path_tie
    assert all(np.diff(g["arc_off"]).max() <= 2 for g in lc.case("permuted").graphs)
    assert max(int(np.bincount(g["nextstate"]).max()) for g in lc.case("indeg3").graphs) == 3
