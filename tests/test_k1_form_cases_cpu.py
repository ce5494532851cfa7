"""The inputs of tests/test_gpu_k1_forms.py without a device (tests/k1_form_cases.py): the record every case states is the one the
restated selection and planning rules give for its shapes and arrays; the oracle's fp32 chain agrees with the float64 yardstick on
every case at the tolerance the GPU test uses; the cases' records name every kernel instantiation K1 can launch; the chain graphs
have the first and last needed frames their comments claim; khg_utts_k1_last is declared, exported, bound and refuses null
arguments."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import k1_form_cases as kc
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KHG_E_ARG = -1
IDS = [c.name for c in kc.CASES]


def test_entry_point_is_declared_exported_and_bound():
    from kaldi_hmm_gmm_amd import _lib
    import kaldi_hmm_gmm_amd as khg
    with open(os.path.join(ROOT, "include", "khg_hip.h")) as fh:
        header = fh.read()
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "kaldi_hmm_gmm_amd", "libkhg_hip.so")], capture_output=True, text=True,
                         check=True).stdout
    name = "khg_utts_k1_last"
    assert re.search(r"\bint %s\(" % name, header) and name in _lib.SIGNATURES and re.search(r" T %s$" % name, out, re.M)
    assert hasattr(khg.UtteranceSet, "k1_last")
    words = int(re.search(r"#define KHG_K1_LAST_WORDS (\d+)", header).group(1))
    assert words == 27
    for v, macro in enumerate(("NONE", "F16X2S", "F16X2", "PDF", "UTT", "WIDE")):
        assert re.search(r"#define KHG_K1L_%s %d\b" % (macro, v), header), macro


def test_getter_refuses_bad_arguments():
    from kaldi_hmm_gmm_amd import _lib
    lib = _lib.lib
    out = (C.c_int32 * 27)(*([-1] * 27))
    assert lib.khg_utts_k1_last(None, out) == KHG_E_ARG and b"khg_utts_k1_last" in lib.khg_last_error()
    assert all(v == -1 for v in out), "the buffer is left alone"
    assert lib.khg_utts_k1_last(None, None) == KHG_E_ARG


@pytest.mark.parametrize("name", IDS)
def test_stated_record_is_the_restated_rule(name):
    b = kc.build(name)
    want = kc.restate(b)
    assert b.case.expect == want, {k: (b.case.expect[k], want[k]) for k in want if b.case.expect[k] != want[k]}
    assert set(b.case.expect) == set(kc.ZERO)


@pytest.mark.parametrize("name", IDS)
def test_oracle_fp32_chain_is_inside_the_tolerance(name):
    b = kc.build(name)
    c = b.case
    om = orc.OModel(b.m.gauss_off, b.gc, b.m.means_invvars, b.m.inv_vars)
    worst = 0.0
    for u in range(len(b.lists)):
        x = b.feats[b.frame_off[u]: b.frame_off[u + 1]]
        if not len(b.lists[u]) or not len(x):
            continue
        got = orc.loglikes_matrix(om, x, b.lists[u])
        tol = kc.tolerance(b.bound[u], c.D)
        err = np.abs(got - b.exact[u])
        worst = max(worst, float((err / tol).max()))
        assert np.isfinite(b.exact[u]).all() and (err <= tol).all(), f"utt {u}: max err/tol {(err / tol).max()}"
        if c.bitwise:
            assert all(g == 1 for g in c.gauss)
    print(name, "oracle worst err/tol", worst)


def test_cases_launch_every_instantiation():
    got = set()
    for c in kc.CASES:
        got |= kc.instantiations(c.expect)
    assert got == kc.ALL_INSTANTIATIONS, {"no case": sorted(kc.ALL_INSTANTIATIONS - got), "unknown": sorted(got - kc.ALL_INSTANTIATIONS)}
    print("\n".join(sorted(got)))


def test_cases_reach_the_edges_they_claim():
    forms = {c.expect["form"] for c in kc.CASES}
    assert forms == {"none", "f16x2s", "f16x2", "pdf", "utt", "wide"}
    assert {c.expect["declined"] for c in kc.CASES} >= {0, 1, 2, 8, 9}
    assert {c.expect["pack"] for c in kc.CASES if c.expect["form"] == "f16x2s"} == {1, 2, 4}
    assert {c.expect["order"] for c in kc.CASES if c.expect["form"] == "f16x2s"} == {0, 1, 2, 3, 4}
    assert {(c.expect["pack"], c.expect["mode"]) for c in kc.CASES if c.expect["form"] == "f16x2s"} >= {(1, 0), (1, 1), (1, 2), (4, 0), (4, 1), (2, 0), (2, 1)}
    # order 4 with empty work items: more items than plan_x32_chunks cut chunks
    b = kc.build("s41_17")
    lens, nlist = [int(t) for t in np.diff(b.frame_off)], [len(x) for x in b.lists]
    ch = kc.x32_chunks(lens, nlist, 7, 4)
    assert len(ch) == 33 and sum(1 for c in ch if c[2] == 0) == 6 and sorted(c for c in ch if c[2]) == sorted(kc.x32_chunks(lens, nlist, 7, 1))
    # the pdf-major slices: an entry split over slices (TS = 3), a slice of K1P_MAXENT entries, entries without tiles inside and at the end
    sl = kc.pdf_slices(kc.build("p40_ts3"), False, 3)
    assert any(s[3] > 0 for s in sl) and all(s[4] <= 3 for s in sl)
    assert max(s[2] for s in kc.pdf_slices(kc.build("p40_300"), False, 1024)) == kc.K1P_MAXENT
    g4 = kc.build("p40_g4_reach")
    assert [min(7 if u % 2 == 0 else 5, g4.first[u][10] // 16) for u in range(4)] == [0, 5, 0, 5], "pdf 10: tiles, none, tiles, none"
    assert max(s[4] for s in kc.pdf_slices(kc.build("p39_4200"), False, 1024)) == 263


def test_chain_graphs_have_the_frames_they_claim():
    b = kc.build("s40_g4_band")
    fa, la = b.first[1], b.last[1]
    assert [fa[p] for p in range(8)] == [0, 1, 15, 16, 17, 31, 32, 33] and [la[p] - fa[p] for p in range(8)] == [31] * 8
    assert la[9] == -1 and fa[9] == 3 and fa[10] == 100 and la[10] == 69 and int(np.diff(b.frame_off)[1]) == 70
    shifts = [kc.shift_of(fa[p], la[p], 70, "band", 2) for p in range(8)]
    assert shifts == [0, 1, 15, 16, 17, 31, 0, 1]
    assert [kc.shift_of(fa[p], la[p], 70, "band", 1) for p in range(8)] == [0, 0, 0, 16, 0, 0, 0, 0]       # [16, 47]: the one band that ends in a tile's first half
    assert [kc.shift_of(fa[p], la[p], 70, "reach", 2) for p in range(8)] == [0, 0, 15, 16, 17, 31, 0, 0]   # (the tail ends at frame 69 = 2 x 32 + 5)
    assert b.first[0][10] == 5 and int(np.diff(b.frame_off)[0]) == 100
    lg = kc.build("s40_long_reach")
    assert [lg.first[0][p] for p in (0, 1, 2, 3)] == [0, 2050, 8161, 8195] and int(lg.frame_off[-1]) == 8200
    assert 2050 // 16 > 127 and 8161 // 32 == 255 and 8195 // 32 > 255, "past both clamps"
    ge = kc.build("s40_ge_band")
    assert [len(x) for x in ge.lists] == [11, 0, 1, 11] and np.diff(ge.frame_off).tolist() == [70, 40, 0, 100]


def test_domain_restatements_on_the_rescaled_models():
    """tests/test_gpu_parity.py's recipes: dimension 5 of the model in units 1e-3 smaller takes f16x2s over its error floor (f16x2
    fits); 1e-6 takes both split forms out of their domain"""
    for name, want in (("h40", (True, True, True)), ("h40_auto", (True, False, True)), ("p40_auto", (False, None, None))):
        b = kc.build(name)
        xk, wk, gcmax = kc.column_maxima(b.m, b.gc, b.feats, 80)
        dom = kc.split_domain(xk, wk, gcmax)
        got = (dom, kc.f16x2s_scales(xk, wk) if dom else None, kc.k1h_fits(xk, wk) if dom else None)
        assert got == want, (name, got)
