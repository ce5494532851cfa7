"""The inputs of tests/test_gpu_k3_forms.py without a device (tests/k3_form_cases.py): the float64 restatement agrees with the oracle's
fp32 chain on every case at the tolerances the GPU test uses; every case has the bucket sizes, Gaussian counts, diffuseness and fp16
domain it claims; the rows the cases expect are the library's table (khg_k3_forms) exactly; the two entry points are declared,
exported, bound and refuse null arguments."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import k3_form_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KHG_E_ARG = -1
IDS = [c.name for c in kc.CASES]


def _row(r):
    return (r["variant"], r["KQ"], r["NB"], r["waves"], r["POST"], r["f16a"])


def test_entry_points_are_declared_exported_and_bound():
    from kaldi_hmm_gmm_amd import _lib
    import kaldi_hmm_gmm_amd as khg
    with open(os.path.join(ROOT, "include", "khg_hip.h")) as fh:
        header = fh.read()
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "kaldi_hmm_gmm_amd", "libkhg_hip.so")], capture_output=True, text=True,
                         check=True).stdout
    for name in ("khg_k3_forms", "khg_utts_k3_last"):
        assert re.search(r"\bint %s\(" % name, header) and name in _lib.SIGNATURES and re.search(r" T %s$" % name, out, re.M), name
    assert callable(khg.k3_forms) and hasattr(khg.UtteranceSet, "k3_last")
    names = ["wave", "wave16", "wave16_records", "finalize", "mfma", "block16", "valu"]
    for v, (macro, name) in enumerate(zip(("WAVE", "WAVE16", "WAVE16P", "FINALIZE", "MFMA", "BLOCK16", "VALU"), names)):
        assert re.search(r"#define KHG_K3V_%s %d\b" % (macro, v), header), macro
    assert {r["variant"] for r in khg.k3_forms()} == set(names)


def test_getters_refuse_bad_arguments():
    from kaldi_hmm_gmm_amd import _lib
    lib = _lib.lib
    n = C.c_int32(-7)
    assert lib.khg_k3_forms(None, 0, None) == KHG_E_ARG and b"khg_k3_forms" in lib.khg_last_error()
    assert lib.khg_k3_forms(None, 0, C.byref(n)) == 0 and n.value > 0          # rows == NULL: n alone
    total = n.value
    rows = (C.c_int32 * (6 * total))(*([-1] * (6 * total)))
    assert lib.khg_k3_forms(rows, total - 1, C.byref(n)) == KHG_E_ARG and all(v == -1 for v in rows), "too small a buffer is left alone"
    assert lib.khg_k3_forms(rows, total, C.byref(n)) == 0 and n.value == total and all(v >= 0 for v in rows)
    out, nr = (C.c_int32 * 24)(*([-1] * 24)), C.c_int32(-7)
    assert lib.khg_utts_k3_last(None, out, C.byref(nr)) == KHG_E_ARG and b"khg_utts_k3_last" in lib.khg_last_error()
    assert nr.value == -7 and all(v == -1 for v in out)
    assert lib.khg_utts_k3_last(None, None, None) == KHG_E_ARG


def test_table_through_ctypes_is_the_bound_one():
    import kaldi_hmm_gmm_amd as khg
    from kaldi_hmm_gmm_amd import _lib
    n = C.c_int32(0)
    assert _lib.lib.khg_k3_forms(None, 0, C.byref(n)) == 0
    rows = (C.c_int32 * (6 * n.value))()
    assert _lib.lib.khg_k3_forms(rows, n.value, C.byref(n)) == 0
    names = ["wave", "wave16", "wave16_records", "finalize", "mfma", "block16", "valu"]
    raw = [(names[rows[6 * i]], rows[6 * i + 1], rows[6 * i + 2], rows[6 * i + 3], bool(rows[6 * i + 4]), bool(rows[6 * i + 5])) for i in range(n.value)]
    assert raw == [_row(r) for r in khg.k3_forms()] and len(set(raw)) == len(raw) == 37


def test_cases_cover_the_table_exactly():
    """a table row without a case, or a case naming a row that is not there; and no case is spare: without any one of them the rows it
    alone reaches -- or, for a second case of a row, the dimension, weight, option or fallback it alone brings -- are gone"""
    import kaldi_hmm_gmm_amd as khg
    table = {_row(r) for r in khg.k3_forms()}
    want = kc.expected_rows()
    assert want == table, {"no case": sorted(table - want), "no such row": sorted(want - table)}
    # what a case brings besides its rows: its dimension per row, and its route (options, weight, posteriors' source, fallback)
    def brings(c):
        return {(r[:6], c.D) for r in c.expect} | {(r[:6], c.opts, c.weight, c.post, c.tweak, len(c.expect)) for r in c.expect}
    for c in kc.CASES:
        others = set().union(*(brings(o) for o in kc.CASES if o is not c))
        assert brings(c) - others, c.name
    assert len(kc.CASES) == 67, "a case was added or taken out: say here what it brought"


def test_dimensions_weights_and_routes_the_cases_claim():
    rows_at = {}
    for c in kc.CASES:
        for r in c.expect:
            rows_at.setdefault(r[:6], set()).add(c.D)
    top = {10: 40, 20: 80, 0: 81}
    for row, dims in rows_at.items():
        assert top[row[1]] in dims, ("every row at the top of its KQ", row, dims)
    by_variant = {}
    for c in kc.CASES:
        for r in c.expect:
            by_variant.setdefault((r[0], r[1]), set()).add(c.D)
    for v in ("wave", "wave16", "wave16_records", "mfma", "block16", "valu"):
        assert 1 in by_variant[(v, 10)] and 39 in by_variant[(v, 10)], v
    for v in ("mfma", "block16", "valu"):
        assert 41 in by_variant[(v, 20)] and 79 in by_variant[(v, 20)], v
    assert {81, 83} <= by_variant[("valu", 0)]
    # -0.5 once per variant with an fp16 phase B; the weight that is no ordinary number towards both fallbacks; the option routes
    for v in ("wave16", "wave16_records", "block16"):
        assert any(c.weight == -0.5 and c.expect[0][0] == v for c in kc.CASES), v
    tiny = {c.expect[0][:1] + (c.expect[0][5],) for c in kc.CASES if c.weight == kc.TINY}
    assert ("wave", True) in tiny and ("mfma", False) in tiny
    assert any(dict(c.opts).get("k3_ny") == 3 and c.expect[0][0] == "wave16_records" for c in kc.CASES)
    assert any(dict(c.opts).get("k3_planes") == 1 and c.expect[0][0] == "wave16" for c in kc.CASES)
    assert {c.tweak for c in kc.CASES} == {"", "narrow", "spike"}
    assert {len(c.expect) for c in kc.CASES} == {1, 2}
    assert {c.post for c in kc.CASES} == {"", "arrays", "alignment"}
    for c in kc.CASES:
        assert all(r[4] == bool(c.post) and r[1] == c.kq for r in c.expect), c.name


@pytest.mark.parametrize("name", IDS)
def test_case_is_what_it_claims(name):
    b = kc.build(name)
    c, m = b.case, b.m
    G = np.diff(m.gauss_off)
    # buckets: exactly COUNTS, scattered, the frames without an id outside
    assert sorted(b.counts) == sorted(kc.COUNTS) and len(b.frame_off) == kc.N_UTT + 1 and (np.diff(b.frame_off) > 0).all()
    assert (np.bincount(m.id2pdf[b.ali[b.ali > 0]], minlength=kc.P) == b.counts).all() and int((b.ali == 0).sum()) == kc.N_SKIP
    assert len(b.ali) == b.frame_off[-1] == len(b.feats) and b.feats.shape[1] == c.D
    for p in np.nonzero(b.counts >= 15)[0]:
        fr = np.nonzero(m.id2pdf[b.ali] * (b.ali > 0) + (b.ali > 0) - 1 == p)[0]
        assert (np.diff(fr) > 1).any(), ("the frames of a pdf are not contiguous", p)
    if c.post == "alignment":       # the frames without an id: one whole utterance (a failed one), not the first
        u = np.nonzero(b.ali[b.frame_off[:-1]] == 0)[0]
        assert len(u) == 1 and u[0] > 0 and (b.ali[b.frame_off[u[0]]: b.frame_off[u[0] + 1]] == 0).all() and b.frame_off[u[0] + 1] - b.frame_off[u[0]] == kc.N_SKIP
    else:
        assert len(np.unique(np.searchsorted(b.frame_off, np.nonzero(b.ali == 0)[0], side="right"))) >= 4, "mixed in among the others"
    # Gaussian counts: the class pinned at both ends
    if len(c.gauss) == 2:
        lo, hi = c.gauss
        assert lo in G and hi in G and G.max() == hi and ((G >= lo) | (G == 1) | (G == 17)).all()
        if hi <= 64 or c.post or c.D > 40 or "k3_form" in dict(c.opts):
            assert (lo == 1 or 1 in G) and (lo <= 17 or 17 in G), "pdfs of 1 and 17 Gaussians inside the wider instantiation"
    else:
        wide = G[G > 64]
        assert len(wide) == 1 and G[G <= 64].max() == 64 and 49 in G and 1 in G and b.counts[np.argmax(G)] == 65
    # both sides of every Gaussian-count boundary the case's expected kernel has: the widest pdf decides NB
    r0 = c.expect[-1]
    if r0[0] in kc.WAVE_VARIANTS:
        assert r0[2] == (G[G <= 64].max() + 15) // 16
    elif r0[0] == "mfma":
        assert r0[2] == max(1, (G.max() + 63) // 64)
    elif r0[0] == "block16":
        assert (r0[2], r0[3]) == ((1, 4) if G.max() <= 64 else (1, 8) if G.max() <= 128 else (3, 4))
    # diffuse posteriors; random features
    assert kc.diffuseness(b) < 0.5
    assert len(np.unique(b.feats)) > 0.99 * b.feats.size
    # the fp16 domain the expected record rests on
    model_ok, set_ok, floor = kc.fp16_domain(m, b.gc, b.feats)
    print(name, "fp16 phase A: model", model_ok, "set", set_ok, "floor", floor)
    if c.tweak == "narrow":
        assert not model_ok and floor is not None and floor > 8e-6, "the model's side fails, by a factor of two at the least"
    elif c.tweak == "spike":
        assert model_ok and not set_ok and floor < 2e-6
    elif c.kq:
        assert model_ok and set_ok and floor < 2e-6, "the domain holds, by a factor of two at the least"
    if any(r[5] for r in c.expect):
        assert model_ok and set_ok


@pytest.mark.parametrize("name", IDS)
def test_restatement_agrees_with_the_oracle(name):
    b = kc.build(name)
    kc.assert_stats(kc.oracle_stats(b), b, name)


def test_restatement_notices_what_the_gpu_test_is_for():
    """the yardstick's power on these inputs: a frame dropped at a tile's end, a padding Gaussian let into the softmax, the last
    dimension dropped -- each moves the restated statistics of a case past the tolerances"""
    b = kc.build("wave16r_4_d39")
    p = int(np.nonzero(b.counts == 17)[0][0])
    sel = np.nonzero(b.m.id2pdf[b.tids] == p)[0]
    keep = np.ones(len(b.frames), bool)
    keep[sel[-1]] = False                                            # the 17th frame of the bucket: the lane past the first tile
    dropped = kc.restate(b.m, b.gc, b.feats, b.frames[keep], b.tids[keep], b.w[keep], True)
    dropped["trans_acc"], dropped["total_frames"] = b.ref["trans_acc"], b.ref["total_frames"]
    with pytest.raises(AssertionError):
        kc.assert_stats(dropped, b)
    x = b.feats.copy()
    x[:, -1] = 0.0                                                   # dimension D - 1 at odd D
    nodim = kc.restate(b.m, b.gc, x, b.frames, b.tids, b.w, True)
    with pytest.raises(AssertionError):
        kc.assert_stats(nodim, b)
    # a padding Gaussian with log-likelihood 0 instead of -inf in the pdf of 17 Gaussians (one more term in the softmax's sum)
    q = int(np.nonzero(np.diff(b.m.gauss_off) == 17)[0][0])
    if b.counts[q]:
        a, e = int(b.m.gauss_off[q]), int(b.m.gauss_off[q + 1])
        pad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in b.ref.items()}
        xs = b.feats[b.frames[b.m.id2pdf[b.tids] == q]].astype(np.float64)
        ll = b.gc[a:e].astype(np.float64)[None, :] + xs @ b.m.means_invvars[a:e].astype(np.float64).T - 0.5 * (xs * xs) @ b.m.inv_vars[a:e].astype(np.float64).T
        g = np.exp(ll) / (np.exp(ll).sum(1, keepdims=True) + 1.0)
        pad["occ"][a:e] = 0.75 * g.sum(0)
        with pytest.raises(AssertionError):
            kc.assert_stats(pad, b)
