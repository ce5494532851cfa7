"""MPE / sMBR posteriors of raw lattices without a GPU: the host Lattice.forward_backward_mpe against the
plain-Python restatement (tests/lattice_mpe_ref.py) -- statuses, list structure and exact zeros equal, values within the derived
tolerance -- for both criteria, both one_silence_class settings and five scale pairs on the 120 lattice-faster rule lattices and the
constructed lattices of tests/lattice_mpe_cases.py; the restatement itself against 60-digit decimal arithmetic and against the
brute-force sum over paths; that the bound discriminates; properties of the result; what is refused; the C-ABI names."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lattice_mpe_cases as mc  # noqa: E402
import lattice_mpe_ref as mr  # noqa: E402
import lattice_ops_ref as ops  # noqa: E402
import lattice_post_cases as pc  # noqa: E402
import lattice_post_ref as pr  # noqa: E402
from test_lattice_ops_cpu import _lattice  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = [(c, o, p) for c, o in mc.VARIANTS for p in mc.SCALES]


def _host(lat, ref, criterion="smbr", one_sil=True, gs=1.0, as_=1.0):
    tid2phone, tid2pdf, ali = ref
    r = _lattice(lat).forward_backward_mpe(tid2phone.tolist(), list(mc.SILENCE), np.asarray(ali).tolist(), criterion, tid2pdf.tolist(), one_sil, gs, as_)
    return {"status": r["status"], "tot": r["tot_like"], "avg": r["avg_acc"], "arc_post": np.asarray(r["arc_post"]), "post": r["post"],
            "A": np.asarray(r["acc_fwd"]), "B": np.asarray(r["acc_bwd"]), "alpha": np.asarray(r["alpha"]), "beta": np.asarray(r["beta"])}


def _properties(res, want, lat, tag):
    """every frame's signed weights sum to 0; B[start] = avg (sum_final is avg itself)"""
    tol_acc, tol_avg, tol_d = mr.tolerances(want, lat)
    worst = 0.0
    for t, (row, mcnt) in enumerate(zip(res["post"], want["merged"])):
        assert row, (tag, t)
        worst = max(worst, abs(sum(w for _, w in row)) / (sum(mcnt) * tol_d))
    worst = max(worst, abs(res["B"][int(lat["start"])] - res["avg"]) / (tol_acc + tol_avg))
    assert worst <= 1.0, (tag, worst)
    return worst


def _likelihood_part_equal(got, lat, gs, as_, tag):
    """statuses, structure and tot_like are forward_backward's, on the bits"""
    fb = _lattice(lat).forward_backward(gs, as_)
    assert got["status"] == fb["status"], tag
    assert got["tot"] == fb["tot_like"], tag
    assert [[t for t, _ in row] for row in got["post"]] == [[t for t, _ in row] for row in fb["post"]], tag
    assert ((got["arc_post"] == 0.0) | (np.asarray(fb["arc_post"]) != 0.0)).all(), tag       # a dead arc of forward_backward's is dead here


def _group(cases, criterion, one_sil, pair, what):
    gs, as_ = pair
    worst = props = 0.0
    significant = 0
    for name, lat, ref in cases:
        w = mc.want(lat, ref, criterion, one_sil, gs, as_)
        assert w["status"] == mr.SUCCEEDED, name
        got = _host(lat, ref, criterion, one_sil, gs, as_)
        tag = (name, criterion, one_sil, pair)
        worst = max(worst, mr.compare(got, w, lat, tag))
        props = max(props, _properties(got, w, lat, tag), _properties(w, w, lat, ("restatement",) + tag))
        _likelihood_part_equal(got, lat, gs, as_, tag)
        significant += mr.count_significant(w, lat) > 0
    print("%s %s one_silence_class=%s %s: host / restatement worst error / bound %.3g; properties %.3g; %d of %d lattices with an entry over 100 x its bound"
          % (what, criterion, one_sil, pair, worst, props, significant, len(cases)))
    assert 2 * significant >= len(cases), (significant, len(cases))


def test_the_calls_and_the_names_exist():
    with open(os.path.join(ROOT, "include", "khg_hip.h")) as fh:
        text = fh.read()
    from kaldi_hmm_gmm_amd import _lib
    so = os.path.join(ROOT, "kaldi_hmm_gmm_amd", "libkhg_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    for name in ("khg_lattices_mpe_posteriors",):
        assert re.search(r"\bint %s\(" % name, text), name
        assert name in _lib.SIGNATURES and getattr(_lib.lib, name) is not None, name
        assert re.search(r" T %s$" % name, out, re.M), name
    assert re.search(r"#define KHG_MPE_MPFE 0\b", text) and re.search(r"#define KHG_MPE_SMBR 1\b", text)
    import kaldi_hmm_gmm_amd as khg
    assert hasattr(khg.DeviceLattices, "mpe_posteriors") and hasattr(khg.Lattice, "forward_backward_mpe") and hasattr(khg.DevicePosteriors, "avg_acc")
    assert hasattr(khg.TransitionModel, "transition_id_to_pdf_array")


@pytest.mark.parametrize("criterion,one_sil,pair", GROUPS)
def test_lattice_faster_rule_lattices(criterion, one_sil, pair):
    cases = mc.faster_rule()
    assert len(cases) == 120
    _group(cases, criterion, one_sil, pair, "rule lattices")


@pytest.mark.parametrize("criterion,one_sil,pair", GROUPS)
def test_constructed_lattices(criterion, one_sil, pair):
    _group(mc.constructed(), criterion, one_sil, pair, "constructed")


def test_restatement_against_60_digits():
    """the yardstick's own error: the float64 left fold against the decimal evaluation, inside the same bound"""
    todo = [c for c in mc.constructed() if len(c[1]["ilabel"]) <= 700] + mc.faster_rule()[:12]
    worst = 0.0
    for name, lat, ref in todo:
        for (criterion, one_sil), (gs, as_) in zip(mc.VARIANTS, mc.SCALES[1:3] * 2):
            w = mc.want(lat, ref, criterion, one_sil, gs, as_)
            d = mr.forward_backward_mpe_decimal(lat, ref[0], ref[1], mc.SILENCE, ref[2], criterion, one_sil, gs, as_)
            worst = max(worst, mr.compare(w, d, lat, (name, criterion, one_sil, gs, as_)))
    print("restatement / 60 digits: worst error / bound %.3g over %d lattices" % (worst, len(todo)))
    assert worst < 0.1


def test_hand_built_against_all_paths():
    cases = [c for c in mc.constructed() if c[0] in pc.hand_built()]
    assert len(cases) == len(pc.hand_built())
    for name, lat, ref in cases:
        for criterion, one_sil in mc.VARIANTS:
            for gs, as_ in mc.SCALES:
                avg, d, n = mr.enumerate_paths(lat, ref[0], ref[1], mc.SILENCE, ref[2], criterion, one_sil, gs, as_)
                assert 2 <= n <= 500, (name, n)
                w = mc.want(lat, ref, criterion, one_sil, gs, as_)
                _, tol_avg, tol_d = mr.tolerances(w, lat)
                for res in (w, _host(lat, ref, criterion, one_sil, gs, as_)):
                    assert res["status"] == mr.SUCCEEDED
                    assert abs(res["avg"] - avg) <= tol_avg and np.abs(res["arc_post"] - d).max() <= tol_d, (name, criterion, one_sil, gs, as_)


def test_the_bound_discriminates():
    """by the restatement alone: one changed frame of the reference (to an id whose phone and pdf no arc has) moves avg by more than
    100 x the bound on that lattice.  Every lattice and variant with a correct arc; the frame is the one where the correct arcs weigh
    most (with one_silence_class on, a silence arc there may stay correct against the new id's phone: the new id is no silence id)."""
    n = 0
    for name, lat, ref in mc.constructed() + mc.faster_rule()[:20]:
        ali = ref[2]
        if name == "tile_N5003":        # 5003 states in one chain over 1001 frames: the bound on avg_acc there is 0.66 frames, and says so (7k)
            assert mr.tolerances(mc.want(lat, ref, "smbr", True, 1.0, 1.0), lat)[1] > 0.1
            continue
        nt = mc.num_tids_of(lat)
        tid2phone, tid2pdf = mc.tables(nt + 6)
        for criterion, one_sil in mc.VARIANTS:
            a = mr.forward_backward_mpe(lat, tid2phone, tid2pdf, mc.SILENCE, ali, criterion, one_sil, 1.0, 1.0)
            # the frame whose correct arcs carry the most posterior
            mass = np.bincount(lat["frame"][_src(lat)], weights=a["g"] * np.asarray(a["acc"]), minlength=len(ali) + 1)[: len(ali)]
            if not mass.any():
                continue
            changed = ali.copy()
            changed[int(np.argmax(mass))] = nt + 6
            b = mr.forward_backward_mpe(lat, tid2phone, tid2pdf, mc.SILENCE, changed, criterion, one_sil, 1.0, 1.0)
            tol_avg = mr.tolerances(a, lat)[1]
            assert abs(a["avg"] - b["avg"]) > 100 * tol_avg, (name, criterion, one_sil, a["avg"], b["avg"], tol_avg)
            n += 1
    print("(lattice, variant) pairs whose avg_acc moves by more than 100 x the bound when one reference frame changes: %d" % n)
    assert n >= 150, n


def _src(lat):
    ab = lat["arc_begin"]
    return np.repeat(np.arange(len(lat["frame"])), np.diff(ab))


def test_one_path():
    """one path: every weight is exactly 0.0 and avg_acc exactly the number of matching frames"""
    lat, ref = mc.one_path_reference()
    arcs = pr._arcs(lat)
    for criterion, one_sil in mc.VARIANTS:
        count = sum(mr.arc_acc(lat, arcs, ref[0], ref[1], mc.SILENCE, ref[2], criterion, one_sil))
        for gs, as_ in mc.SCALES:
            for res in (_host(lat, ref, criterion, one_sil, gs, as_), mc.want(lat, ref, criterion, one_sil, gs, as_)):
                assert res["status"] == mr.SUCCEEDED
                assert res["avg"] == float(count), (criterion, one_sil, res["avg"], count)
                assert (np.asarray(res["arc_post"]) == 0.0).all()
                assert all(len(row) == 1 and row[0][1] == 0.0 for row in res["post"])
    counts = {v: sum(mr.arc_acc(lat, arcs, ref[0], ref[1], mc.SILENCE, ref[2], *v)) for v in mc.VARIANTS}
    assert counts[("smbr", True)] == 5 and counts[("smbr", False)] == 3 and counts[("mpfe", False)] == 3, counts      # ids 1, 2 are silence ids


def test_dead_arcs_give_exact_zeros_and_no_entries():
    lat, dead = pc.dead_states()
    ref = [c for c in mc.constructed() if c[0] == "dead_states"][0][2]
    for criterion, one_sil in mc.VARIANTS:
        w = mc.want(lat, ref, criterion, one_sil, 1.0, 1.0)
        assert [a for a, x in enumerate(w["live"]) if not x] == dead
        got = _host(lat, ref, criterion, one_sil)
        mr.compare(got, w, lat, "dead")
        assert (got["arc_post"][dead] == 0.0).all() and not np.signbit(got["arc_post"][dead]).any()
        assert [[t for t, _ in row] for row in got["post"]] == [[1], [2]]
        assert got["A"][2] == 0.0 and got["B"][3] == 0.0 and got["B"][5] == 0.0


def test_no_ref():
    """no alignment, one of another length, an id outside 1 .. num_tids: KHG_LAT_NO_REF, nothing else"""
    name, lat, (tid2phone, tid2pdf, ali) = mc.constructed()[-2]
    T = len(ali)
    assert T >= 2
    bad_id = ali.copy()
    bad_id[T // 2] = len(tid2phone)
    zero_id = ali.copy()
    zero_id[0] = 0
    for a in (np.zeros(0, np.int32), ali[:-1], np.concatenate([ali, ali[:1]]), bad_id, zero_id):
        for res in (_host(lat, (tid2phone, tid2pdf, a)), mr.forward_backward_mpe(lat, tid2phone, tid2pdf, mc.SILENCE, a)):
            assert res["status"] == mr.NO_REF and res["tot"] == -np.inf and res["avg"] == 0.0
            assert len(res["post"]) == 0 and len(res["arc_post"]) == 0
    assert _host(lat, (tid2phone, tid2pdf, ali))["status"] == mr.SUCCEEDED
    # an empty lattice is NO_PATH whatever the reference; a refused structure keeps its status when the reference is usable
    e = _host(ops.empty_lattice(), (tid2phone, tid2pdf, np.zeros(0, np.int32)))
    assert e["status"] == mr.NO_PATH and e["avg"] == 0.0
    tp, td = mc.tables(4)
    for lat2, st in ((pc.eps_self_loop(), mr.EPS_LOOP), (pc.eps_to_lower_state(), mr.EPS_LOOP), (pc.no_reachable_final(), mr.NO_PATH)):
        a = np.ones(int(lat2["frame"][-1]), np.int32)
        for res in (_host(lat2, (tp, td, a)), mr.forward_backward_mpe(lat2, tp, td, mc.SILENCE, a)):
            assert res["status"] == st and res["tot"] == -np.inf and res["avg"] == 0.0 and len(res["post"]) == 0


def test_refusals():
    lat, (tid2phone, tid2pdf, ali) = mc.one_path_reference()
    L = _lattice(lat)
    args = (tid2phone.tolist(), [1], ali.tolist())
    assert L.forward_backward_mpe(*args, "smbr", tid2pdf.tolist())["status"] == mr.SUCCEEDED
    for gs, as_ in ((-1.0, 1.0), (1.0, -0.5), (float("nan"), 1.0), (1.0, float("nan")), (float("inf"), 1.0), (1.0, float("inf"))):
        with pytest.raises(Exception):
            L.forward_backward_mpe(*args, "smbr", tid2pdf.tolist(), True, gs, as_)
    with pytest.raises(Exception):
        L.forward_backward_mpe(*args, "mmi", tid2pdf.tolist())                              # an unknown criterion
    with pytest.raises(Exception):
        L.forward_backward_mpe(*args, "smbr")                                               # sMBR without tid2pdf
    assert L.forward_backward_mpe(*args, "mpfe")["status"] == mr.SUCCEEDED                  # MPFE does without
    with pytest.raises(Exception):
        L.forward_backward_mpe(tid2phone.tolist(), [99], ali.tolist(), "mpfe")              # a silence phone of no id
    with pytest.raises(Exception):
        L.forward_backward_mpe(tid2phone[:4].tolist(), [1], ali.tolist(), "mpfe")           # an arc's ilabel above num_tids
    with pytest.raises(Exception):
        L.forward_backward_mpe([], [], ali.tolist(), "mpfe")
