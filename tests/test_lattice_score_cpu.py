"""Scoring lattices on the host: the host forms Lattice.add_penalty, Lattice.oracle and khg_edit_distance against
the plain-Python restatement (tests/lattice_score_ref.py) on every output, and against what knows nothing of the rule: a textbook
Levenshtein distance and the brute-force enumeration of a small lattice's paths.  All integers, so no tolerance anywhere.  The device
forms are held to the host forms by tests/test_gpu_lattice_score.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lattice_score_cases as cases  # noqa: E402
import lattice_score_ref as ref  # noqa: E402

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "khg_hip.h")


def _lattice(khg, lat):
    return khg.Lattice.from_arrays(*[lat[k] for k in ref.FIELDS], int(lat["start"]))


@pytest.fixture(scope="module")
def work():
    """every case with the restatement's answer, computed once"""
    import kaldi_hmm_gmm_amd as khg
    items = [(name,) + c for name, c in sorted(cases.hand_cases().items())]
    items += [("random%d" % i, lat, r, None) for i, (lat, r) in enumerate(cases.random_cases())]
    return khg, [{"name": n, "lat": lat, "ref": r, "expect": st, "want": ref.oracle(lat, r)} for n, lat, r, st in items]


def test_host_oracle_equals_the_restatement_on_every_output(work):
    khg, items = work
    seen = {}
    for x in items:
        got = _lattice(khg, x["lat"]).oracle(x["ref"])
        want = x["want"]
        assert got["status"] == want["status"], x["name"]
        if x["expect"] is not None:
            assert got["status"] == x["expect"], x["name"]
        for k in ("counts", "words", "ali", "arcs"):
            assert got[k].dtype == np.int32 and got[k].tolist() == want[k], (x["name"], k)
        seen[got["status"]] = seen.get(got["status"], 0) + 1
    assert seen[ref.SUCCEEDED] > 200 and seen[ref.NO_PATH] >= 3 and seen[ref.EPS_LOOP] == 2, seen


def test_what_the_hand_cases_are_there_for(work):
    khg, items = work
    w = {x["name"]: x["want"] for x in items}
    lat = {x["name"]: x["lat"] for x in items}
    assert w["one_state"]["counts"] == [2, 0, 2, 0] and w["one_state_r0"]["counts"] == [0, 0, 0, 0] and w["empty"]["counts"] == [2, 0, 2, 0]
    assert w["no_word"]["counts"] == [1, 0, 1, 0] and w["no_word"]["words"] == [] and len(w["no_word"]["arcs"]) >= 2
    assert w["r0"]["counts"][0] == w["r0"]["counts"][1] == len(w["r0"]["words"]) > 0
    assert w["single_path_exact"]["counts"] == [0, 0, 0, 0] and w["single_path_sub_del"]["counts"] == [2, 0, 1, 1]
    assert w["single_path_ins"]["counts"] == [2, 2, 0, 0]
    assert w["two_paths_equal_errors"]["counts"] == [1, 0, 0, 1] and w["two_paths_equal_errors"]["words"] == [1]       # the lower arc
    assert w["tie_one_word"]["counts"] == [1, 0, 0, 1]                  # DIAG is tried before INS, and DEL only wins when strictly smaller
    assert w["tie_diag_ins_del"]["counts"][0] == 2 and w["tie_repeats"]["counts"][0] == 2
    assert w["unreachable_state"]["words"] == [1, 3] and w["start_not_first"]["words"] == [2, 3]
    assert w["last_frame_not_final"]["words"] == [2] and w["last_frame_not_final"]["counts"] == [1, 0, 0, 1]
    assert w["final_before_last_frame"]["words"] == [1, 2] and w["final_before_last_frame"]["counts"] == [1, 1, 0, 0]
    assert w["several_finals_equal_errors"]["words"] == [3]             # the lowest final state among equal errors
    assert w["epsilon_chain"]["counts"] == [0, 0, 0, 0] and w["epsilon_chain"]["words"] == [1, 2, 3, 4]
    assert w["hub_70_in_arcs"]["words"] == [35, 1] and w["hub_70_in_arcs"]["counts"] == [0, 0, 0, 0]
    assert np.bincount(lat["hub_70_in_arcs"]["nextstate"]).max() == 70
    assert w["words_the_reference_lacks"]["counts"][3] == 2 and w["words_the_reference_lacks"]["counts"][1] >= 1
    assert w["reference_longer_than_any_path"]["counts"][2] >= 6
    for W in (63, 64, 65, 130):
        x = [y for y in items if y["name"] == "segment_edge_w%d" % W][0]
        assert len(x["ref"]) + 1 == W and x["want"]["status"] == ref.SUCCEEDED and 0 < x["want"]["counts"][0] < W - 1, W
    assert len([y for y in items if y["name"] == "chain_against_long_reference_w65"][0]["ref"]) == 64
    big = lat["frame_of_200_states_w131"]
    assert np.bincount(big["frame"]).max() == 200 and 2 * 200 * 131 * 4 > 160 * 1024
    assert len([y for y in items if y["name"] == "frame_of_200_states_w131"][0]["ref"]) == 130
    # ties are common among the random cases: several paths reach the least number of errors
    tied = 0
    for x in items:
        if x["name"].startswith("random") and x["want"]["status"] == ref.SUCCEEDED:
            ps = ref.paths(x["lat"])
            if ps:
                d = sorted(ref.levenshtein(x["ref"], p[0]) for p in ps)
                tied += len(d) > 1 and d[0] == d[1]
    assert tied > 40, tied


def test_oracle_against_levenshtein_over_every_path(work):
    """On every case with at most 2000 paths: the errors are the least textbook distance over the paths, the words are a path's, and
    the counts add up."""
    khg, items = work
    n = 0
    for x in items:
        ps = ref.paths(x["lat"])
        got = _lattice(khg, x["lat"]).oracle(x["ref"])
        R = len(x["ref"])
        if ps is None:
            continue
        if not ps:
            assert got["status"] == ref.NO_PATH and got["counts"].tolist() == [R, 0, R, 0], x["name"]
            continue
        assert got["status"] == ref.SUCCEEDED, x["name"]
        err, ins, dele, sub = got["counts"].tolist()
        assert err == min(ref.levenshtein(x["ref"], p[0]) for p in ps), x["name"]
        assert (got["words"].tolist(), got["arcs"].tolist()) in [(p[0], p[1]) for p in ps], x["name"]
        assert ins + dele + sub == err and len(got["words"]) == R - dele + ins, x["name"]
        assert ref.levenshtein(x["ref"], got["words"].tolist()) == err, x["name"]
        n += 1
    assert n > 150, n          # (the other cases have more than 2000 paths)


def _pairs(n=1000, seed=99):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        v = int(rng.integers(1, 6))
        r = rng.integers(1, v + 1, size=int(rng.integers(0, 14))).tolist()
        h = cases.perturbed(rng, r, v, p=0.5) if i % 2 else rng.integers(1, v + 1, size=int(rng.integers(0, 14))).tolist()
        out.append((r, h))
    out += [([1] * 64, [1] * 63), ([1, 2] * 65, [2, 1] * 64), ([], []), ([], [3, 3]), ([3], [])]
    return out


def test_edit_distance_total_is_levenshtein_and_counts_are_the_restatements():
    import kaldi_hmm_gmm_amd as khg
    from kaldi_hmm_gmm_amd import _lib
    pairs = _pairs()
    ro, ho = np.zeros(len(pairs) + 1, np.int64), np.zeros(len(pairs) + 1, np.int64)
    for i, (r, h) in enumerate(pairs):
        ro[i + 1], ho[i + 1] = ro[i] + len(r), ho[i] + len(h)
    rf = np.asarray([w for r, _ in pairs for w in r], np.int32)
    hf = np.asarray([w for _, h in pairs for w in h], np.int32)
    counts = np.zeros((len(pairs), 4), np.int32)
    p32, p64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    assert _lib.lib.khg_edit_distance(len(pairs), rf.ctypes.data_as(p32), ro.ctypes.data_as(p64), hf.ctypes.data_as(p32), ho.ctypes.data_as(p64),
                                      counts.ctypes.data_as(p32)) == 0
    subs = 0
    for i, (r, h) in enumerate(pairs):
        err, ins, dele, sub = counts[i].tolist()
        assert err == ref.levenshtein(r, h) == ins + dele + sub and len(h) == len(r) - dele + ins, i
        assert counts[i].tolist() == ref.edit_counts(r, h), i
        assert khg.edit_distance_counts(r, h).tolist() == counts[i].tolist(), i
        subs += sub
    assert subs > 500
    wer, tot = khg.compute_wer([p[0] for p in pairs], [p[1] for p in pairs])
    assert tot == {"errors": int(counts[:, 0].sum()), "insertions": int(counts[:, 1].sum()), "deletions": int(counts[:, 2].sum()),
                   "substitutions": int(counts[:, 3].sum()), "ref_words": int(ro[-1])}
    assert wer == 100.0 * tot["errors"] / tot["ref_words"]


def test_oracle_of_a_single_path_is_the_edit_distance_of_its_words():
    import kaldi_hmm_gmm_amd as khg
    for r, h in _pairs(150, seed=5):
        got = _lattice(khg, cases.chain_lattice(h)).oracle(r)
        assert got["counts"].tolist() == khg.edit_distance_counts(r, h).tolist() and got["words"].tolist() == h


def test_add_penalty_equals_the_restatement_on_the_bits(work):
    khg, items = work
    changed = 0
    for x in items[::3]:
        for p in (0.5, -1.25, 0.0, 1e-3):
            got = _lattice(khg, x["lat"]).add_penalty(p)
            want = ref.add_penalty(x["lat"], p)
            for k in ref.FIELDS:
                g = np.asarray(getattr(got, k))
                assert g.dtype == want[k].dtype and g.tobytes() == np.ascontiguousarray(want[k]).tobytes(), (x["name"], p, k)
            assert got.start == want["start"]
            changed += int((want["graph_cost"] != x["lat"]["graph_cost"]).sum())
    assert changed > 1000
    with pytest.raises(RuntimeError, match="finite"):
        _lattice(khg, items[0]["lat"]).add_penalty(float("inf"))
    with pytest.raises(RuntimeError, match="not > 0"):
        _lattice(khg, cases.diamond()).oracle([1, 0])


def test_refusals_need_no_context_and_no_device():
    from kaldi_hmm_gmm_amd import _lib
    lib = _lib.lib
    E_ARG = -1
    assert lib.khg_lattices_add_penalty(None, None, 0.5, None) == E_ARG
    assert lib.khg_lattices_oracle(None, None, 0, None, None, 0, None, None, None, 0, None, None) == E_ARG
    assert lib.khg_lattices_wer(None, None, 0, None, None, 1, None, None, None, None, None, None) == E_ARG
    p32, p64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    off = np.array([0, 1], np.int64)
    bad = np.array([1, 0], np.int64)
    w = np.array([3], np.int32)
    out = np.zeros(4, np.int32)
    a = lambda x, t: x.ctypes.data_as(t)      # noqa: E731
    assert lib.khg_edit_distance(1, a(w, p32), a(off, p64), a(w, p32), a(off, p64), a(out, p32)) == 0 and out.tolist() == [0, 0, 0, 0]
    assert lib.khg_edit_distance(1, a(w, p32), a(bad, p64), a(w, p32), a(off, p64), a(out, p32)) == E_ARG
    assert b"start at 0" in lib.khg_last_error()
    assert lib.khg_edit_distance(1, None, a(off, p64), a(w, p32), a(off, p64), a(out, p32)) == E_ARG
    assert lib.khg_edit_distance(-1, None, None, None, None, None) == E_ARG
    assert lib.khg_edit_distance(1, a(w, p32), a(off, p64), a(w, p32), a(np.array([0, -1], np.int64), p64), a(out, p32)) == E_ARG


def test_symbols_are_declared_exported_and_bound():
    import kaldi_hmm_gmm_amd as khg
    from kaldi_hmm_gmm_amd import _lib
    header = open(HEADER).read()
    for name in ("khg_lattices_add_penalty", "khg_lattices_oracle", "khg_lattices_wer", "khg_edit_distance"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name) and ("int %s(" % name) in header, name
    for name in ("add_penalty", "oracle", "wer"):
        assert hasattr(khg.DeviceLattices, name), name
    for name in ("add_penalty", "oracle"):
        assert hasattr(khg.Lattice, name), name
    for name in ("edit_distance_counts", "lattice_add_penalty", "lattice_add_penalty_batch", "lattice_oracle", "lattice_oracle_batch", "compute_wer",
                 "score_lattices"):
        assert callable(getattr(khg, name)), name
    assert "khg_lattices_oracle" in header[header.index("KHG_OPT_LAT_OPS_LDS"):header.index("KHG_OPT_K1_LAUNCH")]
