"""Minimum Bayes risk decoding on the host: the host form Lattice.mbr against the plain-Python restatement
(tests/lattice_mbr_ref.py) -- given the restatement's weights every output is EQUAL, gamma bit for bit; the host's own weights within
the bound section 7g derived for an arc posterior -- and the restatement against what knows nothing of the rule: the brute-force
expected Levenshtein distance over a small lattice's paths.  The device form is held to the host form by tests/test_gpu_lattice_mbr.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lattice_mbr_cases as cases  # noqa: E402
import lattice_mbr_ref as ref  # noqa: E402
import lattice_post_ref as post  # noqa: E402
from lattice_score_ref import FIELDS  # noqa: E402

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "khg_hip.h")
OUTPUTS = ("status", "iters", "bayes_risk", "words", "conf", "vocab", "gamma", "risks", "cap")


def _lattice(khg, lat):
    return khg.Lattice.from_arrays(*[lat[k] for k in FIELDS], int(lat["start"]))


def _args(x):
    return x["decode_mbr"], x["max_iter"], x["init"], x["max_words"]


def _same(got, want, tag):
    """every output of the host form equal to the restatement's (floats by ==: the lists hold Python floats of the same doubles)"""
    assert got["status"] == want["status"] and got["iters"] == want["iters"] and got["cap"] == want["cap"], (tag, got["status"], want["status"])
    assert got["bayes_risk"] == want["bayes_risk"], (tag, got["bayes_risk"], want["bayes_risk"])
    assert got["words"].dtype == np.int32 and got["words"].tolist() == want["words"], tag
    assert got["vocab"].tolist() == want["vocab"] and got["conf"].tolist() == want["conf"] and got["risks"].tolist() == want["risks"], tag
    assert got["gamma"].shape == ((len(want["gamma"]), len(want["vocab"])) if want["gamma"] else (0, 0)), (tag, got["gamma"].shape)
    assert got["gamma"].tolist() == [list(g) for g in want["gamma"]], tag


@pytest.fixture(scope="module")
def work():
    """every case at every pair with the restatement's answer, computed once and left unchanged"""
    import kaldi_hmm_gmm_amd as khg
    items = []
    for gs, as_ in cases.PAIRS:
        for x in cases.hand_cases() + cases.seeded_cases():
            items.append(dict(x, gs=gs, as_=as_, want=ref.mbr(x["lat"], gs, as_, *_args(x))))
    return khg, items


def test_host_equals_the_restatement_given_its_weights(work):
    khg, items = work
    seen, iters = {}, {}
    for x in items:
        want = x["want"]
        got = _lattice(khg, x["lat"]).mbr(x["gs"], x["as_"], *_args(x), arc_cond=want["arc_cond"], final_cond=want["final_cond"])
        _same(got, want, (x["name"], x["gs"], x["as_"]))
        if x["expect"] is not None:
            assert got["status"] == x["expect"], x["name"]
        seen[got["status"]] = seen.get(got["status"], 0) + 1
        iters[got["iters"]] = iters.get(got["iters"], 0) + 1
    assert seen[ref.SUCCEEDED] > 1000 and seen[ref.NO_PATH] >= 9 and seen[ref.EPS_LOOP] == 6 and seen[ref.WORDS] == 6, seen
    assert seen[ref.SUCCEEDED | ref.NOT_CONVERGED] == 6, seen
    assert sum(n for k, n in iters.items() if k >= 2) > 100 and max(iters) >= 4, iters


def test_host_weights_agree_with_the_restatements_within_the_posterior_bound(work):
    """a weight is exp of a difference of two alphas, each within tol_log, plus an arc term: section 7g's bound for an arc posterior
    (p <= 1); exact zeros are equal; with its own weights the host refuses what the restatement refuses"""
    khg, items = work
    worst = 0.0
    for x in items:
        got = _lattice(khg, x["lat"]).mbr(x["gs"], x["as_"], *_args(x))
        st, ac, fc, fb = ref.weights(x["lat"], x["gs"], x["as_"])
        assert (got["status"] & ref.SUCCEEDED) == (x["want"]["status"] & ref.SUCCEEDED), x["name"]
        for g, w in ((got["arc_cond"], np.asarray(ac)), (got["final_cond"], np.asarray(fc))):
            assert g.shape == w.shape and ((g == 0.0) == (w == 0.0)).all(), x["name"]
            if st == ref.SUCCEEDED and len(w):
                tol = post.tolerances(fb, x["lat"])[1]
                assert np.abs(g - w).max() <= tol, (x["name"], np.abs(g - w).max(), tol)
                worst = max(worst, float(np.abs(g - w).max()) / tol)
                assert g.max() <= 1.0 + tol
    print("worst weight error / bound: %.3g" % worst)


def _admissible_from_best_path(items, gs, as_):
    return [x for x in items if (x["gs"], x["as_"]) == (gs, as_) and x["init"] is None and x["decode_mbr"] and x["max_words"] == 0
            and x["want"]["status"] == ref.SUCCEEDED]


def test_mass_is_conserved_at_every_position(work):
    """sum over words of gamma[q][.] = 1 within one rounding per addition: (states + arcs) * (Q + 1) * 2^-52"""
    _, items = work
    worst, n = 0.0, 0
    for x in items:
        want = x["want"]
        if not want["status"] & ref.SUCCEEDED:
            continue
        Q = 2 * len(want["words"]) + 1
        bound = (len(x["lat"]["frame"]) + len(x["lat"]["ilabel"])) * (Q + 1) * 2.0 ** -52
        assert len(want["gamma"]) == Q, x["name"]
        for g in want["gamma"]:
            err = abs(sum(g) - 1.0)
            assert err <= bound, (x["name"], err, bound)
            worst = max(worst, err)
        n += 1
    assert n > 1000
    print("worst |sum gamma - 1|: %.3g" % worst)


def test_bayes_risk_bounds_the_expected_levenshtein_distance(work):
    """a theorem: the recursion takes the expectation of a min as a min of expectations, so bayes_risk >= the brute-force expected
    Levenshtein distance of the hypothesis (slack 1e-9).  NOT theorems, asserted on exactly these inputs (the hand cases and
    random_cases(200, seed=2025) at (1, 0.1) from the best path): the risk never rises from one iteration to the next, and the final
    hypothesis's brute-force expected distance is not above the best path's (compared with a slack of 1e-9 as well: both sides are
    math.fsum sums over up to 3000 path probabilities that are themselves rounded)."""
    _, items = work
    n_paths, n = 0, 0
    for x in _admissible_from_best_path(items, 1.0, 0.1):
        want = x["want"]
        n += 1
        assert all(b <= a for a, b in zip(want["risks"], want["risks"][1:])), (x["name"], want["risks"])
        paths = ref.path_probs(x["lat"], 1.0, 0.1)
        if paths is None:
            continue
        n_paths += 1
        final = ref.expected_levenshtein(paths, want["words"])
        assert want["bayes_risk"] >= final - 1e-9, (x["name"], want["bayes_risk"], final)
        first = ref.mbr(x["lat"], 1.0, 0.1, decode_mbr=False)
        assert first["bayes_risk"] >= ref.expected_levenshtein(paths, first["words"]) - 1e-9, x["name"]
        assert final <= ref.expected_levenshtein(paths, first["words"]) + 1e-9, x["name"]
    assert n >= 200 and n_paths >= 150, (n, n_paths)      # (the other lattices have more than 3000 paths)


def test_single_path_lattices_give_the_edit_distance_and_one_hot_bins(work):
    _, items = work
    n = 0
    for x in items:
        if not x["name"].startswith(("single_path", "chain3")) or not x["want"]["status"] & ref.SUCCEEDED:
            continue
        want, words = x["want"], [int(w) for w in x["lat"]["olabel"]]
        assert all(p == 1.0 for p in want["arc_cond"]) and want["final_cond"][-1] == 1.0, x["name"]
        for risk, h in ((want["risks"][0], x["init"]), (want["bayes_risk"], want["words"])):
            lev = ref.levenshtein(words, h)
            assert lev - 1e-12 <= risk <= lev + 1e-5 * len(words) + 1e-9, (x["name"], risk, lev)
        for g in want["gamma"]:
            assert sorted(g)[-1] == 1.0 and sum(1 for v in g if v != 0.0) == 1, (x["name"], g)
        if x["max_iter"] == 32 and x["decode_mbr"]:
            assert want["words"] == words and want["bayes_risk"] == 0.0 and want["conf"] == [1.0] * len(words), x["name"]
        n += 1
    assert n >= 3 * 9


def test_what_the_hand_cases_are_there_for(work):
    _, items = work
    w = {x["name"]: x["want"] for x in items if (x["gs"], x["as_"]) == (1.0, 0.1)}
    assert w["single_path_ins_from_1_4"]["iters"] == 2 and w["single_path_ins_from_1_4"]["words"] == [1, 2, 3, 4]
    assert w["single_path_ins_max_iter_0"]["iters"] == 0 and w["single_path_ins_max_iter_0"]["words"] == [1, 4]
    assert w["single_path_ins_max_iter_1"]["iters"] == 1 and w["single_path_ins_max_iter_1"]["status"] == ref.SUCCEEDED | ref.NOT_CONVERGED
    assert w["single_path_confidences_only"]["iters"] == 0 and w["single_path_confidences_only"]["words"] == [1, 4, 3]
    assert w["single_path_confidences_only"]["conf"] == [1.0, 0.0, 1.0]
    assert w["gamma_tie_lowest_id"]["words"] == [1] and w["gamma_tie_from_the_higher_word"]["words"] == [1]
    g = w["gamma_tie_lowest_id"]["gamma"][1]
    assert w["gamma_tie_lowest_id"]["vocab"] == [0, 1, 2] and g[1] == g[2] > 0.4
    assert w["gamma_tie_then_word"]["words"] == [4, 3]
    for W in (30, 31, 32, 63, 64):
        x = [y for y in items if y["name"] == "segment_edge_w%d" % W][0]
        assert len(x["init"]) == W and x["want"]["status"] & ref.SUCCEEDED
    assert len([y for y in items if y["name"] == "chain3_against_64_words"][0]["init"]) == 64 and w["chain3_against_64_words"]["words"] == [1, 2, 3]
    assert w["one_state"]["words"] == [] and w["one_state"]["bayes_risk"] == 0.0 and w["one_state"]["gamma"] == [[1.0]]
    assert w["one_state_init_2_words"]["words"] == [] and w["one_state_init_2_words"]["iters"] == 1 and w["one_state_init_2_words"]["risks"][0] == 2.0
    assert w["no_word"]["words"] == [] and w["no_word"]["vocab"] == [0] and w["no_word_init_1"]["words"] == []
    assert w["empty_init"]["iters"] >= 1 and len(w["empty_init"]["words"]) >= 3
    assert w["empty_lattice"]["bayes_risk"] == np.inf and w["empty_lattice"]["gamma"] == [] and w["self_loop"]["words"] == []
    assert w["max_words_1_on_3_words"]["status"] == ref.WORDS and w["max_words_2_grows_to_3"]["status"] == ref.WORDS
    assert w["max_words_3_is_enough"]["words"] == [1, 2, 3]
    assert w["confidences_of_a_foreign_word"]["conf"][1] == 0.0 and w["confidences_of_a_foreign_word"]["conf"][0] > 0.0      # 9 is on no arc
    assert np.bincount(w["hub_70_in_arcs"]["vocab"]).sum() == 71
    # with the default cap no seeded run ends with KHG_LAT_WORDS, from the best path or from the unrelated reference
    assert all(x["want"]["status"] & ref.SUCCEEDED for x in items if x["name"].startswith("random"))
    assert all(len(x["want"]["words"]) <= x["want"]["cap"] for x in items if x["want"]["status"] & ref.SUCCEEDED)


def test_confidences_only_keeps_the_initial_hypothesis(work):
    khg, items = work
    n = 0
    for x in items[::7]:
        if x["want"]["status"] & ref.SUCCEEDED == 0 or x["max_words"]:
            continue
        got = _lattice(khg, x["lat"]).mbr(x["gs"], x["as_"], False, 32, x["init"])
        init = x["init"] if x["init"] is not None else _lattice(khg, x["lat"]).best_path(x["gs"], x["as_"])["words"]
        assert got["iters"] == 0 and got["status"] == ref.SUCCEEDED and got["words"].tolist() == list(init), x["name"]
        assert len(got["risks"]) == 1 and ((got["conf"] >= 0) & (got["conf"] <= 1 + 1e-12)).all(), x["name"]
        n += 1
    assert n > 100
    lat = _lattice(khg, cases.diamond())
    with pytest.raises(RuntimeError, match="not > 0"):
        lat.mbr(1.0, 0.1, init=[1, 0])
    with pytest.raises(RuntimeError, match="max_iter"):
        lat.mbr(1.0, 0.1, max_iter=-1)
    with pytest.raises(RuntimeError, match="come together"):
        lat.mbr(1.0, 0.1, arc_cond=np.zeros(7))


def test_refusals_need_no_context_and_no_device():
    from kaldi_hmm_gmm_amd import _lib
    lib = _lib.lib
    E_ARG = -1
    out = C.c_void_p()
    call = lambda gs, as_, it, mw, sb: lib.khg_lattices_mbr(None, None, gs, as_, 1, it, 0, None, None, None, mw, sb, C.byref(out))  # noqa: E731
    for args, text in (((float("nan"), 0.1, 4, 0, 0), b"finite"), ((1.0, -0.5, 4, 0, 0), b"finite"), ((float("inf"), 1.0, 4, 0, 0), b"finite"),
                       ((1.0, 0.1, -1, 0, 0), b"max_iter"), ((1.0, 0.1, 4, -1, 0), b"max_words"), ((1.0, 0.1, 4, 2048, 0), b"max_words"),
                       ((1.0, 0.1, 4, 0, -1), b"scratch_bytes"), ((1.0, 0.1, 4, 0, 0), b"bad arguments")):
        assert call(*args) == E_ARG and text in lib.khg_last_error(), args
    assert lib.khg_mbr_sizes(None, None, None, None) == E_ARG and lib.khg_mbr_device_bytes(None, None) == E_ARG
    assert lib.khg_mbr_download(None, None, None, None, None, None, None, None, None, None, None) == E_ARG
    assert lib.khg_mbr_destroy(None) == 0


def test_symbols_are_declared_exported_and_bound():
    import kaldi_hmm_gmm_amd as khg
    from kaldi_hmm_gmm_amd import _lib
    header = open(HEADER).read()
    for name in ("khg_lattices_mbr", "khg_mbr_sizes", "khg_mbr_download", "khg_mbr_device_bytes", "khg_mbr_destroy"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name) and ("int %s(" % name) in header, name
    assert "#define KHG_LAT_NOT_CONVERGED 2048" in header and "typedef struct khg_mbr khg_mbr;" in header
    assert hasattr(khg.DeviceLattices, "mbr") and hasattr(khg.Lattice, "mbr")
    for name in ("lattice_mbr_decode", "lattice_mbr_decode_batch", "mbr_utterances"):
        assert callable(getattr(khg, name)), name
