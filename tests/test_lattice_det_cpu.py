"""lattice-determinize-pruned on the host: Lattice.determinize against the plain restatement
(tests/lattice_det_ref.py) on the bits, and, independent of the restatement, the property that makes the rule determinization, by
brute-force path enumeration: the word sequences of the result are those of the input, each has exactly one path, and that path is the
cheapest the sequence has.  No GPU."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lattice_det_cases as cases  # noqa: E402
import lattice_det_ref as ref  # noqa: E402

F = np.float32


def _khg():
    import kaldi_hmm_gmm_amd as khg
    return khg


def _lattice(lat):
    return _khg().Lattice.from_arrays(*[lat[k] for k in ref.FIELDS], int(lat["start"]))


def _arrays(l):
    out = {k: np.asarray(getattr(l, k)) for k in ref.FIELDS}
    out["start"] = l.start
    return out


def _same_lattice(got, want, tag):
    for k in ref.FIELDS:
        g = np.asarray(getattr(got, k))
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (tag, k, g.shape, want[k].shape)
        assert g.tobytes() == want[k].tobytes(), (tag, k)
    assert got.start == want["start"], tag


@functools.lru_cache(maxsize=None)
def _all_cases():
    return cases.all_cases()


def test_c_abi_symbol_and_null_arguments():
    from kaldi_hmm_gmm_amd import _lib
    assert "khg_lattices_determinize" in _lib.SIGNATURES and hasattr(_lib.lib, "khg_lattices_determinize")
    assert _lib.lib.khg_lattices_determinize(None, None, 1.0, 1.0, 10.0, 0.0, 8, None, None, None) == -1


@pytest.mark.parametrize("kw, message", [
    ({"beam": -1.0}, "beam must be finite and >= 0"), ({"beam": np.inf}, "beam must be finite and >= 0"),
    ({"delta": -0.5}, "delta must be finite and >= 0"), ({"delta": np.nan}, "delta must be finite and >= 0"),
    ({"state_factor": 0}, "state_factor must be >= 1"), ({"graph_scale": -1.0}, "must be finite and >= 0"),
    ({"acoustic_scale": np.inf}, "must be finite and >= 0"),
])
def test_arguments_are_refused_by_name(kw, message):
    khg = _khg()
    with pytest.raises(khg.KhgError, match=message):
        _lattice(cases.two_alignments()).determinize(**kw)


def test_host_form_equals_the_restatement_on_the_bits():
    seen = {}
    for name, lat, gs, as_, beam, delta, sf, expect in _all_cases():
        want, st, stats = ref.determinize(lat, gs, as_, beam, delta, sf)
        if expect is not None:
            assert st == expect, (name, st)
        got, gst, gstats = _lattice(lat).determinize(gs, as_, beam, delta, sf)
        assert gst == st, (name, gst, st)
        _same_lattice(got, want, name)
        assert gstats == stats, (name, gstats, stats)
        seen[st] = seen.get(st, 0) + 1
    assert seen[ref.SUCCEEDED] > 100 and seen[ref.SCRATCH] >= 1 and seen[ref.EPS_LOOP] == 2 and seen[ref.NO_PATH] >= 2, seen


def test_what_the_hand_cases_are_there_for():
    c = cases.hand_cases()

    def run(name):
        lat, gs, as_, beam, delta, sf, _ = c[name]
        return (lat,) + ref.determinize(lat, gs, as_, beam, delta, sf)

    # the cheaper alignment survives; in an exact tie the lower arc
    lat, out, _, stats = run("two_alignments")
    assert out["ilabel"].tolist() == [6, 8] and stats["max_subset"] == 2
    lat, out, _, _ = run("exact_tie")
    assert out["ilabel"].tolist() == [5, 7]
    # the outside arc into a dominated state is gone; when the state is not dominated it is the arc inside the closure that goes
    lat, out, _, stats = run("dominated_initial")
    assert sorted(out["ilabel"].tolist()) == [0, 5, 8] and stats["max_subset"] == 1
    lat, out, _, stats = run("initial_not_dominated")
    assert sorted(out["ilabel"].tolist()) == [6, 8] and stats["max_subset"] == 2
    lat, out, _, stats = run("negative_best_dominated")
    assert sorted(out["ilabel"].tolist()) == [0, 5, 8] and stats["max_subset"] == 1
    # one final per determinized state
    lat, out, _, _ = run("two_finals")
    assert np.isfinite(out["final_cost"]).sum() == 1 and out["final_cost"][2] == F(0.125)
    lat, out, _, stats = run("dead_ends_unreachable")
    assert out["graph_state"].tolist() == [100, 102, 105] and stats["pruned_states"] == 3
    assert run("state_factor_1")[2] == ref.SCRATCH and run("state_factor_2")[2] == ref.SUCCEEDED
    assert run("fan70_words")[3]["det_states"] == 72 and run("fan70_into_one_state")[3]["max_subset"] == 70
    s = run("sausage")[3]
    assert (s["in_states"], s["det_states"], s["out_states"]) == (58, 22, 86)
    assert run("near_pair_merges")[3]["det_states"] + 1 == run("near_pair_apart")[3]["det_states"]


def _paths(lat, gs, as_):
    """every path from the start to a final state of the last frame: [(words, cost, arcs on it, largest partial cost)]; the cost is the
    double sum of the float arc weights"""
    out = []
    N = len(lat["frame"])
    if N == 0:
        return out
    ab, T = lat["arc_begin"], lat["frame"][N - 1]
    gs, as_ = F(gs), F(as_)

    def walk(s, words, cost, n, big):
        if np.isfinite(lat["final_cost"][s]) and lat["frame"][s] == T:
            c = cost + float(F(gs * lat["final_cost"][s]))
            out.append((tuple(words), c, n, max(big, abs(c))))
        for a in range(ab[s], ab[s + 1]):
            w = float(F(gs * lat["graph_cost"][a])) + (float(F(as_ * lat["acoustic_cost"][a])) if lat["ilabel"][a] != 0 else 0.0)
            ol = int(lat["olabel"][a])
            walk(int(lat["nextstate"][a]), words + [ol] if ol else words, cost + w, n + 1, max(big, abs(cost + w), abs(w)))

    walk(int(lat["start"]), [], 0.0, 0, 0.0)
    return out


def _cheapest(paths):
    best = {}
    for w, c, n, big in paths:
        if w not in best or c < best[w][0]:
            best[w] = (c, n, big)
    return best


def _bound(words, n, big, delta):
    # one rounding per normalisation and per sum along the path, and one possible misranking of at most 2 * delta per merge
    return 4 * (len(words) + 1) * float(F(delta)) + 16 * max(n, 1) * 2.0 ** -24 * big


def test_one_path_per_word_sequence_and_it_is_the_cheapest():
    """beam 1e30: the word sequences of the result are exactly those of the input, each on exactly one path, whose cost is within
    4 (n_words + 1) delta + 16 L 2^-24 M of the brute-force minimum over the input"""
    n_lat = n_seq = 0
    worst = 0.0
    for name, lat, gs, as_, _, delta, sf, _ in _all_cases():
        got, st, _ = _lattice(lat).determinize(gs, as_, cases.BIG, delta, sf)
        if st != ref.SUCCEEDED:
            assert got.num_states == 0, name
            continue
        pin, pout = _paths(lat, gs, as_), _paths(_arrays(got), gs, as_)
        want = _cheapest(pin)
        assert sorted(p[0] for p in pout) == sorted(want), name       # the same sequences, each once
        for w, c, n, big in pout:
            excess = c - want[w][0]
            worst = max(worst, excess)
            assert -1e-12 <= excess <= _bound(w, n, max(big, want[w][2]), delta), (name, w, c, want[w][0])
            n_seq += 1
        n_lat += 1
    print("largest excess over the brute-force minimum: %.3e over %d sequences of %d lattices" % (worst, n_seq, n_lat))
    assert n_lat > 100 and n_seq > 3000


def test_finite_beam_keeps_what_is_within_it_and_the_best_path_of_prune():
    n = 0
    for name, lat, gs, as_, beam, delta, sf, _ in _all_cases():
        if beam >= cases.BIG:
            continue
        got, st, _ = _lattice(lat).determinize(gs, as_, beam, delta, sf)
        if st != ref.SUCCEEDED:
            continue
        want = _cheapest(_paths(lat, gs, as_))
        pout = _paths(_arrays(got), gs, as_)
        have = [p[0] for p in pout]
        assert len(set(have)) == len(have) and set(have) <= set(want), name
        best = min(c for c, _, _ in want.values())
        for w, (c, k, big) in want.items():
            if c + _bound(w, k, big, delta) < best + beam:
                assert w in have, (name, w, c, best, beam)
        pruned, pst = _lattice(lat).prune_with_status(beam, gs, as_)
        assert pst == ref.SUCCEEDED
        a, b = got.best_path(gs, as_), pruned.best_path(gs, as_)
        assert a["status"] == b["status"] == ref.SUCCEEDED and a["words"] == b["words"] and a["weight"] == b["weight"], (name, a["weight"], b["weight"])
        n += 1
    assert n > 50


def test_determinizing_a_result_again_keeps_sequences_and_costs():
    n = 0
    for name, lat, gs, as_, beam, delta, sf, _ in _all_cases():
        got, st, _ = _lattice(lat).determinize(gs, as_, beam, delta, sf)
        if st != ref.SUCCEEDED:
            continue
        again, st2, stats = got.determinize(gs, as_, beam, delta, sf)
        assert st2 == ref.SUCCEEDED, name
        p1 = sorted((p[0], p[1]) for p in _paths(_arrays(got), gs, as_))
        p2 = sorted((p[0], p[1]) for p in _paths(_arrays(again), gs, as_))
        assert p1 == p2, name
        n += 1
    assert n > 100
