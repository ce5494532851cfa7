"""The backoff n-gram LM and lattice-lmrescore on the host: the ARPA reader, khg_lm_validate, khg_lm_score, the
estimator, Lattice.lm_rescore against the plain restatement (tests/lattice_lm_ref.py) on the bits, and the property that makes the
rule lattice-lmrescore: the paths of the result are the paths of the input, each costing scale * score(words) more.  No GPU."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lattice_lm_cases as cases  # noqa: E402
import lattice_lm_ref as ref  # noqa: E402

F = np.float32

ARPA = """
\\data\\
ngram 1=5
ngram 2=6
ngram 3=3

\\1-grams:
-99 <s> -0.5
-0.7 </s>
-0.6 yes -0.4
-0.5 no -0.3
-1.2 maybe

\\2-grams:
-0.3 <s> yes -0.2
-0.4 <s> no
-0.25 yes no -0.1
-0.9 yes </s>
-0.35 no yes
-0.45 no </s>

\\3-grams:
-0.15 <s> yes no
-0.2 yes no yes
-0.1 yes no </s>

\\end\\
"""
W2I = {"yes": 1, "no": 2, "maybe": 3}


def _khg():
    import kaldi_hmm_gmm_amd as khg
    return khg


def _lm(arrays):
    return _khg().NgramLm(**arrays)


def _lattice(lat):
    return _khg().Lattice.from_arrays(*[lat[k] for k in ref.FIELDS], int(lat["start"]))


def _same_lattice(got, want, tag):
    for k in ref.FIELDS:
        g = np.asarray(getattr(got, k))
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (tag, k, g.shape, want[k].shape)
        assert g.tobytes() == want[k].tobytes(), (tag, k)
    assert got.start == want["start"], tag


def _bits(x):
    return int(np.asarray(x, np.float32).view(np.uint32))


def test_from_arpa_builds_the_recorded_automaton():
    lm = _khg().NgramLm.from_arpa(ARPA, W2I)
    # the empty history; <s>, yes, no, maybe; (<s>, yes), (<s>, no), (yes, no), (no, yes)
    assert lm.num_states == 9 and lm.start == 1
    assert lm.backoff.tolist() == [-1, 0, 0, 0, 0, 2, 3, 3, 2]
    assert lm.arc_begin.tolist() == [0, 3, 5, 6, 7, 7, 8, 8, 9, 9]
    assert lm.word.tolist() == [1, 2, 3, 1, 2, 2, 1, 2, 1]
    # an arc goes to the longest suffix of history + word that is a state
    assert lm.next.tolist() == [2, 3, 4, 5, 6, 7, 8, 7, 8]
    ln10 = math.log(10.0)
    assert _bits(lm.cost[0]) == _bits(F(-ln10 * -0.6)) and _bits(lm.cost[8]) == _bits(F(-ln10 * -0.2))
    assert _bits(lm.cost[0]) == 0x3FB0D6AA and _bits(lm.cost[8]) == 0x3EEBC8E3      # 1.3815511, 0.4605170
    assert _bits(lm.backoff_cost[2]) == _bits(F(-ln10 * -0.4)) and lm.backoff_cost[4] == 0.0 and lm.backoff_cost[6] == 0.0 and lm.backoff_cost[8] == 0.0
    # final_cost by the lookup rule: (yes, no) lists </s>; (<s>, yes) backs off to yes, which lists it; maybe goes down to the unigram
    assert _bits(lm.final_cost[7]) == _bits(F(-ln10 * -0.1))
    assert _bits(lm.final_cost[5]) == _bits(F(F(-ln10 * -0.2) + F(-ln10 * -0.9)))
    assert _bits(lm.final_cost[4]) == _bits(F(F(0.0) + F(-ln10 * -0.7)))
    assert _bits(lm.final_cost[1]) == _bits(F(F(-ln10 * -0.5) + F(-ln10 * -0.7)))


@pytest.mark.parametrize("edit, word2id, message", [
    (lambda t: t.replace("-0.7 </s>\n", "").replace("ngram 1=5", "ngram 1=4"), W2I, "no unigram for </s>"),
    (lambda t: t.replace("-99 <s> -0.5\n", "").replace("ngram 1=5", "ngram 1=4"), W2I, "no unigram for <s>"),
    (lambda t: t, {"yes": 1, "no": 2}, "'maybe' is not in word2id"),
    (lambda t: t, {"yes": 1, "no": 2, "maybe": 0}, "word-ids are > 0"),
    (lambda t: t.replace("ngram 2=6", "ngram 2=7"), W2I, "announces 7 2-grams, the section lists 6"),
    (lambda t: t.replace("ngram 3=3\n", ""), W2I, "announces no 3-grams"),
    (lambda t: t.replace("-0.2 yes no yes", "-0.2 maybe no yes"), W2I, "is not listed"),
])
def test_from_arpa_refuses_by_name(edit, word2id, message):
    khg = _khg()
    with pytest.raises(khg.KhgError, match=message):
        khg.NgramLm.from_arpa(edit(ARPA), word2id)


def _broken(key, index, value):
    def f(lm):
        lm[key] = lm[key].copy()
        lm[key][index] = value
    return f


@pytest.mark.parametrize("edit, message", [
    (_broken("backoff", 0, 0), r"backoff\[0\] must be -1"),
    (_broken("backoff", 3, 3), "state 3: backoff must name a lower state"),
    (_broken("backoff", 3, -1), "state 3: backoff must name a lower state"),
    (_broken("backoff_cost", 2, np.inf), "state 2: backoff_cost is not finite"),
    (_broken("final_cost", 5, np.inf), "state 5: final_cost is not finite"),
    (_broken("final_cost", 0, np.nan), "state 0: final_cost is not finite"),
    (_broken("word", 0, 0), "arc 0: word must be > 0"),
    (_broken("word", 1, 1), "arc 1: words must ascend strictly"),
    (_broken("cost", 4, -np.inf), "arc 4: cost is not finite"),
    (_broken("next", 2, 9), "arc 2: next out of range"),
    (_broken("next", 2, -1), "arc 2: next out of range"),
    (_broken("arc_begin", 0, 1), "arc_begin must run from 0"),
    (_broken("arc_begin", 3, 2), "arc_begin must run from 0, monotone"),
    (lambda lm: lm.update(start=9), "start out of range"),
    (lambda lm: lm.update(start=-1), "start out of range"),
    (lambda lm: lm.update(cost=lm["cost"][:-1]), "one word, cost and next per arc"),
    (lambda lm: lm.update(final_cost=lm["final_cost"][:-1]), "one backoff, backoff_cost and final_cost per state"),
])
def test_lm_validate_refuses_by_name(edit, message):
    khg = _khg()
    lm = dict(khg.NgramLm.from_arpa(ARPA, W2I).to_arrays())
    edit(lm)
    with pytest.raises(khg.KhgError, match=message):
        khg.NgramLm(**lm)


def test_c_abi_symbols_and_null_arguments():
    from kaldi_hmm_gmm_amd import _lib
    for name in ("khg_lm_validate", "khg_lm_create", "khg_lm_destroy", "khg_lm_num_states", "khg_lm_device_bytes", "khg_lm_score",
                 "khg_lattices_lm_rescore"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert _lib.lib.khg_lm_validate(0, None, None, None, None, None, None, None, 0) == -1
    assert _lib.lib.khg_lm_num_states(None, None) == -1 and _lib.lib.khg_lm_device_bytes(None, None) == -1
    assert _lib.lib.khg_lm_destroy(None) == 0
    assert _lib.lib.khg_lattices_lm_rescore(None, None, None, 1.0, 8, None, None, None) == -1


def test_score_equals_the_restatement_on_the_bits():
    khg = _khg()
    rng = np.random.default_rng(3)
    lms = [khg.NgramLm.from_arpa(ARPA, W2I).to_arrays(), cases.trigram_chain(), cases.bigram(3), cases.unigram(3)] + [cases.random_lm(rng, 3) for _ in range(20)]
    n = 0
    for k, arrays in enumerate(lms):
        lm = _lm(arrays)
        for _ in range(30):
            words = rng.integers(1, 4, size=int(rng.integers(0, 9))).tolist()
            want = ref.score(arrays, words)
            assert _bits(lm.score(words)) == _bits(want), (k, words)
            n += 1
        with pytest.raises(khg.KhgError, match=r"word 1 \(7\) is out of vocabulary"):
            lm.score([1, 7])
        with pytest.raises(khg.KhgError, match="word 0 is not > 0"):
            lm.score([0])
    assert n == 720
    # by hand: <s> yes no </s> takes the trigram, then the trigram's </s>
    lm = khg.NgramLm.from_arpa(ARPA, W2I)
    ln10 = math.log(10.0)
    want = F(F(F(F(0.0) + F(-ln10 * -0.3)) + F(-ln10 * -0.15)) + F(-ln10 * -0.1))
    assert _bits(lm.score([1, 2])) == _bits(want)


def _advance64(lm, h, w):
    c = 0.0
    while True:
        a, b = int(lm["arc_begin"][h]), int(lm["arc_begin"][h + 1])
        hit = [i for i in range(a, b) if lm["word"][i] == w]
        if hit:
            return int(lm["next"][hit[0]]), c + float(lm["cost"][hit[0]]), [float(lm["cost"][hit[0]])]
        assert h != 0
        c += float(lm["backoff_cost"][h])
        h = int(lm["backoff"][h])


@pytest.mark.parametrize("order", [1, 2, 3])
def test_estimated_lm_normalises_for_every_history(order):
    khg = _khg()
    rng = np.random.default_rng(order)
    vocab = [1, 2, 3, 4, 7]
    trans = np.array([[0.1, 0.6, 0.1, 0.1, 0.1], [0.5, 0.1, 0.2, 0.1, 0.1], [0.1, 0.1, 0.1, 0.6, 0.1], [0.3, 0.3, 0.2, 0.1, 0.1], [0.2, 0.2, 0.2, 0.2, 0.2]])
    transcripts = []
    for _ in range(60):
        k, t = int(rng.integers(0, 5)), []
        for _ in range(int(rng.integers(0, 7))):
            t.append(vocab[k])
            k = int(rng.choice(5, p=trans[k]))
        transcripts.append(t)
    lm = khg.estimate_ngram_lm(transcripts, order, vocab, 0.5)
    a = lm.to_arrays()
    assert lm.num_states > (1 if order > 1 else 0)
    worst = 0.0
    for h in range(lm.num_states):
        tot = math.exp(-float(a["final_cost"][h])) + sum(math.exp(-_advance64(a, h, w)[1]) for w in vocab)
        worst = max(worst, abs(tot - 1.0))
    assert worst <= 1e-6, worst
    with pytest.raises(khg.KhgError, match="not in the vocabulary"):
        khg.estimate_ngram_lm([[1, 5]], order, vocab)
    # the empty corpus: uniform over the vocabulary and the sentence end
    u = khg.estimate_ngram_lm([], order, vocab)
    assert u.num_states == 1 and np.allclose(u.cost, math.log(6.0)) and np.allclose(u.final_cost, math.log(6.0))


def test_unigram_is_the_word_loop_graphs_lm():
    lm = _khg().NgramLm.unigram({3: 0.5, 1: 0.25, 2: 0.25})
    assert lm.num_states == 1 and lm.start == 0 and lm.word.tolist() == [1, 2, 3] and lm.final_cost.tolist() == [0.0]
    assert _bits(lm.cost[2]) == _bits(F(-math.log(0.5))) and _bits(lm.score([3, 3])) == _bits(F(F(-math.log(0.5)) + F(-math.log(0.5))))


def _all_cases():
    out = [(name,) + c for name, c in sorted(cases.hand_cases().items())]
    out += [("random%d" % i,) + c + (None,) for i, c in enumerate(cases.random_cases())]
    return out


def test_host_form_equals_the_restatement_on_the_bits():
    seen = {}
    for name, lat, lm, scale, hf, expect in _all_cases():
        want, st, mh = ref.lm_rescore(lat, lm, scale, hf)
        if expect is not None:
            assert st == expect, (name, st)
        got, gst, stats = _lattice(lat).lm_rescore(_lm(lm), scale, hf)
        assert gst == st, (name, gst, st)
        _same_lattice(got, want, name)
        assert stats == {"in_states": len(lat["frame"]), "in_arcs": len(lat["ilabel"]), "out_states": len(want["frame"]),
                         "out_arcs": len(want["ilabel"]), "max_hist": mh}, (name, stats)
        seen[st] = seen.get(st, 0) + 1
    assert seen[ref.SUCCEEDED] > 150 and seen[ref.SCRATCH] > 5 and seen[ref.LM_OOV] == 1 and seen[ref.EPS_LOOP] == 2 and seen[ref.NO_PATH] == 1


def test_what_the_hand_cases_are_there_for():
    c = cases.hand_cases()

    def run(name):
        lat, lm, scale, hf, _ = c[name]
        return (lat,) + ref.lm_rescore(lat, lm, scale, hf)

    assert run("diamond_bigram")[3] == 2 and run("diamond_unigram")[3] == 1 and run("diamond_trigram_backoff2")[3] == 2
    assert run("fan70_distinct")[3] == 70 and run("fan70_three_histories")[3] == 3
    lat, out, st, _ = run("no_words")
    assert all(out[k].tobytes() == lat[k].tobytes() for k in ref.FIELDS if k != "final_cost")
    lat, out, st, _ = run("unreachable")
    assert len(out["frame"]) == 3 and out["graph_state"].tolist() == [100, 102, 103] and out["start"] == 0
    lat, out, st, _ = run("start_not_first")
    assert out["graph_state"].tolist() == [101, 102, 103] and out["start"] == 0
    lat, out, st, _ = run("one_state")
    assert len(out["frame"]) == 1 and len(out["ilabel"]) == 0
    # scale 0: the structure expands, every cost keeps its bits
    lat, out, st, _ = run("scale_0")
    assert len(out["frame"]) == 9
    old = sorted(zip(lat["ilabel"].tolist(), lat["graph_cost"].view(np.uint32).tolist()))
    assert sorted(set(zip(out["ilabel"].tolist(), out["graph_cost"].view(np.uint32).tolist()))) == old
    assert set(out["final_cost"].view(np.uint32).tolist()) == set(lat["final_cost"].view(np.uint32).tolist())
    # the depth-2 backoff chain: (1, 3) and (3,) lack word 2
    tri = cases.trigram_chain()
    h13 = 6
    assert ref.advance(tri, h13, 2) == (3, F(F(F(F(0.0) + tri["backoff_cost"][h13]) + tri["backoff_cost"][4]) + F(2.3)))
    assert (run("negative_costs")[1]["graph_cost"] < 0).any()


def _paths(lat):
    """every path from the start to a state with a finite final cost: [(labels, acoustic bits, graph terms)]"""
    out = []
    if len(lat["frame"]) == 0:
        return out
    ab = lat["arc_begin"]

    def walk(s, labels, ac, g):
        if np.isfinite(lat["final_cost"][s]):
            out.append((tuple(labels), tuple(ac), g + [float(lat["final_cost"][s])]))
        for a in range(ab[s], ab[s + 1]):
            walk(int(lat["nextstate"][a]), labels + [(int(lat["ilabel"][a]), int(lat["olabel"][a]))],
                 ac + [int(lat["acoustic_cost"][a:a + 1].view(np.uint32)[0])], g + [float(lat["graph_cost"][a])])

    walk(int(lat["start"]), [], [], [])
    return out


def test_the_paths_of_the_result_are_the_paths_of_the_input_rescored():
    """Independent of the restatement: brute-force path enumeration of the input and of Lattice.lm_rescore's result."""
    n_paths = n_lat = 0
    for name, lat, lm, scale, hf, _ in _all_cases():
        got, st, _ = _lattice(lat).lm_rescore(_lm(lm), scale, hf)
        if st != ref.SUCCEEDED:
            assert got.num_states == 0, name
            continue
        out = {k: np.asarray(getattr(got, k)) for k in ref.FIELDS}
        out["start"] = got.start
        pin, pout = _paths(lat), _paths(out)
        key = lambda p: (p[0], p[1])       # noqa: E731
        assert sorted(map(key, pin)) == sorted(map(key, pout)), name
        # pair the paths that share labels and acoustic costs by their graph cost (the LM's part is the same inside such a group)
        pin.sort(key=lambda p: (p[0], p[1], sum(p[2])))
        pout.sort(key=lambda p: (p[0], p[1], sum(p[2])))
        s64 = float(F(scale))
        for (labels, _, gin), (_, _, gout) in zip(pin, pout):
            h, terms = int(lm["start"]), []
            for _, w in labels:
                if w:
                    c = 0.0
                    while True:
                        a, b = int(lm["arc_begin"][h]), int(lm["arc_begin"][h + 1])
                        hit = [i for i in range(a, b) if lm["word"][i] == w]
                        if hit:
                            terms.append(float(lm["cost"][hit[0]])); h = int(lm["next"][hit[0]])
                            break
                        terms.append(float(lm["backoff_cost"][h])); h = int(lm["backoff"][h])
            terms.append(float(lm["final_cost"][h]))
            want = sum(gin) + s64 * sum(terms)
            # The path's own sum is taken in double here, so the roundings are those inside each arc: at most two additions along a
            # trigram's backoff chain, the product with the scale and the addition to the graph cost -- four, each within 2^-24 of the
            # arc's own terms, 2^-22 in all; the final weight (counted as one more arc) has two.  n_arcs >= 2 wherever there is an arc.
            bound = (len(labels) + 1) * 2.0 ** -23 * (sum(abs(x) for x in gin) + abs(s64) * sum(abs(x) for x in terms))
            assert abs(sum(gout) - want) <= bound, (name, sum(gout), want, bound)
            n_paths += 1
        n_lat += 1
    assert n_lat > 150 and n_paths > 2000
