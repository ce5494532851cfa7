"""Hand-made and seeded cases for minimum Bayes risk decoding of lattices.  The lattices are those of the
scoring and LM-rescoring cases (by import), plus a few of this file's.  A case is a dict: name, lat, init (None: the best path's words),
decode_mbr, max_iter, max_words, expect (the status the case is there for, or None)."""
import numpy as np

import lattice_mbr_ref as ref
from lattice_lm_cases import diamond, fan, hand  # noqa: F401
from lattice_score_cases import chain_lattice, layered, random_cases, reference_of_length
from lattice_score_cases import hand_cases as score_hand_cases

INF = np.inf
S, NO_PATH, EPS_LOOP, WORDS, NOT_CONVERGED = ref.SUCCEEDED, ref.NO_PATH, ref.EPS_LOOP, ref.WORDS, ref.NOT_CONVERGED
PAIRS = [(1.0, 0.1), (1.0, 1.0), (0.0, 0.0)]


def case(name, lat, init=None, decode_mbr=True, max_iter=32, max_words=0, expect=None):
    return {"name": name, "lat": lat, "init": None if init is None else [int(w) for w in init], "decode_mbr": decode_mbr, "max_iter": max_iter,
            "max_words": max_words, "expect": expect}


def two_equal_paths():
    """two paths of exactly equal weight, words 2 (the lower arc) and 1: gamma ties at position 2, the lowest id must win"""
    return hand([(0, INF), (1, 0.5), (1, 0.5)], [(0, 7, 2, 0.5, 1.0, 1), (0, 8, 1, 0.5, 1.0, 2)])


def two_equal_paths_then_word():
    """the same tie, then both paths carry word 3 through a common state"""
    return hand([(0, INF), (1, INF), (1, INF), (2, 0.25)], [(0, 7, 5, 0.5, 1.0, 1), (0, 8, 4, 0.5, 1.0, 2), (1, 9, 3, 0.25, 2.0, 3), (2, 9, 3, 0.25, 2.0, 3)])


def hand_cases():
    sc = score_hand_cases()
    rng = np.random.default_rng(777)
    c = []
    # single-path lattices: every weight is exactly 1.0 on every side
    c.append(case("single_path_exact", chain_lattice([1, 2, 3]), [1, 2, 3], expect=S))
    c.append(case("single_path_sub", chain_lattice([1, 2, 3]), [1, 4, 3], expect=S))
    c.append(case("single_path_lattice_word_extra", chain_lattice([1, 2, 3]), [1, 3], expect=S))
    c.append(case("single_path_hyp_word_extra", chain_lattice([1, 2, 3]), [1, 2, 5, 3], expect=S))
    c.append(case("single_path_tie_12_21", chain_lattice([1, 2]), [2, 1], expect=S))
    c.append(case("single_path_ins_from_1_4", chain_lattice([1, 2, 3, 4]), [1, 4], expect=S))
    c.append(case("single_path_ins_max_iter_0", chain_lattice([1, 2, 3, 4]), [1, 4], max_iter=0, expect=S | NOT_CONVERGED))
    c.append(case("single_path_ins_max_iter_1", chain_lattice([1, 2, 3, 4]), [1, 4], max_iter=1, expect=S | NOT_CONVERGED))
    c.append(case("single_path_confidences_only", chain_lattice([1, 2, 3]), [1, 4, 3], decode_mbr=False, expect=S))
    c.append(case("chain3_against_64_words", chain_lattice([1, 2, 3]), [3, 1, 2, 2] * 16, expect=S))
    # exact gamma ties
    c.append(case("gamma_tie_lowest_id", two_equal_paths(), expect=S))
    c.append(case("gamma_tie_from_the_higher_word", two_equal_paths(), [2], expect=S))
    c.append(case("gamma_tie_then_word", two_equal_paths_then_word(), expect=S))
    # the wave-segment edges: Q + 1 = 62, 64, 66, 128, 130
    for W in (30, 31, 32, 63, 64):
        lat = layered(rng, [1] + [int(rng.integers(1, 4)) for _ in range(W + 1)], 4, p_word=0.9)
        c.append(case("segment_edge_w%d" % W, lat, reference_of_length(rng, lat, 4, W), expect=S))
    # hubs, epsilons, odd starts, several finals
    for name in ("hub_70_in_arcs", "hub_70_few_words", "epsilon_chain", "start_not_first", "unreachable_state", "several_finals_equal_errors",
                 "last_frame_not_final", "final_before_last_frame", "two_paths_rejoin_equal_errors"):
        c.append(case(name, sc[name][0], expect=S))
        c.append(case(name + "_from_reference", sc[name][0], sc[name][1], expect=S))
    # empty and refused
    c.append(case("one_state", sc["one_state"][0], expect=S))
    c.append(case("one_state_init_2_words", sc["one_state"][0], [1, 2], expect=S))
    c.append(case("no_word", sc["no_word"][0], expect=S))
    c.append(case("no_word_init_1", sc["no_word"][0], [1], expect=S))
    c.append(case("empty_init", diamond(), [], expect=S))
    c.append(case("empty_lattice", sc["empty"][0], expect=NO_PATH))
    c.append(case("empty_lattice_init", sc["empty"][0], [1, 2], expect=NO_PATH))
    c.append(case("no_final_reachable", sc["no_final_reachable"][0], expect=NO_PATH))
    c.append(case("self_loop", sc["self_loop"][0], expect=EPS_LOOP))
    c.append(case("arc_to_lower_state", sc["arc_to_lower_state"][0], [1, 2], expect=EPS_LOOP))
    # caps
    c.append(case("max_words_1_on_3_words", chain_lattice([1, 2, 3]), max_words=1, expect=WORDS))
    c.append(case("max_words_2_grows_to_3", chain_lattice([1, 2, 3]), [1, 2], max_words=2, expect=WORDS))
    c.append(case("max_words_3_is_enough", chain_lattice([1, 2, 3]), [1], max_words=3, expect=S))
    c.append(case("confidences_of_a_foreign_word", diamond(), [1, 9, 3], decode_mbr=False, expect=S))
    return c


def seeded(n=200, seed=2025):
    """[(lattice, unrelated reference)]: lattice_score_cases.random_cases"""
    return random_cases(n, seed)


def seeded_cases(n=200, seed=2025):
    """every seeded lattice from the best path and from its reference"""
    out = []
    for i, (lat, r) in enumerate(seeded(n, seed)):
        out.append(case("random%d" % i, lat))
        out.append(case("random%d_from_reference" % i, lat, r))
    return out
