"""Hand-made and seeded random cases for lattice-to-nbest: the smallest shapes at which each part of the rule
can go wrong.  A case is (name, lattice, expected status or None); lattices are the dicts of arrays the other lattice tests use.  Every
lattice passes khg_lattices_validate: states ordered by frame, an emitting arc goes one frame on, an epsilon arc stays in its frame."""
import numpy as np

import lattice_nbest_ref as ref
from lattice_lm_cases import diamond, fan, hand, random_lattice

INF = np.inf
NAN = np.nan
PAIRS = ((1.0, 1.0), (1.0, 0.1), (0.5, 1.7), (0.0, 0.0))
NS = (1, 2, 5, 63, 64, 65, 130, 1024)


def tie_in_arcs():
    """two paths of exactly the same cost meet in state 3 through the arcs 2 and 3: the lower arc comes first"""
    return hand([(0, INF), (1, INF), (1, INF), (2, 0.25)],
                [(0, 5, 1, 1.0, 0.5, 1), (0, 6, 2, 1.0, 0.5, 2), (1, 7, 3, 0.5, 0.25, 3), (2, 8, 4, 0.5, 0.25, 3)])


def tie_ranks():
    """two parallel arcs of the same cost give state 1 two prefixes that tie; along the one arc 1 -> 2 they are two ranks of one source"""
    return hand([(0, INF), (1, INF), (2, 0.0)], [(0, 5, 1, 1.0, 0.5, 1), (0, 6, 2, 1.0, 0.5, 1), (1, 7, 3, 0.5, 0.25, 2)])


def negative():
    return hand([(0, INF), (1, INF), (1, INF), (2, -0.75)],
                [(0, 5, 1, -1.0, 0.5, 1), (0, 6, 2, 2.0, 0.25, 2), (1, 7, 3, 0.5, 0.25, 3), (2, 8, 4, -3.5, 0.125, 3), (1, 0, 5, -0.125, 0.0, 2)])


def finals():
    """two finals on the last frame (3 and 4); state 1 is final before it, which is ignored"""
    return hand([(0, INF), (1, 0.5), (1, INF), (2, 0.125), (2, 0.375)],
                [(0, 5, 1, 0.5, 1.0, 1), (0, 6, 2, 0.25, 1.5, 2), (1, 7, 3, 0.75, 0.5, 3), (2, 8, 0, 0.5, 0.25, 3), (2, 9, 4, 0.125, 0.75, 4),
                 (1, 10, 0, 0.25, 0.25, 4)])


def bad_cost(x):
    """the arc 1 -> 3 costs x (+inf or NaN): every candidate through it is dropped"""
    return hand([(0, INF), (1, INF), (1, INF), (2, 0.25)],
                [(0, 5, 1, 0.5, 0.5, 1), (0, 6, 2, 1.0, 0.5, 2), (1, 7, 3, x, 0.25, 3), (2, 8, 4, 0.5, 0.25, 3)])


def dead_end_unreachable():
    """state 1 cannot be reached, state 3 leads nowhere"""
    return hand([(0, INF), (0, INF), (1, INF), (1, INF), (2, 0.5)],
                [(0, 5, 1, 0.5, 1.0, 2), (0, 6, 2, 0.25, 1.0, 3), (1, 7, 3, 0.125, 2.0, 2), (2, 8, 4, 0.75, 0.5, 4)])


def sausage(segments=7, width=3, seed=11, equal=False):
    """`segments` segments of `width` parallel arcs each: width ** segments paths"""
    rng = np.random.default_rng(seed)
    states = [(f, INF) for f in range(segments)] + [(segments, 0.5)]
    arcs = []
    for f in range(segments):
        for k in range(width):
            g, a = (0.5, 1.0) if equal else (float(rng.uniform(0.0, 3.0)), float(rng.uniform(0.0, 6.0)))
            arcs.append((f, 10 + k, 1 + k, g, a, f + 1))
    return hand(states, arcs)


def hand_cases():
    """name -> (lattice, expected status at the pair (1, 1))"""
    S = ref.SUCCEEDED
    c = {}
    c["one_state"] = (hand([(0, 0.75)], []), S)
    c["chain3"] = (hand([(0, INF), (1, INF), (2, INF), (3, 0.5)], [(0, 5, 1, 0.5, 1.0, 1), (1, 6, 2, 0.25, 2.0, 2), (2, 7, 3, 0.125, 3.0, 3)]), S)
    c["diamond"] = (diamond(), S)
    c["tie_in_arcs"] = (tie_in_arcs(), S)
    c["tie_ranks"] = (tie_ranks(), S)
    c["negative_costs"] = (negative(), S)
    c["word_on_ilabel_0"] = (hand([(0, INF), (0, INF), (1, 0.25)], [(0, 0, 2, 0.3, 0.0, 1), (1, 4, 1, 0.5, 1.0, 2), (0, 5, 3, 0.75, 0.5, 2)]), S)
    c["two_finals_and_an_early_one"] = (finals(), S)
    c["inf_arc_into_final"] = (bad_cost(INF), S)
    c["nan_cost"] = (bad_cost(NAN), S)
    c["only_path_is_inf"] = (hand([(0, INF), (1, 0.5)], [(0, 5, 1, INF, 1.0, 1)]), ref.NO_PATH)
    c["dead_end_unreachable"] = (dead_end_unreachable(), S)
    c["start_not_first"] = (hand([(0, INF), (0, INF), (1, INF), (2, 0.5)], [(0, 5, 1, 0.5, 1.0, 2), (1, 6, 2, 0.25, 2.0, 2), (2, 7, 3, 0.125, 3.0, 3)], start=1), S)
    c["empty"] = (hand([], []), ref.NO_PATH)
    c["no_final"] = (hand([(0, INF), (1, INF)], [(0, 5, 1, 0.5, 1.0, 1)]), ref.NO_PATH)
    c["arc_to_lower_state"] = (hand([(0, INF), (0, INF), (1, 0.0)], [(0, 0, 1, 0.5, 0.0, 1), (1, 0, 0, 0.25, 0.0, 0), (1, 4, 2, 0.75, 2.0, 2)]), ref.EPS_LOOP)
    c["self_loop"] = (hand([(0, INF), (1, 0.0)], [(0, 0, 0, 0.5, 0.0, 0), (0, 4, 2, 0.75, 2.0, 1)]), ref.EPS_LOOP)
    c["fan70_into_one_state"] = (fan(70, lambda i: 1 + i), S)
    c["sausage7x3"] = (sausage(), S)
    c["sausage7x3_all_equal"] = (sausage(equal=True), S)
    return c


def random_cases(n=200, seed=2026):
    rng = np.random.default_rng(seed)
    return [random_lattice(rng) for _ in range(n)]


def all_cases():
    """[(name, lattice, expected status at (1, 1) or None)]"""
    return [(name,) + c for name, c in sorted(hand_cases().items())] + [("random%d" % i, lat, None) for i, lat in enumerate(random_cases())]
