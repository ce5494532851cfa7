"""Hand-made and seeded random cases for lattice-determinize-pruned: the smallest shapes at which each clause of
the rule can go wrong.  A case is (lattice, graph_scale, acoustic_scale, beam, delta, state_factor, expected status or None); lattices
are the dicts of arrays the other lattice tests use and pass khg_lattices_validate: states ordered by frame, an emitting arc goes one
frame on, an arc with ilabel 0 stays in its frame."""
import numpy as np

import lattice_det_ref as ref
from lattice_lm_cases import diamond, fan, hand, random_lattice

INF = np.inf
DELTA = 1.0 / 1024
BIG = 1e30
SCALES = [(1.0, 1.0), (1.0, 0.1), (0.5, 1.7)]
BEAMS = [0.0, 2.0, BIG]


def two_alignments(tie=False):
    """the word sequence (1) along two alignments; the second is cheaper (or, tie: they cost the same, bit for bit)"""
    g = 0.5 if tie else 0.25
    return hand([(0, INF), (1, INF), (1, INF), (2, 0.5)],
                [(0, 5, 1, 0.5, 1.0, 1), (0, 6, 1, g, 1.0, 2), (1, 7, 0, 0.5, 0.75, 3), (2, 8, 0, 0.5, 0.75, 3)])


def dominated(direct=5.0, through=0.5):
    """word 1 enters states 1 and 2; an arc without a word goes 1 -> 2.  When it is the cheaper way into 2, state 2 is dominated and the
    word arc 0 -> 2 must vanish: kept, the sequence (1) would have two paths"""
    return hand([(0, INF), (1, INF), (1, INF), (2, 0.0)],
                [(0, 5, 1, 1.0, 1.0, 1), (0, 6, 1, direct, 1.0, 2), (1, 0, 0, through, 0.0, 2), (1, 7, 0, 0.25, 2.0, 3), (2, 8, 0, 0.5, 0.5, 3)])


def two_finals():
    """two final states of the last frame in one closure: only the better one stays final"""
    return hand([(0, INF), (1, 0.5), (1, 0.125)], [(0, 5, 1, 1.0, 1.0, 1), (1, 0, 0, 0.25, 0.0, 2)])


def dead_ends():
    """state 1 cannot be reached, state 3 is a dead end, state 4 is final but not of the last frame"""
    return hand([(0, INF), (0, INF), (1, INF), (1, INF), (1, 0.25), (2, 0.5)],
                [(0, 5, 1, 0.5, 1.0, 2), (1, 6, 2, 0.25, 2.0, 2), (0, 9, 2, 0.25, 0.5, 3), (0, 4, 3, 0.1, 0.1, 4), (2, 7, 3, 0.125, 3.0, 5)])


def sausage(segments=7, words=3, seed=11):
    """start -> B0 without a label; per segment every word is a chain of two states from B, then the join states A -> B.  58 states for
    7 segments of 3 words, 3^7 word sequences; one determinized state per (segment, word) and the first: 22, of 86 elements"""
    rng = np.random.default_rng(seed)
    states, arcs = [(0, INF), (0, INF)], [(0, 0, 0, 0.125, 0.0, 1)]
    b, f = 1, 0
    for k in range(segments):
        n = len(states)
        a_state, b_state = n + 2 * words, n + 2 * words + 1
        for w in range(words):
            m1, m2 = n + 2 * w, n + 2 * w + 1
            arcs.append((b, 10 + w, 1 + w, float(rng.uniform(0.0, 3.0)), float(rng.uniform(0.0, 5.0)), m1))
            arcs.append((m1, 20 + w, 0, float(rng.uniform(0.0, 1.0)), float(rng.uniform(0.0, 5.0)), m2))
            arcs.append((m2, 30 + w, 0, float(rng.uniform(0.0, 1.0)), float(rng.uniform(0.0, 5.0)), a_state))
        for w in range(words):
            states += [(f + 1, INF), (f + 2, INF)]
        states += [(f + 3, INF), (f + 3, 0.75 if k + 1 == segments else INF)]
        arcs.append((a_state, 0, 0, 0.25, 0.0, b_state))
        b, f = b_state, f + 3
    # states of one frame must lie together: order them by frame, stably
    order = sorted(range(len(states)), key=lambda s: states[s][0])
    new = {s: i for i, s in enumerate(order)}
    return hand([states[s] for s in order], [(new[a[0]],) + a[1:5] + (new[a[5]],) for a in arcs], start=new[0])


def near_pair(eps=2.0 ** -11):
    """the histories (1) and (2) reach the subset {3, 4} under word 3 with relative costs that differ by eps: one determinized state
    when delta >= eps, two when delta = 0"""
    return hand([(0, INF), (1, INF), (1, INF), (2, INF), (2, INF), (3, 0.5)],
                [(0, 5, 1, 0.5, 1.0, 1), (0, 6, 2, 0.75, 1.5, 2), (1, 7, 3, 1.0, 1.0, 3), (1, 8, 3, 2.0, 1.0, 4), (2, 9, 3, 1.0, 1.0, 3),
                 (2, 10, 3, 2.0 + eps, 1.0, 4), (3, 11, 4, 0.25, 0.5, 5), (4, 12, 5, 0.125, 0.25, 5)])


def negative_best_dominated():
    """word 1 enters 1 at 3.0 and 2 at 1.0 (the best); the arc 1 -> 2 costs -2.5, so the best initial state is dominated"""
    return hand([(0, INF), (1, INF), (1, INF), (2, 0.0)],
                [(0, 5, 1, 3.0, 0.0, 1), (0, 6, 1, 1.0, 0.0, 2), (1, 0, 0, -2.5, 0.0, 2), (1, 7, 0, 0.25, 2.0, 3), (2, 8, 0, 0.5, 0.5, 3)])


def hand_cases():
    """name -> (lattice, gs, as, beam, delta, state_factor, expected status)"""
    S = ref.SUCCEEDED
    c = {}

    def add(name, lat, gs=1.0, as_=1.0, beam=BIG, delta=DELTA, sf=8, expect=S):
        c[name] = (lat, gs, as_, beam, delta, sf, expect)

    add("one_state", hand([(0, 0.75)], []))
    add("chain3", hand([(0, INF), (1, INF), (2, INF), (3, 0.5)], [(0, 5, 1, 0.5, 1.0, 1), (1, 6, 2, 0.25, 2.0, 2), (2, 7, 3, 0.125, 3.0, 3)]))
    add("two_words_rejoin", diamond())
    add("two_alignments", two_alignments())
    add("two_alignments_scaled", two_alignments(), gs=0.5, as_=1.7)
    add("exact_tie", two_alignments(tie=True))
    add("word_on_ilabel_0", hand([(0, INF), (0, INF), (1, 0.25)], [(0, 0, 2, 0.3, 0.0, 1), (1, 4, 1, 0.5, 1.0, 2), (0, 5, 3, 0.75, 0.5, 2)]))
    add("dominated_initial", dominated())
    add("initial_not_dominated", dominated(direct=1.25, through=0.5))
    add("negative_best_dominated", negative_best_dominated())
    add("two_finals", two_finals())
    add("dead_ends_unreachable", dead_ends())
    add("arc_to_lower_state", hand([(0, INF), (0, INF), (1, 0.0)], [(0, 0, 1, 0.5, 0.0, 1), (1, 0, 0, 0.25, 0.0, 0), (1, 4, 2, 0.75, 2.0, 2)]), expect=ref.EPS_LOOP)
    add("self_loop", hand([(0, INF), (1, 0.0)], [(0, 0, 0, 0.5, 0.0, 0), (0, 4, 2, 0.75, 2.0, 1)]), expect=ref.EPS_LOOP)
    add("empty", hand([], []), expect=ref.NO_PATH)
    add("no_final", hand([(0, INF), (1, INF)], [(0, 5, 1, 0.5, 1.0, 1)]), expect=ref.NO_PATH)
    add("state_factor_1", diamond(), sf=1, expect=ref.SCRATCH)
    add("state_factor_2", diamond(), sf=2)
    add("fan70_words", fan(70, lambda i: 1 + i))
    add("fan70_into_one_state", fan(70, lambda i: 1))
    add("fan70_two_words", fan(70, lambda i: 1 + i % 2), beam=2.0)
    add("sausage", sausage())
    add("sausage_beam_2", sausage(), beam=2.0)
    add("near_pair_merges", near_pair(), delta=DELTA)
    add("near_pair_apart", near_pair(), delta=0.0)
    add("beam_0", diamond(), beam=0.0)
    return c


def random_cases(n=200, seed=2025):
    """[(lattice, gs, as, beam, delta, state_factor, None)]: lattice_lm_cases.random_lattice, every (scale pair, beam) in turn"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        gs, as_ = SCALES[i % 3]
        out.append((random_lattice(rng), gs, as_, BEAMS[(i // 3) % 3], DELTA if i % 7 else 0.0, 8 if i % 5 else 2, None))
    return out


def all_cases():
    return [(name,) + c for name, c in sorted(hand_cases().items())] + [("random%d" % i,) + c for i, c in enumerate(random_cases())]
