"""Hand-made and seeded random cases for scoring lattices: the smallest shapes at which each part of the rule
can go wrong.  A case is (lattice, reference, expected status); lattices are the dicts of arrays the other lattice tests use.  Every
lattice passes khg_lattices_validate: states ordered by frame, an emitting arc goes one frame on, an epsilon arc stays in its frame."""
import numpy as np

import lattice_score_ref as ref
from lattice_lm_cases import diamond, fan, hand

INF = np.inf
S, NO_PATH, EPS_LOOP = ref.SUCCEEDED, ref.NO_PATH, ref.EPS_LOOP


def chain_lattice(words):
    """one path; every arc emits"""
    n = len(words)
    return hand([(f, INF) for f in range(n)] + [(n, 0.25)], [(i, 10 + i, w, 0.5, 1.0, i + 1) for i, w in enumerate(words)])


def layered(rng, per, n_words, p_word=0.75, p_eps=0.25, p_final=0.1):
    """frames of per[f] states; every state has 1 to 3 emitting arcs into the next frame, every state of a frame after the first at least
    one in-arc, now and then an epsilon arc to a higher state of the same frame; the last frame's states are final (most of them)"""
    T = len(per) - 1
    first = np.concatenate([[0], np.cumsum(per)])
    states, arcs = [], []
    for f, n in enumerate(per):
        for k in range(n):
            s = int(first[f]) + k
            states.append((f, float(rng.uniform(0.0, 2.0)) if (f == T and (k == 0 or rng.random() < 0.7)) or rng.random() < p_final else INF))
            if f < T:
                for _ in range(int(rng.integers(1, 4))):
                    w = int(rng.integers(1, n_words + 1)) if rng.random() < p_word else 0
                    arcs.append((s, int(rng.integers(1, 30)), w, float(rng.uniform(-1.0, 5.0)), float(rng.uniform(0.0, 9.0)), int(first[f + 1] + rng.integers(0, per[f + 1]))))
            if k + 1 < n and rng.random() < p_eps:
                arcs.append((s, 0, int(rng.integers(0, n_words + 1)), float(rng.uniform(0.0, 1.0)), 0.0, s + 1 + int(rng.integers(0, n - k - 1))))
    for f in range(1, T + 1):          # no state without an in-arc
        have = {a[5] for a in arcs}
        for k in range(per[f]):
            d = int(first[f]) + k
            if d not in have:
                w = int(rng.integers(1, n_words + 1)) if rng.random() < p_word else 0
                arcs.append((int(first[f - 1] + rng.integers(0, per[f - 1])), int(rng.integers(1, 30)), w, float(rng.uniform(-1.0, 5.0)), float(rng.uniform(0.0, 9.0)), d))
    return hand(states, arcs)


def walk(rng, lat):
    """the words of a random path from the start until a state without arcs"""
    ab, nxt, ol = lat["arc_begin"], lat["nextstate"], lat["olabel"]
    s, words = int(lat["start"]), []
    while ab[s + 1] > ab[s]:
        a = int(rng.integers(ab[s], ab[s + 1]))
        if ol[a] != 0:
            words.append(int(ol[a]))
        s = int(nxt[a])
    return words


def perturbed(rng, words, n_words, p=0.25):
    out = []
    for w in words:
        r = rng.random()
        if r < p / 3:
            continue
        out.append(int(rng.integers(1, n_words + 1)) if r < 2 * p / 3 else w)
        if r > 1 - p / 3:
            out.append(int(rng.integers(1, n_words + 1)))
    return out


def reference_of_length(rng, lat, n_words, R):
    """a walk's words, perturbed, repeated or cut to exactly R words"""
    w = perturbed(rng, walk(rng, lat), n_words) or [1]
    return (w * (R // len(w) + 1))[:R]


def hand_cases():
    """name -> (lattice, reference, expected status)"""
    c = {}
    rng = np.random.default_rng(4321)
    c["empty"] = (hand([], []), [1, 2], NO_PATH)
    c["empty_r0"] = (hand([], []), [], NO_PATH)
    c["one_state"] = (hand([(0, 0.75)], []), [1, 2], S)
    c["one_state_r0"] = (hand([(0, 0.75)], []), [], S)
    c["no_word"] = (hand([(0, INF), (1, INF), (1, INF), (2, 0.0)], [(0, 3, 0, 0.5, 1.0, 1), (1, 0, 0, 0.25, 0.0, 2), (2, 4, 0, 0.75, 2.0, 3), (0, 5, 0, 0.1, 0.2, 2)]), [1], S)
    c["r0"] = (diamond(), [], S)
    c["single_path_exact"] = (chain_lattice([1, 2, 3]), [1, 2, 3], S)
    c["single_path_sub_del"] = (chain_lattice([1, 2, 3]), [1, 4, 3, 5], S)
    c["single_path_ins"] = (chain_lattice([1, 2, 3, 4]), [1, 4], S)
    # two paths, one error each, different words: the lower arc wins
    c["two_paths_equal_errors"] = (hand([(0, INF), (1, 0.5), (1, 0.25)], [(0, 7, 1, 0.5, 1.0, 1), (0, 8, 2, 0.25, 2.0, 2)]), [3], S)
    c["two_paths_rejoin_equal_errors"] = (diamond(), [4, 3, 2], S)
    # "1 2" against "2 1": two substitutions, or an insertion and a deletion around a match
    c["tie_diag_ins_del"] = (chain_lattice([1, 2]), [2, 1], S)
    c["tie_one_word"] = (chain_lattice([5]), [7], S)
    c["tie_repeats"] = (chain_lattice([1, 1, 2, 1]), [1, 2, 1, 1], S)
    c["unreachable_state"] = (hand([(0, INF), (0, INF), (1, INF), (2, 0.5)], [(0, 5, 1, 0.5, 1.0, 2), (1, 6, 2, 0.25, 2.0, 2), (2, 7, 3, 0.125, 3.0, 3)]), [2, 3], S)
    c["start_not_first"] = (hand([(0, INF), (0, INF), (1, INF), (2, 0.5)], [(0, 5, 1, 0.5, 1.0, 2), (1, 6, 2, 0.25, 2.0, 2), (2, 7, 3, 0.125, 3.0, 3)], start=1), [1, 3], S)
    # the state that matches the reference is on the last frame but not final
    c["last_frame_not_final"] = (hand([(0, INF), (1, INF), (1, 0.5)], [(0, 7, 1, 0.5, 1.0, 1), (0, 8, 2, 0.25, 2.0, 2)]), [1], S)
    c["no_final_reachable"] = (hand([(0, INF), (0, INF), (1, INF), (1, 0.5)], [(0, 7, 1, 0.5, 1.0, 2), (1, 8, 2, 0.25, 2.0, 3)]), [1], NO_PATH)
    c["final_before_last_frame"] = (hand([(0, INF), (1, 0.0), (2, 0.5)], [(0, 7, 1, 0.5, 1.0, 1), (1, 8, 2, 0.25, 2.0, 2)]), [1], S)
    c["several_finals_equal_errors"] = (hand([(0, INF), (1, 0.5), (1, 0.25), (1, 0.125)], [(0, 7, 3, 0.5, 1.0, 1), (0, 8, 1, 0.25, 2.0, 2), (0, 9, 2, 0.25, 2.0, 3)]), [4], S)
    # a chain of epsilon arcs inside frame 1, two of them with words
    c["epsilon_chain"] = (hand([(0, INF), (1, INF), (1, INF), (1, INF), (1, INF), (2, 0.0)],
                               [(0, 3, 1, 0.5, 1.0, 1), (1, 0, 2, 0.25, 0.0, 2), (2, 0, 0, 0.25, 0.0, 3), (3, 0, 3, 0.25, 0.0, 4), (1, 0, 0, 0.1, 0.0, 4),
                                (4, 4, 4, 0.75, 2.0, 5), (2, 5, 4, 0.75, 2.0, 5)]), [1, 2, 3, 4], S)
    c["hub_70_in_arcs"] = (fan(70, lambda i: 1 + i), [35, 1], S)
    c["hub_70_few_words"] = (fan(70, lambda i: 1 + i % 3), [3, 2], S)
    c["self_loop"] = (hand([(0, INF), (1, 0.0)], [(0, 0, 0, 0.5, 0.0, 0), (0, 4, 2, 0.75, 2.0, 1)]), [2], EPS_LOOP)
    c["arc_to_lower_state"] = (hand([(0, INF), (0, INF), (1, 0.0)], [(0, 0, 1, 0.5, 0.0, 1), (1, 0, 0, 0.25, 0.0, 0), (1, 4, 2, 0.75, 2.0, 2)]), [1, 2], EPS_LOOP)
    c["words_the_reference_lacks"] = (diamond(), [9, 9], S)
    c["reference_longer_than_any_path"] = (diamond(), [1, 3, 2, 1, 3, 2, 1, 3, 2], S)
    # the wave-segment edges: R + 1 at 63, 64, 65 and 130
    for W in (63, 64, 65, 130):
        lat = layered(rng, [1] + [int(rng.integers(1, 4)) for _ in range(W)], 4, p_word=0.9)
        c["segment_edge_w%d" % W] = (lat, reference_of_length(rng, lat, 4, W - 1), S)
    c["chain_against_long_reference_w65"] = (chain_lattice([1, 2, 3]), ([3, 1, 2, 2] * 16), S)
    # a frame of 200 states at R = 130: its two-frame ring of 2 * 200 * 131 * 4 bytes exceeds the 160 KiB of LDS
    lat = layered(rng, [1, 3, 200, 4, 200, 2, 1], 5, p_word=0.9, p_eps=0.05)
    c["frame_of_200_states_w131"] = (lat, reference_of_length(rng, lat, 5, 130), S)
    return c


def random_cases(n=200, seed=2025):
    """[(lattice, reference)]: seeded, top-sorted, 2 to 60 states, 2 to 5 words, so that ties are common; about half the references are a
    path's words (perturbed), the others random"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        n_words = int(rng.integers(2, 6))
        T = int(rng.integers(1, 12))
        per = [1] + [int(rng.integers(1, 7)) for _ in range(T)]
        if not 2 <= sum(per) <= 60:
            continue
        lat = layered(rng, per, n_words, p_word=float(rng.choice([0.5, 0.75, 1.0])), p_final=0.05)
        if rng.random() < 0.5:
            r = perturbed(rng, walk(rng, lat), n_words, p=float(rng.choice([0.0, 0.25, 0.6])))
        else:
            r = rng.integers(1, n_words + 1, size=int(rng.integers(0, 10))).tolist()
        out.append((lat, [int(w) for w in r]))
    return out
