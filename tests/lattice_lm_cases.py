"""Hand-made and seeded random cases for lattice-lmrescore: the smallest shapes at which each part of the rule
can go wrong.  A case is (lattice, lm, scale, hist_factor, expected status); lattices are the dicts of arrays the other lattice tests use,
LMs the dicts of NgramLm.to_arrays().  Every lattice passes khg_lattices_validate: states ordered by frame, an emitting arc goes one
frame on, an epsilon arc stays in its frame."""
import numpy as np

import lattice_lm_ref as ref

F = np.float32
INF = np.inf
BOS = 0


def hand(states, arcs, start=0):
    """states: [(frame, final_cost)], arcs: [(src, ilabel, olabel, graph, acoustic, dst)] in any order -> the dict of arrays"""
    arcs = sorted(arcs, key=lambda a: a[0])
    N = len(states)
    ab = np.zeros(N + 1, np.int32)
    for a in arcs:
        ab[a[0] + 1] += 1
    return {"frame": np.array([s[0] for s in states], np.int32), "graph_state": np.arange(100, 100 + N, dtype=np.int32),
            "tot_cost": np.arange(N, dtype=np.float32) * F(0.5), "extra_cost": np.arange(N, dtype=np.float32) * F(0.25),
            "final_cost": np.array([s[1] for s in states], np.float32), "arc_begin": np.cumsum(ab).astype(np.int32),
            "ilabel": np.array([a[1] for a in arcs], np.int32), "olabel": np.array([a[2] for a in arcs], np.int32),
            "graph_cost": np.array([a[3] for a in arcs], np.float32), "acoustic_cost": np.array([a[4] for a in arcs], np.float32),
            "nextstate": np.array([a[5] for a in arcs], np.int32), "start": start if N else -1}


def build_lm(hists, arcs, backoff_cost, final_cost, start=(BOS,)):
    """hists: the history tuples besides () (<s> is 0 inside a tuple); arcs: {history: {word: cost}}; -> the automaton's arrays.  States
    are numbered by (length, tuple); an arc goes to the longest suffix of history + word that is a state, a state backs off to its
    longest proper suffix that is one."""
    hs = [()] + sorted(set(hists), key=lambda g: (len(g), g))
    idx = {h: i for i, h in enumerate(hs)}

    def suffix(g):
        while g not in idx:
            g = g[1:]
        return idx[g]

    order = max(len(h) for h in hs) + 1
    lm = {"backoff": np.array([-1] + [suffix(h[1:]) for h in hs[1:]], np.int32),
          "backoff_cost": np.array([backoff_cost.get(h, 0.0) for h in hs], np.float32),
          "final_cost": np.array([final_cost.get(h, 0.0) for h in hs], np.float32), "start": idx.get(start, 0)}
    ab, word, cost, nxt = [0], [], [], []
    for h in hs:
        for w, c in sorted(arcs.get(h, {}).items()):
            g = h + (w,)
            word.append(w); cost.append(c); nxt.append(suffix(g if len(g) < order else g[1:]))
        ab.append(len(word))
    lm.update(arc_begin=np.array(ab, np.int32), word=np.array(word, np.int32), cost=np.array(cost, np.float32), next=np.array(nxt, np.int32))
    return lm


def unigram(n_words, seed=1):
    rng = np.random.default_rng(seed)
    return build_lm([], {(): {w: float(rng.uniform(0.2, 4.0)) for w in range(1, n_words + 1)}}, {}, {(): 0.0}, start=())


def bigram(n_words, seed=2, states=None, negative=False):
    """every word listed in the empty history; the words in `states` (default: all) are histories of their own, listing about half the words"""
    rng = np.random.default_rng(seed)
    lo = -3.0 if negative else 0.2
    states = list(range(1, n_words + 1)) if states is None else states
    hists = [(BOS,)] + [(w,) for w in states]
    arcs = {(): {w: float(rng.uniform(lo, 4.0)) for w in range(1, n_words + 1)}}
    for h in hists:
        arcs[h] = {w: float(rng.uniform(lo, 4.0)) for w in range(1, n_words + 1) if rng.random() < 0.5}
    return build_lm(hists, arcs, {h: float(rng.uniform(0.1, 2.0)) for h in hists}, {h: float(rng.uniform(lo, 3.0)) for h in [()] + hists})


def trigram_chain():
    """three words; (1, 3) and (3,) both lack word 2: advance((1, 3), 2) backs off twice"""
    hists = [(BOS,), (1,), (2,), (3,), (BOS, 1), (1, 3), (2, 3)]
    arcs = {(): {1: 1.1, 2: 2.3, 3: 0.7}, (BOS,): {1: 0.9, 2: 1.3}, (1,): {3: 0.4}, (2,): {3: 0.6, 1: 1.9}, (3,): {1: 2.2},
            (BOS, 1): {3: 0.35}, (1, 3): {1: 0.8}, (2, 3): {2: 0.15}}
    bo = {(BOS,): 0.3, (1,): 0.55, (2,): 0.21, (3,): 0.77, (BOS, 1): 0.13, (1, 3): 0.19, (2, 3): 0.41}
    fin = {(): 3.3, (BOS,): 5.1, (1,): 2.7, (2,): 1.9, (3,): 0.8, (BOS, 1): 2.9, (1, 3): 0.66, (2, 3): 0.52}
    return build_lm(hists, arcs, bo, fin)


def random_lm(rng, n_words=5):
    """a random trigram: every word in the empty history, about half of them elsewhere, costs of both signs"""
    hists = [(BOS,)] + [(w,) for w in range(1, n_words + 1) if rng.random() < 0.8]
    hists += [(a, b) for a in range(0, n_words + 1) for b in range(1, n_words + 1) if rng.random() < 0.35]
    arcs = {(): {w: float(rng.uniform(-1.0, 6.0)) for w in range(1, n_words + 1)}}
    for h in hists:
        arcs[h] = {w: float(rng.uniform(-1.0, 6.0)) for w in range(1, n_words + 1) if rng.random() < 0.5}
    return build_lm(hists, arcs, {h: float(rng.uniform(0.0, 2.0)) for h in hists}, {h: float(rng.uniform(-1.0, 4.0)) for h in [()] + hists})


def diamond(last_word=2):
    """two different words rejoin (through arcs without a word), a third follows, then `last_word`"""
    return hand([(0, INF), (1, INF), (1, INF), (2, INF), (3, INF), (4, INF), (5, 0.25)],
                [(0, 11, 1, 0.5, 1.5, 1), (0, 12, 2, 0.3, 2.5, 2), (1, 13, 0, 0.1, 0.5, 3), (2, 14, 0, 0.2, 0.75, 3), (3, 17, 3, 0.6, 0.125, 4),
                 (4, 15, last_word, 0.7, 1.25, 5), (5, 16, 0, 0.05, 0.3, 6)])


def fan(n, words_of):
    """start -> n states (word words_of(i)) -> one state through arcs without a word -> the final state"""
    states = [(0, INF)] + [(1, INF)] * n + [(2, INF), (3, 1.5)]
    arcs = [(0, 20 + i, words_of(i), 0.01 * i, 0.5 + 0.125 * i, 1 + i) for i in range(n)]
    arcs += [(1 + i, 200 + i, 0, 0.3 + 0.02 * i, 1.0, n + 1) for i in range(n)]
    arcs += [(n + 1, 7, 1, 0.9, 2.0, n + 2)]
    return hand(states, arcs)


def hand_cases():
    """name -> (lattice, lm, scale, hist_factor, expected status)"""
    S = ref.SUCCEEDED
    bi3, uni3, tri = bigram(3), unigram(3), trigram_chain()
    c = {}
    c["one_state"] = (hand([(0, 0.75)], []), bi3, 1.0, 8, S)
    c["chain3"] = (hand([(0, INF), (1, INF), (2, INF), (3, 0.5)], [(0, 5, 1, 0.5, 1.0, 1), (1, 6, 2, 0.25, 2.0, 2), (2, 7, 3, 0.125, 3.0, 3)]), bi3, 1.0, 8, S)
    c["diamond_bigram"] = (diamond(), bi3, 1.0, 8, S)
    c["diamond_unigram"] = (diamond(), uni3, 1.0, 8, S)
    c["diamond_trigram_backoff2"] = (diamond(), tri, 1.0, 8, S)
    c["no_words"] = (hand([(0, INF), (1, INF), (1, INF), (2, 0.0)], [(0, 3, 0, 0.5, 1.0, 1), (1, 0, 0, 0.25, 0.0, 2), (2, 4, 0, 0.75, 2.0, 3), (0, 5, 0, 0.1, 0.2, 2)]),
                     bi3, 1.0, 8, S)
    c["fan70_distinct"] = (fan(70, lambda i: 1 + i), bigram(70, seed=5), 1.0, 8, S)
    c["fan70_three_histories"] = (fan(70, lambda i: 1 + i), bigram(70, seed=6, states=[1, 2]), 1.0, 8, S)
    # state 1 cannot be reached from the start: dropped, the rest renumbered
    c["unreachable"] = (hand([(0, INF), (0, INF), (1, INF), (2, 0.5)], [(0, 5, 1, 0.5, 1.0, 2), (1, 6, 2, 0.25, 2.0, 2), (2, 7, 3, 0.125, 3.0, 3)]), bi3, 1.0, 8, S)
    c["start_not_first"] = (hand([(0, INF), (0, INF), (1, INF), (2, 0.5)], [(0, 5, 1, 0.5, 1.0, 2), (1, 6, 2, 0.25, 2.0, 2), (2, 7, 3, 0.125, 3.0, 3)], start=1), bi3, 1.0, 8, S)
    c["oov_reachable"] = (diamond(last_word=9), bi3, 1.0, 8, ref.LM_OOV)
    c["oov_unreachable"] = (hand([(0, INF), (0, INF), (1, INF), (2, 0.5)], [(0, 5, 1, 0.5, 1.0, 2), (1, 6, 9, 0.25, 2.0, 2), (2, 7, 3, 0.125, 3.0, 3)]), bi3, 1.0, 8, S)
    c["diamond_hist_factor_1"] = (diamond(), bi3, 1.0, 1, ref.SCRATCH)
    c["diamond_hist_factor_2"] = (diamond(), bi3, 1.0, 2, S)
    c["arc_to_lower_state"] = (hand([(0, INF), (0, INF), (1, 0.0)], [(0, 0, 1, 0.5, 0.0, 1), (1, 0, 0, 0.25, 0.0, 0), (1, 4, 2, 0.75, 2.0, 2)]), bi3, 1.0, 8, ref.EPS_LOOP)
    c["self_loop"] = (hand([(0, INF), (1, 0.0)], [(0, 0, 0, 0.5, 0.0, 0), (0, 4, 2, 0.75, 2.0, 1)]), bi3, 1.0, 8, ref.EPS_LOOP)
    c["empty"] = (hand([], []), bi3, 1.0, 8, ref.NO_PATH)
    c["scale_0"] = (diamond(), tri, 0.0, 8, S)
    c["scale_minus_1"] = (diamond(), tri, -1.0, 8, S)
    c["scale_half"] = (diamond(), bi3, 0.5, 8, S)
    c["negative_costs"] = (diamond(), bigram(3, seed=9, negative=True), 2.0, 8, S)
    return c


def random_lattice(rng, n_words=5):
    """a top-sorted lattice of at most 40 states: 2 to 8 frames of 1 to 4 states, 1 to 3 arcs per state to the next frame (a word on
    about two thirds of them) and now and then an epsilon arc to a higher state of the same frame; some states are dead ends or cannot
    be reached"""
    T = int(rng.integers(2, 9))
    per = [1] + [int(rng.integers(1, 5)) for _ in range(T)]
    first = np.concatenate([[0], np.cumsum(per)])
    states, arcs = [], []
    for f, n in enumerate(per):
        for k in range(n):
            s = int(first[f]) + k
            states.append((f, float(rng.uniform(-0.5, 2.0)) if f == T or rng.random() < 0.1 else INF))
            if f < T:
                for _ in range(int(rng.integers(0 if f else 1, 4))):
                    w = int(rng.integers(1, n_words + 1)) if rng.random() < 0.67 else 0
                    arcs.append((s, int(rng.integers(1, 30)), w, float(rng.uniform(-1.0, 5.0)), float(rng.uniform(0.0, 9.0)), int(first[f + 1] + rng.integers(0, per[f + 1]))))
            if k + 1 < n and rng.random() < 0.25:
                arcs.append((s, 0, int(rng.integers(0, n_words + 1)), float(rng.uniform(0.0, 1.0)), 0.0, s + 1 + int(rng.integers(0, n - k - 1))))
    return hand(states, arcs)


def random_cases(n=200, seed=2024):
    """[(lattice, lm, scale, hist_factor)]: seeded, top-sorted, five words, a random trigram each"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        out.append((random_lattice(rng), random_lm(rng), float(rng.choice([1.0, -1.0, 0.5, 2.0, 0.0])), int(rng.choice([8, 8, 8, 2, 1]))))
    return out
