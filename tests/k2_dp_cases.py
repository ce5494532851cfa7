"""Inputs built for every instantiation of the exact-DP aligner kernel (k2_viterbi_dp<KS, DEG, FAST, GMEM, SC>, chosen per batch in
csrc/khg_k2.hip), for tests/test_gpu_k2_dp_forms.py; tests/test_k2_dp_cases_cpu.py shows without a GPU that they have the properties
the GPU tests rest on.  Scores are random float32 matrices (UtteranceSet.upload_loglikes): K2 alone.

A batch holds one graph per size at which the kernel's indexing changes (wave trimming, state slot tid + nthr k, the three trace-back
widths and the general trace), each with the lengths at which the back-pointer words, the strip / block folds and the score
prefetch change; the batch's LARGEST graph, largest in-degree, epsilon arcs and score rows select the form, so the small graphs of
a batch run on trimmed waves of a block sized for the largest."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import k2_dp_ref as ref  # noqa: E402
from graphs import concat, hub_graph, permute_states, random_graph  # noqa: E402

NP = 24                                                   # pdfs; transition-ids 2 p + 1 and 2 p + 2 read pdf p
ID2PDF = np.concatenate([[0], np.repeat(np.arange(NP), 2)]).astype(np.int32)
SCALE = 0.7
SIZES = (2, 63, 64, 65, 128, 129, 256, 257)
LENGTHS = (7, 8, 9, 31, 32, 33, 63, 64, 65)
INT32_MAX = 2**31 - 1


def ltr_graph(rng, S, max_hop, same_row, grid=False, p_skip=None, wscale=1.0):
    """Left-to-right graph of S states: a self-loop on every state but the first, forward arcs, skip arcs of 2 .. max_hop states
    (in-degree <= max_hop + 1; the longest skip from every state, every skip from the even ones, the others from half of the odd
    ones: the shortest path has ceil((S - 1) / max_hop) arcs, and a state's in-arc slots are not all filled); labels by destination
    state (one score row per state) or at random; a word label on a fifth of the forward arcs; grid: weights on a 0.25 grid;
    p_skip: every skip arc with this probability instead; wscale: the range of the random weights."""
    def wt():
        return float(rng.integers(0, 4)) * 0.25 if grid else wscale * float(rng.random())
    row = rng.integers(0, NP, size=S)

    def tid(dst):
        p = int(row[dst]) if same_row else int(rng.integers(0, NP))
        return 2 * p + 1 + int(rng.integers(0, 2))
    arcs = []
    for s in range(S):
        if s > 0:
            arcs.append((s, tid(s), 0, wt(), s))
        for hop in range(1, max_hop + 1):
            if s + hop < S and (hop == 1 or (rng.random() < p_skip if p_skip is not None else hop == max_hop or s % 2 == 0 or rng.random() < 0.5)):
                word = int(rng.integers(1, 50)) if rng.random() < 0.2 else 0
                arcs.append((s, tid(s + hop), word, wt() + (0.0 if grid else 0.3 * (hop - 1)), s + hop))
    arc_off = np.zeros(S + 1, np.int64)
    for a in arcs:
        arc_off[a[0] + 1] += 1
    final = np.full(S, np.inf, np.float32)
    final[S - 1] = float(rng.integers(0, 4)) * 0.25 if grid else float(rng.random())
    return {"start": 0, "arc_off": np.cumsum(arc_off),
            "ilabel": np.array([a[1] for a in arcs], np.int32), "olabel": np.array([a[2] for a in arcs], np.int32),
            "weight": np.array([a[3] for a in arcs], np.float32), "nextstate": np.array([a[4] for a in arcs], np.int32), "final": final}


def shortest(S, max_hop):
    return max(1, -(-(S - 1) // max_hop))


def pdf_list(g):
    il = g["ilabel"]
    return np.unique(ID2PDF[il[il >= 1]]).astype(np.int32)


#          name          hop same_row k2_ks  extra sizes      plan (KS, DEG, FAST, SC)
FORMS = {
    "1_2_sc":        (1, True, 0, (), (1, 2, True, True)),
    "1_2":           (1, False, 0, (), (1, 2, True, False)),
    "1_3_sc":        (2, True, 0, (), (1, 3, True, True)),
    "1_3":           (2, False, 0, (), (1, 3, True, False)),
    "1_3_forced":    (1, True, 3, (), (1, 3, True, False)),       # the three-slot form on in-degree-2 graphs
    "1_6":           (5, False, 0, (), (1, 6, True, False)),
    "2_2_sc":        (1, True, 2, (127,), (2, 2, True, True)),
    "2_2":           (1, False, 2, (127,), (2, 2, True, False)),
    "2_3":           (2, False, 2, (127,), (2, 3, True, False)),
    "4_2_sc":        (1, True, 4, (255,), (4, 2, True, True)),
    "4_2":           (1, False, 4, (255,), (4, 2, True, False)),
    "4_3":           (2, False, 4, (255,), (4, 3, True, False)),
    "generic_deg7":  (6, False, 0, (), (1, 1, False, False)),
    "tie_1_3":       (2, False, 0, (), (1, 3, True, False)),      # weights and scores on a 0.25 grid
    "tie_1_6":       (5, False, 0, (), (1, 6, True, False)),
}
NATURAL = {"2_nat": ((1030, 1027, 1041), (2, 3, True, False)), "4_nat": ((2050, 2049, 2065), (4, 3, True, False))}
TIE_FREE = [n for n in FORMS if not n.startswith("tie")] + list(NATURAL)
SEEDS = {}                                                # name -> seed, where the default does not meet the conditions of the CPU tests


class Case:
    """name, option k2_ks, plan, graphs, T, mats (scores [rows, T] per utterance), pdfs, results of the restatement (ref), the
    three configurations (cfgs: keyword arguments of UtteranceSet.align / the oracle)"""

    def expected_nthr(self):
        S = max(len(g["final"]) for g in self.graphs)
        ks = self.k2_ks if self.k2_ks in (2, 4) else 1
        return min(1024, (-(-S // ks) + 63) // 64 * 64)


def _finish(c, rng, grid, score_range=3.0):
    c.pdfs = [pdf_list(g) for g in c.graphs]
    if grid:
        c.mats = [(-0.25 * rng.integers(0, 8, size=(len(p), t))).astype(np.float32) for p, t in zip(c.pdfs, c.T)]
    else:       # (a range of 3: the forced path of a chain traversed in its shortest time stays within 200 of every layer's minimum)
        c.mats = [(-score_range * rng.random((len(p), t))).astype(np.float32) for p, t in zip(c.pdfs, c.T)]
    c.scale = 1.0 if grid else SCALE                      # (a scale of 0.7 takes the products off the grid)
    c.ref = [ref.viterbi(g, ID2PDF, p, m, c.scale) for g, p, m in zip(c.graphs, c.pdfs, c.mats)]
    good = [r for r in c.ref if r.ok]
    c.median_beam = float(np.float32(np.median([r.required_beam for r in good])))
    c.median_live = int(np.median(np.concatenate([r.layer_cnt for r in good])))
    c.cfgs = [dict(beam=200.0), dict(beam=c.median_beam, min_active=0), dict(beam=c.median_beam, min_active=c.median_live)]
    c.frame_off = np.concatenate([[0], np.cumsum(c.T)]).astype(np.int64)
    return c


@functools.lru_cache(maxsize=None)
def form_case(name):
    hop, same_row, ks, extra, plan = FORMS[name]
    grid = name.startswith("tie")
    rng = np.random.default_rng(SEEDS.get(name, 1000 + sorted(FORMS).index(name)))
    c = Case()
    c.name, c.k2_ks, c.plan, c.hop = name, ks, plan, hop
    c.graphs, c.T = [], []
    for i, S in enumerate(sorted(SIZES + extra)):
        sp = shortest(S, hop)
        Ts = sorted({sp, sp + 1, sp + 6} | {t for t in LENGTHS if t >= sp})
        if S == 65:
            Ts = [sp - 1] + Ts                             # too short to reach the final state: ERROR
        for j, T in enumerate(Ts):
            g = ltr_graph(rng, S, hop, same_row, grid)
            if (i + j) % 2:
                g = permute_states(g, rng)                 # the start state is not 0 and falls in any slot
            c.graphs.append(g)
            c.T.append(T)
    return _finish(c, rng, grid)


@functools.lru_cache(maxsize=None)
def natural_case(name):
    """graphs just above 1024 / 2048 states (in-degree 3, score rows at random): KS = 2 / 4 selected by size alone; with 2-, 65- and
    130-state graphs beside them; T ~ 1.3 S.  Above 2048 states the DP's tables (two cost vectors, the in-arcs, five groups of
    back-pointer words for 1024 lanes x 4 states) fit the 160 KB of LDS only up to ~2.2 in-arcs per state -- beyond that the batch
    goes to the HBM-scratch form -- so those graphs get a skip arc from a sixth of their states only."""
    big, plan = NATURAL[name]
    rng = np.random.default_rng(SEEDS.get(name, 2000 + len(name) + big[0]))
    c = Case()
    c.name, c.k2_ks, c.plan, c.hop = name, 0, plan, 2
    c.graphs, c.T = [], []
    for i, S in enumerate(big + (2, 65, 130)):
        g = ltr_graph(rng, S, 2, False, p_skip=0.15 if big[0] > 2048 else None, wscale=0.25 if big[0] > 2048 else 1.0)
        c.graphs.append(permute_states(g, rng) if i % 2 == 0 else g)
        c.T.append(max(9, int(1.3 * S) + i))
    # (near-chains of 2000 states in 1.3 frames per state: weights and scores in [0, 0.25) keep the hurried best path within 200 of
    #  the states that linger on cheap self-loops)
    return _finish(c, rng, False, 0.25 if big[0] > 2048 else 3.0)


@functools.lru_cache(maxsize=None)
def generic_eps_case():
    """the generic form through epsilon-input arcs: the random graphs and the hub graphs (in-degree far above 6) of tests/graphs.py,
    weights and scores on a 0.25 grid -- ties everywhere"""
    rng = np.random.default_rng(4242)
    c = Case()
    c.name, c.k2_ks, c.plan, c.hop = "generic_eps", 0, (1, 1, False, False), 0
    c.graphs = [random_graph(rng, 2 * NP, n_main=n, p_eps=0.4, p_branch=0.5, p_long=0.4) for n in (1, 5, 9, 31, 62, 63, 64, 127, 128, 129)]
    c.graphs += [hub_graph(rng, 2 * NP, fan=int(f), tail=5, eps_ties=bool(i % 2)) for i, f in enumerate((9, 20, 31))]
    for g in c.graphs[::2]:
        g["weight"] = (np.round(g["weight"] * 4) / 4).astype(np.float32)
    c.graphs = [permute_states(g, rng) if i % 3 == 1 else g for i, g in enumerate(c.graphs)]
    c.T = [len(g["final"]) + int(rng.integers(0, 12)) for g in c.graphs]
    c.pdfs = [pdf_list(g) for g in c.graphs]
    c.mats = [((-0.25 * rng.integers(0, 24, size=(len(p), t))) if i % 2 == 0 else -8.0 * rng.random((len(p), t))).astype(np.float32)
              for i, (p, t) in enumerate(zip(c.pdfs, c.T))]
    c.scale = 1.0
    c.ref = [ref.viterbi(g, ID2PDF, p, m, c.scale) for g, p, m in zip(c.graphs, c.pdfs, c.mats)]
    c.cfgs = [dict(beam=200.0), dict(beam=6.0, min_active=0), dict(beam=6.0, min_active=4)]
    c.frame_off = np.concatenate([[0], np.cumsum(c.T)]).astype(np.int64)
    return c


def walk_graph(rng, S, back=None):
    """Out-degree 1: state s goes to s + 1, the last state -- the final one -- back to state `back` (None: nowhere, a plain chain).
    One path per length, so T frames end in the final state for T = S - 1 and every S - back frames after.  Word labels on a fifth of
    the arcs before the cycle: the aligner sizes an utterance's word buffer by the graph's labelled arcs, each taken once."""
    n = S - 1 + (back is not None)
    dst = np.concatenate([np.arange(1, S), [] if back is None else [back]]).astype(np.int32)
    final = np.full(S, np.inf, np.float32)
    final[S - 1] = float(rng.random())
    olabel = np.where(rng.random(n) < 0.2, rng.integers(1, 50, size=n), 0).astype(np.int32)
    if back is not None:
        olabel[back:] = 0
    return {"start": 0, "arc_off": np.minimum(np.arange(S + 1), n).astype(np.int64),
            "ilabel": rng.integers(1, 2 * NP + 1, size=n).astype(np.int32), "olabel": olabel,
            "weight": rng.random(n).astype(np.float32), "nextstate": dst, "final": final}


@functools.lru_cache(maxsize=None)
def chain_case(odeg):
    """Three utterances for k2_viterbi_faithful_chain<odeg> at the out-degrees no batch above has (1 and 4; the batches of hop 1 and 2
    run <2> and <3>): no epsilon arcs, at most 20 states, the largest out-degree exactly odeg, 8 to 30 frames."""
    rng = np.random.default_rng(3100 + odeg)
    c = Case()
    c.name, c.k2_ks, c.hop = "chain_odeg%d" % odeg, 0, odeg - 1
    if odeg == 1:
        c.graphs, c.T = [walk_graph(rng, 9), walk_graph(rng, 12, back=5), walk_graph(rng, 20)], [8, 18, 19]
    else:       # self-loop + hops of 1 .. odeg - 1
        c.graphs, c.T = [ltr_graph(rng, 20, odeg - 1, False), permute_states(ltr_graph(rng, 13, odeg - 1, True), rng), ltr_graph(rng, 7, odeg - 1, False)], [30, 9, 8]
    return _finish(c, rng, False)


def case(name):
    return generic_eps_case() if name == "generic_eps" else natural_case(name) if name in NATURAL else form_case(name)


ALL = list(FORMS) + list(NATURAL) + ["generic_eps"]


def batch_facts(c):
    f = [ref.graph_facts(g, ID2PDF) for g in c.graphs]
    return {"S": max(x["S"] for x in f), "inarcs": max(len(g["ilabel"]) for g in c.graphs), "indeg": max(x["indeg"] for x in f), "eps": any(x["eps"] for x in f),
            "same_row": all(x["same_row"] for x in f), "outdeg": max(x["outdeg"] for x in f)}


def oracle_graph(g):
    from oracle import oracle as orc
    return orc.OGraph(g["start"], g["arc_off"], g["ilabel"], g["olabel"], g["weight"], g["nextstate"], g["final"])


def oracle_align(c, u, **kw):
    from oracle import oracle as orc
    m = c.mats[u] if c.mats[u].size else np.zeros((1, max(c.T[u], 1)), np.float32)
    return orc.align_utterance_ll(oracle_graph(c.graphs[u]), ID2PDF, c.T[u], c.pdfs[u], m, acoustic_scale=c.scale, **kw)
