"""Inputs for the ladder form of K2's exact DP (k2_viterbi_dp<1, 2, true, false, SC, true>, csrc/khg_k2_viterbi.hip.inc), for
tests/test_gpu_k2_ladder.py; tests/test_k2_ladder_cpu.py shows their properties without a GPU.  Built on tests/k2_dp_cases.py.

A chain graph: state s has a self-loop (but state 0) and one arc to s + 1 -- every in-arc of s comes from s or s - 1, the host's
`ladder` fact.  Sizes at the wave boundaries on both sides (1 to 4 waves), lengths at the group edges: T = S - 2 reaches no final
state, T = S - 1 leaves exactly one path, then a partial last group, a full one, and a tail where only the last wave still works."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import k2_dp_cases as kc  # noqa: E402
import k2_dp_ref as ref  # noqa: E402
from graphs import permute_states  # noqa: E402

SIZES = (2, 63, 64, 65, 66, 128, 129, 192, 193, 256)


def lengths(S):
    return sorted({max(0, S - 2), S - 1, S, S + 6, S + 7, S + 8, S + 9, S + 33})


def is_ladder(g):
    """the host fact: no epsilon arc, in-degree <= 2, every in-arc of s from s or s - 1, one of either at most"""
    src = np.repeat(np.arange(len(g["final"])), np.diff(g["arc_off"]))
    dst = np.asarray(g["nextstate"])
    if (np.asarray(g["ilabel"]) == 0).any() or not np.isin(dst - src, (0, 1)).all():
        return False
    return len(set(zip(src.tolist(), dst.tolist()))) == len(src) and (np.bincount(dst, minlength=1).max() if len(dst) else 0) <= 2


def chain_graph(rng, S, same_row, loop0=False):
    """a chain of S states (k2_dp_cases.ltr_graph at hop 1); loop0: a self-loop on state 0 too (a state whose FIRST in-arc slot is
    the self-loop; everywhere else the arc from s - 1 comes first)"""
    g = kc.ltr_graph(rng, S, 1, same_row)
    if loop0:
        tid = int(g["ilabel"][0]) if same_row and len(g["ilabel"]) else 1 + int(rng.integers(0, 2 * kc.NP))
        for k, v in (("ilabel", tid), ("olabel", 0), ("weight", float(rng.random())), ("nextstate", 0)):
            g[k] = np.concatenate([[v], g[k]]).astype(g[k].dtype)
        g["arc_off"] = np.concatenate([[0], g["arc_off"][1:] + 1]).astype(np.int64)
    return g


def _finish(c, mats=None, scale=kc.SCALE, narrow=None):
    c.pdfs = [kc.pdf_list(g) for g in c.graphs]
    c.mats = mats if mats is not None else [(-3.0 * c.rng.random((len(p), t))).astype(np.float32) for p, t in zip(c.pdfs, c.T)]
    c.scale = scale
    c.ref = [ref.viterbi(g, kc.ID2PDF, p, m, c.scale) for g, p, m in zip(c.graphs, c.pdfs, c.mats)]
    good = [r for r in c.ref if r.ok]
    beam = narrow if narrow is not None else float(np.float32(np.median([r.required_beam for r in good])))
    live = int(np.median(np.concatenate([r.layer_cnt for r in good])))
    c.cfgs = [dict(beam=200.0), dict(beam=beam, min_active=0), dict(beam=beam, min_active=live)]
    c.frame_off = np.concatenate([[0], np.cumsum(c.T)]).astype(np.int64)
    return c


class Case:
    pass


def _new(name, seed, ladder, sc):
    c = Case()
    c.name, c.rng, c.ladder, c.sc = name, np.random.default_rng(seed), ladder, sc
    c.plan = (1, 2, True, sc)
    c.graphs, c.T = [], []
    return c


def _sizes(name, seed, same_row):
    c = _new(name, seed, True, same_row)
    for i, S in enumerate(SIZES):
        for j, T in enumerate(lengths(S)):
            c.graphs.append(chain_graph(c.rng, S, same_row, loop0=(i + j) % 3 == 0))
            c.T.append(T)
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "sizes":                                    # one score row per state: the SC instantiation
        return _finish(_sizes(name, 7001, True))
    if name == "sizes_rows":                               # score rows at random: the other one
        return _finish(_sizes(name, 7002, False))
    if name == "permuted":
        # the utterances of "sizes" (c.of: which) with their states renumbered: not ladders, the same alignments.  (Two states in
        # chain order stay a ladder under one of their two numberings: left out.)
        b = case("sizes")
        c = _new(name, 7007, False, True)
        c.of = [k for k, g in enumerate(b.graphs) if len(g["final"]) > 2]
        c.graphs, c.T = [permute_states(b.graphs[k], c.rng) for k in c.of], [b.T[k] for k in c.of]
        return _finish(c, [b.mats[k] for k in c.of])
    if name == "mixed":                                    # the block is sized by the largest; smaller utterances keep fewer waves
        c = _new(name, 7003, True, True)
        for S in (40, 70, 200):
            for T in (S - 1, S + 5, S + 8, S + 40):
                c.graphs.append(chain_graph(c.rng, S, True))
                c.T.append(T)
        return _finish(c)
    if name == "constant":                                 # every weight and score the same: every merge is a tie
        c = _new(name, 7004, True, True)
        for S in (2, 64, 65, 130, 256):
            for T in (S, S + 9):
                g = chain_graph(c.rng, S, True, loop0=True)
                g["weight"][:] = 0.5
                g["final"][S - 1] = 0.0
                c.graphs.append(g)
                c.T.append(T)
        pdfs = [kc.pdf_list(g) for g in c.graphs]
        return _finish(c, [np.full((len(p), t), -1.0, np.float32) for p, t in zip(pdfs, c.T)], 1.0, narrow=4.0)
    if name == "boundary_tie":
        # Scores 0, forward arcs 0, the self-loop of state s costs s + 1 -- but state 64's costs 2, as state 1's: waiting is cheapest
        # in state 1 and, equally, in state 64.  cost(t, s) = 2 (t - s) for every live cell, so a cell's two candidates differ by
        # (its self-loop's weight - 2): equal at state 64 alone, whose forward arc comes from lane 63 of the wave below.  Small
        # integers: exact in every float format on the way.
        c = _new(name, 7005, True, True)
        for S, T in ((66, 70), (130, 131), (130, 150), (200, 240)):
            g = chain_graph(c.rng, S, True)
            src = np.repeat(np.arange(S), np.diff(g["arc_off"]))
            loop = src == g["nextstate"]
            g["weight"][:] = 0.0
            g["weight"][loop] = (src[loop] + 1).astype(np.float32)
            g["weight"][loop & (src == 64)] = 2.0
            g["final"][S - 1] = 0.0
            c.graphs.append(g)
            c.T.append(T)
        pdfs = [kc.pdf_list(g) for g in c.graphs]
        return _finish(c, [np.zeros((len(p), t), np.float32) for p, t in zip(pdfs, c.T)], 1.0, narrow=40.0)
    if name == "indeg3":                                   # skip arcs: in-degree 3, the three-slot kernel as before
        c = _new(name, 7006, False, True)
        c.plan = (1, 3, True, True)
        for S, T in ((65, 40), (130, 70), (130, 131)):
            c.graphs.append(kc.ltr_graph(c.rng, S, 2, True))
            c.T.append(T)
        return _finish(c)
    raise KeyError(name)


LADDERS = ["sizes", "sizes_rows", "mixed", "constant", "boundary_tie"]
ALL = LADDERS + ["permuted", "indeg3"]
