"""The tail of K2's exact DP (csrc/khg_k2_viterbi.hip.inc, KHG_OPT_K2_TAIL): the rule under which the replay's fp64 cost chain may run
as a wave scan, restated in numpy, and the batches tests/test_gpu_k2_tail.py runs.  tests/test_k2_tail_cpu.py shows the rule's
properties without a GPU.  Built on tests/k2_dp_cases.py and tests/k2_ladder_cases.py.

The rule.  The addends of an utterance are the floats w_i (arc weight) and ac_i (acoustic cost) of its path entries, in path order, 64
entries a batch.  With e_min the smallest binary exponent among the non-zero addends SO FAR and q = 2^(e_min - 23), a batch is scanned
when every addend so far is finite, every non-zero one is >= 2^-100 in magnitude (so: normal, a multiple of q) and the sum of the
magnitudes so far is <= 2^52 q; then every partial sum, in any order, is a multiple of q below 2^53 q -- a binary64 number -- and no
addition rounds.  The first batch that fails and every later batch of the utterance take the serial loop."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import k2_dp_cases as kc  # noqa: E402
import k2_dp_ref as ref  # noqa: E402
import k2_ladder_cases as lc  # noqa: E402
from graphs import permute_states  # noqa: E402

F32 = np.float32
BATCH = 64
TINY = 2.0 ** -100


def exact_ok(addends):
    """the rule on all addends so far (float32 values)"""
    x = np.abs(np.asarray(addends, F32).astype(np.float64))
    if not np.isfinite(x).all():
        return False
    nz = x[x != 0]
    if nz.size == 0:
        return True
    if nz.min() < TINY:
        return False
    e_min = int(np.frexp(nz.min())[1]) - 1                # nz.min() = m 2^e, 0.5 <= m < 1
    return bool(x.sum() <= 2.0 ** (52 + e_min - 23))


def batch_plan(w, ac):
    """-> (scanned, serial) batch counts of a path whose entries carry the addends w[i], ac[i]"""
    w, ac = np.asarray(w, F32), np.asarray(ac, F32)
    scanned = serial = 0
    for end in [min(b + BATCH, len(w)) for b in range(0, len(w), BATCH)]:
        if serial == 0 and exact_ok(np.concatenate([w[:end], ac[:end]])):
            scanned += 1
        else:
            serial += 1
    return scanned, serial


def serial_chain(w, ac, cost=0.0):
    """the reference's chain: cost <- (cost + w) + ac, one rounding per add; -> the cost after every entry"""
    out = np.empty(len(w))
    c = np.float64(cost)
    for i in range(len(w)):
        c = (c + np.float64(w[i])) + np.float64(ac[i])
        out[i] = c
    return out


def hillis_steele(d):
    d = np.array(d, np.float64)
    o = 1
    while o < len(d):
        d[o:] = d[o:] + d[:-o]
        o *= 2
    return d


def wave_scan(d):
    """the kernel's order on 64 lanes: four shifts inside the rows of 16, lane 15 of rows 0 / 2 into rows 1 / 3, lane 31 into rows 2, 3"""
    v = np.zeros(64)
    v[:len(d)] = d
    for o in (1, 2, 4, 8):
        s = np.zeros(64)
        for r in range(0, 64, 16):
            s[r + o: r + 16] = v[r: r + 16 - o]
        v = v + s
    s = np.zeros(64); s[16:32] = v[15]; s[48:64] = v[47]
    v = v + s
    s = np.zeros(64); s[32:64] = v[31]
    v = v + s
    return v[:len(d)]


def scanned_chain(w, ac, cost=0.0):
    """what the kernel computes for one batch (<= 64 entries) when the rule holds"""
    d = np.asarray(w, F32).astype(np.float64) + np.asarray(ac, F32).astype(np.float64)
    d[0] = np.float64(cost) + d[0]
    return wave_scan(d)


# ---- the GPU test's batches ----
T_EDGES = (1, 7, 8, 9, 63, 64, 65, 130)                   # the groups of eight layers and the batches of 64 entries, on both sides
S_EDGES = (1, 2, 63, 64, 65, 128, 129, 256)               # one, two and four state slots per lane of the trace-back
FEW = ((2, 7), (2, 130), (65, 64), (65, 130), (129, 65), (129, 130), (256, 9), (256, 130))
TABLES = ("grid", "tiny", "huge", "zeros", "positive", "ties", "random", "alltiny")


class Case:
    pass


def _graph(rng, S, T, i, hop=1):
    """a chain of S states.  Where T frames can cross it, only the last state is final (the path visits every state: every slot of the
    trace-back); where they cannot, every state is final"""
    g = lc.chain_graph(rng, S, True, loop0=(S == 1 or i % 3 == 0)) if hop == 1 else kc.ltr_graph(rng, S, hop, True)
    if T < kc.shortest(S, hop):
        g["final"] = rng.random(S).astype(F32)
    return g


def _scores(c, table):
    rng, c.scale = c.rng, kc.SCALE
    shape = [(len(p), t) for p, t in zip(c.pdfs, c.T)]
    if table == "random":                                  # the other cases' scores: the rule holds, nothing is arranged
        return [(-3.0 * rng.random(s)).astype(F32) for s in shape]
    c.scale = 1.0
    if table in ("grid", "tiny", "huge", "positive"):      # weights on a 2^-10 grid, no two alike by chance
        for g in c.graphs:
            g["weight"] = (rng.integers(0, 1024, size=len(g["weight"])) / 1024.0).astype(F32)
            g["final"] = np.where(np.isfinite(g["final"]), (rng.integers(0, 1024, size=len(g["final"])) / 1024.0), np.inf).astype(F32)
    if table == "grid":                                    # (a) the scan runs everywhere
        return [(-rng.integers(0, 3072, size=s) / 1024.0).astype(F32) for s in shape]
    if table == "tiny":                                    # (b) one frame's score ~1e-30 in the middle: scanned up to its batch, serial from it on
        m = [(-rng.integers(0, 3072, size=s) / 1024.0).astype(F32) for s in shape]
        for x, t in zip(m, c.T):
            x[:, t // 2] = F32(-1e-30)
        return m
    if table == "huge":                                    # (c) scores ~ -1e7: sum |addend| passes 2^52 q = 2^19 within the first batch
        return [np.full(s, -1e7, F32) - rng.integers(0, 8, size=s).astype(F32) for s in shape]
    if table == "positive":                                # (e) positive log-likelihoods: negative acoustic costs
        return [(rng.integers(0, 3072, size=s) / 1024.0).astype(F32) for s in shape]
    if table == "zeros":                                   # (d) zero weights of either sign, zero scores: signed zeros all the way
        for g in c.graphs:
            g["weight"] = np.where(rng.random(len(g["weight"])) < 0.5, 0.0, -0.0).astype(F32)
            g["final"] = np.where(np.isfinite(g["final"]), 0.0, np.inf).astype(F32)
        return [np.zeros(s, F32) for s in shape]
    if table == "alltiny":                                 # zero weights, scores ~1e-35: the sum bound holds, only the 2^-100 clause refuses
        for g in c.graphs:
            g["weight"][:] = 0.0
            g["final"] = np.where(np.isfinite(g["final"]), 0.0, np.inf).astype(F32)
        return [(-1e-35 * rng.integers(1, 4096, size=s)).astype(F32) for s in shape]
    if table == "ties":                                    # (f) every weight and score the same: equal-cost paths, a tie on the path
        for g in c.graphs:
            g["weight"][:] = 0.5
            g["final"] = np.where(np.isfinite(g["final"]), 0.0, np.inf).astype(F32)
        return [np.full(s, -1.0, F32) for s in shape]
    raise KeyError(table)


@functools.lru_cache(maxsize=None)
def case(table, permuted=False, kind="chain"):
    """kind: chain (in-degree 2; every (S, T) of the edges for "grid", a few of them else), deg3 (skip arcs), wide (> 256 states: the
    general trace-back, not the eight-layer one)"""
    if permuted:                                           # the same graphs and scores, states renumbered: the general body
        b = case(table, False, kind)
        c = Case()
        c.name, c.rng, c.T, c.scale = b.name + "_permuted", np.random.default_rng(99), b.T, b.scale
        c.graphs = [permute_states(g, c.rng) for g in b.graphs]
        c.mats = b.mats
    else:
        c = Case()
        c.name, c.rng = "%s_%s" % (kind, table), np.random.default_rng(8100 + TABLES.index(table) + 50 * ("chain", "deg3", "wide").index(kind))
        if kind == "chain":
            shapes = [(S, T) for S in S_EDGES for T in T_EDGES] if table == "grid" else list(FEW)
            shapes += [(129, 133), (256, 260)] if table in ("grid", "random") else []       # paths through the third and fourth slot
        elif kind == "deg3":
            shapes = [(65, 40), (65, 64), (130, 65), (130, 130), (256, 130), (256, 200)]
        else:
            shapes = [(257, 260), (300, 310), (300, 65), (64, 130)]
        c.T = [t for _, t in shapes]
        c.graphs = [_graph(c.rng, S, T, i, 2 if kind == "deg3" else 1) for i, (S, T) in enumerate(shapes)]
        c.pdfs = [kc.pdf_list(g) for g in c.graphs]
        c.mats = _scores(c, table)
    c.pdfs = [kc.pdf_list(g) for g in c.graphs]
    c.ref = [ref.viterbi(g, kc.ID2PDF, p, m, c.scale) for g, p, m in zip(c.graphs, c.pdfs, c.mats)]
    c.frame_off = np.concatenate([[0], np.cumsum(c.T)]).astype(np.int64)
    c.cfg = dict(beam=200.0)
    return c


def addends(c, u):
    """the floats the replay adds along the best path of utterance u: arc weights, acoustic costs -(scale * score) in float32"""
    r, g, m = c.ref[u], c.graphs[u], c.mats[u]
    row = {int(p): j for j, p in enumerate(c.pdfs[u])}
    rows = np.array([row[int(kc.ID2PDF[g["ilabel"][a]])] for a in r.arcs], np.int64)
    ac = (-(F32(c.scale) * m[rows, np.arange(len(rows))].astype(F32))).astype(F32)
    return np.asarray(g["weight"], F32)[r.arcs], ac


def expected_batches(c, u):
    return batch_plan(*addends(c, u)) if c.ref[u].ok else (0, 0)
