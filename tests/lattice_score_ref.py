"""Scoring lattices, restated in plain Python (the rules are written out at khg_lattices_oracle in
include/khg_hip.h): lattice-add-penalty, lattice-oracle, compute-wer's counts and the sweep of score.sh; beside them a textbook
Levenshtein distance and a brute-force enumerator of a small lattice's paths, which know nothing of the rule.  A lattice is the dict of
arrays the other lattice restatements use (lattice_ops_ref.FIELDS + "start")."""
import numpy as np

import lattice_ops_ref as ops

F = np.float32
FINF = F(np.inf)
INF = 1 << 30
SUCCEEDED, SCRATCH, NO_PATH, EPS_LOOP, WORDS = 1, 4, 8, 16, 256
NONE, DEL = -1, -2
FIELDS = ops.FIELDS


def add_penalty(lat, penalty):
    """rule 1: graph_cost' = fl(graph_cost + penalty) on the arcs with a word; everything else as stored"""
    out = {k: (np.array(v, copy=True) if k != "start" else v) for k, v in lat.items()}
    g = np.asarray(lat["graph_cost"], F)
    out["graph_cost"] = np.where(np.asarray(lat["olabel"]) != 0, (g + F(penalty)).astype(F), g).astype(F)
    return out


def _fail(status, R, T):
    return {"status": status, "counts": [R, 0, R, 0], "words": [], "ali": [0] * T, "arcs": []}


def oracle(lat, ref):
    """rule 2 -> dict(status, counts [errors, insertions, deletions, substitutions], words, ali (one id per frame), arcs)"""
    N, R = len(lat["frame"]), len(ref)
    if N == 0 or lat["start"] < 0:
        return _fail(NO_PATH, R, 0)
    ab, nxt, ol, il, fr = (np.asarray(lat[k]) for k in ("arc_begin", "nextstate", "olabel", "ilabel", "frame"))
    T = max(int(fr[N - 1]), 0)
    ins = [[] for _ in range(N)]
    for s in range(N):
        for a in range(ab[s], ab[s + 1]):
            if nxt[a] <= s:
                return _fail(EPS_LOOP, R, T)
            ins[nxt[a]].append((a, s))          # ascending arc number
    E = [[INF] * (R + 1) for _ in range(N)]
    M = [[NONE] * (R + 1) for _ in range(N)]
    for s in range(N):
        for q in range(R + 1):
            c, mv = (0 if s == lat["start"] and q == 0 else INF), NONE
            for a, p in ins[s]:
                w = int(ol[a])
                if w == 0:
                    if E[p][q] < INF and E[p][q] < c:
                        c, mv = E[p][q], a
                else:
                    if q >= 1 and E[p][q - 1] < INF and E[p][q - 1] + (w != ref[q - 1]) < c:
                        c, mv = E[p][q - 1] + (w != ref[q - 1]), a
                    if E[p][q] < INF and E[p][q] + 1 < c:
                        c, mv = E[p][q] + 1, -3 - a
            if q >= 1 and E[s][q - 1] < INF and E[s][q - 1] + 1 < c:
                c, mv = E[s][q - 1] + 1, DEL
            E[s][q], M[s][q] = c, mv
    fin = -1
    for s in range(N):
        if fr[s] == fr[N - 1] and lat["final_cost"][s] != FINF and E[s][R] < INF and (fin < 0 or E[s][R] < E[fin][R]):
            fin = s
    if fin < 0:
        return _fail(NO_PATH, R, T)
    src = ops._src_of(lat)
    s, q, n_ins, n_del, n_sub, words, arcs, ali = fin, R, 0, 0, 0, [], [], [0] * T
    while M[s][q] != NONE:
        mv = M[s][q]
        if mv == DEL:
            n_del, q = n_del + 1, q - 1
            continue
        a = mv if mv >= 0 else -3 - mv
        w = int(ol[a])
        if mv < 0:
            n_ins += 1
        elif w != 0:
            q -= 1
            n_sub += int(w != ref[q])
        if w != 0:
            words.append(w)
        arcs.append(a)
        p = int(src[a])
        if il[a] != 0 and 0 <= fr[p] < T:
            ali[fr[p]] = int(il[a])
        s = p
    assert s == lat["start"] and q == 0
    assert n_ins + n_del + n_sub == E[fin][R]
    return {"status": SUCCEEDED, "counts": [n_ins + n_del + n_sub, n_ins, n_del, n_sub], "words": words[::-1], "ali": ali, "arcs": arcs[::-1]}


def chain(words):
    """the single-path lattice of a word sequence: state i after i words, the last one final"""
    n = len(words)
    return {"frame": np.arange(n + 1, dtype=np.int32), "graph_state": np.zeros(n + 1, np.int32), "tot_cost": np.zeros(n + 1, F),
            "extra_cost": np.zeros(n + 1, F), "final_cost": np.array([FINF] * n + [0.0], F), "arc_begin": np.arange(n + 2, dtype=np.int32).clip(0, n),
            "ilabel": np.arange(1, n + 1, dtype=np.int32), "olabel": np.asarray(words, np.int32).reshape(-1), "graph_cost": np.zeros(n, F),
            "acoustic_cost": np.zeros(n, F), "nextstate": np.arange(1, n + 1, dtype=np.int32), "start": 0}


def edit_counts(ref, hyp):
    """compute-wer's counts by rule 2 on the chain of the hypothesis words"""
    return oracle(chain([int(w) for w in hyp]), [int(w) for w in ref])["counts"]


def best_path_words(lat, gs, as_, penalty):
    """lattice_ops_ref.best_path with w1 = fl(fl(gs * graph_cost) + penalty) on the arcs with a word -> (status, words)"""
    plain = ops._weights

    def weights(l, g, a):
        w1, w2, fw = plain(l, g, a)
        return np.where(np.asarray(l["olabel"]) != 0, (w1 + F(penalty)).astype(F), w1).astype(F), w2, fw

    ops._weights = weights
    try:
        r = ops.best_path(lat, gs, as_)
    finally:
        ops._weights = plain
    return r["status"], r["words"]


def wer(lat, ref, gs, as_, penalty):
    """rule 3 for one triple -> (status, number of words, counts); no path: an empty hypothesis"""
    st, words = best_path_words(lat, gs, as_, penalty)
    words = words if st == SUCCEEDED else []
    return st, len(words), edit_counts(ref, words)


def levenshtein(ref, hyp):
    """the textbook distance: the total only"""
    d = list(range(len(hyp) + 1))
    for i, r in enumerate(ref, 1):
        prev, d[0] = d[0], i
        for j, h in enumerate(hyp, 1):
            prev, d[j] = d[j], min(d[j] + 1, d[j - 1] + 1, prev + (r != h))
    return d[len(hyp)]


def paths(lat, limit=2000):
    """the word sequences of every path from the start to a final state of the last frame (a final state as best_path takes it), as a
    list of (words, arcs); None when there are more than `limit` or an arc does not go to a higher state"""
    N = len(lat["frame"])
    if N == 0 or lat["start"] < 0:
        return []
    ab, nxt, ol, fr = (np.asarray(lat[k]) for k in ("arc_begin", "nextstate", "olabel", "frame"))
    for s in range(N):
        for a in range(ab[s], ab[s + 1]):
            if nxt[a] <= s:
                return None
    out = []
    stack = [(int(lat["start"]), (), ())]
    while stack:
        s, words, arcs = stack.pop()
        if fr[s] == fr[N - 1] and lat["final_cost"][s] != FINF:
            out.append((list(words), list(arcs)))
            if len(out) > limit:
                return None
        for a in range(ab[s], ab[s + 1]):
            stack.append((int(nxt[a]), words + ((int(ol[a]),) if ol[a] != 0 else ()), arcs + (a,)))
            if len(stack) > 50 * limit:
                return None
    return out
