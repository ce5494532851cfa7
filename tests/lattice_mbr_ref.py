"""Minimum Bayes risk decoding of a raw lattice, restated in plain Python from the text at khg_lattices_mbr in include/khg_hip.h
(DESIGN.md section 7t), not from the C++ or the kernels; beside it what knows nothing of the rule: the brute-force enumeration of a
small lattice's paths with their probabilities and word strings, and a textbook Levenshtein distance.  A lattice is the dict of arrays
the other lattice restatements use (lattice_ops_ref.FIELDS + "start").  Python floats are IEEE doubles and `a + b * c` rounds the
product, then the sum: the order written here is the order of the rule."""
import math

import numpy as np

import lattice_ops_ref as ops
import lattice_post_ref as post
from lattice_score_ref import levenshtein  # noqa: F401

SUCCEEDED, SCRATCH, NO_PATH, EPS_LOOP, WORDS, NOT_CONVERGED = 1, 4, 8, 16, 32, 2048
F = np.float32
FINF = F(np.inf)
NINF = float("-inf")
DEL = 1.0 + 1e-5
MAX_WORDS = 2047


def _fail(status, lat, arc_cond=None, final_cond=None):
    return {"status": status, "iters": 0, "bayes_risk": math.inf, "words": [], "conf": [], "vocab": [], "gamma": [],
            "arc_cond": arc_cond if arc_cond is not None else [0.0] * len(lat["ilabel"]),
            "final_cond": final_cond if final_cond is not None else [0.0] * len(lat["frame"]), "risks": [], "cap": 0}


def _structure(lat):
    """src per arc, the in-arcs of every state in ascending arc number, the first state of the last frame"""
    N = len(lat["frame"])
    ab, nxt = lat["arc_begin"], lat["nextstate"]
    src, ins = [0] * len(nxt), [[] for _ in range(N)]
    for s in range(N):
        for a in range(int(ab[s]), int(ab[s + 1])):
            src[a] = s
            ins[int(nxt[a])].append(a)
    lo = N - 1
    while lo > 0 and lat["frame"][lo - 1] == lat["frame"][N - 1]:
        lo -= 1
    return src, ins, lo


def weights(lat, gs, as_):
    """-> (status, arc_cond, final_cond, the forward-backward restatement's dict): section Weights of the rule, on the restatement's alpha"""
    fb = post.forward_backward(lat, gs, as_)
    N, A = len(lat["frame"]), len(lat["ilabel"])
    arc_cond, final_cond = [0.0] * A, [0.0] * N
    if fb["status"] != SUCCEEDED:
        return fb["status"], arc_cond, final_cond, fb
    g, c = float(F(gs)), float(F(as_))
    src, _, lo = _structure(lat)
    alpha, tot = fb["alpha"], fb["tot"]
    for a in range(A):
        s, d = src[a], int(lat["nextstate"][a])
        if alpha[s] == NINF or alpha[d] == NINF:
            continue
        w = -(g * float(lat["graph_cost"][a]) + (c * float(lat["acoustic_cost"][a]) if lat["ilabel"][a] != 0 else 0.0))
        arc_cond[a] = math.exp((alpha[s] + w) - alpha[d])
    for f in range(lo, N):
        if lat["final_cost"][f] != FINF and alpha[f] != NINF:
            final_cond[f] = math.exp((alpha[f] + -(g * float(lat["final_cost"][f]))) - tot)
    return SUCCEEDED, arc_cond, final_cond, fb


def longest_path_words(lat):
    """the greatest number of words on a path from the start to a final state of the last frame (0 when there is none)"""
    N = len(lat["frame"])
    src, _, lo = _structure(lat)
    L = [-1] * N
    L[int(lat["start"])] = 0
    for a in range(len(src)):
        s, d = src[a], int(lat["nextstate"][a])
        if L[s] >= 0:
            L[d] = max(L[d], L[s] + (1 if lat["olabel"][a] != 0 else 0))
    return max([0] + [L[f] for f in range(lo, N) if lat["final_cost"][f] != FINF])


def accumulate(lat, h, arc_cond, final_cond, vocab):
    """one accumulation on the hypothesis h -> (bayes_risk, gamma [Q][len(vocab)] with gamma[q - 1] for position q)"""
    N, start = len(lat["frame"]), int(lat["start"])
    src, ins, lo = _structure(lat)
    ol = [int(w) for w in lat["olabel"]]
    col = {w: k for k, w in enumerate(vocab)}
    W = len(h)
    Q = 2 * W + 1
    r = [0] * (Q + 1)
    for i, w in enumerate(h):
        r[2 * (i + 1)] = int(w)

    def in_arcs(n):
        if n < N:
            return [(src[a], ol[a], arc_cond[a]) for a in ins[n]]
        return [(f, 0, final_cond[f]) for f in range(lo, N)]

    def row(ADs, w):
        dele = 0.0 if w == 0 else DEL
        arc, b = [0.0] * (Q + 1), [0] * (Q + 2)
        arc[0] = ADs[0] + dele
        for q in range(1, Q + 1):
            a1 = ADs[q - 1] + (0.0 if w == r[q] else 1.0)
            a2 = ADs[q] + dele
            a3 = arc[q - 1] + (0.0 if r[q] == 0 else 1.0)
            if a1 <= a2 and a1 <= a3:
                b[q], arc[q] = 1, a1
            elif a2 < a1 and a2 <= a3:
                b[q], arc[q] = 2, a2
            else:
                b[q], arc[q] = 3, a3
        return arc, b

    AD = [[0.0] * (Q + 1) for _ in range(N + 1)]
    for q in range(1, Q + 1):
        AD[start][q] = AD[start][q - 1] + (0.0 if r[q] == 0 else 1.0)
    for n in range(N + 1):
        if n == start:
            continue
        for s, w, p in in_arcs(n):
            if p == 0.0:
                continue
            arc, _ = row(AD[s], w)
            for q in range(Q + 1):
                AD[n][q] = AD[n][q] + p * arc[q]
    risk = AD[N][Q]
    BD = [[0.0] * (Q + 1) for _ in range(N + 1)]
    BD[N][Q] = 1.0
    gamma = [[0.0] * len(vocab) for _ in range(Q + 1)]
    for n in range(N, -1, -1):
        if n == start:
            continue
        for s, w, p in in_arcs(n):
            if p == 0.0:
                continue
            _, b = row(AD[s], w)
            ba = [0.0] * (Q + 2)
            for q in range(Q, 0, -1):
                ba[q] = (ba[q + 1] if b[q + 1] == 3 else 0.0) + p * BD[n][q]
                if b[q] == 1:
                    BD[s][q - 1] += ba[q]
                    gamma[q][col[w]] += ba[q]
                elif b[q] == 2:
                    BD[s][q] += ba[q]
                else:
                    gamma[q][0] += ba[q]
            ba[0] = (ba[1] if b[1] == 3 else 0.0) + p * BD[n][0]
            BD[s][0] += ba[0]
    x = 0.0
    for q in range(Q, 0, -1):
        x = x + BD[start][q]
        gamma[q][0] += x
    return risk, gamma[1:]


def mbr(lat, gs=1.0, as_=1.0, decode_mbr=True, max_iter=32, init=None, max_words=0, arc_cond=None, final_cond=None):
    """the whole rule -> dict(status, iters, bayes_risk, words, conf, vocab, gamma, arc_cond, final_cond, risks (one per accumulation), cap)"""
    st, ac, fc, _ = weights(lat, gs, as_)
    if st != SUCCEEDED:
        return _fail(st, lat)
    if arc_cond is not None:
        ac, fc = [float(x) for x in arc_cond], [float(x) for x in final_cond]
    vocab = [0] + sorted({int(w) for w in lat["olabel"] if w != 0})
    if init is None:
        bp = ops.best_path(lat, gs, as_)
        h = [int(w) for w in bp["words"]] if bp["status"] == SUCCEEDED else []
    else:
        h = [int(w) for w in init]
    cap = max_words if max_words > 0 else max(len(h), longest_path_words(lat))
    if len(h) > cap or cap > MAX_WORDS:
        return dict(_fail(WORDS, lat, ac, fc), cap=cap)
    status, iters, risks = SUCCEEDED, 0, []
    while True:
        risk, gamma = accumulate(lat, h, ac, fc, vocab)
        risks.append(risk)
        if not decode_mbr:
            break
        hn = []
        for g in gamma:
            bi = 0
            for k in range(1, len(vocab)):
                if g[bi] < g[k]:
                    bi = k
            if vocab[bi] != 0:
                hn.append(vocab[bi])
        if hn == h:
            break
        if iters == max_iter:
            status |= NOT_CONVERGED
            break
        if len(hn) > cap:
            return dict(_fail(WORDS, lat, ac, fc), iters=iters, risks=risks, cap=cap)
        h, iters = hn, iters + 1
    conf = [gamma[2 * i + 1][vocab.index(w)] if w in vocab else 0.0 for i, w in enumerate(h)]
    return {"status": status, "iters": iters, "bayes_risk": risk, "words": h, "conf": conf, "vocab": vocab, "gamma": gamma, "arc_cond": ac,
            "final_cond": fc, "risks": risks, "cap": cap}


def table_bytes(lat, cap):
    """the device's table of one utterance: 8 * (2 * (states + 1) + len(vocab)) * (2 * cap + 2)"""
    V = 1 + len({int(w) for w in lat["olabel"] if w != 0})
    return 8 * (2 * (len(lat["frame"]) + 1) + V) * (2 * cap + 2)


def path_probs(lat, gs=1.0, as_=1.0, limit=3000):
    """brute force: [(probability, words)] of every path from the start to a final state of the last frame, the probabilities
    normalised with math.fsum; None when there are more than `limit` paths or the lattice is not admissible; [] without a path"""
    N = len(lat["frame"])
    if N == 0 or lat["start"] < 0:
        return []
    g, c = float(F(gs)), float(F(as_))
    ab, nxt, olab, il, fr = (np.asarray(lat[k]) for k in ("arc_begin", "nextstate", "olabel", "ilabel", "frame"))
    for s in range(N):
        for a in range(ab[s], ab[s + 1]):
            if nxt[a] <= s:
                return None
    out, stack = [], [(int(lat["start"]), 0.0, ())]
    while stack:
        s, ll, words = stack.pop()
        if fr[s] == fr[N - 1] and lat["final_cost"][s] != FINF:
            out.append((ll - g * float(lat["final_cost"][s]), list(words)))
            if len(out) > limit:
                return None
        for a in range(ab[s], ab[s + 1]):
            w = -(g * float(lat["graph_cost"][a]) + (c * float(lat["acoustic_cost"][a]) if il[a] != 0 else 0.0))
            stack.append((int(nxt[a]), ll + w, words + ((int(olab[a]),) if olab[a] != 0 else ())))
            if len(stack) > 50 * limit:
                return None
    if not out:
        return []
    top = max(p[0] for p in out)
    z = math.fsum(math.exp(p[0] - top) for p in out)
    return [(math.exp(p[0] - top) / z, p[1]) for p in out]


def expected_levenshtein(paths, h):
    """sum over the paths of probability * textbook distance between the path's words and h"""
    return math.fsum(p * levenshtein(w, h) for p, w in paths)
