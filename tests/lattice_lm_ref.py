"""lattice-lmrescore with a backoff n-gram LM, restated in plain Python (the rule is written out at
khg_lattices_lm_rescore in include/khg_hip.h).  Numpy float32 scalars, one rounding per operation.  A lattice is the dict of arrays the
other lattice restatements use (lattice_ops_ref.FIELDS + "start"); an LM is NgramLm.to_arrays()'s dict."""
import numpy as np

F = np.float32
INF = F(np.inf)
SUCCEEDED, SCRATCH, NO_PATH, EPS_LOOP, LM_OOV = 1, 4, 8, 16, 1024
INT32_MAX = 2**31 - 1
FIELDS = ("frame", "graph_state", "tot_cost", "extra_cost", "final_cost", "arc_begin", "ilabel", "olabel", "graph_cost", "acoustic_cost", "nextstate")
INTS = ("frame", "graph_state", "arc_begin", "ilabel", "olabel", "nextstate")


def advance(lm, h, w):
    """-> (next state, cost); (-1, cost so far) for a word out of vocabulary"""
    c = F(0.0)
    while True:
        lo, hi = int(lm["arc_begin"][h]), int(lm["arc_begin"][h + 1])
        while lo < hi:
            mid = (lo + hi) // 2
            if lm["word"][mid] < w:
                lo = mid + 1
            else:
                hi = mid
        if lo < lm["arc_begin"][h + 1] and lm["word"][lo] == w:
            return int(lm["next"][lo]), F(c + lm["cost"][lo])
        if h == 0:
            return -1, c
        c = F(c + lm["backoff_cost"][h])
        h = int(lm["backoff"][h])


def score(lm, words):
    """the float cost of a sentence, <s> implied and </s> added; None with a word out of vocabulary"""
    h, t = int(lm["start"]), F(0.0)
    for w in words:
        h, c = advance(lm, h, int(w))
        if h < 0:
            return None
        t = F(t + c)
    return F(t + lm["final_cost"][h])


def empty():
    lat = {k: np.zeros(0, np.int32 if k in INTS else np.float32) for k in FIELDS}
    lat["arc_begin"] = np.zeros(1, np.int32)
    lat["start"] = -1
    return lat


def lm_rescore(lat, lm, scale=1.0, hist_factor=8):
    """-> (the rescored lattice (empty unless SUCCEEDED), status, the largest |H(s)| (0 unless SUCCEEDED))"""
    scale = F(scale)
    N = len(lat["frame"])
    if N == 0:
        return empty(), NO_PATH, 0
    ab, nxt, ol = lat["arc_begin"], lat["nextstate"], lat["olabel"]
    for s in range(N):
        for a in range(ab[s], ab[s + 1]):
            if nxt[a] <= s:
                return empty(), EPS_LOOP, 0
    # in-arcs
    ins = [[] for _ in range(N)]
    for s in range(N):
        for a in range(ab[s], ab[s + 1]):
            ins[nxt[a]].append((s, a))
    cap = min(hist_factor * N, INT32_MAX)
    H, used = [], 0
    for d in range(N):
        cand = {int(lm["start"])} if d == lat["start"] else set()
        for s, a in ins[d]:
            for h in H[s]:
                cand.add(h if ol[a] == 0 else advance(lm, h, int(ol[a]))[0])
        if -1 in cand:
            return empty(), LM_OOV, 0
        used += len(cand)
        if used > cap:
            return empty(), SCRATCH, 0
        H.append(sorted(cand))
    first = np.concatenate([[0], np.cumsum([len(h) for h in H])])
    out = {k: [] for k in FIELDS}
    out["arc_begin"].append(0)
    for s in range(N):
        for h in H[s]:
            for k in ("frame", "graph_state", "tot_cost", "extra_cost"):
                out[k].append(lat[k][s])
            f = F(lat["final_cost"][s])
            out["final_cost"].append(f if f == INF else F(f + F(scale * lm["final_cost"][h])))
            for a in range(ab[s], ab[s + 1]):
                d, w, g, hh = int(nxt[a]), int(ol[a]), F(lat["graph_cost"][a]), h
                if w != 0:
                    hh, c = advance(lm, h, w)
                    g = F(g + F(scale * c))
                out["ilabel"].append(lat["ilabel"][a]); out["olabel"].append(w); out["graph_cost"].append(g)
                out["acoustic_cost"].append(lat["acoustic_cost"][a])
                out["nextstate"].append(int(first[d]) + H[d].index(hh))
            out["arc_begin"].append(len(out["ilabel"]))
    res = {k: np.asarray(out[k], np.int32 if k in INTS else np.float32) for k in FIELDS}
    res["start"] = int(first[lat["start"]])
    return res, SUCCEEDED, max(len(h) for h in H)
