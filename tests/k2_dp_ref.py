"""A plain numpy restatement of K2's exact DP and of its beam certificate, for the tests of
k2_viterbi_dp's instantiations: float64 token arithmetic, a cell's cost is (prev + w) + float32(-(float32(scale) * ll)), the
minimum over the state's in-arcs (in arc order: by source state, then by the arc's place among the source's out-arcs), the first
arc that attains it wins.  Nothing here is derived from the kernel's output; the oracle's FasterDecoder checks it on the CPU
(tests/test_k2_dp_cases_cpu.py).

A graph is one dict of tests/graphs.py: start, arc_off, ilabel, olabel, weight, nextstate, final.  Scores are a float32 matrix
[rows, T] whose row j belongs to the pdf pdfs[j] (the utterance's sorted pdf list)."""
import numpy as np

F32 = np.float32
INF = float("inf")
INT32_MAX = 2**31 - 1


def in_arcs(g):
    """-> (in_off [S+1], arc index of every in-arc) with a state's in-arcs in arc order"""
    S = len(g["final"])
    dst = np.asarray(g["nextstate"], np.int64)
    order = np.argsort(dst, kind="stable")
    in_off = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=S))]).astype(np.int64)
    return in_off, order


def graph_facts(g, id2pdf):
    """what the dispatch looks at: states, largest in-degree (epsilon arcs counted), any epsilon-input arc, every state's in-arcs
    read one score row, largest out-degree"""
    in_off, order = in_arcs(g)
    il = np.asarray(g["ilabel"])[order]
    pdf = np.where(il >= 1, np.asarray(id2pdf)[np.maximum(il, 0)], -1)
    same = all(len(set(pdf[in_off[s]: in_off[s + 1]].tolist())) <= 1 for s in range(len(g["final"])))
    return {"S": len(g["final"]), "indeg": int(np.diff(in_off).max()) if len(il) else 0, "eps": bool((np.asarray(g["ilabel"]) == 0).any()),
            "same_row": same, "outdeg": int(np.diff(g["arc_off"]).max()) if len(il) else 0}


def step_down(x):
    """float32(x) rounded to nearest, then one float down: a lower bound of x, as the kernel keeps a layer's minimum"""
    return float(np.nextafter(F32(x), F32(-INF)))


def _src_of_arcs(g):
    return np.repeat(np.arange(len(g["final"]), dtype=np.int64), np.diff(g["arc_off"]))


class Result:
    """ok (a final state is reachable in T frames), best_final, final_tie, states [T+1], arcs [T] (graph arc indices; with epsilon
    arcs: every arc of the path, in order), ali, words, like, layer_min [T+1], layer_cnt [T+1], tie (bool [T+1, S]: two arcs attain
    the cell's minimum), path_cost [T+1] (the token cost at the path's node of every layer), path_tie, any_tie"""

    def certified(self, beam, min_active=20, max_active=INT32_MAX):
        if not self.ok or self.path_tie or self.final_tie or max_active != INT32_MAX:
            return False
        b = float(F32(beam))
        for t in range(len(self.path_cost)):
            inside = self.path_cost[t] < step_down(self.layer_min[t]) + b
            few = self.layer_cnt[t] <= min_active and (t == 0 or self.layer_cnt[t - 1] <= min_active)
            if not (inside or few):
                return False
        return True

    @property
    def required_beam(self):
        return max(self.path_cost[t] - step_down(self.layer_min[t]) for t in range(len(self.path_cost)))


def _finish(r, g, pdf_row, id2pdf, ac, scale, like_scale):
    """alignment, words and `like` of the path r.arcs in the reference's float chain (faster-decoder.cc:384-417, decoder-wrappers.cc:95)"""
    il, ol, w = np.asarray(g["ilabel"]), np.asarray(g["olabel"]), np.asarray(g["weight"], F32)
    cost, t = 0.0, 0
    v1 = v2 = F32(0)
    ali, words, pc = [], [], [0.0]
    for a in r.arcs:
        before = cost
        if il[a] >= 1:
            cost = (cost + float(w[a])) + float(ac[pdf_row[int(id2pdf[il[a]])], t])
            t += 1
            ali.append(int(il[a]))
            pc.append(cost)
        else:
            cost = cost + float(w[a])
            pc[-1] = cost
        if ol[a] != 0:
            words.append(int(ol[a]))
        tot = F32(cost - before)
        v1 = F32(w[a] + v1)
        v2 = F32(F32(tot - w[a]) + v2)
    v1 = F32(F32(g["final"][r.best_final]) + v1)
    r.ali, r.words = np.asarray(ali, np.int32), np.asarray(words, np.int32)
    r.like = float(F32(-(v1 + v2)) / F32(like_scale if like_scale else scale))
    r.path_cost = np.asarray(pc)
    return r


def viterbi(g, id2pdf, pdfs, ll, scale=1.0, like_scale=0.0):
    """the exact DP of one utterance; ll is [len(pdfs), T] float32"""
    if (np.asarray(g["ilabel"]) == 0).any():
        return _viterbi_eps(g, id2pdf, pdfs, ll, scale, like_scale)
    S, T = len(g["final"]), int(ll.shape[1])
    pdf_row = {int(p): j for j, p in enumerate(pdfs)}
    ac = (-(F32(scale) * np.asarray(ll, F32))).astype(F32).astype(np.float64)
    in_off, order = in_arcs(g)
    deg = np.diff(in_off)
    D = max(1, int(deg.max()))
    srcs = _src_of_arcs(g)
    src = np.zeros((S, D), np.int64); w = np.full((S, D), INF); row = np.zeros((S, D), np.int64); arc = np.full((S, D), -1, np.int64)
    for s in range(S):
        for j, a in enumerate(order[in_off[s]: in_off[s + 1]]):
            src[s, j], w[s, j], arc[s, j] = srcs[a], float(F32(g["weight"][a])), a
            row[s, j] = pdf_row[int(id2pdf[g["ilabel"][a]])]
    cur = np.full(S, INF); cur[g["start"]] = 0.0
    bp = np.full((T + 1, S), -1, np.int8)
    r = Result()
    r.tie = np.zeros((T + 1, S), bool)
    r.layer_min, r.layer_cnt = np.empty(T + 1), np.empty(T + 1, np.int64)
    with np.errstate(invalid="ignore"):
        for t in range(T + 1):
            r.layer_min[t], r.layer_cnt[t] = cur.min(), np.isfinite(cur).sum()
            if t == T:
                break
            cand = (cur[src] + w) + ac[row, t]
            cand[np.isnan(cand)] = INF
            best = cand.min(1)
            hit = (cand == best[:, None]) & np.isfinite(best)[:, None]
            bp[t + 1] = np.where(hit.any(1), hit.argmax(1), -1)
            r.tie[t + 1] = hit.sum(1) > 1
            cur = best
    fin = cur + np.asarray(g["final"], np.float64)
    r.ok = bool(np.isfinite(fin).any())
    r.any_tie = bool(r.tie.any())
    if not r.ok:
        r.best_final, r.final_tie, r.path_tie = -1, False, False
        return r
    r.best_final = int(np.argmin(fin))                      # the smallest state among equal minima
    r.final_tie = int((fin == fin.min()).sum()) > 1
    r.any_tie = r.any_tie or r.final_tie
    st = np.empty(T + 1, np.int64); st[T] = r.best_final
    arcs = np.empty(T, np.int64)
    for t in range(T, 0, -1):
        j = bp[t, st[t]]
        arcs[t - 1], st[t - 1] = arc[st[t], j], src[st[t], j]
    assert st[0] == g["start"]
    r.states, r.arcs = st, arcs
    r.path_tie = bool(r.tie[np.arange(T + 1), st].any())
    return _finish(r, g, pdf_row, id2pdf, ac, scale, like_scale)


def _viterbi_eps(g, id2pdf, pdfs, ll, scale, like_scale):
    """graphs with epsilon-input arcs: the path and whether any cell's minimum is attained by two arcs (plain loops: small graphs)"""
    S, T = len(g["final"]), int(ll.shape[1])
    pdf_row = {int(p): j for j, p in enumerate(pdfs)}
    ac = (-(F32(scale) * np.asarray(ll, F32))).astype(F32).astype(np.float64)
    in_off, order = in_arcs(g)
    srcs, il = _src_of_arcs(g), np.asarray(g["ilabel"])
    wt = np.asarray(g["weight"], F32).astype(np.float64)
    ins = [[int(a) for a in order[in_off[s]: in_off[s + 1]]] for s in range(S)]
    r = Result()
    r.layer_min, r.layer_cnt = np.empty(T + 1), np.empty(T + 1, np.int64)
    r.tie = np.zeros((T + 1, S), bool)
    bp = np.full((T + 1, S), -1, np.int64)
    prev = None
    for t in range(T + 1):
        cur = np.full(S, INF)
        if t == 0:
            cur[g["start"]] = 0.0
        else:
            for s in range(S):
                for a in ins[s]:
                    if il[a] >= 1 and prev[srcs[a]] != INF:
                        c = (prev[srcs[a]] + wt[a]) + ac[pdf_row[int(id2pdf[il[a]])], t - 1]
                        if c < cur[s]:
                            cur[s], bp[t, s] = c, a
        changed = True
        while changed:                                     # epsilon closure
            changed = False
            for s in range(S):
                for a in ins[s]:
                    if il[a] == 0 and cur[srcs[a]] != INF and cur[srcs[a]] + wt[a] < cur[s]:
                        cur[s], bp[t, s], changed = cur[srcs[a]] + wt[a], a, True
        for s in range(S):                                 # at the fixed point: how many arcs attain the cell's cost
            if cur[s] == INF:
                continue
            n = 0
            for a in ins[s]:
                if il[a] >= 1 and t > 0 and prev[srcs[a]] != INF:
                    n += ((prev[srcs[a]] + wt[a]) + ac[pdf_row[int(id2pdf[il[a]])], t - 1]) == cur[s]
                elif il[a] == 0 and cur[srcs[a]] != INF:
                    n += (cur[srcs[a]] + wt[a]) == cur[s]
            r.tie[t, s] = n > 1
        r.layer_min[t], r.layer_cnt[t] = cur.min(), np.isfinite(cur).sum()
        prev = cur
    fin = prev + np.asarray(g["final"], np.float64)
    r.ok = bool(np.isfinite(fin).any())
    r.any_tie = bool(r.tie.any())
    if not r.ok:
        r.best_final, r.final_tie, r.path_tie = -1, False, False
        return r
    r.best_final = int(np.argmin(fin))
    r.final_tie = int((fin == fin.min()).sum()) > 1
    r.any_tie = r.any_tie or r.final_tie
    arcs, s, t = [], r.best_final, T
    while not (t == 0 and bp[t, s] < 0):
        a = int(bp[t, s])
        arcs.append(a)
        s = int(srcs[a])
        t -= 1 if il[a] >= 1 else 0
    assert s == g["start"]
    r.arcs = np.asarray(arcs[::-1], np.int64)
    r.path_tie = r.any_tie
    return _finish(r, g, pdf_row, id2pdf, ac, scale, like_scale)
