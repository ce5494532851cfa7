"""lattice-to-nbest restated in plain Python (the rule is written out at khg_lattices_nbest in include/khg_hip.h).
Numpy float32 scalars, one rounding per operation.  A lattice is the dict of arrays the other lattice restatements use.  Every
candidate of a state is generated, the lot is sorted by its key and cut at n: no merge."""
import numpy as np

F = np.float32
INF = F(np.inf)
SUCCEEDED, SCRATCH, NO_PATH, EPS_LOOP = 1, 4, 8, 16
INT32_MAX = 2**31 - 1
NBEST_MAX = 1024
FIELDS = ("frame", "graph_state", "tot_cost", "extra_cost", "final_cost", "arc_begin", "ilabel", "olabel", "graph_cost", "acoustic_cost", "nextstate")


def _key(c):
    # (t', e, j): Python compares the float32 scalars as floats (-0 == +0), then the integers
    return (c[0], c[4], c[5])


def nbest(lat, n, gs=1.0, as_=1.0):
    """-> (status, [(words, ali, (a, b), total)]) with float32 scalars"""
    assert 1 <= n <= NBEST_MAX
    with np.errstate(all="ignore"):
        return _nbest(lat, n, F(gs), F(as_))


def _nbest(lat, n, gs, as_):
    N, A = len(lat["frame"]), len(lat["ilabel"])
    if N == 0:
        return NO_PATH, []
    ab, nxt, il, ol, frame, fin = lat["arc_begin"], lat["nextstate"], lat["ilabel"], lat["olabel"], lat["frame"], lat["final_cost"]
    src = [0] * A
    ins = [[] for _ in range(N)]
    for s in range(N):
        for a in range(ab[s], ab[s + 1]):
            if nxt[a] <= s:
                return EPS_LOOP, []
            src[a] = s
            ins[nxt[a]].append(a)
    start = int(lat["start"])
    # the bound of the lists (it does not know of dropped candidates)
    bound, tot = [0] * N, 0
    for s in range(N):
        bound[s] = 1 if s == start else min(n, sum(bound[src[e]] for e in ins[s]))
        tot += bound[s]
    if tot > INT32_MAX:
        return SCRATCH, []
    lists = []
    for s in range(N):
        if s == start:
            lists.append([(F(0), F(0), F(0), 0, -1, 0)])
            continue
        cand = []
        for e in ins[s]:
            wa = F(gs * lat["graph_cost"][e])
            wb = F(as_ * lat["acoustic_cost"][e]) if il[e] != 0 else F(0)
            c = F(wa + wb)
            for j, (t, a, b, nw, _, _) in enumerate(lists[src[e]]):
                t2 = F(t + c)
                if t2 < INF:
                    cand.append((t2, F(a + wa), F(b + wb), nw + (1 if ol[e] != 0 else 0), e, j))
        cand.sort(key=_key)
        lists.append(cand[:n])
    T = int(frame[N - 1])
    done = []
    for s in range(N):
        if frame[s] != T or not np.isfinite(fin[s]):
            continue
        fw = F(gs * fin[s])
        for j, (t, a, b, nw, _, _) in enumerate(lists[s]):
            tt = F(t + fw)
            if tt < INF:
                done.append((tt, F(a + fw), b, nw, s, j))
    done.sort(key=_key)
    done = done[:n]
    if not done:
        return NO_PATH, []
    out = []
    for tt, a, b, nw, s, j in done:
        words, ali = [], [0] * max(T, 0)
        while True:
            e, jj = lists[s][j][4], lists[s][j][5]
            if e < 0:
                break
            s, j = src[e], jj
            if il[e] != 0 and 0 <= frame[s] < T:
                ali[frame[s]] = int(il[e])
            if ol[e] != 0:
                words.append(int(ol[e]))
        words.reverse()
        assert len(words) == nw
        out.append((words, ali, (a, b), tt))
    return SUCCEEDED, out


def all_paths(lat, limit=10000):
    """every path from the start to a finite final state of the last frame, as tuples of arcs with the final state last; None when there
    are more than `limit` (or an arc does not go to a higher state)"""
    N = len(lat["frame"])
    if N == 0:
        return []
    ab, nxt, frame, fin = lat["arc_begin"], lat["nextstate"], lat["frame"], lat["final_cost"]
    for s in range(N):
        for a in range(ab[s], ab[s + 1]):
            if nxt[a] <= s:
                return None
    T = frame[N - 1]
    out = []
    stack = [(int(lat["start"]), ())]
    while stack:
        s, arcs = stack.pop()
        if frame[s] == T and np.isfinite(fin[s]):
            out.append(arcs + (s,))
            if len(out) > limit:
                return None
        for a in range(ab[s], ab[s + 1]):
            stack.append((int(nxt[a]), arcs + (a,)))
    return out


def path_values(lat, path, gs=1.0, as_=1.0):
    """-> (total, (a, b), words, ali, d, m) of a path of all_paths: the sums taken left to right in float32; d the float64 sum of the same
    terms, m the largest absolute partial sum (of the total, the graph part or the acoustic part) in float64"""
    gs, as_ = F(gs), F(as_)
    N = len(lat["frame"])
    T = int(lat["frame"][N - 1])
    ab = lat["arc_begin"]
    t, a, b = F(0), F(0), F(0)
    d = da = db = m = 0.0
    words, ali = [], [0] * max(T, 0)
    with np.errstate(all="ignore"):
        for e in path[:-1]:
            wa = F(gs * lat["graph_cost"][e])
            wb = F(as_ * lat["acoustic_cost"][e]) if lat["ilabel"][e] != 0 else F(0)
            t, a, b = F(t + F(wa + wb)), F(a + wa), F(b + wb)
            d, da, db = d + float(wa) + float(wb), da + float(wa), db + float(wb)
            m = max(m, abs(d), abs(da), abs(db))
            s = int(np.searchsorted(ab, e, side="right")) - 1
            if lat["ilabel"][e] != 0 and 0 <= lat["frame"][s] < T:
                ali[lat["frame"][s]] = int(lat["ilabel"][e])
            if lat["olabel"][e] != 0:
                words.append(int(lat["olabel"][e]))
        fw = F(gs * lat["final_cost"][path[-1]])
        t, a = F(t + fw), F(a + fw)
        d, da = d + float(fw), da + float(fw)
        m = max(m, abs(d), abs(da))
    return t, (a, b), words, ali, d, m


def gap_exceeds_rounding(vals):
    """vals: {path: path_values(...)} of EVERY path of a lattice under one pair.  True when the float64 gap between the two cheapest
    paths exceeds (L + 1) * 2^-22 * M -- L the arcs of the longest path, M the largest absolute partial sum: the accumulated rounding
    of the n-best order and of best_path's.  A path whose cost is NaN (0 * inf at the pair (0, 0)) makes the gap NaN and the answer
    False: best_path's order says nothing about such a path, while the n-best rule drops it.  None: no path has a total < +inf."""
    if not any(v[0] < INF for v in vals.values()):
        return None
    ds = sorted((v[4] for v in vals.values()), key=lambda d: (np.isnan(d), d))
    with np.errstate(all="ignore"):
        gap = np.inf if len(ds) == 1 else (np.nan if np.isnan(ds[-1]) else ds[1] - ds[0])
    longest = max(len(p) - 1 for p in vals)
    m = max(v[5] for v in vals.values())
    return bool(gap > (longest + 1) * 2.0 ** -22 * m)


def bits(x):
    return np.asarray(x, np.float32).tobytes()
