"""lattice-determinize-pruned restated in plain Python (the rule is written out at khg_lattices_determinize in
include/khg_hip.h).  Numpy float32 scalars, one rounding per operation.  A lattice is the dict of arrays the other lattice restatements
use.  The two prune steps are the existing operation (Lattice.prune_with_status); everything between them is restated here."""
import numpy as np

F = np.float32
INF = F(np.inf)
SUCCEEDED, SCRATCH, NO_PATH, EPS_LOOP = 1, 4, 8, 16
INT32_MAX = 2**31 - 1
FIELDS = ("frame", "graph_state", "tot_cost", "extra_cost", "final_cost", "arc_begin", "ilabel", "olabel", "graph_cost", "acoustic_cost", "nextstate")
INTS = ("frame", "graph_state", "arc_begin", "ilabel", "olabel", "nextstate")
STATS = ("in_states", "in_arcs", "pruned_states", "det_states", "out_states", "out_arcs", "max_subset", "max_closure")


def empty():
    lat = {k: np.zeros(0, np.int32 if k in INTS else np.float32) for k in FIELDS}
    lat["arc_begin"] = np.zeros(1, np.int32)
    lat["start"] = -1
    return lat


def better(x, y):
    """the order of best_path on weight pairs: fl(a + b) first, then a; strictly"""
    sx, sy = F(x[0] + x[1]), F(y[0] + y[1])
    if sx < sy:
        return True
    if sx > sy:
        return False
    return x[0] < y[0]


def arc_weights(lat, gs, as_):
    gs, as_ = F(gs), F(as_)
    wa = [F(gs * g) for g in lat["graph_cost"]]
    wb = [F(as_ * c) if il != 0 else F(0.0) for c, il in zip(lat["acoustic_cost"], lat["ilabel"])]
    return wa, wb


class Scratch(Exception):
    pass


def split(X, gs, as_, delta, state_factor):
    """steps 2 to 5 on the pruned lattice X (at least one state, every arc to a higher state) -> (Y, det_states, max_subset, max_closure);
    raises Scratch"""
    gs, delta = F(gs), F(delta)
    N, A = len(X["frame"]), len(X["ilabel"])
    ab, nxt, ol, fin, frame = X["arc_begin"], X["nextstate"], X["olabel"], X["final_cost"], X["frame"]
    wa, wb = arc_weights(X, gs, as_)
    src = np.zeros(A, np.int64)
    ins = [[] for _ in range(N)]
    for s in range(N):
        for a in range(ab[s], ab[s + 1]):
            src[a] = s
            ins[nxt[a]].append(a)
    cap_s, cap_a = min(state_factor * N, INT32_MAX), min(state_factor * A, INT32_MAX)
    T = frame[N - 1]
    Ds = []          # {"K": [...], "R": [...], "E": {s: cost}, "pred": {s: arc or -1}}
    used = [0, 0]    # elements, their states' arcs

    def arrive(I):
        """-> (the number of the determinized state, pred of this arrival)"""
        best = None
        for s in sorted(I):
            if best is None or better(I[s], I[best]):
                best = s
        b = I[best]
        norm = {s: (F(c[0] - b[0]), F(c[1] - b[1])) for s, c in I.items()}
        E, pred = {}, {}
        for s in range(min(I), N):
            inc, p = norm.get(s), -1
            for a in ins[s]:
                if ol[a] != 0 or src[a] not in E:
                    continue
                e = E[src[a]]
                cand = (F(e[0] + wa[a]), F(e[1] + wb[a]))
                if inc is None or better(cand, inc):
                    inc, p = cand, a
            if inc is not None:
                E[s], pred[s] = inc, p
        K = [s for s in sorted(I) if pred[s] == -1]
        R = [E[s] for s in K]
        for d, D in enumerate(Ds):
            if D["K"] == K and all(abs(F(r[0] - q[0])) <= delta and abs(F(r[1] - q[1])) <= delta for r, q in zip(R, D["R"])):
                return d, pred
        used[0] += len(E)
        used[1] += sum(int(ab[s + 1] - ab[s]) for s in E)
        if used[0] > cap_s or used[1] > cap_a:
            raise Scratch()
        Ds.append({"K": K, "R": R, "E": E, "pred": pred})
        return len(Ds) - 1, pred

    arrive({int(X["start"]): (F(0.0), F(0.0))})
    emit = {}        # (D, arc) -> D'
    d = 0
    while d < len(Ds):
        E = Ds[d]["E"]
        kept = {}
        for p in sorted(E):
            for a in range(ab[p], ab[p + 1]):
                if ol[a] == 0:
                    continue
                cand = (F(E[p][0] + wa[a]), F(E[p][1] + wb[a]))
                key = (int(ol[a]), int(nxt[a]))
                if key not in kept or better(cand, kept[key][0]):
                    kept[key] = (cand, a)
        for w in sorted({k[0] for k in kept}):
            I = {dest: kept[(ww, dest)][0] for (ww, dest) in kept if ww == w}
            d2, pred = arrive(I)
            for dest in I:
                if pred[dest] == -1:
                    emit[(d, kept[(w, dest)][1])] = d2
        d += 1
    # finals
    for D in Ds:
        bs, bv = -1, None
        for s in sorted(D["E"]):
            if fin[s] == INF or frame[s] != T:
                continue
            v = (F(D["E"][s][0] + F(gs * fin[s])), D["E"][s][1])
            if bs < 0 or better(v, bv):
                bs, bv = s, v
        D["final"] = bs
    # the split lattice
    elems = sorted((s, d) for d, D in enumerate(Ds) for s in D["E"])
    newid = {e: i for i, e in enumerate(elems)}
    out = {k: [] for k in FIELDS}
    for s, d in elems:
        D = Ds[d]
        for k in ("frame", "graph_state", "tot_cost", "extra_cost"):
            out[k].append(X[k][s])
        out["final_cost"].append(fin[s] if D["final"] == s else INF)
        out["arc_begin"].append(len(out["ilabel"]))
        for a in range(ab[s], ab[s + 1]):
            dest = int(nxt[a])
            if ol[a] == 0:
                if D["pred"].get(dest, -2) != a:
                    continue
                to = newid[(dest, d)]
            else:
                if (d, a) not in emit:
                    continue
                to = newid[(dest, emit[(d, a)])]
            for k in ("ilabel", "olabel", "graph_cost", "acoustic_cost"):
                out[k].append(X[k][a])
            out["nextstate"].append(to)
    out["arc_begin"].append(len(out["ilabel"]))
    Y = {k: np.asarray(out[k], np.int32 if k in INTS else np.float32) for k in FIELDS}
    Y["start"] = newid[(int(X["start"]), 0)]
    return Y, len(Ds), max(len(D["K"]) for D in Ds), max(len(D["E"]) for D in Ds)


def _host(lat):
    import kaldi_hmm_gmm_amd as khg
    return khg.Lattice.from_arrays(*[lat[k] for k in FIELDS], int(lat["start"]))


def _arrays(l):
    lat = {k: np.asarray(getattr(l, k)).copy() for k in FIELDS}
    lat["start"] = l.start
    return lat


def prune(lat, gs, as_, beam):
    """the existing operation -> (lattice, status)"""
    if len(lat["frame"]) == 0:
        return empty(), NO_PATH
    r, st = _host(lat).prune_with_status(float(beam), float(F(gs)), float(F(as_)))
    return _arrays(r), st


def determinize(lat, gs=1.0, as_=1.0, beam=10.0, delta=1.0 / 1024, state_factor=8):
    """-> (the determinized lattice (empty unless SUCCEEDED), status, stats)"""
    stats = dict.fromkeys(STATS, 0)
    stats["in_states"], stats["in_arcs"] = len(lat["frame"]), len(lat["ilabel"])
    N = len(lat["frame"])
    if N == 0:
        return empty(), NO_PATH, stats
    ab, nxt = lat["arc_begin"], lat["nextstate"]
    for s in range(N):
        for a in range(ab[s], ab[s + 1]):
            if nxt[a] <= s:
                return empty(), EPS_LOOP, stats
    X, st = prune(lat, gs, as_, beam)
    if st != SUCCEEDED:
        return empty(), st, stats
    stats["pruned_states"] = len(X["frame"])
    try:
        Y, nd, ms, mc = split(X, gs, as_, delta, state_factor)
    except Scratch:
        return empty(), SCRATCH, stats
    out, st = prune(Y, gs, as_, beam)
    if st != SUCCEEDED:
        return empty(), st, stats
    stats.update(det_states=nd, max_subset=ms, max_closure=mc, out_states=len(out["frame"]), out_arcs=len(out["ilabel"]))
    return out, st, stats
