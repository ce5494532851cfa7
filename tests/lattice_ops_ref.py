"""Best path under scales and beam pruning of a raw lattice, restated in plain float32 Python (the yardstick of
tests/test_lattice_ops_cpu.py and tests/test_gpu_lattice_ops.py).  Written from the rule's text, not from the
C++ or the kernels.

A lattice is a dict of the arrays of khg.Lattice (frame, graph_state, tot_cost, extra_cost, final_cost, arc_begin with one more entry
than states, ilabel, olabel, graph_cost, acoustic_cost, nextstate) plus start.  Every sum and product below is one float32
operation (fl), nothing is contracted.

  arc weights      w1 = fl(gs * graph_cost), w2 = fl(as * acoustic_cost) (0 for an epsilon arc: ilabel == 0); final (fl(gs * final_cost), 0)
  better           (a1, a2) < (b1, b2)  iff  fl(a1 + a2) < fl(b1 + b2), or the sums are equal and a1 < b1
  forward          frame by frame: a state of frame f > 0 starts from INF and takes its emitting in-links in global arc order, then
                   the frame's states take their epsilon in-links in Jacobi rounds (a round reads the values of the round before);
                   a value is replaced only by a strictly better one; `reached` means value1 != INF; a frame of n states may change in
                   rounds 0 .. n, a change in a later round is EPS_LOOP
  final state      the lowest state of the last frame, reached and final, among the best (alpha1 + final, alpha2 + 0)
  best path        the back-pointer chain; its sums are taken again left to right from (0, 0), the final weight last
  backward         frames T .. 0: a state starts from its final weight (last frame only) or INF, takes its emitting out-arcs in arc
                   order, then the frame's states take their epsilon out-arcs in Jacobi rounds, same cap
  prune            best = fl(f1 + f2) of the final state's pair, limit = fl(best + beam); a state is kept iff it is on the best path
                   or alpha and beta are reached and fl(fl(a1 + b1) + fl(a2 + b2)) <= limit; an arc iff both ends are kept and it is
                   on the best path or fl(fl(fl(a1[src] + w1) + b1[dst]) + fl(fl(a2[src] + w2) + b2[dst])) <= limit

numpy only."""
import numpy as np

F = np.float32
INF = F(np.inf)
SUCCEEDED, NO_PATH, EPS_LOOP, WORDS = 1, 8, 16, 32
FIELDS = ("frame", "graph_state", "tot_cost", "extra_cost", "final_cost", "arc_begin", "ilabel", "olabel", "graph_cost", "acoustic_cost", "nextstate")
INTS = ("frame", "graph_state", "arc_begin", "ilabel", "olabel", "nextstate")


def _better(a1, a2, b1, b2):
    sa, sb = F(a1 + a2), F(b1 + b2)
    if sa < sb:
        return True
    if sa > sb:
        return False
    return bool(a1 < b1)


def _weights(lat, gs, as_):
    gs, as_ = F(gs), F(as_)
    il = np.asarray(lat["ilabel"])
    with np.errstate(invalid="ignore"):
        w1 = (gs * np.asarray(lat["graph_cost"], F)).astype(F)
        w2 = np.where(il != 0, (as_ * np.asarray(lat["acoustic_cost"], F)).astype(F), F(0.0)).astype(F)
        fw = (gs * np.asarray(lat["final_cost"], F)).astype(F)
    fw = np.where(np.asarray(lat["final_cost"], F) == INF, INF, fw).astype(F)
    return w1, w2, fw


def _frames(lat):
    """[(lo, hi)] of the states of every frame present, in order"""
    fr = np.asarray(lat["frame"])
    out, lo = [], 0
    while lo < len(fr):
        hi = lo
        while hi < len(fr) and fr[hi] == fr[lo]:
            hi += 1
        out.append((lo, hi))
        lo = hi
    return out


def _src_of(lat):
    ab = np.asarray(lat["arc_begin"])
    src = np.zeros(len(lat["ilabel"]), np.int64)
    for s in range(len(ab) - 1):
        src[ab[s]: ab[s + 1]] = s
    return src


def forward(lat, gs, as_):
    """-> (alpha1, alpha2, back-pointer arc per state, eps_loop)"""
    N = len(lat["frame"])
    w1, w2, _ = _weights(lat, gs, as_)
    il, nx = np.asarray(lat["ilabel"]), np.asarray(lat["nextstate"])
    src = _src_of(lat)
    ins = [[] for _ in range(N)]
    for a in range(len(il)):          # global arc order = (source state, arc) order
        ins[nx[a]].append(a)
    d1, d2, bp = [INF] * N, [INF] * N, [-1] * N
    d1[lat["start"]], d2[lat["start"]] = F(0.0), F(0.0)
    fr = np.asarray(lat["frame"])
    for lo, hi in _frames(lat):
        if fr[lo] > 0:
            for n in range(lo, hi):
                b1, b2 = INF, INF
                for a in ins[n]:
                    m = src[a]
                    if il[a] == 0 or d1[m] == INF:
                        continue
                    c1, c2 = F(d1[m] + w1[a]), F(d2[m] + w2[a])
                    if b1 == INF or _better(c1, c2, b1, b2):
                        b1, b2, bp[n] = c1, c2, a
                d1[n], d2[n] = b1, b2
        rnd = 0
        while True:
            changed = False
            new = {}
            for n in range(lo, hi):
                b1, b2 = d1[n], d2[n]
                for a in ins[n]:
                    m = src[a]
                    if il[a] != 0 or d1[m] == INF:
                        continue
                    c1, c2 = F(d1[m] + w1[a]), F(d2[m] + F(0.0))
                    if b1 == INF or _better(c1, c2, b1, b2):
                        b1, b2, bp[n], changed = c1, c2, a, True
                new[n] = (b1, b2)
            for n in range(lo, hi):
                d1[n], d2[n] = new[n]
            if not changed:
                break
            if rnd > hi - lo:
                return d1, d2, bp, True
            rnd += 1
    return d1, d2, bp, False


def backward(lat, gs, as_):
    """-> (beta1, beta2, eps_loop)"""
    N = len(lat["frame"])
    w1, w2, fw = _weights(lat, gs, as_)
    il, nx, ab, fr = np.asarray(lat["ilabel"]), np.asarray(lat["nextstate"]), np.asarray(lat["arc_begin"]), np.asarray(lat["frame"])
    T = fr[N - 1]
    e1, e2 = [INF] * N, [INF] * N
    for lo, hi in reversed(_frames(lat)):
        for n in range(lo, hi):
            b1, b2 = (fw[n], F(0.0)) if fr[n] == T and fw[n] != INF else (INF, INF)
            for a in range(ab[n], ab[n + 1]):
                k = nx[a]
                if il[a] == 0 or e1[k] == INF:
                    continue
                c1, c2 = F(w1[a] + e1[k]), F(w2[a] + e2[k])
                if b1 == INF or _better(c1, c2, b1, b2):
                    b1, b2 = c1, c2
            e1[n], e2[n] = b1, b2
        rnd = 0
        while True:
            changed = False
            new = {}
            for n in range(lo, hi):
                b1, b2 = e1[n], e2[n]
                for a in range(ab[n], ab[n + 1]):
                    k = nx[a]
                    if il[a] != 0 or e1[k] == INF:
                        continue
                    c1, c2 = F(w1[a] + e1[k]), F(F(0.0) + e2[k])
                    if b1 == INF or _better(c1, c2, b1, b2):
                        b1, b2, changed = c1, c2, True
                new[n] = (b1, b2)
            for n in range(lo, hi):
                e1[n], e2[n] = new[n]
            if not changed:
                break
            if rnd > hi - lo:
                return e1, e2, True
            rnd += 1
    return e1, e2, False


def _final_state(lat, gs, d1, d2):
    N = len(lat["frame"])
    _, _, fw = _weights(lat, gs, 1.0)
    fr = np.asarray(lat["frame"])
    T = fr[N - 1]
    fin, f1, f2 = -1, INF, INF
    for n in range(N):
        if fr[n] != T or d1[n] == INF or fw[n] == INF:
            continue
        c1, c2 = F(d1[n] + fw[n]), F(d2[n] + F(0.0))
        if fin < 0 or _better(c1, c2, f1, f2):
            fin, f1, f2 = n, c1, c2
    return fin, f1, f2


def _chain(lat, bp, fin):
    """the arcs of the back-pointer chain from the start to fin, or None"""
    src = _src_of(lat)
    path, n = [], fin
    while not (n == lat["start"] and bp[n] < 0):
        a = bp[n]
        if a < 0 or len(path) > len(src):
            return None
        path.append(a)
        n = int(src[a])
    return path[::-1]


def best_path(lat, gs=1.0, as_=1.0):
    """-> dict(status, ali, words, weight (v1, v2), arcs (the path's lattice arcs), final (the final state), f (the final pair))"""
    fail = dict(ali=[], words=[], weight=(INF, INF), arcs=[], final=-1, f=(INF, INF))
    if len(lat["frame"]) == 0 or lat["start"] < 0:
        return dict(fail, status=NO_PATH)
    d1, d2, bp, loop = forward(lat, gs, as_)
    if loop:
        return dict(fail, status=EPS_LOOP)
    fin, f1, f2 = _final_state(lat, gs, d1, d2)
    path = _chain(lat, bp, fin) if fin >= 0 else None
    if path is None:
        return dict(fail, status=NO_PATH)
    w1, w2, fw = _weights(lat, gs, as_)
    v1, v2 = F(0.0), F(0.0)
    for a in path:
        v1, v2 = F(v1 + w1[a]), F(v2 + w2[a])
    v1, v2 = F(v1 + fw[fin]), F(v2 + F(0.0))
    return dict(status=SUCCEEDED, ali=[int(lat["ilabel"][a]) for a in path if lat["ilabel"][a] != 0],
                words=[int(lat["olabel"][a]) for a in path if lat["olabel"][a] != 0], weight=(v1, v2), arcs=path, final=fin, f=(f1, f2),
                alpha=(d1, d2))


def empty_lattice():
    out = {k: np.zeros(0, np.int32 if k in INTS else np.float32) for k in FIELDS}
    out["arc_begin"] = np.zeros(1, np.int32)
    out["start"] = -1
    return out


def prune(lat, beam, gs=1.0, as_=1.0):
    """-> (pruned lattice, status); the kept state and arc index lists ride along as "kept_states" / "kept_arcs" """
    bp_ = best_path(lat, gs, as_)
    if bp_["status"] != SUCCEEDED:
        return dict(empty_lattice(), kept_states=[], kept_arcs=[]), bp_["status"]
    e1, e2, loop = backward(lat, gs, as_)
    if loop:
        return dict(empty_lattice(), kept_states=[], kept_arcs=[]), EPS_LOOP
    d1, d2 = bp_["alpha"]
    w1, w2, _ = _weights(lat, gs, as_)
    N = len(lat["frame"])
    ab, nx = np.asarray(lat["arc_begin"]), np.asarray(lat["nextstate"])
    src = _src_of(lat)
    limit = F(F(bp_["f"][0] + bp_["f"][1]) + F(beam))
    on_arc = set(bp_["arcs"])
    on_state = {lat["start"], bp_["final"]} | {int(nx[a]) for a in on_arc} | {int(src[a]) for a in on_arc}
    keep = []
    for s in range(N):
        ok = d1[s] != INF and e1[s] != INF and bool(F(F(d1[s] + e1[s]) + F(d2[s] + e2[s])) <= limit)
        keep.append(ok or s in on_state)
    newid, n = [-1] * N, 0
    for s in range(N):
        if keep[s]:
            newid[s] = n
            n += 1
    out = {k: [] for k in FIELDS}
    kept_arcs = []
    for s in range(N):
        if not keep[s]:
            continue
        for k in ("frame", "graph_state", "tot_cost", "extra_cost", "final_cost"):
            out[k].append(lat[k][s])
        out["arc_begin"].append(len(out["ilabel"]))
        for a in range(ab[s], ab[s + 1]):
            if not keep[nx[a]]:
                continue
            with np.errstate(invalid="ignore"):
                tot = F(F(F(d1[s] + w1[a]) + e1[nx[a]]) + F(F(d2[s] + w2[a]) + e2[nx[a]]))
            if not (bool(tot <= limit) or a in on_arc):
                continue
            kept_arcs.append(a)
            for k in ("ilabel", "olabel", "graph_cost", "acoustic_cost"):
                out[k].append(lat[k][a])
            out["nextstate"].append(newid[nx[a]])
    out["arc_begin"].append(len(out["ilabel"]))
    res = {k: np.asarray(v, np.int32 if k in INTS else np.float32) for k, v in out.items()}
    res["start"] = newid[lat["start"]]
    res["kept_states"] = [s for s in range(N) if keep[s]]
    res["kept_arcs"] = kept_arcs
    return res, SUCCEEDED


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32).tolist()
