"""The raw lattice of the lattice-simple decoder, two ways (the yardsticks of tests/test_lattice_raw_cpu.py and
tests/test_gpu_lattice_raw.py).

rule_lattice: a plain float32 restatement of the rule the GPU kernels follow -- the order-independent lattice.  Dense rows per
frame, as in the decoder kernel: D (token costs), R (PruneCurrentTokens' survivors), pcut / ecut (the cutoffs), X (the exact extra
costs of FinalizeDecoding).  Then
  state  (f, s): D[f][s] != INF and X[f][s] != INF, numbered by frame, then by graph state
  emitting link (f, m) -> (f + 1, k): tot = (D[f][m] + ac) + g < pcut[f + 1] and R[f + 1][k]
  epsilon link  (f, m) -> (f, k):     D[f][m] + g < ecut[f]
  either survives iff its link extra cost (the kernel's association order) is <= lattice_beam
  arcs per state in the order of the graph's arcs in that state; final weights on the last frame's final states.

walk_lattice: the raw lattice read off a finished lattice_simple_ref.LatticeSimpleDecoder (the reference's GetRawLattice,
lattice-simple-decoder.cc:654-735, for one walk order of its hash maps): tokens keyed (frame, state), links keyed (frame, state,
arc index), with their costs.

numpy only."""
import numpy as np

F = np.float32
INF = F(np.inf)


def rule_rows(g, cfg, ll, T):
    """Passes 1 and 2 of the decoder kernel on a lattice_faster_ref.Graph -> dict(D, R, pcut, ecut, X), or None when the utterance
    does not decode (Quirk 1, a NaN link, a negative epsilon cycle, no final state live at the end, no frames)."""
    S = len(g.final)
    beam, lbeam = F(cfg.beam), F(cfg.lattice_beam)
    D = [[INF] * S for _ in range(T + 1)]
    R = [[False] * S for _ in range(T + 1)]
    pcut, ecut = [INF] * (T + 1), [INF] * (T + 1)

    def closure(row, cut):
        for _ in range(S + 3):
            changed = False
            for s in range(S):
                if row[s] == INF:
                    continue
                for a in g.arcs(s):
                    if g.ilabel[a] != 0:
                        continue
                    tot = F(row[s] + g.weight[a])
                    if tot < cut and tot < row[g.nextstate[a]]:
                        row[g.nextstate[a]] = tot
                        changed = True
            if not changed:
                return True
        return False

    if g.start < 0 or g.num_ieps[g.start] == 0 or T <= 0:
        return None
    D[0][g.start] = F(0.0)
    ecut[0] = F(F(0.0) + beam)
    if not closure(D[0], ecut[0]):
        return None
    for t in range(T):
        Dn = D[t + 1]
        for s in range(S):
            if D[t][s] == INF:
                continue
            for a in g.arcs(s):
                if g.ilabel[a] == 0:
                    continue
                tot = F(F(D[t][s] + F(-ll(t, g.ilabel[a]))) + g.weight[a])
                if tot != tot:
                    return None
                if tot < Dn[g.nextstate[a]]:
                    Dn[g.nextstate[a]] = tot
        best = min(Dn)
        pc = F(min(F(1.0e10), best) + beam)
        best2, eps = INF, False
        for s in range(S):
            keep = bool(Dn[s] < pc)
            R[t + 1][s] = keep
            if keep:
                best2 = min(best2, Dn[s])
                eps = eps or g.num_ieps[s] != 0
            else:
                Dn[s] = INF
        if not eps:
            return None
        pcut[t + 1], ecut[t + 1] = pc, F(best2 + beam)
        if not closure(Dn, ecut[t + 1]):
            return None
    live = [s for s in range(S) if D[T][s] != INF]
    if not any(g.final[s] != INF for s in live):
        return None
    best_cost = min(D[T][s] for s in live)
    bcwf = min(F(D[T][s] + g.final[s]) for s in live)
    fbc = bcwf if bcwf != INF else best_cost
    X = [[INF if D[f][s] == INF else F(0.0) for s in range(S)] for f in range(T + 1)]
    rows = dict(D=D, R=R, pcut=pcut, ecut=ecut, X=X, T=T, S=S)
    for f in range(T, -1, -1):
        changed = True
        while changed:
            changed = False
            for m in range(S):
                if D[f][m] == INF:
                    continue
                te = F(F(D[f][m] + g.final[m]) - fbc) if f == T else INF
                for a in g.arcs(m):
                    le = link_extra(g, rows, ll, lbeam, f, m, a)
                    if le is None or le[0] > lbeam:
                        continue
                    v = F(0.0) if le[0] < 0.0 else le[0]
                    if v < te:
                        te = v
                if f == T and te > lbeam:
                    te = INF
                if not (te == X[f][m]):
                    X[f][m] = te
                    changed = True
    return rows


def link_extra(g, rows, ll, lbeam, f, m, a):
    """The link of arc a from the live token (f, m): None when it does not exist, else (link extra cost, graph cost, acoustic cost,
    destination (frame, state))."""
    D, X, R, T = rows["D"], rows["X"], rows["R"], rows["T"]
    dm, w, k = D[f][m], g.weight[a], g.nextstate[a]
    if g.ilabel[a] != 0:
        if f == T:
            return None
        ac = F(-ll(f, g.ilabel[a]))
        tot = F(F(dm + ac) + w)
        if not (tot < rows["pcut"][f + 1]) or not R[f + 1][k]:
            return None
        with np.errstate(invalid="ignore"):
            return F(X[f + 1][k] + F(tot - D[f + 1][k])), w, ac, (f + 1, k)
    if not (F(dm + w) < rows["ecut"][f]):
        return None
    with np.errstate(invalid="ignore"):
        return F(X[f][k] + F(F(F(dm + F(0.0)) + w) - D[f][k])), w, F(0.0), (f, k)


def rule_lattice(g, cfg, ll, T):
    """-> None when the utterance does not decode, else the lattice as the arrays of khg.Lattice (states by frame, then graph state;
    arcs per state in graph order; arc_begin with one more entry) plus arc_index (the graph arc of every lattice arc), `excised` (links
    that passed their cutoff and fell to lattice_beam) and `paths_gt_1` (some state has more than one surviving in-link or is final
    next to another final state: more than one path)."""
    rows = rule_rows(g, cfg, ll, T)
    if rows is None:
        return None
    D, X, S = rows["D"], rows["X"], rows["S"]
    lbeam = F(cfg.lattice_beam)
    sid = {}
    for f in range(T + 1):
        for s in range(S):
            if D[f][s] != INF and X[f][s] != INF:
                sid[(f, s)] = len(sid)
    out = {k: [] for k in ("frame", "graph_state", "tot_cost", "extra_cost", "final_cost", "arc_begin", "ilabel", "olabel", "graph_cost",
                           "acoustic_cost", "nextstate", "arc_index")}
    excised = 0
    for (f, s) in sid:
        out["frame"].append(f); out["graph_state"].append(s); out["tot_cost"].append(D[f][s]); out["extra_cost"].append(X[f][s])
        out["final_cost"].append(g.final[s] if f == T else INF)
        out["arc_begin"].append(len(out["ilabel"]))
        for a in g.arcs(s):
            le = link_extra(g, rows, ll, lbeam, f, s, a)
            if le is None:
                continue
            if not (le[0] <= lbeam):
                excised += 1
                continue
            out["ilabel"].append(g.ilabel[a]); out["olabel"].append(g.olabel[a]); out["graph_cost"].append(le[1])
            out["acoustic_cost"].append(le[2]); out["nextstate"].append(sid[le[3]]); out["arc_index"].append(a)
    # links out of tokens that did not survive are excised too (their own extra cost is INF): counted for the tests' evidence
    for f in range(T + 1):
        for s in range(S):
            if D[f][s] != INF and X[f][s] == INF:
                excised += sum(1 for a in g.arcs(s) if link_extra(g, rows, ll, lbeam, f, s, a) is not None)
    out["arc_begin"].append(len(out["ilabel"]))
    ints = ("frame", "graph_state", "arc_begin", "ilabel", "olabel", "nextstate", "arc_index")
    lat = {k: np.asarray(v, np.int32 if k in ints else np.float32) for k, v in out.items()}
    lat["start"] = sid.get((0, g.start), -1)
    lat["excised"] = excised
    indeg = np.bincount(lat["nextstate"], minlength=len(sid)) if len(sid) else np.zeros(0, np.int64)
    lat["paths_gt_1"] = bool((indeg > 1).any()) or int((lat["final_cost"] != INF).sum()) > 1
    lat["rows"] = rows
    return lat


def lattice_sets(lat):
    """The arrays of a lattice (rule_lattice's dict) -> (tokens {(f, s): (tot, extra)}, links {(f, s, graph arc): (ilabel, olabel,
    graph cost, acoustic cost, (f', s'))}): the form walk_lattice gives."""
    toks, links = {}, {}
    fr, gs = lat["frame"], lat["graph_state"]
    for i in range(len(fr)):
        toks[(int(fr[i]), int(gs[i]))] = (lat["tot_cost"][i], lat["extra_cost"][i])
        for j in range(int(lat["arc_begin"][i]), int(lat["arc_begin"][i + 1])):
            n = int(lat["nextstate"][j])
            links[(int(fr[i]), int(gs[i]), int(lat["arc_index"][j]))] = (int(lat["ilabel"][j]), int(lat["olabel"][j]), lat["graph_cost"][j],
                                                                        lat["acoustic_cost"][j], (int(fr[n]), int(gs[n])))
    return toks, links


def walk_lattice(dec):
    """GetRawLattice off a finished lattice_simple_ref.LatticeSimpleDecoder (decode() returned True) -> (tokens, links) as
    lattice_sets gives them; finals {(T, s): final cost}."""
    toks, links, finals = {}, {}, {}
    T = dec.num_frames_decoded()
    for f in range(T + 1):
        for tok in dec.active_toks[f]:
            assert (f, tok.state) not in toks, "two surviving tokens of one state on a frame"
            toks[(f, tok.state)] = (tok.tot_cost, tok.extra_cost)
            if f == T and tok.uid in dec.final_costs:
                finals[(f, tok.state)] = dec.final_costs[tok.uid]
            for link in tok.links:
                nf = f + 1 if link.ilabel != 0 else f
                links[(f, tok.state, link.arc)] = (link.ilabel, link.olabel, link.graph_cost, link.acoustic_cost, (nf, link.next_tok.state))
    return toks, links, finals


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32).tolist() if np.ndim(x) else int(np.asarray(x, np.float32).view(np.uint32))


def same_token(a, b):
    return bits(a[0]) == bits(b[0]) and bits(a[1]) == bits(b[1])


def same_link(a, b):
    return a[0] == b[0] and a[1] == b[1] and bits(a[2]) == bits(b[2]) and bits(a[3]) == bits(b[3]) and a[4] == b[4]


def path_like(lin):
    """`like` of a LinearLattice the way the decoder kernel sums it: float32, left to right from One(), then the final weight."""
    v1, v2 = F(0.0), F(0.0)
    for a in lin.arcs:
        v1, v2 = F(v1 + F(a.weight.value1)), F(v2 + F(a.weight.value2))
    v1, v2 = F(v1 + F(lin.final.value1)), F(v2 + F(0.0))
    return float(F(-F(v1 + v2)))
