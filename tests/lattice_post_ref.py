"""Forward-backward posteriors of a raw lattice, restated in plain Python from the text of DESIGN.md section 7g (not from the C++ or
the kernels): a float64 pass, serial in state order, every log-sum a left fold of log-adds; the same in 60-digit `decimal` for
lattices small enough for it; and `enumerate_paths`, the brute-force sum over all start -> final paths with math.fsum, for hand-built
lattices of a few hundred paths.  A lattice is the dict of arrays of tests/lattice_ops_ref.py (FIELDS, "start")."""
import decimal
import math

import numpy as np

SUCCEEDED, NO_PATH, EPS_LOOP = 1, 8, 16
NINF = float("-inf")
F = np.float32


def _arcs(lat):
    """[(src, dst, ilabel, graph_cost, acoustic_cost)] in arc order, as Python numbers"""
    ab = lat["arc_begin"]
    out = []
    for s in range(len(lat["frame"])):
        for a in range(int(ab[s]), int(ab[s + 1])):
            out.append((s, int(lat["nextstate"][a]), int(lat["ilabel"][a]), float(lat["graph_cost"][a]), float(lat["acoustic_cost"][a])))
    return out


def admissible(lat):
    """every epsilon arc goes to a higher state number (emitting arcs do: khg_lattices_validate)"""
    return all(d > s for s, d, il, _, _ in _arcs(lat) if il == 0)


def _failed(status):
    return {"status": status, "tot": NINF, "alpha": [], "beta": [], "arc_post": np.zeros(0), "post": [], "merged": [], "live": []}


def _logadd(a, b):
    if a == NINF:
        return b
    if b == NINF:
        return a
    m, n = (a, b) if a >= b else (b, a)
    return m + math.log1p(math.exp(n - m))


def _posts(lat, arcs, live, arc_post, T):
    """per frame 0 .. T - 1: [(tid, weight)] ascending, and how many arcs each entry merges.  An entry exists when one of its arcs
    is live (both ends reached), whatever its weight."""
    post = [dict() for _ in range(T)]
    cnt = [dict() for _ in range(T)]
    for a, (s, d, il, _, _) in enumerate(arcs):
        if il == 0 or not live[a]:
            continue
        t = int(lat["frame"][s])
        post[t][il] = post[t].get(il, 0.0) + arc_post[a]          # (arc order)
        cnt[t][il] = cnt[t].get(il, 0) + 1
    return [sorted(p.items()) for p in post], [[c[k] for k in sorted(c)] for c in cnt]


def forward_backward(lat, gs=1.0, as_=1.0):
    """-> {"status", "tot", "alpha", "beta", "arc_post", "post", "merged", "live"}.  gs, as_ are float32 values widened to double."""
    gs, as_ = float(F(gs)), float(F(as_))
    N = len(lat["frame"])
    if N == 0 or lat["start"] < 0:
        return _failed(NO_PATH)
    if not admissible(lat):
        return _failed(EPS_LOOP)
    arcs = _arcs(lat)
    T = int(lat["frame"][-1])
    w = [-(gs * g + (as_ * ac if il != 0 else 0.0)) for _, _, il, g, ac in arcs]
    fin = [-(gs * float(c)) if int(f) == T and c != np.inf else NINF for f, c in zip(lat["frame"], lat["final_cost"])]
    alpha = [NINF] * N
    alpha[int(lat["start"])] = 0.0
    for a, (s, d, _, _, _) in enumerate(arcs):                  # arcs by source state; every arc goes up: alpha[s] is complete
        if alpha[s] != NINF:
            alpha[d] = _logadd(alpha[d], alpha[s] + w[a])
    tot = NINF
    for s in range(N):
        if fin[s] != NINF and alpha[s] != NINF:
            tot = _logadd(tot, alpha[s] + fin[s])
    if tot == NINF:
        return _failed(NO_PATH)
    beta = list(fin)
    ab = lat["arc_begin"]
    for s in range(N - 1, -1, -1):
        for a in range(int(ab[s]), int(ab[s + 1])):
            d = arcs[a][1]
            if beta[d] != NINF:
                beta[s] = _logadd(beta[s], w[a] + beta[d])
    live = [alpha[s] != NINF and beta[d] != NINF for s, d, _, _, _ in arcs]
    arc_post = np.array([math.exp(alpha[s] + w[a] + beta[d] - tot) if live[a] else 0.0 for a, (s, d, _, _, _) in enumerate(arcs)], np.float64)
    post, merged = _posts(lat, arcs, live, arc_post, T)
    return {"status": SUCCEEDED, "tot": tot, "alpha": alpha, "beta": beta, "arc_post": arc_post, "post": post, "merged": merged, "live": live}


def forward_backward_decimal(lat, gs=1.0, as_=1.0, digits=60):
    """the same evaluated in `digits`-digit decimal arithmetic (an admissible lattice with a path), rounded to float64 at the end"""
    D = decimal.Decimal
    with decimal.localcontext() as ctx:
        ctx.prec = digits
        gs, as_ = D(float(F(gs))), D(float(F(as_)))
        N = len(lat["frame"])
        arcs = _arcs(lat)
        T = int(lat["frame"][-1])
        w = [-(gs * D(g) + (as_ * D(ac) if il != 0 else D(0))) for _, _, il, g, ac in arcs]
        fin = [-(gs * D(float(c))) if int(f) == T and c != np.inf else None for f, c in zip(lat["frame"], lat["final_cost"])]

        def add(a, b):              # linear domain would overflow: log-add, exactly enough at 60 digits
            if a is None:
                return b
            if b is None:
                return a
            m, n = (a, b) if a >= b else (b, a)
            return m + (D(1) + (n - m).exp()).ln()

        alpha = [None] * N
        alpha[int(lat["start"])] = D(0)
        for a, (s, d, _, _, _) in enumerate(arcs):
            if alpha[s] is not None:
                alpha[d] = add(alpha[d], alpha[s] + w[a])
        tot = None
        for s in range(N):
            if fin[s] is not None and alpha[s] is not None:
                tot = add(tot, alpha[s] + fin[s])
        assert tot is not None
        beta = list(fin)
        ab = lat["arc_begin"]
        for s in range(N - 1, -1, -1):
            for a in range(int(ab[s]), int(ab[s + 1])):
                d = arcs[a][1]
                if beta[d] is not None:
                    beta[s] = add(beta[s], w[a] + beta[d])
        live = [alpha[s] is not None and beta[d] is not None for s, d, _, _, _ in arcs]
        arc_post = np.array([float((alpha[s] + w[a] + beta[d] - tot).exp()) if live[a] else 0.0 for a, (s, d, _, _, _) in enumerate(arcs)], np.float64)
        fl = lambda x: NINF if x is None else float(x)  # noqa: E731
        post, merged = _posts(lat, arcs, live, arc_post, T)
        return {"status": SUCCEEDED, "tot": float(tot), "alpha": [fl(x) for x in alpha], "beta": [fl(x) for x in beta], "arc_post": arc_post,
                "post": post, "merged": merged, "live": live}


def enumerate_paths(lat, gs=1.0, as_=1.0, limit=100000):
    """brute force: every start -> final path's log-likelihood; -> (tot, arc_post) with the sums by math.fsum in the linear domain
    (hand-built lattices: the likelihoods are far from underflow)"""
    gs, as_ = float(F(gs)), float(F(as_))
    arcs = _arcs(lat)
    ab = lat["arc_begin"]
    T = int(lat["frame"][-1])
    paths = []

    def walk(s, ll, used):
        assert len(paths) <= limit
        if int(lat["frame"][s]) == T and lat["final_cost"][s] != np.inf:
            paths.append((ll - gs * float(lat["final_cost"][s]), tuple(used)))
        for a in range(int(ab[s]), int(ab[s + 1])):
            _, d, il, g, ac = arcs[a]
            walk(d, ll - (gs * g + (as_ * ac if il != 0 else 0.0)), used + [a])

    walk(int(lat["start"]), 0.0, [])
    assert paths
    top = max(p[0] for p in paths)
    z = math.fsum(math.exp(p[0] - top) for p in paths)
    post = np.array([math.fsum(math.exp(p[0] - top) for p in paths if a in p[1]) / z for a in range(len(arcs))], np.float64)
    return top + math.log(z), post, len(paths)


def tolerances(want, lat):
    """(tol_log, tol_post) of DESIGN.md 7g from the yardstick `want`: M = max(1, the largest finite |alpha|, |beta|)"""
    vals = [abs(x) for x in list(want["alpha"]) + list(want["beta"]) if x != NINF]
    M = max([1.0] + vals)
    tol_log = 8 * 2.0 ** -52 * M * (len(lat["frame"]) + len(lat["ilabel"]))
    return tol_log, 3 * tol_log + 2.0 ** -50


def compare(got, want, lat, tag=None):
    """`got`: {"status", "tot", "arc_post", "post"} (and, when present, "alpha" / "beta") of the code under test.  Status, list
    structure and exact zeros must be equal; values within the derived tolerance.  -> the largest error / bound ratio."""
    assert got["status"] == want["status"], (tag, got["status"], want["status"])
    if want["status"] != SUCCEEDED:
        assert got["tot"] == NINF and len(got["arc_post"]) == 0 and len(got["post"]) == 0, tag
        return 0.0
    tol_log, tol_post = tolerances(want, lat)
    worst = abs(got["tot"] - want["tot"]) / tol_log
    for k in ("alpha", "beta"):
        if k in got and len(got[k]):
            g, w = np.asarray(got[k], np.float64), np.asarray(want[k], np.float64)
            assert ((g == NINF) == (w == NINF)).all(), (tag, k)
            fin = w != NINF
            if fin.any():
                worst = max(worst, float(np.abs(g[fin] - w[fin]).max()) / tol_log)
    ga, wa = np.asarray(got["arc_post"], np.float64), want["arc_post"]
    assert ga.shape == wa.shape, (tag, ga.shape, wa.shape)
    dead = ~np.asarray(want["live"], bool)
    assert (ga[dead] == 0.0).all() and not np.signbit(ga[dead]).any(), tag
    if len(wa):
        worst = max(worst, float(np.abs(ga - wa).max()) / tol_post)
    assert len(got["post"]) == len(want["post"]), (tag, len(got["post"]), len(want["post"]))
    for t, (gp, wp, mc) in enumerate(zip(got["post"], want["post"], want["merged"])):
        assert [int(x[0]) for x in gp] == [x[0] for x in wp], (tag, t, gp, wp)
        for (_, gw), (_, ww), m in zip(gp, wp, mc):
            worst = max(worst, abs(gw - ww) / (m * tol_post))
    assert worst <= 1.0, (tag, worst)
    return worst
