"""MPE / sMBR posteriors of a raw lattice, restated in plain Python from the text of DESIGN.md section 7k (not from the C++ or the
kernel): a float64 pass that takes alpha, beta and tot from the section 7g restatement (tests/lattice_post_ref.py) and folds the
forward and backward accuracies left to right in the rule's order; the same in 60-digit `decimal`, in the linear domain; and
`enumerate_paths`, the brute-force sum over all start -> final paths.  A lattice is the dict of arrays of tests/lattice_ops_ref.py.
A reference is (tid2phone, tid2pdf, silence_phones, alignment): two tables [num_tids + 1], a set of phones, one id per frame."""
import decimal
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lattice_post_ref as pr  # noqa: E402

SUCCEEDED, NO_PATH, EPS_LOOP, NO_REF = pr.SUCCEEDED, pr.NO_PATH, pr.EPS_LOOP, 512
NINF = pr.NINF
F = np.float32


def ref_ok(lat, tid2phone, alignment):
    """boost's three conditions, negated: an alignment, of the lattice's frame count, every id in 1 .. num_tids"""
    T = int(lat["frame"][-1])
    return len(alignment) > 0 and len(alignment) == T and all(1 <= int(x) <= len(tid2phone) - 1 for x in alignment)


def arc_acc(lat, arcs, tid2phone, tid2pdf, silence_phones, alignment, criterion, one_silence_class):
    """the frame accuracy of every arc: 0 or 1"""
    T = int(lat["frame"][-1])
    sil = lambda x: int(tid2phone[x]) in silence_phones  # noqa: E731
    out = []
    for s, _, il, _, _ in arcs:
        t = int(lat["frame"][s])
        if il == 0 or t >= T:
            out.append(0)
            continue
        r = int(alignment[t])
        match = int(tid2pdf[il]) == int(tid2pdf[r]) if criterion == "smbr" else int(tid2phone[il]) == int(tid2phone[r])
        out.append(int((match or (sil(il) and sil(r))) if one_silence_class else (match and not sil(il))))
    return out


def _failed(status):
    r = pr._failed(status)
    r.update({"avg": 0.0, "A": [], "B": [], "g": np.zeros(0), "acc": []})
    return r


def forward_backward_mpe(lat, tid2phone, tid2pdf, silence_phones, alignment, criterion="smbr", one_silence_class=True, gs=1.0, as_=1.0):
    """-> {"status", "tot", "avg", "alpha", "beta", "A", "B", "g", "arc_post" (the signed d), "post", "merged", "live", "acc"}"""
    assert criterion in ("smbr", "mpfe")
    N = len(lat["frame"])
    if N == 0 or lat["start"] < 0:
        return _failed(NO_PATH)
    if not ref_ok(lat, tid2phone, alignment):
        return _failed(NO_REF)
    fb = pr.forward_backward(lat, gs, as_)
    if fb["status"] != SUCCEEDED:
        return _failed(fb["status"])
    gs, as_ = float(F(gs)), float(F(as_))
    arcs = pr._arcs(lat)
    T = int(lat["frame"][-1])
    w = [-(gs * g + (as_ * ac if il != 0 else 0.0)) for _, _, il, g, ac in arcs]
    fin = [-(gs * float(c)) if int(f) == T and c != np.inf else NINF for f, c in zip(lat["frame"], lat["final_cost"])]
    alpha, beta, tot = fb["alpha"], fb["beta"], fb["tot"]
    acc = arc_acc(lat, arcs, tid2phone, tid2pdf, silence_phones, alignment, criterion, one_silence_class)
    start = int(lat["start"])
    ins = [[] for _ in range(N)]
    for a, (_, d, _, _, _) in enumerate(arcs):
        ins[d].append(a)                                   # in-arc index order: global arc order
    A = [0.0] * N
    for s in range(N):                                     # every arc goes up: the sources are complete
        if s == start or alpha[s] == NINF:
            continue
        x = 0.0
        for a in ins[s]:
            src = arcs[a][0]
            if alpha[src] != NINF:
                x += math.exp((alpha[src] + w[a]) - alpha[s]) * (A[src] + acc[a])
        A[s] = x
    avg = 0.0
    for s in range(N):
        if fin[s] != NINF and alpha[s] != NINF:
            avg += math.exp((alpha[s] + fin[s]) - tot) * A[s]
    B = [0.0] * N
    ab = lat["arc_begin"]
    for s in range(N - 1, -1, -1):
        if beta[s] == NINF:
            continue
        x = 0.0
        for a in range(int(ab[s]), int(ab[s + 1])):
            d = arcs[a][1]
            if beta[d] != NINF:
                x += math.exp((w[a] + beta[d]) - beta[s]) * (acc[a] + B[d])
        B[s] = x
    live = fb["live"]
    g = np.array([math.exp(((alpha[s] + w[a]) + beta[d]) - tot) if live[a] else 0.0 for a, (s, d, _, _, _) in enumerate(arcs)], np.float64)
    dd = np.array([g[a] * (((A[s] + acc[a]) + B[d]) - avg) if live[a] else 0.0 for a, (s, d, _, _, _) in enumerate(arcs)], np.float64)
    post, merged = pr._posts(lat, arcs, live, dd, T)
    return {"status": SUCCEEDED, "tot": tot, "avg": avg, "alpha": alpha, "beta": beta, "A": A, "B": B, "g": g, "arc_post": dd, "post": post,
            "merged": merged, "live": live, "acc": acc}


def forward_backward_mpe_decimal(lat, tid2phone, tid2pdf, silence_phones, alignment, criterion="smbr", one_silence_class=True, gs=1.0, as_=1.0,
                                 digits=60):
    """the same in `digits`-digit decimal arithmetic, in the linear domain (decimal's exponent range holds every path weight), rounded to
    float64 at the end (an admissible lattice with a path and a reference)"""
    D = decimal.Decimal
    with decimal.localcontext() as ctx:
        ctx.prec = digits
        gs, as_ = D(float(F(gs))), D(float(F(as_)))
        N = len(lat["frame"])
        arcs = pr._arcs(lat)
        T = int(lat["frame"][-1])
        ew = [(-(gs * D(g) + (as_ * D(ac) if il != 0 else D(0)))).exp() for _, _, il, g, ac in arcs]
        efin = [(-(gs * D(float(c)))).exp() if int(f) == T and c != np.inf else None for f, c in zip(lat["frame"], lat["final_cost"])]
        acc = arc_acc(lat, arcs, tid2phone, tid2pdf, silence_phones, alignment, criterion, one_silence_class)
        start = int(lat["start"])
        al = [None] * N                                    # exp(alpha), and exp(alpha) A
        aA = [D(0)] * N
        al[start] = D(1)
        for a, (s, d, _, _, _) in enumerate(arcs):         # arcs by source state; every arc goes up
            if al[s] is not None:
                al[d] = (al[d] or D(0)) + al[s] * ew[a]
                if d != start:
                    aA[d] += ew[a] * (aA[s] + al[s] * acc[a])
        aA[start] = D(0)
        tot = sum((al[s] * efin[s] for s in range(N) if efin[s] is not None and al[s] is not None), D(0))
        assert tot > 0
        avg = sum((aA[s] * efin[s] for s in range(N) if efin[s] is not None and al[s] is not None), D(0)) / tot
        be = list(efin)
        bB = [D(0)] * N
        ab = lat["arc_begin"]
        for s in range(N - 1, -1, -1):
            for a in range(int(ab[s]), int(ab[s + 1])):
                d = arcs[a][1]
                if be[d] is not None:
                    be[s] = (be[s] or D(0)) + ew[a] * be[d]
                    bB[s] += ew[a] * (be[d] * acc[a] + bB[d])
        live = [al[s] is not None and be[d] is not None for s, d, _, _, _ in arcs]
        A = [float(aA[s] / al[s]) if al[s] is not None else 0.0 for s in range(N)]
        B = [float(bB[s] / be[s]) if be[s] is not None else 0.0 for s in range(N)]
        dd = np.zeros(len(arcs))
        g = np.zeros(len(arcs))
        for a, (s, d, _, _, _) in enumerate(arcs):
            if live[a]:
                ga = al[s] * ew[a] * be[d] / tot
                g[a] = float(ga)
                dd[a] = float(ga * (aA[s] / al[s] + acc[a] + bB[d] / be[d] - avg))
        fl = lambda x: NINF if x is None else float(x.ln())  # noqa: E731
        post, merged = pr._posts(lat, arcs, live, dd, T)
        return {"status": SUCCEEDED, "tot": float(tot.ln()), "avg": float(avg), "alpha": [fl(x) for x in al], "beta": [fl(x) for x in be], "A": A, "B": B,
                "g": g, "arc_post": dd, "post": post, "merged": merged, "live": live, "acc": acc}


def enumerate_paths(lat, tid2phone, tid2pdf, silence_phones, alignment, criterion="smbr", one_silence_class=True, gs=1.0, as_=1.0, limit=100000):
    """brute force: avg = sum_path p(path) acc(path), d[a] = sum_{paths through a} p(path) (acc(path) - avg), the sums by math.fsum
    -> (avg, d, number of paths)"""
    gs, as_ = float(F(gs)), float(F(as_))
    arcs = pr._arcs(lat)
    acc = arc_acc(lat, arcs, tid2phone, tid2pdf, silence_phones, alignment, criterion, one_silence_class)
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
    pacc = [sum(acc[a] for a in p[1]) for p in paths]
    avg = math.fsum(math.exp(p[0] - top) * c for p, c in zip(paths, pacc)) / z
    d = np.array([math.fsum(math.exp(p[0] - top) * (c - avg) for p, c in zip(paths, pacc) if a in p[1]) / z for a in range(len(arcs))], np.float64)
    return avg, d, len(paths)


def longest_path_states(lat):
    """the number of states on the longest path of an admissible lattice (every arc goes up)"""
    N = len(lat["frame"])
    depth = [1] * N
    for s, d, _, _, _ in pr._arcs(lat):
        depth[d] = max(depth[d], depth[s] + 1)
    return max(depth)


def tolerances(want, lat):
    """(tol_acc, tol_avg, tol_d) of DESIGN.md 7k from the yardstick `want`: with tol_post of 7g, T the frame count and L the number of
    states on the longest path, 2 tol_post (T + 1) L for A and B, 2 tol_post (T + 1) (L + 1) for avg, tol_post (T + 1) (6 L + 3) for d"""
    _, tol_post = pr.tolerances(want, lat)
    T, L = int(lat["frame"][-1]), longest_path_states(lat)
    return 2 * tol_post * (T + 1) * L, 2 * tol_post * (T + 1) * (L + 1), tol_post * (T + 1) * (6 * L + 3)


def compare(got, want, lat, tag=None):
    """`got`: {"status", "tot", "avg", "arc_post", "post"} (and, when present, "A" / "B") of the code under test.  Status, list structure
    and exact zeros must be equal; values within the derived tolerance.  -> the largest error / bound ratio."""
    assert got["status"] == want["status"], (tag, got["status"], want["status"])
    if want["status"] != SUCCEEDED:
        assert got["tot"] == NINF and got["avg"] == 0.0 and len(got["arc_post"]) == 0 and len(got["post"]) == 0, tag
        return 0.0
    tol_log, _ = pr.tolerances(want, lat)
    tol_acc, tol_avg, tol_d = tolerances(want, lat)
    assert abs(got["tot"] - want["tot"]) <= tol_log, tag
    worst = abs(got["avg"] - want["avg"]) / tol_avg
    for k in ("A", "B"):
        if k in got and len(got[k]):
            worst = max(worst, float(np.abs(np.asarray(got[k], np.float64) - np.asarray(want[k], np.float64)).max()) / tol_acc)
    ga, wa = np.asarray(got["arc_post"], np.float64), want["arc_post"]
    assert ga.shape == wa.shape, (tag, ga.shape, wa.shape)
    dead = ~np.asarray(want["live"], bool)
    assert (ga[dead] == 0.0).all() and not np.signbit(ga[dead]).any(), tag
    if len(wa):
        worst = max(worst, float(np.abs(ga - wa).max()) / tol_d)
    assert len(got["post"]) == len(want["post"]), (tag, len(got["post"]), len(want["post"]))
    for t, (gp, wp, mc) in enumerate(zip(got["post"], want["post"], want["merged"])):
        assert [int(x[0]) for x in gp] == [x[0] for x in wp], (tag, t, gp, wp)
        for (_, gw), (_, ww), m in zip(gp, wp, mc):
            worst = max(worst, abs(gw - ww) / (m * tol_d))
    assert worst <= 1.0, (tag, worst)
    return worst


def count_significant(want, lat):
    """entries whose |weight| exceeds 100 x its bound"""
    if want["status"] != SUCCEEDED:
        return 0
    tol_d = tolerances(want, lat)[2]
    return sum(abs(w) > 100 * m * tol_d for row, mc in zip(want["post"], want["merged"]) for (_, w), m in zip(row, mc))
