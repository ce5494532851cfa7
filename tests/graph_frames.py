"""Host restatements of the two per-pdf frame bounds an utterance set derives from its graphs (khg_utts_pdf_first / _pdf_last), on the
CSR dicts the sets are built from; shared by tests/test_gpu_parity.py and the K1 form cases (tests/k1_form_cases.py)."""
from collections import deque

import numpy as np


def first_frames(g, u, id2pdf, pdfs):
    """Fewest emitting arcs before an arc with each listed pdf can be taken (0-1 BFS from the start state)."""
    s0, s1 = int(g["state_off"][u]), int(g["state_off"][u + 1])
    S = s1 - s0
    ao = g["arc_off"]
    dmin = [None] * S
    st = int(g["start"][u])
    dmin[st] = 0
    q = deque([st])
    while q:
        s = q.popleft()
        for a in range(int(ao[s0 + s]), int(ao[s0 + s + 1])):
            d, w = int(g["nextstate"][a]), 1 if g["ilabel"][a] >= 1 else 0
            if dmin[d] is None or dmin[s] + w < dmin[d]:
                dmin[d] = dmin[s] + w
                (q.append if w else q.appendleft)(d)
    first = {int(p): 10**9 for p in pdfs}
    for s in range(S):
        if dmin[s] is None:
            continue
        for a in range(int(ao[s0 + s]), int(ao[s0 + s + 1])):
            if g["ilabel"][a] >= 1:
                p = int(id2pdf[g["ilabel"][a]])
                first[p] = min(first[p], dmin[s])
    return first


def last_frames(graphs, u, id2pdf, pdf_list, T):
    """last frame at which an arc carrying each pdf can still lead to a final state by frame T (host restatement of pdf_last)."""
    g = graphs
    s0, s1 = int(g["state_off"][u]), int(g["state_off"][u + 1])
    S = s1 - s0
    ao = g["arc_off"]
    dfin = np.full(S, 10**9, np.int64)
    fin = np.isfinite(g["final"][s0:s1])
    dfin[fin] = 0
    changed = True
    while changed:                      # Bellman-Ford on the reversed graph (tiny graphs): emitting arcs weigh 1, epsilons 0
        changed = False
        for s in reversed(range(S)):    # (highest state first: a left-to-right chain of thousands of states settles in two sweeps)
            for a in range(int(ao[s0 + s]), int(ao[s0 + s + 1])):
                d, w = int(g["nextstate"][a]), int(g["ilabel"][a] >= 1)
                if dfin[d] + w < dfin[s]:
                    dfin[s] = dfin[d] + w; changed = True
    last = {int(p): -1 for p in pdf_list}
    for s in range(S):
        for a in range(int(ao[s0 + s]), int(ao[s0 + s + 1])):
            if g["ilabel"][a] >= 1 and dfin[int(g["nextstate"][a])] < 10**9:
                p = int(id2pdf[g["ilabel"][a]])
                last[p] = max(last[p], T - 1 - int(dfin[int(g["nextstate"][a])]))
    return last
