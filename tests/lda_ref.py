"""The restatement of the LDA rule in plain numpy: the oracle of tests/test_lda_cpu.py and tests/test_gpu_lda.py.
The reference has no LDA, so the rule written in 7n is the specification and this file says it a second time, the slow and obvious
way: `splice` (SpliceFrames), `definition_stats` (LdaEstimate::Accumulate per posterior entry: float64 terms in Kaldi's order, added in extended precision),
`estimate` (LdaEstimate::Estimate with numpy.linalg.cholesky / eigh) and the canonical sign of a row."""
import numpy as np

F32 = np.float32
OK, SINGULAR = 0, 1


def entry_weight(scale, w64):
    """the rule's one rounding (as khg_acc_stats_post)"""
    return F32(np.float64(F32(scale)) * np.float64(w64))


def splice(x, left, right):
    """z_t[k D + j] = x[clamp(t + k - left, 0, T - 1)][j], written as the loops of the definition"""
    x = np.asarray(x)
    T, D = x.shape
    z = np.zeros((T, D * (left + right + 1)), x.dtype)
    for t in range(T):
        for k in range(left + right + 1):
            r = min(max(t + k - left, 0), T - 1)
            z[t, k * D:(k + 1) * D] = x[r]
    return z


def packed(S):
    il, jl = np.tril_indices(S.shape[0])
    return np.ascontiguousarray(S[il, jl])


def unpacked(p, n):
    S = np.zeros((n, n))
    il, jl = np.tril_indices(n)
    S[il, jl] = p
    S[jl, il] = p
    return S


def definition_stats(feats, posts, id2pdf, C, left, right, scale=1.0):
    """Every entry (u, t, tid, w64) in utterance, frame, entry order: w = (float)((double)scale w64), c = id2pdf[tid];
    zero[c] += w, first[c] += w z_t, second += w z_t z_t^T.  posts[u] == [] is an utterance without frames in the handle.  The terms
    are float64 values; they are ADDED in numpy.longdouble (64 bits of mantissa here) and the sums rounded to float64 once, so that
    the yardstick's own rounding (2^-11 of a double's) stays out of the bound the device is held to.
    -> dict(zero, first, second (full symmetric), the sums of the terms' magnitudes abs_zero / abs_first / abs_second, the number of
    terms per class n_cls and in all n_second)."""
    LD = np.longdouble
    Dz = feats[0].shape[1] * (left + right + 1)
    zero, first, second = np.zeros(C, LD), np.zeros((C, Dz), LD), np.zeros((Dz, Dz), LD)
    azero, afirst, asecond = np.zeros(C), np.zeros((C, Dz)), np.zeros((Dz, Dz))
    n_cls = np.zeros(C, np.int64)
    for x, post in zip(feats, posts):
        if not post:
            continue
        z = splice(np.asarray(x, F32), left, right).astype(np.float64)
        assert len(post) == len(z)
        ts, cs, ws = [], [], []
        for t, f in enumerate(post):
            for tid, w64 in f:
                w = float(entry_weight(scale, w64))
                if w != 0.0:
                    ts.append(t); cs.append(int(id2pdf[tid])); ws.append(w)
        if not ts:
            continue
        ts, cs, ws = np.array(ts), np.array(cs), np.array(ws, np.float64)
        ze = z[ts]
        wz = ws.astype(LD)[:, None] * ze.astype(LD)
        np.add.at(zero, cs, ws.astype(LD))
        np.add.at(first, cs, wz)
        second += wz.T @ ze.astype(LD)
        np.add.at(azero, cs, np.abs(ws))
        np.add.at(afirst, cs, np.abs(ws)[:, None] * np.abs(ze))
        asecond += (np.abs(ws)[:, None] * np.abs(ze)).T @ np.abs(ze)
        np.add.at(n_cls, cs, 1)
    return dict(zero=zero.astype(np.float64), first=first.astype(np.float64), second=second.astype(np.float64), abs_zero=azero, abs_first=afirst,
                abs_second=asecond, n_cls=n_cls, n_second=int(n_cls.sum()))


def scatter(zero, first, second):
    """N, mu, Tc, Bc, Wc of the rule from the three accumulators (second: full symmetric or packed)"""
    zero, first = np.asarray(zero, np.float64), np.asarray(first, np.float64)
    n = first.shape[1]
    second = np.asarray(second, np.float64)
    if second.ndim == 1:
        second = unpacked(second, n)
    N = zero.sum()
    mu = first.sum(0) / N
    Tc = second / N - np.outer(mu, mu)
    Bc = -np.outer(mu, mu)
    for c in range(len(zero)):
        if zero[c] != 0:
            Bc = Bc + np.outer(first[c], first[c]) / (N * zero[c])
    return N, mu, Tc, Bc, Tc - Bc


def canonical_sign(M):
    """every row's element of largest magnitude (lowest index among equals) made positive"""
    M = np.array(M, np.float64, copy=True)
    for r in M:
        if r[int(np.argmax(np.abs(r)))] < 0:
            r *= -1.0
    return M


def estimate(zero, first, second, target_dim, remove_offset=False, within_class_factor=1.0):
    """-> dict(status, M (float64, [target_dim, n (+ 1)]), M_full, eig (descending), P, mu, Tc, Bc, Wc)"""
    n = np.asarray(first).shape[1]
    if not (np.asarray(zero, np.float64).sum() > 0):
        return dict(status=SINGULAR, M=np.eye(target_dim, n + (1 if remove_offset else 0)), M_full=np.eye(n), eig=np.zeros(n))
    N, mu, Tc, Bc, Wc = scatter(zero, first, second)
    try:
        Lc = np.linalg.cholesky(Wc)
    except np.linalg.LinAlgError:
        return dict(status=SINGULAR, M=np.eye(target_dim, n + (1 if remove_offset else 0)), M_full=np.eye(n), eig=np.zeros(n))
    Li = np.linalg.inv(Lc)
    P = Li @ Bc @ Li.T
    P = 0.5 * (P + P.T)
    lam, U = np.linalg.eigh(P)
    order = np.argsort(-lam, kind="stable")
    lam, U = lam[order], U[:, order]
    M_full = U.T @ Li
    f = within_class_factor
    if f != 1.0:
        M_full = M_full * np.sqrt((f + lam) / (1.0 + lam))[:, None]
    M_full = canonical_sign(M_full)
    M = M_full[:target_dim]
    if remove_offset:
        M = np.concatenate([M, -(M @ mu)[:, None]], 1)
    return dict(status=OK, M=M, M_full=M_full, eig=lam, P=P, mu=mu, Tc=Tc, Bc=Bc, Wc=Wc, N=N)
