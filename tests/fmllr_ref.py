"""The fMLLR rule of DESIGN.md 7l restated in plain Python / numpy: the statistics (FmllrDiagGmmAccs from posteriors), the estimate
(ComputeFmllrMatrixDiagGmmFull, update type "full") and the auxiliary function.  The reference has no fMLLR; this file and the
design text are the specification the library is tested against.

Every sum is written out in index order.  numpy is used for elementwise row operations only (one IEEE operation per element, the
same operation the C++ loop does); there is no BLAS call on a value path."""
import math

import numpy as np

OK, LOW_COUNT, SINGULAR = 0, 1, 2


def packed_index(i, j):
    return i * (i + 1) // 2 + j if j <= i else j * (j + 1) // 2 + i


def unpack(g, D1):
    """Kaldi's packed lower triangle -> the full symmetric matrix"""
    M = np.zeros((D1, D1))
    for i in range(D1):
        for j in range(i + 1):
            M[i, j] = M[j, i] = g[i * (i + 1) // 2 + j]
    return M


# ---- statistics -------------------------------------------------------------------------------------------------------------------
def component_posteriors(gc, miv, iv, x, w, dtype):
    """gamma_g = w exp(ll_g - max) / sum, ll_g = gconst + M . x - 1/2 V . x^2 in dimension order, all in `dtype`"""
    x = x.astype(dtype)
    ll = gc.astype(dtype).copy()
    nh = (dtype(-0.5) * iv.astype(dtype))
    M = miv.astype(dtype)
    x2 = x * x
    for d in range(len(x)):
        ll = ll + M[:, d] * x[d]
        ll = ll + nh[:, d] * x2[d]
    e = np.exp(ll - ll.max())
    s = dtype(0)
    for v in e:
        s = s + v
    return e * (dtype(w) / s)


def acc_stats(m, gc, feats, posts, utt2spk, n_spk, scale=1.0, dtype=np.float64):
    """The accumulation rule.  feats[u]: float32 [T, D]; posts[u]: per frame a list of (tid, weight), or [] for an utterance without
    frames in the handle.  Per entry in `dtype` (float32: the rule as written; float64: the yardstick of the GPU tests), per frame
    a_t / b_t in `dtype` and c_t in double, per speaker in double over its frames in set order.  -> beta [S], K [S, D, D + 1],
    G [S, D, packed]."""
    D = feats[0].shape[1]
    D1 = D + 1
    NP = D1 * (D1 + 1) // 2
    il, jl = np.tril_indices(D1)
    beta = np.zeros(n_spk)
    K = np.zeros((n_spk, D, D1))
    G = np.zeros((n_spk, D, NP))
    id2pdf = np.asarray(m.id2pdf)
    for u, (x_u, post) in enumerate(zip(feats, posts)):
        s = int(utt2spk[u])
        if s < 0 or len(post) == 0:
            continue
        assert len(post) == len(x_u)
        for t, frame in enumerate(post):
            x = x_u[t]
            a_t = np.zeros(D, dtype)
            b_t = np.zeros(D, dtype)
            c_t = 0.0
            for tid, w64 in frame:
                w = np.float32(np.float64(scale) * np.float64(w64))
                if w == 0:
                    continue
                p = int(id2pdf[tid])
                g0, g1 = int(m.gauss_off[p]), int(m.gauss_off[p + 1])
                gam = component_posteriors(gc[g0:g1], m.means_invvars[g0:g1], m.inv_vars[g0:g1], x, w, dtype)
                ea = np.zeros(D, dtype)
                eb = np.zeros(D, dtype)
                ec = dtype(0)
                for g in range(g1 - g0):
                    ea = ea + gam[g] * m.inv_vars[g0 + g].astype(dtype)
                    eb = eb + gam[g] * m.means_invvars[g0 + g].astype(dtype)
                    ec = ec + gam[g]
                a_t = a_t + ea
                b_t = b_t + eb
                c_t = c_t + float(ec)
            xp = np.concatenate([x.astype(np.float64), [1.0]])
            beta[s] += c_t
            K[s] += np.outer(b_t.astype(np.float64), xp)                 # elementwise products, one add per element per frame
            G[s] += np.outer(a_t.astype(np.float64), xp[il] * xp[jl])
    return beta, K, G


def definition_stats(m, gc, feats, posts, utt2spk, n_spk):
    """The definition, per Gaussian, in float64: K = sum gamma_g (mu_g / sigma_g^2) x+^T, G[d] = sum gamma_g sigma_{g,d}^-2 x+ x+^T,
    beta = sum gamma_g, with gamma from a float64 log-sum-exp."""
    D = feats[0].shape[1]
    D1 = D + 1
    beta = np.zeros(n_spk)
    K = np.zeros((n_spk, D, D1))
    Gf = np.zeros((n_spk, D, D1, D1))
    for u, (x_u, post) in enumerate(zip(feats, posts)):
        s = int(utt2spk[u])
        if s < 0 or len(post) == 0:
            continue
        for t, frame in enumerate(post):
            x = x_u[t].astype(np.float64)
            xp = np.concatenate([x, [1.0]])
            for tid, w in frame:
                p = int(m.id2pdf[tid])
                g0, g1 = int(m.gauss_off[p]), int(m.gauss_off[p + 1])
                miv = m.means_invvars[g0:g1].astype(np.float64)
                iv = m.inv_vars[g0:g1].astype(np.float64)
                ll = gc[g0:g1].astype(np.float64) + (miv * x).sum(1) - 0.5 * (iv * x * x).sum(1)
                gam = np.exp(ll - ll.max())
                gam = float(np.float32(w)) * gam / gam.sum()
                for g in range(g1 - g0):
                    beta[s] += gam[g]
                    K[s] += gam[g] * np.outer(miv[g], xp)
                    Gf[s] += gam[g] * iv[g][:, None, None] * np.outer(xp, xp)[None]
    il, jl = np.tril_indices(D1)
    return beta, K, Gf[:, :, il, jl]


# ---- estimate ---------------------------------------------------------------------------------------------------------------------
def inv_sym(g, D1):
    """Gauss-Jordan without pivoting; None: a pivot that is not finite or not > 0"""
    M = unpack(g, D1)
    inv = np.eye(D1)
    for p in range(D1):
        piv = M[p, p]
        if not (math.isfinite(piv) and piv > 0.0):
            return None
        M[p] = M[p] / piv
        inv[p] = inv[p] / piv
        rowM, rowI = M[p].copy(), inv[p].copy()
        f = M[:, p].copy()
        M = M - f[:, None] * rowM[None, :]
        inv = inv - f[:, None] * rowI[None, :]
        M[p], inv[p] = rowM, rowI
    return inv


def inv_piv(M):
    """Gauss-Jordan with partial pivoting (largest magnitude, lowest row among equals) -> (inverse, sum of log |pivot|), or None"""
    M = M.copy()
    n = M.shape[0]
    inv = np.eye(n)
    ld = 0.0
    for p in range(n):
        best, bv = p, abs(M[p, p])
        for r in range(p + 1, n):
            if abs(M[r, p]) > bv:
                best, bv = r, abs(M[r, p])
        if best != p:
            M[[p, best]] = M[[best, p]]
            inv[[p, best]] = inv[[best, p]]
        piv = M[p, p]
        if not math.isfinite(piv) or piv == 0.0:
            return None
        ld = ld + math.log(abs(piv))
        M[p] = M[p] / piv
        inv[p] = inv[p] / piv
        rowM, rowI = M[p].copy(), inv[p].copy()
        f = M[:, p].copy()
        M = M - f[:, None] * rowM[None, :]
        inv = inv - f[:, None] * rowI[None, :]
        M[p], inv[p] = rowM, rowI
    return inv, ld


def matvec(A, v):
    """r[i] = sum_j A[i][j] v[j], j ascending"""
    r = np.zeros(A.shape[0])
    for j in range(A.shape[1]):
        r = r + A[:, j] * v[j]
    return r


def dot(a, b):
    s = 0.0
    for x, y in zip(a, b):
        s = s + x * y
    return s


def auxf(beta, K, G, W):
    """Q(W) = beta log |det A| + sum_d (W[d] . K[d] - 1/2 W[d] G[d] W[d]^T), or None when A is singular"""
    D, D1 = K.shape
    r = inv_piv(W[:, :D].T.copy())
    if r is None:
        return None
    acc = 0.0
    for d in range(D):
        Gd = unpack(G[d], D1)
        t1 = dot(W[d], K[d])
        t2 = dot(W[d], matvec(Gd, W[d]))
        acc = acc + (t1 - 0.5 * t2)
    return beta * r[1] + acc


def estimate(beta, K, G, min_count=500.0, num_iters=40, sqrt_ulps=0, trace=False):
    """One speaker.  -> dict(W float64 [D, D + 1], status, objf_impr, gap: the smallest |f1 - f2| / (|f1| + |f2|) over all row updates,
    q: with trace, Q after every row update).  sqrt_ulps moves every square root by that many ulps (the spread a device primitive
    that rounds differently could cause)."""
    D, D1 = K.shape
    W = np.concatenate([np.eye(D), np.zeros((D, 1))], 1)
    out = {"W": W, "status": OK, "objf_impr": 0.0, "gap": math.inf, "q": []}
    if beta < min_count:
        out["status"] = LOW_COUNT
        return out
    invG = []
    for d in range(D):
        ig = inv_sym(G[d], D1)
        if ig is None:
            out["status"] = SINGULAR
            return out
        invG.append(ig)
    q0 = auxf(beta, K, G, W)
    W = W.copy()
    for _ in range(num_iters):
        for d in range(D):
            r = inv_piv(W[:, :D].T.copy())
            if r is None:
                out["status"] = SINGULAR
                return out
            c = np.concatenate([r[0][d], [0.0]])
            cg = matvec(invG[d], c)
            e1 = dot(cg, c)
            e2 = dot(cg, K[d])
            disc = math.sqrt(e2 * e2 + (4.0 * e1) * beta)
            for _k in range(abs(sqrt_ulps)):
                disc = math.nextafter(disc, math.inf if sqrt_ulps > 0 else -math.inf)
            a1 = (-e2 + disc) / (2.0 * e1)
            a2 = (-e2 - disc) / (2.0 * e1)
            f1 = beta * math.log(abs(a1 * e1 + e2)) - ((0.5 * a1) * a1) * e1
            f2 = beta * math.log(abs(a2 * e1 + e2)) - ((0.5 * a2) * a2) * e1
            out["gap"] = min(out["gap"], abs(f1 - f2) / (abs(f1) + abs(f2)))
            alpha = a1 if f1 > f2 else a2
            W[d] = matvec(invG[d], alpha * c + K[d])
            if trace:
                out["q"].append(auxf(beta, K, G, W))
    q1 = auxf(beta, K, G, W)
    if q1 is None:
        out["status"] = SINGULAR
        return out
    out["W"] = W
    out["objf_impr"] = q1 - q0
    return out


# ---- likelihoods ------------------------------------------------------------------------------------------------------------------
def loglike(m, gc, x, pdf):
    """float64 log-likelihood of the rows of x under one pdf"""
    g0, g1 = int(m.gauss_off[pdf]), int(m.gauss_off[pdf + 1])
    x = x.astype(np.float64)
    ll = gc[g0:g1].astype(np.float64)[None] + x @ m.means_invvars[g0:g1].astype(np.float64).T - 0.5 * (x * x) @ m.inv_vars[g0:g1].astype(np.float64).T
    mx = ll.max(1, keepdims=True)
    return (mx + np.log(np.exp(ll - mx).sum(1, keepdims=True)))[:, 0]
