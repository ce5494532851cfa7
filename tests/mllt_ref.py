"""The MLLT rule of DESIGN.md 7m restated in plain Python / numpy: the statistics (MlltAccs from posteriors, as a definition and in
the computed form the device uses), the estimate (MlltAccs::Update) and the auxiliary function.  The reference has no MLLT; this
file and the design text are the specification the library is tested against.

The estimate writes every sum out in index order and uses numpy for elementwise row operations only (one IEEE operation per
element, the same operation the C++ loop does); the Gauss-Jordan forms are fmllr_ref's.  The statistics are float64 yardsticks:
their large sums go through einsum (the tests hold the device to them within tolerances, not on the bits)."""
import math

import numpy as np

import fmllr_ref as fref

OK, SINGULAR = 0, 1
GSLICE = 1024         # Gaussians of one slice of the Gaussian side and of the shift's sum (khg_mllt_stats.hip.inc: MT_GSLICE)


def unpack(g, D):
    return fref.unpack(g, D)


def means(m):
    """mu_g = means_invvars / inv_vars, one float division per element (DiagGmm::GetMeans)"""
    return (m.means_invvars.astype(np.float32) / m.inv_vars.astype(np.float32)).astype(np.float32)


def shift(m):
    """c: the fp64 sum of mu_g[j] per slice of 1024 consecutive Gaussians in (pdf, g) order, the slices' sums added in slice order,
    divided by the number of Gaussians, narrowed to float"""
    mu = means(m).astype(np.float64)
    tot = np.zeros(mu.shape[1])
    for s0 in range(0, len(mu), GSLICE):
        part = np.zeros(mu.shape[1])
        for g in range(s0, min(s0 + GSLICE, len(mu))):
            part = part + mu[g]
        tot = tot + part
    return (tot / float(len(mu))).astype(np.float32)


def _entries(m, gc, feats, posts, scale, dtype):
    """per frame with entries: (x float32, [(g0, g1, gamma [g1 - g0] in dtype)])"""
    id2pdf = np.asarray(m.id2pdf)
    for x_u, post in zip(feats, posts):
        if len(post) == 0:
            continue
        assert len(post) == len(x_u)
        for t, frame in enumerate(post):
            ents = []
            for tid, w64 in frame:
                w = np.float32(np.float64(scale) * np.float64(w64))
                if w == 0:
                    continue
                p = int(id2pdf[tid])
                g0, g1 = int(m.gauss_off[p]), int(m.gauss_off[p + 1])
                ents.append((g0, g1, fref.component_posteriors(gc[g0:g1], m.means_invvars[g0:g1], m.inv_vars[g0:g1], x_u[t], w, dtype)))
            yield x_u[t], ents


def acc_stats(m, gc, feats, posts, scale=1.0, dtype=np.float64, use_shift=True):
    """The computed form.  feats[u]: float32 [T, D]; posts[u]: per frame a list of (tid, weight), or [] for an utterance without
    frames in the handle.  Per entry in `dtype` (float32: the rule as written; float64: the yardstick of the tests), a_t in `dtype`,
    c_t, occ_g, m_g and everything after in double.  -> dict(beta, G [D, packed], S, C: the two uncancelled terms, c: the shift)"""
    D = feats[0].shape[1]
    il, jl = np.tril_indices(D)
    sumG = int(m.gauss_off[-1])
    c = shift(m) if use_shift else np.zeros(D, np.float32)
    c64 = c.astype(np.float64)
    iv = m.inv_vars.astype(dtype)
    A, X = [], []
    beta = 0.0
    occ = np.zeros(sumG)
    macc = np.zeros((sumG, D))
    for x, ents in _entries(m, gc, feats, posts, scale, dtype):
        a_t = np.zeros(D, dtype)
        c_t = 0.0
        x64 = x.astype(np.float64)
        for g0, g1, gam in ents:
            ea = np.zeros(D, dtype)
            ec = dtype(0)
            for g in range(g1 - g0):
                ea = ea + gam[g] * iv[g0 + g]
                ec = ec + gam[g]
            a_t = a_t + ea
            c_t = c_t + float(ec)
            g64 = gam.astype(np.float64)
            occ[g0:g1] += g64
            macc[g0:g1] += g64[:, None] * x64[None, :]
        beta += c_t
        A.append(a_t.astype(np.float64))
        X.append(x64 - c64)                                   # the difference of two floats: exact in a double
    if A:
        A, X = np.stack(A), np.stack(X)
        S = np.einsum("td,tp->dp", A, X[:, il] * X[:, jl])
    else:
        S = np.zeros((D, len(il)))
    mu = means(m).astype(np.float64) - c64
    ms = macc - occ[:, None] * c64[None, :]
    Z = (ms[:, il] * mu[:, jl] + mu[:, il] * ms[:, jl]) - (occ[:, None] * mu[:, il]) * mu[:, jl]
    C = np.einsum("gd,gp->dp", m.inv_vars.astype(np.float64), Z)
    return dict(beta=beta, G=S - C, S=S, C=C, c=c)


def definition_stats(m, gc, feats, posts, scale=1.0):
    """The definition, per Gaussian, in float64: beta = sum gamma_g, G[d] = sum gamma_g inv_var[g][d] (x - mu_g)(x - mu_g)^T with gamma
    from a float64 log-sum-exp.  -> (beta, G [D, packed])"""
    D = feats[0].shape[1]
    il, jl = np.tril_indices(D)
    mu = means(m).astype(np.float64)
    iv = m.inv_vars.astype(np.float64)
    G = np.zeros((D, len(il)))
    beta = 0.0
    for x, ents in _entries(m, gc, feats, posts, scale, np.float64):
        x64 = x.astype(np.float64)
        for g0, g1, gam in ents:
            off = x64[None, :] - mu[g0:g1]
            beta += float(gam.sum())
            G += np.einsum("gd,gp->dp", gam[:, None] * iv[g0:g1], off[:, il] * off[:, jl])
    return beta, G


# ---- estimate ---------------------------------------------------------------------------------------------------------------------
def auxf(beta, G, A):
    """Q(A) = beta log |det A| - 1/2 sum_d A[d] G[d] A[d]^T, or None when A is singular"""
    D = A.shape[0]
    r = fref.inv_piv(A.T.copy())
    if r is None:
        return None
    acc = 0.0
    for d in range(D):
        Gd = unpack(G[d], D)
        acc = acc + fref.dot(A[d], fref.matvec(Gd, A[d]))
    return beta * r[1] - 0.5 * acc


def estimate(beta, G, num_iters=200, trace=False):
    """-> dict(M float64 [D, D], status, objf_impr, q: with trace, Q after every row update)"""
    D = G.shape[0]
    A = np.eye(D)
    out = {"M": A, "status": OK, "objf_impr": 0.0, "q": []}
    if not (math.isfinite(beta) and beta > 0.0):
        out["status"] = SINGULAR
        return out
    invG = []
    for d in range(D):
        ig = fref.inv_sym(G[d], D)
        if ig is None:
            out["status"] = SINGULAR
            return out
        invG.append(ig)
    q0 = auxf(beta, G, A)
    A = A.copy()
    for _ in range(num_iters):
        for d in range(D):
            r = fref.inv_piv(A.T.copy())
            if r is None:
                out["status"] = SINGULAR
                return out
            c = r[0][d].copy()
            v = fref.matvec(invG[d], c)
            cv = fref.dot(c, v)
            s = math.sqrt(beta / cv) if cv != 0 and beta / cv >= 0 else math.nan
            if not math.isfinite(s):
                out["status"] = SINGULAR
                return out
            A[d] = v * s
            if trace:
                out["q"].append(auxf(beta, G, A))
    q1 = auxf(beta, G, A)
    if q1 is None:
        out["status"] = SINGULAR
        return out
    out["M"] = A
    out["objf_impr"] = q1 - q0
    return out


def loglike64(w, mu, iv, x):
    """float64 log-likelihood of the rows of x under one mixture given by weights, means and inverse variances"""
    gc = np.log(w) - 0.5 * mu.shape[1] * math.log(2 * math.pi) + 0.5 * np.log(iv).sum(1) - 0.5 * (mu * mu * iv).sum(1)
    ll = gc[None] + x @ (mu * iv).T - 0.5 * (x * x) @ iv.T
    mx = ll.max(1, keepdims=True)
    return (mx + np.log(np.exp(ll - mx).sum(1, keepdims=True)))[:, 0]


# ---- gmm-transform-means ------------------------------------------------------------------------------------------------------------
def fmaf32(a, b, c):
    """The float32 fused multiply-add of float32 values held in float64 arrays.  The product of two floats is exact in a double; the
    double sum p + c is then moved to the neighbour with an odd last bit whenever it is inexact (its error from the two-sum), so that
    narrowing to float32 is the single rounding of the exact a b + c.  tests/test_mllt_cpu.py holds this to exact rational arithmetic."""
    p = a * b
    s = p + c
    t = s - p
    err = (p - (s - t)) + (c - t)
    bits = s.view(np.int64).copy()
    inexact_even = (err != 0) & ((bits & 1) == 0) & np.isfinite(s)
    away = (err > 0) == (s > 0)
    bits[inexact_even & away] += 1
    bits[inexact_even & ~away] -= 1
    return bits.view(np.float64).astype(np.float32)


def transform_means(miv, iv, M):
    """means_invvars after gmm-transform-means, float32 in the kernel's order: mu = miv / iv, y = 0 then y = fmaf(M[d][j], mu[j], y) in
    j order, y * iv"""
    miv, iv, M = np.asarray(miv, np.float32), np.asarray(iv, np.float32), np.asarray(M, np.float32)
    mu = (miv / iv).astype(np.float32)
    y = np.zeros(mu.shape, np.float64)
    for j in range(mu.shape[1]):
        y = fmaf32(M[:, j].astype(np.float64)[None, :], mu[:, j].astype(np.float64)[:, None], y).astype(np.float64)
    return (y.astype(np.float32) * iv).astype(np.float32)
