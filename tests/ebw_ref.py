"""Plain-Python restatement of the Extended Baum-Welch update of DESIGN.md 7i (the specification of
khg_ebw_am_diag_gmm_update and khg_model_ebw_update) and of the three accumulator operations beside it
(AccumAmDiagGmm::Add / Scale, AccumDiagGmm::SmoothWithAccum).

Every value is a numpy scalar: np.float64 operations are IEEE fp64, one rounding each, in the written order; the
conversions to and from the model's float parameters go through np.float32 (DiagGmmNormal::CopyFromDiagGmm /
CopyToDiagGmm, csrc/diag-gmm-normal.cc:14-48).  Nothing here is vectorised over d on purpose: the order of the
operations IS the specification."""
import math

import numpy as np

F64 = np.float64
F32 = np.float32

EBW_E = 2.0
EBW_TAU = 0.0
W_MIN_COUNT = 10.0
W_MIN_WEIGHT = 1e-5
W_TAU = 0.0

M, V, W = 1, 2, 4


def normal_form(miv_row, iv_row):
    """-> (mu[d], var[d]) fp64 lists of one Gaussian (csrc/diag-gmm-normal.cc:14-20)."""
    var = [F64(1.0) / F64(iv) for iv in iv_row]
    mu = [F64(mi) * v for mi, v in zip(miv_row, var)]
    return mu, var


def try_d(Dv, flags, occ, x, x2, mu, var):
    """One evaluation of the update at smoothing constant Dv -> (ok, mu', var')."""
    c = occ + Dv
    nmu, nvar, ok = [], [], True
    for d in range(len(mu)):
        m_new = (x[d] + Dv * mu[d]) / c if flags & M else mu[d]
        v_new = var[d]
        if flags & V:
            if flags & M:
                v_new = (x2[d] + Dv * (var[d] + mu[d] * mu[d])) / c - m_new * m_new
            else:
                v_new = (x2[d] - F64(2.0) * mu[d] * x[d] + occ * mu[d] * mu[d] + Dv * var[d]) / c
            if not (v_new > 0.0):
                ok = False
        nmu.append(m_new)
        nvar.append(v_new)
    return ok, nmu, nvar


def q_terms(c, X, X2, m, s):
    """The per-dimension summands of -2 Q(m, s)."""
    return [c * F64(math.log(s[d])) + (X2[d] - F64(2.0) * m[d] * X[d] + c * m[d] * m[d]) / s[d] for d in range(len(m))]


def ebw_gauss(flags, E, tau, occ_n, x_n, x2_n, occ_d, x_d, x2_d, miv_row, iv_row, trace=None):
    """One Gaussian.  -> dict(status = 'skipped' | 'failed' | 'ok', iters, miv, iv (float32 rows), impr, abs_terms, n_terms,
    D_rejected, D_accepted, mu_new, var_new (fp64, before the float cast))."""
    Dm = len(miv_row)
    miv_row = np.asarray(miv_row, F32)
    iv_row = np.asarray(iv_row, F32)
    out = dict(status="ok", iters=0, miv=miv_row.copy(), iv=iv_row.copy(), impr=F64(0.0), abs_terms=F64(0.0), n_terms=0)
    occ_n, occ_d, E, tau = F64(occ_n), F64(occ_d), F64(E), F64(tau)
    if occ_n == 0.0 and occ_d == 0.0:
        out["status"] = "skipped"
        return out
    occ = occ_n - occ_d
    x = [F64(a) - F64(b) for a, b in zip(x_n, x_d)]
    x2 = [F64(a) - F64(b) for a, b in zip(x2_n, x2_d)]
    mu, var = normal_form(miv_row, iv_row)
    Dv = (tau + E * occ_d) / F64(2.0)
    out["branch_neg"] = bool(Dv + occ <= 0.0)
    if Dv + occ <= 0.0:
        Dv = F64(-1.0001) * occ + F64(1e-10)
    rejected = None
    with np.errstate(all="ignore"):
        for it in range(100):
            ok, _, _ = try_d(Dv, flags, occ, x, x2, mu, var)
            if ok:
                Dv = F64(2.0) * Dv
                _, nmu, nvar = try_d(Dv, flags, occ, x, x2, mu, var)
                break
            rejected = Dv
            Dv = F64(1.1) * Dv
        else:
            out["status"] = "failed"
            return out
        out.update(iters=it, D_rejected=rejected, D_accepted=Dv / F64(2.0), D_committed=Dv, mu_new=nmu, var_new=nvar)
        # CopyToDiagGmm for the flagged parts (csrc/diag-gmm-normal.cc:22-48)
        iv_new = iv_row.copy()
        miv_new = miv_row.copy()
        for d in range(Dm):
            if flags & V:
                iv_new[d] = F32(F64(1.0) / nvar[d])
                if not flags & M:
                    miv_new[d] = F32(mu[d]) * iv_new[d]
            if flags & M:
                miv_new[d] = F32(nmu[d]) * iv_new[d]
        out["miv"], out["iv"] = miv_new, iv_new
        # the diagnostic: Q at the committed values minus Q at the old ones, both with the smoothed statistics
        c = occ + Dv
        X = [x[d] + Dv * mu[d] for d in range(Dm)]
        X2 = [x2[d] + Dv * (var[d] + mu[d] * mu[d]) for d in range(Dm)]
        t_new = q_terms(c, X, X2, nmu, nvar)
        t_old = q_terms(c, X, X2, mu, var)
        diff = F64(0.0)
        ab = F64(0.0)
        for d in range(Dm):
            diff = diff + (t_old[d] - t_new[d])
            ab = ab + F64(0.5) * (abs(t_old[d]) + abs(t_new[d]))
        out["impr"] = F64(0.5) * diff
        out["abs_terms"] = ab
        out["n_terms"] = 2 * Dm
    return out


def ebw_weights(min_count, min_weight, tau_w, occ_n, occ_d, w_row):
    """One pdf's weights.  -> dict(status = 'skipped' | 'ok', weights (float32), w_new (fp64), impr, abs_terms, n_terms,
    floored (how many sat at the floor after the last round))."""
    G = len(w_row)
    w_row = np.asarray(w_row, F32)
    out = dict(status="ok", weights=w_row.copy(), impr=F64(0.0), abs_terms=F64(0.0), n_terms=0, floored=0)
    w0 = [F64(w) for w in w_row]
    n = [F64(occ_n[g]) + F64(tau_w) * w0[g] for g in range(G)]
    dd = [F64(occ_d[g]) for g in range(G)]
    tot = F64(0.0)
    for g in range(G):
        tot = tot + n[g]
    if tot < F64(min_count):
        out["status"] = "skipped"
        return out
    with np.errstate(all="ignore"):
        ratio = [dd[g] / w0[g] for g in range(G)]
        k_max = ratio[0]
        for g in range(1, G):
            if ratio[g] > k_max:
                k_max = ratio[g]
        cur = list(w0)
        floor = F64(min_weight)
        for _ in range(50):
            for g in range(G):
                cur[g] = n[g] + (k_max - ratio[g]) * cur[g]
                if cur[g] < floor:
                    cur[g] = floor
            s = F64(0.0)
            for g in range(G):
                s = s + cur[g]
            for g in range(G):
                cur[g] = cur[g] / s
        out["floored"] = sum(1 for g in range(G) if cur[g] == floor / s)
        out["last_sum"] = s
        out["w_new"] = cur
        out["weights"] = np.asarray([F32(v) for v in cur], F32)
        impr, ab = F64(0.0), F64(0.0)
        for g in range(G):
            t = n[g] * F64(math.log(cur[g] / w0[g])) - dd[g] * (cur[g] - w0[g]) / w0[g]
            impr = impr + t
            ab = ab + abs(n[g] * F64(math.log(cur[g] / w0[g]))) + abs(dd[g] * (cur[g] - w0[g]) / w0[g])
        out.update(impr=impr, abs_terms=ab, n_terms=2 * G)
    return out


def gconsts(w_row, miv, iv):
    """DiagGmm::ComputeGconsts (csrc/diag-gmm.cc:103-147): float accumulator, double right-hand side."""
    G, Dm = miv.shape
    offset = F32(-0.5 * 1.8378770664093454835606594728112 * Dm)
    out = np.zeros(G, F32)
    with np.errstate(all="ignore"):
        for g in range(G):
            gc = F32(np.log(F32(w_row[g]))) + offset
            for d in range(Dm):
                rhs = F64(0.5) * F64(np.log(F32(iv[g, d]))) - F64(0.5) * F64(miv[g, d]) * F64(miv[g, d]) / F64(iv[g, d])
                gc = F32(F64(gc) + rhs)
            if np.isinf(gc) and gc > 0:
                gc = -gc
            out[g] = gc
    return out


def ebw_update(gauss_off, weights, miv, iv, num, den, flags, E=EBW_E, tau=EBW_TAU, min_count=W_MIN_COUNT, min_weight=W_MIN_WEIGHT,
               tau_w=W_TAU, want_gconsts=True):
    """The whole model.  num / den = (occ[G], x[G, D], x2[G, D]) fp64.  -> dict of the new float parameters, the counters and
    diagnostics of khg_ebw_results, and per-Gaussian / per-pdf records for the tests (`gauss`, `pdfs`)."""
    weights = np.array(weights, F32)
    miv = np.array(miv, F32)
    iv = np.array(iv, F32)
    P = len(gauss_off) - 1
    r = dict(auxf_impr_gauss=F64(0.0), count=F64(0.0), auxf_impr_weights=F64(0.0), floored=0, failed=0, skipped=0, weights_skipped=0,
             abs_gauss=F64(0.0), n_gauss=0, abs_weights=F64(0.0), n_weights=0, gauss=[], pdfs=[])
    new_w = weights.copy()
    for p in range(P):
        a, b = int(gauss_off[p]), int(gauss_off[p + 1])
        impr_p, cnt_p = F64(0.0), F64(0.0)
        for g in range(a, b):
            cnt_p = cnt_p + F64(num[0][g])
        if flags & (M | V):
            for g in range(a, b):
                o = ebw_gauss(flags, E, tau, num[0][g], num[1][g], num[2][g], den[0][g], den[1][g], den[2][g], miv[g], iv[g])
                r["gauss"].append(o)
                if o["status"] == "skipped":
                    r["skipped"] += 1
                elif o["status"] == "failed":
                    r["failed"] += 1
                else:
                    miv[g], iv[g] = o["miv"], o["iv"]
                    r["floored"] += 1 if o["iters"] > 0 else 0
                    impr_p = impr_p + o["impr"]
                    r["abs_gauss"] += o["abs_terms"]
                    r["n_gauss"] += o["n_terms"]
        r["auxf_impr_gauss"] = r["auxf_impr_gauss"] + impr_p
        r["count"] = r["count"] + cnt_p
        if flags & W:
            o = ebw_weights(min_count, min_weight, tau_w, num[0][a:b], den[0][a:b], weights[a:b])
            r["pdfs"].append(o)
            if o["status"] == "skipped":
                r["weights_skipped"] += 1
            else:
                new_w[a:b] = o["weights"]
                r["auxf_impr_weights"] = r["auxf_impr_weights"] + o["impr"]
                r["abs_weights"] += o["abs_terms"]
                r["n_weights"] += o["n_terms"]
    r.update(weights=new_w, means_invvars=miv, inv_vars=iv)
    if want_gconsts:
        r["gconsts"] = np.concatenate([gconsts(new_w[int(gauss_off[p]):int(gauss_off[p + 1])], miv[int(gauss_off[p]):int(gauss_off[p + 1])],
                                               iv[int(gauss_off[p]):int(gauss_off[p + 1])]) for p in range(P)])
    return r


# ---- the accumulator operations, on blocks split as DeviceAccs.download() splits them ------------------------------------------
def accs_add(dst, scale, src):
    """dst += (double)(float)scale * src over the whole block (a 1-D fp64 array)."""
    return dst + F64(F32(scale)) * src


def accs_scale(dst, f):
    return dst * F64(F32(f))


def accs_smooth_with_accum(occ, mean, var, tau, s_occ, s_mean, s_var):
    """AccumDiagGmm::SmoothWithAccum (csrc/mle-diag-gmm.cc:209-226) on flat rows -> (occ, mean, var, untouched)."""
    occ, mean, var = occ.copy(), mean.copy(), var.copy()
    tau = F64(F32(tau))
    untouched = 0
    with np.errstate(all="ignore"):
        for g in range(len(occ)):
            so = F64(s_occ[g])
            if so != 0.0:
                new_occ = occ[g] + tau
                mean[g] = mean[g] + s_mean[g] * tau / so
                var[g] = var[g] + s_var[g] * tau / so
                occ[g] = new_occ
            else:
                untouched += 1
    return occ, mean, var, untouched
