// khg_k4_ebw.hip.inc -- K4, discriminative form: the Extended Baum-Welch update of the GMMs on the device (DESIGN.md 7i).
//
// Kaldi's gmm-est-gmm-ebw / gmm-est-weights-ebw on a numerator and a denominator block of statistics that K3 left in HBM.  The
// reference has no EBW update; the rule in DESIGN.md 7i is the specification, khg_host.cpp (khg_ebw_am_diag_gmm_update) the host form
// and tests/ebw_ref.py the restatement.  Every parameter-path operation is one IEEE fp64 / fp32 operation in that rule's order with
// contraction off, so weights, inv_vars and means_invvars are bit-identical to the host form's.
//
// One workgroup of 4 waves per pdf.  A wave takes one Gaussian at a time with its lanes over d (NPER elements per lane: 64 NPER >=
// dim): the four statistic rows and the two parameter rows are read ONCE into registers and the whole search for the smoothing
// constant D runs there.  The only cross-lane step on the parameter path is the boolean "every variance positive", a wave-wide
// __all: it has no order, so bit-exactness costs nothing.  The diagnostic sums go through a fixed butterfly (tolerance-checked, not
// bit-checked).  The weight rounds of a pdf are serial in the round; the normalising sum is one lane's ascending sum, as on the host.
//
// HBM-bound like k4_mle_update: per Gaussian 4*D fp64 statistic reads + 2*D float parameter reads and writes = D*48 bytes (+ the two
// occupancies) -- 614 MB for the 5000 x 64 x 40 model, 8*D*2 bytes per Gaussian more than the ML update; nothing goes on MFMA.
#pragma once

struct K4EbwRes {           // per pdf, summed on the host in pdf order (fp64, as khg_ebw_am_diag_gmm_update adds them)
  double impr_gauss, count, impr_w;
  int32_t floored, failed, skipped, w_skipped, bad, pad;
};

struct K4EbwArgs {
  const int32_t* gauss_off;
  int D;
  const double *occ_n, *mean_n, *var_n, *occ_d, *mean_d, *var_d;
  float *w, *gc, *miv, *iv;
  K4EbwRes* res;
  double E, tau, w_min_count, w_min_weight, w_tau;
  unsigned flags;
};

// try(D) of the rule for this lane's elements -> every variance of the lane positive (or v is off)
template <int NPER>
__device__ inline bool k4_ebw_try(double Dv, unsigned flags, double occ, const double (&x)[NPER], const double (&x2)[NPER],
                                  const double (&mu)[NPER], const double (&var)[NPER], const bool (&live)[NPER], double (&nmu)[NPER],
                                  double (&nvar)[NPER]) {
#pragma clang fp contract(off)
  const double c = occ + Dv;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < NPER; ++k) {
    const double m_new = (flags & K4_MEANS) ? (x[k] + Dv * mu[k]) / c : mu[k];
    double v_new = var[k];
    if (flags & K4_VARS) {
      if (flags & K4_MEANS) v_new = (x2[k] + Dv * (var[k] + mu[k] * mu[k])) / c - m_new * m_new;
      else v_new = (x2[k] - 2.0 * mu[k] * x[k] + occ * mu[k] * mu[k] + Dv * var[k]) / c;
      if (live[k] && !(v_new > 0.0)) ok = false;
    }
    nmu[k] = m_new; nvar[k] = v_new;
  }
  return ok;
}

__device__ inline double k4_ebw_wave_sum(double v) {      // fixed butterfly over the 64 lanes: every lane ends with the same total
  for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
  return v;
}

template <int NPER>
__global__ __launch_bounds__(256) void k4_ebw_update(K4EbwArgs a) {
#pragma clang fp contract(off)
  extern __shared__ double k4e_lds[];
  const int p = blockIdx.x, tid = threadIdx.x, D = a.D, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int g0 = a.gauss_off[p], G = a.gauss_off[p + 1] - g0;
  double* s_n = k4e_lds;                 // [G] occ_n, then n = occ_n + tau_w w_orig
  double* s_ratio = s_n + G;             // [G] d / w_orig
  double* s_cur = s_ratio + G;           // [G] the weights of the current round
  double* s_red = s_cur + G;             // [8]: 0..3 per-wave diagnostic sums, 4 count, 5 the round's sum, 6 weight diagnostic, 7 k_max
  int* s_cnt = (int*)(s_red + 8);        // [16]: 3 counters per wave, then [12] bad, [13] weights updated
  const double* occ_n = a.occ_n + g0;
  const double* occ_d = a.occ_d + g0;
  float* w = a.w + g0;
  float* miv = a.miv + (size_t)g0 * D;
  float* iv = a.iv + (size_t)g0 * D;

  for (int g = tid; g < G; g += 256) s_n[g] = occ_n[g];
  if (tid < 16) s_cnt[tid] = 0;
  __syncthreads();

  // ---- the Gaussians: means and variances ---------------------------------------------------------------------------------
  double impr = 0.0;                     // wave-uniform
  int floored = 0, failed = 0, skipped = 0;
  if (a.flags & (K4_MEANS | K4_VARS)) {
    for (int g = wave; g < G; g += 4) {
      const double on = occ_n[g], od = occ_d[g];
      if (on == 0.0 && od == 0.0) { ++skipped; continue; }
      const size_t row = (size_t)(g0 + g) * D;
      const double occ = on - od;
      double x[NPER], x2[NPER], mu[NPER], var[NPER], nmu[NPER], nvar[NPER];
      float iv_old[NPER], miv_old[NPER];
      bool live[NPER];
#pragma unroll
      for (int k = 0; k < NPER; ++k) {
        const int d = lane + 64 * k;
        live[k] = d < D;
        if (live[k]) {
          x[k] = a.mean_n[row + d] - a.mean_d[row + d];
          x2[k] = a.var_n[row + d] - a.var_d[row + d];
          iv_old[k] = a.iv[row + d];
          miv_old[k] = a.miv[row + d];
        } else {
          x[k] = 0.0; x2[k] = 0.0; iv_old[k] = 1.0f; miv_old[k] = 0.0f;
        }
        var[k] = 1.0 / (double)iv_old[k];            // DiagGmmNormal::CopyFromDiagGmm (csrc/diag-gmm-normal.cc:14-20)
        mu[k] = (double)miv_old[k] * var[k];
      }
      double Dv = (a.tau + a.E * od) / 2.0;
      if (Dv + occ <= 0.0) Dv = -1.0001 * occ + 1e-10;
      int it = 0;
      for (; it < 100; ++it) {
        if (__all(k4_ebw_try<NPER>(Dv, a.flags, occ, x, x2, mu, var, live, nmu, nvar))) {
          Dv = 2.0 * Dv;
          (void)k4_ebw_try<NPER>(Dv, a.flags, occ, x, x2, mu, var, live, nmu, nvar);
          break;
        }
        Dv = 1.1 * Dv;
      }
      if (it == 100) { ++failed; continue; }
      if (it > 0) ++floored;
      const double c = occ + Dv;
      double diff = 0.0;
#pragma unroll
      for (int k = 0; k < NPER; ++k) {
        if (!live[k]) continue;
        const int d = lane + 64 * k;
        const double X = x[k] + Dv * mu[k], X2 = x2[k] + Dv * (var[k] + mu[k] * mu[k]);
        const double t_new = c * log(nvar[k]) + (X2 - 2.0 * nmu[k] * X + c * nmu[k] * nmu[k]) / nvar[k];
        const double t_old = c * log(var[k]) + (X2 - 2.0 * mu[k] * X + c * mu[k] * mu[k]) / var[k];
        diff += t_old - t_new;
        // DiagGmmNormal::CopyToDiagGmm for the flagged parts (csrc/diag-gmm-normal.cc:22-48)
        float ivn = iv_old[k], mivn = miv_old[k];
        if (a.flags & K4_VARS) {
          ivn = (float)(1.0 / nvar[k]);
          if (!(a.flags & K4_MEANS)) mivn = (float)mu[k] * ivn;
        }
        if (a.flags & K4_MEANS) mivn = (float)nmu[k] * ivn;
        a.iv[row + d] = ivn;
        a.miv[row + d] = mivn;
      }
      impr += 0.5 * k4_ebw_wave_sum(diff);
    }
  }
  if (lane == 0) {
    s_red[wave] = impr;
    s_cnt[3 * wave] = floored; s_cnt[3 * wave + 1] = failed; s_cnt[3 * wave + 2] = skipped;
  }
  __syncthreads();

  // ---- the weights of the pdf ---------------------------------------------------------------------------------------------
  if (tid == 0) {
    double cnt = 0.0;
    for (int g = 0; g < G; ++g) cnt = cnt + s_n[g];
    s_red[4] = cnt;
    s_red[6] = 0.0;
  }
  __syncthreads();
  if ((a.flags & K4_WEIGHTS) && G > 0) {
    for (int g = tid; g < G; g += 256) {
      const double w0 = (double)w[g];
      s_n[g] = s_n[g] + a.w_tau * w0;
      s_ratio[g] = occ_d[g] / w0;
      s_cur[g] = w0;
    }
    __syncthreads();
    if (tid == 0) {
      double tot = 0.0;
      for (int g = 0; g < G; ++g) tot = tot + s_n[g];
      s_cnt[13] = tot < a.w_min_count ? 0 : 1;
      double k_max = s_ratio[0];
      for (int g = 1; g < G; ++g) if (s_ratio[g] > k_max) k_max = s_ratio[g];
      s_red[7] = k_max;
    }
    __syncthreads();
    if (s_cnt[13]) {
      const double k_max = s_red[7];
      for (int round = 0; round < 50; ++round) {
        for (int g = tid; g < G; g += 256) {
          double v = s_n[g] + (k_max - s_ratio[g]) * s_cur[g];
          if (v < a.w_min_weight) v = a.w_min_weight;
          s_cur[g] = v;
        }
        __syncthreads();
        if (tid == 0) {
          double s = 0.0;
          for (int g = 0; g < G; ++g) s = s + s_cur[g];
          s_red[5] = s;
        }
        __syncthreads();
        const double s = s_red[5];
        for (int g = tid; g < G; g += 256) s_cur[g] = s_cur[g] / s;     // each thread keeps its own g's: no barrier before the next round's update
      }
      __syncthreads();
      if (tid == 0) {
        double acc = 0.0;
        for (int g = 0; g < G; ++g) {
          const double w0 = (double)w[g];
          acc = acc + (s_n[g] * log(s_cur[g] / w0) - occ_d[g] * (s_cur[g] - w0) / w0);
        }
        s_red[6] = acc;
      }
      __syncthreads();
      for (int g = tid; g < G; g += 256) w[g] = (float)s_cur[g];
    }
  }
  __syncthreads();      // the rows and weights this block wrote are visible to its own threads

  // ---- gconsts (DiagGmm::ComputeGconsts), as k4_mle_update ends ---------------------------------------------------------------
  const float offset = (float)(-0.5 * 1.8378770664093454835606594728112 * D);
  for (int g = tid; g < G; g += 256) {
    float gc = k4_gconst(D, w[g], iv + (size_t)g * D, miv + (size_t)g * D, offset);
    if (gc != gc) atomicOr(&s_cnt[12], 1);
    if (isinf(gc) && gc > 0) gc = -gc;
    a.gc[g0 + g] = gc;
  }
  __syncthreads();
  if (tid == 0) {
    K4EbwRes r;
    r.impr_gauss = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
    r.count = s_red[4];
    r.impr_w = s_red[6];
    r.floored = s_cnt[0] + s_cnt[3] + s_cnt[6] + s_cnt[9];
    r.failed = s_cnt[1] + s_cnt[4] + s_cnt[7] + s_cnt[10];
    r.skipped = s_cnt[2] + s_cnt[5] + s_cnt[8] + s_cnt[11];
    r.w_skipped = ((a.flags & K4_WEIGHTS) && !(G > 0 && s_cnt[13])) ? 1 : 0;
    r.bad = s_cnt[12]; r.pad = 0;
    a.res[p] = r;
  }
}
