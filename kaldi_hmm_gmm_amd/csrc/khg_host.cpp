// kaldi_hmm_gmm_amd/csrc/khg_host.cpp -- host-side (no GPU) entry points of include/khg_hip.h:
// gconsts, the M-step, the Extended Baum-Welch update and the transition-model update.  The
// reference keeps these on the host too (O(P*G*D) once per EM iteration); they run on the all-reduced accumulators.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

#include "../../include/khg_hip.h"

int khg_set_error(int code, const std::string& msg);  // khg_ctx_model.hip

namespace {

constexpr double kLog2Pi = 1.8378770664093454835606594728112;  // M_LOG_2PI, csrc/kaldi-math.h
constexpr uint16_t kMeans = 0x1, kVars = 0x2, kWeights = 0x4;  // csrc/model-common.h:18-26

// csrc/diag-gmm.cc:103-147 for one DiagGmm.  Returns false on NaN (the reference throws).
bool ComputeGconstsOne(int G, int D, const float* w, const float* iv, const float* miv, float* gc_out, int* num_bad) {
  const float offset = -0.5 * kLog2Pi * D;
  for (int mix = 0; mix < G; ++mix) {
    float gc = std::log(w[mix]) + offset;
    const float* ivr = iv + (size_t)mix * D;
    const float* mir = miv + (size_t)mix * D;
    for (int d = 0; d < D; ++d)  // double right-hand side, float accumulator (diag-gmm.cc:121-123)
      gc += 0.5 * std::log(ivr[d]) - 0.5 * mir[d] * mir[d] / ivr[d];
    if (std::isnan(gc)) return false;
    if (std::isinf(gc)) { ++*num_bad; if (gc > 0) gc = -gc; }
    gc_out[mix] = gc;
  }
  return true;
}

// csrc/mle-diag-gmm.cc:479-499
float MlObjective(int G, int D, const float* gc, const float* miv, const float* iv, const double* occ,
                  const double* macc, const double* vacc, uint16_t acc_flags) {
  double dot = 0.0;
  for (int g = 0; g < G; ++g) dot += occ[g] * static_cast<double>(gc[g]);
  float obj = dot;
  const size_t n = (size_t)G * D;
  if (acc_flags & kMeans) {
    double s = 0.0;
    for (size_t i = 0; i < n; ++i) s += macc[i] * static_cast<double>(miv[i]);
    obj += s;
  }
  if (acc_flags & kVars) {
    double s = 0.0;
    for (size_t i = 0; i < n; ++i) s += vacc[i] * static_cast<double>(iv[i]);
    obj -= 0.5 * s;
  }
  return obj;
}

struct UpdateResult { float obj_change = 0, count = 0; int floored_elems = 0, floored_gauss = 0, removed = 0; };

// csrc/mle-diag-gmm.cc:243-390 MleDiagGmmUpdate on one pdf held in vectors (may shrink).
bool MleUpdateOne(const khg_mle_options& o, int D, const double* occ, const double* macc, const double* vacc,
                  uint16_t acc_flags, uint16_t flags, std::vector<float>& w, std::vector<float>& gc,
                  std::vector<float>& miv, std::vector<float>& iv, UpdateResult* res) {
  int G = (int)w.size();
  const size_t n = (size_t)G * D;
  double occ_sum = 0.0;
  for (int g = 0; g < G; ++g) occ_sum += occ[g];
  int nb = 0;
  if (!ComputeGconstsOne(G, D, w.data(), iv.data(), miv.data(), gc.data(), &nb)) return false;
  const float obj_old = MlObjective(G, D, gc.data(), miv.data(), iv.data(), occ, macc, vacc, acc_flags);
  // DiagGmmNormal (csrc/diag-gmm-normal.cc:14-20)
  std::vector<double> nw(G), nvars(n), nmeans(n), oldmeans;
  for (int g = 0; g < G; ++g) nw[g] = w[g];
  for (size_t i = 0; i < n; ++i) { nvars[i] = 1.0 / static_cast<double>(iv[i]); nmeans[i] = static_cast<double>(miv[i]) * nvars[i]; }
  oldmeans = nmeans;
  std::vector<int> to_remove;
  std::vector<double> var(D), old_mean(D);
  for (int i = 0; i < G; ++i) {
    const double oc = occ[i];
    const double prob = occ_sum > 0.0 ? oc / occ_sum : 1.0 / G;
    if (oc > o.min_gaussian_occupancy && prob > o.min_gaussian_weight) {
      nw[i] = prob;
      double* mu = &nmeans[(size_t)i * D];
      for (int d = 0; d < D; ++d) old_mean[d] = mu[d];
      if (acc_flags & (kMeans | kVars))
        for (int d = 0; d < D; ++d) mu[d] = macc[(size_t)i * D + d] / oc;
      if (acc_flags & kVars) {
        for (int d = 0; d < D; ++d) var[d] = vacc[(size_t)i * D + d] / oc - mu[d] * mu[d];
        if (!(flags & kMeans))
          for (int d = 0; d < D; ++d) { const double dm = old_mean[d] - mu[d]; var[d] += dm * dm; }
        int floored = 0;
        for (int d = 0; d < D; ++d) {   // csrc/mle-diag-gmm.cc:311-333: the floor vector when supplied, else min_variance
          const double fl = o.variance_floor_vector ? o.variance_floor_vector[d] : o.min_variance;
          if (var[d] < fl) { var[d] = fl; ++floored; }
        }
        if (floored) { res->floored_elems += floored; ++res->floored_gauss; }
        for (int d = 0; d < D; ++d) nvars[(size_t)i * D + d] = var[d];
      }
    } else if (o.remove_low_count_gaussians && (int)to_remove.size() < G - 1) {
      to_remove.push_back(i);
    } else {
      nw[i] = std::max(prob, static_cast<double>(o.min_gaussian_weight));
    }
  }
  // CopyToDiagGmm (csrc/diag-gmm-normal.cc:22-48)
  if (flags & kWeights) for (int g = 0; g < G; ++g) w[g] = static_cast<float>(nw[g]);
  if (flags & kVars) {
    for (size_t i = 0; i < n; ++i) iv[i] = static_cast<float>(1.0 / nvars[i]);
    if (!(flags & kMeans)) for (size_t i = 0; i < n; ++i) miv[i] = static_cast<float>(oldmeans[i]) * iv[i];
  }
  if (flags & kMeans) for (size_t i = 0; i < n; ++i) miv[i] = static_cast<float>(nmeans[i]) * iv[i];
  if (!ComputeGconstsOne(G, D, w.data(), iv.data(), miv.data(), gc.data(), &nb)) return false;
  const float obj_new = MlObjective(G, D, gc.data(), miv.data(), iv.data(), occ, macc, vacc, acc_flags);
  res->obj_change = obj_new - obj_old;
  res->count = occ_sum;
  res->removed = (int)to_remove.size();
  if (!to_remove.empty()) {
    // DiagGmm::RemoveComponents(to_remove, renorm=true) (csrc/diag-gmm.cc:853-938): one at a
    // time, weights renormalised (float) after every removal
    for (size_t r = 0; r < to_remove.size(); ++r) {
      const int gi = to_remove[r] - (int)r;
      w.erase(w.begin() + gi);
      gc.erase(gc.begin() + gi);
      miv.erase(miv.begin() + (size_t)gi * D, miv.begin() + (size_t)(gi + 1) * D);
      iv.erase(iv.begin() + (size_t)gi * D, iv.begin() + (size_t)(gi + 1) * D);
      float s = 0.0f;
      for (float x : w) s += x;
      for (float& x : w) x /= s;
    }
    G = (int)w.size();
    if (!ComputeGconstsOne(G, D, w.data(), iv.data(), miv.data(), gc.data(), &nb)) return false;
  }
  return true;
}

}  // namespace

extern "C" void khg_mle_options_default(khg_mle_options* o) {
  o->min_gaussian_weight = 1.0e-05f; o->min_gaussian_occupancy = 10.0f; o->min_variance = 0.001; o->remove_low_count_gaussians = 1; o->variance_floor_vector = nullptr;
}

extern "C" int khg_compute_gconsts(int32_t P, int32_t D, const int32_t* gauss_off, const float* weights,
                                   const float* inv_vars, const float* means_invvars, float* gconsts, int32_t* num_bad_out) {
  if (P <= 0 || D <= 0 || !gauss_off || !weights || !inv_vars || !means_invvars || !gconsts)
    return khg_set_error(KHG_E_ARG, "khg_compute_gconsts: bad arguments");
  int nb = 0;
  for (int p = 0; p < P; ++p) {
    const int g0 = gauss_off[p], G = gauss_off[p + 1] - g0;
    for (int g = 0; g < G; ++g)
      if (!(weights[g0 + g] >= 0)) return khg_set_error(KHG_E_RUNTIME, "ComputeGconsts: negative weight");  // :114
    if (!ComputeGconstsOne(G, D, weights + g0, inv_vars + (size_t)g0 * D, means_invvars + (size_t)g0 * D, gconsts + g0, &nb))
      return khg_set_error(KHG_E_RUNTIME, "At component of pdf " + std::to_string(p) + ", not a number in gconst computation");
  }
  if (num_bad_out) *num_bad_out = nb;
  return KHG_OK;
}

extern "C" int khg_mle_am_diag_gmm_update(const khg_mle_options* o, int32_t P, int32_t D, const int32_t* gauss_off,
                                          const double* occ, const double* mean_acc, const double* var_acc,
                                          uint16_t acc_flags, uint16_t flags, float* weights, float* gconsts,
                                          float* means_invvars, float* inv_vars, int32_t* new_gauss_off,
                                          float* objf_change, float* count, int32_t* floored_elems,
                                          int32_t* floored_gauss, int32_t* removed) {
  if (!o || P <= 0 || D <= 0 || !gauss_off || !occ || !weights || !gconsts || !means_invvars || !inv_vars || !new_gauss_off)
    return khg_set_error(KHG_E_ARG, "khg_mle_am_diag_gmm_update: bad arguments");
  if (flags & ~acc_flags) return khg_set_error(KHG_E_RUNTIME, "Flags in argument do not match the active accumulators");  // mle-diag-gmm.cc:252
  if ((acc_flags & kMeans) && !mean_acc) return khg_set_error(KHG_E_ARG, "mean accumulator missing");
  if ((acc_flags & kVars) && !var_acc) return khg_set_error(KHG_E_ARG, "variance accumulator missing");
  // Pdfs are independent (csrc/mle-am-diag-gmm.cc:177-193 loops over them): each host thread updates a
  // contiguous range IN PLACE at the pdf's original offset (a pdf never grows), then one sequential pass
  // compacts the arrays and adds the per-pdf statistics in pdf order with the reference's float totals
  // (:153-202), so results do not depend on the thread count.
  std::vector<UpdateResult> res((size_t)P);
  std::vector<int32_t> newG((size_t)P, 0);
  std::vector<uint8_t> bad((size_t)P, 0);
  int nthr = (int)std::thread::hardware_concurrency();
  if (const char* e = getenv("KHG_HOST_THREADS")) nthr = atoi(e);
  nthr = std::max(1, std::min(nthr, 64));
  if ((int64_t)gauss_off[P] * D < (1 << 16)) nthr = 1;
  nthr = std::min(nthr, P);
  auto work = [&](int p0, int p1) {
    std::vector<float> w, gc, miv, iv;
    for (int p = p0; p < p1; ++p) {
      const int g0 = gauss_off[p], G = gauss_off[p + 1] - g0;
      w.assign(weights + g0, weights + g0 + G);
      gc.assign(G, 0.0f);
      miv.assign(means_invvars + (size_t)g0 * D, means_invvars + (size_t)(g0 + G) * D);
      iv.assign(inv_vars + (size_t)g0 * D, inv_vars + (size_t)(g0 + G) * D);
      if (!MleUpdateOne(*o, D, occ + g0, mean_acc ? mean_acc + (size_t)g0 * D : nullptr,
                        var_acc ? var_acc + (size_t)g0 * D : nullptr, acc_flags, flags, w, gc, miv, iv, &res[p])) {
        bad[p] = 1;
        continue;
      }
      newG[p] = (int32_t)w.size();
      std::copy(w.begin(), w.end(), weights + g0);
      std::copy(gc.begin(), gc.end(), gconsts + g0);
      std::copy(miv.begin(), miv.end(), means_invvars + (size_t)g0 * D);
      std::copy(iv.begin(), iv.end(), inv_vars + (size_t)g0 * D);
    }
  };
  if (nthr == 1) {
    work(0, P);
  } else {
    std::vector<std::thread> th;
    for (int t = 0; t < nthr; ++t) th.emplace_back(work, (int)((int64_t)P * t / nthr), (int)((int64_t)P * (t + 1) / nthr));
    for (auto& t : th) t.join();
  }
  float tot_obj = 0.0f, tot_count = 0.0f;
  int tfe = 0, tfg = 0, trm = 0;
  int out = 0;
  for (int p = 0; p < P; ++p) {
    if (bad[p]) return khg_set_error(KHG_E_RUNTIME, "pdf " + std::to_string(p) + ": not a number in gconst computation");
    const UpdateResult& r = res[p];
    tot_obj += r.obj_change; tot_count += r.count; tfe += r.floored_elems; tfg += r.floored_gauss; trm += r.removed;
    const int g0 = gauss_off[p], Gn = newG[p];
    new_gauss_off[p] = out;
    if (out != g0) {   // compaction never overtakes the read cursor (out <= g0)
      std::memmove(weights + out, weights + g0, sizeof(float) * Gn);
      std::memmove(gconsts + out, gconsts + g0, sizeof(float) * Gn);
      std::memmove(means_invvars + (size_t)out * D, means_invvars + (size_t)g0 * D, sizeof(float) * (size_t)Gn * D);
      std::memmove(inv_vars + (size_t)out * D, inv_vars + (size_t)g0 * D, sizeof(float) * (size_t)Gn * D);
    }
    out += Gn;
  }
  new_gauss_off[P] = out;
  if (objf_change) *objf_change = tot_obj;
  if (count) *count = tot_count;
  if (floored_elems) *floored_elems = tfe;
  if (floored_gauss) *floored_gauss = tfg;
  if (removed) *removed = trm;
  return KHG_OK;
}

// ---- Extended Baum-Welch: the reference has no EBW update, the rule written there is the specification ----------
// Every operation below is one IEEE fp64 operation in the written order (no contraction): tests/ebw_ref.py restates it in numpy
// scalars and khg_k4_ebw.hip.inc on the device, and the three agree bit for bit on the parameters.
namespace {

struct EbwGaussOut { int status = 0 /* 0 updated, 1 skipped, 2 failed */, iters = 0; double impr = 0.0; };

// try(D) of the rule: the candidate mean / variance rows at smoothing constant Dv -> every variance positive (or v is off)
inline bool EbwTry(double Dv, uint16_t flags, int D, double occ, const double* x, const double* x2, const double* mu, const double* var,
                   double* nmu, double* nvar) {
  const double c = occ + Dv;
  bool ok = true;
  for (int d = 0; d < D; ++d) {
    const double m_new = (flags & kMeans) ? (x[d] + Dv * mu[d]) / c : mu[d];
    double v_new = var[d];
    if (flags & kVars) {
      if (flags & kMeans) v_new = (x2[d] + Dv * (var[d] + mu[d] * mu[d])) / c - m_new * m_new;
      else v_new = (x2[d] - 2.0 * mu[d] * x[d] + occ * mu[d] * mu[d] + Dv * var[d]) / c;
      if (!(v_new > 0.0)) ok = false;
    }
    nmu[d] = m_new; nvar[d] = v_new;
  }
  return ok;
}

void EbwGaussOne(const khg_ebw_options& o, uint16_t flags, int D, double occ_n, const double* xn, const double* x2n, double occ_d, const double* xd,
                 const double* x2d, float* miv, float* iv, std::vector<double>& wk, EbwGaussOut* out) {
  if (occ_n == 0.0 && occ_d == 0.0) { out->status = 1; return; }
  wk.resize((size_t)6 * D);
  double *x = wk.data(), *x2 = x + D, *mu = x2 + D, *var = mu + D, *nmu = var + D, *nvar = nmu + D;
  const double occ = occ_n - occ_d;
  for (int d = 0; d < D; ++d) {
    x[d] = xn[d] - xd[d];
    x2[d] = x2n[d] - x2d[d];
    var[d] = 1.0 / static_cast<double>(iv[d]);            // DiagGmmNormal::CopyFromDiagGmm (csrc/diag-gmm-normal.cc:14-20)
    mu[d] = static_cast<double>(miv[d]) * var[d];
  }
  double Dv = (o.tau + o.E * occ_d) / 2.0;
  if (Dv + occ <= 0.0) Dv = -1.0001 * occ + 1e-10;
  int it = 0;
  for (; it < 100; ++it) {
    if (EbwTry(Dv, flags, D, occ, x, x2, mu, var, nmu, nvar)) {
      Dv = 2.0 * Dv;
      EbwTry(Dv, flags, D, occ, x, x2, mu, var, nmu, nvar);
      break;
    }
    Dv = 1.1 * Dv;
  }
  if (it == 100) { out->status = 2; return; }
  out->iters = it;
  // the diagnostic first (it needs the old float rows' normal form, which mu / var hold): Q(new) - Q(old) on the smoothed statistics
  const double c = occ + Dv;
  double diff = 0.0;
  for (int d = 0; d < D; ++d) {
    const double X = x[d] + Dv * mu[d], X2 = x2[d] + Dv * (var[d] + mu[d] * mu[d]);
    const double t_new = c * std::log(nvar[d]) + (X2 - 2.0 * nmu[d] * X + c * nmu[d] * nmu[d]) / nvar[d];
    const double t_old = c * std::log(var[d]) + (X2 - 2.0 * mu[d] * X + c * mu[d] * mu[d]) / var[d];
    diff = diff + (t_old - t_new);
  }
  out->impr = 0.5 * diff;
  // DiagGmmNormal::CopyToDiagGmm for the flagged parts (csrc/diag-gmm-normal.cc:22-48)
  for (int d = 0; d < D; ++d) {
    if (flags & kVars) {
      iv[d] = static_cast<float>(1.0 / nvar[d]);
      if (!(flags & kMeans)) miv[d] = static_cast<float>(mu[d]) * iv[d];
    }
    if (flags & kMeans) miv[d] = static_cast<float>(nmu[d]) * iv[d];
  }
}

// the weights of one pdf -> false when the pdf is below min_num_count_weight_update (weights untouched)
bool EbwWeightsOne(const khg_ebw_weight_options& o, int G, const double* occ_n, const double* occ_d, float* w, std::vector<double>& wk, double* impr) {
  wk.resize((size_t)5 * G);
  double *w0 = wk.data(), *n = w0 + G, *dd = n + G, *ratio = dd + G, *cur = ratio + G;
  double tot = 0.0;
  for (int g = 0; g < G; ++g) {
    w0[g] = static_cast<double>(w[g]);
    n[g] = occ_n[g] + o.tau * w0[g];
    dd[g] = occ_d[g];
    tot = tot + n[g];
  }
  if (tot < o.min_num_count_weight_update) return false;
  for (int g = 0; g < G; ++g) ratio[g] = dd[g] / w0[g];
  double k_max = ratio[0];
  for (int g = 1; g < G; ++g) if (ratio[g] > k_max) k_max = ratio[g];
  for (int g = 0; g < G; ++g) cur[g] = w0[g];
  for (int round = 0; round < 50; ++round) {
    for (int g = 0; g < G; ++g) {
      cur[g] = n[g] + (k_max - ratio[g]) * cur[g];
      if (cur[g] < o.min_gaussian_weight) cur[g] = o.min_gaussian_weight;
    }
    double s = 0.0;
    for (int g = 0; g < G; ++g) s = s + cur[g];
    for (int g = 0; g < G; ++g) cur[g] = cur[g] / s;
  }
  double a = 0.0;
  for (int g = 0; g < G; ++g) {
    a = a + (n[g] * std::log(cur[g] / w0[g]) - dd[g] * (cur[g] - w0[g]) / w0[g]);
    w[g] = static_cast<float>(cur[g]);
  }
  *impr = a;
  return true;
}

bool EbwFinite(const khg_ebw_options* o, const khg_ebw_weight_options* wo) {
  return std::isfinite(o->E) && std::isfinite(o->tau) && std::isfinite(wo->min_num_count_weight_update) &&
         std::isfinite(wo->min_gaussian_weight) && std::isfinite(wo->tau);
}

}  // namespace

extern "C" void khg_ebw_options_default(khg_ebw_options* o) { o->E = 2.0; o->tau = 0.0; }
extern "C" void khg_ebw_weight_options_default(khg_ebw_weight_options* o) {
  o->min_num_count_weight_update = 10.0; o->min_gaussian_weight = 1.0e-05; o->tau = 0.0;
}

extern "C" int khg_ebw_am_diag_gmm_update(const khg_ebw_options* o, const khg_ebw_weight_options* wo, int32_t P, int32_t D,
                                          const int32_t* gauss_off, const double* num_occ, const double* num_mean, const double* num_var,
                                          const double* den_occ, const double* den_mean, const double* den_var, uint16_t flags,
                                          float* weights, float* gconsts, float* means_invvars, float* inv_vars, khg_ebw_results* res) {
  if (!o || !wo || P <= 0 || D <= 0 || !gauss_off || !num_occ || !den_occ || !weights || !gconsts || !means_invvars || !inv_vars)
    return khg_set_error(KHG_E_ARG, "khg_ebw_am_diag_gmm_update: bad arguments");
  if (!EbwFinite(o, wo)) return khg_set_error(KHG_E_ARG, "khg_ebw_am_diag_gmm_update: an option is not finite");
  flags &= (kMeans | kVars | kWeights);         // t is ignored
  if ((flags & (kMeans | kVars)) && (!num_mean || !num_var || !den_mean || !den_var))      // (a weights-only update reads the occupancies alone)
    return khg_set_error(KHG_E_ARG, "khg_ebw_am_diag_gmm_update: mean / variance accumulators missing");
  khg_ebw_results r{};
  std::vector<double> wk;
  for (int p = 0; p < P; ++p) {
    const int g0 = gauss_off[p], G = gauss_off[p + 1] - g0;
    double impr_p = 0.0, count_p = 0.0;
    for (int g = 0; g < G; ++g) count_p = count_p + num_occ[g0 + g];
    if (flags & (kMeans | kVars)) {
      for (int g = g0; g < g0 + G; ++g) {
        EbwGaussOut go;
        const size_t row = (size_t)g * D;
        EbwGaussOne(*o, flags, D, num_occ[g], num_mean + row, num_var + row, den_occ[g], den_mean + row, den_var + row, means_invvars + row,
                    inv_vars + row, wk, &go);
        if (go.status == 1) ++r.skipped;
        else if (go.status == 2) ++r.failed;
        else { impr_p = impr_p + go.impr; if (go.iters > 0) ++r.floored; }
      }
    }
    r.auxf_impr_gauss = r.auxf_impr_gauss + impr_p;
    r.count = r.count + count_p;
    if (flags & kWeights) {
      double iw = 0.0;
      if (G > 0 && EbwWeightsOne(*wo, G, num_occ + g0, den_occ + g0, weights + g0, wk, &iw)) r.auxf_impr_weights = r.auxf_impr_weights + iw;
      else ++r.weights_skipped;
    }
    int nb = 0;
    if (!ComputeGconstsOne(G, D, weights + g0, inv_vars + (size_t)g0 * D, means_invvars + (size_t)g0 * D, gconsts + g0, &nb))
      return khg_set_error(KHG_E_RUNTIME, "pdf " + std::to_string(p) + ": not a number in gconst computation");
  }
  if (res) *res = r;
  return KHG_OK;
}

// csrc/transition-model.cc:657-750 (share_for_pdfs == false) + :339-359
extern "C" int khg_transition_mle_update(int32_t num_tstates, const int32_t* state2id, const int32_t* self_loop_of,
                                         const double* stats, float floor_, float mincount, float* log_probs,
                                         float* nsl, float* objf_impr, float* count) {
  if (num_tstates <= 0 || !state2id || !self_loop_of || !stats || !log_probs || !nsl)
    return khg_set_error(KHG_E_ARG, "khg_transition_mle_update: bad arguments");
  float count_sum = 0.0f, objf_impr_sum = 0.0f;
  std::vector<float> new_probs, old_probs;
  for (int ts = 1; ts <= num_tstates; ++ts) {
    const int first = state2id[ts], n = state2id[ts + 1] - first;
    if (n < 1) return khg_set_error(KHG_E_RUNTIME, "transition-state with no transitions");
    if (n == 1) continue;
    double tot = 0;
    for (int k = 0; k < n; ++k) tot += stats[first + k];
    count_sum += tot;
    if (tot < mincount) continue;
    new_probs.resize(n); old_probs.resize(n);
    for (int k = 0; k < n; ++k) { old_probs[k] = std::exp(log_probs[first + k]); new_probs[k] = stats[first + k] / tot; }
    for (int it = 0; it < 3; ++it) {  // floor + renormalise three times (:693-699)
      float s = 0.0f;
      for (float x : new_probs) s += x;
      for (float& x : new_probs) { x /= s; }
      for (float& x : new_probs) x = std::max(x, floor_);
    }
    for (int k = 0; k < n; ++k) {
      const double ch = stats[first + k] * (std::log(new_probs[k]) - std::log(old_probs[k]));
      objf_impr_sum += ch;
    }
    for (int k = 0; k < n; ++k) {
      const float lp = std::log(new_probs[k]);
      if (lp - lp != 0.0f) return khg_set_error(KHG_E_RUNTIME, "Log probs is inf or NaN: error in update or bad stats?");
      log_probs[first + k] = lp;
    }
  }
  if (objf_impr) *objf_impr = objf_impr_sum;
  if (count) *count = count_sum;
  for (int ts = 1; ts <= num_tstates; ++ts) {
    const int tid = self_loop_of[ts];
    if (tid == 0) { nsl[ts] = 0.0f; continue; }
    const float slp = std::exp(log_probs[tid]);
    float nslp = 1.0 - slp;
    if (nslp <= 0.0) nslp = 1.0e-10;
    nsl[ts] = std::log(nslp);
  }
  return KHG_OK;
}

// csrc/hmm-utils.cc:442-463, negated (what AddTransitionProbs multiplies into the arc weight)
extern "C" int khg_scaled_trans_cost(int32_t num_tids, const float* log_probs, const float* nsl, const int32_t* id2state,
                                     const uint8_t* is_self_loop, float transition_scale, float self_loop_scale, float* out) {
  if (num_tids <= 0 || !log_probs || !nsl || !id2state || !is_self_loop || !out)
    return khg_set_error(KHG_E_ARG, "khg_scaled_trans_cost: bad arguments");
  out[0] = 0.0f;
  for (int tid = 1; tid <= num_tids; ++tid) {
    float s;
    if (transition_scale == self_loop_scale) s = log_probs[tid] * transition_scale;
    else if (is_self_loop[tid]) s = self_loop_scale * log_probs[tid];
    else {
      const int ts = id2state[tid];
      const float ignoring = log_probs[tid] - nsl[ts];  // GetTransitionLogProbIgnoringSelfLoops
      s = self_loop_scale * nsl[ts] + transition_scale * ignoring;
    }
    out[tid] = -s;
  }
  return KHG_OK;
}

// ------------------------------------------------------------------------------------------
// DiagGmm::Merge (csrc/diag-gmm.cc:557-759).  Second-order statistics per component (mean, E[x^2]) normalised by the
// weight; the likelihood change of merging (i, j) is w_sum * logdet(merged) - w_i logdet_i - w_j logdet_j with
// logdet = -1/2 sum log var; the pair with the LARGEST change (least loss) is merged, strict '>' over the lower triangle
// in (i, j < i) order, so ties go to the first pair scanned.
namespace {
struct MergeState {
  int G, D;
  std::vector<float> mean, m2, logdet, delta;   // delta: G x G, symmetric once touched
  std::vector<char> gone;
  float* w;
  float PairLogdet(int i, int j) const {          // MergedComponentsLogdet (:761-778)
    const float w1 = w[i], w2 = w[j], ratio = w2 / w1, scale = w1 / (w1 + w2);
    const float *f1 = &mean[(size_t)i * D], *f2 = &mean[(size_t)j * D], *s1 = &m2[(size_t)i * D], *s2 = &m2[(size_t)j * D];
    float acc = 0.0f;
    for (int d = 0; d < D; ++d) {
      const float mu = (f1[d] + f2[d] * ratio) * scale;
      acc += std::log((s1[d] + s2[d] * ratio) * scale - mu * mu);
    }
    return static_cast<float>(-0.5 * acc);
  }
  float Delta(int i, int j) const { const float w1 = w[i], w2 = w[j]; return (w1 + w2) * PairLogdet(i, j) - w1 * logdet[i] - w2 * logdet[j]; }
};
}  // namespace

extern "C" int khg_diag_gmm_merge(int32_t* num_gauss, int32_t D, int32_t target, float* weights, float* gconsts, float* miv,
                                  float* iv, int32_t* history, int32_t* num_history) {
  if (!num_gauss || !weights || !gconsts || !miv || !iv || D <= 0) return khg_set_error(KHG_E_ARG, "khg_diag_gmm_merge: bad arguments");
  const int G = *num_gauss;
  if (num_history) *num_history = 0;
  if (target <= 0 || G < target)
    return khg_set_error(KHG_E_RUNTIME, "Invalid argument for target number of Gaussians (=" + std::to_string(target) + "), #Gauss = " + std::to_string(G));
  if (G == target) return KHG_OK;
  MergeState st;
  st.G = G; st.D = D; st.w = weights;
  st.mean.resize((size_t)G * D); st.m2.resize((size_t)G * D);
  for (size_t k = 0; k < (size_t)G * D; ++k) {
    const float var = 1.0f / iv[k], mu = miv[k] * var;
    st.mean[k] = mu; st.m2[k] = var + mu * mu;
  }
  int nb = 0;
  if (target == 1) {   // :571-611: one Gaussian with the mixture's global mean and variance
    std::vector<float> gm((size_t)D, 0.0f), gs((size_t)D, 0.0f);
    for (int d = 0; d < D; ++d)
      for (int g = 0; g < G; ++g) { gm[d] += weights[g] * st.mean[(size_t)g * D + d]; gs[d] += weights[g] * st.m2[(size_t)g * D + d]; }
    float wsum = 0.0f;
    for (int g = 0; g < G; ++g) wsum += weights[g];
    weights[0] = wsum;
    if (!(std::fabs(wsum - 1.0f) <= 1e-6f * (std::fabs(wsum) + 1.0f))) {   // !ApproxEqual(w, 1, 1e-6): ":rescaling" as the reference writes it
      for (int d = 0; d < D; ++d) { gm[d] *= weights[0]; gs[d] *= weights[0]; }
      weights[0] = 1.0f;
    }
    for (int d = 0; d < D; ++d) { iv[d] = 1.0f / (gs[d] - gm[d] * gm[d]); miv[d] = gm[d] * iv[d]; }
    *num_gauss = 1;
    if (!ComputeGconstsOne(1, D, weights, iv, miv, gconsts, &nb)) return khg_set_error(KHG_E_RUNTIME, "At component 0, not a number in gconst computation");
    return KHG_OK;
  }
  st.logdet.resize((size_t)G); st.delta.assign((size_t)G * G, 0.0f); st.gone.assign((size_t)G, 0);
  for (int g = 0; g < G; ++g) {
    float acc = 0.0f;
    for (int d = 0; d < D; ++d) acc += std::log(iv[(size_t)g * D + d]);
    st.logdet[g] = 0.5f * acc;
  }
  for (int i = 1; i < G; ++i)
    for (int j = 0; j < i; ++j) st.delta[(size_t)i * G + j] = st.Delta(i, j);
  int nh = 0;
  for (int step = G; step > target; --step) {
    float best = -std::numeric_limits<float>::max();
    int bi = -1, bj = -1;
    for (int i = 1; i < G; ++i) {
      if (st.gone[i]) continue;
      const float* row = &st.delta[(size_t)i * G];
      for (int j = 0; j < i; ++j)
        if (!st.gone[j] && row[j] > best) { best = row[j]; bi = i; bj = j; }
    }
    if (bi < 0 || bj < 0) return khg_set_error(KHG_E_RUNTIME, "max_i != max_j && max_i != -1 && max_j != -1 assertion failed");
    if (history) { history[nh] = bi; history[nh + 1] = bj; }
    nh += 2;
    const float w1 = weights[bi], w2 = weights[bj], w_sum = w1 + w2, ratio = w2 / w1;
    float ld = 0.0f;
    for (int d = 0; d < D; ++d) {
      const size_t a = (size_t)bi * D + d, b = (size_t)bj * D + d;
      st.mean[a] = (st.mean[a] + ratio * st.mean[b]) * w1 / w_sum;
      st.m2[a] = (st.m2[a] + ratio * st.m2[b]) * w1 / w_sum;
      iv[a] = 1.0f / (st.m2[a] - st.mean[a] * st.mean[a]);
      miv[a] = st.mean[a] * iv[a];
      ld += std::log(iv[a]);
    }
    weights[bi] = w_sum;
    st.logdet[bi] = 0.5f * ld;
    st.gone[bj] = 1;
    for (int j = 0; j < G; ++j) {
      if (j == bi || st.gone[j]) continue;
      const float t = st.Delta(bi, j);
      st.delta[(size_t)bi * G + j] = t; st.delta[(size_t)j * G + bi] = t;
    }
  }
  int kept = 0;
  for (int i = 0; i < G; ++i) {
    if (st.gone[i]) continue;
    if (kept != i) {
      weights[kept] = weights[i];
      std::memmove(miv + (size_t)kept * D, miv + (size_t)i * D, sizeof(float) * D);
      std::memmove(iv + (size_t)kept * D, iv + (size_t)i * D, sizeof(float) * D);
    }
    ++kept;
  }
  *num_gauss = kept;
  if (num_history) *num_history = nh;
  if (!ComputeGconstsOne(kept, D, weights, iv, miv, gconsts, &nb)) return khg_set_error(KHG_E_RUNTIME, "not a number in gconst computation");
  return KHG_OK;
}

// ------------------------------------------------------------------------------------------
// ModifyGraphForCarefulAlignment (csrc/decoder-wrappers.cc:111-140) on flat CSR arrays.
extern "C" int khg_careful_graph(int32_t S, int32_t start, const int64_t* arc_off, const int32_t* il, const int32_t* ol,
                                 const float* wt, const int32_t* ns, const float* fin, int32_t* oS, int32_t* ostart,
                                 int64_t* o_off, int32_t* o_il, int32_t* o_ol, float* o_wt, int32_t* o_ns, float* o_fin) {
  if (S < 0 || !oS || !ostart || !o_off) return khg_set_error(KHG_E_ARG, "khg_careful_graph: bad arguments");
  if (S == 0) { *oS = 0; *ostart = start; o_off[0] = 0; return KHG_OK; }     // "Empty FST input." -- left as it is
  if (!arc_off || !il || !ol || !wt || !ns || !fin || !o_il || !o_ol || !o_wt || !o_ns || !o_fin || start < 0 || start >= S)
    return khg_set_error(KHG_E_ARG, "khg_careful_graph: bad arguments");
  const int32_t pre_initial = 2 * S;
  int64_t n = 0;
  auto put = [&](int32_t i, int32_t o, float w, int32_t d) { o_il[n] = i; o_ol[n] = o; o_wt[n] = w; o_ns[n] = d; ++n; };
  for (int32_t s = 0; s < S; ++s) {                       // left copy: own arcs, then the Concat epsilon of a final state
    o_off[s] = n;
    for (int64_t a = arc_off[s]; a < arc_off[s + 1]; ++a) put(il[a], ol[a], wt[a], ns[a]);
    if (!std::isinf(fin[s])) put(0, 0, fin[s], pre_initial);
    o_fin[s] = INFINITY;
  }
  for (int32_t s = 0; s < S; ++s) {                       // right copy, no final weights
    o_off[S + s] = n;
    for (int64_t a = arc_off[s]; a < arc_off[s + 1]; ++a) put(il[a], ol[a], wt[a], ns[a] + S);
    o_fin[S + s] = INFINITY;
  }
  o_off[pre_initial] = n;                                 // the pre-initial state of the right copy: final (One) + epsilon to its start
  put(0, 0, 0.0f, start + S);
  o_fin[pre_initial] = 0.0f;
  o_off[pre_initial + 1] = n;
  *oS = 2 * S + 1;
  *ostart = start;
  return KHG_OK;
}

// ---- fMLLR estimate: the reference has no fMLLR, the rule written there is the specification -----------------------
// Kaldi's ComputeFmllrMatrixDiagGmmFull on one speaker's statistics.  Every operation below is one IEEE fp64 operation in the written
// order (no contraction), every sum runs in index order: tests/fmllr_ref.py restates it and agrees on the bits of W.
#pragma clang fp contract(off)
namespace {

// the inverse of the symmetric matrix behind a packed lower triangle, by Gauss-Jordan without pivoting; false: a pivot that is not
// finite or not > 0.  M and inv are n x n.
bool FmInvSym(int n, const double* packed, double* M, double* inv) {
  for (int i = 0; i < n; ++i)
    for (int j = 0; j <= i; ++j) { M[i * n + j] = packed[i * (i + 1) / 2 + j]; M[j * n + i] = M[i * n + j]; }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) inv[i * n + j] = i == j ? 1.0 : 0.0;
  for (int p = 0; p < n; ++p) {
    const double piv = M[p * n + p];
    if (!(std::isfinite(piv) && piv > 0.0)) return false;
    for (int j = 0; j < n; ++j) { M[p * n + j] = M[p * n + j] / piv; inv[p * n + j] = inv[p * n + j] / piv; }
    for (int r = 0; r < n; ++r) {
      if (r == p) continue;
      const double f = M[r * n + p];
      for (int j = 0; j < n; ++j) { M[r * n + j] = M[r * n + j] - f * M[p * n + j]; inv[r * n + j] = inv[r * n + j] - f * inv[p * n + j]; }
    }
  }
  return true;
}
// inv = M^-1 by Gauss-Jordan with partial pivoting (the largest magnitude wins, the lowest row among equals); M is destroyed;
// *logabsdet = sum over the pivots of log |pivot|, in order.  false: a pivot that is zero or not finite.
bool FmInvPiv(int n, double* M, double* inv, double* logabsdet) {
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) inv[i * n + j] = i == j ? 1.0 : 0.0;
  double ld = 0.0;
  for (int p = 0; p < n; ++p) {
    int best = p;
    double bv = std::fabs(M[p * n + p]);
    for (int r = p + 1; r < n; ++r) { const double v = std::fabs(M[r * n + p]); if (v > bv) { bv = v; best = r; } }
    if (best != p)
      for (int j = 0; j < n; ++j) { std::swap(M[p * n + j], M[best * n + j]); std::swap(inv[p * n + j], inv[best * n + j]); }
    const double piv = M[p * n + p];
    if (!(std::isfinite(piv)) || piv == 0.0) return false;
    ld = ld + std::log(std::fabs(piv));
    for (int j = 0; j < n; ++j) { M[p * n + j] = M[p * n + j] / piv; inv[p * n + j] = inv[p * n + j] / piv; }
    for (int r = 0; r < n; ++r) {
      if (r == p) continue;
      const double f = M[r * n + p];
      for (int j = 0; j < n; ++j) { M[r * n + j] = M[r * n + j] - f * M[p * n + j]; inv[r * n + j] = inv[r * n + j] - f * inv[p * n + j]; }
    }
  }
  *logabsdet = ld;
  return true;
}
// Q(W) = beta log |det A| + sum_d (W[d] . K[d] - 1/2 W[d] G[d] W[d]^T); false: A is singular
bool FmAuxf(int D, double beta, const double* K, const double* G, const double* W, double* q, double* M, double* inv) {
  const int D1 = D + 1, NP = D1 * (D1 + 1) / 2;
  for (int i = 0; i < D; ++i)
    for (int j = 0; j < D; ++j) M[i * D + j] = W[j * D1 + i];
  double ld = 0.0;
  if (!FmInvPiv(D, M, inv, &ld)) return false;
  double acc = 0.0;
  for (int d = 0; d < D; ++d) {
    const double* g = G + (size_t)d * NP;
    const double* w = W + (size_t)d * D1;
    double t1 = 0.0, t2 = 0.0;
    for (int i = 0; i < D1; ++i) t1 = t1 + w[i] * K[d * D1 + i];
    for (int i = 0; i < D1; ++i) {
      double r = 0.0;
      for (int j = 0; j < D1; ++j) r = r + g[j <= i ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i] * w[j];
      t2 = t2 + w[i] * r;
    }
    acc = acc + (t1 - 0.5 * t2);
  }
  *q = beta * ld + acc;
  return true;
}

// one speaker; W: D x (D + 1) doubles
int32_t FmllrOne(const khg_fmllr_options* o, int D, double beta, const double* K, const double* G, double* W, double* objf_impr) {
  const int D1 = D + 1, NP = D1 * (D1 + 1) / 2;
  auto identity = [&] {
    for (int d = 0; d < D; ++d)
      for (int j = 0; j < D1; ++j) W[d * D1 + j] = d == j ? 1.0 : 0.0;
  };
  identity();
  *objf_impr = 0.0;
  if (beta < o->min_count) return KHG_FMLLR_LOW_COUNT;
  std::vector<double> invG((size_t)D * D1 * D1), M((size_t)D1 * D1), inv((size_t)D1 * D1), c(D1), cg(D1), v(D1);
  for (int d = 0; d < D; ++d)
    if (!FmInvSym(D1, G + (size_t)d * NP, M.data(), invG.data() + (size_t)d * D1 * D1)) return KHG_FMLLR_SINGULAR;
  double q0 = 0.0;
  if (!FmAuxf(D, beta, K, G, W, &q0, M.data(), inv.data())) return KHG_FMLLR_SINGULAR;
  for (int it = 0; it < o->num_iters; ++it)
    for (int d = 0; d < D; ++d) {
      for (int i = 0; i < D; ++i)
        for (int j = 0; j < D; ++j) M[i * D + j] = W[j * D1 + i];            // A^T
      double ld = 0.0;
      if (!FmInvPiv(D, M.data(), inv.data(), &ld)) { identity(); return KHG_FMLLR_SINGULAR; }
      for (int j = 0; j < D; ++j) c[j] = inv[d * D + j];
      c[D] = 0.0;
      const double* ig = invG.data() + (size_t)d * D1 * D1;
      const double* k = K + (size_t)d * D1;
      for (int i = 0; i < D1; ++i) {
        double r = 0.0;
        for (int j = 0; j < D1; ++j) r = r + ig[i * D1 + j] * c[j];
        cg[i] = r;
      }
      double e1 = 0.0, e2 = 0.0;
      for (int i = 0; i < D1; ++i) e1 = e1 + cg[i] * c[i];
      for (int i = 0; i < D1; ++i) e2 = e2 + cg[i] * k[i];
      const double disc = std::sqrt(e2 * e2 + (4.0 * e1) * beta);
      const double a1 = (-e2 + disc) / (2.0 * e1), a2 = (-e2 - disc) / (2.0 * e1);
      const double f1 = beta * std::log(std::fabs(a1 * e1 + e2)) - ((0.5 * a1) * a1) * e1;
      const double f2 = beta * std::log(std::fabs(a2 * e1 + e2)) - ((0.5 * a2) * a2) * e1;
      const double alpha = f1 > f2 ? a1 : a2;
      for (int i = 0; i < D1; ++i) v[i] = alpha * c[i] + k[i];
      for (int i = 0; i < D1; ++i) {
        double r = 0.0;
        for (int j = 0; j < D1; ++j) r = r + ig[i * D1 + j] * v[j];
        W[d * D1 + i] = r;
      }
    }
  double q1 = 0.0;
  if (!FmAuxf(D, beta, K, G, W, &q1, M.data(), inv.data())) { identity(); return KHG_FMLLR_SINGULAR; }
  *objf_impr = q1 - q0;
  return KHG_FMLLR_OK;
}

}  // namespace

extern "C" void khg_fmllr_options_default(khg_fmllr_options* o) { o->min_count = 500.0; o->num_iters = 40; }

extern "C" int khg_fmllr_compute(const khg_fmllr_options* o, int32_t n_spk, int32_t dim, const double* beta_h, const double* K_h, const double* G_h,
                                 float* W_h, double* W64_h, double* objf_impr_h, double* count_h, int32_t* status_h) {
  khg_fmllr_options def;
  khg_fmllr_options_default(&def);
  if (!o) o = &def;
  if (n_spk < 1 || dim < 1 || dim > KHG_FMLLR_MAX_DIM || !beta_h || !K_h || !G_h || (!W_h && !W64_h))
    return khg_set_error(KHG_E_ARG, "khg_fmllr_compute: bad arguments");
  if (!std::isfinite(o->min_count) || o->num_iters < 0) return khg_set_error(KHG_E_ARG, "khg_fmllr_compute: an option is not finite or negative");
  const int D = dim, D1 = D + 1;
  const size_t nk = (size_t)D * D1, ng = (size_t)D * (D1 * (D1 + 1) / 2);
  auto work = [&](int s0, int step) {
    std::vector<double> W(nk);
    for (int s = s0; s < n_spk; s += step) {
      double impr = 0.0;
      const int32_t st = FmllrOne(o, D, beta_h[s], K_h + (size_t)s * nk, G_h + (size_t)s * ng, W.data(), &impr);
      if (status_h) status_h[s] = st;
      if (objf_impr_h) objf_impr_h[s] = impr;
      if (count_h) count_h[s] = beta_h[s];
      if (W64_h) memcpy(W64_h + (size_t)s * nk, W.data(), sizeof(double) * nk);
      if (W_h) for (size_t i = 0; i < nk; ++i) W_h[(size_t)s * nk + i] = (float)W[i];
    }
  };
  // speakers are independent: up to 16 threads, each its own speakers (the results do not depend on the thread count)
  const int nthr = (int)std::max(1u, std::min({16u, std::thread::hardware_concurrency(), (unsigned)n_spk}));
  if (nthr == 1) { work(0, 1); return KHG_OK; }
  std::vector<std::thread> th;
  for (int t = 0; t < nthr; ++t) th.emplace_back(work, t, nthr);
  for (auto& t : th) t.join();
  return KHG_OK;
}

// ---- MLLT estimate: the reference has no MLLT, the rule written there is the specification -------------------------
// Kaldi's MlltAccs::Update on the statistics of khg_mllt_stats_download, with the Gauss-Jordan forms of the fMLLR estimate above.  One
// IEEE fp64 operation at a time in the written order (contraction is off for this file from the fMLLR section on), every sum in index
// order: tests/mllt_ref.py restates it and agrees on the bits of M.
namespace {

// Q(A) = beta log |det A| - 1/2 sum_d A[d] G[d] A[d]^T; false: A is singular
bool MlltAuxf(int D, double beta, const double* G, const double* A, double* q, double* M, double* inv) {
  const int NP = D * (D + 1) / 2;
  for (int i = 0; i < D; ++i)
    for (int j = 0; j < D; ++j) M[i * D + j] = A[j * D + i];
  double ld = 0.0;
  if (!FmInvPiv(D, M, inv, &ld)) return false;
  double acc = 0.0;
  for (int d = 0; d < D; ++d) {
    const double* g = G + (size_t)d * NP;
    const double* a = A + (size_t)d * D;
    double t2 = 0.0;
    for (int i = 0; i < D; ++i) {
      double r = 0.0;
      for (int j = 0; j < D; ++j) r = r + g[j <= i ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i] * a[j];
      t2 = t2 + a[i] * r;
    }
    acc = acc + t2;
  }
  *q = beta * ld - 0.5 * acc;
  return true;
}

int32_t MlltOne(const khg_mllt_options* o, int D, double beta, const double* G, double* A, double* objf_impr) {
  const int NP = D * (D + 1) / 2;
  auto identity = [&] {
    for (int d = 0; d < D; ++d)
      for (int j = 0; j < D; ++j) A[d * D + j] = d == j ? 1.0 : 0.0;
  };
  identity();
  *objf_impr = 0.0;
  if (!(beta > 0.0) || !std::isfinite(beta)) return KHG_MLLT_SINGULAR;
  std::vector<double> invG((size_t)D * D * D), M((size_t)D * D), inv((size_t)D * D), c(D), v(D);
  for (int d = 0; d < D; ++d)
    if (!FmInvSym(D, G + (size_t)d * NP, M.data(), invG.data() + (size_t)d * D * D)) return KHG_MLLT_SINGULAR;
  double q0 = 0.0;
  if (!MlltAuxf(D, beta, G, A, &q0, M.data(), inv.data())) return KHG_MLLT_SINGULAR;
  for (int it = 0; it < o->num_iters; ++it)
    for (int d = 0; d < D; ++d) {
      for (int i = 0; i < D; ++i)
        for (int j = 0; j < D; ++j) M[i * D + j] = A[j * D + i];              // A^T
      double ld = 0.0;
      if (!FmInvPiv(D, M.data(), inv.data(), &ld)) { identity(); return KHG_MLLT_SINGULAR; }
      for (int j = 0; j < D; ++j) c[j] = inv[d * D + j];
      const double* ig = invG.data() + (size_t)d * D * D;
      for (int i = 0; i < D; ++i) {
        double r = 0.0;
        for (int j = 0; j < D; ++j) r = r + ig[i * D + j] * c[j];
        v[i] = r;
      }
      double cv = 0.0;
      for (int i = 0; i < D; ++i) cv = cv + c[i] * v[i];
      const double s = std::sqrt(beta / cv);
      if (!std::isfinite(s)) { identity(); return KHG_MLLT_SINGULAR; }
      for (int i = 0; i < D; ++i) A[d * D + i] = v[i] * s;
    }
  double q1 = 0.0;
  if (!MlltAuxf(D, beta, G, A, &q1, M.data(), inv.data())) { identity(); return KHG_MLLT_SINGULAR; }
  *objf_impr = q1 - q0;
  return KHG_MLLT_OK;
}

}  // namespace

extern "C" void khg_mllt_options_default(khg_mllt_options* o) { o->num_iters = 200; }

extern "C" int khg_mllt_compute(const khg_mllt_options* o, int32_t dim, double beta, const double* G_h, float* M_h, double* M64_h, double* objf_impr,
                                double* count, int32_t* status) {
  khg_mllt_options def;
  khg_mllt_options_default(&def);
  if (!o) o = &def;
  if (dim < 1 || !G_h || (!M_h && !M64_h)) return khg_set_error(KHG_E_ARG, "khg_mllt_compute: bad arguments");
  if (dim > KHG_MLLT_MAX_DIM) return khg_set_error(KHG_E_UNSUPPORTED, "khg_mllt_compute: dim " + std::to_string(dim) + " is above KHG_MLLT_MAX_DIM");
  if (o->num_iters < 0) return khg_set_error(KHG_E_ARG, "khg_mllt_compute: num_iters is negative");
  const size_t n = (size_t)dim * dim;
  std::vector<double> A(n);
  double impr = 0.0;
  const int32_t st = MlltOne(o, dim, beta, G_h, A.data(), &impr);
  if (status) *status = st;
  if (objf_impr) *objf_impr = impr;
  if (count) *count = beta;
  if (M64_h) memcpy(M64_h, A.data(), sizeof(double) * n);
  if (M_h) for (size_t i = 0; i < n; ++i) M_h[i] = (float)A[i];
  return KHG_OK;
}

// ---- LDA estimate: the reference has no LDA, the rule written there is the specification ---------------------------
// Kaldi's LdaEstimate::Estimate on the statistics of khg_lda_stats_download.  One IEEE fp64 operation at a time in the written order
// (contraction is off for this file from the fMLLR section on), every sum in index order.  tests/lda_ref.py restates the rule with
// numpy's Cholesky and eigh; the two agree to the residuals 7n records, not on the bits.
namespace {

constexpr int kLdaMaxSweeps = 64;

// The eigen-decomposition of the symmetric n x n matrix A by cyclic Jacobi (rows p < q in index order).  A is destroyed (its diagonal
// ends as the eigenvalues); Vt's ROWS end as the eigenvectors.  A pair is left alone when its off-diagonal element is exactly zero,
// is lost in the rounding of both its diagonal elements, or is below 2^-100 of the largest diagonal magnitude the matrix started
// with (then it is set to zero).  true: a full sweep rotated nothing.  false: kLdaMaxSweeps sweeps did not get there, or a value
// stopped being finite.
bool LdaJacobi(int n, double* A, double* Vt) {
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) Vt[(size_t)i * n + j] = i == j ? 1.0 : 0.0;
  double anorm = 0.0;
  for (int i = 0; i < n; ++i) anorm = std::max(anorm, std::fabs(A[(size_t)i * n + i]));
  if (!std::isfinite(anorm)) return false;
  const double tiny = std::ldexp(anorm, -100);
  for (int sweep = 0; sweep < kLdaMaxSweeps; ++sweep) {
    int rotated = 0;
    for (int p = 0; p + 1 < n; ++p)
      for (int q = p + 1; q < n; ++q) {
        const double apq = A[(size_t)p * n + q];
        if (apq == 0.0) continue;
        const double app = A[(size_t)p * n + p], aqq = A[(size_t)q * n + q], g = std::fabs(apq);
        if (!std::isfinite(apq)) return false;
        if (g <= tiny || (std::fabs(app) + g == std::fabs(app) && std::fabs(aqq) + g == std::fabs(aqq))) {
          A[(size_t)p * n + q] = 0.0; A[(size_t)q * n + p] = 0.0;
          continue;
        }
        ++rotated;
        const double theta = (aqq - app) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        double* rp = A + (size_t)p * n;
        double* rq = A + (size_t)q * n;
        for (int k = 0; k < n; ++k) {
          const double akp = rp[k], akq = rq[k];
          rp[k] = c * akp - s * akq;
          rq[k] = s * akp + c * akq;
        }
        rp[p] = app - t * apq; rq[q] = aqq + t * apq; rp[q] = 0.0; rq[p] = 0.0;
        for (int k = 0; k < n; ++k) { A[(size_t)k * n + p] = rp[k]; A[(size_t)k * n + q] = rq[k]; }
        double* vp = Vt + (size_t)p * n;
        double* vq = Vt + (size_t)q * n;
        for (int k = 0; k < n; ++k) {
          const double vkp = vp[k], vkq = vq[k];
          vp[k] = c * vkp - s * vkq;
          vq[k] = s * vkp + c * vkq;
        }
      }
    if (rotated == 0) return true;
  }
  return false;
}

// Mfull: n x n, eig: n, mu: n.  KHG_LDA_OK or KHG_LDA_SINGULAR (then the outputs are untouched).
int32_t LdaOne(const khg_lda_options* o, int C, int n, const double* zero, const double* first, const double* second, double* Mfull, double* eig,
               double* mu, double* count) {
  double N = 0.0;
  for (int c = 0; c < C; ++c) N = N + zero[c];
  *count = N;
  if (!(N > 0.0) || !std::isfinite(N)) return KHG_LDA_SINGULAR;
  const size_t nn = (size_t)n * n;
  std::vector<double> Bc(nn), Wc(nn), Lc(nn, 0.0), Li(nn, 0.0), T1(nn), P(nn), Vt(nn);
  for (int i = 0; i < n; ++i) {
    double s = 0.0;
    for (int c = 0; c < C; ++c) s = s + first[(size_t)c * n + i];
    mu[i] = s / N;
  }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j <= i; ++j) {
      const double mm = mu[i] * mu[j];
      double b = 0.0;
      for (int c = 0; c < C; ++c)
        if (zero[c] != 0.0) b = b + (first[(size_t)c * n + i] * first[(size_t)c * n + j]) / (N * zero[c]);
      b = b - mm;
      const double tc = second[(size_t)i * (i + 1) / 2 + j] / N - mm;
      Bc[(size_t)i * n + j] = b; Bc[(size_t)j * n + i] = b;
      Wc[(size_t)i * n + j] = tc - b; Wc[(size_t)j * n + i] = tc - b;
    }
  // Wc = Lc Lc^T
  for (int i = 0; i < n; ++i)
    for (int j = 0; j <= i; ++j) {
      double s = Wc[(size_t)i * n + j];
      for (int k = 0; k < j; ++k) s = s - Lc[(size_t)i * n + k] * Lc[(size_t)j * n + k];
      if (i == j) {
        if (!(std::isfinite(s) && s > 0.0)) return KHG_LDA_SINGULAR;
        Lc[(size_t)i * n + i] = std::sqrt(s);
      } else {
        Lc[(size_t)i * n + j] = s / Lc[(size_t)j * n + j];
      }
    }
  // Li = Lc^-1 (lower triangular), column by column
  for (int j = 0; j < n; ++j) {
    Li[(size_t)j * n + j] = 1.0 / Lc[(size_t)j * n + j];
    for (int i = j + 1; i < n; ++i) {
      double s = 0.0;
      for (int k = j; k < i; ++k) s = s + Lc[(size_t)i * n + k] * Li[(size_t)k * n + j];
      Li[(size_t)i * n + j] = -s / Lc[(size_t)i * n + i];
    }
  }
  // P = Li Bc Li^T, the lower triangle computed and mirrored
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      double s = 0.0;
      for (int k = 0; k <= i; ++k) s = s + Li[(size_t)i * n + k] * Bc[(size_t)k * n + j];
      T1[(size_t)i * n + j] = s;
    }
  for (int i = 0; i < n; ++i)
    for (int j = 0; j <= i; ++j) {
      double s = 0.0;
      for (int k = 0; k <= j; ++k) s = s + T1[(size_t)i * n + k] * Li[(size_t)j * n + k];
      P[(size_t)i * n + j] = s; P[(size_t)j * n + i] = s;
    }
  if (!LdaJacobi(n, P.data(), Vt.data())) return KHG_LDA_SINGULAR;      // NOT_CONVERGED is treated as SINGULAR
  std::vector<int> order(n);
  for (int i = 0; i < n; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return P[(size_t)a * n + a] > P[(size_t)b * n + b]; });
  const double f = o->within_class_factor;
  for (int i = 0; i < n; ++i) {
    const double lam = P[(size_t)order[i] * n + order[i]];
    if (!std::isfinite(lam)) return KHG_LDA_SINGULAR;
    const double* v = Vt.data() + (size_t)order[i] * n;
    double* row = T1.data() + (size_t)i * n;                              // T1 is free again: the rows of M_full before they are accepted
    for (int j = 0; j < n; ++j) {
      double s = 0.0;
      for (int k = j; k < n; ++k) s = s + v[k] * Li[(size_t)k * n + j];
      row[j] = s;
    }
    if (f != 1.0) {
      const double sc = std::sqrt((f + lam) / (1.0 + lam));
      if (!std::isfinite(sc)) return KHG_LDA_SINGULAR;
      for (int j = 0; j < n; ++j) row[j] = row[j] * sc;
    }
    int best = 0;
    for (int j = 1; j < n; ++j)
      if (std::fabs(row[j]) > std::fabs(row[best])) best = j;
    if (row[best] < 0.0)
      for (int j = 0; j < n; ++j) row[j] = -row[j];
    Wc[i] = lam;                                                          // Wc is free again: the sorted eigenvalues
  }
  memcpy(Mfull, T1.data(), sizeof(double) * nn);
  memcpy(eig, Wc.data(), sizeof(double) * (size_t)n);
  return KHG_LDA_OK;
}

}  // namespace

extern "C" void khg_lda_options_default(khg_lda_options* o) { o->target_dim = 40; o->remove_offset = 0; o->within_class_factor = 1.0; }

extern "C" int khg_lda_compute(const khg_lda_options* o, int32_t num_classes, int32_t dim_z, const double* zero_h, const double* first_h,
                               const double* second_h, float* M_h, double* M64_h, double* Mfull64_h, double* eig_h, double* count, int32_t* status) {
  khg_lda_options def;
  khg_lda_options_default(&def);
  if (!o) o = &def;
  if (num_classes < 1 || dim_z < 1 || !zero_h || !first_h || !second_h || (!M_h && !M64_h)) return khg_set_error(KHG_E_ARG, "khg_lda_compute: bad arguments");
  if (dim_z > KHG_LDA_MAX_SPLICED_DIM)
    return khg_set_error(KHG_E_UNSUPPORTED, "khg_lda_compute: dim " + std::to_string(dim_z) + " is above KHG_LDA_MAX_SPLICED_DIM");
  if (o->target_dim < 1 || o->target_dim > dim_z)
    return khg_set_error(KHG_E_ARG, "khg_lda_compute: target_dim " + std::to_string(o->target_dim) + " is outside 1 .. " + std::to_string(dim_z));
  if (!std::isfinite(o->within_class_factor)) return khg_set_error(KHG_E_ARG, "khg_lda_compute: within_class_factor is not finite");
  const int n = dim_z, T = o->target_dim, MW = n + (o->remove_offset ? 1 : 0);
  std::vector<double> Mfull((size_t)n * n, 0.0), eig((size_t)n, 0.0), mu((size_t)n, 0.0), M((size_t)T * MW, 0.0);
  for (int i = 0; i < n; ++i) Mfull[(size_t)i * n + i] = 1.0;
  double N = 0.0;
  const int32_t st = LdaOne(o, num_classes, n, zero_h, first_h, second_h, Mfull.data(), eig.data(), mu.data(), &N);
  for (int i = 0; i < T; ++i) {
    for (int j = 0; j < n; ++j) M[(size_t)i * MW + j] = Mfull[(size_t)i * n + j];
    if (o->remove_offset && st == KHG_LDA_OK) {
      double s = 0.0;
      for (int j = 0; j < n; ++j) s = s + Mfull[(size_t)i * n + j] * mu[j];
      M[(size_t)i * MW + n] = -s;
    }
  }
  if (status) *status = st;
  if (count) *count = N;
  if (M64_h) memcpy(M64_h, M.data(), sizeof(double) * M.size());
  if (M_h) for (size_t i = 0; i < M.size(); ++i) M_h[i] = (float)M[i];
  if (Mfull64_h) memcpy(Mfull64_h, Mfull.data(), sizeof(double) * Mfull.size());
  if (eig_h) memcpy(eig_h, eig.data(), sizeof(double) * eig.size());
  return KHG_OK;
}
