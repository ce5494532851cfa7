// kaldi_hmm_gmm_amd/csrc/khg_host_feat.cpp -- the host side of CMVN and delta features: Kaldi's ApplyCmvn normaliser
// from the statistics (khg_cmvn_compute) and DeltaFeatures' coefficient tables (khg_delta_scales).  One operation at a time, in the
// written order: built with -ffp-contract=off, so that s2 / count - mean * mean is two roundings, not a fused one.
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/khg_hip.h"

int khg_set_error(int code, const std::string& msg);      // khg_ctx_model.hip

extern "C" int khg_cmvn_compute(int32_t n_spk, int32_t dim, const double* stats_h, int32_t norm_means, int32_t norm_vars, int32_t reverse,
                                float* norm_h, int32_t* status_h) {
  if (n_spk < 0 || dim < 1 || !stats_h || !norm_h) return khg_set_error(KHG_E_ARG, "khg_cmvn_compute: bad arguments");
  const size_t D = (size_t)dim;
  for (int32_t s = 0; s < n_spk; ++s) {
    const double* s1 = stats_h + (size_t)s * 2 * (D + 1);
    const double* s2 = s1 + (D + 1);
    float* off = norm_h + (size_t)s * 2 * D;
    float* scl = off + D;
    const double count = s1[D];
    int32_t st = (count >= 1.0) ? KHG_CMVN_OK : KHG_CMVN_NO_DATA;      // a NaN count is NO_DATA
    if (st == KHG_CMVN_OK)
      for (size_t d = 0; d < D; ++d) {
        const double mean = s1[d] / count;
        double scale = 1.0, offset = -mean;
        if (norm_vars) {
          double var = s2[d] / count - mean * mean;
          if (var < 1e-20) var = 1e-20;
          scale = 1.0 / std::sqrt(var);
          offset = -(mean * scale);
          if (reverse) scale = std::sqrt(var);
        }
        if (reverse) offset = mean;
        off[d] = (float)offset;
        scl[d] = (float)scale;
        if (!std::isfinite(off[d]) || !std::isfinite(scl[d])) st = KHG_CMVN_NONFINITE;      // judged before norm_means: the status does not depend on it
        if (!norm_means) off[d] = 0.0f;
      }
    if (st != KHG_CMVN_OK)
      for (size_t d = 0; d < D; ++d) { off[d] = 0.0f; scl[d] = 1.0f; }
    if (status_h) status_h[s] = st;
  }
  return KHG_OK;
}

extern "C" int khg_delta_scales(int32_t order, int32_t window, float* scales_h) {
  if (order < 0 || window < 1 || !scales_h) return khg_set_error(KHG_E_ARG, "khg_delta_scales: order must be >= 0 and window >= 1");
  std::vector<float> prev{1.0f}, cur;
  scales_h[0] = 1.0f;
  size_t at = 1;
  for (int32_t i = 1; i <= order; ++i) {
    const int po = (int)(prev.size() - 1) / 2, co = po + window;
    cur.assign((size_t)(2 * co + 1), 0.0f);
    float normalizer = 0.0f;
    for (int j = -window; j <= window; ++j) {
      normalizer += (float)(j * j);
      for (int k = -po; k <= po; ++k) cur[(size_t)(j + k + co)] += (float)j * prev[(size_t)(k + po)];
    }
    const float inv = (float)(1.0 / normalizer);
    for (float& c : cur) c *= inv;
    for (float c : cur) scales_h[at++] = c;
    prev.swap(cur);
  }
  return KHG_OK;
}
