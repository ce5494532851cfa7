// kaldi_hmm_gmm_amd/csrc/khg_host_feat.cpp -- the host side of CMVN and delta features: Kaldi's ApplyCmvn normaliser
// from the statistics (khg_cmvn_compute) and DeltaFeatures' coefficient tables (khg_delta_scales); and of the waveform front end
// (DESIGN.md 7q): its options, frame counts and tables (khg_frontend_opts_default, _dims, _num_frames, _tables).  One operation at a
// time, in the written order: built with -ffp-contract=off, so that s2 / count - mean * mean is two roundings, not a fused one.
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

// ---- the waveform front end: options, frame counts and the tables.  Everything in double by the written operations
// (libm cos, pow, log, sin), narrowed to float once.
extern "C" void khg_frontend_opts_default(khg_frontend_opts* o) {
  if (!o) return;
  *o = khg_frontend_opts{KHG_FE_MFCC, 16000.0f, 25.0f, 10.0f, 0.97f, 1, KHG_WIN_POVEY, 0.42f, 1, 1, 0.0f, 23, 20.0f, 0.0f, 1.0f, 0, 13, 22.0f, 0, 1, 0.0f, 1, 1};
}

namespace {
constexpr double kPi = 3.14159265358979323846;
struct FeDims { int32_t L, S, N, B, C, out_dim, n_w; double high; };
inline double mel_scale(double f) { return 1127.0 * std::log(1.0 + f / 700.0); }

// the filters' runs: filter b covers the spectrum bins k of 0 .. N / 2 - 1 with left < mel(k) < right
void mel_runs(const khg_frontend_opts& o, const FeDims& d, std::vector<int32_t>* off, std::vector<int32_t>* len, std::vector<float>* w) {
  const double width = (double)o.samp_freq / d.N;
  const double mel_low = mel_scale((double)o.low_freq), mel_high = mel_scale(d.high);
  const double delta = (mel_high - mel_low) / (d.B + 1);
  off->assign((size_t)d.B, 0); len->assign((size_t)d.B, 0); w->clear();
  for (int b = 0; b < d.B; ++b) {
    const double left = mel_low + b * delta, center = mel_low + (b + 1) * delta, right = mel_low + (b + 2) * delta;
    int first = -1;
    for (int k = 0; k < d.N / 2; ++k) {
      const double mel = mel_scale(width * k);
      if (mel > left && mel < right) {
        const double weight = (mel <= center) ? (mel - left) / (center - left) : (right - mel) / (right - center);
        if (first < 0) first = k;
        w->push_back((float)weight);
        (*len)[(size_t)b]++;
      }
    }
    (*off)[(size_t)b] = first < 0 ? 0 : first;
  }
}

int fe_dims(const khg_frontend_opts* o, const char* name, FeDims* d) {
  const std::string who = std::string(name) + ": ";
  if (!o) return khg_set_error(KHG_E_ARG, who + "bad arguments");
  if (o->kind != KHG_FE_MFCC && o->kind != KHG_FE_FBANK) return khg_set_error(KHG_E_ARG, who + "kind must be KHG_FE_MFCC or KHG_FE_FBANK");
  if (o->window_type < KHG_WIN_POVEY || o->window_type > KHG_WIN_BLACKMAN) return khg_set_error(KHG_E_ARG, who + "unknown window_type");
  for (float v : {o->samp_freq, o->frame_length_ms, o->frame_shift_ms, o->preemph_coeff, o->blackman_coeff, o->dither, o->low_freq, o->high_freq, o->vtln_warp,
                  o->cepstral_lifter, o->energy_floor})
    if (!std::isfinite(v)) return khg_set_error(KHG_E_ARG, who + "an option is not finite");
  if (o->dither != 0.0f) return khg_set_error(KHG_E_UNSUPPORTED, who + "dither must be 0 (dither is random; the default here is 0)");
  if (!o->round_to_power_of_two) return khg_set_error(KHG_E_UNSUPPORTED, who + "round_to_power_of_two = false is not supported");
  if (o->vtln_warp != 1.0f) return khg_set_error(KHG_E_UNSUPPORTED, who + "vtln_warp must be 1 (VTLN is not supported)");
  if (o->htk_compat) return khg_set_error(KHG_E_UNSUPPORTED, who + "htk_compat is not supported");
  if (!(o->samp_freq > 0.0f) || !(o->frame_length_ms > 0.0f) || !(o->frame_shift_ms > 0.0f) || o->samp_freq > 1e6f || o->frame_length_ms > 1e4f || o->frame_shift_ms > 1e4f)
    return khg_set_error(KHG_E_ARG, who + "samp_freq, frame_length_ms and frame_shift_ms must be positive");
  if (o->energy_floor < 0.0f || o->preemph_coeff < 0.0f || o->preemph_coeff > 1.0f) return khg_set_error(KHG_E_ARG, who + "energy_floor must be >= 0 and preemph_coeff in 0 .. 1");
  d->L = (int32_t)(o->samp_freq * 0.001 * o->frame_length_ms);
  d->S = (int32_t)(o->samp_freq * 0.001 * o->frame_shift_ms);
  if (d->L < 2 || d->S < 1) return khg_set_error(KHG_E_ARG, who + "a frame needs at least two samples and a shift at least one");
  int64_t N = 1;
  while (N < d->L) N *= 2;
  if (N != 256 && N != 512 && N != 1024)
    return khg_set_error(KHG_E_UNSUPPORTED, who + "frame_length_ms gives a padded window of " + std::to_string(N) + " samples; 256, 512 and 1024 are supported");
  d->N = (int32_t)N;
  if (o->num_mel_bins < 3 || o->num_mel_bins > 128) return khg_set_error(KHG_E_UNSUPPORTED, who + "num_mel_bins must be in 3 .. 128");
  d->B = o->num_mel_bins;
  d->C = 0;
  if (o->kind == KHG_FE_MFCC) {
    if (o->num_ceps < 1) return khg_set_error(KHG_E_ARG, who + "num_ceps must be >= 1");
    if (o->num_ceps > o->num_mel_bins) return khg_set_error(KHG_E_UNSUPPORTED, who + "num_ceps must not exceed num_mel_bins");
    d->C = o->num_ceps;
  }
  const double nyquist = 0.5 * (double)o->samp_freq;
  d->high = (double)o->high_freq;
  if (o->high_freq <= 0.0f) d->high += nyquist;
  if (o->low_freq < 0.0f || (double)o->low_freq >= nyquist || d->high <= 0.0 || d->high > nyquist || d->high <= (double)o->low_freq)
    return khg_set_error(KHG_E_ARG, who + "low_freq and high_freq must satisfy 0 <= low_freq < high_freq <= Nyquist");
  d->out_dim = o->kind == KHG_FE_MFCC ? d->C : d->B + (o->use_energy ? 1 : 0);
  d->n_w = 0;                                                  // the filters are built only where they are wanted (khg_frontend_dims, _tables)
  return KHG_OK;
}
}  // namespace

extern "C" int khg_frontend_dims(const khg_frontend_opts* o, int32_t* dims_h) {
  FeDims d;
  if (!dims_h) return khg_set_error(KHG_E_ARG, "khg_frontend_dims: bad arguments");
  int rc = fe_dims(o, "khg_frontend_dims", &d);
  if (rc) return rc;
  {
    std::vector<int32_t> off, len; std::vector<float> w;
    mel_runs(*o, d, &off, &len, &w);
    d.n_w = (int32_t)w.size();
  }
  const int32_t v[8] = {d.L, d.S, d.N, d.B, d.C, d.out_dim, d.n_w, 0};
  for (int i = 0; i < 8; ++i) dims_h[i] = v[i];
  return KHG_OK;
}

extern "C" int khg_frontend_num_frames(const khg_frontend_opts* o, int64_t n_samples, int64_t* num_frames) {
  FeDims d;
  if (!num_frames || n_samples < 0) return khg_set_error(KHG_E_ARG, "khg_frontend_num_frames: bad arguments");
  int rc = fe_dims(o, "khg_frontend_num_frames", &d);
  if (rc) return rc;
  if (o->snip_edges) *num_frames = n_samples < d.L ? 0 : 1 + (n_samples - d.L) / d.S;
  else *num_frames = (n_samples + d.S / 2) / d.S;
  return KHG_OK;
}

extern "C" int khg_frontend_tables(const khg_frontend_opts* o, float* window_h, int32_t* mel_off_h, int32_t* mel_len_h, float* mel_w_h, float* dct_h, float* lifter_h,
                                   float* twiddle_h) {
  FeDims d;
  int rc = fe_dims(o, "khg_frontend_tables", &d);
  if (rc) return rc;
  if (window_h) {
    const double a = 2.0 * kPi / (d.L - 1);
    for (int i = 0; i < d.L; ++i) {
      const double x = (double)i;
      double w = 1.0;
      switch (o->window_type) {
        case KHG_WIN_HANNING: w = 0.5 - 0.5 * std::cos(a * x); break;
        case KHG_WIN_HAMMING: w = 0.54 - 0.46 * std::cos(a * x); break;
        case KHG_WIN_POVEY: w = std::pow(0.5 - 0.5 * std::cos(a * x), 0.85); break;
        case KHG_WIN_BLACKMAN: w = (double)o->blackman_coeff - 0.5 * std::cos(a * x) + (0.5 - (double)o->blackman_coeff) * std::cos(2.0 * a * x); break;
        default: break;
      }
      window_h[i] = (float)w;
    }
  }
  if (mel_off_h || mel_len_h || mel_w_h) {
    std::vector<int32_t> off, len; std::vector<float> w;
    mel_runs(*o, d, &off, &len, &w);
    for (int b = 0; b < d.B; ++b) {
      if (mel_off_h) mel_off_h[b] = off[(size_t)b];
      if (mel_len_h) mel_len_h[b] = len[(size_t)b];
    }
    if (mel_w_h) for (size_t i = 0; i < w.size(); ++i) mel_w_h[i] = w[i];
  }
  if (dct_h) {                                                  // the first num_ceps rows of ComputeDctMatrix of [bins][bins]
    const double n0 = std::sqrt(1.0 / d.B), n1 = std::sqrt(2.0 / d.B);
    for (int c = 0; c < d.C; ++c)
      for (int b = 0; b < d.B; ++b) dct_h[(size_t)c * d.B + b] = (float)(c == 0 ? n0 : n1 * std::cos(kPi / d.B * (b + 0.5) * c));
  }
  if (lifter_h) {
    const double Q = (double)o->cepstral_lifter;
    for (int c = 0; c < d.C; ++c) lifter_h[c] = (float)(Q != 0.0 ? 1.0 + 0.5 * Q * std::sin(kPi * c / Q) : 1.0);
  }
  if (twiddle_h)
    for (int k = 0; k < d.N / 2; ++k) {
      const double ang = 2.0 * kPi * k / d.N;
      twiddle_h[2 * k] = (float)std::cos(ang);
      twiddle_h[2 * k + 1] = (float)(-std::sin(ang));
    }
  return KHG_OK;
}
