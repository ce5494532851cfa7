// kaldi_hmm_gmm_amd/csrc/khg_k3.hip -- C-ABI (include/khg_hip.h): the accumulator block and K3, sufficient statistics
// (khg_acc_stats / khg_acc_stats_reduce; khg_acc_stats_post from posteriors): bucketing of frames by pdf, work items, form selection,
// the launches.  gfx950 only.
#include "khg_internal.hpp"

#include <hipcub/hipcub.hpp>   // DeviceRadixSort: the stable (pdf, frame) sort of K3's bucketing

#include "khg_k3_accstats.hip.inc"
#include "khg_k3_post.hip.inc"
#include "khg_k3_accops.hip.inc"

// ------------------------------------------------------------------------------------------
// accumulators + K3
extern "C" int khg_accs_create(khg_ctx* ctx, const khg_model* m, const khg_tm* tm, khg_accs** out) {
  if (ctx_dead(ctx) || !m || !tm || !out) return khg_set_error(KHG_E_ARG, "khg_accs_create: bad arguments");
  khg_accs* a = new khg_accs();
  a->ctx = ctx; a->sumG = m->sumG; a->D = m->D; a->num_tids = tm->num_tids;
  a->n = a->sumG * (1 + 2 * (int64_t)a->D) + a->num_tids + 1 + 8;
  int rc = dev_alloc(&a->buf_d, (size_t)a->n);
  if (rc) { delete a; return rc; }
  a->cap = a->n;
  *out = a;
  return khg_accs_zero(ctx, a);
}
extern "C" int khg_accs_destroy(khg_accs* a) { if (a) { DEVFREE(a->buf_d); DEVFREE(a->wire_d); delete a; } return KHG_OK; }
extern "C" int khg_accs_zero(khg_ctx* ctx, khg_accs* a) {
  if (ctx_dead(ctx) || !a) return khg_set_error(KHG_E_ARG, "bad arguments");
  HIPCHK(hipMemsetAsync(a->buf_d, 0, sizeof(double) * (size_t)a->n, ctx->stream));
  return KHG_OK;
}
extern "C" int khg_accs_size(const khg_accs* a, int64_t* n) { if (!a || !n) return khg_set_error(KHG_E_ARG, "bad arguments"); *n = a->n; return KHG_OK; }
extern "C" int khg_accs_device_ptr(const khg_accs* a, void** p) { if (!a || !p) return khg_set_error(KHG_E_ARG, "bad arguments"); *p = a->buf_d; return KHG_OK; }
extern "C" int khg_accs_download(khg_ctx* ctx, const khg_accs* a, double* buf) {
  if (ctx_dead(ctx) || !a || !buf) return khg_set_error(KHG_E_ARG, "bad arguments");
  { int rc = check_err_flag(ctx, "khg_acc_stats"); if (rc) return rc; }
  HIPCHK(hipMemcpyAsync(buf, a->buf_d, sizeof(double) * (size_t)a->n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return KHG_OK;
}
extern "C" int khg_accs_upload(khg_ctx* ctx, khg_accs* a, const double* buf) {
  if (ctx_dead(ctx) || !a || !buf) return khg_set_error(KHG_E_ARG, "bad arguments");
  HIPCHK(hipMemcpyAsync(a->buf_d, buf, sizeof(double) * (size_t)a->n, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return KHG_OK;
}

// gmm-sum-accs / gmm-ismooth-stats on blocks resident in HBM (khg_k3_accops.hip.inc); asynchronous on the context's stream
static int accs_pair_check(const khg_ctx* ctx, const khg_accs* dst, const khg_accs* src, const char* where) {
  if (dst->ctx != ctx || src->ctx != ctx) return khg_set_error(KHG_E_ARG, std::string(where) + ": an accumulator block belongs to another context");
  if (dst->sumG != src->sumG || dst->D != src->D || dst->num_tids != src->num_tids || dst->n != src->n)
    return khg_set_error(KHG_E_ARG, std::string(where) + ": the two blocks have different layouts");
  return KHG_OK;
}
static inline int accs_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(4096, (n + 255) / 256)); }
extern "C" int khg_accs_add(khg_ctx* ctx, khg_accs* dst, float scale, const khg_accs* src) {
  if (ctx_dead(ctx) || !dst || !src) return khg_set_error(KHG_E_ARG, "khg_accs_add: bad arguments");
  if (!std::isfinite(scale)) return khg_set_error(KHG_E_ARG, "khg_accs_add: the scale is not finite");
  { int rc = accs_pair_check(ctx, dst, src, "khg_accs_add"); if (rc) return rc; }
  KernelTimer kt(ctx, "k3_accs_add");
  KHG_LAUNCH(ctx, k3_accs_add, dim3(accs_grid(dst->n)), dim3(256), 0, ctx->stream, dst->buf_d, src->buf_d, (double)scale, dst->n);
  HIPCHK(hipGetLastError());
  return KHG_OK;
}
extern "C" int khg_accs_scale(khg_ctx* ctx, khg_accs* dst, float f) {
  if (ctx_dead(ctx) || !dst) return khg_set_error(KHG_E_ARG, "khg_accs_scale: bad arguments");
  if (!std::isfinite(f)) return khg_set_error(KHG_E_ARG, "khg_accs_scale: the scale is not finite");
  if (dst->ctx != ctx) return khg_set_error(KHG_E_ARG, "khg_accs_scale: the accumulator block belongs to another context");
  KernelTimer kt(ctx, "k3_accs_scale");
  KHG_LAUNCH(ctx, k3_accs_scale, dim3(accs_grid(dst->n)), dim3(256), 0, ctx->stream, dst->buf_d, (double)f, dst->n);
  HIPCHK(hipGetLastError());
  return KHG_OK;
}
extern "C" int khg_accs_smooth_with_accum(khg_ctx* ctx, khg_accs* dst, float tau, const khg_accs* src, const khg_model* m, int32_t* untouched_out) {
  if (ctx_dead(ctx) || !dst || !src || !m) return khg_set_error(KHG_E_ARG, "khg_accs_smooth_with_accum: bad arguments");
  if (!std::isfinite(tau)) return khg_set_error(KHG_E_ARG, "khg_accs_smooth_with_accum: tau is not finite");
  { int rc = accs_pair_check(ctx, dst, src, "khg_accs_smooth_with_accum"); if (rc) return rc; }
  if (dst->sumG != m->sumG || dst->D != m->D) return khg_set_error(KHG_E_ARG, "khg_accs_smooth_with_accum: accumulator / model layouts differ");
  int32_t* cnt_d = nullptr;
  if (untouched_out) {
    int rc = dev_alloc(&cnt_d, 1);
    if (rc) return rc;
    hipError_t e = hipMemsetAsync(cnt_d, 0, sizeof(int32_t), ctx->stream);
    if (e != hipSuccess) { DEVFREE(cnt_d); return khg_set_error(KHG_E_HIP, hipGetErrorString(e)); }
  }
  hipError_t e = hipSuccess;
  if (dst->sumG > 0) {
    KernelTimer kt(ctx, "k3_accs_smooth");
    KHG_LAUNCH(ctx, k3_accs_smooth, dim3((unsigned)((dst->sumG + 3) / 4)), dim3(256), 0, ctx->stream, dst->occ(), dst->mean(), dst->var(), src->occ(),
               src->mean(), src->var(), (double)tau, dst->sumG, (int)dst->D, cnt_d);
    e = hipGetLastError();
  }
  if (untouched_out) {
    int32_t cnt = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&cnt, cnt_d, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    DEVFREE(cnt_d);
    if (e == hipSuccess) *untouched_out = cnt;
  }
  if (e != hipSuccess) return khg_set_error(KHG_E_HIP, hipGetErrorString(e));
  return KHG_OK;
}

// K3's phase A on the fp16 matrix cores (khg_k3_accstats.hip.inc, k3_accumulate_wave<NB, true>): the scale exponents come from the
// MODEL alone -- every rank of a sharded run derives the same ones, so the statistics do not depend on the sharding: per
// dimension the features are expected inside xb = max_g (|mean| + 8 sigma); x' = x 2^ex peaks in [2^12, 2^13) there (fp16 overflows
// at ~8 xb), fl(x^2)' in [2^9, 2^10) (same limit), and the largest weight column peaks in [2^14, 2^15) (S).  *use = false (the fp32
// phase A runs) when the model side of the f16x2s domain fails (khg_k1_f16x2s.hip.inc: the absolute part of the error bound,
// evaluated at xb, above 4e-6; |S| > 40; the log-sum-exp's 2^28 bound at 16 xb) or when a feature of THIS set overflows fp16.
static int k3_phase_a_scales(khg_ctx* ctx, khg_model* m, khg_utts* u, bool* use) {
  *use = false;
  const int D = m->D, K = 8 * m->KQ;           // 80 exponents at D <= 40 (the wave forms), 160 at D <= 80 (k3_accumulate_block16)
  if (m->KQ == 0) return KHG_OK;
  std::vector<float> xk;
  int rc = k1_maxima(ctx, m, u, &xk);          // the set's column maxima (cached) and the model's (wmax, gcmax; cached per version)
  if (rc) return rc;
  if (m->k3_xb.empty()) {
    if (m->wmax.empty() || (int)m->k3_xb_raw.size() != D) { m->wmax.clear(); rc = model_stats(ctx, m); if (rc) return rc; }
    m->k3_xb = m->k3_xb_raw;          // (read with the column maxima: k0_model_stats, one pass per parameter version)
    m->k3_ex.assign((size_t)K, 0);
    bool ok = true;
    for (int d = 0; d < D; ++d) {
      const float xb = m->k3_xb[(size_t)d];
      if (!(xb > 0.0f) || !(xb < 1.0e18f)) { ok = false; break; }
      m->k3_ex[(size_t)2 * d] = 12 - std::ilogb(xb);               // xb 2^ex in [2^12, 2^13): fp16 overflows beyond 8 xb
      m->k3_ex[(size_t)2 * d + 1] = 9 - std::ilogb(xb * xb);        // xb^2 2^ex in [2^9, 2^10): beyond 8 xb as well
    }
    int S = INT_MAX;
    if (ok) {
      for (int k = 0; k < 2 * D; ++k) if (m->wmax[(size_t)k] > 0.0f) S = std::min(S, 14 - std::ilogb(m->wmax[(size_t)k]) + m->k3_ex[(size_t)k]);
      if (S == INT_MAX) S = 0;
      if (S < -40 || S > 40) ok = false;
    }
    if (ok) {
      double floor_sum = 0.0, bound = (double)m->gcmax;
      for (int k = 0; k < 2 * D; ++k) {
        const double xbk = (k & 1) ? (double)m->k3_xb[(size_t)(k >> 1)] * (double)m->k3_xb[(size_t)(k >> 1)] : (double)m->k3_xb[(size_t)(k >> 1)];
        floor_sum += std::ldexp((double)m->wmax[(size_t)k], S - m->k3_ex[(size_t)k]) + std::ldexp(xbk, m->k3_ex[(size_t)k]);
        bound += (double)m->wmax[(size_t)k] * xbk * ((k & 1) ? 128.0 : 16.0);
      }
      // (4e-6: the headroom for features outside the model's envelope costs two bits against K1s, whose planes peak at 2^14 by
      //  construction; the fp32 chain this replaces carries ~7e-7 B, i.e. ~1e-4 at the same shapes)
      if (!(std::ldexp(floor_sum, -25 - S) <= 4.0e-6) || !(bound <= 268435456.0)) ok = false;
      if (ctx->opt[KHG_OPT_DEBUG]) fprintf(stderr, "[khg] K3 fp16 phase A: S %d, floor %.3g, bound %.3g -> %s\n", S, std::ldexp(floor_sum, -25 - S), bound, ok ? "on" : "off");
    }
    m->k3_S = ok ? S : 0;
    m->k3_f16_ok = ok;
    if (ok) {
      if (!m->k3_ex_d) { rc = dev_alloc(&m->k3_ex_d, (size_t)K); if (rc) return rc; }
      HIPCHK(hipMemcpyAsync(m->k3_ex_d, m->k3_ex.data(), sizeof(int32_t) * (size_t)K, hipMemcpyHostToDevice, ctx->stream));
      HIPCHK(hipStreamSynchronize(ctx->stream));
    }
  }
  if (!m->k3_f16_ok) return KHG_OK;
  for (int k = 0; k < 2 * D; ++k)
    if (!(std::ldexp((double)xk[(size_t)k], m->k3_ex[(size_t)k]) < 65504.0)) return KHG_OK;     // a feature beyond 64 xb: fp32 phase A for this set
  *use = true;
  return KHG_OK;
}

// LDS of the VALU form (k3_accumulate) for a widest pdf of maxG Gaussians: the chunk's rows, gammas and reductions
static size_t k3_valu_lds(const khg_model* m, int maxG, bool post) {
  return sizeof(float) * (size_t)K3_CHUNK * ((size_t)(m->KQ ? 4 * m->KQ : (m->D | 1)) + (maxG | 1) + (post ? 5 : 4));
}
#define K3_VALU_LDS_MAX (160 * 1024)
// ------------------------------------------------------------------------------------------
// The ONE dispatch rule of the statistics pass: which accumulate form takes which pdfs, with how many slices per pdf, which bounds
// for the work-item buffers, which block size and dynamic LDS.  The form is chosen per pdf, so the answer is one RUN -- a class of
// pdfs (cls_lo < Gaussians <= cls_hi) with its form -- or two: one pdf that Split (csrc/diag-gmm.cc:780-851) pushed past 64
// Gaussians does not take every other pdf off the wave form.  acc_stats_pass launches what this says and k3_post_check asks it for
// the one refusal; nothing is launched or allocated here.
enum K3Form { K3F_WAVE, K3F_MFMA, K3F_VALU };
struct K3Run {
  int form = K3F_VALU;
  int cls_lo = 0, cls_hi = INT_MAX;          // the run's class of pdfs; the others get no work item
  int maxG = 0, n_cls = 0;                   // the widest pdf of the class; the pdfs a range's grid counts at most (wave form: all P)
  bool second = false;                       // the second class of a mixed call keeps its items in the upper halves of the buffers
  int NB = 0, NB16 = 0, nwv16 = 4;           // Gaussian blocks: of 16 per block (wave), of 64 per wave (MFMA); k3_accumulate_block16's, and its waves (else 4)
  int ny = 1;                                // slices per pdf, before k3_make_items cuts a far-above-average bucket finer
  bool parked = false;                       // the slices park images (wave form), of nsum1 doubles each
  size_t nsum1 = 0;
  int target = 0;                            // work items, from N and P alone (the bucket sizes stay on the device): frames per extra slice,
  int64_t extra_blocks = 0, max_items = 0, max_slots = 0;   // ... blocks beyond pdfs x ny, and what the buffers must hold
  // The fp16 phases rest on model-derived scales (k3_phase_a_scales: device work, cached per parameter version) and on the weight
  // being an ordinary number: the plan says what MAY run, the run settles it once when it starts.
  bool may_f16a = false, may_f16b = false;
  bool may_planes = false;                   // k3_accumulate_wave16 may read the set's split feature records (k3_planes settles it when the run starts)
  size_t lds[3] = {0, 0, 0};                 // dynamic LDS: fp32 phase A | fp16 phase A | both phases on the fp16 matrix cores
  bool too_wide = false;                     // VALU form: the widest pdf does not fit the LDS chunk buffers
};
struct K3Plan { int nruns = 0; K3Run run[2]; };

static K3Plan k3_plan(const khg_ctx* ctx, const khg_model* m, bool post, int64_t Neff, bool one_block) {
  const int P = m->P, KQ = m->KQ;
  const int k3form = ctx->opt[KHG_OPT_K3_FORM];     // 1: the chunk-per-block MFMA form for every shape; 2: the VALU form
  const int pha = ctx->opt[KHG_OPT_K3_PHASE_A], phb = ctx->opt[KHG_OPT_K3_PHASE_B], ny_opt = ctx->opt[KHG_OPT_K3_NY];
  const int64_t avg = Neff / std::max(1, P);
  // Work items (k3_make_items): ny slices per pdf, more for a pdf whose bucket is far above the average slice (2 x; silence in real
  // transcripts).  (one_block: no bucket is cut, so every cell of the block receives ONE work item's sum, made in chunk order -- the
  // fp64 atomics that end an item then have no second item to race with, and the statistics have the same bits from run to run)
  auto items = [&](K3Run& r) {
    r.target = one_block ? INT_MAX : (int)std::min<int64_t>(1 << 30, std::max<int64_t>(512, 2 * avg / r.ny));
    const int64_t per_t = Neff / r.target;
    r.extra_blocks = std::min<int64_t>(per_t + P, 2 * per_t) + 1;
    r.max_items = (int64_t)P * r.ny + r.extra_blocks;
    r.max_slots = !r.parked ? INT_MAX : r.ny > 1 ? r.max_items : 2 * per_t + 1;
  };
  // ---- the wave-local form (pdfs of <= 64 Gaussians at D <= 40): W in LDS + per-wave planes during the tile loop, the fp64 fold image afterwards ----
  auto wave = [&](int cls_lo, int cls_hi, int maxG) {
    K3Run r;
    r.form = K3F_WAVE; r.cls_lo = cls_lo; r.cls_hi = cls_hi; r.maxG = maxG; r.n_cls = P;
    const size_t nb = (size_t)(r.NB = (maxG + 15) / 16);
    // phase A on the fp16 matrix cores where the model-derived scales hold (KHG_K3_PHASEA=f32 keeps the fp32 chain; so does
    // KHG_OPT_K3_PHASE_B = 1); phase B there as well (k3_accumulate_wave16; KHG_OPT_K3_PHASE_B = 2) where phase A's split planes exist
    // (pdfs of <= 32 Gaussians keep the fp32 chain: 40 MFMAs per tile are not worth the split, and the two-waves-per-SIMD instantiations have no registers for the fp16 W pieces)
    r.may_f16a = nb >= 3 && pha == 0 && phb != 1; r.may_f16b = phb == 2;
    // fp32 phase A: W + the waves' planes; fp16 phase A: the waves' planes + their split planes; k3_accumulate_wave16: per wave two
    // tiles' split planes (halves; one frame-major image for both phases), then the split W operands; then, in each, the fold image
    const size_t fold = sizeof(double) * (nb * 16 * 80 + nb * 16);
    r.lds[0] = std::max<size_t>(sizeof(float) * (nb * 20 * 64 + 4 * 4 * 16 * 20), fold);
    r.lds[1] = std::max<size_t>(sizeof(float) * (4 * 4 * 16 * 20) + 2 * (size_t)(4 * 2 * 16 * K3_XH_ROW), fold);
    r.lds[2] = std::max<size_t>(2 * (size_t)4 * (2 * (2 * 16 * K3_X16_ROW)) + nb * 3 * 2 * 64 * 16, fold);
    r.may_planes = r.may_f16b && ctx->opt[KHG_OPT_K3_PLANES] != 1;
    const int64_t avg_tiles = (avg + 15) / 16;
    r.ny = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(32, (avg_tiles + 15) / 16), (4096 + P - 1) / P));
    if (ny_opt > 0) r.ny = ny_opt;
    // per-pdf log-like partials (always) and, with several blocks per pdf, the slice images they park
    r.parked = true; r.nsum1 = nb * 16 * 80 + nb * 16 + 1;
    items(r);
    return r;
  };
  // ---- the chunk-per-block forms: fp32 + fp64 MFMA (fewer, longer blocks: the fp64 accumulators stay in registers per block); VALU (any size) ----
  auto block = [&](int form, int cls_lo, int cls_hi, int maxG, int n_cls, bool second) {
    K3Run r;
    r.form = form; r.cls_lo = cls_lo; r.cls_hi = cls_hi; r.maxG = maxG; r.n_cls = n_cls; r.second = second;
    const int64_t avg_chunks = (avg + K3_CHUNK - 1) / K3_CHUNK;
    if (form == K3F_MFMA) {
      r.NB = std::max(1, (maxG + 63) / 64);
      r.lds[0] = sizeof(float) * ((size_t)4 * K3_CHUNK * 2 * KQ + (post ? 6 : 5) * K3_CHUNK);   // 4 planes [64][KH] + reductions (+ the entries' weights)
      // slices per pdf: every block ends with one fp64 atomic per accumulator cell (G*(2D+1) of them), so use as few blocks as still fill the chip (~4096 = 256 CUs x 8 blocks x 2 rounds)
      // (a class of a few pdfs -- the ones a split has grown -- is cut finer: one block walking a whole bucket is a latency of its own)
      r.ny = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(32, avg_chunks), (4096 + n_cls - 1) / std::max(1, n_cls)));
      if (ny_opt > 0) r.ny = ny_opt;
      // Both phases on the fp16 matrix cores (k3_accumulate_block16) under the conditions of the wave form's fp16 phases: <= 128
      // Gaussians at D <= 80, <= 192 at D <= 40.  KHG_K3_PHASEA=f32 or KHG_K3_PHASEB=f64 keep the fp32 / fp64 MFMA form.
      r.may_f16a = r.may_f16b = !post && pha == 0 && phb == 2 && ((KQ == 20 && maxG <= 128) || (KQ == 10 && maxG <= 192));
      // (one Gaussian block per wave: < 256 registers, so a block of eight waves runs two per SIMD; four blocks per wave -- 193..256
      //  Gaussians -- spill at 512 registers: the fp32 / fp64 form keeps them)
      r.NB16 = maxG <= 128 ? 1 : 3; r.nwv16 = maxG > 64 && maxG <= 128 ? 8 : 4;
      // split planes of a chunk in both layouts + the softmax's exchange: [2][64][KPAD + 8] + [2][2 XP][72] halves, 5 x 64 floats
      // ... or, before the chunk loop, the pdf's parameter rows [2][lanes' Gaussians][D | 1] + the columns' exponents
      const size_t kpad = ((size_t)8 * KQ + 31) / 32 * 32, gp_b16 = maxG <= 64 ? 64 : (maxG <= 128 ? 128 : 192);
      r.lds[2] = std::max<size_t>(2 * (2 * (size_t)K3_CHUNK * (kpad + 8) + 2 * (size_t)8 * KQ * (K3_CHUNK + 8)) + sizeof(float) * 9 * K3_CHUNK,
                                  sizeof(float) * (2 * gp_b16 * (size_t)(m->D | 1) + 8 * (size_t)KQ));
    } else {
      r.lds[0] = k3_valu_lds(m, maxG, post); r.too_wide = r.lds[0] > K3_VALU_LDS_MAX;
      r.ny = (int)std::max<int64_t>(1, std::min<int64_t>(64, (avg_chunks + 3) / 4));
    }
    if (one_block) r.ny = 1;
    items(r);
    return r;
  };
  // Form per pdf: the wave form takes every pdf of <= 64 Gaussians (D <= 40); what is left -- a few pdfs a split grew, or a model
  // of wide pdfs throughout -- goes to the chunk-per-block MFMA form (<= 256 Gaussians at D <= 40, <= 128 at D <= 80) or the VALU form.
  int maxG = 0, maxG_lo = 0, n_hi = 0;
  for (int p = 0; p < P; ++p) {
    const int Gp = m->gauss_off[(size_t)p + 1] - m->gauss_off[(size_t)p];
    maxG = std::max(maxG, Gp);
    if (Gp <= 64) maxG_lo = std::max(maxG_lo, Gp); else ++n_hi;
  }
  const bool mfma_ok = (maxG <= 128 || (maxG <= 256 && KQ == 10)) && k3form != 2 && KQ != 0;
  const bool wave_ok = !post && KQ == 10 && k3form == 0 && maxG_lo > 0;       // (the wave forms' fp16 phase B rests on ONE |weight|: 7h)
  const int rest = mfma_ok ? K3F_MFMA : K3F_VALU;
  K3Plan pl;
  if (wave_ok && n_hi == 0) pl.run[pl.nruns++] = wave(0, INT_MAX, maxG);
  else if (wave_ok) {
    pl.run[pl.nruns++] = wave(0, 64, maxG_lo);
    pl.run[pl.nruns++] = block(rest, 64, INT_MAX, maxG, n_hi, true);
  } else pl.run[pl.nruns++] = block(rest, 0, INT_MAX, maxG, P, false);
  return pl;
}

// The one refusal khg_acc_stats_post raises behind its argument checks, for khg_acc_mllt_stats_post to raise among its own: the
// posterior pass sends a model to the chunk-per-block MFMA form or, past that form's sizes, to the VALU form, whose LDS bounds the pdf.
int k3_post_check(khg_ctx* ctx, const khg_model* m, const std::string& who) {
  const K3Run r = k3_plan(ctx, m, true, 0, false).run[0];     // (from posteriors: one run)
  if (r.too_wide) return khg_set_error(KHG_E_UNSUPPORTED, who + "a pdf of " + std::to_string(r.maxG) + " Gaussians is too large for the LDS chunk buffers of the statistics pass");
  return KHG_OK;
}

// Every instantiation of the accumulate kernels, once: (variant, KQ, Gaussian blocks, waves, POST, fp16 phase A) -> the kernel.
// (the fp16 phases of the wave form exist for three and four Gaussian blocks only: k3_plan allows them for nb >= 3, so there is no
//  row -- and no code object -- for one or two blocks; khg_k3_forms hands the table to a test)
typedef void (*K3Kernel)(K3Args);
enum K3Variant { K3V_WAVE = KHG_K3V_WAVE, K3V_WAVE16 = KHG_K3V_WAVE16, K3V_WAVE16P = KHG_K3V_WAVE16P, K3V_FINALIZE = KHG_K3V_FINALIZE,
                 K3V_MFMA = KHG_K3V_MFMA, K3V_BLOCK16 = KHG_K3V_BLOCK16, K3V_VALU = KHG_K3V_VALU };
struct K3Inst { int variant, KQ, NB, nwv; bool post, f16a; K3Kernel fn; };
#define K3_WAVE_ROWS(NB) {K3V_WAVE, 10, NB, 4, false, false, k3_accumulate_wave<NB>}, {K3V_FINALIZE, 10, NB, 4, false, false, k3_wave_finalize<NB>}
#define K3_WAVE_F16_ROWS(NB)                                                                                                        \
  {K3V_WAVE, 10, NB, 4, false, true, k3_accumulate_wave<NB, true>}, {K3V_WAVE16, 10, NB, 4, false, true, k3_accumulate_wave16<NB>}, \
  {K3V_WAVE16P, 10, NB, 4, false, true, k3_accumulate_wave16<NB, true>}
#define K3_MFMA_ROWS(KQ, NBW) {K3V_MFMA, KQ, NBW, 4, false, false, k3_accumulate_mfma<KQ, NBW>}, {K3V_MFMA, KQ, NBW, 4, true, false, k3_accumulate_mfma<KQ, NBW, true>}
#define K3_VALU_ROWS(KQ) {K3V_VALU, KQ, 0, 4, false, false, k3_accumulate<KQ>}, {K3V_VALU, KQ, 0, 4, true, false, k3_accumulate<KQ, true>}
static const K3Inst k3_insts[] = {
  K3_WAVE_ROWS(1), K3_WAVE_ROWS(2), K3_WAVE_ROWS(3), K3_WAVE_ROWS(4), K3_WAVE_F16_ROWS(3), K3_WAVE_F16_ROWS(4),
  K3_MFMA_ROWS(10, 1), K3_MFMA_ROWS(10, 2), K3_MFMA_ROWS(10, 3), K3_MFMA_ROWS(10, 4), K3_MFMA_ROWS(20, 1), K3_MFMA_ROWS(20, 2),
  {K3V_BLOCK16, 20, 1, 4, false, true, k3_accumulate_block16<20, 1, 4>}, {K3V_BLOCK16, 10, 1, 4, false, true, k3_accumulate_block16<10, 1, 4>},
  {K3V_BLOCK16, 20, 1, 8, false, true, k3_accumulate_block16<20, 1, 8>}, {K3V_BLOCK16, 10, 1, 8, false, true, k3_accumulate_block16<10, 1, 8>},
  {K3V_BLOCK16, 10, 3, 4, false, true, k3_accumulate_block16<10, 3, 4>},
  K3_VALU_ROWS(10), K3_VALU_ROWS(20), K3_VALU_ROWS(0),
};
static K3Kernel k3_kernel(int variant, int KQ, int NB, int nwv, bool post, bool f16a) {
  for (const K3Inst& i : k3_insts)
    if (i.variant == variant && i.KQ == KQ && i.NB == NB && i.nwv == nwv && i.post == post && i.f16a == f16a) return i.fn;
  return nullptr;
}
extern "C" int khg_k3_forms(int32_t* rows, int32_t cap, int32_t* n) {
  const int32_t cnt = (int32_t)(sizeof(k3_insts) / sizeof(k3_insts[0]));
  if (!n || (rows && cap < cnt)) return khg_set_error(KHG_E_ARG, "khg_k3_forms: bad arguments");
  *n = cnt;
  if (!rows) return KHG_OK;
  for (int32_t i = 0; i < cnt; ++i) {
    const K3Inst& k = k3_insts[i];
    int32_t* o = rows + 6 * (size_t)i;
    o[0] = k.variant; o[1] = k.KQ; o[2] = k.NB; o[3] = k.nwv; o[4] = k.post; o[5] = k.f16a;
  }
  return KHG_OK;
}
extern "C" int khg_utts_k3_last(const khg_utts* u, int32_t out[2][12], int32_t* nruns) {
  if (!u || !out || !nruns) return khg_set_error(KHG_E_ARG, "khg_utts_k3_last: bad arguments");
  *nruns = u->k3_last_n;
  for (int i = 0; i < u->k3_last_n; ++i) std::copy(u->k3_last[i], u->k3_last[i] + 12, out[i]);
  return KHG_OK;
}
// ... and the one launch of them
static int k3_launch(khg_ctx* ctx, K3Kernel fn, unsigned grid, int nthr, size_t lds, const K3Args& a) {
  int rc = khg_lds_attribute((const void*)fn, lds);
  if (rc) return rc;
  KHG_LAUNCH(ctx, fn, dim3(grid), dim3(nthr), lds, ctx->stream, a);
  return KHG_OK;
}

// K3, optionally with C1 pipelined behind it: the pdfs are cut into `nparts` ranges; launch(p0, np) enqueues the accumulate kernels of
// one range on the context's stream, and they run while the all-reduce of the previous range's accumulator rows runs on the context's
// communication stream.  The sequence of collectives is a function of (P, nparts) only, whatever `launch` does.
template <class Launch>
static int k3_for_ranges(khg_ctx* ctx, const khg_model* m, khg_accs* acc, void* comm, int nparts, Launch&& launch) {
  const int n = comm ? nparts : 1;
  for (int part = 0; part < n; ++part) {
    const int p0 = (int)((int64_t)m->P * part / n), np = (int)((int64_t)m->P * (part + 1) / n) - p0;
    int rc = launch(p0, np);
    if (!rc && comm && n > 1) rc = accs_allreduce_pieces(ctx, acc, m, p0, np, comm, nullptr);
    if (rc) return rc;
  }
  return KHG_OK;
}

static K3Args k3_args(khg_ctx* ctx, const khg_model* m, const khg_tm* tm, const khg_utts* u, khg_accs* acc, float weight, bool post, int64_t Neff) {
  K3Args a;
  a.feats = u->feats_d; a.ali = post ? u->pe_tid_d : u->ali_d; a.id2pdf = tm->id2pdf_d; a.num_tids = tm->num_tids;
  a.N = Neff; a.P = m->P; a.D = m->D;
  a.gauss_off = m->gauss_off_d; a.gconsts = m->gconsts_d; a.means_invvars = m->miv_d; a.inv_vars = m->iv_d; a.nhalf_inv_vars = m->nhiv_d;
  a.pdf_count = u->pdf_count_d; a.pdf_start = post ? u->pe_start_d : u->pdf_start_d; a.pdf_cursor = u->pdf_cursor_d;
  a.frame_ids = post ? u->pe_ids_d : u->frame_ids_d; a.tid_count = u->tid_count_d;
  a.e_row = post ? u->pe_row_d : nullptr; a.e_w = post ? u->pe_w_d : nullptr;
  a.occ = acc->occ(); a.mean_acc = acc->mean(); a.var_acc = acc->var(); a.trans_acc = acc->trans(); a.scalars = acc->scalars();
  a.weight = weight; a.err_flag = ctx->err_flag_d; a.part = nullptr; a.ll_part = nullptr; a.pdf0 = 0; a.npdf = m->P; a.items = nullptr; a.item_off = nullptr;
  a.pa_ex = nullptr; a.pa_S = 0; a.pa_scale = 1.0f; a.pa_inv = 1.0f; a.pa_c1 = 1.44269504088896340736f; a.pb_gscale = 1.0f; a.pb_SG = 0;   // (k3_set_scales)
  a.xrec = nullptr; a.xrec_zero = 0;         // (k3_planes)
  return a;
}
// the fp16 phases' scales: the model's for phase A (k3_phase_a_scales said they hold), the weight's for phase B
static bool k3_weight_ordinary(float weight) { return std::isfinite(weight) && std::fabs(weight) > 1.0e-30f && std::fabs(weight) < 1.0e30f; }
static void k3_set_scales(K3Args& a, const khg_model* m, bool f16a, bool f16b) {
  if (f16a) {
    a.pa_ex = m->k3_ex_d; a.pa_S = m->k3_S;
    a.pa_scale = std::ldexp(1.0f, m->k3_S); a.pa_inv = std::ldexp(1.0f, -m->k3_S); a.pa_c1 = std::ldexp(1.44269504088896340736f, -m->k3_S);
  }
  if (f16b) { a.pb_SG = 13 - std::ilogb(std::fabs(a.weight)); a.pb_gscale = std::ldexp(1.0f, a.pb_SG); }
}

// The set's split feature records for k3_accumulate_wave16 (KHG_OPT_K3_PLANES): N + 1 records of 320 B, the pieces phase A stages --
// x' = x 2^ex, fl(x^2) 2^ex2, each as two fp16 pieces -- made ONCE per (set, exponents) instead of in every pass over every frame: the
// features of a set do not change from EM iteration to EM iteration, and the exponents (m->k3_ex, from the model's envelope alone)
// move only when a dimension's envelope crosses a power of two.  Built when absent or keyed by other exponents; dropped by
// khg_utts_features_changed.  auto: only where the records fit half of the free device memory at that moment; a set from the context's
// arena (one call each) never.  *use = false -- the pass splits in its loop, same bits -- whenever there are no records.
static int k3_planes(khg_ctx* ctx, const khg_model* m, khg_utts* u, bool* use) {
  *use = false;
  const int mode = ctx->opt[KHG_OPT_K3_PLANES];
  if (mode == 1 || u->N >= (int64_t)INT_MAX - 1 || (mode == 0 && u->small)) return KHG_OK;
  const size_t bytes = sizeof(_Float16) * K3_XREC * ((size_t)u->N + 1);
  if (u->k3x_d && u->k3x_key == m->k3_ex) { *use = true; return KHG_OK; }
  if (!u->k3x_d) {
    if (mode == 0) {
      size_t free_b = 0, total_b = 0;
      if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return KHG_OK; }
      if (bytes > free_b / 2) return KHG_OK;
    }
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); return KHG_OK; }     // no room: not an error
    u->k3x_d = p; u->k3x_bytes = (int64_t)bytes;
  }
  {
    KernelTimer kt(ctx, "k3_pack_x");
    const int64_t nthr = ((int64_t)u->N + 1) * 5;
    KHG_LAUNCH(ctx, k3_pack_x, dim3((unsigned)std::min<int64_t>(65536, (nthr + 255) / 256)), dim3(256), 0, ctx->stream, u->feats_d, u->N, (int)u->D, m->k3_ex_d,
               reinterpret_cast<_Float16*>(u->k3x_d));
  }
  HIPCHK(hipGetLastError());
  u->k3x_key = m->k3_ex; ++u->k3x_packs;
  *use = true;
  return KHG_OK;
}
extern "C" int khg_utts_k3_planes(const khg_utts* u, int64_t* bytes, int64_t* packs, int32_t* used) {
  if (!u || !bytes || !packs || !used) return khg_set_error(KHG_E_ARG, "khg_utts_k3_planes: bad arguments");
  *bytes = u->k3x_d ? u->k3x_bytes : 0; *packs = u->k3x_packs; *used = u->k3x_used ? 1 : 0;
  return KHG_OK;
}

// Frames (entries) -> buckets by pdf, one of three ways; the transition statistics on the way
template int u_alloc<uint32_t>(khg_utts*, uint32_t**, size_t);     // (one copy out of line for the sort's buffers, as it always was: the library's dynamic symbols stay what they were)
static int k3_bucket(khg_ctx* ctx, const khg_model* m, const khg_tm* tm, khg_utts* u, const K3Args& a, bool post, int64_t nsub, int64_t Neff) {
  int rc = KHG_OK;
  // the sort's buffers: K3's own, cached on the set for its N frames, or the posteriors' (sized by the caller for the entries)
  uint32_t *&sort_keys = post ? u->pe_keys_d : u->sort_keys_d, *&sort_keys_out = post ? u->pe_keys_out_d : u->sort_keys_out_d;
  uint32_t*& sort_vals = post ? u->pe_vals_d : u->sort_vals_d;
  void*& sort_tmp = post ? u->pe_tmp_d : u->sort_tmp_d;
  size_t& sort_tmp_bytes = post ? u->pe_tmp_bytes : u->sort_tmp_bytes;
  const int gb = (int)std::min<int64_t>(4096, (Neff + 255) / 256);
  {
    KernelTimer kt(ctx, nsub < 0 ? "k3_bucket" : "k3_bucket_pass2");
    // KHG_OPT_K3_BUCKET = 1: cursor-bump scatter (bucket order depends on the atomics)
    if (!post && nsub < 0 && (ctx->opt[KHG_OPT_K3_BUCKET] == 1 || u->N >= (int64_t)INT_MAX)) {
      KHG_LAUNCH(ctx, k3_count, dim3(gb), dim3(256), 0, ctx->stream, a);
      KHG_LAUNCH(ctx, k3_scan, dim3(1), dim3(1024), 0, ctx->stream, a);
      KHG_LAUNCH(ctx, k3_scatter, dim3(gb), dim3(256), 0, ctx->stream, a);
    } else if (!post && nsub < 0 && ctx->opt[KHG_OPT_K3_BUCKET] == 2 && m->P <= K3_CS_MAXP) {
      // the library's own stable counting sort (khg_k3_accstats.hip.inc: k3_cs_*; opt-in: 1.27 ms against the radix sort's 0.80 at the
      // bench size): blocks of CB consecutive frames
      const int nw = m->P + 1 <= 7168 ? 4 : 2;                      // waves of a placing block: nw x (P + 1 + 1024) counters of LDS
      int64_t CB = 32768;
      while (CB > 64 * nw * 4 && (u->N + CB - 1) / CB < 1024) CB /= 2;   // enough blocks to fill the chip on small sets
      const int nblk = (int)((u->N + CB - 1) / CB);
      const size_t hist_n = (size_t)nblk * ((size_t)m->P + 1);
      if (u->cs_hist_n < hist_n) { DEVFREE(u->cs_hist_d); rc = u_alloc(u, &u->cs_hist_d, hist_n); if (rc) return rc; u->cs_hist_n = hist_n; }
      if (u->cs_tot_n < (size_t)m->P + 1) { DEVFREE(u->cs_tot_d); rc = u_alloc(u, &u->cs_tot_d, (size_t)m->P + 1); if (rc) return rc; u->cs_tot_n = (size_t)m->P + 1; }
      K3CsArgs c{u->cs_hist_d, u->cs_tot_d, (int32_t)CB, nblk};
      const bool ldst = tm->num_tids <= K3_LDS_TIDS;
      const size_t lds_h = sizeof(unsigned int) * ((size_t)m->P + 1 + (ldst ? (size_t)tm->num_tids + 1 : 0));
      const size_t lds_p = sizeof(unsigned int) * (size_t)nw * ((size_t)m->P + 1 + 1024);     // per-wave counters + the run-head hash tags
      if ((rc = khg_lds_attribute((const void*)k3_cs_hist<true>, lds_h)) || (rc = khg_lds_attribute((const void*)k3_cs_hist<false>, lds_h)) ||
          (rc = khg_lds_attribute((const void*)k3_cs_place, lds_p))) return rc;
      if (ldst) KHG_LAUNCH(ctx, k3_cs_hist<true>, dim3(nblk), dim3(256), lds_h, ctx->stream, a, c);
      else KHG_LAUNCH(ctx, k3_cs_hist<false>, dim3(nblk), dim3(256), lds_h, ctx->stream, a, c);
      KHG_LAUNCH(ctx, k3_cs_scan, dim3((m->P + 256) / 256), dim3(256), 0, ctx->stream, a, c);
      KHG_LAUNCH(ctx, k3_cs_starts, dim3(1), dim3(1024), 0, ctx->stream, a, c);
      KHG_LAUNCH(ctx, k3_cs_place, dim3(nblk), dim3(64 * nw), lds_p, ctx->stream, a, c);
    } else {
      // stable sort of (pdf, frame) pairs: frames of a pdf stay in frame order; the bucket boundaries are read
      // off the sorted keys
      int bits = 1;
      while ((1 << bits) <= m->P) ++bits;            // keys are 0..P
      if (!sort_keys) {
        rc = u_alloc(u, &sort_keys, (size_t)u->N);
        if (!rc) rc = u_alloc(u, &sort_keys_out, (size_t)u->N);
        if (!rc) rc = u_alloc(u, &sort_vals, (size_t)u->N);
        if (rc) return rc;
      }
      size_t need = 0;
      HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, need, sort_keys, sort_keys_out, sort_vals,
                                                reinterpret_cast<uint32_t*>(a.frame_ids), (int)Neff, 0, bits, ctx->stream));
      if (need > sort_tmp_bytes) {
        DEVFREE(sort_tmp);
        { int rt = u_alloc(u, reinterpret_cast<char**>(&sort_tmp), need); if (rt) return rt; }
        sort_tmp_bytes = need;
      }
      if (post) {
        // the (pdf, entry) pairs and the weighted transition statistics (khg_k3_post.hip.inc)
        const bool ldst = tm->num_tids <= K3_LDS_TIDS;
        if (ldst) KHG_LAUNCH(ctx, k3_post_keys<true>, dim3(std::min(gb, 1024)), dim3(256), sizeof(double) * ((size_t)tm->num_tids + 1), ctx->stream, a, sort_keys, sort_vals);
        else KHG_LAUNCH(ctx, k3_post_keys<false>, dim3(std::min(gb, 1024)), dim3(256), 0, ctx->stream, a, sort_keys, sort_vals);
      } else if (nsub >= 0) {
        // the (pdf, frame) pairs of the flagged utterances only, utterances in order: positions from an exclusive sum of their lengths
        if (!u->sub_off_d) { rc = u_alloc(u, &u->sub_off_d, (size_t)u->n_utt + 1); if (rc) return rc; }
        KHG_LAUNCH(ctx, k3_sub_scan, dim3(1), dim3(1024), 0, ctx->stream, u->unc_d, u->frame_off_d, u->n_utt, u->sub_off_d);
        KHG_LAUNCH(ctx, k3_sub_keys, dim3((unsigned)std::min(u->n_utt, 8192)), dim3(64), 0, ctx->stream, a, u->unc_d, u->frame_off_d, u->sub_off_d, u->n_utt, sort_keys, sort_vals);
      } else if (tm->num_tids <= K3_LDS_TIDS) KHG_LAUNCH(ctx, k3_sort_keys<true>, dim3(std::min(gb, 1024)), dim3(256), 0, ctx->stream, a, sort_keys, sort_vals);
      else KHG_LAUNCH(ctx, k3_sort_keys<false>, dim3(std::min(gb, 1024)), dim3(256), 0, ctx->stream, a, sort_keys, sort_vals);
      HIPCHK(hipcub::DeviceRadixSort::SortPairs(sort_tmp, need, sort_keys, sort_keys_out, sort_vals,
                                                reinterpret_cast<uint32_t*>(a.frame_ids), (int)Neff, 0, bits, ctx->stream));
      if (post) {
        K3Args b = a;
        b.num_tids = -1;        // k3_bounds has no integer counts to fold: k3_post_keys added the weighted ones itself
        KHG_LAUNCH(ctx, k3_bounds, dim3((m->P + 256) / 256), dim3(256), 0, ctx->stream, b, sort_keys_out);
      } else KHG_LAUNCH(ctx, k3_bounds, dim3((m->P + 256) / 256), dim3(256), 0, ctx->stream, a, sort_keys_out);
    }
  }
  return KHG_OK;
}
// Work items of one run (k3_make_items) into the set's buffers, grown to the plan's bounds; two classes keep their item lists side by
// side in the same buffers (r.second: the upper halves).  -> *items, *item_off: the run's lists
static int k3_make_work_items(khg_ctx* ctx, const khg_model* m, khg_utts* u, const K3Args& a, const K3Run& r, K3Item** items, int32_t** item_off) {
  if (r.max_items >= INT_MAX / 2) return khg_set_error(KHG_E_UNSUPPORTED, "khg_acc_stats: too many work items");
  const size_t n_items = (size_t)r.max_items, n_off = (size_t)m->P + 1, n_part = r.parked ? (size_t)r.max_slots * r.nsum1 : 0;
  int rc = KHG_OK;
  if (u->k3_items_n < n_items) { DEVFREE(u->k3_items_d); rc = u_alloc(u, reinterpret_cast<K3Item**>(&u->k3_items_d), 2 * n_items); if (rc) return rc; u->k3_items_n = n_items; }
  if (u->k3_item_off_n < n_off) { DEVFREE(u->k3_item_off_d); rc = u_alloc(u, &u->k3_item_off_d, 2 * n_off); if (rc) return rc; u->k3_item_off_n = n_off; }
  if (u->k3_part_n < n_part) { DEVFREE(u->k3_part_d); rc = u_alloc(u, &u->k3_part_d, n_part); if (rc) return rc; u->k3_part_n = n_part; }
  *items = reinterpret_cast<K3Item*>(u->k3_items_d) + (r.second ? u->k3_items_n : 0);
  *item_off = u->k3_item_off_d + (r.second ? u->k3_item_off_n : 0);
  KHG_LAUNCH(ctx, k3_make_items, dim3(1), dim3(1024), 0, ctx->stream, a, r.ny, r.target, (int)r.max_items, (int)std::min<int64_t>(r.max_slots, INT_MAX),
             *items, *item_off, r.cls_lo, r.cls_hi);
  return KHG_OK;
}
// One run of the plan: the fp16 phases settled, its work items, its kernels range by range.  `a` carries on from run to run.
static int k3_run(khg_ctx* ctx, const khg_model* m, khg_utts* u, khg_accs* acc, K3Args& a, const K3Run& r, bool post, const char* timer, void* comm, int nparts) {
  if (r.too_wide) return khg_set_error(KHG_E_UNSUPPORTED, "khg_acc_stats: pdf too large for the LDS chunk buffers");
  const bool wave = r.form == K3F_WAVE;
  // (the MFMA form has both phases on the fp16 matrix cores or neither, so the weight is asked first; the wave form keeps phase A alone)
  const bool wt = k3_weight_ordinary(a.weight);
  bool f16a = false;
  if (r.may_f16a && (wave || wt)) { int rs = k3_phase_a_scales(ctx, const_cast<khg_model*>(m), u, &f16a); if (rs) return rs; }
  const bool f16b = f16a && r.may_f16b && wt;
  k3_set_scales(a, m, f16a, f16b);
  int variant = wave ? (f16b ? K3V_WAVE16 : K3V_WAVE) : r.form == K3F_VALU ? K3V_VALU : f16b ? K3V_BLOCK16 : K3V_MFMA;
  if (variant == K3V_WAVE16 && r.may_planes) {
    bool planes = false;
    { int rp = k3_planes(ctx, m, u, &planes); if (rp) return rp; }
    if (planes) { variant = K3V_WAVE16P; a.xrec = reinterpret_cast<const _Float16*>(u->k3x_d); a.xrec_zero = (int32_t)u->N; u->k3x_used = true; }
  }
  const int nwv = variant == K3V_BLOCK16 ? r.nwv16 : 4;     // the block size
  const K3Kernel fn = k3_kernel(variant, m->KQ, variant == K3V_BLOCK16 ? r.NB16 : r.NB, nwv, post, f16a);
  const K3Kernel fin = wave ? k3_kernel(K3V_FINALIZE, m->KQ, r.NB, 4, false, false) : nullptr;
  if (!fn || (wave && !fin)) return khg_set_error(KHG_E_RUNTIME, "khg_acc_stats: no kernel for the planned form");
  const size_t lds = r.lds[f16b ? 2 : f16a ? 1 : 0];
  if (u->k3_last_n < 2) {                       // khg_utts_k3_last: what this run launches, as settled above
    int32_t* o = u->k3_last[u->k3_last_n++];
    o[0] = variant; o[1] = m->KQ; o[2] = variant == K3V_BLOCK16 ? r.NB16 : r.NB; o[3] = nwv; o[4] = post; o[5] = f16a; o[6] = f16b;
    o[7] = variant == K3V_WAVE16P; o[8] = r.ny; o[9] = r.cls_lo; o[10] = r.cls_hi; o[11] = (int32_t)lds;
  }
  int rc = KHG_OK;
  if (wave && u->k3_llpart_n < (size_t)m->P) { DEVFREE(u->k3_llpart_d); rc = u_alloc(u, &u->k3_llpart_d, (size_t)m->P); if (rc) return rc; u->k3_llpart_n = (size_t)m->P; }
  K3Item* items = nullptr; int32_t* item_off = nullptr;
  rc = k3_make_work_items(ctx, m, u, a, r, &items, &item_off); if (rc) return rc;
  a.items = items; a.item_off = item_off;
  if (wave) {
    HIPCHK(hipMemsetAsync(u->k3_llpart_d, 0, sizeof(double) * (size_t)m->P, ctx->stream));
    a.ll_part = u->k3_llpart_d; a.part = u->k3_part_d;
  }
  rc = k3_for_ranges(ctx, m, acc, comm, nparts, [&](int p0, int np) -> int {
    a.pdf0 = p0; a.npdf = np;
    const unsigned nblk = (unsigned)((int64_t)std::min(np, r.n_cls) * r.ny + r.extra_blocks);
    KernelTimer kt(ctx, timer);
    int rl = k3_launch(ctx, fn, nblk, 64 * nwv, lds, a);
    if (!rl && wave) rl = k3_launch(ctx, fin, (unsigned)np, 256, 0, a);
    return rl;
  });
  if (rc) return rc;
  a.pdf0 = 0; a.npdf = m->P;
  if (wave) KHG_LAUNCH(ctx, k3_wave_scalars, dim3(1), dim3(1024), 0, ctx->stream, a, r.cls_lo, r.cls_hi);
  return KHG_OK;
}
// One pass of K3 over the set's resident alignment: all N frames (nsub < 0), or -- the second pass of the split mode -- the nsub frames
// of the utterances the DP left to the order-faithful decoders (flagged in u->unc_d; their alignments are merged into ali_d by now).
// npost >= 0 (khg_acc_stats_post): the pass runs over the npost flattened entries in u->pe_* instead of the alignment -- its own
// sort buffers and bucket bounds, the POST instantiations of the fp32-chain forms (`weight` is unused: every entry carries its own);
// one_block: ONE work item per pdf whatever its bucket holds (khg_acc_mllt_stats_post).
static int acc_stats_pass(khg_ctx* ctx, const khg_model* m, const khg_tm* tm, khg_utts* u, float weight, khg_accs* acc, void* comm, int nparts, int64_t nsub,
                          int64_t npost = -1, bool one_block = false) {
  int rc = KHG_OK;
  const bool post = npost >= 0;
  const int64_t Neff = post ? npost : nsub < 0 ? u->N : nsub;
  if (!post) {
    HIPCHK(hipMemsetAsync(u->pdf_count_d, 0, sizeof(int32_t) * (size_t)m->P, ctx->stream));
    HIPCHK(hipMemsetAsync(u->tid_count_d, 0, sizeof(unsigned long long) * ((size_t)tm->num_tids + 1), ctx->stream));
  }
  K3Args a = k3_args(ctx, m, tm, u, acc, weight, post, Neff);
  if (!post) u->k3x_used = false;              // (khg_utts_k3_planes: whether THIS pass read the split feature records)
  u->k3_last_n = 0;                            // (khg_utts_k3_last: the runs of THIS pass; none over zero frames)
  nparts = std::max(1, std::min(nparts, m->P));
  if (comm && nparts > 1) { rc = ctx_comm_stream(ctx); if (rc) return rc; }
  if (Neff > 0) {
    rc = k3_bucket(ctx, m, tm, u, a, post, nsub, Neff); if (rc) return rc;
    const K3Plan pl = k3_plan(ctx, m, post, Neff, one_block);
    // (a mixed call with an exchange: the first class runs without it, the pieces follow the second class's kernels)
    for (int i = 0; i < pl.nruns && !rc; ++i)
      rc = k3_run(ctx, m, u, acc, a, pl.run[i], post, nsub < 0 ? "k3_accumulate" : "k3_accumulate_pass2", i + 1 == pl.nruns ? comm : nullptr, nparts);
    if (rc) return rc;
    HIPCHK(hipGetLastError());
  } else {
    // a rank without frames launches nothing but takes part in the same collectives, in the same order, as every other rank
    rc = k3_for_ranges(ctx, m, acc, nparts > 1 ? comm : nullptr, nparts, [](int, int) { return (int)KHG_OK; }); if (rc) return rc;
  }
  if (comm) {
    // the rest of the block: all of it when nothing was pipelined, else the transition counts and the scalars; then the kernels'
    // stream waits for the communication stream
    if (nparts > 1) rc = accs_allreduce_pieces(ctx, acc, m, -1, 0, comm, nullptr);
    else rc = khg_accs_allreduce(ctx, acc, comm);
    if (rc) return rc;
  }
  return KHG_OK;   // asynchronous: kernel-side errors surface at khg_ctx_sync / khg_accs_download
}
static int acc_stats_impl(khg_ctx* ctx, const khg_model* m, const khg_tm* tm, khg_utts* u, float weight, khg_accs* acc, void* comm, int nparts) {
  if (ctx_dead(ctx) || !m || !tm || !u || !acc) return khg_set_error(KHG_E_ARG, "khg_acc_stats: bad arguments");
  { int rf = utts_foreign_ctx(ctx, u, "khg_acc_stats"); if (rf) return rf; }
  if (!u->ali_valid) return khg_set_error(KHG_E_ARG, "khg_acc_stats: no resident alignment (khg_align or khg_ali_upload first)");
  if (m->D != u->D || acc->D != m->D || acc->sumG != m->sumG || acc->num_tids != tm->num_tids)
    return khg_set_error(KHG_E_RUNTIME, "khg_acc_stats: accumulator / model / feature dimensions do not match");
  if (tm->max_pdf >= m->P) return khg_set_error(KHG_E_RUNTIME, "khg_acc_stats: transition model refers to pdf-ids the model does not have");
  // Split mode (khg_k2.hip): the order-faithful decoders may still be running on their side stream, writing to their own buffer.  The DP
  // kernel counted what it left to them: wait for IT (the host joins the stream once, right behind K2), and if there is anything,
  // accumulate the certified utterances now -- their ranges of ali_d are final, the others' are zero -- and the rest in a second pass
  // once the decoders are done.  Statistics are additive (csrc/mle-am-diag-gmm.cc:41-52); the second pass is the same kernels over
  // the flagged utterances' frames.
  int64_t nsub = -1;
  if (u->ali_pending && u->ali_split && u->N > 0) {
    HIPCHK(hipEventSynchronize(u->ev_dp));
    if (u->unc_cnt_h[0] == 0) u->ali_split = false;         // nothing to merge, nothing to wait for but the (empty) side stream
    else nsub = u->unc_cnt_h[1];
  }
  int rc = nsub < 0 ? wait_ali(ctx, u) : KHG_OK;
  if (!rc) rc = arena_flush(ctx);
  if (rc) return rc;
  if (!u->frame_ids_d || u->k3_P != m->P || u->k3_tids != tm->num_tids) {
    DEVFREE(u->pdf_count_d); DEVFREE(u->pdf_cursor_d); DEVFREE(u->pdf_start_d); DEVFREE(u->tid_count_d); DEVFREE(u->frame_ids_d);
    rc = u_alloc(u, &u->pdf_count_d, (size_t)m->P);
    if (!rc) rc = u_alloc(u, &u->pdf_cursor_d, (size_t)m->P);
    if (!rc) rc = u_alloc(u, &u->pdf_start_d, (size_t)m->P + 1);
    if (!rc) rc = u_alloc(u, &u->tid_count_d, (size_t)tm->num_tids + 1);
    if (!rc) rc = u_alloc(u, &u->frame_ids_d, (size_t)u->N);
    if (rc) return rc;
    u->k3_P = m->P; u->k3_tids = tm->num_tids;
  }
  if (nsub < 0) return acc_stats_pass(ctx, m, tm, u, weight, acc, comm, nparts, -1);
  rc = acc_stats_pass(ctx, m, tm, u, weight, acc, nullptr, 1, -1);          // the exchange (if any) follows the second pass
  if (!rc) rc = wait_ali(ctx, u);                                             // decoders done -> their alignments merged into ali_d
  if (!rc) rc = acc_stats_pass(ctx, m, tm, u, weight, acc, comm, nparts, nsub);
  return rc;
}
extern "C" int khg_acc_stats(khg_ctx* ctx, const khg_model* m, const khg_tm* tm, khg_utts* u, float weight, khg_accs* acc) {
  return acc_stats_impl(ctx, m, tm, u, weight, acc, nullptr, 1);
}
extern "C" int khg_acc_stats_reduce(khg_ctx* ctx, const khg_model* m, const khg_tm* tm, khg_utts* u, float weight, khg_accs* acc, void* comm, int32_t nparts) {
  return acc_stats_impl(ctx, m, tm, u, weight, acc, comm, nparts <= 0 ? 4 : nparts);
}

// gmm-acc-stats and gmm-acc-stats2 (7k): every check on the host first, then flatten -> bucket -> accumulate on the
// context's stream -- once into `acc`, or (acc2 != nullptr) the positive entries into `acc` and the negated negative ones into `acc2`.
static int acc_stats_post_impl(const std::string& name, khg_ctx* ctx, const khg_model* m, const khg_tm* tm, khg_utts* u, const khg_posteriors* p, float scale,
                               khg_accs* acc, khg_accs* acc2, bool two, bool one_block = false) {
  const std::string who = name + ": ";
  if (ctx_dead(ctx) || !m || !tm || !u || !p || !acc || (two && !acc2)) return khg_set_error(KHG_E_ARG, who + "bad arguments");
  if (two && acc == acc2) return khg_set_error(KHG_E_ARG, who + "num_accs and den_accs are the same block");
  { int rf = utts_foreign_ctx(ctx, u, name.c_str()); if (rf) return rf; }
  PostInfo pi;
  posteriors_info(p, &pi);
  if (pi.ctx != ctx || m->ctx != ctx || tm->ctx != ctx || acc->ctx != ctx || u->ctx != ctx || (two && acc2->ctx != ctx))
    return khg_set_error(KHG_E_ARG, who + "a handle of another context");
  if (pi.U != u->n_utt)
    return khg_set_error(KHG_E_ARG, who + "the posteriors hold " + std::to_string(pi.U) + " utterances, the set " + std::to_string(u->n_utt));
  for (int i = 0; i < pi.U; ++i) {
    const int64_t tp = pi.frame_off[i + 1] - pi.frame_off[i], ts = u->frame_off[(size_t)i + 1] - u->frame_off[(size_t)i];
    if (tp != 0 && tp != ts)
      return khg_set_error(KHG_E_ARG, who + "utterance " + std::to_string(i) + " has " + std::to_string(tp) + " frames of posteriors and " + std::to_string(ts) + " frames of features");
  }
  if (m->D != u->D || acc->D != m->D || acc->sumG != m->sumG || acc->num_tids != tm->num_tids ||
      (two && (acc2->D != m->D || acc2->sumG != m->sumG || acc2->num_tids != tm->num_tids)))
    return khg_set_error(KHG_E_ARG, who + "accumulator / model / feature dimensions do not match");
  if (tm->max_pdf >= m->P) return khg_set_error(KHG_E_ARG, who + "transition model refers to pdf-ids the model does not have");
  if (!std::isfinite(scale)) return khg_set_error(KHG_E_ARG, who + "scale must be finite");
  if (pi.max_tid > tm->num_tids)
    return khg_set_error(KHG_E_ARG, who + "the posteriors hold transition-id " + std::to_string(pi.max_tid) + ", the transition model has " + std::to_string(tm->num_tids));
  const int64_t E = pi.entry_off[pi.U];
  if (E >= (int64_t)INT_MAX || u->N >= (int64_t)INT_MAX) return khg_set_error(KHG_E_UNSUPPORTED, who + "2^31 - 1 or more entries or frames");
  if (E == 0) { u->k3_last_n = 0; return KHG_OK; }
  int rc = arena_flush(ctx);
  if (rc) return rc;
  rc = utts_grow_pe(u, (size_t)E);
  if (rc) return rc;
  if (!u->pe_start_d || u->pe_P != m->P) {
    DEVFREE(u->pe_start_d);
    rc = u_alloc(u, &u->pe_start_d, (size_t)m->P + 1);
    if (rc) return rc;
    u->pe_P = m->P;
  }
  // (two blocks: the flattened entries are made twice, once per sign; the stream orders the second flatten behind the first pass)
  rc = posteriors_flatten(ctx, p, u->frame_off_d, (double)scale, tm->num_tids, u->pe_row_d, u->pe_tid_d, u->pe_w_d, two ? 1 : 0);
  if (!rc) rc = acc_stats_pass(ctx, m, tm, u, 1.0f, acc, nullptr, 1, -1, E, one_block);
  if (rc || !two) return rc;
  rc = posteriors_flatten(ctx, p, u->frame_off_d, (double)scale, tm->num_tids, u->pe_row_d, u->pe_tid_d, u->pe_w_d, -1);
  if (!rc) rc = acc_stats_pass(ctx, m, tm, u, 1.0f, acc2, nullptr, 1, -1, E, one_block);
  return rc;
}
extern "C" int khg_acc_stats_post(khg_ctx* ctx, const khg_model* m, const khg_tm* tm, khg_utts* u, const khg_posteriors* p, float scale, khg_accs* acc) {
  return acc_stats_post_impl("khg_acc_stats_post", ctx, m, tm, u, p, scale, acc, nullptr, false);
}
int k3_acc_stats_post_one_block(khg_ctx* ctx, const khg_model* m, const khg_tm* tm, khg_utts* u, const khg_posteriors* p, float scale, khg_accs* acc) {
  return acc_stats_post_impl("khg_acc_stats_post", ctx, m, tm, u, p, scale, acc, nullptr, false, true);
}
extern "C" int khg_acc_stats_post2(khg_ctx* ctx, const khg_model* m, const khg_tm* tm, khg_utts* u, const khg_posteriors* p, float scale, khg_accs* num_accs,
                                   khg_accs* den_accs) {
  return acc_stats_post_impl("khg_acc_stats_post2", ctx, m, tm, u, p, scale, num_accs, den_accs, true);
}
