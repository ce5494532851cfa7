// kaldi_hmm_gmm_amd/csrc/khg_k1.hip -- C-ABI (include/khg_hip.h): K1, the log-likelihoods (khg_loglikes / _reachable / _band): the
// kernel table (k1_insts) and its one launch, form selection, scale exponents and domain checks of the split forms (k1_plan),
// per-set plans (chunks, units, walks) and one run function per form.  gfx950 only.
#include "khg_internal.hpp"

#include "khg_k1_loglikes.hip.inc"
#include "khg_k1_pdfmajor.hip.inc"
#include "khg_k1_split_common.hip.inc"
#include "khg_k1_f16x2.hip.inc"
#include "khg_k1_wide.hip.inc"
#include "khg_k1_f16x2s.hip.inc"

// ------------------------------------------------------------------------------------------
// K1
// khg_utts_k1_last: the words of khg_utts::k1_last (include/khg_hip.h): k1_record writes the call's plan, the run functions add what
// only device-side planning settles (chunks, grid, slices per block count, what was packed), k1_band_repair the last one
enum { K1L_SET, K1L_FORM, K1L_ASKED, K1L_DECLINED, K1L_K, K1L_MODE, K1L_PACK, K1L_PERSISTENT, K1L_GRID, K1L_CHUNKS, K1L_PER, K1L_ORDER,
       K1L_TAIL_SHIFT, K1L_SHIFT_MODE, K1L_NF, K1L_ALIGNED, K1L_INTERLEAVE, K1L_NB_SLICES /* 8 words */, K1L_REPACKED = K1L_NB_SLICES + 8, K1L_REPAIRED };
static_assert(K1L_REPAIRED + 1 == KHG_K1_LAST_WORDS, "khg_utts_k1_last: the record's layout");
static int k1l_form(int form) {
  return form == KHG_K1_F16X2 ? KHG_K1L_F16X2 : form == KHG_K1_FP32_PDF ? KHG_K1L_PDF : form == KHG_K1_FP32_UTT ? KHG_K1L_UTT : KHG_K1L_F16X2S;
}
extern "C" int khg_utts_k1_last(const khg_utts* u, int32_t out[KHG_K1_LAST_WORDS]) {
  if (!u || !out) return khg_set_error(KHG_E_ARG, "khg_utts_k1_last: bad arguments");
  std::copy(u->k1_last, u->k1_last + KHG_K1_LAST_WORDS, out);
  return KHG_OK;
}

// Every instantiation of K1's kernels, once: (family, K = KQ or KS, the family's further template parameters) -> the kernel, its block
// size and, where the kernel fixes it, its dynamic LDS.  A family is one kernel signature's use; K1Sig names the signature, and a row
// whose kernel has another one does not compile.
#ifndef K1H_NT10
#define K1H_NT10 2      // 32-frame tiles per wave of the f16x2 form at D <= 80 (12 spilled registers; 1: none)
#endif
enum K1Family { K1_UTT /* NF, aligned */, K1_PDF /* Gaussian blocks */, K1_WIDE, K1_H /* NTMAX */, K1_S /* pdfs per tile */, K1_S_PERSISTENT, K1_S_REPAIR,
                K1_PACK_P, K1_PACK_H, K1_PACK_S, K1_IMG_H, K1_IMG_S };
template <int F> struct K1Sig;
#define K1_SIG(F, ...) template <> struct K1Sig<F> { typedef void (*Fn)(__VA_ARGS__); }
#define K1_X_TILES const float*, const int64_t*, const int64_t*, const int32_t*, int64_t, int                          /* the *_pack_x kernels' common head */
#define K1_W_ROWS const float*, const float*, const float*, const int32_t*, const int32_t*, const int32_t*, int        /* the *_pack_tiles kernels' */
K1_SIG(K1_UTT, K1Args); K1_SIG(K1_PDF, K1pArgs); K1_SIG(K1_WIDE, KwArgs); K1_SIG(K1_H, K1hArgs); K1_SIG(K1_S, K1sArgs);
K1_SIG(K1_S_PERSISTENT, K1sArgs, int, int*); K1_SIG(K1_S_REPAIR, K1sArgs, int);
K1_SIG(K1_PACK_P, K1_X_TILES, float*); K1_SIG(K1_PACK_H, K1_X_TILES, const int32_t*, k1b_u32x4*); K1_SIG(K1_PACK_S, K1_X_TILES, const int32_t*, k1b_u32x4*);
K1_SIG(K1_IMG_H, K1_W_ROWS, const int32_t*, char*); K1_SIG(K1_IMG_S, K1_W_ROWS, const int32_t*, float, char*);
static size_t k1h_lds_of(int KS) { return (size_t)k1h_lds_bytes(KS); }
static size_t k1s_lds_of(int KS) { return (size_t)k1s_nmax(KS) * k1s_xtile_bytes(KS) + K1S_CTL_BYTES; }      // + the control and stamp words
static size_t k1s_repair_lds_of(int KS) { return k1s_lds_of(KS) + 4 * 513; }                                    // + the list of flagged chunks
typedef void (*K1Any)();
struct K1Inst { int family, K, p1, p2, nthr; size_t (*lds)(int K); K1Any fn; };
#define K1_ROW(F, K, p1, p2, nthr, lds, ...) {F, K, p1, p2, nthr, lds, reinterpret_cast<K1Any>(static_cast<K1Sig<F>::Fn>(__VA_ARGS__))}
#define K1_UTT_ROWS(KQ, NF, WPS) K1_ROW(K1_UTT, KQ, NF, 1, 256, nullptr, k1_loglikes<KQ, NF, true, WPS>), K1_ROW(K1_UTT, KQ, NF, 0, 256, nullptr, k1_loglikes<KQ, NF, false, WPS>)
#define K1_PDF_ROW(KQ, NB, WPS) K1_ROW(K1_PDF, KQ, NB, 0, 256, nullptr, k1p_loglikes<KQ, NB, WPS>)
#define K1_PDF_ROWS(KQ, WPS) K1_PDF_ROW(KQ, 1, WPS), K1_PDF_ROW(KQ, 2, WPS), K1_PDF_ROW(KQ, 3, WPS), K1_PDF_ROW(KQ, 4, WPS), \
                             K1_PDF_ROW(KQ, 5, WPS), K1_PDF_ROW(KQ, 6, WPS), K1_PDF_ROW(KQ, 7, WPS), K1_PDF_ROW(KQ, 8, WPS)
#define K1_KS_ROWS(KS)                                                                                                           \
  K1_ROW(K1_S, KS, 1, 0, 512, k1s_lds_of, k1s_loglikes<KS>), K1_ROW(K1_S_PERSISTENT, KS, 0, 0, 512, k1s_lds_of, k1s_persistent<KS>),  \
  K1_ROW(K1_S_REPAIR, KS, 0, 0, 512, k1s_repair_lds_of, k1s_repair<KS>), K1_ROW(K1_PACK_H, KS, 0, 0, 256, nullptr, k1h_pack_x<KS>), \
  K1_ROW(K1_PACK_S, KS, 0, 0, 256, nullptr, k1s_pack_x<KS>), K1_ROW(K1_IMG_H, KS, 0, 0, 256, nullptr, k0h_pack_tiles<KS>),       \
  K1_ROW(K1_IMG_S, KS, 0, 0, 256, nullptr, k0s_pack_tiles<KS>)
static const K1Inst k1_insts[] = {
  K1_UTT_ROWS(10, 6, 2), K1_UTT_ROWS(10, 5, 2), K1_UTT_ROWS(20, 5, 1), K1_PDF_ROWS(10, 2), K1_PDF_ROWS(20, 1),
  K1_ROW(K1_WIDE, 0, 0, 0, 256, nullptr, k1w_loglikes),       // (its LDS goes with D)
  K1_ROW(K1_H, 5, 2, 0, 512, k1h_lds_of, k1h_loglikes<5, 2>), K1_ROW(K1_H, 10, K1H_NT10, 0, 512, k1h_lds_of, k1h_loglikes<10, K1H_NT10>),
  K1_KS_ROWS(5), K1_KS_ROWS(10), K1_ROW(K1_S, 5, 4, 0, 512, k1s_lds_of, k1s_loglikes_packed<5, 4>), K1_ROW(K1_S, 5, 2, 0, 512, k1s_lds_of, k1s_loglikes_packed<5, 2>),
  K1_ROW(K1_PACK_P, 10, 0, 0, 256, nullptr, k1p_pack_x<10>), K1_ROW(K1_PACK_P, 20, 0, 0, 256, nullptr, k1p_pack_x<20>),
};
template <int F> struct K1Kernel { typename K1Sig<F>::Fn fn; int nthr; size_t lds; };
template <int F>
static K1Kernel<F> k1_kernel(int K, int p1 = 0, int p2 = 0) {
  for (const K1Inst& i : k1_insts)
    if (i.family == F && i.K == K && i.p1 == p1 && i.p2 == p2) return {reinterpret_cast<typename K1Sig<F>::Fn>(i.fn), i.nthr, i.lds ? i.lds(K) : 0};
  return {nullptr, 0, 0};
}
// ... and the one launch of them (a missing kernel is an error)
template <class... Params, class... Args>
static int k1_launch(khg_ctx* ctx, void (*fn)(Params...), unsigned grid, int nthr, size_t lds, hipStream_t s, const Args&... args) {
  if (!fn) return khg_set_error(KHG_E_UNSUPPORTED, "khg_loglikes: no kernel of this form was built");
  int rc = khg_lds_attribute((const void*)fn, lds);
  if (rc) return rc;
  KHG_LAUNCH(ctx, fn, dim3(grid), dim3(nthr), lds, s, args...);
  return KHG_OK;
}
// the three *_pack_x kernels: a grid-stride loop over `work` items per tile of the layout (xoff_d, xutt_d); `tail`: what follows D
template <int F, class... Tail>
static int k1_pack_x(khg_ctx* ctx, int K, const khg_utts* u, const int64_t* xoff_d, const int32_t* xutt_d, int64_t nx, int work, const Tail&... tail) {
  const K1Kernel<F> k = k1_kernel<F>(K);
  const unsigned gb = (unsigned)std::min<int64_t>(65535, (nx * work + 255) / 256);
  return k1_launch(ctx, k.fn, gb, k.nthr, 0, ctx->stream, u->feats_d, u->frame_off_d, xoff_d, xutt_d, nx, u->D, tail...);
}

// 16-frame tiles per wave: 6 x 20 B-operand VGPRs fit 2 waves/SIMD at D <= 40 (KHG_K1_NF=5 selects the smaller chunk)
static int k1_nf(const khg_ctx* ctx, int KQ) { return KQ != 10 ? 5 : ctx->opt[KHG_OPT_K1_NF] == 5 ? 5 : 6; }

// f16x2 scale exponents (khg_k1_f16x2.hip.inc): per k = 2 d + kind, x' = x 2^e and w' = w 2^-e.  `fits`: every scaled
// operand stays <= 2^15 (fp16 overflows at 65504).
static const float K1H_LIMIT = 32768.0f;
static bool k1h_fits(const std::vector<int32_t>& ex, const std::vector<float>& xk, const std::vector<float>& wk) {
  for (size_t k = 0; k < ex.size(); ++k) {
    if (!(std::ldexp(xk[k], ex[k]) <= K1H_LIMIT) || !(std::ldexp(wk[k], -ex[k]) <= K1H_LIMIT)) return false;
  }
  return true;
}
static void k1h_balance(const std::vector<float>& xk, const std::vector<float>& wk, std::vector<int32_t>* ex) {
  ex->assign(xk.size(), 0);
  for (size_t k = 0; k < xk.size(); ++k) {
    const bool hx = xk[k] > 0.0f && std::isfinite(xk[k]), hw = wk[k] > 0.0f && std::isfinite(wk[k]);
    double e = 0.0;
    if (hx && hw) e = 0.5 * (std::log2((double)wk[k]) - std::log2((double)xk[k]));
    else if (hx) e = -std::log2((double)xk[k]);      // only one side has values: bring its maximum to ~1
    else if (hw) e = std::log2((double)wk[k]);
    (*ex)[k] = (int32_t)std::lrint(std::min(120.0, std::max(-120.0, e)));
  }
}
// The split forms (f16x2, f16x2s) fold the log-sum-exp's subtraction into an fma (k1_exp2_le1): valid while every
// log-likelihood term sum stays below 2^28 in magnitude (khg_k1_f16x2.hip.inc, "Domain").
static bool k1_split_domain(const khg_model* m, const std::vector<float>& xk) {
  double bound = (double)m->gcmax;
  for (size_t k = 0; k < xk.size(); ++k) bound += (double)m->wmax[k] * (double)xk[k];
  return bound <= 268435456.0;      // also false for NaN / inf
}

// What one khg_loglikes* call will run: k1_plan decides it from the options, the model's and the set's host-side state and the
// column maxima -- it launches nothing, allocates nothing and writes to neither handle -- and the run function of `form` prepares
// and launches exactly that.  Fields of the forms that do not run stay 0: k1_record copies the plan into khg_utts::k1_last.
struct __attribute__((visibility("hidden"))) K1Plan {
  int form = KHG_K1L_NONE;         // KHG_K1L_*: none for a set without frames or without listed pdfs
  int declined = 0;                // why earlier forms handed over: 1 the split forms' domain, 2 the f16x2s scales, 4 the f16x2 range, 8 a pdf of more than 128 Gaussians
  int K = 0;                       // KS (split forms) or KQ (fp32-MFMA forms)
  int mode = 0;                    // khg_utts::ll_mode of the scores: 0 every cell, 1 from the first needed tile, 2 band
  int maxG = 0;                    // Gaussians of the largest pdf
  int per = 0, order = 0;          // frame tiles per workgroup (wide: frames; pdf-major: TS), chunk order (split forms)
  // f16x2s
  int pack = 0, persistent = 0, tail_shift = 0, shift_mode = 0, units_key = 0, S = 0;
  bool band = false;
  std::vector<int32_t> ex, ew;     // feature exponents to pack with (f16x2s, f16x2); f16x2s: the weights' exponents, S their common part
  // f16x2
  int NTMAX = 0;
  bool planes_fit = false;         // the set's planes are kept: the model still fits their scales
  // utterance-major
  int nf = 0, aligned = 0, interleave = 0;
};
static bool k1_empty(const khg_utts* u) { return u->N == 0 || u->pdfs.empty(); }
// the forms that need k1_maxima: the caller asks for it before k1_plan exactly then (no absmax kernel, no model_stats pass otherwise)
static bool k1_split_asked(const khg_ctx* ctx, const khg_model* m, const khg_utts* u) {
  const int form = ctx->opt[KHG_OPT_K1_FORM];
  return !k1_empty(u) && m->KQ != 0 && (form == KHG_K1_AUTO || form == KHG_K1_F16X2S || form == KHG_K1_F16X2);
}
// f16x2s: one accumulator per chain (khg_k1_f16x2s.hip.inc; the default).  false: the absolute part of its error bound is too large
// for this model.
static bool k1_plan_f16x2s(const khg_ctx* ctx, const khg_model* m, const khg_utts* u, int reach, const std::vector<float>& xk, K1Plan* p) {
  const int KS = m->KS, K = 16 * KS, NMAX = k1s_nmax(KS);
  // exponents: every feature column peaks in [2^14, 2^15) (the set's own property), the largest weight column too (S)
  std::vector<int32_t> ex((size_t)K, 0), ew((size_t)K, 0);
  for (int k = 0; k < K; ++k) if (xk[(size_t)k] > 0.0f) ex[(size_t)k] = 14 - std::ilogb(xk[(size_t)k]);
  // Several utterance sets score against one model (batches of a shard, two contexts): the image is keyed by the feature
  // exponents, so per-set exponents would re-pack the 100 MB image on every alternating call.  The model keeps the element-wise
  // minimum of the exponents of the sets it has scored (a smaller exponent never overflows fp16; the absolute part of the error
  // bound is re-checked below for the exponents actually used) and every set packs its planes with those.
  // (When the shared exponents push the absolute part of the error bound past its limit -- a set with far larger features scored
  //  against this model earlier -- and the set's OWN exponents hold it, the model follows this set: one re-pack instead of the
  //  slower two-accumulator form for every set from here on.)
  const std::vector<int32_t> ex_own = ex;
  int S = 0;
  auto scales = [&]() -> bool {         // S, ew and the floor for the current `ex`
    S = INT_MAX;
    for (int k = 0; k < K; ++k) if (m->wmax[(size_t)k] > 0.0f) S = std::min(S, 14 - std::ilogb(m->wmax[(size_t)k]) + ex[(size_t)k]);
    if (S == INT_MAX) S = 0;
    if (S < -100 || S > 100) return false;
    double floor_sum = 0.0;      // the absolute part of the error bound, at the column maxima (khg_k1_f16x2s.hip.inc)
    for (int k = 0; k < K; ++k) {
      ew[(size_t)k] = S - ex[(size_t)k];
      floor_sum += std::ldexp((double)m->wmax[(size_t)k], ew[(size_t)k]) + std::ldexp((double)xk[(size_t)k], ex[(size_t)k]);
    }
    return std::ldexp(floor_sum, -25 - S) <= 2.0e-6;
  };
  const bool shared = m->xs_ex_seen.size() == ex.size();
  if (shared) for (int k = 0; k < K; ++k) ex[(size_t)k] = std::min(ex[(size_t)k], m->xs_ex_seen[(size_t)k]);
  if (!scales()) {
    if (!shared || ex == ex_own) return false;
    ex = ex_own;
    if (!scales()) return false;
  }
  const bool reachable_only = reach != 0;
  const int dbg = ctx->opt[KHG_OPT_K1_DBG], lopt = ctx->opt[KHG_OPT_K1_LAUNCH];
  p->form = KHG_K1L_F16X2S; p->K = KS; p->ex = std::move(ex); p->ew = std::move(ew); p->S = S;
  // (the order and the cap are the plan's: the chunks are planned once per set)
  // (D > 40: the W image does not fit the Infinity Cache and an utterance is two or three chunks -- their order puts siblings on one XCD:
  //  K1 55.6 -> 52.2 ms at 10 000 x 128 x 80 / 20 000 utterances; at D <= 40 it changes nothing: 56.9 ms either way)
  p->order = (ctx->opt[KHG_OPT_K1_ORDER] == 0 && KS == 10 && !u->small) ? 4 : ctx->opt[KHG_OPT_K1_ORDER];
  // (one or two utterances -- the per-utterance call pattern -- cannot fill the chip with whole utterances: short chunks spread them
  //  over more workgroups; the W tiles are re-read per chunk from the cache, a band that crosses chunks keeps its aligned tiles)
  p->per = (u->small && u->n_utt <= 2) ? std::min(NMAX, 3) : NMAX;
  // models of small pdfs (all <= 8 / <= 16 Gaussians, D <= 40): 4 / 2 pdfs share one MFMA tile (k1s_loglikes_packed)
  p->pack = (KS != 5 || (dbg & 16)) ? 1 : p->maxG <= 8 ? 4 : p->maxG <= 16 ? 2 : 1;
  p->band = reach == 2 && p->pack == 1 && u->pdf_last.size() == u->pdfs.size();     // (the packed kernel keeps the front-only form)
  // (KHG_K1B_DBG bits 32 / 64, A/B only: no shifted tiles / only the 16-frame shift)
  p->shift_mode = (dbg & 32) ? 0 : (dbg & 64) ? 1 : 2;
  // khg_loglikes_reachable (no band): a pdf's tiles run to the utterance's end, which is a band whose last frame is T - 1 -- the same
  // shifted tiles save the same tile (every second pdf); the kernel takes its band path, the fill only meets padding frames
  p->tail_shift = !p->band && reachable_only && p->pack == 1 && p->shift_mode != 0 && u->pdf_first.size() == u->pdfs.size();
  p->units_key = (p->band ? 2 : (int)reachable_only) + 4 * p->shift_mode;
  p->mode = p->band ? 2 : (int)reachable_only;
  // KHG_OPT_K1_LAUNCH: 1 one workgroup per chunk, 2 one persistent workgroup per CU (k1s_persistent); 0: persistent where it
  // measured faster -- at KS = 5 and KS = 10 alike (profiles/r15_k1_chunk_boundary.txt: 54.05 -> 52.78 ms at 100 000 utterances,
  // 6.92 -> 6.68 at 12 500, 50.4 -> 50.0 at D = 80) -- but never for the packed kernels or a small set (the per-utterance call
  // pattern: fewer chunks than CUs, and one more stream-ordered memset per call)
  p->persistent = p->pack == 1 && (lopt == 2 || (lopt == 0 && !u->small));
  return true;
}
// f16x2: two accumulators per chain (khg_k1_f16x2.hip.inc).  false: no exponents bring both operands into fp16's range.
static bool k1_plan_f16x2(const khg_ctx* ctx, const khg_model* m, const khg_utts* u, const std::vector<float>& xk, K1Plan* p) {
  const int KS = m->KS;
  // the set's planes are kept while the model still fits their scales
  const K1Planes& xh = u->k1.xh;
  const bool fit = xh.d && xh.ks == KS && (int)xh.ex.size() == 16 * KS && k1h_fits(xh.ex, xk, m->wmax);
  std::vector<int32_t> ex;
  if (!fit) {
    k1h_balance(xk, m->wmax, &ex);
    if (!k1h_fits(ex, xk, m->wmax)) return false;
  }
  p->form = KHG_K1L_F16X2; p->K = KS; p->planes_fit = fit; p->ex = std::move(ex);
  p->NTMAX = KS == 5 ? 2 : K1H_NT10; p->per = 8 * p->NTMAX; p->order = ctx->opt[KHG_OPT_K1_ORDER];
  return true;
}
// which K1: f16x2s (default: the fp16 matrix cores at fp32 accuracy) -> f16x2 -> one of the fp32-MFMA forms -- pdf-major (pdfs of
// <= 128 Gaussians) / utterance-major -- whose per-Gaussian fmaf chain is pinned bit for bit by the tests.  reach: 0 every cell,
// 1 from a pdf's first needed tile, 2 band; xk: k1_maxima's, empty unless k1_split_asked.
static K1Plan k1_plan(const khg_ctx* ctx, const khg_model* m, const khg_utts* u, int reach, const std::vector<float>& xk) {
  K1Plan p;
  const bool reachable_only = reach != 0;
  p.mode = (int)reachable_only;
  if (k1_empty(u)) return p;
  if (m->KQ == 0) { p.form = KHG_K1L_WIDE; p.per = 64; return p; }      // D > 80: one form
  for (int q = 0; q < m->P; ++q) p.maxG = std::max(p.maxG, m->gauss_off[q + 1] - m->gauss_off[q]);
  int form = ctx->opt[KHG_OPT_K1_FORM];
  if (form == KHG_K1_AUTO) form = KHG_K1_F16X2S;
  if ((form == KHG_K1_F16X2S || form == KHG_K1_F16X2) && !k1_split_domain(m, xk)) { p.declined |= 1; form = KHG_K1_FP32_PDF; }   // magnitudes outside the split forms' domain
  if (form == KHG_K1_F16X2S) {
    if (k1_plan_f16x2s(ctx, m, u, reach, xk, &p)) return p;
    p.declined |= 2; form = KHG_K1_F16X2;
  }
  if (form == KHG_K1_F16X2) {
    if (k1_plan_f16x2(ctx, m, u, xk, &p)) return p;
    p.declined |= 4; form = KHG_K1_FP32_PDF;
  }
  if (form == KHG_K1_FP32_PDF && p.maxG <= 128) {
    p.form = KHG_K1L_PDF; p.K = m->KQ; p.per = std::max(1, ctx->opt[KHG_OPT_K1P_TS]);      // slices of <= TS tiles
    return p;
  }
  if (form == KHG_K1_FP32_PDF) p.declined |= 8;
  p.form = KHG_K1L_UTT; p.K = m->KQ; p.nf = k1_nf(ctx, m->KQ); p.per = 4 * p.nf;
  p.interleave = ctx->opt[KHG_OPT_K1_INTERLEAVE] >= 0 ? ctx->opt[KHG_OPT_K1_INTERLEAVE] : (int)reachable_only;
  p.aligned = (m->D % 4 == 0) && ((reinterpret_cast<uintptr_t>(u->feats_d) & 15) == 0);
  return p;
}
// khg_utts_k1_last: this call's record
static void k1_record(const khg_ctx* ctx, khg_utts* u, const K1Plan& p) {
  int32_t* r = u->k1_last;
  std::fill(r, r + KHG_K1_LAST_WORDS, 0);
  r[K1L_SET] = 1; r[K1L_FORM] = p.form; r[K1L_ASKED] = k1l_form(ctx->opt[KHG_OPT_K1_FORM]); r[K1L_DECLINED] = p.declined; r[K1L_K] = p.K;
  r[K1L_MODE] = p.mode; r[K1L_PACK] = p.pack; r[K1L_PERSISTENT] = p.persistent; r[K1L_PER] = p.per; r[K1L_ORDER] = p.order;
  r[K1L_TAIL_SHIFT] = p.tail_shift; r[K1L_SHIFT_MODE] = p.shift_mode; r[K1L_NF] = p.nf; r[K1L_ALIGNED] = p.aligned; r[K1L_INTERLEAVE] = p.interleave;
}
static void k1_record_grid(khg_utts* u, int chunks, int grid) { u->k1_last[K1L_CHUNKS] = chunks; u->k1_last[K1L_GRID] = grid; }

// column maxima of |a[n][D]| -> host
static int absmax_cols(khg_ctx* ctx, const float* a_d, int64_t n, int D, std::vector<float>* out) {
  uint32_t* m_d = nullptr;
  int rc = dev_alloc(&m_d, 128);
  if (rc) return rc;
  std::vector<uint32_t> h(128, 0);
  hipError_t e = hipMemsetAsync(m_d, 0, 128 * sizeof(uint32_t), ctx->stream);
  if (e == hipSuccess && n > 0) {
    const int gb = (int)std::min<int64_t>(4096, (n + 1) / 2);
    KernelTimer kt(ctx, "k1_absmax");
    KHG_LAUNCH(ctx, k1h_absmax, dim3(gb), dim3(256), 0, ctx->stream, a_d, n, D, m_d);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(h.data(), m_d, 128 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  DEVFREE(m_d);
  if (e != hipSuccess) return khg_set_error(KHG_E_HIP, hipGetErrorString(e));
  out->resize((size_t)D);
  for (int d = 0; d < D; ++d) memcpy(&(*out)[(size_t)d], &h[(size_t)d], sizeof(float));
  return KHG_OK;
}
// Exact maxima behind the split forms' domain check and the f16x2 scales: per feature dimension over the set (once), per
// k = 2 d + kind and over the gconsts for the model (once per parameter version).  -> xk[k] = max |X[k][.]|.
int k1_maxima(khg_ctx* ctx, khg_model* m, khg_utts* u, std::vector<float>* xk) {
  const int D = m->D, K = 16 * m->KS;
  int rc = KHG_OK;
  if (u->k1.xmax.empty()) { rc = absmax_cols(ctx, u->feats_d, u->N, D, &u->k1.xmax); if (rc) return rc; }
  if (m->wmax.empty()) { rc = model_stats(ctx, m); if (rc) return rc; }      // one pass per parameter version (khg_ctx_model.hip)
  xk->assign((size_t)K, 0.0f);
  for (int d = 0; d < D; ++d) { (*xk)[(size_t)2 * d] = u->k1.xmax[(size_t)d]; (*xk)[(size_t)2 * d + 1] = u->k1.xmax[(size_t)d] * u->k1.xmax[(size_t)d]; }
  return KHG_OK;
}

// The set cut into tiles of `frames` frames, utterance by utterance: tile offsets per utterance, tile -> utterance; -> the number of tiles
static int64_t k1_tile_layout(const khg_utts* u, int frames, std::vector<int64_t>* xoff, std::vector<int32_t>* xutt) {
  xoff->assign((size_t)u->n_utt + 1, 0);
  for (int i = 0; i < u->n_utt; ++i) (*xoff)[(size_t)i + 1] = (*xoff)[(size_t)i] + (u->frame_off[i + 1] - u->frame_off[i] + frames - 1) / frames;
  const int64_t nx = (*xoff)[(size_t)u->n_utt];
  xutt->resize((size_t)nx);
  for (int i = 0; i < u->n_utt; ++i)
    for (int64_t t = (*xoff)[(size_t)i]; t < (*xoff)[(size_t)i + 1]; ++t) (*xutt)[(size_t)t] = i;
  return nx;
}

// D > 80: k1w_loglikes over 64-frame chunks (every cell of every listed pdf; khg_k1_wide.hip.inc)
static int run_wide(khg_ctx* ctx, const khg_model* m, khg_utts* u) {
  K1Set& s = u->k1;
  if (!s.wchunks_d) {
    std::vector<KwChunk> ch;
    for (int i = 0; i < u->n_utt; ++i) {
      const int64_t T = u->frame_off[i + 1] - u->frame_off[i];
      if (T <= 0 || u->pdf_off[i + 1] == u->pdf_off[i]) continue;
      for (int64_t t0 = 0; t0 < T; t0 += 64) ch.push_back(KwChunk{i, (int32_t)t0, (int32_t)std::min<int64_t>(64, T - t0), 0});
    }
    s.n_wchunks = (int)ch.size();
    int rc = u_upload(ctx, u, &s.wchunks_d, ch);
    if (rc) return rc;
    { int rs = sync_pageable(ctx); if (rs) return rs; }
  }
  KwArgs a;
  a.feats = u->feats_d; a.frame_off = u->frame_off_d; a.chunks = s.wchunks_d; a.pdf_off = u->pdf_off_d; a.pdfs = u->pdfs_d;
  a.gauss_off = m->gauss_off_d; a.gconsts = m->gconsts_d; a.means_invvars = m->miv_d; a.nhalf_inv_vars = m->nhiv_d;
  a.ll = u->ll_d; a.ll_off = u->ll_off_d; a.err_flag = ctx->err_flag_d; a.D = m->D;
  k1_record_grid(u, s.n_wchunks, s.n_wchunks);
  if (s.n_wchunks > 0) {
    const K1Kernel<K1_WIDE> k = k1_kernel<K1_WIDE>(0);
    KernelTimer kt(ctx, "k1_loglikes");
    int rc = k1_launch(ctx, k.fn, s.n_wchunks, k.nthr, sizeof(float) * 64 * (size_t)(m->D | 1), ctx->stream, a);
    if (rc) return rc;
  }
  HIPCHK(hipGetLastError());
  return KHG_OK;
}

// K1 in pdf-major form: plan (entries grouped by pdf, cut into workgroup slices) + repacked features.
static int run_pdf_major(khg_ctx* ctx, const khg_model* m, khg_utts* u, const K1Plan& p) {
  K1Set& s = u->k1;
  const bool reachable_only = p.mode != 0;
  int rc = KHG_OK;
  const int KH = 2 * m->KQ;
  if (!s.xpl_d || s.xpl_kq != m->KQ) {
    // x tiles: ceil(T/16) per utterance, parity planes [2][16][KH] each
    DEVFREE(s.xpl_d); DEVFREE(s.utt_xtile_off_d);
    std::vector<int64_t> xoff;
    std::vector<int32_t> xutt;
    const int64_t nx = k1_tile_layout(u, 16, &xoff, &xutt);
    int32_t* xutt_d = nullptr;
    rc = u_upload(ctx, u, &s.utt_xtile_off_d, xoff);
    if (!rc) rc = dev_upload(ctx, &xutt_d, xutt);
    if (!rc) rc = u_alloc(u, &s.xpl_d, (size_t)std::max<int64_t>(nx, 1) * 2 * 16 * KH);
    if (!rc && nx > 0) {
      rc = k1_pack_x<K1_PACK_P>(ctx, m->KQ, u, s.utt_xtile_off_d, xutt_d, nx, 2 * 16 * KH / 4, s.xpl_d);
      hipError_t e = hipGetLastError();
      if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
      if (!rc && e != hipSuccess) rc = khg_set_error(KHG_E_HIP, hipGetErrorString(e));
    }
    DEVFREE(xutt_d);
    if (rc) return rc;
    s.xpl_kq = m->KQ;
    if (nx > 0) u->k1_last[K1L_REPACKED] |= 1;
  }
  if (!s.p_ents_d || s.p_reach != (int)reachable_only || s.p_P != m->P || s.p_goff != m->gauss_off) {
    DEVFREE(s.p_ents_d); DEVFREE(s.p_slices_d);
    // entries grouped by pdf (counting sort keeps utterance order inside a pdf)
    std::vector<int64_t> cnt((size_t)m->P + 1, 0);
    for (int32_t q : u->pdfs) cnt[(size_t)q + 1]++;
    for (int q = 0; q < m->P; ++q) cnt[(size_t)q + 1] += cnt[(size_t)q];
    std::vector<K1pEntry> ents(u->pdfs.size());
    std::vector<int64_t> cur(cnt.begin(), cnt.end() - 1);
    for (int i = 0; i < u->n_utt; ++i) {
      const int n16 = (int)((u->frame_off[i + 1] - u->frame_off[i] + 15) / 16);
      for (int64_t k = u->pdf_off[i]; k < u->pdf_off[i + 1]; ++k) {
        int ef = 0;
        if (reachable_only) ef = (int)std::min<int64_t>(n16, (int64_t)u->pdf_first[(size_t)k] / 16);
        ents[(size_t)cur[(size_t)u->pdfs[(size_t)k]]++] = K1pEntry{i, (int32_t)(k - u->pdf_off[i]), ef, n16 - ef};
      }
    }
    // slices: <= TS tiles and <= K1P_MAXENT entries of one pdf each
    const int TS = p.per;
    std::vector<K1pSlice> slices;
    for (int q = 0; q < m->P; ++q) {
      int64_t e = cnt[(size_t)q];
      const int64_t e_end = cnt[(size_t)q + 1];
      int off = 0;                             // tiles of entry e already given out
      while (e < e_end) {
        while (e < e_end && ents[(size_t)e].nt - off <= 0) { ++e; off = 0; }
        if (e >= e_end) break;
        K1pSlice sl{q, (int32_t)e, 0, off, 0};
        int64_t ee = e;
        int o = off;
        while (ee < e_end && sl.ntiles < TS && sl.nent < K1P_MAXENT) {
          const int avail = ents[(size_t)ee].nt - o;
          if (avail <= 0) { ++sl.nent; ++ee; o = 0; continue; }
          const int take = std::min(avail, TS - sl.ntiles);
          sl.ntiles += take;
          ++sl.nent;
          if (take == avail) { ++ee; o = 0; } else { o += take; break; }
        }
        if (sl.ntiles > 0) slices.push_back(sl);
        e = ee; off = o;
      }
    }
    // group the slices by the pdf's number of 16-Gaussian blocks: one launch (kernel instantiation) per count
    auto nblk_of = [&](const K1pSlice& x) { return (m->gauss_off[x.pdf + 1] - m->gauss_off[x.pdf] + 15) / 16; };
    std::stable_sort(slices.begin(), slices.end(), [&](const K1pSlice& x, const K1pSlice& y) { return nblk_of(x) < nblk_of(y); });
    for (int k = 0; k < 10; ++k) s.p_grp[k] = 0;
    for (const auto& x : slices) s.p_grp[nblk_of(x)]++;          // counts per block count 1..8
    if (ents.size() >= (size_t)INT32_MAX) return khg_set_error(KHG_E_UNSUPPORTED, "khg_loglikes: too many (utterance, pdf) entries");
    rc = u_upload(ctx, u, &s.p_ents_d, ents);
    if (!rc) rc = u_upload(ctx, u, &s.p_slices_d, slices);
    if (rc) return rc;
    { int rs = sync_pageable(ctx); if (rs) return rs; }
    s.p_nslices = (int32_t)slices.size();
    if (ctx->opt[KHG_OPT_DEBUG]) { long long tt = 0; for (auto& x : slices) tt += x.ntiles; fprintf(stderr, "[khg] pdf-major plan: %zu entries, %zu slices, %lld tiles\n", ents.size(), slices.size(), tt); }
    s.p_reach = (int)reachable_only;
    s.p_P = m->P;
    s.p_goff = m->gauss_off;
  }
  K1pArgs a;
  a.xpl = s.xpl_d; a.utt_xtile_off = s.utt_xtile_off_d; a.frame_off = u->frame_off_d;
  a.ents = s.p_ents_d; a.slices = s.p_slices_d; a.wimg = m->wimg_d; a.pdf_tile_off = m->pdf_tile_off_d;
  a.gauss_off = m->gauss_off_d; a.ll = u->ll_d; a.ll_off = u->ll_off_d; a.err_flag = ctx->err_flag_d;
  k1_record_grid(u, s.p_nslices, s.p_nslices);
  for (int nb = 1; nb <= 8; ++nb) u->k1_last[K1L_NB_SLICES + nb - 1] = s.p_grp[nb];
  if (s.p_nslices > 0) {
    KernelTimer kt(ctx, "k1_loglikes");
    int first = 0;
    for (int nb = 1; nb <= 8; ++nb) {
      const int n = s.p_grp[nb];
      if (n == 0) continue;
      a.slice0 = first;
      first += n;
      const K1Kernel<K1_PDF> k = k1_kernel<K1_PDF>(m->KQ, nb);
      rc = k1_launch(ctx, k.fn, n, k.nthr, 0, ctx->stream, a);
      if (rc) return rc;
    }
    HIPCHK(hipGetLastError());
  }
  return KHG_OK;
}

// per-utterance W-tile walk for this model's tile layout (it only changes when the number of Gaussians of some pdf
// crosses a multiple of 32): for every pdf on the utterance's list its 32-Gaussian tiles in order.  Entry = tile id
// (bits 0-21) | first needed 16-frame tile of the pdf, clamped to 127 (bits 22-28; 0 unless reachable_only) |
// last-tile-of-pdf flag (bit 31).  Shared by the utterance-major fp32 kernel and the f16x2 kernel.
static int ensure_walk(khg_ctx* ctx, const khg_model* m, khg_utts* u, bool reachable_only) {
  K1Set& s = u->k1;
  if (s.tiles_pto == m->pdf_tile_off && s.tiles_reach == (int)reachable_only) return KHG_OK;
  if (m->ntiles >= (1 << 22)) return khg_set_error(KHG_E_UNSUPPORTED, "khg_loglikes: more than 4M W tiles");
  DEVFREE(s.tile_off_d); DEVFREE(s.tiles_d);
  std::vector<int64_t> toff((size_t)u->n_utt + 1, 0);
  std::vector<int32_t> tiles;
  for (int i = 0; i < u->n_utt; ++i) {
    for (int64_t k = u->pdf_off[i]; k < u->pdf_off[i + 1]; ++k) {
      const int q = u->pdfs[(size_t)k];
      int ef = 0;
      if (reachable_only) ef = (int)std::min<int64_t>(127, (int64_t)u->pdf_first[(size_t)k] / 16);
      for (int t = m->pdf_tile_off[q]; t < m->pdf_tile_off[q + 1]; ++t)
        tiles.push_back(t | (ef << 22) | (t + 1 == m->pdf_tile_off[q + 1] ? (int32_t)0x80000000 : 0));
    }
    toff[(size_t)i + 1] = (int64_t)tiles.size();
  }
  int rc = u_upload(ctx, u, &s.tile_off_d, toff);
  if (!rc) rc = u_upload(ctx, u, &s.tiles_d, tiles);
  if (rc) return rc;
  { int rs = sync_pageable(ctx); if (rs) return rs; }
  s.tiles_pto = m->pdf_tile_off;
  s.tiles_reach = (int)reachable_only;
  return KHG_OK;
}

// the utterance-major fp32-MFMA form (khg_k1_loglikes.hip.inc): chunks of <= 4 nf 16-frame tiles, equal parts per utterance
static int run_utt_major(khg_ctx* ctx, const khg_model* m, khg_utts* u, const K1Plan& p) {
  K1Set& s = u->k1;
  int rc = KHG_OK;
  if (!s.chunks_d || s.chunk_kq != m->KQ * 16 + p.nf) {
    DEVFREE(s.chunks_d);
    const int maxtiles = p.per;
    std::vector<K1Chunk> ch;
    for (int i = 0; i < u->n_utt; ++i) {
      int64_t T = u->frame_off[i + 1] - u->frame_off[i];
      if (T <= 0 || u->pdf_off[i + 1] == u->pdf_off[i]) continue;
      int n16 = (int)((T + 15) / 16);
      int nchunks = (n16 + maxtiles - 1) / maxtiles;
      int per = (n16 + nchunks - 1) / nchunks;
      for (int c = 0; c < nchunks; ++c) {
        int t0 = c * per * 16;
        int nfr = (int)std::min<int64_t>((int64_t)per * 16, T - t0);
        if (nfr <= 0) break;
        ch.push_back(K1Chunk{i, t0, nfr, 0});
      }
    }
    s.n_chunks = (int)ch.size();
    s.chunk_kq = m->KQ * 16 + p.nf;
    rc = u_upload(ctx, u, &s.chunks_d, ch);
    if (rc) return rc;
    { int rs = sync_pageable(ctx); if (rs) return rs; }  // ch is a local
  }
  rc = ensure_walk(ctx, m, u, p.mode != 0);
  if (rc) return rc;
  K1Args a;
  a.feats = u->feats_d; a.frame_off = u->frame_off_d; a.chunks = s.chunks_d; a.wimg = m->wimg_d;
  a.utt_tile_off = s.tile_off_d; a.utt_tiles = s.tiles_d;
  a.ll = u->ll_d; a.ll_off = u->ll_off_d; a.err_flag = ctx->err_flag_d; a.D = m->D;
  a.interleave = p.interleave;
  k1_record_grid(u, s.n_chunks, s.n_chunks);
  if (s.n_chunks > 0) {
    const K1Kernel<K1_UTT> k = k1_kernel<K1_UTT>(m->KQ, p.nf, p.aligned);
    KernelTimer kt(ctx, "k1_loglikes");
    rc = k1_launch(ctx, k.fn, s.n_chunks, k.nthr, 0, ctx->stream, a);
    if (rc) return rc;
    HIPCHK(hipGetLastError());
  }
  return KHG_OK;
}

// 32-frame tile layout of the set shared by the f16x2 / f16x2s forms: tile offsets per utterance, tile -> utterance.
static int ensure_x32_layout(khg_ctx* ctx, khg_utts* u) {
  K1Set& s = u->k1;
  if (s.utt_x32_off_d) return KHG_OK;
  std::vector<int64_t> xoff;
  std::vector<int32_t> xutt;
  const int64_t nx = k1_tile_layout(u, 32, &xoff, &xutt);
  int rc = u_upload(ctx, u, &s.utt_x32_off_d, xoff);
  if (!rc) rc = u_upload(ctx, u, &s.x32_utt_d, xutt);
  if (rc) return rc;
  { int rs = sync_pageable(ctx); if (rs) return rs; }
  s.n_x32 = nx;
  return KHG_OK;
}
// Workgroup chunks of <= `per` 32-frame tiles: an utterance is cut into equal parts (a 17-tile utterance becomes 9 + 8 tiles, not
// 16 + 1), and the chunks are launched longest first (duration ~ frame tiles x pdfs): the workgroups still running when the grid
// drains are then the short ones (a launch of 12 500 utterances -- the 8-GPU shard -- is ~49 rounds of workgroups whose durations
// differ 4x).  K1bChunk and K1sChunk have the same layout.
template <class Chunk>
static void plan_x32_chunks(const khg_utts* u, int per, int order, std::vector<Chunk>* ch) {
  ch->clear();
  for (int i = 0; i < u->n_utt; ++i) {
    const int n32 = (int)((u->frame_off[i + 1] - u->frame_off[i] + 31) / 32);
    if (u->pdf_off[i + 1] == u->pdf_off[i]) continue;
    const int nch = (n32 + per - 1) / per;
    for (int c = 0; c < nch; ++c) {
      const int t0 = (int)((int64_t)n32 * c / nch), t1 = (int)((int64_t)n32 * (c + 1) / nch);
      if (t1 > t0) ch->push_back(Chunk{i, t0, t1 - t0, 0});
    }
  }
  // KHG_OPT_K1_ORDER (experiments): 0 frame tiles x pdfs descending (default), 1 utterance order, 2 ascending, 3 frame tiles descending,
  // 4 the chunks of ONE utterance eight positions apart: workgroups go to the eight XCDs round-robin, so siblings -- which walk the same
  // pdf list, i.e. the same W tiles, at about the same time -- share an L2 (the second one's W loads need not come from HBM)
  if (order == 4) {
    std::vector<int32_t> first(1, 0);                       // chunks are grouped by utterance: first[i] = first chunk of group i
    for (size_t i = 1; i < ch->size(); ++i) if ((*ch)[i].utt != (*ch)[i - 1].utt) first.push_back((int32_t)i);
    first.push_back((int32_t)ch->size());
    const int ng = (int)first.size() - 1;
    std::vector<int32_t> grp((size_t)ng);
    for (int i = 0; i < ng; ++i) grp[(size_t)i] = i;
    auto gcost = [&](int g) { int64_t t = 0; for (int k = first[(size_t)g]; k < first[(size_t)g + 1]; ++k) t += (*ch)[(size_t)k].ntiles; return t * (u->pdf_off[(*ch)[(size_t)first[(size_t)g]].utt + 1] - u->pdf_off[(*ch)[(size_t)first[(size_t)g]].utt]); };
    auto gn = [&](int g) { return first[(size_t)g + 1] - first[(size_t)g]; };
    std::stable_sort(grp.begin(), grp.end(), [&](int a, int b) { return gn(a) != gn(b) ? gn(a) > gn(b) : gcost(a) > gcost(b); });
    std::vector<Chunk> out;
    out.reserve(ch->size());
    for (int b = 0; b < ng; b += 8) {                       // a band of eight utterances: round r = chunk r of each
      const int nb = std::min(8, ng - b);
      int rounds = 0;
      for (int i = 0; i < nb; ++i) rounds = std::max(rounds, gn(grp[(size_t)(b + i)]));
      for (int r = 0; r < rounds; ++r)
        for (int i = 0; i < nb; ++i) {
          const int g = grp[(size_t)(b + i)];
          if (r < gn(g)) out.push_back((*ch)[(size_t)(first[(size_t)g] + r)]);
          else out.push_back(Chunk{(*ch)[(size_t)first[(size_t)g]].utt, 0, 0, 0});      // (an empty workgroup keeps the band's XCD alignment)
        }
    }
    ch->swap(out);
    return;
  }
  auto cost = [&](const Chunk& c) { return (int64_t)c.ntiles * (order == 3 ? 1 : (u->pdf_off[c.utt + 1] - u->pdf_off[c.utt])); };
  if (order == 2) std::stable_sort(ch->begin(), ch->end(), [&](const Chunk& a, const Chunk& b) { return cost(a) < cost(b); });
  else if (order != 1) std::stable_sort(ch->begin(), ch->end(), [&](const Chunk& a, const Chunk& b) { return cost(a) > cost(b); });
}
// the layout, and the set's chunks for a cap of `per` tiles: planned once per (set, key), whichever order that call asked for
template <class Chunk>
static int ensure_x32_chunks(khg_ctx* ctx, khg_utts* u, int per, int order, int key, Chunk** chunks_d, int32_t* n, int32_t* have_key) {
  int rc = ensure_x32_layout(ctx, u);
  if (rc) return rc;
  if (*chunks_d && *have_key == key) return KHG_OK;
  DEVFREE(*chunks_d);
  std::vector<Chunk> ch;
  plan_x32_chunks(u, per, order, &ch);
  rc = u_upload(ctx, u, chunks_d, ch);
  if (rc) return rc;
  { int rs = sync_pageable(ctx); if (rs) return rs; }
  *n = (int32_t)ch.size(); *have_key = key;
  return KHG_OK;
}

// the set's B fragments of a split form (F: its *_pack_x family) packed with the exponents `ex`: the planes, `ex` on the device and on the host
template <int F>
static int k1_pack_planes(khg_ctx* ctx, khg_utts* u, int KS, const std::vector<int32_t>& ex, const char* timer, K1Planes* x) {
  const K1Set& s = u->k1;
  if (!x->d || x->ks != KS) {
    DEVFREE(x->d);
    int rc = u_alloc(u, &x->d, (size_t)std::max<int64_t>(s.n_x32, 1) * 2 * KS * 64);
    if (rc) return rc;
  }
  DEVFREE(x->ex_d);
  int rc = u_upload(ctx, u, &x->ex_d, ex);
  if (rc) return rc;
  if (s.n_x32 > 0) {
    KernelTimer kt(ctx, timer);
    rc = k1_pack_x<F>(ctx, KS, u, s.utt_x32_off_d, s.x32_utt_d, s.n_x32, KS * 64, x->ex_d, x->d);
    if (rc) return rc;
    HIPCHK(hipGetLastError());
  }
  { int rs = sync_pageable(ctx); if (rs) return rs; }    // the upload has read `ex` (pageable) after this
  x->ks = KS; x->ex = ex;
  if (s.n_x32 > 0) u->k1_last[K1L_REPACKED] |= 1;
  return KHG_OK;
}

// K1H_TIMING, the measurement build of the f16x2 form (its kernel part: khg_k1_f16x2.hip.inc): 8 counters per wave, reported as a
// per-wave cycle breakdown averaged by the number of frame tiles the wave owns
#ifdef K1H_TIMING
static int k1h_timing_begin(khg_ctx* ctx, int nchunks, K1hArgs* a) {
  int rc = dev_alloc(&a->tbuf, (size_t)nchunks * 64);
  if (rc) return rc;
  HIPCHK(hipMemsetAsync(a->tbuf, 0, (size_t)nchunks * 64 * sizeof(uint64_t), ctx->stream));
  return KHG_OK;
}
static int k1h_timing_report(khg_ctx* ctx, int nchunks, K1hArgs* a) {
  std::vector<uint64_t> h((size_t)nchunks * 64);
  HIPCHK(hipMemcpyAsync(h.data(), a->tbuf, h.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  double sum[3][8] = {};
  long cnt[3] = {0, 0, 0};
  for (size_t w = 0; w < h.size() / 8; ++w) {
    const uint64_t* o = &h[w * 8];
    if (o[5] == 0 || o[6] > 2) continue;
    for (int i = 0; i < 8; ++i) sum[o[6]][i] += (double)o[i];
    ++cnt[o[6]];
  }
  for (int nt = 0; nt < 3; ++nt)
    if (cnt[nt]) fprintf(stderr, "k1h timing NT=%d waves=%ld: per wave cycles(100MHz-or-core clock units): barrier %.0f frag-wait %.0f chains %.0f tail %.0f total %.0f; tiles %.1f intervals %.1f\n",
                         nt, cnt[nt], sum[nt][0] / cnt[nt], sum[nt][1] / cnt[nt], sum[nt][2] / cnt[nt], sum[nt][3] / cnt[nt], sum[nt][5] / cnt[nt], sum[nt][4] / cnt[nt], sum[nt][7] / cnt[nt]);
  DEVFREE(a->tbuf);
  return KHG_OK;
}
#else
static int k1h_timing_begin(khg_ctx*, int, K1hArgs*) { return KHG_OK; }
static int k1h_timing_report(khg_ctx*, int, K1hArgs*) { return KHG_OK; }
#endif

// K1 on the fp16 matrix cores, two accumulators per chain (khg_k1_f16x2.hip.inc)
static int run_f16x2(khg_ctx* ctx, khg_model* m, khg_utts* u, const K1Plan& p) {
  K1Set& s = u->k1;
  const int KS = p.K;
  int rc = ensure_x32_chunks(ctx, u, p.per, p.order, p.NTMAX, &s.bchunks_d, &s.n_bchunks, &s.bchunk_nt);
  if (rc) return rc;
  if (!p.planes_fit) { rc = k1_pack_planes<K1_PACK_H>(ctx, u, KS, p.ex, "k1h_pack_x", &s.xh); if (rc) return rc; }
  if (m->wimgh_ex != s.xh.ex) {
    if (!m->wimgh_d || m->wimgh_tiles < m->ntiles) {
      DEVFREE(m->wimgh_d);
      rc = dev_alloc(&m->wimgh_d, (size_t)m->ntiles * k1h_tile_bytes(KS));
      if (rc) return rc;
      m->wimgh_tiles = m->ntiles;
    }
    rc = m->wimgh_sync.before_pack(ctx->stream);
    if (rc) return rc;
    const K1Kernel<K1_IMG_H> k = k1_kernel<K1_IMG_H>(KS);
    KernelTimer kt(ctx, "k0h_pack_tiles");
    rc = k1_launch(ctx, k.fn, m->ntiles, k.nthr, 0, ctx->stream, m->gconsts_d, m->miv_d, m->iv_d, m->gauss_off_d, m->pdf_tile_off_d, m->tile_pdf_d, m->D, s.xh.ex_d, m->wimgh_d);
    if (rc) return rc;
    HIPCHK(hipGetLastError());
    rc = m->wimgh_sync.after_pack(ctx->stream);
    if (rc) return rc;
    m->wimgh_ex = s.xh.ex;
    u->k1_last[K1L_REPACKED] |= 2;
  }
  rc = ensure_walk(ctx, m, u, p.mode != 0);
  if (rc) return rc;
  K1hArgs a;
  a.xh = s.xh.d; a.utt_xtile_off = s.utt_x32_off_d; a.frame_off = u->frame_off_d; a.chunks = s.bchunks_d;
  a.wimg = m->wimgh_d; a.utt_tile_off = s.tile_off_d; a.utt_tiles = s.tiles_d;
  a.ll = u->ll_d; a.ll_off = u->ll_off_d; a.err_flag = ctx->err_flag_d;
  a.dbg = ctx->opt[KHG_OPT_K1_DBG];
  a.tbuf = nullptr;
  k1_record_grid(u, s.n_bchunks, s.n_bchunks);
  if (s.n_bchunks <= 0) return KHG_OK;
  rc = k1h_timing_begin(ctx, s.n_bchunks, &a);
  if (rc) return rc;
  rc = m->wimgh_sync.before_read(ctx->stream);
  if (rc) return rc;
  {
    const K1Kernel<K1_H> k = k1_kernel<K1_H>(KS, p.NTMAX);
    KernelTimer kt(ctx, "k1_loglikes");
    rc = k1_launch(ctx, k.fn, s.n_bchunks, k.nthr, k.lds, ctx->stream, a);
    if (rc) return rc;
  }
  HIPCHK(hipGetLastError());
  rc = m->wimgh_sync.after_read(ctx->stream);
  if (rc) return rc;
  return k1h_timing_report(ctx, s.n_bchunks, &a);
}

// KHG_OPT_K1_PROF: the chunks' stamps (K1sArgs::stamps) -> one line on stderr.  Per CU the chunks are put in the order they ran;
// "boundary" is the time between the moment a chunk's LAST wave found the work-item counter exhausted and the moment the next chunk
// of that CU passed its barrier (no MFMA of either in between), "tail" the time between a chunk's FIRST and LAST exhausted wave
// (some SIMDs idle), "fill" entry to barrier; all as shares of the CUs' busy spans (first entry to last exhaustion).
static void k1_prof_report(const std::vector<long long>& st, const char* launch, int KS) {
  struct Rec { long long cu, t0, t1, t2, t3; };
  std::vector<Rec> r;
  for (size_t i = 0; i + 8 <= st.size(); i += 8)
    if (st[i + 3] > 0 && st[i + 1] > 0) r.push_back(Rec{st[i + 4], st[i], st[i + 1], st[i + 2], st[i + 3]});
  std::sort(r.begin(), r.end(), [](const Rec& x, const Rec& y) { return x.cu != y.cu ? x.cu < y.cu : x.t1 < y.t1; });
  double span = 0, boundary = 0, tail = 0, fill = 0;
  size_t ncu = 0;
  for (size_t i = 0; i < r.size();) {
    size_t j = i;
    while (j < r.size() && r[j].cu == r[i].cu) ++j;
    long long end = r[i].t3;
    for (size_t k = i; k < j; ++k) {
      if (k > i && r[k].t1 > r[k - 1].t3) boundary += (double)(r[k].t1 - r[k - 1].t3);
      tail += (double)(r[k].t3 - r[k].t2);
      fill += (double)(r[k].t1 - r[k].t0);
      end = std::max(end, r[k].t3);
    }
    span += (double)(end - r[i].t0);
    ++ncu; i = j;
  }
  if (span <= 0) { fprintf(stderr, "[KHG_K1_PROF] no stamps\n"); return; }
  fprintf(stderr, "[KHG_K1_PROF] KS %d, %s: %zu chunks on %zu CUs | shares of the CUs' busy span: boundary (last wave done -> next chunk past its barrier) %.4f, "
          "tail (first -> last wave done) %.4f, fill (entry -> barrier) %.4f | ticks per chunk: boundary %.0f tail %.0f fill %.0f span %.0f\n",
          KS, launch, r.size(), ncu, boundary / span, tail / span, fill / span, boundary / r.size(), tail / r.size(), fill / r.size(), span / r.size());
}
// ... boundary stamps of every chunk (a diagnostic: the launch is followed by a download and a wait)
static int k1_prof_begin(khg_ctx* ctx, int nchunks, K1sArgs* a) {
  int rc = dev_alloc(&a->stamps, (size_t)nchunks * 8);
  if (rc) return rc;
  HIPCHK(hipMemsetAsync(a->stamps, 0, sizeof(long long) * 8 * (size_t)nchunks, ctx->stream));
  return KHG_OK;
}
static int k1_prof_end(khg_ctx* ctx, int nchunks, K1sArgs* a, bool persistent, int KS) {
  std::vector<long long> st((size_t)nchunks * 8);
  hipError_t e = hipMemcpyAsync(st.data(), a->stamps, sizeof(long long) * st.size(), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  DEVFREE(a->stamps);
  if (e != hipSuccess) return khg_set_error(KHG_E_HIP, hipGetErrorString(e));
  k1_prof_report(st, persistent ? "persistent" : "one chunk per workgroup", KS);
  return KHG_OK;
}

// the persistent launch's grid: one workgroup per CU that can hold one -- from the occupancy query, once per context and kernel, asked
// after the kernel's LDS attribute is set -- but no more than there are chunks (or KHG_OPT_K1_PGRID); its chunk counter, zeroed on the stream
static int k1_persistent_grid(khg_ctx* ctx, const K1Kernel<K1_S_PERSISTENT>& k, int KS, int nchunks, int* pgrid) {
  int& cached = ctx->k1_pgrid[KS == 5 ? 0 : 1];
  if (cached <= 0) {
    int per_cu = 0, ncu = 0;
    int rc = khg_lds_attribute((const void*)k.fn, k.lds);
    if (rc) return rc;
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)k.fn, k.nthr, k.lds));
    HIPCHK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, ctx->device));
    if (per_cu <= 0 || ncu <= 0) return khg_set_error(KHG_E_HIP, "khg_loglikes: the persistent K1 kernel does not fit a CU");
    cached = per_cu * ncu;
  }
  *pgrid = std::min<int>(cached, nchunks);
  if (ctx->opt[KHG_OPT_K1_PGRID] > 0) *pgrid = std::min(*pgrid, ctx->opt[KHG_OPT_K1_PGRID]);
  if (!ctx->k1_next_d) { int rc = dev_alloc(&ctx->k1_next_d, 1); if (rc) return rc; }
  int rc = arena_flush(ctx);
  if (rc) return rc;
  HIPCHK(hipMemsetAsync(ctx->k1_next_d, 0, sizeof(int32_t), ctx->stream));
  return KHG_OK;
}

// K1 on the fp16 matrix cores, one accumulator per chain, transposed decomposition (khg_k1_f16x2s.hip.inc; the default)
static int run_f16x2s(khg_ctx* ctx, khg_model* m, khg_utts* u, const K1Plan& p) {
  K1Set& s = u->k1;
  const bool reachable_only = p.mode != 0, bounded = p.band || p.tail_shift;
  const int KS = p.K;
  int rc = ensure_x32_chunks(ctx, u, p.per, p.order, k1s_nmax(KS), &s.schunks_d, &s.n_schunks, &s.schunk_nmax);
  if (rc) return rc;
  // the set's B fragments: packed once (the exponents depend on the features alone)
  if (!s.xs.d || s.xs.ks != KS || s.xs.ex != p.ex) { rc = k1_pack_planes<K1_PACK_S>(ctx, u, KS, p.ex, "k1s_pack_x", &s.xs); if (rc) return rc; }
  // the model's image for these exponents
  std::vector<int32_t> key(p.ex);
  key.push_back(p.S);
  if (m->wimgs_key != key) {
    rc = m->wimgs_sync.before_pack(ctx->stream);
    if (rc) return rc;
    if (!m->wimgs_d || m->wimgs_tiles < m->ntiles) {
      HIPCHK(hipStreamSynchronize(ctx->stream));     // (the waits on other streams' readers were enqueued above)
      DEVFREE(m->wimgs_d);
      rc = dev_alloc(&m->wimgs_d, (size_t)m->ntiles * k1s_tile_bytes(KS));
      if (rc) return rc;
      m->wimgs_tiles = m->ntiles;
    }
    int32_t* ew_d = nullptr;
    rc = dev_upload(ctx, &ew_d, p.ew);
    if (rc) return rc;
    {
      const K1Kernel<K1_IMG_S> k = k1_kernel<K1_IMG_S>(KS);
      KernelTimer kt(ctx, "k0s_pack_tiles");
      rc = k1_launch(ctx, k.fn, m->ntiles, k.nthr, 0, ctx->stream, m->gconsts_d, m->miv_d, m->iv_d, m->gauss_off_d, m->pdf_tile_off_d, m->tile_pdf_d, m->D, ew_d, std::ldexp(1.0f, p.S), m->wimgs_d);
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);     // the upload of `p.ew` (pageable) has read it, ew_d is free after this
    DEVFREE(ew_d);
    if (rc) return rc;
    if (e != hipSuccess) return khg_set_error(KHG_E_HIP, hipGetErrorString(e));
    rc = m->wimgs_sync.after_pack(ctx->stream);
    if (rc) return rc;
    m->wimgs_key = key;
    u->k1_last[K1L_REPACKED] |= 2;
  }
  // one unit per (utterance, listed pdf): first W tile, number of W tiles, first (and, BAND form, last) needed 32-frame tile
  if (s.sunits_pto != m->pdf_tile_off || s.sunits_reach != p.units_key) {
    DEVFREE(s.sunits_d);
    std::vector<K1sUnit> units(u->pdfs.size());
    std::vector<int32_t> unit_T;                     // tail_shift: the utterance length of every unit
    if (p.tail_shift) {
      unit_T.resize(u->pdfs.size());
      for (int i = 0; i < u->n_utt; ++i)
        for (int64_t k = u->pdf_off[(size_t)i]; k < u->pdf_off[(size_t)i + 1]; ++k) unit_T[(size_t)k] = (int32_t)std::min<int64_t>(INT32_MAX, u->frame_off[(size_t)i + 1] - u->frame_off[(size_t)i]);
    }
    for (size_t k = 0; k < u->pdfs.size(); ++k) {
      const int q = u->pdfs[k];
      const int nt = m->pdf_tile_off[q + 1] - m->pdf_tile_off[q];
      if (nt > (int)K1S_NT_MASK) return khg_set_error(KHG_E_UNSUPPORTED, "khg_loglikes: a pdf of more than 65 504 Gaussians");
      const uint32_t need = reachable_only ? (uint32_t)std::min<int64_t>(255, (int64_t)u->pdf_first[k] / 32) : 0u;
      // last needed tile: 255 = no limit (also a pdf no accepting path reads, last = -1: tile 0 ... nothing past it is computed
      // only when last >= 0; a never-needed pdf keeps last tile 0 so that the kernel's [first, last] range is at most one tile)
      uint32_t last = 255u, shift = 0u;
      if (bounded) {
        const int32_t pl = p.band ? u->pdf_last[k] : unit_T[k] - 1;
        last = pl < 0 ? 0u : (uint32_t)std::min<int32_t>(255, pl / 32);
        // the band ends earlier inside its tile than it starts: tiles that start at its first frame cover it with one tile fewer
        if (pl >= 0 && need < 255u && last < 255u && last > need && (pl % 32) < (u->pdf_first[k] % 32)) shift = (uint32_t)(u->pdf_first[k] % 32);
        if (p.shift_mode == 0) shift = 0u;
        else if (p.shift_mode == 1) shift = (shift >= 16u && (pl % 32) < 16) ? 16u : 0u;
      }
      units[k] = K1sUnit{m->pdf_tile_off[q], (uint32_t)nt | (shift << 11) | (need << 16) | (last << 24)};
    }
    rc = u_upload(ctx, u, &s.sunits_d, units);
    if (rc) return rc;
    { int rs = sync_pageable(ctx); if (rs) return rs; }
    s.sunits_pto = m->pdf_tile_off;
    s.sunits_reach = p.units_key;
  }
  // BAND form: the per-pdf upper bounds the skipped tiles are filled with, indexed by a pdf's first W tile; per parameter version
  if (bounded && !m->ubound_valid) {       // (filled by model_stats with the column maxima; only a stale flag gets here)
    m->wmax.clear();
    rc = model_stats(ctx, m);
    if (rc) return rc;
  }
  K1sArgs a;
  a.xs = s.xs.d; a.utt_xtile_off = s.utt_x32_off_d; a.frame_off = u->frame_off_d; a.chunks = s.schunks_d;
  a.wimg = m->wimgs_d; a.pdf_off = u->pdf_off_d; a.units = s.sunits_d;
  a.ll = u->ll_d; a.ll_off = u->ll_off_d; a.dump = ctx->dump_d; a.err_flag = ctx->err_flag_d;
  a.c1 = std::ldexp(1.44269504088896340736f, -p.S);
  a.inv_scale = std::ldexp(1.0f, -p.S);
  a.mfloor = -3.0e38f / std::max(1.0f, a.c1);
  a.ubound = bounded ? m->ubound_d : nullptr; a.repair_status = nullptr; a.repair_bit = 0; a.stamps = nullptr;
  if (s.n_schunks <= 0) { u->k1_last[K1L_PERSISTENT] = 0; k1_record_grid(u, 0, 0); return KHG_OK; }      // nothing to launch
  rc = m->wimgs_sync.before_read(ctx->stream);
  if (rc) return rc;
  if (p.band) {      // what k1_band_repair launches with
    K1Band& b = s.band;
    if (!b.args) b.args = new K1sArgs();
    *b.args = a; b.model = m; b.ks = KS; b.serial = m->serial; b.version = m->version; b.key = m->wimgs_key;
  }
  const K1Kernel<K1_S_PERSISTENT> kp = p.persistent ? k1_kernel<K1_S_PERSISTENT>(KS) : K1Kernel<K1_S_PERSISTENT>();
  int grid = s.n_schunks;
  if (p.persistent) { rc = k1_persistent_grid(ctx, kp, KS, s.n_schunks, &grid); if (rc) return rc; }
  k1_record_grid(u, s.n_schunks, grid);
  const bool prof = ctx->opt[KHG_OPT_K1_PROF] && p.pack == 1;
  if (prof) { rc = k1_prof_begin(ctx, s.n_schunks, &a); if (rc) return rc; }
  {
    const K1Kernel<K1_S> k = p.persistent ? K1Kernel<K1_S>() : k1_kernel<K1_S>(KS, p.pack);
    KernelTimer kt(ctx, "k1_loglikes");
    if (p.persistent) rc = k1_launch(ctx, kp.fn, grid, kp.nthr, kp.lds, ctx->stream, a, (int)s.n_schunks, ctx->k1_next_d);
    else rc = k1_launch(ctx, k.fn, grid, k.nthr, k.lds, ctx->stream, a);
    if (rc) return rc;
  }
  if (prof) { rc = k1_prof_end(ctx, s.n_schunks, &a, p.persistent, KS); if (rc) return rc; }
  HIPCHK(hipGetLastError());
  return m->wimgs_sync.after_read(ctx->stream);
}

// the pdf lists, the score block and its offsets on the device
static int ensure_lists_on_device(khg_ctx* ctx, khg_utts* u) {
  if (u->pdf_off_d) return KHG_OK;
  int rc = u_upload(ctx, u, &u->pdf_off_d, u->pdf_off);
  if (!rc) rc = u_upload(ctx, u, &u->pdfs_d, u->pdfs);
  if (!rc) rc = u_upload(ctx, u, &u->ll_off_d, u->ll_off);
  if (!rc) rc = u_alloc(u, &u->ll_d, (size_t)u->ll_total);
  return rc;
}

static int loglikes_impl(khg_ctx* ctx, khg_model* m, khg_utts* u, int reach) {
  if (ctx_dead(ctx) || !m || !u) return khg_set_error(KHG_E_ARG, "khg_loglikes: bad arguments");
  { int rf = utts_foreign_ctx(ctx, u, "khg_loglikes"); if (rf) return rf; }
  if (u->pdf_first.size() != u->pdfs.size()) reach = 0;
  K1Plan p;                             // (nothing chosen yet: the record of a call that is refused below)
  p.mode = u->ll_mode = reach != 0;
  k1_record(ctx, u, p);
  if (m->D != u->D) return khg_set_error(KHG_E_RUNTIME, "Dim mismatch: data dim = " + std::to_string(u->D) + " vs. model dim = " + std::to_string(m->D));
  if (u->pdfs_checked_P != m->P) {     // once per (set, model size): 7 M entries at the bench size, 1.5 ms of host time per call
    for (int32_t q : u->pdfs)
      if (q < 0 || q >= m->P) return khg_set_error(KHG_E_RUNTIME, "Likely graph/model mismatch, e.g. using wrong HCLG.fst (pdf-id " + std::to_string(q) + ")");
    u->pdfs_checked_P = m->P;
  }
  int rc = wait_ali(ctx, u);
  if (!rc) rc = ensure_lists_on_device(ctx, u);
  if (rc) return rc;
  std::vector<float> xk;
  if (k1_split_asked(ctx, m, u)) { rc = k1_maxima(ctx, m, u, &xk); if (rc) return rc; }
  p = k1_plan(ctx, m, u, reach, xk);
  k1_record(ctx, u, p);
  u->ll_mode = p.mode;
  switch (p.form) {
    case KHG_K1L_NONE: break;
    case KHG_K1L_WIDE: rc = run_wide(ctx, m, u); break;
    case KHG_K1L_F16X2S: m->xs_ex_seen = p.ex; rc = run_f16x2s(ctx, m, u, p); break;      // (the model follows the exponents it is scored with)
    case KHG_K1L_F16X2: rc = run_f16x2(ctx, m, u, p); break;
    case KHG_K1L_PDF: rc = run_pdf_major(ctx, m, u, p); break;
    default: rc = run_utt_major(ctx, m, u, p); break;
  }
  if (rc) { u->k1_last[K1L_FORM] = KHG_K1L_NONE; return rc; }      // (a call that fails leaves the form at NONE)
  u->ll_valid = true;
  return KHG_OK;
}
extern "C" int khg_utts_pdf_first(const khg_utts* u, int32_t* first) {
  if (!u || !first) return khg_set_error(KHG_E_ARG, "bad arguments");
  if (u->pdf_first.size() != u->pdfs.size()) std::fill(first, first + u->pdfs.size(), 0);
  else std::copy(u->pdf_first.begin(), u->pdf_first.end(), first);
  return KHG_OK;
}
// (the model handle is const in the C-ABI: K1 keeps its fp16 images and their scale exponents in it)
extern "C" int khg_loglikes(khg_ctx* ctx, const khg_model* m, khg_utts* u) { return loglikes_impl(ctx, const_cast<khg_model*>(m), u, 0); }
extern "C" int khg_loglikes_reachable(khg_ctx* ctx, const khg_model* m, khg_utts* u) { return loglikes_impl(ctx, const_cast<khg_model*>(m), u, 1); }
extern "C" int khg_loglikes_band(khg_ctx* ctx, const khg_model* m, khg_utts* u) { return loglikes_impl(ctx, const_cast<khg_model*>(m), u, 2); }
extern "C" int khg_utts_pdf_last(const khg_utts* u, int32_t* last) {
  if (!u || !last) return khg_set_error(KHG_E_ARG, "bad arguments");
  if (u->pdf_last.size() != u->pdfs.size()) std::fill(last, last + u->pdfs.size(), INT32_MAX);
  else std::copy(u->pdf_last.begin(), u->pdf_last.end(), last);
  return KHG_OK;
}
extern "C" int khg_loglikes_layout(const khg_utts* u, int64_t* ll_off, int64_t* total) {
  if (!u) return khg_set_error(KHG_E_ARG, "bad arguments");
  if (ll_off) std::copy(u->ll_off.begin(), u->ll_off.end(), ll_off);
  if (total) *total = u->ll_total;
  return KHG_OK;
}
extern "C" int khg_loglikes_download(khg_ctx* ctx, const khg_utts* u, float* ll) {
  if (ctx_dead(ctx) || !u || !ll) return khg_set_error(KHG_E_ARG, "bad arguments");
  if (!u->ll_valid) return khg_set_error(KHG_E_ARG, "khg_loglikes_download: call khg_loglikes first");
  { int rf = utts_foreign_ctx(ctx, u, "khg_loglikes_download"); if (rf) return rf; }
  int rc = check_err_flag(ctx, "khg_loglikes");
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(ll, u->ll_d, sizeof(float) * (size_t)u->ll_total, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return KHG_OK;
}
extern "C" int khg_loglikes_upload(khg_ctx* ctx, khg_utts* u, const float* ll) {
  if (ctx_dead(ctx) || !u || !ll) return khg_set_error(KHG_E_ARG, "bad arguments");
  { int rf = utts_foreign_ctx(ctx, u, "khg_loglikes_upload"); if (rf) return rf; }
  int rc = wait_ali(ctx, u);
  if (!rc) rc = ensure_lists_on_device(ctx, u);
  if (rc) return rc;
  rc = arena_flush(ctx);      // (staged uploads first: none may land on the score block after this copy)
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(u->ll_d, ll, sizeof(float) * (size_t)u->ll_total, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  u->ll_mode = 0; u->k1.band.model = nullptr;      // the caller's scores: every cell as given
  u->ll_valid = true;
  return KHG_OK;
}

// BAND form: khg_align's repair launch reads the model the scores were computed with -- its fp16 image, its upper bounds -- through
// pointers saved at khg_loglikes_band.  Before anything is launched: that handle must still be alive (by serial, not by address) and
// at the same parameter version; and if only its IMAGE was re-packed since (another set lowered the shared feature exponents), this
// set's planes no longer match it: the set is scored again, in the band form, against the current image.
int k1_band_check(khg_ctx* ctx, khg_utts* u) {
  const K1Band& b = u->k1.band;
  if (u->ll_mode != 2 || !b.args) return KHG_OK;
  khg_model* bm = khg_model_lookup(b.serial);
  if (!bm || bm != b.model || bm->version != b.version) {
    u->ll_valid = false;
    return khg_set_error(KHG_E_ARG, "khg_align: the model these scores were computed with (khg_loglikes_band) was destroyed or updated since; call khg_loglikes_band again");
  }
  if (bm->wimgs_key != b.key) return loglikes_impl(ctx, bm, u, 2);
  return KHG_OK;
}

// BAND form of K1: the utterances the DP could not certify are about to be decoded by the order-faithful kernel, which reads
// every cell a token reaches -- also the ones the band left at their upper bound.  Recompute exactly those utterances (from
// their first needed tile on, no upper limit) on `side`; a workgroup of any other utterance returns at once.
int k1_band_repair(khg_ctx* ctx, khg_utts* u, int32_t* status_d, int repair_bit, hipStream_t side) {
  const K1Band& b = u->k1.band;
  if (u->ll_mode != 2 || !b.model || !b.args || u->k1.n_schunks <= 0) return KHG_OK;
  K1sArgs ra = *b.args;
  ra.repair_status = status_d; ra.repair_bit = repair_bit; ra.stamps = nullptr;
  int rc = b.model->wimgs_sync.before_read(side);
  if (rc) return rc;
  {
    const K1Kernel<K1_S_REPAIR> k = k1_kernel<K1_S_REPAIR>(b.ks);
    KernelTimer kt(ctx, "k1_band_repair", side);
    const unsigned gr = (unsigned)std::min<int64_t>(256, ((int64_t)u->k1.n_schunks + 511) / 512);
    rc = k1_launch(ctx, k.fn, gr, k.nthr, k.lds, side, ra, (int)u->k1.n_schunks);
    if (rc) return rc;
    u->k1_last[K1L_REPAIRED] = 1;
  }
  HIPCHK(hipGetLastError());
  return b.model->wimgs_sync.after_read(side);
}

// khg_utts::k1 when the set's pdf lists are replaced (khg_utts_set_pdf_list): every plan that reads pdf_off / pdfs goes -- the wide and
// utterance-major chunks and the 32-frame chunks (they leave out utterances without pdfs), the walk, the pdf-major plan, the unit
// table; the tile layouts and the feature planes depend on the frames alone and stay
void k1_lists_changed(khg_utts* u) {
  K1Set& s = u->k1;
  DEVFREE(s.chunks_d); DEVFREE(s.wchunks_d);
  DEVFREE(s.tile_off_d); DEVFREE(s.tiles_d); s.tiles_pto.clear(); s.tiles_reach = -1;
  DEVFREE(s.p_ents_d); DEVFREE(s.p_slices_d); s.p_reach = -1;
  DEVFREE(s.bchunks_d); s.n_bchunks = s.bchunk_nt = 0;
  DEVFREE(s.schunks_d); s.n_schunks = s.schunk_nmax = 0;
  DEVFREE(s.sunits_d); s.sunits_pto.clear(); s.sunits_reach = -1;
}
// ... when borrowed device features were rewritten in place (khg_utts_features_changed): the column maxima and the split forms' planes
void k1_features_changed(khg_utts* u) {
  K1Set& s = u->k1;
  s.xmax.clear();
  s.xs.ks = 0; s.xs.ex.clear();
  s.xh.ks = 0; s.xh.ex.clear();
}
// ... and when the set goes (khg_utts_destroy)
void k1_free(khg_utts* u) {
  K1Set& s = u->k1;
  k1_lists_changed(u);
  DEVFREE(s.xpl_d); DEVFREE(s.utt_xtile_off_d); DEVFREE(s.utt_x32_off_d); DEVFREE(s.x32_utt_d);
  DEVFREE(s.xh.d); DEVFREE(s.xh.ex_d); DEVFREE(s.xs.d); DEVFREE(s.xs.ex_d);
  delete s.band.args;
  s.band.args = nullptr; s.band.model = nullptr;
}
