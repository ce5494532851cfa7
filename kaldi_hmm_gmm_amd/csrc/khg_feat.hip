// kaldi_hmm_gmm_amd/csrc/khg_feat.hip -- the feature stage in front of the acoustic model (compute-cmvn-stats, apply-cmvn, add-deltas;
// DESIGN.md 7p): the per-speaker statistics handle (khg_cmvn_stats), its accumulation from a set's resident rows and the fused
// normalise-and-delta of those rows.  The normaliser (khg_cmvn_compute) and the coefficient tables (khg_delta_scales) are host code
// and live in khg_host_feat.cpp.  Also the waveform front end in front of that stage (compute-mfcc-feats, compute-fbank-feats; DESIGN.md
// 7q): the resident tables (khg_frontend) and khg_frontend_compute; its options and tables are host code in khg_host_feat.cpp too.
// gfx950 only.
#include "khg_internal.hpp"

#include <cfloat>

#include "khg_feat_stats.hip.inc"
#include "khg_feat_tile.hip.inc"
#include "khg_feat_wave.hip.inc"

struct khg_cmvn_stats {
  khg_ctx* ctx = nullptr;
  int32_t S = 0, D = 0;
  int64_t SZ = 0;                    // doubles of the block: [S][2][D + 1]
  double* buf_d = nullptr;           // [SZ]
  double* call_d = nullptr;          // [SZ] the sums of the call in progress
  // scratch of the accumulation (grown on demand, kept)
  int64_t chunk_frames = int64_t(1) << 24;
  double* part_d = nullptr; size_t part_cap = 0;
  CvSeg* segs_d = nullptr; size_t segs_cap = 0;
  CvItem* items_d = nullptr; size_t items_cap = 0;
  CvRun* runs_d = nullptr; size_t runs_cap = 0;
  int32_t n_chunks_last = 0;
};

static inline int cv_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(4096, (n + 255) / 256)); }

template <class T>
static int cv_grow(T** p, size_t* cap, size_t need) {
  if (need <= *cap && *p) return KHG_OK;
  DEVFREE(*p); *cap = 0;
  int rc = dev_alloc(p, need);
  if (rc) return rc;
  *cap = need;
  return KHG_OK;
}

extern "C" int khg_cmvn_stats_create(khg_ctx* ctx, int32_t n_spk, int32_t dim, khg_cmvn_stats** out) {
  if (ctx_dead(ctx) || !out || n_spk < 1 || dim < 1) return khg_set_error(KHG_E_ARG, "khg_cmvn_stats_create: bad arguments");
  khg_cmvn_stats* s = new khg_cmvn_stats();
  s->ctx = ctx; s->S = n_spk; s->D = dim; s->SZ = (int64_t)n_spk * 2 * ((int64_t)dim + 1);
  int rc = dev_alloc(&s->buf_d, (size_t)s->SZ);
  if (!rc) rc = dev_alloc(&s->call_d, (size_t)s->SZ);
  if (rc) { (void)khg_cmvn_stats_destroy(s); return rc; }
  *out = s;
  return khg_cmvn_stats_zero(ctx, s);
}
extern "C" int khg_cmvn_stats_destroy(khg_cmvn_stats* s) {
  if (!s) return KHG_OK;
  DEVFREE(s->buf_d); DEVFREE(s->call_d); DEVFREE(s->part_d); DEVFREE(s->segs_d); DEVFREE(s->items_d); DEVFREE(s->runs_d);
  delete s;
  return KHG_OK;
}
extern "C" int khg_cmvn_stats_zero(khg_ctx* ctx, khg_cmvn_stats* s) {
  if (ctx_dead(ctx) || !s || s->ctx != ctx) return khg_set_error(KHG_E_ARG, "khg_cmvn_stats_zero: bad arguments");
  HIPCHK(hipMemsetAsync(s->buf_d, 0, sizeof(double) * (size_t)s->SZ, ctx->stream));
  return KHG_OK;
}
extern "C" int khg_cmvn_stats_set_chunk_frames(khg_cmvn_stats* s, int64_t frames) {
  if (!s || frames < 1) return khg_set_error(KHG_E_ARG, "khg_cmvn_stats_set_chunk_frames: bad arguments");
  s->chunk_frames = std::min<int64_t>(frames, int64_t(1) << 24);
  return KHG_OK;
}
extern "C" int khg_cmvn_stats_num_chunks(const khg_cmvn_stats* s, int32_t* n) {
  if (!s || !n) return khg_set_error(KHG_E_ARG, "khg_cmvn_stats_num_chunks: bad arguments");
  *n = s->n_chunks_last;
  return KHG_OK;
}
extern "C" int khg_cmvn_stats_download(khg_ctx* ctx, const khg_cmvn_stats* s, double* stats_h) {
  if (ctx_dead(ctx) || !s || s->ctx != ctx || !stats_h) return khg_set_error(KHG_E_ARG, "khg_cmvn_stats_download: bad arguments");
  { int rc = check_err_flag(ctx, "khg_acc_cmvn_stats"); if (rc) return rc; }
  HIPCHK(hipMemcpyAsync(stats_h, s->buf_d, sizeof(double) * (size_t)s->SZ, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return KHG_OK;
}
extern "C" int khg_cmvn_stats_upload(khg_ctx* ctx, khg_cmvn_stats* s, const double* stats_h) {
  if (ctx_dead(ctx) || !s || s->ctx != ctx || !stats_h) return khg_set_error(KHG_E_ARG, "khg_cmvn_stats_upload: bad arguments");
  HIPCHK(hipMemcpyAsync(s->buf_d, stats_h, sizeof(double) * (size_t)s->SZ, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return KHG_OK;
}
extern "C" int khg_cmvn_stats_add(khg_ctx* ctx, khg_cmvn_stats* dst, float scale, const khg_cmvn_stats* src) {
  if (ctx_dead(ctx) || !dst || !src) return khg_set_error(KHG_E_ARG, "khg_cmvn_stats_add: bad arguments");
  if (!std::isfinite(scale)) return khg_set_error(KHG_E_ARG, "khg_cmvn_stats_add: the scale is not finite");
  if (dst->ctx != ctx || src->ctx != ctx) return khg_set_error(KHG_E_ARG, "khg_cmvn_stats_add: a handle of another context");
  if (dst->S != src->S || dst->D != src->D) return khg_set_error(KHG_E_ARG, "khg_cmvn_stats_add: the two handles differ in speakers or dimension");
  if (dst == src) return khg_set_error(KHG_E_ARG, "khg_cmvn_stats_add: dst and src are the same handle");
  KernelTimer kt(ctx, "k_cmvn_axpy");
  KHG_LAUNCH(ctx, k_cmvn_axpy, dim3(cv_grid(dst->SZ)), dim3(256), 0, ctx->stream, dst->buf_d, src->buf_d, (double)scale, dst->SZ);
  HIPCHK(hipGetLastError());
  return KHG_OK;
}

// compute-cmvn-stats: every check on the host first (the handle keeps its bits), then the plan -- per speaker its utterances in set
// order, cut into slices of CV_SLICE frames, chunks of whole slices -- and per chunk k_cmvn_slice + k_cmvn_reduce on the context's stream.
extern "C" int khg_acc_cmvn_stats(khg_ctx* ctx, khg_utts* u, const int32_t* utt2spk_h, khg_cmvn_stats* st) {
  const char* name = "khg_acc_cmvn_stats";
  const std::string who = std::string(name) + ": ";
  if (ctx_dead(ctx) || !u || !utt2spk_h || !st) return khg_set_error(KHG_E_ARG, who + "bad arguments");
  { int rf = utts_foreign_ctx(ctx, u, name); if (rf) return rf; }
  if (u->ctx != ctx || st->ctx != ctx) return khg_set_error(KHG_E_ARG, who + "a handle of another context");
  if (st->D != u->D) return khg_set_error(KHG_E_ARG, who + "the statistics are of dimension " + std::to_string(st->D) + ", the features of " + std::to_string(u->D));
  for (int i = 0; i < u->n_utt; ++i)
    if (utt2spk_h[i] >= st->S)
      return khg_set_error(KHG_E_ARG, who + "utterance " + std::to_string(i) + " belongs to speaker " + std::to_string(utt2spk_h[i]) + " of " + std::to_string(st->S));
  st->n_chunks_last = 0;

  // ---- the plan ----
  const int D = st->D, S = st->S;
  const int64_t CI = std::max<int64_t>(1, st->chunk_frames / CV_SLICE);
  struct Chunk { size_t item0, item1, run0, run1; };
  std::vector<CvSeg> segs; std::vector<CvItem> items; std::vector<CvRun> runs; std::vector<Chunk> chunks;
  {
    std::vector<int64_t> first((size_t)S + 1, 0);           // the speakers' utterances with frames, in set order (a counting sort)
    for (int i = 0; i < u->n_utt; ++i)
      if (utt2spk_h[i] >= 0 && u->frame_off[(size_t)i + 1] > u->frame_off[(size_t)i]) first[(size_t)utt2spk_h[i] + 1]++;
    for (int s = 0; s < S; ++s) first[(size_t)s + 1] += first[(size_t)s];
    std::vector<int32_t> list((size_t)first[(size_t)S]);
    {
      std::vector<int64_t> at(first.begin(), first.end() - 1);
      for (int i = 0; i < u->n_utt; ++i)
        if (utt2spk_h[i] >= 0 && u->frame_off[(size_t)i + 1] > u->frame_off[(size_t)i]) list[(size_t)at[(size_t)utt2spk_h[i]]++] = i;
    }
    Chunk cur{0, 0, 0, 0};
    auto close_chunk = [&] {
      cur.item1 = items.size(); cur.run1 = runs.size();
      if (cur.item1 > cur.item0) chunks.push_back(cur);
      cur = Chunk{items.size(), items.size(), runs.size(), runs.size()};
    };
    for (int s = 0; s < S; ++s) {
      int64_t open = -1;                                    // the speaker's slice that still has room
      for (int64_t k = first[(size_t)s]; k < first[(size_t)s + 1]; ++k) {
        const int32_t ui = list[(size_t)k];
        const int64_t f0 = u->frame_off[(size_t)ui], T = u->frame_off[(size_t)ui + 1] - f0;
        int64_t used = 0;
        while (used < T) {
          if (open < 0 || items[(size_t)open].n == CV_SLICE) {
            if ((int64_t)(items.size() - cur.item0) >= CI) close_chunk();
            open = (int64_t)items.size();
            const int32_t slot = (int32_t)(items.size() - cur.item0);
            items.push_back(CvItem{(int32_t)segs.size(), 0, 0, slot});
            if (runs.size() > cur.run0 && runs.back().spk == s) runs.back().nslot++;
            else runs.push_back(CvRun{s, slot, 1, 0, 0.0});
          }
          CvItem& it = items[(size_t)open];
          const int32_t take = (int32_t)std::min<int64_t>(T - used, CV_SLICE - it.n);
          segs.push_back(CvSeg{f0 + used, take, it.n});
          it.nseg++; it.n += take; runs.back().frames += (double)take; used += take;
        }
      }
    }
    close_chunk();
  }
  if (chunks.empty()) return KHG_OK;
  if (segs.size() >= (size_t)INT_MAX) return khg_set_error(KHG_E_UNSUPPORTED, who + "2^31 - 1 or more row segments");

  int rc = arena_flush(ctx);
  if (rc) return rc;
  size_t maxi = 0;
  for (const Chunk& c : chunks) maxi = std::max(maxi, c.item1 - c.item0);
  rc = cv_grow(&st->part_d, &st->part_cap, maxi * 2 * (size_t)D);
  if (!rc) rc = cv_grow(&st->segs_d, &st->segs_cap, segs.size());
  if (!rc) rc = cv_grow(&st->items_d, &st->items_cap, items.size());
  if (!rc) rc = cv_grow(&st->runs_d, &st->runs_cap, runs.size());
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(st->segs_d, segs.data(), sizeof(CvSeg) * segs.size(), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(st->items_d, items.data(), sizeof(CvItem) * items.size(), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(st->runs_d, runs.data(), sizeof(CvRun) * runs.size(), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));                // the plan is up, its host vectors are free again
  HIPCHK(hipMemsetAsync(st->call_d, 0, sizeof(double) * (size_t)st->SZ, ctx->stream));
  for (const Chunk& c : chunks) {
    const int nit = (int)(c.item1 - c.item0), nrun = (int)(c.run1 - c.run0);
    {
      KernelTimer kt(ctx, "k_cmvn_slice");
      KHG_LAUNCH(ctx, k_cmvn_slice, dim3((unsigned)nit), dim3(256), 0, ctx->stream, u->feats_d, D, st->segs_d, st->items_d + c.item0, st->part_d);
      HIPCHK(hipGetLastError());
    }
    {
      KernelTimer kt(ctx, "k_cmvn_reduce");
      KHG_LAUNCH(ctx, k_cmvn_reduce, dim3(cv_grid((int64_t)nrun * 2 * (D + 1))), dim3(256), 0, ctx->stream, st->runs_d + c.run0, nrun, st->part_d, st->call_d, D);
      HIPCHK(hipGetLastError());
    }
  }
  {
    KernelTimer kt(ctx, "k_cmvn_axpy");
    KHG_LAUNCH(ctx, k_cmvn_axpy, dim3(cv_grid(st->SZ)), dim3(256), 0, ctx->stream, st->buf_d, st->call_d, 1.0, st->SZ);
    HIPCHK(hipGetLastError());
  }
  st->n_chunks_last = (int32_t)chunks.size();
  return KHG_OK;
}

// apply-cmvn (apply: order 0, in place when out_d is NULL) and add-deltas: the checks, the 64-row items, one launch of k_feat_cmvn_deltas
static int feat_tile(const char* name, khg_ctx* ctx, khg_utts* u, int32_t order, int32_t window, int32_t n_spk, const int32_t* utt2spk_h,
                     const float* norm_h, const int32_t* status_h, float* out_d, bool apply) {
  const std::string who = std::string(name) + ": ";
  if (ctx_dead(ctx) || !u || (!apply && !out_d) || (apply && !norm_h)) return khg_set_error(KHG_E_ARG, who + "bad arguments");
  if (norm_h && (!utt2spk_h || n_spk < 0)) return khg_set_error(KHG_E_ARG, who + "bad arguments (a normaliser needs utt2spk and n_spk)");
  { int rf = utts_foreign_ctx(ctx, u, name); if (rf) return rf; }
  if (u->ctx != ctx) return khg_set_error(KHG_E_ARG, who + "a handle of another context");
  if (order < 0 || window < 1) return khg_set_error(KHG_E_ARG, who + "order must be >= 0 and window >= 1");
  if (norm_h)
    for (int i = 0; i < u->n_utt; ++i)
      if (utt2spk_h[i] >= n_spk)
        return khg_set_error(KHG_E_ARG, who + "utterance " + std::to_string(i) + " belongs to speaker " + std::to_string(utt2spk_h[i]) + " of " + std::to_string(n_spk));
  const int D = u->D;
  const int64_t H = (int64_t)order * window, nsc = ((int64_t)order + 1) + (int64_t)window * order * ((int64_t)order + 1);
  const int64_t lds = apply ? 0 : 4 * (FT2_ROWS + 2 * H) * D;
  if (lds > KHG_FEAT_TILE_LDS_BYTES)
    return khg_set_error(KHG_E_UNSUPPORTED, who + "order " + std::to_string(order) + " at window " + std::to_string(window) + " and dim " + std::to_string(D) + " needs " +
                                                std::to_string(lds) + " bytes of LDS for the rows and their halo, above KHG_FEAT_TILE_LDS_BYTES (" +
                                                std::to_string(KHG_FEAT_TILE_LDS_BYTES) + ")");
  if (u->N == 0) return KHG_OK;
  const bool in_place = apply && !out_d;
  std::vector<Ft2Item> items;
  for (int i = 0; i < u->n_utt; ++i) {
    int32_t spk = norm_h ? utt2spk_h[i] : -1;
    if (spk >= 0 && status_h && status_h[spk] != KHG_CMVN_OK) spk = -1;
    if (spk < 0) spk = -1;
    if (in_place && spk < 0) continue;                      // the rows stay as they are
    const int64_t f0 = u->frame_off[(size_t)i], f1 = u->frame_off[(size_t)i + 1];
    for (int64_t r = f0; r < f1; r += FT2_ROWS) items.push_back(Ft2Item{r, (int32_t)std::min<int64_t>(FT2_ROWS, f1 - r), spk, f0, f1 - 1});
  }
  if (items.size() >= (size_t)INT_MAX) return khg_set_error(KHG_E_UNSUPPORTED, who + "too many rows");
  if (items.empty()) return KHG_OK;
  std::vector<float> scales((size_t)nsc);
  if (!apply) { int rs = khg_delta_scales(order, window, scales.data()); if (rs) return rs; }
  int rc = arena_flush(ctx);
  if (rc) return rc;
  Ft2Item* items_d = nullptr; float* norm_d = nullptr; float* scales_d = nullptr;
  auto cleanup = [&] { DEVFREE(items_d); DEVFREE(norm_d); DEVFREE(scales_d); };
  rc = dev_alloc(&items_d, items.size());
  if (!rc && norm_h) rc = dev_alloc(&norm_d, (size_t)n_spk * 2 * D);
  if (!rc && !apply) rc = dev_alloc(&scales_d, scales.size());
  if (rc) { cleanup(); return rc; }
  hipError_t e = hipMemcpyAsync(items_d, items.data(), sizeof(Ft2Item) * items.size(), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess && norm_h && n_spk > 0) e = hipMemcpyAsync(norm_d, norm_h, sizeof(float) * (size_t)n_spk * 2 * D, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess && !apply) e = hipMemcpyAsync(scales_d, scales.data(), sizeof(float) * scales.size(), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess && lds > 48 * 1024) e = hipFuncSetAttribute((const void*)k_feat_cmvn_deltas, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) { cleanup(); return khg_set_error(KHG_E_HIP, who + hipGetErrorString(e)); }
  float* dst = out_d ? out_d : const_cast<float*>(u->feats_d);
  {
    KernelTimer kt(ctx, apply ? "k_feat_cmvn" : "k_feat_cmvn_deltas");
    KHG_LAUNCH(ctx, k_feat_cmvn_deltas, dim3((unsigned)items.size()), dim3(256), (size_t)lds, ctx->stream, items_d, norm_d, scales_d, u->feats_d, dst, D, order, window,
               apply ? 1 : 0);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);     // the temporaries and the caller's host arrays are free again
  cleanup();
  if (e != hipSuccess) return khg_set_error(KHG_E_HIP, who + hipGetErrorString(e));
  if (in_place) return khg_utts_features_changed(u);
  return KHG_OK;
}

extern "C" int khg_utts_apply_cmvn(khg_ctx* ctx, khg_utts* u, int32_t n_spk, const int32_t* utt2spk_h, const float* norm_h, const int32_t* status_h,
                                   float* out_d) {
  return feat_tile("khg_utts_apply_cmvn", ctx, u, 0, 1, n_spk, utt2spk_h, norm_h, status_h, out_d, true);
}
extern "C" int khg_utts_add_deltas(khg_ctx* ctx, khg_utts* u, int32_t order, int32_t window, int32_t n_spk, const int32_t* utt2spk_h, const float* norm_h,
                                   const int32_t* status_h, float* out_d) {
  return feat_tile("khg_utts_add_deltas", ctx, u, order, window, n_spk, utt2spk_h, norm_h, status_h, out_d, false);
}

// ---- the waveform front end: the tables resident on a handle, and compute-mfcc-feats / compute-fbank-feats ----
struct khg_frontend {
  khg_ctx* ctx = nullptr;
  khg_frontend_opts opts;
  FeParams p;
  size_t lds_bytes = 0;
  float* tab_d = nullptr;            // window [L], twiddles [N], mel weights [n_w]
  int32_t* runs_d = nullptr;         // [3][B]: first bin, length, first weight
  float* dctT_d = nullptr;           // [B][C]
  float* lifter_d = nullptr;         // [C]
};

extern "C" int khg_frontend_create(khg_ctx* ctx, const khg_frontend_opts* o, khg_frontend** out) {
  const std::string who = "khg_frontend_create: ";
  if (ctx_dead(ctx) || !o || !out) return khg_set_error(KHG_E_ARG, who + "bad arguments");
  int32_t d[8];
  int rc = khg_frontend_dims(o, d);
  if (rc) return rc;
  FeParams p{};
  p.L = d[0]; p.S = d[1]; p.N = d[2]; p.B = d[3]; p.C = d[4]; p.out_dim = d[5]; p.n_w = d[6];
  p.logM = 0;
  while ((2 << p.logM) < p.N) p.logM++;
  p.mfcc = o->kind == KHG_FE_MFCC; p.remove_dc = o->remove_dc_offset != 0; p.snip = o->snip_edges != 0; p.use_energy = o->use_energy != 0;
  p.raw_energy = o->raw_energy != 0; p.use_log = p.mfcc || o->use_log_fbank; p.use_power = p.mfcc || o->use_power; p.i16 = 0;
  p.has_floor = o->energy_floor > 0.0f; p.preemph = o->preemph_coeff; p.inv_L = (float)(1.0 / p.L);
  p.log_floor = p.has_floor ? (float)std::log((double)o->energy_floor) : 0.0f;
  const int64_t lds = 4 * fe_lds_floats(p);
  if (lds > KHG_FEAT_TILE_LDS_BYTES)
    return khg_set_error(KHG_E_UNSUPPORTED, who + "frame_shift_ms and frame_length_ms need " + std::to_string(lds) + " bytes of LDS for " + std::to_string(FE_TILE) +
                                                " frames and the tables, above KHG_FEAT_TILE_LDS_BYTES (" + std::to_string(KHG_FEAT_TILE_LDS_BYTES) + ")");
  std::vector<float> tab((size_t)p.L + p.N + p.n_w), dct((size_t)p.C * p.B), dctT((size_t)p.C * p.B), lifter((size_t)p.C);
  std::vector<int32_t> runs((size_t)3 * p.B);
  rc = khg_frontend_tables(o, tab.data(), runs.data(), runs.data() + p.B, tab.data() + p.L + p.N, dct.data(), lifter.data(), tab.data() + p.L);
  if (rc) return rc;
  for (int b = 0, at = 0; b < p.B; ++b) { runs[(size_t)2 * p.B + b] = at; at += runs[(size_t)p.B + b]; }
  for (int c = 0; c < p.C; ++c)
    for (int b = 0; b < p.B; ++b) dctT[(size_t)b * p.C + c] = dct[(size_t)c * p.B + b];
  for (int b = 0; b < p.B; ++b)                              // the kernel walks pw[off .. off + len): inside the N / 2 bins
    if (runs[b] < 0 || runs[(size_t)p.B + b] < 0 || runs[b] + runs[(size_t)p.B + b] > p.N / 2) return khg_set_error(KHG_E_RUNTIME, who + "a mel filter leaves the spectrum");
  khg_frontend* fe = new khg_frontend();
  fe->ctx = ctx; fe->opts = *o; fe->p = p; fe->lds_bytes = (size_t)lds;
  rc = arena_flush(ctx);
  if (!rc) rc = dev_alloc(&fe->tab_d, tab.size());
  if (!rc) rc = dev_alloc(&fe->runs_d, runs.size());
  if (!rc) rc = dev_alloc(&fe->dctT_d, dctT.size());
  if (!rc) rc = dev_alloc(&fe->lifter_d, lifter.size());
  hipError_t e = hipSuccess;
  if (!rc) {
    e = hipMemcpyAsync(fe->tab_d, tab.data(), sizeof(float) * tab.size(), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(fe->runs_d, runs.data(), sizeof(int32_t) * runs.size(), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && p.C) e = hipMemcpyAsync(fe->dctT_d, dctT.data(), sizeof(float) * dctT.size(), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && p.C) e = hipMemcpyAsync(fe->lifter_d, lifter.data(), sizeof(float) * lifter.size(), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  }
  if (rc || e != hipSuccess) {
    (void)khg_frontend_destroy(fe);
    return rc ? rc : khg_set_error(KHG_E_HIP, who + hipGetErrorString(e));
  }
  *out = fe;
  return KHG_OK;
}
extern "C" int khg_frontend_destroy(khg_frontend* fe) {
  if (!fe) return KHG_OK;
  DEVFREE(fe->tab_d); DEVFREE(fe->runs_d); DEVFREE(fe->dctT_d); DEVFREE(fe->lifter_d);
  delete fe;
  return KHG_OK;
}

extern "C" int khg_frontend_compute(khg_ctx* ctx, khg_frontend* fe, int32_t n_utt, const int64_t* sample_off_h, const void* samples_h, const void* samples_d,
                                    int32_t sample_type, int64_t* frame_off_h, float* out_d) {
  const std::string who = "khg_frontend_compute: ";
  if (ctx_dead(ctx) || !fe || n_utt < 0 || !sample_off_h || !frame_off_h) return khg_set_error(KHG_E_ARG, who + "bad arguments");
  if (fe->ctx != ctx) return khg_set_error(KHG_E_ARG, who + "a handle of another context");
  if (sample_type != KHG_WAVE_F32 && sample_type != KHG_WAVE_I16) return khg_set_error(KHG_E_ARG, who + "sample_type must be KHG_WAVE_F32 or KHG_WAVE_I16");
  if (sample_off_h[0] < 0) return khg_set_error(KHG_E_ARG, who + "sample_off must start at or above 0");
  for (int i = 0; i < n_utt; ++i)
    if (sample_off_h[i + 1] < sample_off_h[i]) return khg_set_error(KHG_E_ARG, who + "sample_off must not descend (utterance " + std::to_string(i) + ")");
  const int64_t n_samples = sample_off_h[n_utt];
  FeParams p = fe->p;
  p.i16 = sample_type == KHG_WAVE_I16;
  std::vector<int64_t> fo((size_t)n_utt + 1, 0);
  for (int i = 0; i < n_utt; ++i) {                          // khg_frontend_num_frames' rule on the handle's own L, S and snip_edges
    const int64_t n = sample_off_h[i + 1] - sample_off_h[i];
    const int64_t T = p.snip ? (n < p.L ? 0 : 1 + (n - p.L) / p.S) : (n + p.S / 2) / p.S;
    if (T > INT_MAX - FE_TILE) return khg_set_error(KHG_E_UNSUPPORTED, who + "utterance " + std::to_string(i) + " has 2^31 or more frames");
    fo[(size_t)i + 1] = fo[(size_t)i] + T;
  }
  if (out_d && fo[(size_t)n_utt] > 0 && n_samples > 0 && ((samples_h != nullptr) == (samples_d != nullptr)))
    return khg_set_error(KHG_E_ARG, who + "exactly one of samples_h and samples_d must be given");
  for (int i = 0; i <= n_utt; ++i) frame_off_h[i] = fo[(size_t)i];
  if (!out_d || fo[(size_t)n_utt] == 0) return KHG_OK;
  std::vector<FeItem> items;
  for (int i = 0; i < n_utt; ++i) {
    const int64_t T = fo[(size_t)i + 1] - fo[(size_t)i];
    for (int64_t t = 0; t < T; t += FE_TILE)
      items.push_back(FeItem{sample_off_h[i], sample_off_h[i + 1] - sample_off_h[i], fo[(size_t)i] + t, (int32_t)t, (int32_t)std::min<int64_t>(FE_TILE, T - t)});
  }
  if (items.size() >= (size_t)INT_MAX) return khg_set_error(KHG_E_UNSUPPORTED, who + "too many frames in one call");
  int rc = arena_flush(ctx);
  if (rc) return rc;
  FeItem* items_d = nullptr; char* up_d = nullptr;
  auto cleanup = [&] { DEVFREE(items_d); DEVFREE(up_d); };
  const size_t ssz = p.i16 ? sizeof(int16_t) : sizeof(float);
  rc = dev_alloc(&items_d, items.size());
  if (!rc && samples_h) rc = dev_alloc(&up_d, (size_t)n_samples * ssz);
  if (rc) { cleanup(); return rc; }
  hipError_t e = hipMemcpyAsync(items_d, items.data(), sizeof(FeItem) * items.size(), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess && samples_h) e = hipMemcpyAsync(up_d, samples_h, (size_t)n_samples * ssz, hipMemcpyHostToDevice, ctx->stream);
  // a per-function attribute that another handle may have set lower: set for this launch, as khg_utts_add_deltas does
  if (e == hipSuccess && fe->lds_bytes > 48 * 1024) e = hipFuncSetAttribute((const void*)k_fe_wave, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fe->lds_bytes);
  if (e != hipSuccess) { cleanup(); return khg_set_error(KHG_E_HIP, who + hipGetErrorString(e)); }
  {
    KernelTimer kt(ctx, "k_fe_wave");
    KHG_LAUNCH(ctx, k_fe_wave, dim3((unsigned)items.size()), dim3(256), fe->lds_bytes, ctx->stream, items_d, p, samples_h ? (const void*)up_d : samples_d, fe->tab_d,
               fe->runs_d, fe->dctT_d, fe->lifter_d, out_d);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);     // the temporaries and the caller's host arrays are free again
  cleanup();
  if (e != hipSuccess) return khg_set_error(KHG_E_HIP, who + hipGetErrorString(e));
  return KHG_OK;
}
