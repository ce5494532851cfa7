// kaldi_hmm_gmm_amd/csrc/khg_fmllr.hip -- fMLLR speaker adaptation (gmm-est-fmllr / transform-feats): the per-speaker
// statistics handle (khg_fmllr_stats), their accumulation from posteriors resident on the device and the feature transform.  The
// estimate's host form (khg_fmllr_compute) lives in khg_host.cpp.  MLLT (gmm-acc-mllt / gmm-transform-means) shares the
// accumulation's plan and per-entry stage and lives at the end of this unit; its estimate (khg_mllt_compute) is in khg_host.cpp too.
// gfx950 only.
#include "khg_internal.hpp"

#include <hipcub/hipcub.hpp>   // DeviceRadixSort: the stable (pdf, entry) sort of the per-entry stage, as K3's bucketing

#include "khg_fmllr_stats.hip.inc"
#include "khg_fmllr_entry.hip.inc"
#include "khg_fmllr_transform.hip.inc"
#include "khg_fmllr_estimate.hip.inc"
#include "khg_mllt_stats.hip.inc"

struct khg_fmllr_stats {
  khg_ctx* ctx = nullptr;
  int32_t S = 0, D = 0;
  int64_t SZ = 0;                    // doubles per speaker: K | G | beta
  double* buf_d = nullptr;           // [S][SZ]
  double* call_d = nullptr;          // [S][SZ] the sums of the call in progress (made by the first accumulation)
  // scratch of the accumulation, bounded by chunk_frames (grown on demand, kept)
  int64_t chunk_frames = int64_t(1) << 18;
  int32_t* pos_row_d = nullptr; float *a_d = nullptr, *b_d = nullptr; double* c_d = nullptr; size_t pos_cap = 0;
  double* part_d = nullptr; size_t part_cap = 0;       // slots
  int32_t *cnt_d = nullptr, *ent_id_d = nullptr; float *ea_d = nullptr, *eb_d = nullptr, *ec_d = nullptr; size_t cnt_cap = 0, ent_cap = 0;   // the per-entry stage
  int32_t* row_first_d = nullptr; size_t row_cap = 0;
  FmSeg* segs_d = nullptr; size_t segs_cap = 0;
  FmItem* items_d = nullptr; size_t items_cap = 0;
  FmRun* runs_d = nullptr; size_t runs_cap = 0;
  int32_t n_chunks_last = 0;
};

static inline int64_t fm_block_size(int D) { const int64_t D1 = D + 1; return (int64_t)D * D1 + (int64_t)D * (D1 * (D1 + 1) / 2) + 1; }
static inline int fm_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(4096, (n + 255) / 256)); }

extern "C" int khg_fmllr_stats_create(khg_ctx* ctx, int32_t n_spk, int32_t dim, khg_fmllr_stats** out) {
  if (ctx_dead(ctx) || !out || n_spk < 1 || dim < 1) return khg_set_error(KHG_E_ARG, "khg_fmllr_stats_create: bad arguments");
  if (dim > KHG_FMLLR_MAX_DIM)
    return khg_set_error(KHG_E_UNSUPPORTED, "khg_fmllr_stats_create: dim " + std::to_string(dim) + " is above KHG_FMLLR_MAX_DIM");
  khg_fmllr_stats* s = new khg_fmllr_stats();
  s->ctx = ctx; s->S = n_spk; s->D = dim; s->SZ = fm_block_size(dim);
  int rc = dev_alloc(&s->buf_d, (size_t)s->S * (size_t)s->SZ);
  if (rc) { delete s; return rc; }
  *out = s;
  return khg_fmllr_stats_zero(ctx, s);
}
extern "C" int khg_fmllr_stats_destroy(khg_fmllr_stats* s) {
  if (!s) return KHG_OK;
  DEVFREE(s->buf_d); DEVFREE(s->call_d); DEVFREE(s->pos_row_d); DEVFREE(s->a_d); DEVFREE(s->b_d); DEVFREE(s->c_d); DEVFREE(s->part_d);
  DEVFREE(s->cnt_d); DEVFREE(s->ent_id_d); DEVFREE(s->ea_d); DEVFREE(s->eb_d); DEVFREE(s->ec_d);
  DEVFREE(s->row_first_d); DEVFREE(s->segs_d); DEVFREE(s->items_d); DEVFREE(s->runs_d);
  delete s;
  return KHG_OK;
}
extern "C" int khg_fmllr_stats_zero(khg_ctx* ctx, khg_fmllr_stats* s) {
  if (ctx_dead(ctx) || !s || s->ctx != ctx) return khg_set_error(KHG_E_ARG, "khg_fmllr_stats_zero: bad arguments");
  HIPCHK(hipMemsetAsync(s->buf_d, 0, sizeof(double) * (size_t)s->S * (size_t)s->SZ, ctx->stream));
  return KHG_OK;
}
extern "C" int khg_fmllr_stats_set_chunk_frames(khg_fmllr_stats* s, int64_t frames) {
  if (!s || frames < 1) return khg_set_error(KHG_E_ARG, "khg_fmllr_stats_set_chunk_frames: bad arguments");
  s->chunk_frames = std::min<int64_t>(frames, int64_t(1) << 24);
  return KHG_OK;
}
extern "C" int khg_fmllr_stats_num_chunks(const khg_fmllr_stats* s, int32_t* n) {
  if (!s || !n) return khg_set_error(KHG_E_ARG, "khg_fmllr_stats_num_chunks: bad arguments");
  *n = s->n_chunks_last;
  return KHG_OK;
}
// the block on the host: one speaker after the other, split into the three arrays of the header
extern "C" int khg_fmllr_stats_download(khg_ctx* ctx, const khg_fmllr_stats* s, double* beta_h, double* K_h, double* G_h) {
  if (ctx_dead(ctx) || !s || s->ctx != ctx) return khg_set_error(KHG_E_ARG, "khg_fmllr_stats_download: bad arguments");
  { int rc = check_err_flag(ctx, "khg_acc_fmllr_stats_post"); if (rc) return rc; }
  std::vector<double> h((size_t)s->S * (size_t)s->SZ);
  HIPCHK(hipMemcpyAsync(h.data(), s->buf_d, sizeof(double) * h.size(), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  const size_t nk = (size_t)s->D * (s->D + 1), ng = (size_t)s->SZ - nk - 1;
  for (int i = 0; i < s->S; ++i) {
    const double* b = h.data() + (size_t)i * (size_t)s->SZ;
    if (K_h) memcpy(K_h + (size_t)i * nk, b, sizeof(double) * nk);
    if (G_h) memcpy(G_h + (size_t)i * ng, b + nk, sizeof(double) * ng);
    if (beta_h) beta_h[i] = b[nk + ng];
  }
  return KHG_OK;
}
extern "C" int khg_fmllr_stats_upload(khg_ctx* ctx, khg_fmllr_stats* s, const double* beta_h, const double* K_h, const double* G_h) {
  if (ctx_dead(ctx) || !s || s->ctx != ctx || !beta_h || !K_h || !G_h) return khg_set_error(KHG_E_ARG, "khg_fmllr_stats_upload: bad arguments");
  std::vector<double> h((size_t)s->S * (size_t)s->SZ);
  const size_t nk = (size_t)s->D * (s->D + 1), ng = (size_t)s->SZ - nk - 1;
  for (int i = 0; i < s->S; ++i) {
    double* b = h.data() + (size_t)i * (size_t)s->SZ;
    memcpy(b, K_h + (size_t)i * nk, sizeof(double) * nk);
    memcpy(b + nk, G_h + (size_t)i * ng, sizeof(double) * ng);
    b[nk + ng] = beta_h[i];
  }
  HIPCHK(hipMemcpyAsync(s->buf_d, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return KHG_OK;
}
extern "C" int khg_fmllr_stats_add(khg_ctx* ctx, khg_fmllr_stats* dst, float scale, const khg_fmllr_stats* src) {
  if (ctx_dead(ctx) || !dst || !src) return khg_set_error(KHG_E_ARG, "khg_fmllr_stats_add: bad arguments");
  if (!std::isfinite(scale)) return khg_set_error(KHG_E_ARG, "khg_fmllr_stats_add: the scale is not finite");
  if (dst->ctx != ctx || src->ctx != ctx) return khg_set_error(KHG_E_ARG, "khg_fmllr_stats_add: a handle of another context");
  if (dst->S != src->S || dst->D != src->D) return khg_set_error(KHG_E_ARG, "khg_fmllr_stats_add: the two handles differ in speakers or dimension");
  if (dst == src) return khg_set_error(KHG_E_ARG, "khg_fmllr_stats_add: dst and src are the same handle");
  const int64_t n = (int64_t)dst->S * dst->SZ;
  KernelTimer kt(ctx, "k_fmllr_axpy");
  KHG_LAUNCH(ctx, k_fmllr_axpy, dim3(fm_grid(n)), dim3(256), 0, ctx->stream, dst->buf_d, src->buf_d, (double)scale, n);
  HIPCHK(hipGetLastError());
  return KHG_OK;
}

template <class T>
static int fm_grow(T** p, size_t* cap, size_t need) {
  if (need <= *cap && *p) return KHG_OK;
  DEVFREE(*p); *cap = 0;
  int rc = dev_alloc(p, need);
  if (rc) return rc;
  *cap = need;
  return KHG_OK;
}

template <int NDT>
static int mt_launch_gram(khg_ctx* ctx, const FmArgs& a, const FmItem* items, int nitems, int ngroups, size_t lds, const float* shift) {
  int rc = khg_lds_attribute((const void*)k_mllt_gram<NDT>, lds);
  if (rc) return rc;
  KHG_LAUNCH(ctx, k_mllt_gram<NDT>, dim3((unsigned)nitems, (unsigned)ngroups), dim3(256), lds, ctx->stream, a, items, shift);
  HIPCHK(hipGetLastError());
  return KHG_OK;
}
template <int NDT>
static int fm_launch_gram(khg_ctx* ctx, const FmArgs& a, const FmItem* items, int nitems, int ngroups, size_t lds) {
  int rc = khg_lds_attribute((const void*)k_fmllr_gram<NDT>, lds);
  if (rc) return rc;
  KHG_LAUNCH(ctx, k_fmllr_gram<NDT>, dim3((unsigned)nitems, (unsigned)ngroups), dim3(256), lds, ctx->stream, a, items);
  HIPCHK(hipGetLastError());
  return KHG_OK;
}

// The checks of the two accumulations below: khg_acc_stats_post's refusals, before anything is launched.  n_spk, st_ctx, st_D: the
// speakers, context and dimension of the statistics handle the caller was given.
static int fm_check_post(const char* name, khg_ctx* ctx, const khg_model* m, const khg_tm* tm, khg_utts* u, const khg_posteriors* p, float scale,
                         const int32_t* utt2spk_h, int32_t n_spk, const khg_ctx* st_ctx, int32_t st_D, PostInfo* pinfo) {
  const std::string who = std::string(name) + ": ";
  { int rf = utts_foreign_ctx(ctx, u, name); if (rf) return rf; }
  PostInfo& pi = *pinfo;
  posteriors_info(p, &pi);
  if (pi.ctx != ctx || m->ctx != ctx || tm->ctx != ctx || st_ctx != ctx || u->ctx != ctx) return khg_set_error(KHG_E_ARG, who + "a handle of another context");
  if (pi.U != u->n_utt)
    return khg_set_error(KHG_E_ARG, who + "the posteriors hold " + std::to_string(pi.U) + " utterances, the set " + std::to_string(u->n_utt));
  for (int i = 0; i < pi.U; ++i) {
    const int64_t tp = pi.frame_off[i + 1] - pi.frame_off[i], ts = u->frame_off[(size_t)i + 1] - u->frame_off[(size_t)i];
    if (tp != 0 && tp != ts)
      return khg_set_error(KHG_E_ARG, who + "utterance " + std::to_string(i) + " has " + std::to_string(tp) + " frames of posteriors and " + std::to_string(ts) + " frames of features");
  }
  if (m->D != u->D || st_D != m->D) return khg_set_error(KHG_E_ARG, who + "statistics / model / feature dimensions do not match");
  if (tm->max_pdf >= m->P) return khg_set_error(KHG_E_ARG, who + "transition model refers to pdf-ids the model does not have");
  if (!std::isfinite(scale)) return khg_set_error(KHG_E_ARG, who + "scale must be finite");
  if (pi.max_tid > tm->num_tids)
    return khg_set_error(KHG_E_ARG, who + "the posteriors hold transition-id " + std::to_string(pi.max_tid) + ", the transition model has " + std::to_string(tm->num_tids));
  for (int i = 0; i < pi.U; ++i)
    if (utt2spk_h[i] >= n_spk)
      return khg_set_error(KHG_E_ARG, who + "utterance " + std::to_string(i) + " belongs to speaker " + std::to_string(utt2spk_h[i]) + ", the statistics hold " + std::to_string(n_spk));
  const int64_t E = pi.entry_off[pi.U];
  if (E >= (int64_t)INT_MAX || u->N >= (int64_t)INT_MAX) return khg_set_error(KHG_E_UNSUPPORTED, who + "2^31 - 1 or more entries or frames");
  return KHG_OK;
}
// The accumulation shared by gmm-est-fmllr and the frame side of gmm-acc-mllt (7m, shift_d != nullptr: one speaker, the
// Gram kernel on x - shift without K and the border column, the call's sums left in st->call_d for the caller to fold): every check on
// the host first (fm_check_post, by the caller: pi is what it filled); then flatten -> heads -> per chunk of slices posrow / frame /
// gram / reduce -> the call's sums, all on the context's stream.  The MLLT call comes here behind its khg_acc_stats_post on the same
// posteriors and scale, which left the flattened entries in the set's buffers: they are not made again.  *ran: the call's sums were made.
static int fm_acc_post(const char* name, khg_ctx* ctx, const khg_model* m, const khg_tm* tm, khg_utts* u, const khg_posteriors* p, float scale,
                       const int32_t* utt2spk_h, khg_fmllr_stats* st, const PostInfo& pi, const float* shift_d, bool* ran) {
  const std::string who = std::string(name) + ": ";
  *ran = false;
  const int64_t E = pi.entry_off[pi.U];
  st->n_chunks_last = 0;
  if (E == 0) return KHG_OK;

  // ---- the plan: per speaker its utterances in set order, cut into slices of FM_SLICE frames; chunks of whole slices ----
  const int D = m->D;
  const int64_t CF = std::max<int64_t>(st->chunk_frames, FM_SLICE);               // frames of a chunk
  // slices of a chunk: twice the full slices its frames hold (short last slices of speakers), and no more parked images than 256 MiB
  const int64_t CI = std::max<int64_t>(1, std::min<int64_t>(2 * std::max<int64_t>(1, CF / FM_SLICE), (int64_t(256) << 20) / (8 * st->SZ)));
  std::vector<std::vector<int32_t>> spk_utts((size_t)st->S);
  for (int i = 0; i < pi.U; ++i)
    if (utt2spk_h[i] >= 0 && pi.frame_off[i + 1] > pi.frame_off[i]) spk_utts[(size_t)utt2spk_h[i]].push_back(i);
  struct Chunk { size_t seg0, seg1, item0, item1, run0, run1; int64_t frames, ents; };   // ents: an upper bound of the chunk's entries (its utterances')
  std::vector<FmSeg> segs; std::vector<FmItem> items; std::vector<FmRun> runs; std::vector<Chunk> chunks;
  Chunk cur{0, 0, 0, 0, 0, 0, 0, 0};
  const int64_t CE = 2 * CF;                         // entries of a chunk (exceeded by at most one slice's utterances)
  auto close_chunk = [&] {
    cur.seg1 = segs.size(); cur.item1 = items.size(); cur.run1 = runs.size();
    if (cur.item1 > cur.item0) chunks.push_back(cur);
    cur = Chunk{segs.size(), segs.size(), items.size(), items.size(), runs.size(), runs.size(), 0, 0};
  };
  for (int s = 0; s < st->S; ++s) {
    int64_t left = 0;
    for (int32_t ui : spk_utts[(size_t)s]) left += u->frame_off[(size_t)ui + 1] - u->frame_off[(size_t)ui];
    size_t k = 0; int64_t used = 0;                  // next utterance of the speaker, frames of it already placed
    while (left > 0) {
      const int n = (int)std::min<int64_t>(left, FM_SLICE);
      if (cur.frames + n > CF || (int64_t)(items.size() - cur.item0) >= CI || cur.ents > CE) close_chunk();
      const int slot = (int)(items.size() - cur.item0);
      items.push_back(FmItem{s, (int32_t)cur.frames, n, slot});
      if (runs.size() > cur.run0 && runs.back().spk == s) runs.back().nslot++;
      else runs.push_back(FmRun{s, slot, 1, 0});
      int need = n;
      while (need > 0) {
        const int32_t ui = spk_utts[(size_t)s][k];
        const int64_t T = u->frame_off[(size_t)ui + 1] - u->frame_off[(size_t)ui];
        const int take = (int)std::min<int64_t>(need, T - used);
        segs.push_back(FmSeg{(int32_t)(u->frame_off[(size_t)ui] + used), take, (int32_t)cur.frames, 0});
        cur.frames += take; used += take; need -= take;
        cur.ents += pi.entry_off[ui + 1] - pi.entry_off[ui];
        if (used == T) { ++k; used = 0; }
      }
      left -= n;
    }
  }
  close_chunk();
  if (chunks.empty()) return KHG_OK;                 // no utterance with a speaker and frames

  int rc = arena_flush(ctx);
  if (rc) return rc;
  // the flattened entries: the set's own buffers of khg_acc_stats_post
  rc = utts_grow_pe(u, (size_t)E);
  if (rc) return rc;
  int64_t maxf = 0; size_t maxi = 0;
  for (const Chunk& c : chunks) { maxf = std::max(maxf, c.frames); maxi = std::max(maxi, c.item1 - c.item0); }
  rc = KHG_OK;
  if ((size_t)maxf > st->pos_cap) {                  // the four per-frame arrays grow together
    DEVFREE(st->pos_row_d); DEVFREE(st->a_d); DEVFREE(st->b_d); DEVFREE(st->c_d);
    st->pos_cap = 0;
    rc = dev_alloc(&st->pos_row_d, (size_t)maxf);
    if (!rc) rc = dev_alloc(&st->a_d, (size_t)maxf * (size_t)D);
    if (!rc) rc = dev_alloc(&st->b_d, (size_t)maxf * (size_t)D);
    if (!rc) rc = dev_alloc(&st->c_d, (size_t)maxf);
    if (!rc) st->pos_cap = (size_t)maxf;
  }
  int64_t maxe = 1;
  for (const Chunk& c : chunks) maxe = std::max(maxe, std::min<int64_t>(c.ents, E));
  if (!rc) rc = fm_grow(&st->cnt_d, &st->cnt_cap, (size_t)maxf + 1);
  if (!rc && (size_t)maxe > st->ent_cap) {             // the per-entry arrays grow together
    DEVFREE(st->ent_id_d); DEVFREE(st->ea_d); DEVFREE(st->eb_d); DEVFREE(st->ec_d);
    st->ent_cap = 0;
    rc = dev_alloc(&st->ent_id_d, (size_t)maxe);
    if (!rc) rc = dev_alloc(&st->ea_d, (size_t)maxe * (size_t)D);
    if (!rc) rc = dev_alloc(&st->eb_d, (size_t)maxe * (size_t)D);
    if (!rc) rc = dev_alloc(&st->ec_d, (size_t)maxe);
    if (!rc) st->ent_cap = (size_t)maxe;
  }
  if (!rc) rc = fm_grow(&st->part_d, &st->part_cap, maxi * (size_t)st->SZ);
  if (!rc) rc = fm_grow(&st->row_first_d, &st->row_cap, (size_t)u->N);
  if (!rc) rc = fm_grow(&st->segs_d, &st->segs_cap, segs.size());
  if (!rc) rc = fm_grow(&st->items_d, &st->items_cap, items.size());
  if (!rc) rc = fm_grow(&st->runs_d, &st->runs_cap, runs.size());
  if (!rc && !st->call_d) rc = dev_alloc(&st->call_d, (size_t)st->S * (size_t)st->SZ);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(st->segs_d, segs.data(), sizeof(FmSeg) * segs.size(), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(st->items_d, items.data(), sizeof(FmItem) * items.size(), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(st->runs_d, runs.data(), sizeof(FmRun) * runs.size(), hipMemcpyHostToDevice, ctx->stream));
  ctx->pageable_pending = true;
  rc = sync_pageable(ctx);                           // the plan's host vectors go out of scope with the call
  if (rc) return rc;

  if (!shift_d) {
    rc = posteriors_flatten(ctx, p, u->frame_off_d, (double)scale, tm->num_tids, u->pe_row_d, u->pe_tid_d, u->pe_w_d, 0);
    if (rc) return rc;
  }
  HIPCHK(hipMemsetAsync(st->row_first_d, 0xFF, sizeof(int32_t) * (size_t)u->N, ctx->stream));
  HIPCHK(hipMemsetAsync(st->call_d, 0, sizeof(double) * (size_t)st->S * (size_t)st->SZ, ctx->stream));
  FmArgs a;
  a.feats = u->feats_d; a.D = D; a.N = u->N;
  a.gauss_off = m->gauss_off_d; a.gconsts = m->gconsts_d; a.miv = m->miv_d; a.iv = m->iv_d; a.nhiv = m->nhiv_d; a.P = m->P;
  a.id2pdf = tm->id2pdf_d; a.num_tids = tm->num_tids;
  a.e_row = u->pe_row_d; a.e_tid = u->pe_tid_d; a.e_w = u->pe_w_d; a.E = E;
  a.row_first = st->row_first_d; a.pos_row = st->pos_row_d; a.a = st->a_d; a.b = st->b_d; a.c = st->c_d;
  a.part = st->part_d; a.SZ = st->SZ; a.err_flag = ctx->err_flag_d;
  {
    KernelTimer kt(ctx, "k_fmllr_heads");
    KHG_LAUNCH(ctx, k_fmllr_heads, dim3(fm_grid(E)), dim3(256), 0, ctx->stream, a);
    HIPCHK(hipGetLastError());
  }
  int GM = 1;
  for (int i = 0; i < m->P; ++i) GM = std::max(GM, m->gauss_off[(size_t)i + 1] - m->gauss_off[(size_t)i]);
  const int NDT = (D + 15) / 16, DPf = (D + 3) & ~3;
  // the bucketed per-entry stage: a tile of GT Gaussians' rows (<= 40 KB) and FE_EB entries' ll rows and features share 62.5 KiB of LDS
  FeEntArgs ea;
  ea.DS = D | 1;
  ea.GT = std::max(1, std::min(GM, 40960 / (8 * ea.DS)));
  ea.GS = GM;
  const size_t lds_fix = sizeof(float) * (size_t)(2 * ea.GT * ea.DS + ea.GT), lds_per = sizeof(float) * (size_t)(GM + D);
  ea.EB = (int)std::min<size_t>(64, (64000 - lds_fix) / lds_per);
  const bool bucketed = ea.EB >= 4;                  // a pdf of more than ~3900 Gaussians: the one-wave-per-frame form below
  const size_t lds_entry = lds_fix + lds_per * (size_t)std::max(ea.EB, 1);
  if (bucketed && lds_entry > 48 * 1024) HIPCHK(hipFuncSetAttribute((const void*)k_fmllr_entry, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_entry));
  const size_t lds_frame = sizeof(float) * 4 * (size_t)(2 * DPf + GM);
  if (!bucketed) {
    if (lds_frame > 64 * 1024) return khg_set_error(KHG_E_UNSUPPORTED, who + "a pdf of " + std::to_string(GM) + " Gaussians is too large for the frame kernel");
    if (lds_frame > 48 * 1024) HIPCHK(hipFuncSetAttribute((const void*)k_fmllr_frame, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_frame));
  }
  int sort_bits = 1;
  while ((1 << sort_bits) <= m->P) ++sort_bits;        // keys are 0 .. P
  const int D1 = D + 1, NP = D1 * (D1 + 1) / 2, NT = (NP + 15) / 16 + (D1 + 15) / 16, ngroups = (NT + FM_TPG - 1) / FM_TPG;
  const size_t lds_gram = sizeof(float) * (size_t)FM_TB * (size_t)((D1 | 1) + 2 * 16 * NDT);
  const int mt_ngroups = ((D * D1 / 2 + 15) / 16 + FM_TPG - 1) / FM_TPG;
  const size_t mt_lds_gram = sizeof(float) * (size_t)FM_TB * (size_t)((D1 | 1) + 16 * NDT);
  for (const Chunk& c : chunks) {
    const int nseg = (int)(c.seg1 - c.seg0), nit = (int)(c.item1 - c.item0), nrun = (int)(c.run1 - c.run0);
    {
      KernelTimer kt(ctx, "k_fmllr_posrow");
      KHG_LAUNCH(ctx, k_fmllr_posrow, dim3((unsigned)std::min(nseg, 4096)), dim3(256), 0, ctx->stream, st->segs_d + c.seg0, nseg, st->pos_row_d);
      HIPCHK(hipGetLastError());
    }
    if (bucketed) {
      ea.f = a; ea.npos = (int32_t)c.frames; ea.capE = (int32_t)std::min<int64_t>(c.ents, E);
      ea.cnt = st->cnt_d; ea.ent_id = st->ent_id_d; ea.keys = u->pe_keys_d; ea.vals = u->pe_vals_d;
      ea.skeys = u->pe_keys_out_d; ea.svals = reinterpret_cast<uint32_t*>(u->pe_ids_d);
      ea.ea = st->ea_d; ea.eb = st->eb_d; ea.ec = st->ec_d;
      size_t need = 0;
      HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, need, ea.keys, u->pe_keys_out_d, ea.vals, reinterpret_cast<uint32_t*>(u->pe_ids_d), ea.capE, 0, sort_bits, ctx->stream));
      if (need > u->pe_tmp_bytes) {
        DEVFREE(u->pe_tmp_d);
        { int rt = u_alloc(u, reinterpret_cast<char**>(&u->pe_tmp_d), need); if (rt) return rt; }
        u->pe_tmp_bytes = need;
      }
      {
        KernelTimer kt(ctx, "k_fmllr_bucket");
        KHG_LAUNCH(ctx, k_fmllr_count, dim3(fm_grid(c.frames)), dim3(256), 0, ctx->stream, ea);
        KHG_LAUNCH(ctx, k_fmllr_scan, dim3(1), dim3(1024), 0, ctx->stream, st->cnt_d, (int32_t)c.frames);
        KHG_LAUNCH(ctx, k_fmllr_keys, dim3(fm_grid(std::max<int64_t>(c.frames, ea.capE))), dim3(256), 0, ctx->stream, ea);
        HIPCHK(hipGetLastError());
        HIPCHK(hipcub::DeviceRadixSort::SortPairs(u->pe_tmp_d, need, ea.keys, u->pe_keys_out_d, ea.vals, reinterpret_cast<uint32_t*>(u->pe_ids_d), ea.capE, 0, sort_bits, ctx->stream));
      }
      {
        KernelTimer kt(ctx, "k_fmllr_entry");
        KHG_LAUNCH(ctx, k_fmllr_entry, dim3((unsigned)((ea.capE + ea.EB - 1) / ea.EB)), dim3(256), lds_entry, ctx->stream, ea);
        HIPCHK(hipGetLastError());
      }
      {
        KernelTimer kt(ctx, "k_fmllr_fsum");
        KHG_LAUNCH(ctx, k_fmllr_fsum, dim3(fm_grid(c.frames * D)), dim3(256), 0, ctx->stream, ea);
        HIPCHK(hipGetLastError());
      }
    } else {
      KernelTimer kt(ctx, "k_fmllr_frame");
      KHG_LAUNCH(ctx, k_fmllr_frame, dim3((unsigned)std::min<int64_t>(65536, (c.frames + 3) / 4)), dim3(256), lds_frame, ctx->stream, a, (int32_t)c.frames, DPf, GM);
      HIPCHK(hipGetLastError());
    }
    if (shift_d) {
      KernelTimer kt(ctx, "k_mllt_gram");
      const FmItem* it = st->items_d + c.item0;
      switch (NDT) {
        case 1: rc = mt_launch_gram<1>(ctx, a, it, nit, mt_ngroups, mt_lds_gram, shift_d); break;
        case 2: rc = mt_launch_gram<2>(ctx, a, it, nit, mt_ngroups, mt_lds_gram, shift_d); break;
        case 3: rc = mt_launch_gram<3>(ctx, a, it, nit, mt_ngroups, mt_lds_gram, shift_d); break;
        case 4: rc = mt_launch_gram<4>(ctx, a, it, nit, mt_ngroups, mt_lds_gram, shift_d); break;
        default: rc = mt_launch_gram<5>(ctx, a, it, nit, mt_ngroups, mt_lds_gram, shift_d); break;
      }
      if (rc) return rc;
    } else {
      KernelTimer kt(ctx, "k_fmllr_gram");
      const FmItem* it = st->items_d + c.item0;
      switch (NDT) {
        case 1: rc = fm_launch_gram<1>(ctx, a, it, nit, ngroups, lds_gram); break;
        case 2: rc = fm_launch_gram<2>(ctx, a, it, nit, ngroups, lds_gram); break;
        case 3: rc = fm_launch_gram<3>(ctx, a, it, nit, ngroups, lds_gram); break;
        case 4: rc = fm_launch_gram<4>(ctx, a, it, nit, ngroups, lds_gram); break;
        default: rc = fm_launch_gram<5>(ctx, a, it, nit, ngroups, lds_gram); break;
      }
      if (rc) return rc;
    }
    {
      KernelTimer kt(ctx, "k_fmllr_reduce");
      const unsigned gy = (unsigned)std::min<int64_t>(64, (st->SZ + 255) / 256);
      KHG_LAUNCH(ctx, k_fmllr_reduce, dim3((unsigned)nrun, gy), dim3(256), 0, ctx->stream, st->runs_d + c.run0, st->part_d, st->call_d, st->SZ);
      HIPCHK(hipGetLastError());
    }
  }
  if (!shift_d) {
    KernelTimer kt(ctx, "k_fmllr_axpy");
    const int64_t n = (int64_t)st->S * st->SZ;
    KHG_LAUNCH(ctx, k_fmllr_axpy, dim3(fm_grid(n)), dim3(256), 0, ctx->stream, st->buf_d, st->call_d, 1.0, n);
    HIPCHK(hipGetLastError());
  }
  st->n_chunks_last = (int32_t)chunks.size();
  *ran = true;
  return KHG_OK;
}
extern "C" int khg_acc_fmllr_stats_post(khg_ctx* ctx, const khg_model* m, const khg_tm* tm, khg_utts* u, const khg_posteriors* p, float scale,
                                        const int32_t* utt2spk_h, khg_fmllr_stats* st) {
  if (ctx_dead(ctx) || !m || !tm || !u || !p || !utt2spk_h || !st) return khg_set_error(KHG_E_ARG, "khg_acc_fmllr_stats_post: bad arguments");
  const char* name = "khg_acc_fmllr_stats_post";
  PostInfo pi;
  int rc = fm_check_post(name, ctx, m, tm, u, p, scale, utt2spk_h, st->S, st->ctx, st->D, &pi);
  if (rc) return rc;
  bool ran = false;
  return fm_acc_post(name, ctx, m, tm, u, p, scale, utt2spk_h, st, pi, nullptr, &ran);
}

// transform-feats: the rows of every utterance through its speaker's W.  W_h (host, [n_spk][D][D + 1]) or W_d (device, the same
// layout); out_d: a caller's buffer of the set's size, or NULL for the set's own rows in place.
extern "C" int khg_utts_transform_feats(khg_ctx* ctx, khg_utts* u, int32_t n_spk, const int32_t* utt2spk_h, const float* W_h, const float* W_d,
                                        float* out_d) {
  const std::string who = "khg_utts_transform_feats: ";
  if (ctx_dead(ctx) || !u || !utt2spk_h || n_spk < 1 || (!W_h) == (!W_d)) return khg_set_error(KHG_E_ARG, who + "bad arguments (exactly one of W_h / W_d)");
  { int rf = utts_foreign_ctx(ctx, u, "khg_utts_transform_feats"); if (rf) return rf; }
  if (u->ctx != ctx) return khg_set_error(KHG_E_ARG, who + "a handle of another context");
  if (u->D > KHG_FMLLR_MAX_DIM) return khg_set_error(KHG_E_UNSUPPORTED, who + "dim " + std::to_string(u->D) + " is above KHG_FMLLR_MAX_DIM");
  for (int i = 0; i < u->n_utt; ++i)
    if (utt2spk_h[i] >= n_spk)
      return khg_set_error(KHG_E_ARG, who + "utterance " + std::to_string(i) + " belongs to speaker " + std::to_string(utt2spk_h[i]) + " of " + std::to_string(n_spk));
  if (u->N == 0) return KHG_OK;
  const int D = u->D;
  std::vector<FtItem> items;
  for (int i = 0; i < u->n_utt; ++i)
    for (int64_t r = u->frame_off[(size_t)i]; r < u->frame_off[(size_t)i + 1]; r += FT_ROWS)
      items.push_back(FtItem{i, (int32_t)std::min<int64_t>(FT_ROWS, u->frame_off[(size_t)i + 1] - r), r});
  if (items.size() >= (size_t)INT_MAX) return khg_set_error(KHG_E_UNSUPPORTED, who + "too many rows");
  int rc = arena_flush(ctx);
  if (rc) return rc;
  FtItem* items_d = nullptr; int32_t* u2s_d = nullptr; float* Wup_d = nullptr;
  auto cleanup = [&] { DEVFREE(items_d); DEVFREE(u2s_d); DEVFREE(Wup_d); };
  rc = dev_alloc(&items_d, items.size());
  if (!rc) rc = dev_alloc(&u2s_d, (size_t)u->n_utt);
  if (!rc && W_h) rc = dev_alloc(&Wup_d, (size_t)n_spk * D * (D + 1));
  if (rc) { cleanup(); return rc; }
  hipError_t e = hipMemcpyAsync(items_d, items.data(), sizeof(FtItem) * items.size(), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(u2s_d, utt2spk_h, sizeof(int32_t) * (size_t)u->n_utt, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess && W_h) e = hipMemcpyAsync(Wup_d, W_h, sizeof(float) * (size_t)n_spk * D * (D + 1), hipMemcpyHostToDevice, ctx->stream);
  if (e != hipSuccess) { cleanup(); return khg_set_error(KHG_E_HIP, who + hipGetErrorString(e)); }
  const size_t lds = sizeof(float) * ((size_t)D * (D + 1) + (size_t)FT_ROWS * D);
  float* dst = out_d ? out_d : const_cast<float*>(u->feats_d);
  {
    KernelTimer kt(ctx, "k_fmllr_transform");
    KHG_LAUNCH(ctx, k_fmllr_transform, dim3((unsigned)items.size()), dim3(256), lds, ctx->stream, items_d, u2s_d, W_h ? Wup_d : W_d, u->feats_d, dst, D);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);     // the temporaries and the caller's host arrays are free again
  cleanup();
  if (e != hipSuccess) return khg_set_error(KHG_E_HIP, who + hipGetErrorString(e));
  if (!out_d) return khg_utts_features_changed(u);
  return KHG_OK;
}

// ali-to-post on the device: one entry of weight 1 per frame from the set's resident alignment.  An utterance whose
// alignment failed (its ids are 0) gets no frames.  Only one flag per utterance comes down; the ids never leave the device.
__global__ __launch_bounds__(256) void k_ali_failed(const int32_t* __restrict__ ali, const int64_t* __restrict__ frame_off, int32_t n_utt, int32_t* __restrict__ flag) {
  const int u = blockIdx.x * 256 + threadIdx.x;
  if (u >= n_utt) return;
  const int64_t f0 = frame_off[u], f1 = frame_off[u + 1];
  flag[u] = (f1 > f0 && ali[f0] == 0) ? 1 : 0;
}
// blockIdx.x strides over the utterances; dst_off: the handle's frame offsets (an utterance without frames there is skipped)
__global__ __launch_bounds__(256) void k_post_from_ali(const int32_t* __restrict__ ali, const int64_t* __restrict__ src_off, const int64_t* __restrict__ dst_off,
                                                       int32_t n_utt, int64_t* __restrict__ entry_begin, double* __restrict__ weight, int32_t* __restrict__ tid) {
  for (int u = blockIdx.x; u < n_utt; u += gridDim.x) {
    const int64_t d0 = dst_off[u], n = dst_off[u + 1] - d0, s0 = src_off[u];
    for (int64_t t = threadIdx.x; t < n; t += 256) { entry_begin[d0 + t] = d0 + t; weight[d0 + t] = 1.0; tid[d0 + t] = ali[s0 + t]; }
    if (u == n_utt - 1 && threadIdx.x == 0) entry_begin[dst_off[n_utt]] = dst_off[n_utt];
  }
}
extern "C" int khg_posteriors_from_ali(khg_ctx* ctx, khg_utts* u, khg_posteriors** out) {
  const std::string who = "khg_posteriors_from_ali: ";
  if (ctx_dead(ctx) || !u || !out) return khg_set_error(KHG_E_ARG, who + "bad arguments");
  *out = nullptr;
  { int rf = utts_foreign_ctx(ctx, u, "khg_posteriors_from_ali"); if (rf) return rf; }
  if (u->ctx != ctx) return khg_set_error(KHG_E_ARG, who + "a handle of another context");
  if (!u->ali_valid || !u->ali_d) return khg_set_error(KHG_E_ARG, who + "the set has no resident alignment (khg_align or khg_ali_upload first)");
  int rc = wait_ali(ctx, u);
  if (rc) return rc;
  const int U = u->n_utt;
  std::vector<int32_t> failed((size_t)std::max(U, 1), 0);
  int32_t* flag_d = nullptr;
  if (U > 0) {
    rc = dev_alloc(&flag_d, (size_t)U);
    if (rc) return rc;
    KHG_LAUNCH(ctx, k_ali_failed, dim3((unsigned)((U + 255) / 256)), dim3(256), 0, ctx->stream, u->ali_d, u->frame_off_d, U, flag_d);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(failed.data(), flag_d, sizeof(int32_t) * (size_t)U, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    DEVFREE(flag_d);
    if (e != hipSuccess) return khg_set_error(KHG_E_HIP, who + hipGetErrorString(e));
  }
  std::vector<int64_t> fo((size_t)U + 1, 0);
  for (int i = 0; i < U; ++i) fo[(size_t)i + 1] = fo[(size_t)i] + (failed[(size_t)i] ? 0 : u->frame_off[(size_t)i + 1] - u->frame_off[(size_t)i]);
  int64_t* eb = nullptr; double* w = nullptr; int32_t* tid = nullptr; const int64_t* fo_d = nullptr;
  khg_posteriors* p = nullptr;
  rc = posteriors_make_unit(ctx, U, fo.data(), &eb, &w, &tid, &fo_d, &p);
  if (rc) return rc;
  if (U > 0) {
    KernelTimer kt(ctx, "k_post_from_ali");
    KHG_LAUNCH(ctx, k_post_from_ali, dim3((unsigned)std::min(U, 8192)), dim3(256), 0, ctx->stream, u->ali_d, u->frame_off_d, fo_d, U, eb, w, tid);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { (void)khg_posteriors_destroy(p); return khg_set_error(KHG_E_HIP, who + hipGetErrorString(e)); }
  }
  *out = p;
  return KHG_OK;
}

// The estimate on the device: the statistics stay where the accumulation left them, the transforms can stay in W_d.
extern "C" int khg_fmllr_stats_estimate(khg_ctx* ctx, const khg_fmllr_stats* st, const khg_fmllr_options* o, float* W_h, float* W_d, double* objf_impr_h,
                                        double* count_h, int32_t* status_h) {
  const std::string who = "khg_fmllr_stats_estimate: ";
  if (ctx_dead(ctx) || !st || st->ctx != ctx) return khg_set_error(KHG_E_ARG, who + "bad arguments");
  khg_fmllr_options def;
  khg_fmllr_options_default(&def);
  if (!o) o = &def;
  if (!std::isfinite(o->min_count) || o->num_iters < 0) return khg_set_error(KHG_E_ARG, who + "an option is not finite or negative");
  { int rc = check_err_flag(ctx, "khg_acc_fmllr_stats_post"); if (rc) return rc; }
  const int S = st->S, D = st->D, D1 = D + 1;
  const size_t nW = (size_t)S * D * D1, nM = (size_t)S * D * D1 * D1;
  double *invg = nullptr, *work = nullptr, *W = nullptr, *impr = nullptr; int32_t* status = nullptr; float* Wf = nullptr;
  auto cleanup = [&] { DEVFREE(invg); DEVFREE(work); DEVFREE(W); DEVFREE(impr); DEVFREE(status); DEVFREE(Wf); };
  int rc = dev_alloc(&invg, nM);
  if (!rc) rc = dev_alloc(&work, nM);
  if (!rc) rc = dev_alloc(&W, nW);
  if (!rc) rc = dev_alloc(&impr, (size_t)S);
  if (!rc) rc = dev_alloc(&status, (size_t)S);
  if (!rc && !W_d) rc = dev_alloc(&Wf, nW);
  if (rc) { cleanup(); return rc; }
  FeArgs a;
  a.stats = st->buf_d; a.SZ = st->SZ; a.S = S; a.D = D; a.min_count = o->min_count; a.num_iters = o->num_iters;
  a.invg = invg; a.work = work; a.W = W; a.status = status; a.impr = impr; a.Wf = W_d ? W_d : Wf;
  hipError_t e = hipMemsetAsync(status, 0, sizeof(int32_t) * (size_t)S, ctx->stream);
  if (e == hipSuccess) {
    KernelTimer kt(ctx, "k_fmllr_invg");
    KHG_LAUNCH(ctx, k_fmllr_invg, dim3((unsigned)(S * D)), dim3(256), 0, ctx->stream, a);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    KernelTimer kt(ctx, "k_fmllr_rows");
    const size_t lds_rows = sizeof(double) * 2 * (size_t)D * D;
    const int use_lds = lds_rows <= 56 * 1024;
    if (use_lds && lds_rows > 40 * 1024) e = hipFuncSetAttribute((const void*)k_fmllr_rows, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_rows);
    KHG_LAUNCH(ctx, k_fmllr_rows, dim3((unsigned)S), dim3(256), use_lds ? lds_rows : 0, ctx->stream, a, use_lds);
    e = hipGetLastError();
  }
  if (e == hipSuccess && status_h) e = hipMemcpyAsync(status_h, status, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && objf_impr_h) e = hipMemcpyAsync(objf_impr_h, impr, sizeof(double) * (size_t)S, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && W_h) e = hipMemcpyAsync(W_h, a.Wf, sizeof(float) * nW, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && count_h)
    e = hipMemcpy2DAsync(count_h, sizeof(double), st->buf_d + st->SZ - 1, sizeof(double) * (size_t)st->SZ, sizeof(double), (size_t)S, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  cleanup();
  if (e != hipSuccess) return khg_set_error(KHG_E_HIP, who + hipGetErrorString(e));
  return KHG_OK;
}

// ---- MLLT -------------------------------------------------------------------------------------------------------------
struct khg_mllt_stats {
  khg_ctx* ctx = nullptr;
  int32_t D = 0;
  int64_t SZ = 0;                    // doubles: G | beta
  double* buf_d = nullptr;           // [SZ]
  khg_fmllr_stats fm;                // the frame side's plan scratch: one speaker, blocks of SZ doubles; fm.call_d holds the call's S
  double* gcall_d = nullptr;         // [SZ] the call's C
  khg_accs* acc = nullptr;           // the call's occ_g / m_g, laid out for the model of the last call
  float* shift_d = nullptr;          // [D]
  double* shift_part_d = nullptr; size_t shift_cap = 0;   // [slices][D]
};

static inline int64_t mt_block_size(int D) { return (int64_t)D * ((int64_t)D * (D + 1) / 2) + 1; }
static void mt_free_scratch(khg_fmllr_stats* s) {
  DEVFREE(s->call_d); DEVFREE(s->pos_row_d); DEVFREE(s->a_d); DEVFREE(s->b_d); DEVFREE(s->c_d); DEVFREE(s->part_d);
  DEVFREE(s->cnt_d); DEVFREE(s->ent_id_d); DEVFREE(s->ea_d); DEVFREE(s->eb_d); DEVFREE(s->ec_d);
  DEVFREE(s->row_first_d); DEVFREE(s->segs_d); DEVFREE(s->items_d); DEVFREE(s->runs_d);
}

extern "C" int khg_mllt_stats_create(khg_ctx* ctx, int32_t dim, khg_mllt_stats** out) {
  if (ctx_dead(ctx) || !out || dim < 1) return khg_set_error(KHG_E_ARG, "khg_mllt_stats_create: bad arguments");
  if (dim > KHG_MLLT_MAX_DIM)
    return khg_set_error(KHG_E_UNSUPPORTED, "khg_mllt_stats_create: dim " + std::to_string(dim) + " is above KHG_MLLT_MAX_DIM");
  khg_mllt_stats* s = new khg_mllt_stats();
  s->ctx = ctx; s->D = dim; s->SZ = mt_block_size(dim);
  s->fm.ctx = ctx; s->fm.S = 1; s->fm.D = dim; s->fm.SZ = s->SZ;
  int rc = dev_alloc(&s->buf_d, (size_t)s->SZ);
  if (!rc) rc = dev_alloc(&s->gcall_d, (size_t)s->SZ);
  if (!rc) rc = dev_alloc(&s->shift_d, (size_t)dim);
  if (rc) { (void)khg_mllt_stats_destroy(s); return rc; }
  *out = s;
  return khg_mllt_stats_zero(ctx, s);
}
extern "C" int khg_mllt_stats_destroy(khg_mllt_stats* s) {
  if (!s) return KHG_OK;
  DEVFREE(s->buf_d); DEVFREE(s->gcall_d); DEVFREE(s->shift_d); DEVFREE(s->shift_part_d);
  mt_free_scratch(&s->fm);
  if (s->acc) (void)khg_accs_destroy(s->acc);
  delete s;
  return KHG_OK;
}
extern "C" int khg_mllt_stats_zero(khg_ctx* ctx, khg_mllt_stats* s) {
  if (ctx_dead(ctx) || !s || s->ctx != ctx) return khg_set_error(KHG_E_ARG, "khg_mllt_stats_zero: bad arguments");
  HIPCHK(hipMemsetAsync(s->buf_d, 0, sizeof(double) * (size_t)s->SZ, ctx->stream));
  return KHG_OK;
}
extern "C" int khg_mllt_stats_set_chunk_frames(khg_mllt_stats* s, int64_t frames) {
  if (!s || frames < 1) return khg_set_error(KHG_E_ARG, "khg_mllt_stats_set_chunk_frames: bad arguments");
  return khg_fmllr_stats_set_chunk_frames(&s->fm, frames);
}
extern "C" int khg_mllt_stats_num_chunks(const khg_mllt_stats* s, int32_t* n) {
  if (!s || !n) return khg_set_error(KHG_E_ARG, "khg_mllt_stats_num_chunks: bad arguments");
  *n = s->fm.n_chunks_last;
  return KHG_OK;
}
extern "C" int khg_mllt_stats_download(khg_ctx* ctx, const khg_mllt_stats* s, double* beta_h, double* G_h) {
  if (ctx_dead(ctx) || !s || s->ctx != ctx) return khg_set_error(KHG_E_ARG, "khg_mllt_stats_download: bad arguments");
  { int rc = check_err_flag(ctx, "khg_acc_mllt_stats_post"); if (rc) return rc; }
  if (G_h) HIPCHK(hipMemcpyAsync(G_h, s->buf_d, sizeof(double) * (size_t)(s->SZ - 1), hipMemcpyDeviceToHost, ctx->stream));
  if (beta_h) HIPCHK(hipMemcpyAsync(beta_h, s->buf_d + s->SZ - 1, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return KHG_OK;
}
extern "C" int khg_mllt_stats_upload(khg_ctx* ctx, khg_mllt_stats* s, const double* beta_h, const double* G_h) {
  if (ctx_dead(ctx) || !s || s->ctx != ctx || !beta_h || !G_h) return khg_set_error(KHG_E_ARG, "khg_mllt_stats_upload: bad arguments");
  HIPCHK(hipMemcpyAsync(s->buf_d, G_h, sizeof(double) * (size_t)(s->SZ - 1), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(s->buf_d + s->SZ - 1, beta_h, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return KHG_OK;
}
extern "C" int khg_mllt_stats_add(khg_ctx* ctx, khg_mllt_stats* dst, float scale, const khg_mllt_stats* src) {
  if (ctx_dead(ctx) || !dst || !src) return khg_set_error(KHG_E_ARG, "khg_mllt_stats_add: bad arguments");
  if (!std::isfinite(scale)) return khg_set_error(KHG_E_ARG, "khg_mllt_stats_add: the scale is not finite");
  if (dst->ctx != ctx || src->ctx != ctx) return khg_set_error(KHG_E_ARG, "khg_mllt_stats_add: a handle of another context");
  if (dst->D != src->D) return khg_set_error(KHG_E_ARG, "khg_mllt_stats_add: the two handles differ in dimension");
  if (dst == src) return khg_set_error(KHG_E_ARG, "khg_mllt_stats_add: dst and src are the same handle");
  KernelTimer kt(ctx, "k_fmllr_axpy");
  KHG_LAUNCH(ctx, k_fmllr_axpy, dim3(fm_grid(dst->SZ)), dim3(256), 0, ctx->stream, dst->buf_d, src->buf_d, (double)scale, dst->SZ);
  HIPCHK(hipGetLastError());
  return KHG_OK;
}

template <int NDT>
static int mt_launch_gauss(khg_ctx* ctx, const MtGaussArgs& a, int nslice, int ngroups, size_t lds) {
  int rc = khg_lds_attribute((const void*)k_mllt_gauss<NDT>, lds);
  if (rc) return rc;
  KHG_LAUNCH(ctx, k_mllt_gauss<NDT>, dim3((unsigned)nslice, (unsigned)ngroups), dim3(256), lds, ctx->stream, a);
  HIPCHK(hipGetLastError());
  return KHG_OK;
}

// gmm-acc-mllt: the checks; occ_g / m_g of the call (K3); the shift; the frame side (fm_acc_post); the Gaussian side per
// chunk of slices; S - C into the handle.
extern "C" int khg_acc_mllt_stats_post(khg_ctx* ctx, const khg_model* m, const khg_tm* tm, khg_utts* u, const khg_posteriors* p, float scale,
                                       khg_mllt_stats* st) {
  const char* name = "khg_acc_mllt_stats_post";
  if (ctx_dead(ctx) || !m || !tm || !u || !p || !st) return khg_set_error(KHG_E_ARG, std::string(name) + ": bad arguments");
  std::vector<int32_t> one((size_t)std::max(u->n_utt, 1), 0);        // every utterance belongs to the one speaker
  PostInfo pi;
  int rc = fm_check_post(name, ctx, m, tm, u, p, scale, one.data(), 1, st->ctx, st->D, &pi);
  if (!rc) rc = k3_post_check(ctx, m, std::string(name) + ": ");
  if (rc) return rc;
  st->fm.n_chunks_last = 0;
  if (pi.entry_off[pi.U] == 0 || m->sumG == 0) return KHG_OK;
  const int D = m->D;
  // scratch: the accumulator block for this model's layout, the slices' shift sums, the parked images of both sides
  if (st->acc && (st->acc->sumG != m->sumG || st->acc->D != D || st->acc->num_tids != tm->num_tids)) { (void)khg_accs_destroy(st->acc); st->acc = nullptr; }
  if (!st->acc) { rc = khg_accs_create(ctx, m, tm, &st->acc); if (rc) return rc; }
  const int64_t nslice = (m->sumG + MT_GSLICE - 1) / MT_GSLICE;
  const int64_t CI = std::max<int64_t>(1, std::min<int64_t>(nslice, (int64_t(256) << 20) / (8 * st->SZ)));     // Gaussian-side slices of a chunk
  rc = fm_grow(&st->shift_part_d, &st->shift_cap, (size_t)nslice * (size_t)D);
  if (!rc) rc = fm_grow(&st->fm.part_d, &st->fm.part_cap, (size_t)CI * (size_t)st->SZ);
  if (rc) return rc;
  // K3 from posteriors with ONE work item per pdf, however many entries its bucket holds (k3_acc_stats_post_one_block): a cell of the block
  // then receives one workgroup's sum, made in chunk order over the stably sorted entries, so occ_g / m_g -- and with them C -- have
  // the same bits from run to run.  K3's own choice cuts a bucket into several items, which end with fp64 atomics into the same cells
  // in whatever order they finish.  The price: the pdf with the most entries (silence) is one workgroup's walk.
  rc = khg_accs_zero(ctx, st->acc);
  if (!rc) rc = k3_acc_stats_post_one_block(ctx, m, tm, u, p, scale, st->acc);
  if (rc) return rc;
  {
    KernelTimer kt(ctx, "k_mllt_shift");
    KHG_LAUNCH(ctx, k_mllt_shift_part, dim3((unsigned)nslice), dim3(128), 0, ctx->stream, m->miv_d, m->iv_d, m->sumG, D, st->shift_part_d);
    KHG_LAUNCH(ctx, k_mllt_shift, dim3(1), dim3(128), 0, ctx->stream, st->shift_part_d, (int32_t)nslice, m->sumG, D, st->shift_d);
    HIPCHK(hipGetLastError());
  }
  bool ran = false;
  rc = fm_acc_post(name, ctx, m, tm, u, p, scale, one.data(), &st->fm, pi, st->shift_d, &ran);
  if (rc) return rc;
  if (!ran) return KHG_OK;                                           // no utterance with frames
  HIPCHK(hipMemsetAsync(st->gcall_d, 0, sizeof(double) * (size_t)st->SZ, ctx->stream));
  const int NDT = (D + 15) / 16, NP = D * (D + 1) / 2, ngroups = ((NP + 15) / 16 + FM_TPG - 1) / FM_TPG, XS = (D + 1) | 1;
  const size_t lds = sizeof(double) * (size_t)(2 * MT_GB * XS + MT_GB) + sizeof(float) * (size_t)MT_GB * 16 * (size_t)NDT;
  MtGaussArgs ga;
  ga.miv = m->miv_d; ga.iv = m->iv_d; ga.occ = st->acc->occ(); ga.mean = st->acc->mean(); ga.shift = st->shift_d;
  ga.sumG = m->sumG; ga.D = D; ga.part = st->fm.part_d; ga.SZ = st->SZ;
  for (int64_t s0 = 0; s0 < nslice; s0 += CI) {
    const int ns = (int)std::min<int64_t>(CI, nslice - s0);
    ga.g_first = s0 * MT_GSLICE;
    {
      KernelTimer kt(ctx, "k_mllt_gauss");
      switch (NDT) {
        case 1: rc = mt_launch_gauss<1>(ctx, ga, ns, ngroups, lds); break;
        case 2: rc = mt_launch_gauss<2>(ctx, ga, ns, ngroups, lds); break;
        case 3: rc = mt_launch_gauss<3>(ctx, ga, ns, ngroups, lds); break;
        case 4: rc = mt_launch_gauss<4>(ctx, ga, ns, ngroups, lds); break;
        default: rc = mt_launch_gauss<5>(ctx, ga, ns, ngroups, lds); break;
      }
      if (rc) return rc;
    }
    {
      KernelTimer kt(ctx, "k_mllt_greduce");
      const unsigned gy = (unsigned)std::min<int64_t>(64, (st->SZ + 255) / 256);
      KHG_LAUNCH(ctx, k_mllt_greduce, dim3(gy), dim3(256), 0, ctx->stream, st->fm.part_d, ns, st->gcall_d, st->SZ);
      HIPCHK(hipGetLastError());
    }
  }
  {
    KernelTimer kt(ctx, "k_mllt_fold");
    KHG_LAUNCH(ctx, k_mllt_fold, dim3(fm_grid(st->SZ)), dim3(256), 0, ctx->stream, st->buf_d, st->fm.call_d, st->gcall_d, st->SZ);
    HIPCHK(hipGetLastError());
  }
  return KHG_OK;
}

extern "C" int khg_model_transform_means(khg_ctx* ctx, khg_model* m, const float* M_h) {
  const std::string who = "khg_model_transform_means: ";
  if (ctx_dead(ctx) || !m || !M_h) return khg_set_error(KHG_E_ARG, who + "bad arguments");
  if (m->ctx != ctx) return khg_set_error(KHG_E_ARG, who + "a handle of another context");
  if (m->D > KHG_MLLT_MAX_DIM) return khg_set_error(KHG_E_UNSUPPORTED, who + "dim " + std::to_string(m->D) + " is above KHG_MLLT_MAX_DIM");
  if (!m->has_weights) return khg_set_error(KHG_E_ARG, who + "the model has no weights (khg_model_set_weights)");
  const int D = m->D;
  for (int i = 0; i < D * D; ++i)
    if (!std::isfinite(M_h[i])) return khg_set_error(KHG_E_ARG, who + "the matrix is not finite");
  if (m->sumG == 0) return KHG_OK;
  float* M_d = nullptr; int32_t* bad_d = nullptr;
  int rc = dev_alloc(&M_d, (size_t)D * D);
  if (!rc) rc = dev_alloc(&bad_d, 1);
  int32_t bad = 0;
  if (!rc) {
    hipError_t e = hipMemcpyAsync(M_d, M_h, sizeof(float) * (size_t)D * D, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(bad_d, 0, sizeof(int32_t), ctx->stream);
    if (e == hipSuccess) {
      KernelTimer kt(ctx, "k_model_transform_means");
      const size_t lds = sizeof(float) * ((size_t)D * (D | 1) + 8 * (size_t)D);
      const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(4096, (m->sumG + 3) / 4));
      KHG_LAUNCH(ctx, k_model_transform_means, dim3(grid), dim3(256), lds, ctx->stream, M_d, m->sumG, D, m->weights_d, m->iv_d, m->miv_d, m->gconsts_d, bad_d);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, bad_d, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) rc = khg_set_error(KHG_E_HIP, who + hipGetErrorString(e));
  }
  DEVFREE(M_d); DEVFREE(bad_d);
  if (rc) return rc;
  // new K1 tile image + per-parameter-version data, as khg_model_ebw_update ends -- also behind a gconst that is not a number: the
  // kernel has rewritten the rows by then, and the handle's images must not disagree with them
  rc = model_pack(ctx, m);
  if (bad) return khg_set_error(KHG_E_RUNTIME, who + "not a number in gconst computation (the handle holds the transformed parameters)");
  return rc;
}
