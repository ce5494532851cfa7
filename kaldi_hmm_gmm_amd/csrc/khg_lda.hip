// kaldi_hmm_gmm_amd/csrc/khg_lda.hip -- LDA on spliced features (splice-feats, acc-lda, transform-feats): the statistics
// handle (khg_lda_stats), its accumulation from posteriors resident on the device and the fused splice-and-project of a set's rows.
// The estimate (khg_lda_compute) is host code and lives in khg_host.cpp.  gfx950 only.
#include "khg_internal.hpp"

#include <hipcub/hipcub.hpp>   // DeviceRadixSort: the stable (pdf, entry) sort of the class sums, as K3's bucketing

#include "khg_lda_stats.hip.inc"
#include "khg_lda_transform.hip.inc"

struct khg_lda_stats {
  khg_ctx* ctx = nullptr;
  int32_t C = 0, D = 0, L = 0, R = 0, Dz = 0;
  int64_t SZ2 = 0, SZ = 0;           // doubles of the packed second-order term / of the whole block: zero | first | second
  double* buf_d = nullptr;           // [SZ]
  double* call_d = nullptr;          // [SZ] the sums of the call in progress
  // scratch of the accumulation (grown on demand, kept)
  int64_t chunk_frames = int64_t(1) << 18;
  int32_t *row_lo_d = nullptr, *row_hi_d = nullptr; double* row_w_d = nullptr; size_t row_cap = 0;
  int32_t* pos_row_d = nullptr; size_t pos_cap = 0;
  double* part_d = nullptr; size_t part_cap = 0;
  int32_t* cstart_d = nullptr;
  LdSeg* segs_d = nullptr; size_t segs_cap = 0;
  LdItem* items_d = nullptr; size_t items_cap = 0;
  LdUnit* units_d = nullptr; int32_t nunits = 0;
  LdCItem* citems_d = nullptr; size_t citems_cap = 0;
  LdCRun* cruns_d = nullptr; size_t cruns_cap = 0;
  int32_t n_chunks_last = 0;
};

static inline int ld_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(4096, (n + 255) / 256)); }
constexpr int64_t LD_PARK_BYTES = int64_t(256) << 20;   // parked slice images of one chunk (7l's cap)

template <class T>
static int ld_grow(T** p, size_t* cap, size_t need) {
  if (need <= *cap && *p) return KHG_OK;
  DEVFREE(*p); *cap = 0;
  int rc = dev_alloc(p, need);
  if (rc) return rc;
  *cap = need;
  return KHG_OK;
}

extern "C" int khg_lda_stats_create(khg_ctx* ctx, int32_t num_classes, int32_t dim, int32_t left, int32_t right, khg_lda_stats** out) {
  if (ctx_dead(ctx) || !out || num_classes < 1 || dim < 1 || left < 0 || right < 0) return khg_set_error(KHG_E_ARG, "khg_lda_stats_create: bad arguments");
  const int64_t Dz = (int64_t)dim * ((int64_t)left + right + 1);
  if (Dz > KHG_LDA_MAX_SPLICED_DIM)
    return khg_set_error(KHG_E_UNSUPPORTED, "khg_lda_stats_create: spliced dim " + std::to_string(Dz) + " is above KHG_LDA_MAX_SPLICED_DIM (" +
                                                std::to_string(KHG_LDA_MAX_SPLICED_DIM) + ")");
  khg_lda_stats* s = new khg_lda_stats();
  s->ctx = ctx; s->C = num_classes; s->D = dim; s->L = left; s->R = right; s->Dz = (int32_t)Dz;
  s->SZ2 = Dz * (Dz + 1) / 2; s->SZ = (int64_t)num_classes * (1 + Dz) + s->SZ2;
  // the wave units of the triangle: tile row ti, up to LD_CT column tiles each; the widest first, so that the four waves of a
  // workgroup carry like loads
  std::vector<LdUnit> units;
  const int NTz = (int)((Dz + 15) / 16);
  for (int ti = 0; ti < NTz; ++ti)
    for (int tj0 = 0; tj0 <= ti; tj0 += LD_CT) units.push_back(LdUnit{ti, tj0, std::min(LD_CT, ti + 1 - tj0), 0});
  std::stable_sort(units.begin(), units.end(), [](const LdUnit& a, const LdUnit& b) { return a.ntj > b.ntj; });
  s->nunits = (int32_t)units.size();
  int rc = dev_alloc(&s->buf_d, (size_t)s->SZ);
  if (!rc) rc = dev_alloc(&s->call_d, (size_t)s->SZ);
  if (!rc) rc = dev_alloc(&s->cstart_d, (size_t)num_classes + 1);
  if (!rc) rc = dev_alloc(&s->units_d, units.size());
  if (!rc) {
    hipError_t e = hipMemcpyAsync(s->units_d, units.data(), sizeof(LdUnit) * units.size(), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) rc = khg_set_error(KHG_E_HIP, std::string("khg_lda_stats_create: ") + hipGetErrorString(e));
  }
  if (rc) { (void)khg_lda_stats_destroy(s); return rc; }
  *out = s;
  return khg_lda_stats_zero(ctx, s);
}
extern "C" int khg_lda_stats_destroy(khg_lda_stats* s) {
  if (!s) return KHG_OK;
  DEVFREE(s->buf_d); DEVFREE(s->call_d); DEVFREE(s->row_lo_d); DEVFREE(s->row_hi_d); DEVFREE(s->row_w_d); DEVFREE(s->pos_row_d); DEVFREE(s->part_d);
  DEVFREE(s->cstart_d); DEVFREE(s->segs_d); DEVFREE(s->items_d); DEVFREE(s->units_d); DEVFREE(s->citems_d); DEVFREE(s->cruns_d);
  delete s;
  return KHG_OK;
}
extern "C" int khg_lda_stats_zero(khg_ctx* ctx, khg_lda_stats* s) {
  if (ctx_dead(ctx) || !s || s->ctx != ctx) return khg_set_error(KHG_E_ARG, "khg_lda_stats_zero: bad arguments");
  HIPCHK(hipMemsetAsync(s->buf_d, 0, sizeof(double) * (size_t)s->SZ, ctx->stream));
  return KHG_OK;
}
extern "C" int khg_lda_stats_set_chunk_frames(khg_lda_stats* s, int64_t frames) {
  if (!s || frames < 1) return khg_set_error(KHG_E_ARG, "khg_lda_stats_set_chunk_frames: bad arguments");
  s->chunk_frames = std::min<int64_t>(frames, int64_t(1) << 24);
  return KHG_OK;
}
extern "C" int khg_lda_stats_num_chunks(const khg_lda_stats* s, int32_t* n) {
  if (!s || !n) return khg_set_error(KHG_E_ARG, "khg_lda_stats_num_chunks: bad arguments");
  *n = s->n_chunks_last;
  return KHG_OK;
}
extern "C" int khg_lda_stats_download(khg_ctx* ctx, const khg_lda_stats* s, double* zero_h, double* first_h, double* second_h) {
  if (ctx_dead(ctx) || !s || s->ctx != ctx) return khg_set_error(KHG_E_ARG, "khg_lda_stats_download: bad arguments");
  { int rc = check_err_flag(ctx, "khg_acc_lda_stats_post"); if (rc) return rc; }
  const size_t nz = (size_t)s->C, nf = (size_t)s->C * s->Dz;
  if (zero_h) HIPCHK(hipMemcpyAsync(zero_h, s->buf_d, sizeof(double) * nz, hipMemcpyDeviceToHost, ctx->stream));
  if (first_h) HIPCHK(hipMemcpyAsync(first_h, s->buf_d + nz, sizeof(double) * nf, hipMemcpyDeviceToHost, ctx->stream));
  if (second_h) HIPCHK(hipMemcpyAsync(second_h, s->buf_d + nz + nf, sizeof(double) * (size_t)s->SZ2, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return KHG_OK;
}
extern "C" int khg_lda_stats_upload(khg_ctx* ctx, khg_lda_stats* s, const double* zero_h, const double* first_h, const double* second_h) {
  if (ctx_dead(ctx) || !s || s->ctx != ctx || !zero_h || !first_h || !second_h) return khg_set_error(KHG_E_ARG, "khg_lda_stats_upload: bad arguments");
  const size_t nz = (size_t)s->C, nf = (size_t)s->C * s->Dz;
  HIPCHK(hipMemcpyAsync(s->buf_d, zero_h, sizeof(double) * nz, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(s->buf_d + nz, first_h, sizeof(double) * nf, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(s->buf_d + nz + nf, second_h, sizeof(double) * (size_t)s->SZ2, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return KHG_OK;
}
extern "C" int khg_lda_stats_add(khg_ctx* ctx, khg_lda_stats* dst, float scale, const khg_lda_stats* src) {
  if (ctx_dead(ctx) || !dst || !src) return khg_set_error(KHG_E_ARG, "khg_lda_stats_add: bad arguments");
  if (!std::isfinite(scale)) return khg_set_error(KHG_E_ARG, "khg_lda_stats_add: the scale is not finite");
  if (dst->ctx != ctx || src->ctx != ctx) return khg_set_error(KHG_E_ARG, "khg_lda_stats_add: a handle of another context");
  if (dst->C != src->C || dst->D != src->D || dst->L != src->L || dst->R != src->R)
    return khg_set_error(KHG_E_ARG, "khg_lda_stats_add: the two handles differ in classes, dimension or context frames");
  if (dst == src) return khg_set_error(KHG_E_ARG, "khg_lda_stats_add: dst and src are the same handle");
  KernelTimer kt(ctx, "k_lda_axpy");
  KHG_LAUNCH(ctx, k_lda_axpy, dim3(ld_grid(dst->SZ)), dim3(256), 0, ctx->stream, dst->buf_d, src->buf_d, (double)scale, dst->SZ);
  HIPCHK(hipGetLastError());
  return KHG_OK;
}

// acc-lda from posteriors resident on the device: every check on the host first (khg_acc_stats_post's refusals; the handle keeps its
// bits), then the pipeline of khg_lda_stats.hip.inc on the context's stream.  One word per class is read back for the class plan.
extern "C" int khg_acc_lda_stats_post(khg_ctx* ctx, const khg_tm* tm, khg_utts* u, const khg_posteriors* p, float scale, khg_lda_stats* st) {
  const char* name = "khg_acc_lda_stats_post";
  const std::string who = std::string(name) + ": ";
  if (ctx_dead(ctx) || !tm || !u || !p || !st) return khg_set_error(KHG_E_ARG, who + "bad arguments");
  { int rf = utts_foreign_ctx(ctx, u, name); if (rf) return rf; }
  PostInfo pi;
  posteriors_info(p, &pi);
  if (pi.ctx != ctx || tm->ctx != ctx || st->ctx != ctx || u->ctx != ctx) return khg_set_error(KHG_E_ARG, who + "a handle of another context");
  if (pi.U != u->n_utt)
    return khg_set_error(KHG_E_ARG, who + "the posteriors hold " + std::to_string(pi.U) + " utterances, the set " + std::to_string(u->n_utt));
  for (int i = 0; i < pi.U; ++i) {
    const int64_t tp = pi.frame_off[i + 1] - pi.frame_off[i], ts = u->frame_off[(size_t)i + 1] - u->frame_off[(size_t)i];
    if (tp != 0 && tp != ts)
      return khg_set_error(KHG_E_ARG, who + "utterance " + std::to_string(i) + " has " + std::to_string(tp) + " frames of posteriors and " + std::to_string(ts) + " frames of features");
  }
  if (st->D != u->D) return khg_set_error(KHG_E_ARG, who + "the statistics are of dimension " + std::to_string(st->D) + ", the features of " + std::to_string(u->D));
  if (st->C != tm->max_pdf + 1)
    return khg_set_error(KHG_E_ARG, who + "the statistics hold " + std::to_string(st->C) + " classes, the transition model has " + std::to_string(tm->max_pdf + 1) + " pdfs");
  if (!std::isfinite(scale)) return khg_set_error(KHG_E_ARG, who + "scale must be finite");
  if (pi.max_tid > tm->num_tids)
    return khg_set_error(KHG_E_ARG, who + "the posteriors hold transition-id " + std::to_string(pi.max_tid) + ", the transition model has " + std::to_string(tm->num_tids));
  const int64_t E = pi.entry_off[pi.U];
  if (E >= (int64_t)INT_MAX || u->N >= (int64_t)INT_MAX) return khg_set_error(KHG_E_UNSUPPORTED, who + "2^31 - 1 or more entries or frames");
  st->n_chunks_last = 0;
  if (E == 0) return KHG_OK;

  // ---- the frame plan: the utterances with frames in the handle, in set order, cut into slices of LD_SLICE frames; chunks of whole slices ----
  const int D = st->D, Dz = st->Dz, C = st->C;
  const int64_t CF = std::max<int64_t>(st->chunk_frames, LD_SLICE);
  const int64_t CI = std::max<int64_t>(1, std::min<int64_t>(std::max<int64_t>(1, CF / LD_SLICE), LD_PARK_BYTES / (8 * st->SZ2)));
  struct Chunk { size_t seg0, seg1, item0, item1; int64_t frames; };
  std::vector<LdSeg> segs; std::vector<LdItem> items; std::vector<Chunk> chunks;
  {
    std::vector<int32_t> utts;
    int64_t left = 0;
    for (int i = 0; i < pi.U; ++i)
      if (pi.frame_off[i + 1] > pi.frame_off[i]) { utts.push_back(i); left += u->frame_off[(size_t)i + 1] - u->frame_off[(size_t)i]; }
    Chunk cur{0, 0, 0, 0, 0};
    auto close_chunk = [&] {
      cur.seg1 = segs.size(); cur.item1 = items.size();
      if (cur.item1 > cur.item0) chunks.push_back(cur);
      cur = Chunk{segs.size(), segs.size(), items.size(), items.size(), 0};
    };
    size_t k = 0; int64_t used = 0;
    while (left > 0) {
      const int n = (int)std::min<int64_t>(left, LD_SLICE);
      if ((int64_t)(items.size() - cur.item0) >= CI) close_chunk();
      items.push_back(LdItem{(int32_t)cur.frames, n, (int32_t)(items.size() - cur.item0), 0});
      int need = n;
      while (need > 0) {
        const int32_t ui = utts[k];
        const int64_t T = u->frame_off[(size_t)ui + 1] - u->frame_off[(size_t)ui];
        const int take = (int)std::min<int64_t>(need, T - used);
        segs.push_back(LdSeg{(int32_t)(u->frame_off[(size_t)ui] + used), take, (int32_t)cur.frames, 0});
        cur.frames += take; used += take; need -= take;
        if (used == T) { ++k; used = 0; }
      }
      left -= n;
    }
    close_chunk();
  }
  if (chunks.empty()) return KHG_OK;

  int rc = arena_flush(ctx);
  if (rc) return rc;
  rc = utts_grow_pe(u, (size_t)E);
  if (rc) return rc;
  int64_t maxf = 0; size_t maxi = 0;
  for (const Chunk& c : chunks) { maxf = std::max(maxf, c.frames); maxi = std::max(maxi, c.item1 - c.item0); }
  if ((size_t)u->N > st->row_cap) {
    DEVFREE(st->row_lo_d); DEVFREE(st->row_hi_d); DEVFREE(st->row_w_d);
    st->row_cap = 0;
    rc = dev_alloc(&st->row_lo_d, (size_t)u->N);
    if (!rc) rc = dev_alloc(&st->row_hi_d, (size_t)u->N);
    if (!rc) rc = dev_alloc(&st->row_w_d, (size_t)u->N);
    if (!rc) st->row_cap = (size_t)u->N;
  }
  // the class slices of a chunk: as many as the parked images' cap admits
  const int64_t CCI = std::max<int64_t>(1, LD_PARK_BYTES / (8 * (int64_t)(Dz + 1)));
  const int64_t max_cslices = std::min<int64_t>(CCI, E / LD_SLICE + std::min<int64_t>(C, E) + 1);
  if (!rc) rc = ld_grow(&st->pos_row_d, &st->pos_cap, (size_t)maxf);
  if (!rc) rc = ld_grow(&st->part_d, &st->part_cap, std::max(maxi * (size_t)st->SZ2, (size_t)max_cslices * (size_t)(Dz + 1)));
  if (!rc) rc = ld_grow(&st->segs_d, &st->segs_cap, segs.size());
  if (!rc) rc = ld_grow(&st->items_d, &st->items_cap, items.size());
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(st->segs_d, segs.data(), sizeof(LdSeg) * segs.size(), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(st->items_d, items.data(), sizeof(LdItem) * items.size(), hipMemcpyHostToDevice, ctx->stream));
  ctx->pageable_pending = true;

  rc = posteriors_flatten(ctx, p, u->frame_off_d, (double)scale, tm->num_tids, u->pe_row_d, u->pe_tid_d, u->pe_w_d, 0);
  if (rc) return rc;
  HIPCHK(hipMemsetAsync(st->row_w_d, 0, sizeof(double) * (size_t)u->N, ctx->stream));
  HIPCHK(hipMemsetAsync(st->call_d, 0, sizeof(double) * (size_t)st->SZ, ctx->stream));
  LdArgs a;
  a.feats = u->feats_d; a.D = D; a.L = st->L; a.R = st->R; a.Dz = Dz; a.C = C; a.N = u->N;
  a.frame_off = u->frame_off_d; a.n_utt = u->n_utt;
  a.id2pdf = tm->id2pdf_d; a.num_tids = tm->num_tids;
  a.e_row = u->pe_row_d; a.e_tid = u->pe_tid_d; a.e_w = u->pe_w_d; a.E = E;
  a.row_lo = st->row_lo_d; a.row_hi = st->row_hi_d; a.row_w = st->row_w_d; a.pos_row = st->pos_row_d; a.part = st->part_d;
  a.err_flag = ctx->err_flag_d;
  uint32_t* skeys = u->pe_keys_out_d;
  uint32_t* svals = reinterpret_cast<uint32_t*>(u->pe_ids_d);
  {
    KernelTimer kt(ctx, "k_lda_rows");
    KHG_LAUNCH(ctx, k_lda_rowutt, dim3((unsigned)std::max(1, std::min(u->n_utt, 8192))), dim3(256), 0, ctx->stream, a);
    KHG_LAUNCH(ctx, k_lda_roww, dim3(ld_grid(E)), dim3(256), 0, ctx->stream, a);
    HIPCHK(hipGetLastError());
  }
  {
    KernelTimer kt(ctx, "k_lda_bucket");
    int sort_bits = 1;
    while ((1 << sort_bits) <= C) ++sort_bits;           // keys are 0 .. C
    size_t need = 0;
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, need, u->pe_keys_d, skeys, u->pe_vals_d, svals, (int)E, 0, sort_bits, ctx->stream));
    if (need > u->pe_tmp_bytes) {
      DEVFREE(u->pe_tmp_d);
      { int rt = u_alloc(u, reinterpret_cast<char**>(&u->pe_tmp_d), need); if (rt) return rt; }
      u->pe_tmp_bytes = need;
    }
    KHG_LAUNCH(ctx, k_lda_keys, dim3(ld_grid(E)), dim3(256), 0, ctx->stream, a, u->pe_keys_d, u->pe_vals_d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(u->pe_tmp_d, need, u->pe_keys_d, skeys, u->pe_vals_d, svals, (int)E, 0, sort_bits, ctx->stream));
    KHG_LAUNCH(ctx, k_lda_bounds, dim3((unsigned)((C + 1 + 255) / 256)), dim3(256), 0, ctx->stream, skeys, E, C, st->cstart_d);
    HIPCHK(hipGetLastError());
  }
  std::vector<int32_t> cstart((size_t)C + 1);
  HIPCHK(hipMemcpyAsync(cstart.data(), st->cstart_d, sizeof(int32_t) * cstart.size(), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));                // the bounds are down, the plan's host vectors are free again
  ctx->pageable_pending = false;

  // ---- the class sums: slices of <= LD_SLICE sorted entries of one class, chunks of <= max_cslices parked images ----
  {
    std::vector<LdCItem> ci; std::vector<LdCRun> cr;
    struct CChunk { size_t i0, i1, r0, r1; };
    std::vector<CChunk> cc;
    size_t i0 = 0, r0 = 0;
    auto close_c = [&] {
      if (ci.size() > i0) cc.push_back(CChunk{i0, ci.size(), r0, cr.size()});
      i0 = ci.size(); r0 = cr.size();
    };
    for (int c = 0; c < C; ++c)
      for (int32_t e0 = cstart[(size_t)c]; e0 < cstart[(size_t)c + 1]; e0 += LD_SLICE) {
        if ((int64_t)(ci.size() - i0) >= max_cslices) close_c();
        const int slot = (int)(ci.size() - i0);
        ci.push_back(LdCItem{c, e0, std::min<int32_t>(LD_SLICE, cstart[(size_t)c + 1] - e0), slot});
        if (cr.size() > r0 && cr.back().cls == c) cr.back().nslot++;
        else cr.push_back(LdCRun{c, slot, 1, 0});
      }
    close_c();
    if (!ci.empty()) {
      rc = ld_grow(&st->citems_d, &st->citems_cap, ci.size());
      if (!rc) rc = ld_grow(&st->cruns_d, &st->cruns_cap, cr.size());
      if (rc) return rc;
      HIPCHK(hipMemcpyAsync(st->citems_d, ci.data(), sizeof(LdCItem) * ci.size(), hipMemcpyHostToDevice, ctx->stream));
      HIPCHK(hipMemcpyAsync(st->cruns_d, cr.data(), sizeof(LdCRun) * cr.size(), hipMemcpyHostToDevice, ctx->stream));
      for (const CChunk& c : cc) {
        KernelTimer kt(ctx, "k_lda_class");
        KHG_LAUNCH(ctx, k_lda_class, dim3((unsigned)(c.i1 - c.i0)), dim3(256), 0, ctx->stream, a, st->citems_d + c.i0, svals);
        KHG_LAUNCH(ctx, k_lda_creduce, dim3((unsigned)(c.r1 - c.r0)), dim3(256), 0, ctx->stream, st->cruns_d + c.r0, st->part_d, st->call_d, C, Dz);
        HIPCHK(hipGetLastError());
      }
      HIPCHK(hipStreamSynchronize(ctx->stream));            // ci / cr go out of scope
    }
  }

  // ---- the second-order term ----
  const int NTz = (Dz + 15) / 16, ZS = (16 * NTz) | 1;
  const size_t lds_gram = sizeof(double) * LD_TB + sizeof(float) * (size_t)LD_TB * (size_t)ZS;
  if (lds_gram > 48 * 1024) HIPCHK(hipFuncSetAttribute((const void*)k_lda_gram, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_gram));
  double* call2 = st->call_d + (int64_t)C * (1 + Dz);
  for (const Chunk& c : chunks) {
    const int nseg = (int)(c.seg1 - c.seg0), nit = (int)(c.item1 - c.item0);
    {
      KernelTimer kt(ctx, "k_lda_posrow");
      KHG_LAUNCH(ctx, k_lda_posrow, dim3((unsigned)std::min(nseg, 4096)), dim3(256), 0, ctx->stream, st->segs_d + c.seg0, nseg, st->pos_row_d);
      HIPCHK(hipGetLastError());
    }
    {
      KernelTimer kt(ctx, "k_lda_gram");
      KHG_LAUNCH(ctx, k_lda_gram, dim3((unsigned)nit, (unsigned)((st->nunits + 3) / 4)), dim3(256), lds_gram, ctx->stream, a, st->items_d + c.item0,
                 st->units_d, st->nunits, ZS, st->SZ2);
      HIPCHK(hipGetLastError());
    }
    {
      KernelTimer kt(ctx, "k_lda_reduce");
      KHG_LAUNCH(ctx, k_lda_reduce, dim3(ld_grid(st->SZ2)), dim3(256), 0, ctx->stream, st->part_d, nit, call2, st->SZ2);
      HIPCHK(hipGetLastError());
    }
  }
  {
    KernelTimer kt(ctx, "k_lda_axpy");
    KHG_LAUNCH(ctx, k_lda_axpy, dim3(ld_grid(st->SZ)), dim3(256), 0, ctx->stream, st->buf_d, st->call_d, 1.0, st->SZ);
    HIPCHK(hipGetLastError());
  }
  st->n_chunks_last = (int32_t)chunks.size();
  return KHG_OK;
}

// splice-feats | transform-feats lda.mat: the rows of every utterance, spliced and projected, out of place.  M_h (host, [out_dim]
// [Dz + has_offset]) or NULL for the spliced rows themselves (out_dim = Dz); out_d: a caller's device buffer [rows][out_dim].
extern "C" int khg_utts_splice_transform_feats(khg_ctx* ctx, khg_utts* u, int32_t left, int32_t right, int32_t out_dim, int32_t has_offset,
                                               const float* M_h, float* out_d) {
  const std::string who = "khg_utts_splice_transform_feats: ";
  if (ctx_dead(ctx) || !u || !out_d || left < 0 || right < 0 || out_dim < 1) return khg_set_error(KHG_E_ARG, who + "bad arguments");
  { int rf = utts_foreign_ctx(ctx, u, "khg_utts_splice_transform_feats"); if (rf) return rf; }
  if (u->ctx != ctx) return khg_set_error(KHG_E_ARG, who + "a handle of another context");
  const int D = u->D;
  const int64_t Dz64 = (int64_t)D * ((int64_t)left + right + 1);
  if (Dz64 > KHG_LDA_MAX_SPLICED_DIM)
    return khg_set_error(KHG_E_UNSUPPORTED, who + "spliced dim " + std::to_string(Dz64) + " is above KHG_LDA_MAX_SPLICED_DIM (" + std::to_string(KHG_LDA_MAX_SPLICED_DIM) + ")");
  const int Dz = (int)Dz64;
  if (!M_h && out_dim != Dz) return khg_set_error(KHG_E_ARG, who + "without a matrix out_dim must be the spliced dim " + std::to_string(Dz));
  const int MS = (Dz + 1) | 1, MW = Dz + (has_offset ? 1 : 0);
  const size_t lds = sizeof(float) * ((size_t)(LT_ROWS + left + right) * D + (M_h ? (size_t)out_dim * MS : 0));
  if (lds > KHG_LDA_TRANSFORM_LDS_BYTES)
    return khg_set_error(KHG_E_UNSUPPORTED, who + "out_dim " + std::to_string(out_dim) + " at spliced dim " + std::to_string(Dz) + " needs " + std::to_string(lds) +
                                                " bytes of LDS for the matrix and the rows, above the " + std::to_string(KHG_LDA_TRANSFORM_LDS_BYTES) + " the kernel stages");
  if (u->N == 0) return KHG_OK;
  std::vector<LtItem> items;
  for (int i = 0; i < u->n_utt; ++i) {
    const int64_t f0 = u->frame_off[(size_t)i], f1 = u->frame_off[(size_t)i + 1];
    for (int64_t r = f0; r < f1; r += LT_ROWS) items.push_back(LtItem{r, (int32_t)std::min<int64_t>(LT_ROWS, f1 - r), (int32_t)f0, (int32_t)(f1 - 1), 0});
  }
  if (items.size() >= (size_t)INT_MAX || u->N >= (int64_t)INT_MAX) return khg_set_error(KHG_E_UNSUPPORTED, who + "too many rows");
  int rc = arena_flush(ctx);
  if (rc) return rc;
  LtItem* items_d = nullptr; float* M_d = nullptr;
  auto cleanup = [&] { DEVFREE(items_d); DEVFREE(M_d); };
  rc = dev_alloc(&items_d, items.size());
  if (!rc && M_h) rc = dev_alloc(&M_d, (size_t)out_dim * MW);
  if (rc) { cleanup(); return rc; }
  hipError_t e = hipMemcpyAsync(items_d, items.data(), sizeof(LtItem) * items.size(), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess && M_h) e = hipMemcpyAsync(M_d, M_h, sizeof(float) * (size_t)out_dim * MW, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess && lds > 48 * 1024) e = hipFuncSetAttribute((const void*)k_lda_splice_transform, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) { cleanup(); return khg_set_error(KHG_E_HIP, who + hipGetErrorString(e)); }
  {
    KernelTimer kt(ctx, "k_lda_splice_transform");
    KHG_LAUNCH(ctx, k_lda_splice_transform, dim3((unsigned)items.size()), dim3(256), lds, ctx->stream, items_d, M_d, has_offset ? 1 : 0, u->feats_d, out_d, D, left,
               right, out_dim, MS);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);     // the temporaries and the caller's host array are free again
  cleanup();
  if (e != hipSuccess) return khg_set_error(KHG_E_HIP, who + hipGetErrorString(e));
  return KHG_OK;
}
