// kaldi_hmm_gmm_amd/csrc/khg_tree.hip -- decision-tree statistics (acc-tree-stats): the handle khg_tree_stats (a sorted
// list of event keys with their count / x / x2 sums, fp64, resident on the device), its accumulation from a set's resident alignment
// and feature rows, and the key-union merge.  The tree building itself (khg_build_tree) is host code: khg_host_tree.cpp.  gfx950 only.
#include "khg_internal.hpp"

#include <hipcub/hipcub.hpp>   // DeviceRadixSort (stable, as K3 / fMLLR / LDA use it) and DeviceScan

#include "khg_tree_stats.hip.inc"

struct khg_tree_stats {
  khg_ctx* ctx = nullptr;
  int32_t D = 0, N = 0, P = 0;
  int64_t K = 0;                      // distinct keys held
  uint64_t* key_d = nullptr;          // [K] ascending; window[j] at bits 8 + 16 (N - 1 - j), pdf-class in the low 8
  double *cnt_d = nullptr, *x_d = nullptr, *x2_d = nullptr;
  // scratch of the accumulation and of the merge (grown on demand, kept)
  size_t fr_cap = 0;
  int32_t *tmp_d = nullptr, *seg_start_d = nullptr, *seg_end_d = nullptr, *head_d = nullptr, *inc_d = nullptr, *kstart_d = nullptr;
  uint64_t *skey_d = nullptr, *skey_out_d = nullptr, *kkey_d = nullptr;
  uint32_t *sval_d = nullptr, *sval_out_d = nullptr;
  void* cub_d = nullptr; size_t cub_bytes = 0;
  int32_t* status_d = nullptr; size_t status_cap = 0;
  uint32_t* tidinfo_d = nullptr; size_t tidinfo_cap = 0;
};

// HIPCHK for the stretches where an asynchronous copy to or from a pageable host vector of the caller's frame may be in flight: the
// stream is drained before the error is returned, so the vector is not read or written after it is gone
#define TR_HIPCHK_DRAIN(expr)                                                                \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess) {                                                                  \
      (void)hipStreamSynchronize(ctx->stream);                                               \
      ctx->pageable_pending = false;                                                         \
      return khg_set_error(KHG_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));    \
    }                                                                                        \
  } while (0)

static inline int tr_grid(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(4096, (n + 255) / 256)); }

template <class T>
static int tr_grow(T** p, size_t* cap, size_t need) {
  if (need <= *cap && *p) return KHG_OK;
  DEVFREE(*p); *cap = 0;
  int rc = dev_alloc(p, need);
  if (rc) return rc;
  *cap = need;
  return KHG_OK;
}
// the per-entry scratch, for n sorted entries
static int tr_grow_entries(khg_tree_stats* s, size_t n) {
  if (n <= s->fr_cap) return KHG_OK;
  DEVFREE(s->tmp_d); DEVFREE(s->seg_start_d); DEVFREE(s->seg_end_d); DEVFREE(s->head_d); DEVFREE(s->inc_d); DEVFREE(s->kstart_d);
  DEVFREE(s->skey_d); DEVFREE(s->skey_out_d); DEVFREE(s->kkey_d); DEVFREE(s->sval_d); DEVFREE(s->sval_out_d);
  s->fr_cap = 0;
  int rc = dev_alloc(&s->tmp_d, n);
  if (!rc) rc = dev_alloc(&s->seg_start_d, n);
  if (!rc) rc = dev_alloc(&s->seg_end_d, n);
  if (!rc) rc = dev_alloc(&s->head_d, n);
  if (!rc) rc = dev_alloc(&s->inc_d, n);
  if (!rc) rc = dev_alloc(&s->kstart_d, n + 1);
  if (!rc) rc = dev_alloc(&s->skey_d, n);
  if (!rc) rc = dev_alloc(&s->skey_out_d, n);
  if (!rc) rc = dev_alloc(&s->kkey_d, n);
  if (!rc) rc = dev_alloc(&s->sval_d, n);
  if (!rc) rc = dev_alloc(&s->sval_out_d, n);
  if (rc) return rc;
  s->fr_cap = n;
  return KHG_OK;
}
static void tr_free_keys(khg_tree_stats* s) {
  DEVFREE(s->key_d); DEVFREE(s->cnt_d); DEVFREE(s->x_d); DEVFREE(s->x2_d);
  s->K = 0;
}
static inline bool tr_bad_shape(int64_t N, int64_t P) { return N < 1 || N > KHG_TREE_MAX_CONTEXT || P < 0 || P >= N; }
static inline int tr_bits(uint32_t v) { int b = 1; while ((v >> b) != 0) ++b; return b; }

// sorts skey / sval (n entries, `bits` low bits), marks heads and scans them: the sorted lists are skey_out / sval_out, *K the number of
// distinct keys below `sentinel` (read back: synchronises)
static int tr_sort_heads(khg_ctx* ctx, khg_tree_stats* s, int64_t n, int bits, uint64_t sentinel, int32_t* K) {
  size_t need_sort = 0, need_scan = 0;
  HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, need_sort, s->skey_d, s->skey_out_d, s->sval_d, s->sval_out_d, (int)n, 0, bits, ctx->stream));
  HIPCHK(hipcub::DeviceScan::InclusiveSum(nullptr, need_scan, s->head_d, s->inc_d, (int)n, ctx->stream));
  const size_t need = std::max(need_sort, need_scan);
  if (need > s->cub_bytes || !s->cub_d) {
    DEVFREE(s->cub_d); s->cub_bytes = 0;
    char* p = nullptr;
    int rc = dev_alloc(&p, need);
    if (rc) return rc;
    s->cub_d = p; s->cub_bytes = std::max<size_t>(need, 1);
  }
  {
    KernelTimer kt(ctx, "k_tree_sort");
    size_t b = s->cub_bytes;
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(s->cub_d, b, s->skey_d, s->skey_out_d, s->sval_d, s->sval_out_d, (int)n, 0, bits, ctx->stream));
  }
  {
    KernelTimer kt(ctx, "k_tree_heads");
    KHG_LAUNCH(ctx, k_tree_heads, dim3(tr_grid(n)), dim3(256), 0, ctx->stream, s->skey_out_d, n, sentinel, s->head_d);
    HIPCHK(hipGetLastError());
    size_t b = s->cub_bytes;
    HIPCHK(hipcub::DeviceScan::InclusiveSum(s->cub_d, b, s->head_d, s->inc_d, (int)n, ctx->stream));
  }
  HIPCHK(hipMemcpyAsync(K, s->inc_d + (n - 1), sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return KHG_OK;
}

// dst = dst (+) scale * (bkey, b): concatenate, stable sort, reduce by key.  b's arrays are the caller's; with an empty dst and scale 1
// they are adopted when `adopt` is set (the same bits as the merge gives: 1.0 * v = v).
static int tr_merge(khg_ctx* ctx, khg_tree_stats* dst, double scale, uint64_t** bkey, double** bcnt, double** bx, double** bx2, int64_t Kb, bool adopt) {
  if (Kb == 0) return KHG_OK;
  const int D = dst->D;
  if (dst->K == 0 && scale == 1.0 && adopt) {
    tr_free_keys(dst);
    dst->key_d = *bkey; dst->cnt_d = *bcnt; dst->x_d = *bx; dst->x2_d = *bx2; dst->K = Kb;
    *bkey = nullptr; *bcnt = nullptr; *bx = nullptr; *bx2 = nullptr;
    return KHG_OK;
  }
  const int64_t Ka = dst->K, M = Ka + Kb;
  if (M >= (int64_t)INT_MAX) return khg_set_error(KHG_E_UNSUPPORTED, "khg_tree_stats: 2^31 - 1 or more keys");
  int rc = tr_grow_entries(dst, (size_t)M);
  if (rc) return rc;
  if (Ka) HIPCHK(hipMemcpyAsync(dst->skey_d, dst->key_d, sizeof(uint64_t) * (size_t)Ka, hipMemcpyDeviceToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(dst->skey_d + Ka, *bkey, sizeof(uint64_t) * (size_t)Kb, hipMemcpyDeviceToDevice, ctx->stream));
  KHG_LAUNCH(ctx, k_tree_iota, dim3(tr_grid(M)), dim3(256), 0, ctx->stream, dst->sval_d, M);
  HIPCHK(hipGetLastError());
  int32_t Kn = 0;
  rc = tr_sort_heads(ctx, dst, M, 8 + 16 * dst->N, ~uint64_t(0), &Kn);
  if (rc) return rc;
  uint64_t* nkey = nullptr; double *ncnt = nullptr, *nx = nullptr, *nx2 = nullptr;
  rc = dev_alloc(&nkey, (size_t)Kn);
  if (!rc) rc = dev_alloc(&ncnt, (size_t)Kn);
  if (!rc) rc = dev_alloc(&nx, (size_t)Kn * D);
  if (!rc) rc = dev_alloc(&nx2, (size_t)Kn * D);
  if (rc) { DEVFREE(nkey); DEVFREE(ncnt); DEVFREE(nx); DEVFREE(nx2); return rc; }
  {
    KernelTimer kt(ctx, "k_tree_merge");
    KHG_LAUNCH(ctx, k_tree_merge, dim3(tr_grid(M * (2 * D + 1))), dim3(256), 0, ctx->stream, dst->skey_out_d, dst->sval_out_d, dst->head_d, dst->inc_d, M, (int32_t)Ka,
               TrSide{dst->cnt_d, dst->x_d, dst->x2_d}, TrSide{*bcnt, *bx, *bx2}, scale, D, nkey, ncnt, nx, nx2);
  }
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);      // the old arrays are read no more
  if (e != hipSuccess) { DEVFREE(nkey); DEVFREE(ncnt); DEVFREE(nx); DEVFREE(nx2); return khg_set_error(KHG_E_HIP, std::string("khg_tree_stats merge: ") + hipGetErrorString(e)); }
  tr_free_keys(dst);
  dst->key_d = nkey; dst->cnt_d = ncnt; dst->x_d = nx; dst->x2_d = nx2; dst->K = Kn;
  return KHG_OK;
}

extern "C" int khg_tree_stats_create(khg_ctx* ctx, int32_t dim, int32_t N, int32_t P, khg_tree_stats** out) {
  if (ctx_dead(ctx) || !out || dim < 1) return khg_set_error(KHG_E_ARG, "khg_tree_stats_create: bad arguments");
  if (tr_bad_shape(N, P))
    return khg_set_error(KHG_E_ARG, "khg_tree_stats_create: context width N = " + std::to_string(N) + ", central position P = " + std::to_string(P) +
                                        ": supported are N in 1 .. " + std::to_string(KHG_TREE_MAX_CONTEXT) + " and 0 <= P < N");
  khg_tree_stats* s = new khg_tree_stats();
  s->ctx = ctx; s->D = dim; s->N = N; s->P = P;
  *out = s;
  return KHG_OK;
}
extern "C" int khg_tree_stats_destroy(khg_tree_stats* s) {
  if (!s) return KHG_OK;
  tr_free_keys(s);
  DEVFREE(s->tmp_d); DEVFREE(s->seg_start_d); DEVFREE(s->seg_end_d); DEVFREE(s->head_d); DEVFREE(s->inc_d); DEVFREE(s->kstart_d);
  DEVFREE(s->skey_d); DEVFREE(s->skey_out_d); DEVFREE(s->kkey_d); DEVFREE(s->sval_d); DEVFREE(s->sval_out_d); DEVFREE(s->cub_d);
  DEVFREE(s->status_d); DEVFREE(s->tidinfo_d);
  delete s;
  return KHG_OK;
}
extern "C" int khg_tree_stats_zero(khg_ctx* ctx, khg_tree_stats* s) {
  if (ctx_dead(ctx) || !s || s->ctx != ctx) return khg_set_error(KHG_E_ARG, "khg_tree_stats_zero: bad arguments");
  HIPCHK(hipStreamSynchronize(ctx->stream));
  tr_free_keys(s);
  return KHG_OK;
}
extern "C" int khg_tree_stats_num_keys(khg_ctx* ctx, const khg_tree_stats* s, int64_t* num_keys) {
  if (ctx_dead(ctx) || !s || s->ctx != ctx || !num_keys) return khg_set_error(KHG_E_ARG, "khg_tree_stats_num_keys: bad arguments");
  *num_keys = s->K;
  return KHG_OK;
}
extern "C" int khg_tree_stats_download(khg_ctx* ctx, const khg_tree_stats* s, int32_t* keys_h, double* count_h, double* x_h, double* x2_h) {
  if (ctx_dead(ctx) || !s || s->ctx != ctx) return khg_set_error(KHG_E_ARG, "khg_tree_stats_download: bad arguments");
  { int rc = check_err_flag(ctx, "khg_acc_tree_stats"); if (rc) return rc; }
  const size_t K = (size_t)s->K;
  std::vector<uint64_t> kk(K);
  if (K) {
    if (keys_h) TR_HIPCHK_DRAIN(hipMemcpyAsync(kk.data(), s->key_d, sizeof(uint64_t) * K, hipMemcpyDeviceToHost, ctx->stream));
    if (count_h) TR_HIPCHK_DRAIN(hipMemcpyAsync(count_h, s->cnt_d, sizeof(double) * K, hipMemcpyDeviceToHost, ctx->stream));
    if (x_h) TR_HIPCHK_DRAIN(hipMemcpyAsync(x_h, s->x_d, sizeof(double) * K * s->D, hipMemcpyDeviceToHost, ctx->stream));
    if (x2_h) TR_HIPCHK_DRAIN(hipMemcpyAsync(x2_h, s->x2_d, sizeof(double) * K * s->D, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (keys_h)
    for (size_t i = 0; i < K; ++i) {
      int32_t* row = keys_h + i * (size_t)(s->N + 1);
      for (int j = 0; j < s->N; ++j) row[j] = (int32_t)((kk[i] >> (8 + 16 * (s->N - 1 - j))) & 0xFFFF);
      row[s->N] = (int32_t)(kk[i] & 0xFF);
    }
  return KHG_OK;
}
extern "C" int khg_tree_stats_upload(khg_ctx* ctx, khg_tree_stats* s, int64_t num_keys, const int32_t* keys_h, const double* count_h, const double* x_h,
                                     const double* x2_h) {
  const std::string who = "khg_tree_stats_upload: ";
  if (ctx_dead(ctx) || !s || s->ctx != ctx || num_keys < 0 || (num_keys > 0 && (!keys_h || !count_h || !x_h || !x2_h))) return khg_set_error(KHG_E_ARG, who + "bad arguments");
  if (num_keys >= (int64_t)INT_MAX) return khg_set_error(KHG_E_UNSUPPORTED, who + "2^31 - 1 or more keys");
  const size_t K = (size_t)num_keys;
  std::vector<uint64_t> kk(K);
  for (size_t i = 0; i < K; ++i) {
    const int32_t* row = keys_h + i * (size_t)(s->N + 1);
    uint64_t k = 0;
    for (int j = 0; j < s->N; ++j) {
      if (row[j] < 0 || row[j] > KHG_TREE_MAX_PHONE) return khg_set_error(KHG_E_ARG, who + "key " + std::to_string(i) + " holds phone " + std::to_string(row[j]));
      k = (k << 16) | (uint64_t)row[j];
    }
    if (row[s->N] < 0 || row[s->N] > KHG_TREE_MAX_PDF_CLASS) return khg_set_error(KHG_E_ARG, who + "key " + std::to_string(i) + " holds pdf-class " + std::to_string(row[s->N]));
    kk[i] = (k << 8) | (uint64_t)row[s->N];
    if (i > 0 && kk[i] <= kk[i - 1]) return khg_set_error(KHG_E_ARG, who + "the keys must ascend strictly; key " + std::to_string(i) + " does not");
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  tr_free_keys(s);
  if (K == 0) return KHG_OK;
  int rc = dev_alloc(&s->key_d, K);
  if (!rc) rc = dev_alloc(&s->cnt_d, K);
  if (!rc) rc = dev_alloc(&s->x_d, K * s->D);
  if (!rc) rc = dev_alloc(&s->x2_d, K * s->D);
  if (rc) { tr_free_keys(s); return rc; }
  TR_HIPCHK_DRAIN(hipMemcpyAsync(s->key_d, kk.data(), sizeof(uint64_t) * K, hipMemcpyHostToDevice, ctx->stream));
  TR_HIPCHK_DRAIN(hipMemcpyAsync(s->cnt_d, count_h, sizeof(double) * K, hipMemcpyHostToDevice, ctx->stream));
  TR_HIPCHK_DRAIN(hipMemcpyAsync(s->x_d, x_h, sizeof(double) * K * s->D, hipMemcpyHostToDevice, ctx->stream));
  TR_HIPCHK_DRAIN(hipMemcpyAsync(s->x2_d, x2_h, sizeof(double) * K * s->D, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  s->K = num_keys;
  return KHG_OK;
}
extern "C" int khg_tree_stats_add(khg_ctx* ctx, khg_tree_stats* dst, float scale, const khg_tree_stats* src) {
  if (ctx_dead(ctx) || !dst || !src) return khg_set_error(KHG_E_ARG, "khg_tree_stats_add: bad arguments");
  if (!std::isfinite(scale)) return khg_set_error(KHG_E_ARG, "khg_tree_stats_add: the scale is not finite");
  if (dst->ctx != ctx || src->ctx != ctx) return khg_set_error(KHG_E_ARG, "khg_tree_stats_add: a handle of another context");
  if (dst->D != src->D || dst->N != src->N || dst->P != src->P) return khg_set_error(KHG_E_ARG, "khg_tree_stats_add: the two handles differ in dimension or context");
  if (dst == src) return khg_set_error(KHG_E_ARG, "khg_tree_stats_add: dst and src are the same handle");
  uint64_t* bk = src->key_d; double *bc = src->cnt_d, *bx = src->x_d, *bx2 = src->x2_d;
  return tr_merge(ctx, dst, (double)scale, &bk, &bc, &bx, &bx2, src->K, false);
}

// acc-tree-stats from the set's resident alignment and feature rows.  Every check on the host first (the handle keeps its bits), then
// the pipeline of khg_tree_stats.hip.inc on the context's stream.  The number of distinct keys and their entry ranges are read back
// for the work plan of the gather.
extern "C" int khg_acc_tree_stats(khg_ctx* ctx, khg_utts* u, int32_t num_tids, const int32_t* tid2phone_h, const int32_t* tid2pdf_class_h,
                                  const int32_t* tid_flags_h, int32_t n_ci, const int32_t* ci_phones_h, khg_tree_stats* st, int32_t* status_h) {
  const char* name = "khg_acc_tree_stats";
  const std::string who = std::string(name) + ": ";
  if (ctx_dead(ctx) || !u || !st || num_tids < 1 || !tid2phone_h || !tid2pdf_class_h || !tid_flags_h || n_ci < 0 || (n_ci > 0 && !ci_phones_h))
    return khg_set_error(KHG_E_ARG, who + "bad arguments");
  { int rf = utts_foreign_ctx(ctx, u, name); if (rf) return rf; }
  if (u->ctx != ctx || st->ctx != ctx) return khg_set_error(KHG_E_ARG, who + "a handle of another context");
  if (tr_bad_shape(st->N, st->P)) return khg_set_error(KHG_E_ARG, who + "unsupported context");
  if (st->D != u->D) return khg_set_error(KHG_E_ARG, who + "the statistics are of dimension " + std::to_string(st->D) + ", the features of " + std::to_string(u->D));
  if (!u->ali_valid || !u->ali_d) return khg_set_error(KHG_E_ARG, who + "the set has no resident alignment (khg_align or khg_ali_upload first)");
  if (u->N >= (int64_t)INT_MAX) return khg_set_error(KHG_E_ARG, who + "2^31 - 1 or more frames");
  std::vector<uint8_t> is_ci((size_t)KHG_TREE_MAX_PHONE + 1, 0);
  for (int i = 0; i < n_ci; ++i) {
    if (ci_phones_h[i] < 1 || ci_phones_h[i] > KHG_TREE_MAX_PHONE) return khg_set_error(KHG_E_ARG, who + "context-independent phone " + std::to_string(ci_phones_h[i]));
    is_ci[(size_t)ci_phones_h[i]] = 1;
  }
  std::vector<uint32_t> info((size_t)num_tids + 1, 0);
  uint32_t max_phone = 0, max_pc = 0;
  for (int t = 1; t <= num_tids; ++t) {
    const int32_t ph = tid2phone_h[t], pc = tid2pdf_class_h[t];
    if (ph < 1 || ph > KHG_TREE_MAX_PHONE)
      return khg_set_error(KHG_E_ARG, who + "transition-id " + std::to_string(t) + " has phone " + std::to_string(ph) + " (supported: 1 .. " + std::to_string(KHG_TREE_MAX_PHONE) + ")");
    if (pc < 0 || pc > KHG_TREE_MAX_PDF_CLASS)
      return khg_set_error(KHG_E_ARG, who + "transition-id " + std::to_string(t) + " has pdf-class " + std::to_string(pc) + " (supported: 0 .. " + std::to_string(KHG_TREE_MAX_PDF_CLASS) + ")");
    if (tid_flags_h[t] & ~(KHG_TREE_TID_SELF_LOOP | KHG_TREE_TID_FINAL)) return khg_set_error(KHG_E_ARG, who + "transition-id " + std::to_string(t) + " has unknown flags");
    info[(size_t)t] = (uint32_t)ph | ((uint32_t)pc << 16) | ((tid_flags_h[t] & KHG_TREE_TID_SELF_LOOP) ? TR_SELF : 0u) | ((tid_flags_h[t] & KHG_TREE_TID_FINAL) ? TR_FINAL : 0u) |
                      (is_ci[(size_t)ph] ? TR_CI : 0u);
    max_phone = std::max(max_phone, (uint32_t)ph); max_pc = std::max(max_pc, (uint32_t)pc);
  }
  const int U = u->n_utt;
  if (status_h) std::fill(status_h, status_h + U, 0);
  if (U == 0 || u->N == 0) return KHG_OK;
  const int64_t E = u->N;
  const int D = st->D;

  int rc = wait_ali(ctx, u);
  if (!rc) rc = arena_flush(ctx);
  if (!rc) rc = tr_grow_entries(st, (size_t)E);
  if (!rc) rc = tr_grow(&st->status_d, &st->status_cap, (size_t)U);
  if (!rc) rc = tr_grow(&st->tidinfo_d, &st->tidinfo_cap, info.size());
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(st->tidinfo_d, info.data(), sizeof(uint32_t) * info.size(), hipMemcpyHostToDevice, ctx->stream));
  ctx->pageable_pending = true;

  TrArgs a;
  a.ali = u->ali_d; a.frame_off = u->frame_off_d; a.n_utt = U; a.tidinfo = st->tidinfo_d; a.num_tids = num_tids;
  a.N = st->N; a.P = st->P; a.bp = tr_bits(max_phone); a.bc = tr_bits(max_pc);
  a.tmp = st->tmp_d; a.seg_start = st->seg_start_d; a.seg_end = st->seg_end_d; a.status = st->status_d;
  a.keys = st->skey_d; a.vals = st->sval_d;
  const int key_bits = a.N * a.bp + a.bc;                   // <= 3 * 16 + 8
  const uint64_t sentinel = uint64_t(1) << key_bits;
  // `info` is being read and `status` written by copies on the stream from here to the synchronisation inside tr_sort_heads: every
  // error return in between drains the stream first
  {
    KernelTimer kt(ctx, "k_tree_segments");
    KHG_LAUNCH(ctx, k_tree_segments, dim3((unsigned)std::min(U, 8192)), dim3(256), 0, ctx->stream, a);
    TR_HIPCHK_DRAIN(hipGetLastError());
  }
  {
    KernelTimer kt(ctx, "k_tree_keys");
    KHG_LAUNCH(ctx, k_tree_keys, dim3((unsigned)std::min(U, 8192)), dim3(256), 0, ctx->stream, a);
    TR_HIPCHK_DRAIN(hipGetLastError());
  }
  std::vector<int32_t> status((size_t)U, 0);
  TR_HIPCHK_DRAIN(hipMemcpyAsync(status.data(), st->status_d, sizeof(int32_t) * (size_t)U, hipMemcpyDeviceToHost, ctx->stream));
  int32_t K = 0;
  rc = tr_sort_heads(ctx, st, E, key_bits + 1, sentinel, &K);      // synchronises: info / status are free again
  if (rc) (void)hipStreamSynchronize(ctx->stream);                 // it may have failed before its own synchronisation
  ctx->pageable_pending = false;
  if (rc) return rc;
  if (status_h) std::copy(status.begin(), status.end(), status_h);
  if (K == 0) return KHG_OK;

  KHG_LAUNCH(ctx, k_tree_starts, dim3(tr_grid(E)), dim3(256), 0, ctx->stream, st->skey_out_d, st->head_d, st->inc_d, E, sentinel, st->N, a.bp, a.bc, st->kstart_d, st->kkey_d);
  HIPCHK(hipGetLastError());
  std::vector<int32_t> kstart((size_t)K + 1);
  HIPCHK(hipMemcpyAsync(kstart.data(), st->kstart_d, sizeof(int32_t) * kstart.size(), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));

  // ---- the work plan: slices of <= TR_SLICE entries of one key; a key of several slices parks them and adds them in slice order ----
  // (keys of <= 256 / dim entries go to k_tree_sum_short, several a workgroup: the same sums, see there)
  std::vector<TrItem> items, shorts; std::vector<TrRun> runs;
  int32_t nslot = 0;
  const int32_t short_n = D <= 256 ? 256 / D : 0;
  for (int32_t k = 0; k < K; ++k) {
    const int32_t e0 = kstart[(size_t)k], e1 = kstart[(size_t)k + 1];
    if (e1 - e0 <= short_n) { shorts.push_back(TrItem{k, e0, e1 - e0, -1}); continue; }
    if (e1 - e0 <= TR_SLICE) { items.push_back(TrItem{k, e0, e1 - e0, -1}); continue; }
    runs.push_back(TrRun{k, nslot, 0, 0});
    for (int32_t e = e0; e < e1; e += TR_SLICE) { items.push_back(TrItem{k, e, std::min<int32_t>(TR_SLICE, e1 - e), nslot++}); runs.back().nslot++; }
  }
  uint64_t* ckey = nullptr; double *ccnt = nullptr, *cx = nullptr, *cx2 = nullptr, *part = nullptr;
  TrItem *items_d = nullptr, *shorts_d = nullptr; TrRun* runs_d = nullptr;
  auto cleanup = [&] { DEVFREE(ckey); DEVFREE(ccnt); DEVFREE(cx); DEVFREE(cx2); DEVFREE(part); DEVFREE(items_d); DEVFREE(shorts_d); DEVFREE(runs_d); };
  rc = dev_alloc(&ckey, (size_t)K);
  if (!rc) rc = dev_alloc(&ccnt, (size_t)K);
  if (!rc) rc = dev_alloc(&cx, (size_t)K * D);
  if (!rc) rc = dev_alloc(&cx2, (size_t)K * D);
  if (!rc) rc = dev_alloc(&part, (size_t)nslot * 2 * D);
  if (!rc) rc = dev_alloc(&items_d, items.size());
  if (!rc) rc = dev_alloc(&shorts_d, shorts.size());
  if (!rc) rc = dev_alloc(&runs_d, runs.size());
  if (rc) { cleanup(); return rc; }
  hipError_t e = hipSuccess;
  if (!items.empty()) e = hipMemcpyAsync(items_d, items.data(), sizeof(TrItem) * items.size(), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess && !shorts.empty()) e = hipMemcpyAsync(shorts_d, shorts.data(), sizeof(TrItem) * shorts.size(), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess && !runs.empty()) e = hipMemcpyAsync(runs_d, runs.data(), sizeof(TrRun) * runs.size(), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(ckey, st->kkey_d, sizeof(uint64_t) * (size_t)K, hipMemcpyDeviceToDevice, ctx->stream);
  if (e == hipSuccess) {
    KernelTimer kt(ctx, "k_tree_sum");
    if (!items.empty()) KHG_LAUNCH(ctx, k_tree_sum, dim3((unsigned)items.size()), dim3(256), 0, ctx->stream, items_d, st->sval_out_d, u->feats_d, D, part, cx, cx2);
    if (!shorts.empty()) {
      const int64_t per = 256 / D;
      KHG_LAUNCH(ctx, k_tree_sum_short, dim3((unsigned)(((int64_t)shorts.size() + per - 1) / per)), dim3(256), 0, ctx->stream, shorts_d, (int32_t)shorts.size(), st->sval_out_d,
                 u->feats_d, D, cx, cx2);
    }
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    KernelTimer kt(ctx, "k_tree_reduce");
    if (!runs.empty()) KHG_LAUNCH(ctx, k_tree_reduce, dim3(tr_grid((int64_t)runs.size() * 2 * D)), dim3(256), 0, ctx->stream, runs_d, (int32_t)runs.size(), part, D, cx, cx2);
    KHG_LAUNCH(ctx, k_tree_counts, dim3(tr_grid(K)), dim3(256), 0, ctx->stream, st->kstart_d, K, ccnt);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);      // the plan's host vectors are free again
  else (void)hipStreamSynchronize(ctx->stream);                    // ... on the error path too
  if (e != hipSuccess) { cleanup(); return khg_set_error(KHG_E_HIP, who + hipGetErrorString(e)); }
  rc = tr_merge(ctx, st, 1.0, &ckey, &ccnt, &cx, &cx2, K, true);
  cleanup();
  return rc;
}
