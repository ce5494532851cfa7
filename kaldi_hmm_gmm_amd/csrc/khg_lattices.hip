// kaldi_hmm_gmm_amd/csrc/khg_lattices.hip -- C-ABI (include/khg_hip.h): the lattice side.  The lattice decoder
// (khg_decode_lattice_faster, khg_k2_lattice.hip.inc) and the data-parallel LatticeSimpleDecoder (khg_decode_lattice_simple,
// khg_k2_lattice_simple.hip.inc), each with its raw lattice (khg_decode_lattice_faster_raw, khg_k2_lattice_faster_raw.hip.inc;
// khg_decode_lattice_simple_raw, khg_k2_lattice_raw.hip.inc); the handle of resident lattices (khg_lattices) with the operations on it
// (khg_k2_lattice_ops.hip.inc), its forward-backward posteriors (khg_posteriors, khg_k2_lattice_post.hip.inc) and their MPE / sMBR form
// (khg_k2_lattice_mpe.hip.inc: the same device functions and the same host steps per chunk around a kernel of its own), and rescoring /
// boosting (khg_lattices_rescore, khg_lattices_boost: khg_k2_lattice_rescore.hip.inc, khg_k1_cells.hip.inc), and the backoff n-gram LM
// (khg_lm) with khg_lattices_lm_rescore (khg_k2_lattice_lm.hip.inc), determinization (khg_lattices_determinize,
// khg_k2_lattice_det.hip.inc), and scoring (khg_lattices_add_penalty, khg_lattices_oracle,
// khg_lattices_wer, khg_edit_distance: khg_k2_lattice_score.hip.inc), and minimum Bayes risk decoding (khg_lattices_mbr:
// khg_k2_lattice_mbr.hip.inc).  gfx950 only.
//
// The host steps the families share, each written once (helpers take the bare name of the call the error texts name, "khg_x"):
//   DevBlocks::alloc / upload / zeroed, download   a call's device scratch with the copy or the clearing that fills it, and the copy back
//                                                  into a vector: every entry point below
//   launch                                         one launch under one timer; loops of launches under one timer (k2x_*, add_penalty,
//                                                  the words' packing, k3_post_flatten) and the launches without a timer (lat_meta,
//                                                  lat_width) are written out
//   scan_pairs_and_read, size_out_chunk            mark -> scan, ONE synchronisation, the output chunk -> fill: simple_emit,
//                                                  khg_lattices_prune, khg_lattices_lm_rescore (faster_emit and post_chunk_finish size a
//                                                  block that is not a handle's next chunk: they call the scan themselves)
//   split_by_budget                                the decoders' slices in launches of <= 4 GiB: faster_pass, decode_lattice_simple_impl
//   group_tables                                   utterances' tables in launches under a caller's budget: khg_lattices_oracle, _mbr
//   pack_words                                     the words of the entries that succeeded under words_cap: decode_out_download (over
//                                                  the cap: refused), khg_lattices_best_path and khg_lattices_oracle (KHG_LAT_WORDS)
//   best_path_args                                 the scale pairs and the per-chunk best-path scratch: khg_lattices_best_path, _wer
//   check_offsets                                  offsets from 0 that never decrease, over data that is there: lat_ref_check,
//                                                  score_ref_check, khg_lattices_mbr, khg_posteriors_validate, khg_posteriors_upload
//   lat_ready                                      arena_flush, lat_meta and on request lat_index / lat_width, at the entry of
//                                                  khg_lattices_ali_layout, _best_path, _prune, _posteriors, _rescore, _boost,
//                                                  _mpe_posteriors, _lm_rescore, _oracle, _wer and _mbr (_add_penalty reads no
//                                                  offsets: arena_flush alone; _rescore and _boost call lat_meta again for the
//                                                  copy they make, _mpe_posteriors calls lat_index after the reference's checks)
//   other_ctx                                      the refusal of a handle of another context: khg_lattices_rescore, _boost,
//                                                  _mpe_posteriors (and lat_ref_check for their ali_set), _lm_rescore, _add_penalty,
//                                                  _oracle, _wer, _mbr, khg_mbr_download
//   decode_prologue, DecodeOut, PostRun            the two decoders; khg_lattices_posteriors, _mpe_posteriors and _mbr's weights
#include "khg_internal.hpp"

#include <memory>

#include "khg_k2_hashlist.hip.inc"
#include "khg_k2_lattice.hip.inc"
#include "khg_k2_lattice_simple.hip.inc"
#include "khg_k2_lattice_arrays.hip.inc"
#include "khg_k2_lattice_raw.hip.inc"
#include "khg_k2_lattice_faster_raw.hip.inc"
#include "khg_k2_lattice_ops.hip.inc"
#include "khg_k2_lattice_post.hip.inc"
#include "khg_k1_cells.hip.inc"
#include "khg_k2_lattice_rescore.hip.inc"
#include "khg_k2_lattice_mpe.hip.inc"
#include "khg_k2_lattice_lm.hip.inc"
#include "khg_k2_lattice_det.hip.inc"
#include "khg_k2_lattice_score.hip.inc"
#include "khg_k2_lattice_mbr.hip.inc"
#include "khg_k2_lattice_nbest.hip.inc"

// ------------------------------------------------------------------------------------------
// The raw lattices of one batch (khg_decode_lattice_simple_raw, khg_decode_lattice_faster_raw): per chunk of scratch slices one
// exactly-sized device block holding the six per-state and five per-arc arrays of the chunk's utterances, one after the other.
struct LatChunk {
  int u0 = 0, n = 0;              // utterances u0 .. u0 + n
  int64_t ns = 0, na = 0;         // states, arcs
  unsigned char* buf = nullptr;
  // byte offsets of the arrays inside buf: frame, graph_state, tot_cost, extra_cost, final_cost, arc_begin | ilabel, olabel, graph_cost,
  // acoustic_cost, nextstate
  int64_t st[6] = {0, 0, 0, 0, 0, 0}, ar[5] = {0, 0, 0, 0, 0};
};
struct khg_lattices {
  int U = 0;
  std::vector<int64_t> state_off, arc_off;       // [U + 1]
  std::vector<LatChunk> chunks;
  int32_t* start_d = nullptr;                    // [U]
  int64_t bytes = 0;
  // what the operations on a handle need (khg_lattices_best_path / _prune), made at the first of them: state_off | arc_off on the
  // device, the frame of every utterance's last state as offsets (the layout of an alignment)
  int64_t* off_d = nullptr;                      // [2 * (U + 1)]
  std::vector<int64_t> ali_off;                  // [U + 1]
  // the in-arc index khg_lattices_posteriors gathers through, made at its first call: per chunk one block
  // [in_begin: states + utterances | in_arc: arcs | arc_src: arcs] (int32)
  std::vector<int32_t*> idx_d;
  khg_ctx* ctx = nullptr;                        // the context it was made on
  std::vector<int32_t> op_status;                // [U] KHG_LAT_* bits of the khg_lattices_rescore / _boost / _lm_rescore that made it (empty otherwise)
  // the widest frame (states) of every utterance, made at the first khg_lattices_oracle: it sizes the oracle's ring of rows in LDS
  int32_t* width_d = nullptr;                    // [U]
  std::vector<int32_t> width;                    // [U]
};

namespace {
struct LatFree { void operator()(khg_lattices* l) const { (void)khg_lattices_destroy(l); } };
using LatPtr = std::unique_ptr<khg_lattices, LatFree>;
// device scratch of one call: freed on the way out
struct DevBlocks {
  std::vector<void*> p;
  ~DevBlocks() { for (void* q : p) if (q) (void)hipFree(q); }
  template <class T>
  int alloc(int64_t count, T** out) {
    void* q = nullptr;
    HIPCHK(hipMalloc(&q, (size_t)std::max<int64_t>(count * (int64_t)sizeof(T), 16)));
    p.push_back(q);
    *out = static_cast<T*>(q);
    return KHG_OK;
  }
  // a block of `count` elements and the copy of src[0 .. count) into it, enqueued on the context's stream
  template <class T>
  int upload(khg_ctx* ctx, const T* src, int64_t count, T** out) {
    int rc = alloc(count, out);
    if (rc) return rc;
    if (count > 0) HIPCHK(hipMemcpyAsync(*out, src, sizeof(T) * (size_t)count, hipMemcpyHostToDevice, ctx->stream));
    return KHG_OK;
  }
  template <class T>
  int upload(khg_ctx* ctx, const std::vector<T>& src, T** out) { return upload(ctx, src.data(), (int64_t)src.size(), out); }
  // a block of `count` elements, cleared on the context's stream
  template <class T>
  int zeroed(khg_ctx* ctx, int64_t count, T** out) {
    int rc = alloc(count, out);
    if (rc) return rc;
    if (count > 0) HIPCHK(hipMemsetAsync(*out, 0, sizeof(T) * (size_t)count, ctx->stream));
    return KHG_OK;
  }
};
// dst sized to `count` elements and the copy of src_d[0 .. count) into it, enqueued on the context's stream: dst holds them after the
// next synchronisation
template <class T>
int download(khg_ctx* ctx, const T* src_d, int64_t count, std::vector<T>* dst) {
  dst->resize((size_t)count);
  if (count > 0) HIPCHK(hipMemcpyAsync(dst->data(), src_d, sizeof(T) * (size_t)count, hipMemcpyDeviceToHost, ctx->stream));
  return KHG_OK;
}
// One launch under a timer of its own: the entry `name` of the context's timings, the staged uploads, the launch on the context's
// stream, its error.  (A loop of launches under one timer, and a launch without a timer, are written out where they stand.)
template <class... P, class... A>
int launch(khg_ctx* ctx, const char* name, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, const A&... args) {
  KernelTimer kt(ctx, name);
  KHG_LAUNCH(ctx, kernel, grid, block, lds, ctx->stream, args...);
  HIPCHK(hipGetLastError());
  return KHG_OK;
}
// the refusal of a handle that was made on another context, in the name of the call `who`
int other_ctx(const std::string& who) { return khg_set_error(KHG_E_ARG, who + ": a handle of another context"); }
// Offsets off[0 .. n] (the argument `name`, one entry per `what`): they start at 0 and never decrease; data_name != nullptr: `data`,
// which they index, is there when they end above 0
int check_offsets(const std::string& who, const char* name, const int64_t* off, int64_t n, const char* what, const void* data = nullptr,
                  const char* data_name = nullptr) {
  if (!off || off[0] != 0) return khg_set_error(KHG_E_ARG, who + ": " + name + " must start at 0");
  for (int64_t i = 0; i < n; ++i)
    if (off[i + 1] < off[i]) return khg_set_error(KHG_E_ARG, who + ": " + name + " decreases at " + what + " " + std::to_string(i));
  if (data_name && off[n] > 0 && !data) return khg_set_error(KHG_E_ARG, who + ": " + data_name + " is NULL");
  return KHG_OK;
}
// The words of the entries that succeeded, packed one after the other: entry i of st.size() brings n = count(i) words, the ones at
// src(i, n), when st[i] has KHG_LAT_SUCCEEDED, none otherwise; words_off_h [entries + 1] says where they went in words_h [words_cap].
// An entry whose words do not fit: with `over`, (*over)[i] = KHG_LAT_WORDS and none of them; without, the call `who` is refused.
template <class Cnt, class Src>
int pack_words(const std::string& who, const std::vector<int32_t>& st, std::vector<int32_t>* over, Cnt count, Src src, int32_t* words_h,
               int64_t* words_off_h, int64_t words_cap) {
  int64_t pos = 0;
  for (size_t i = 0; i < st.size(); ++i) {
    words_off_h[i] = pos;
    int64_t n = (st[i] & KHG_LAT_SUCCEEDED) ? (int64_t)count(i) : 0;
    if (pos + n > words_cap) {
      if (!over) return khg_set_error(KHG_E_ARG, who + ": words_cap too small");
      (*over)[i] = KHG_LAT_WORDS; n = 0;
    }
    std::copy_n(src(i, n), n, words_h + pos);
    pos += n;
  }
  words_off_h[st.size()] = pos;
  return KHG_OK;
}

// an empty handle of U utterances, with the start states' array
int new_lattices(khg_ctx* ctx, int U, LatPtr* out) {
  LatPtr l(new khg_lattices);
  l->U = U; l->ctx = ctx;
  l->state_off.assign((size_t)U + 1, 0);
  l->arc_off.assign((size_t)U + 1, 0);
  if (U > 0) {
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&l->start_d), 4 * (size_t)U));
    l->bytes += 4 * (int64_t)U;
  }
  *out = std::move(l);
  return KHG_OK;
}
void lat_chunk_layout(LatChunk* ch, int64_t* total) {
  int64_t o = 0;
  auto take = [&](int64_t cnt) { const int64_t r = o; o += (4 * cnt + 255) & ~int64_t(255); return r; };
  for (int k = 0; k < 6; ++k) ch->st[k] = take(ch->ns);
  for (int k = 0; k < 5; ++k) ch->ar[k] = take(ch->na);
  *total = o;
}
// the block of a chunk whose u0, n, ns, na are set; its size is added to *bytes
int lat_chunk_alloc(LatChunk* ch, int64_t* bytes) {
  int64_t total = 0;
  lat_chunk_layout(ch, &total);
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&ch->buf), (size_t)std::max<int64_t>(total, 16)));
  *bytes += total;
  return KHG_OK;
}
// the chunk's arrays as kernel arguments (LatArrays to fill, LatArraysIn to read)
template <class I, class F>
void lat_chunk_arrays(const LatChunk& c, LatArraysT<I, F>* a) {
  auto i = [&](int64_t o) { return reinterpret_cast<I*>(c.buf + o); };
  auto f = [&](int64_t o) { return reinterpret_cast<F*>(c.buf + o); };
  a->frame = i(c.st[0]); a->gstate = i(c.st[1]); a->tot = f(c.st[2]); a->extra = f(c.st[3]); a->fin = f(c.st[4]); a->arc_begin = i(c.st[5]);
  a->ilabel = i(c.ar[0]); a->olabel = i(c.ar[1]); a->g = f(c.ar[2]); a->ac = f(c.ar[3]); a->next = i(c.ar[4]);
}

// what k2_lattice_scan_pairs left at off_d [2 * (n + 1)], as two prefix arrays [n + 1]: the one copy and the ONE synchronisation that
// size a chunk's output
int read_pair_offsets(khg_ctx* ctx, const int64_t* off_d, int n, std::vector<int64_t>* first, std::vector<int64_t>* second) {
  std::vector<int64_t> h(2 * ((size_t)n + 1), 0);
  HIPCHK(hipMemcpyAsync(h.data(), off_d, 16 * ((size_t)n + 1), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  first->assign(h.begin(), h.begin() + n + 1);
  second->assign(h.begin() + n + 1, h.end());
  return KHG_OK;
}
// the exclusive prefixes of n pairs tot_d [2 n] (k2_lattice_scan_pairs, timed as `timer_name`) to off_d, and read_pair_offsets of them
int scan_pairs_and_read(khg_ctx* ctx, const char* timer_name, const int64_t* tot_d, int64_t* off_d, int n, std::vector<int64_t>* first,
                        std::vector<int64_t>* second) {
  int rc = launch(ctx, timer_name, k2_lattice_scan_pairs, dim3(1), dim3(64), 0, tot_d, off_d, n);
  return rc ? rc : read_pair_offsets(ctx, off_d, n, first, second);
}
// a lattice's arc_begin and nextstate are int32: utterance ids[b] (nullptr: u0 + b) of a chunk with the prefix arrays so / ao is refused
// in the name of `who` when it has more states or arcs
int check_utt_counts(const std::string& who, const int32_t* ids, int u0, const std::vector<int64_t>& so, const std::vector<int64_t>& ao) {
  for (size_t b = 0; b + 1 < so.size(); ++b)
    if (so[b + 1] - so[b] > INT32_MAX || ao[b + 1] - ao[b] > INT32_MAX)
      return khg_set_error(KHG_E_ARG, who + ": the lattice of utterance " + std::to_string(ids ? ids[b] : u0 + (int)b) +
                                          " has more than 2^31 - 1 states or arcs");
  return KHG_OK;
}
// ... and the counts of the chunk's utterances u0 .. go on a handle's two offset vectors (chunks arrive in utterance order)
int add_chunk_counts(const std::string& who, int u0, const std::vector<int64_t>& so, const std::vector<int64_t>& ao,
                     std::vector<int64_t>* state_off, std::vector<int64_t>* arc_off) {
  int rc = check_utt_counts(who, nullptr, u0, so, ao);
  if (rc) return rc;
  for (size_t b = 0; b + 1 < so.size(); ++b) {
    (*state_off)[(size_t)u0 + b + 1] = (*state_off)[(size_t)u0] + so[b + 1];
    (*arc_off)[(size_t)u0 + b + 1] = (*arc_off)[(size_t)u0] + ao[b + 1];
  }
  return KHG_OK;
}
// Between a mark kernel and its fill kernel: a mark left the (states, arcs) of the n utterances u0 .. at utt_tot [2 n].  Their scan to
// utt_off (timed as `scan_name`) with the ONE synchronisation that sizes the output, the counts onto res's offsets (an utterance above
// 2^31 - 1 is refused in the name of `who`), and res's next chunk, allocated: *ch, for the fill to write
int size_out_chunk(khg_ctx* ctx, const std::string& who, const char* scan_name, const int64_t* utt_tot, int64_t* utt_off, int u0, int n,
                   khg_lattices* res, LatChunk* ch) {
  std::vector<int64_t> so, ao;
  int rc = scan_pairs_and_read(ctx, scan_name, utt_tot, utt_off, n, &so, &ao);
  if (!rc) rc = add_chunk_counts(who, u0, so, ao, &res->state_off, &res->arc_off);
  if (rc) return rc;
  ch->u0 = u0; ch->n = n; ch->ns = so[(size_t)n]; ch->na = ao[(size_t)n];
  if ((rc = lat_chunk_alloc(ch, &res->bytes))) return rc;
  res->chunks.push_back(*ch);
  return KHG_OK;
}
// grid.y of a fill over n utterances whose largest has max_n items: stripes of nt items go to workgroups of their own while the launch
// has few utterances
unsigned stripes(int64_t max_n, int nt, int n) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((max_n + nt - 1) / nt, std::max<int64_t>(1, 4096 / n)));
}
// Scratch slices of bytes[k] each are grouped into launches of at most 4 GiB (a slice above that is a launch of its own): launch c takes
// the slices cb[c] .. cb[c + 1], slice k lies rel[k] bytes behind its launch's first, the largest launch needs max_chunk bytes.
const int64_t kScratchBudget = int64_t(4) << 30;
void split_by_budget(const std::vector<int64_t>& bytes, std::vector<size_t>* cb, std::vector<int64_t>* rel, int64_t* max_chunk) {
  cb->assign(1, 0);
  rel->assign(bytes.size(), 0);
  int64_t acc = 0;
  *max_chunk = 0;
  for (size_t k = 0; k < bytes.size(); ++k) {
    if (acc > 0 && acc + bytes[k] > kScratchBudget) { *max_chunk = std::max(*max_chunk, acc); cb->push_back(k); acc = 0; }
    (*rel)[k] = acc;
    acc += bytes[k];
  }
  *max_chunk = std::max(*max_chunk, acc);
  cb->push_back(bytes.size());
}
}  // namespace

extern "C" int khg_lattices_destroy(khg_lattices* l) {
  if (!l) return KHG_OK;
  for (LatChunk& c : l->chunks) if (c.buf) (void)hipFree(c.buf);
  if (l->start_d) (void)hipFree(l->start_d);
  if (l->off_d) (void)hipFree(l->off_d);
  for (int32_t* q : l->idx_d) if (q) (void)hipFree(q);
  if (l->width_d) (void)hipFree(l->width_d);
  delete l;
  return KHG_OK;
}
extern "C" int khg_lattices_sizes(const khg_lattices* l, int64_t* state_off_h, int64_t* arc_off_h) {
  if (!l) return khg_set_error(KHG_E_ARG, "khg_lattices_sizes: bad arguments");
  if (state_off_h) std::copy(l->state_off.begin(), l->state_off.end(), state_off_h);
  if (arc_off_h) std::copy(l->arc_off.begin(), l->arc_off.end(), arc_off_h);
  return KHG_OK;
}
extern "C" int khg_lattices_device_bytes(const khg_lattices* l, int64_t* bytes) {
  if (!l || !bytes) return khg_set_error(KHG_E_ARG, "khg_lattices_device_bytes: bad arguments");
  *bytes = l->bytes;
  return KHG_OK;
}
extern "C" int khg_lattices_download(khg_ctx* ctx, const khg_lattices* l, int32_t* frame_h, int32_t* graph_state_h, float* tot_cost_h,
                                     float* extra_cost_h, float* final_cost_h, int32_t* arc_begin_h, int32_t* ilabel_h, int32_t* olabel_h,
                                     float* graph_cost_h, float* acoustic_cost_h, int32_t* nextstate_h, int32_t* start_h) {
  if (ctx_dead(ctx) || !l) return khg_set_error(KHG_E_ARG, "khg_lattices_download: bad arguments");
  void* st_h[6] = {frame_h, graph_state_h, tot_cost_h, extra_cost_h, final_cost_h, arc_begin_h};
  void* ar_h[5] = {ilabel_h, olabel_h, graph_cost_h, acoustic_cost_h, nextstate_h};
  for (const LatChunk& c : l->chunks) {
    const int64_t s0 = l->state_off[(size_t)c.u0], a0 = l->arc_off[(size_t)c.u0];
    for (int k = 0; k < 6; ++k)
      if (st_h[k] && c.ns) HIPCHK(hipMemcpyAsync(static_cast<char*>(st_h[k]) + 4 * s0, c.buf + c.st[k], 4 * (size_t)c.ns, hipMemcpyDeviceToHost, ctx->stream));
    for (int k = 0; k < 5; ++k)
      if (ar_h[k] && c.na) HIPCHK(hipMemcpyAsync(static_cast<char*>(ar_h[k]) + 4 * a0, c.buf + c.ar[k], 4 * (size_t)c.na, hipMemcpyDeviceToHost, ctx->stream));
  }
  if (start_h && l->U) HIPCHK(hipMemcpyAsync(start_h, l->start_d, 4 * (size_t)l->U, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return KHG_OK;
}

// ------------------------------------------------------------------------------------------
// What the two lattice decoders share: the argument checks, the result buffers and their way back to the host.
namespace {
// `who`: the call the error texts name.  cfg_ok: the decoder's own Config::Check (`config_name` assertion failed).
template <class Cfg, class Ok>
int decode_prologue(const std::string& who, khg_ctx* ctx, const khg_tm* tm, khg_utts* u, const Cfg* cfg, const char* config_name, Ok cfg_ok) {
  if (ctx_dead(ctx) || !tm || !u || !cfg) return khg_set_error(KHG_E_ARG, who + ": bad arguments");
  { int rf = utts_foreign_ctx(ctx, u, who.c_str()); if (rf) return rf; }
  if (!u->has_graphs) return khg_set_error(KHG_E_ARG, who + ": the utterance set has no decoding graphs");
  if (!u->ll_valid) return khg_set_error(KHG_E_ARG, who + ": call khg_loglikes first");
  // khg_loglikes_band leaves upper bounds in the cells past the band: a token the beam keeps (or of a partial path) may read any cell
  if (u->ll_mode == 2)
    return khg_set_error(KHG_E_ARG, who + ": the scores come from khg_loglikes_band; call khg_loglikes (every cell) first");
  if (!cfg_ok(*cfg)) return khg_set_error(KHG_E_RUNTIME, std::string(config_name) + " assertion failed");
  int rc = wait_ali(ctx, u);
  if (!rc) rc = k1_band_check(ctx, u);
  return rc;
}

// the decoders' results on the device; the words of utterance i have room for wcap_off[i + 1] - wcap_off[i]
struct DecodeOut {
  int32_t *ali = nullptr, *words = nullptr, *num_words = nullptr, *status = nullptr, *err_frame = nullptr;
  double* like = nullptr;
  int64_t* words_off = nullptr;
  std::vector<int64_t> wcap_off;
  int64_t N = 0, NW = 0;          // frames, word slots
};
// allocates them in dv (err_frame: the simple decoder's), flushes the arena and enqueues the word offsets and the cleared alignment
int decode_out_alloc(khg_ctx* ctx, const khg_utts* u, bool err_frame, DevBlocks* dv, DecodeOut* o) {
  const int U = u->n_utt;
  o->wcap_off.assign((size_t)U + 1, 0);
  for (int i = 0; i < U; ++i) o->wcap_off[(size_t)i + 1] = o->wcap_off[(size_t)i] + (u->frame_off[i + 1] - u->frame_off[i]) + utt_states(u, i) + 64;
  o->N = u->N; o->NW = o->wcap_off[(size_t)U];
  int rc;
  if ((rc = dv->alloc(std::max<int64_t>(o->N, 1), &o->ali)) || (rc = dv->alloc(std::max<int64_t>(o->NW, 1), &o->words)) ||
      (rc = dv->alloc(U, &o->num_words)) || (rc = dv->alloc(U, &o->status)) || (err_frame && (rc = dv->alloc(U, &o->err_frame))) ||
      (rc = dv->alloc(U, &o->like)) || (rc = dv->alloc(U + 1, &o->words_off)) || (rc = arena_flush(ctx)))
    return rc;
  HIPCHK(hipMemcpyAsync(o->words_off, o->wcap_off.data(), 8 * ((size_t)U + 1), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemsetAsync(o->ali, 0, 4 * (size_t)std::max<int64_t>(o->N, 1), ctx->stream));
  return KHG_OK;
}
// the graph tables, scores and result buffers of a decoder kernel's arguments (LatArgs, LsArgs)
template <class Args>
void decode_args(const khg_tm* tm, const khg_utts* u, const DecodeOut& o, Args* a) {
  a->frame_off = u->frame_off_d; a->gidx = u->gidx_d; a->state_off = u->state_off_d; a->start = u->start_d;
  a->in_off = u->in_off_d; a->in_col = u->in_col_d; a->in_tid = u->in_tid_d; a->in_olabel = u->in_olabel_d; a->in_w = u->in_w_d;
  a->out_off = u->out_off_d; a->out_inidx = u->out_inidx_d; a->final_w = u->final_d;
  a->trans_cost = tm->has_trans_cost ? tm->trans_cost_d : nullptr;
  a->ll = u->ll_d; a->ll_off = u->ll_off_d;
  a->ali = o.ali; a->words = o.words; a->words_off = o.words_off; a->num_words = o.num_words; a->like = o.like; a->status = o.status;
}
// the statuses (synchronous), for a decoder that looks at them before the rest comes back
int decode_out_status(const DecodeOut& o, int U, std::vector<int32_t>* st) {
  st->resize((size_t)U);
  HIPCHK(hipMemcpy(st->data(), o.status, 4 * (size_t)U, hipMemcpyDeviceToHost));
  return KHG_OK;
}
// everything the caller asked for, the words of the utterances that succeeded packed one after the other; st: decode_out_status's
int decode_out_download(khg_ctx* ctx, const std::string& who, const DecodeOut& o, const std::vector<int32_t>& st, int32_t* ali_h,
                        int32_t* words_h, int64_t* words_off_h, int64_t words_cap, double* like_h, int32_t* status_h, int32_t* err_frame_h) {
  const size_t U = st.size();
  std::vector<int32_t> nw(U), w((size_t)std::max<int64_t>(o.NW, 1));
  if (ali_h && o.N) HIPCHK(hipMemcpyAsync(ali_h, o.ali, 4 * (size_t)o.N, hipMemcpyDeviceToHost, ctx->stream));
  if (like_h) HIPCHK(hipMemcpyAsync(like_h, o.like, 8 * U, hipMemcpyDeviceToHost, ctx->stream));
  if (err_frame_h) HIPCHK(hipMemcpyAsync(err_frame_h, o.err_frame, 4 * U, hipMemcpyDeviceToHost, ctx->stream));
  if (words_h && words_off_h) {
    HIPCHK(hipMemcpyAsync(nw.data(), o.num_words, 4 * U, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(w.data(), o.words, 4 * w.size(), hipMemcpyDeviceToHost, ctx->stream));
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (status_h) std::copy(st.begin(), st.end(), status_h);
  if (!(words_h && words_off_h)) return KHG_OK;
  return pack_words(who, st, nullptr, [&](size_t i) { return nw[i]; }, [&](size_t i, int64_t) { return w.begin() + o.wcap_off[i]; }, words_h,
                    words_off_h, words_cap);
}
}  // namespace

// ------------------------------------------------------------------------------------------
// K2L: LatticeFasterDecoder (khg_k2_lattice.hip.inc)
extern "C" void khg_lattice_faster_config_default(khg_lattice_faster_config* c) {
  c->beam = 16.0f; c->max_active = INT32_MAX; c->min_active = 200; c->lattice_beam = 10.0f; c->prune_interval = 25;
  c->beam_delta = 0.5f; c->hash_ratio = 2.0f; c->prune_scale = 0.1f; c->acoustic_scale = 1.0f; c->allow_partial = 1;
  c->scratch_per_frame = 0;
}

namespace {
// (lattices) what a launch emitted: an exactly-sized block of the utterances list[ch.u0 .. ch.u0 + ch.n), with their offsets inside it;
// a block not handed to the handle is freed on the way out
struct EmitBlock { LatChunk ch; std::vector<int64_t> so, ao; int64_t bytes = 0; };
struct EmitBlocks {
  std::vector<EmitBlock> v;
  ~EmitBlocks() { for (EmitBlock& b : v) if (b.ch.buf) (void)hipFree(b.ch.buf); }
};
// one call of the decoder: what its passes share
struct FasterRun {
  khg_ctx* ctx; const khg_utts* u;
  std::string who;                  // the call the user made
  LatArgs a;
  int64_t hb;
  bool lat;                         // khg_decode_lattice_faster_raw: the slices have lattice rows, and what follows
  int64_t *tot_d = nullptr, *off_d = nullptr;      // the utterances' (states, arcs) of a launch and their prefix
  int32_t* start_d = nullptr;       // the handle's
  DevBlocks dv;
};

// the lattices of the launch over list[k0 .. k0 + n), while its slices are alive: the decoder left the rows and the totals, one scan over
// the utterances, ONE synchronisation to size the output, the fill
int faster_emit(FasterRun& r, const std::vector<int32_t>& list, int k0, int n, EmitBlocks* blocks) {
  khg_ctx* ctx = r.ctx;
  blocks->v.emplace_back();
  EmitBlock& eb = blocks->v.back();
  int rc = scan_pairs_and_read(ctx, "k2_lattice_faster_raw_scan", r.tot_d, r.off_d, n, &eb.so, &eb.ao);
  if (!rc) rc = check_utt_counts(r.who, list.data() + k0, 0, eb.so, eb.ao);
  if (rc) return rc;
  LatChunk& ch = eb.ch;
  ch.u0 = k0; ch.n = n; ch.ns = eb.so[(size_t)n]; ch.na = eb.ao[(size_t)n];
  if ((rc = lat_chunk_alloc(&ch, &eb.bytes))) return rc;
  LfrArgs p{};
  p.a = r.a; p.n = n; p.utt_off = r.off_d; p.start_out = r.start_d;
  lat_chunk_arrays(ch, &p.out);
  int64_t max_n = 0;
  for (int b = 0; b < n; ++b) max_n = std::max(max_n, eb.so[(size_t)b + 1] - eb.so[(size_t)b]);
  return launch(ctx, "k2_lattice_faster_raw_fill", k2_lattice_faster_raw_fill, dim3((unsigned)n, stripes(max_n, LFR_NT, n)), dim3(LFR_NT), 0, p, k0);
}

// One pass over a list of utterances: each gets a scratch slice of `per_frame` tokens / links per frame (0: the automatic size,
// -1: the whole graph per frame, i.e. an utterance can never run out); slices are grouped into launches of <= 4 GiB of scratch.
int faster_pass(FasterRun& r, const std::vector<int32_t>& list, int64_t per_frame, EmitBlocks* blocks) {
  khg_ctx* ctx = r.ctx;
  const khg_utts* u = r.u;
  LatArgs& a = r.a;
  const size_t L = list.size();
  std::vector<int32_t> tcap(L), lcap(L);
  std::vector<int64_t> bytes(L);
  for (size_t k = 0; k < L; ++k) {
    const int i = list[k];
    const int64_t T = u->frame_off[i + 1] - u->frame_off[i], S = utt_states(u, i), A = std::max<int64_t>(a.amax, 1);
    const int64_t pt = per_frame > 0 ? per_frame : per_frame < 0 ? S : std::min<int64_t>(S, 256);
    const int64_t pl = per_frame > 0 ? per_frame : per_frame < 0 ? A : std::min<int64_t>(A, 1024);
    const int64_t tc = (T + 1) * pt + (per_frame > 0 ? 0 : S) + 1, lc = (T + 1) * pl + (per_frame > 0 ? 0 : A) + 1;
    if (tc > INT32_MAX / 2 || lc > INT32_MAX / 2) return khg_set_error(KHG_E_ARG, r.who + ": utterance too large for the scratch");
    tcap[k] = (int32_t)tc; lcap[k] = (int32_t)lc;
    bytes[k] = (lat_layout(T, S, a.amax, r.hb, tc, lc, r.lat).total + 255) & ~int64_t(255);
  }
  std::vector<size_t> cb;
  std::vector<int64_t> rel;
  int64_t max_chunk = 0;
  split_by_budget(bytes, &cb, &rel, &max_chunk);
  unsigned char* scratch; int64_t* scr_off_d; int32_t *tcap_d, *lcap_d, *list_d;
  int rc;
  if ((rc = r.dv.alloc(max_chunk, &scratch)) || (rc = r.dv.upload(ctx, rel, &scr_off_d)) || (rc = r.dv.upload(ctx, tcap, &tcap_d)) ||
      (rc = r.dv.upload(ctx, lcap, &lcap_d)) || (rc = r.dv.upload(ctx, list, &list_d)))
    return rc;
  a.scratch = scratch; a.scr_off = scr_off_d; a.tok_cap = tcap_d; a.link_cap = lcap_d; a.list = list_d;
  for (size_t c = 0; c + 1 < cb.size(); ++c) {
    const int n = (int)(cb[c + 1] - cb[c]), k0 = (int)cb[c];
    rc = r.lat ? launch(ctx, "k2_lattice_faster", k2_lattice_faster_lat, dim3((unsigned)n), dim3(64), 0, a, k0, r.tot_d)
               : launch(ctx, "k2_lattice_faster", k2_lattice_faster, dim3((unsigned)n), dim3(64), 0, a, k0);
    if (!rc && r.lat) rc = faster_emit(r, list, k0, n, blocks);
    if (rc) return rc;
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));    // the slices are freed with `dv` or reused by the next pass
  return KHG_OK;
}

// The handle: every utterance in utterance order, its chunks the first pass's launches.  Without a second pass (`again` empty) the first
// pass's blocks are the chunks.  With one, a chunk that holds a re-decoded utterance is rebuilt on the device from the blocks of both
// passes (k2_lattice_faster_raw_gather); only offsets travel.
int faster_assemble(FasterRun& r, EmitBlocks& pass1, EmitBlocks& pass2, const std::vector<int32_t>& again, khg_lattices* lats) {
  khg_ctx* ctx = r.ctx;
  const size_t U = (size_t)lats->U;
  // where every utterance's lattice is: block (first pass's, then second pass's), first state / arc there; its sizes go to the handle
  std::vector<int32_t> src_blk(U, 0);
  std::vector<int64_t> src_off(2 * U, 0);
  std::vector<EmitBlock*> blk;
  for (EmitBlock& b : pass1.v) blk.push_back(&b);
  for (EmitBlock& b : pass2.v) blk.push_back(&b);
  std::vector<char> redone(U, 0);
  for (int32_t i : again) redone[(size_t)i] = 1;
  for (size_t j = 0; j < blk.size(); ++j) {
    const bool second = j >= pass1.v.size();
    const EmitBlock& e = *blk[j];
    for (size_t b = 0; b < (size_t)e.ch.n; ++b) {
      const size_t i = second ? (size_t)again[(size_t)e.ch.u0 + b] : (size_t)e.ch.u0 + b;
      if (!second && redone[i]) continue;        // (empty there: the second pass's is the one)
      src_blk[i] = (int32_t)j;
      src_off[2 * i] = e.so[b]; src_off[2 * i + 1] = e.ao[b];
      lats->state_off[i + 1] = e.so[b + 1] - e.so[b]; lats->arc_off[i + 1] = e.ao[b + 1] - e.ao[b];
    }
  }
  for (size_t i = 0; i < U; ++i) { lats->state_off[i + 1] += lats->state_off[i]; lats->arc_off[i + 1] += lats->arc_off[i]; }
  LfrBlock* blocks_d = nullptr;
  std::vector<LfrBlock> blocks_h;
  std::vector<std::vector<int64_t>> dst_off_keep;      // (host sides of copies in flight until the synchronisation below)
  int rc;
  if (!again.empty()) {
    for (const EmitBlock* e : blk) {
      LfrBlock bd;
      for (int j = 0; j < 6; ++j) bd.st[j] = reinterpret_cast<const int32_t*>(e->ch.buf + e->ch.st[j]);
      for (int j = 0; j < 5; ++j) bd.ar[j] = reinterpret_cast<const int32_t*>(e->ch.buf + e->ch.ar[j]);
      blocks_h.push_back(bd);
    }
    if ((rc = r.dv.upload(ctx, blocks_h, &blocks_d))) return rc;
  }
  for (EmitBlock& e : pass1.v) {
    const size_t u0 = (size_t)e.ch.u0, n = (size_t)e.ch.n;
    bool rebuild = false;
    for (size_t b = 0; b < n; ++b) rebuild = rebuild || redone[u0 + b];
    if (!rebuild) {
      lats->chunks.push_back(e.ch);
      lats->bytes += e.bytes;
      e.ch.buf = nullptr;        // the handle's from here on
      continue;
    }
    dst_off_keep.emplace_back(2 * (n + 1), 0);
    std::vector<int64_t>& dst_off = dst_off_keep.back();
    int64_t max_n = 1;
    for (size_t b = 0; b < n; ++b) {
      dst_off[b + 1] = lats->state_off[u0 + b + 1] - lats->state_off[u0];
      dst_off[n + 2 + b] = lats->arc_off[u0 + b + 1] - lats->arc_off[u0];
      max_n = std::max(max_n, std::max(dst_off[b + 1] - dst_off[b], dst_off[n + 2 + b] - dst_off[n + 1 + b]));
    }
    LatChunk ch;
    ch.u0 = (int)u0; ch.n = (int)n; ch.ns = dst_off[n]; ch.na = dst_off[2 * n + 1];
    if ((rc = lat_chunk_alloc(&ch, &lats->bytes))) return rc;
    lats->chunks.push_back(ch);
    LfrGather g{};
    int32_t* src_blk_d; int64_t *src_off_d, *dst_off_d;
    if ((rc = r.dv.upload(ctx, src_blk.data() + u0, (int64_t)n, &src_blk_d)) || (rc = r.dv.upload(ctx, src_off.data() + 2 * u0, 2 * (int64_t)n, &src_off_d)) ||
        (rc = r.dv.upload(ctx, dst_off, &dst_off_d)))
      return rc;
    g.blocks = blocks_d; g.src_block = src_blk_d; g.src_off = src_off_d; g.dst_off = dst_off_d; g.n = (int32_t)n;
    for (int j = 0; j < 6; ++j) g.st[j] = reinterpret_cast<int32_t*>(ch.buf + ch.st[j]);
    for (int j = 0; j < 5; ++j) g.ar[j] = reinterpret_cast<int32_t*>(ch.buf + ch.ar[j]);
    if ((rc = launch(ctx, "k2_lattice_faster_raw_gather", k2_lattice_faster_raw_gather, dim3((unsigned)n, stripes(max_n, LFR_NT, (int)n)), dim3(LFR_NT), 0, g)))
      return rc;
  }
  if (!again.empty()) return check_err_flag(ctx, r.who.c_str());     // synchronises: the blocks the chunks were gathered from go now
  return KHG_OK;
}

// khg_decode_lattice_faster (lat_out == nullptr: nothing about lattices runs, and the slices have no lattice rows) and
// khg_decode_lattice_faster_raw
int decode_lattice_faster_impl(khg_ctx* ctx, const khg_tm* tm, khg_utts* u, const khg_lattice_faster_config* cfg,
                               int32_t* ali_h, int32_t* words_h, int64_t* words_off_h, int64_t words_cap,
                               double* like_h, int32_t* status_h, khg_lattices** lat_out) {
  FasterRun r;
  r.ctx = ctx; r.u = u; r.lat = lat_out != nullptr;
  r.who = r.lat ? "khg_decode_lattice_faster_raw" : "khg_decode_lattice_faster";
  // LatticeFasterDecoderConfig::Check (csrc/lattice-faster-decoder.h:99-104)
  int rc = decode_prologue(r.who, ctx, tm, u, cfg, "LatticeFasterDecoderConfig", [](const khg_lattice_faster_config& c) {
    return c.beam > 0.0f && c.max_active > 1 && c.lattice_beam > 0.0f && c.min_active <= c.max_active && c.prune_interval > 0 &&
           c.beam_delta > 0.0f && c.hash_ratio >= 1.0f && c.prune_scale > 0.0f && c.prune_scale < 1.0f && c.min_active >= 0 &&
           c.scratch_per_frame >= 0;
  });
  if (rc) return rc;
  const int U = u->n_utt;
  LatPtr lats;
  if (r.lat && (rc = new_lattices(ctx, U, &lats))) return rc;
  if (U == 0) { if (r.lat) *lat_out = lats.release(); return KHG_OK; }
  if (r.lat) {
    r.start_d = lats->start_d;
    if ((rc = r.dv.alloc(2 * (int64_t)U, &r.tot_d)) || (rc = r.dv.alloc(2 * ((int64_t)U + 1), &r.off_d))) return rc;
  }
  DecodeOut o;
  if ((rc = decode_out_alloc(ctx, u, false, &r.dv, &o))) return rc;
  r.hb = std::max<int64_t>(1000, (int64_t)((float)u->max_states * cfg->hash_ratio)) + 1;
  LatArgs& a = r.a;
  decode_args(tm, u, o, &a);
  a.hb = (int32_t)r.hb; a.amax = u->max_inarcs;     // (the kernel lays every slice out with the same arc bound)
  a.beam = cfg->beam; a.lattice_beam = cfg->lattice_beam; a.beam_delta = cfg->beam_delta; a.hash_ratio = cfg->hash_ratio;
  a.prune_scale = cfg->prune_scale; a.acoustic_scale = cfg->acoustic_scale;
  a.max_active = cfg->max_active; a.min_active = cfg->min_active; a.prune_interval = cfg->prune_interval; a.allow_partial = cfg->allow_partial ? 1 : 0;
  EmitBlocks pass1, pass2;
  std::vector<int32_t> all((size_t)U), again, st;
  for (int i = 0; i < U; ++i) all[(size_t)i] = i;
  rc = faster_pass(r, all, cfg->scratch_per_frame, &pass1);
  if (!rc) rc = check_err_flag(ctx, r.who.c_str());     // synchronises
  if (!rc) rc = decode_out_status(o, U, &st);
  if (rc) return rc;
  if (cfg->scratch_per_frame == 0) {
    // the automatic size ran out: those utterances again with room for every state and arc on every frame (a frame never holds more)
    for (int i = 0; i < U; ++i) if (st[(size_t)i] & KHG_LAT_SCRATCH) again.push_back(i);
    if (!again.empty()) {
      rc = faster_pass(r, again, -1, &pass2);
      if (!rc) rc = check_err_flag(ctx, r.who.c_str());
      if (!rc) rc = decode_out_status(o, U, &st);
      if (rc) return rc;
    }
  }
  rc = decode_out_download(ctx, r.who, o, st, ali_h, words_h, words_off_h, words_cap, like_h, status_h, nullptr);
  if (rc || !r.lat) return rc;
  if ((rc = faster_assemble(r, pass1, pass2, again, lats.get()))) return rc;
  *lat_out = lats.release();
  return KHG_OK;
}
}  // namespace

extern "C" int khg_decode_lattice_faster(khg_ctx* ctx, const khg_tm* tm, khg_utts* u, const khg_lattice_faster_config* cfg,
                                         int32_t* ali_h, int32_t* words_h, int64_t* words_off_h, int64_t words_cap,
                                         double* like_h, int32_t* status_h) {
  return decode_lattice_faster_impl(ctx, tm, u, cfg, ali_h, words_h, words_off_h, words_cap, like_h, status_h, nullptr);
}
extern "C" int khg_decode_lattice_faster_raw(khg_ctx* ctx, const khg_tm* tm, khg_utts* u, const khg_lattice_faster_config* cfg,
                                             int32_t* ali_h, int32_t* words_h, int64_t* words_off_h, int64_t words_cap,
                                             double* like_h, int32_t* status_h, khg_lattices** out) {
  if (!out) return khg_set_error(KHG_E_ARG, "khg_decode_lattice_faster_raw: out is NULL");
  *out = nullptr;
  return decode_lattice_faster_impl(ctx, tm, u, cfg, ali_h, words_h, words_off_h, words_cap, like_h, status_h, out);
}

// ------------------------------------------------------------------------------------------
// K2S: LatticeSimpleDecoder (khg_k2_lattice_simple.hip.inc)
extern "C" void khg_lattice_simple_config_default(khg_lattice_simple_config* c) {
  c->beam = 16.0f; c->lattice_beam = 10.0f; c->prune_interval = 25; c->prune_scale = 0.1f; c->acoustic_scale = 1.0f;
  c->allow_partial = 1; c->scratch_per_frame = 0;
}

namespace {
// the lattices of the chunk of utterances u0 .. u0 + p.n, while its slices are alive: count, the two scans, ONE synchronisation to size
// the output, the fill
int simple_emit(khg_ctx* ctx, LrArgs p, int u0, int nt, int64_t max_T, khg_lattices* lats) {
  const int n = p.n;
  // frames are independent: stripes of them go to workgroups of their own while the chunk has few utterances
  const unsigned gy = (unsigned)std::min<int64_t>(max_T + 1, std::max<int64_t>(1, 1024 / n));
  LatChunk ch;
  int rc = launch(ctx, "k2_lattice_raw_count", k2_lattice_raw_count, dim3((unsigned)n, gy), dim3(nt), 0, p, u0);
  if (!rc) rc = launch(ctx, "k2_lattice_raw_scan", k2_lattice_raw_scan_frames, dim3((unsigned)n), dim3(64), 0, p, u0);
  if (!rc) rc = size_out_chunk(ctx, "khg_decode_lattice_simple_raw", "k2_lattice_raw_scan", p.utt_tot, p.utt_off, u0, n, lats, &ch);
  if (rc) return rc;
  lat_chunk_arrays(ch, &p.out);
  return launch(ctx, "k2_lattice_raw_fill", k2_lattice_raw_fill, dim3((unsigned)n, gy), dim3(nt), 0, p, u0);
}

// khg_decode_lattice_simple (lat_out == nullptr: nothing about lattices runs) and khg_decode_lattice_simple_raw
int decode_lattice_simple_impl(khg_ctx* ctx, const khg_tm* tm, khg_utts* u, const khg_lattice_simple_config* cfg,
                               int32_t* ali_h, int32_t* words_h, int64_t* words_off_h, int64_t words_cap,
                               double* like_h, int32_t* status_h, int32_t* err_frame_h, khg_lattices** lat_out) {
  const std::string who = "khg_decode_lattice_simple";
  // LatticeSimpleDecoderConfig::Check (csrc/lattice-simple-decoder.h:76-78)
  int rc = decode_prologue(who, ctx, tm, u, cfg, "LatticeSimpleDecoderConfig", [](const khg_lattice_simple_config& c) {
    return c.beam > 0.0f && c.lattice_beam > 0.0f && c.prune_interval > 0 && c.scratch_per_frame >= 0;
  });
  if (rc) return rc;
  const int U = u->n_utt;
  const bool lat = lat_out != nullptr;
  LatPtr lats;
  if (lat && (rc = new_lattices(ctx, U, &lats))) return rc;
  if (U == 0) { if (lat) *lat_out = lats.release(); return KHG_OK; }
  DevBlocks dv;
  LrArgs p{};        // (lattices) the chunks' emit
  if (lat) {
    p.start_out = lats->start_d;
    if ((rc = dv.alloc(2 * (int64_t)U, &p.utt_tot)) || (rc = dv.alloc(2 * ((int64_t)U + 1), &p.utt_off))) return rc;
  }
  DecodeOut o;
  if ((rc = decode_out_alloc(ctx, u, true, &dv, &o))) return rc;
  LsArgs a;
  decode_args(tm, u, o, &a);
  a.in_src = u->in_src_d; a.err_frame = o.err_frame;
  a.beam = cfg->beam; a.lattice_beam = cfg->lattice_beam; a.acoustic_scale = cfg->acoustic_scale;
  a.prune_interval = cfg->prune_interval; a.tok_cap = cfg->scratch_per_frame; a.amax = u->max_inarcs;
  a.hub = ctx->opt[KHG_OPT_K2S_HUB];
  // every utterance's dense rows, grouped into launches of <= 4 GiB of scratch (an utterance larger than that alone is refused)
  std::vector<int64_t> bytes((size_t)U);
  int64_t max_T = 0;
  for (int i = 0; i < U; ++i) {
    const int64_t T = u->frame_off[i + 1] - u->frame_off[i], S = utt_states(u, i);
    bytes[(size_t)i] = ls_layout(T, S, u->max_inarcs, lat).total;     // (the kernel lays every slice out with the same arc bound)
    if (bytes[(size_t)i] > kScratchBudget)
      return khg_set_error(KHG_E_ARG, who + ": utterance " + std::to_string(i) + " needs more than 4 GiB of lattice scratch");
    max_T = std::max(max_T, T);
  }
  std::vector<size_t> cb;
  std::vector<int64_t> rel;
  int64_t max_chunk = 0;
  split_by_budget(bytes, &cb, &rel, &max_chunk);
  unsigned char* scratch; int64_t* scr_off_d; int32_t* list_d;
  std::vector<int32_t> all((size_t)U);
  for (int i = 0; i < U; ++i) all[(size_t)i] = i;
  if ((rc = dv.alloc(max_chunk, &scratch)) || (rc = dv.upload(ctx, rel, &scr_off_d)) || (rc = dv.upload(ctx, all, &list_d))) return rc;
  a.scratch = scratch; a.scr_off = scr_off_d; a.list = list_d;
  p.a = a;
  // one wave for small graphs, up to four for larger ones (a lane owns states s = lane, lane + NT, ...)
  const int nt = u->max_states <= 64 ? 64 : u->max_states <= 128 ? 128 : LS_NT;
  for (size_t c = 0; c + 1 < cb.size(); ++c) {
    const int n = (int)(cb[c + 1] - cb[c]), u0 = (int)cb[c];
    if ((rc = launch(ctx, "k2_lattice_simple", k2_lattice_simple, dim3((unsigned)n), dim3(nt), 0, a, u0))) return rc;
    p.n = n;
    if (lat && (rc = simple_emit(ctx, p, u0, nt, max_T, lats.get()))) return rc;
    if (c + 2 < cb.size()) HIPCHK(hipStreamSynchronize(ctx->stream));     // the next launch reuses the slices
  }
  rc = check_err_flag(ctx, who.c_str());     // synchronises
  std::vector<int32_t> st;
  if (!rc) rc = decode_out_status(o, U, &st);
  if (!rc) rc = decode_out_download(ctx, who, o, st, ali_h, words_h, words_off_h, words_cap, like_h, status_h, err_frame_h);
  if (rc) return rc;
  if (lat) *lat_out = lats.release();
  return KHG_OK;
}
}  // namespace

extern "C" int khg_decode_lattice_simple(khg_ctx* ctx, const khg_tm* tm, khg_utts* u, const khg_lattice_simple_config* cfg,
                                         int32_t* ali_h, int32_t* words_h, int64_t* words_off_h, int64_t words_cap,
                                         double* like_h, int32_t* status_h, int32_t* err_frame_h) {
  return decode_lattice_simple_impl(ctx, tm, u, cfg, ali_h, words_h, words_off_h, words_cap, like_h, status_h, err_frame_h, nullptr);
}
extern "C" int khg_decode_lattice_simple_raw(khg_ctx* ctx, const khg_tm* tm, khg_utts* u, const khg_lattice_simple_config* cfg,
                                             int32_t* ali_h, int32_t* words_h, int64_t* words_off_h, int64_t words_cap,
                                             double* like_h, int32_t* status_h, int32_t* err_frame_h, khg_lattices** out) {
  if (!out) return khg_set_error(KHG_E_ARG, "khg_decode_lattice_simple_raw: out is NULL");
  *out = nullptr;
  return decode_lattice_simple_impl(ctx, tm, u, cfg, ali_h, words_h, words_off_h, words_cap, like_h, status_h, err_frame_h, out);
}

// ------------------------------------------------------------------------------------------
// K2O: operations on device-resident lattices (khg_k2_lattice_ops.hip.inc)
namespace {
const int64_t kLatOpsLds = 48 << 10;        // an utterance's lattice is staged into LDS up to this many bytes

void lat_chunk_args(const khg_lattices* l, const LatChunk& c, LoArgs* p) {
  lat_chunk_arrays(c, &p->in);
  p->start = l->start_d; p->state_off = l->off_d; p->arc_off = l->off_d + l->U + 1;
  p->s_base = l->state_off[(size_t)c.u0]; p->a_base = l->arc_off[(size_t)c.u0];
  p->u0 = c.u0; p->n = c.n; p->U = l->U;
}
// the dynamic LDS a launch over chunk c asks for: the largest lattice of the chunk that still fits, with per_state bytes of the kernel's
// own beside every staged state
int lat_chunk_lds(const khg_ctx* ctx, const khg_lattices* l, const LatChunk& c, int64_t per_state = 0) {
  if (ctx->opt[KHG_OPT_LAT_OPS_LDS] == 1) return 0;
  int64_t best = 0;
  for (int u = c.u0; u < c.u0 + c.n; ++u) {
    const int64_t N = l->state_off[(size_t)u + 1] - l->state_off[(size_t)u], A = l->arc_off[(size_t)u + 1] - l->arc_off[(size_t)u];
    const int64_t need = per_state * N + 4 * (3 * N + 4 * A);
    if (need <= kLatOpsLds) best = std::max(best, need);
  }
  return (int)best;
}
// the offsets on the device and the alignment layout, once per handle
int lat_meta(khg_ctx* ctx, khg_lattices* l) {
  if (l->off_d || l->U == 0) { if (l->ali_off.empty()) l->ali_off.assign((size_t)l->U + 1, 0); return KHG_OK; }
  const size_t U = (size_t)l->U;
  int64_t* off_d = nullptr;
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&off_d), 16 * (U + 1)));
  l->off_d = off_d;
  l->bytes += 16 * (int64_t)(U + 1);
  HIPCHK(hipMemcpyAsync(off_d, l->state_off.data(), 8 * (U + 1), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(off_d + U + 1, l->arc_off.data(), 8 * (U + 1), hipMemcpyHostToDevice, ctx->stream));
  DevBlocks dv;
  int32_t* t_d = nullptr;
  int rc = dv.alloc((int64_t)U, &t_d);
  if (rc) return rc;
  for (const LatChunk& c : l->chunks) {
    LoArgs p{};
    lat_chunk_args(l, c, &p);
    KHG_LAUNCH(ctx, k2_lattice_ops_last_frame, dim3((unsigned)((c.n + LO_NT - 1) / LO_NT)), dim3(LO_NT), 0, ctx->stream, p, t_d);
    HIPCHK(hipGetLastError());
  }
  std::vector<int32_t> t;
  if ((rc = download(ctx, t_d, (int64_t)U, &t))) return rc;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  l->ali_off.assign(U + 1, 0);
  for (size_t u = 0; u < U; ++u) l->ali_off[u + 1] = l->ali_off[u] + std::max(t[u], 0);
  return KHG_OK;
}
// The entry of an operation on a resident handle: the staged uploads out, then what the operation reads of the handle beside its
// arrays, each made once per handle -- always the offsets and the alignment layout (lat_meta), on request the in-arc index (lat_index)
// and the widest frames (lat_width)
enum { kWithIndex = 1, kWithWidth = 2 };
int lat_index(khg_ctx* ctx, khg_lattices* l);
int lat_width(khg_ctx* ctx, khg_lattices* l);
int lat_ready(khg_ctx* ctx, khg_lattices* l, int with = 0) {
  int rc = arena_flush(ctx);
  if (!rc) rc = lat_meta(ctx, l);
  if (!rc && (with & kWithIndex)) rc = lat_index(ctx, l);
  if (!rc && (with & kWithWidth)) rc = lat_width(ctx, l);
  return rc;
}
// What khg_lattices_best_path and khg_lattices_wer share: the K scale pairs on the device, and per chunk of l the arguments of a
// best-path kernel -- the chunk, its LDS, the pairs, the per-(pair, utterance) word counts and statuses, and the six arrays of a cell
// per (state, pair) -- in *pcs; the scratch is dv's
int best_path_args(khg_ctx* ctx, const khg_lattices* l, int K, const float* graph_scale, const float* acoustic_scale, int32_t* nw_d, int32_t* status_d,
                   DevBlocks* dv, std::vector<LoArgs>* pcs) {
  float *gs_d, *as_d;
  int rc;
  if ((rc = dv->upload(ctx, graph_scale, K, &gs_d)) || (rc = dv->upload(ctx, acoustic_scale, K, &as_d))) return rc;
  for (const LatChunk& c : l->chunks) {
    LoArgs p{};
    lat_chunk_args(l, c, &p);
    p.lds_bytes = lat_chunk_lds(ctx, l, c);
    p.K = K; p.gs = gs_d; p.as = as_d; p.nwords = nw_d; p.status = status_d;
    const int64_t cells = std::max<int64_t>(c.ns * K, 1);
    if ((rc = dv->alloc(cells, &p.d1)) || (rc = dv->alloc(cells, &p.d2)) || (rc = dv->alloc(cells, &p.n1)) || (rc = dv->alloc(cells, &p.n2)) ||
        (rc = dv->alloc(cells, &p.bp)) || (rc = dv->alloc(cells, &p.words)))
      return rc;
    pcs->push_back(p);
  }
  return KHG_OK;
}
// the largest count among the chunk's utterances in a handle's offsets
int64_t chunk_max(const std::vector<int64_t>& off, const LatChunk& c) {
  int64_t m = 0;
  for (int u = c.u0; u < c.u0 + c.n; ++u) m = std::max(m, off[(size_t)u + 1] - off[(size_t)u]);
  return m;
}
bool bad_scale(float x) { return !(x >= 0.0f) || x == std::numeric_limits<float>::infinity(); }
}  // namespace

extern "C" int khg_lattices_validate(int32_t n_utt, const int64_t* state_off, const int64_t* arc_off, const int32_t* frame, const int32_t* graph_state,
                                     const float* tot_cost, const float* extra_cost, const float* final_cost, const int32_t* arc_begin,
                                     const int32_t* ilabel, const int32_t* olabel, const float* graph_cost, const float* acoustic_cost,
                                     const int32_t* nextstate, const int32_t* start) {
  if (n_utt < 0 || !state_off || !arc_off || state_off[0] != 0 || arc_off[0] != 0)
    return khg_set_error(KHG_E_ARG, "khg_lattices_upload: bad arguments (offsets start at 0)");
  const int64_t NS = state_off[n_utt], NA = arc_off[n_utt];
  if ((NS > 0 && (!frame || !graph_state || !tot_cost || !extra_cost || !final_cost || !arc_begin)) ||
      (NA > 0 && (!ilabel || !olabel || !graph_cost || !acoustic_cost || !nextstate)) || (n_utt > 0 && !start))
    return khg_set_error(KHG_E_ARG, "khg_lattices_upload: bad arguments (an array is NULL)");
  for (int u = 0; u < n_utt; ++u) {
    const std::string who = "khg_lattices_upload: utterance " + std::to_string(u) + ": ";
    const int64_t s0 = state_off[u], a0 = arc_off[u], N = state_off[u + 1] - s0, A = arc_off[u + 1] - a0;
    if (N < 0 || A < 0 || N > INT32_MAX || A > INT32_MAX) return khg_set_error(KHG_E_ARG, who + "state_off / arc_off must not decrease (and stay below 2^31 per utterance)");
    if (N == 0) {
      if (A != 0) return khg_set_error(KHG_E_ARG, who + "arcs without states");
      if (start[u] != -1) return khg_set_error(KHG_E_ARG, who + "start out of range (an empty lattice has start -1)");
      continue;
    }
    if (arc_begin[s0] != 0) return khg_set_error(KHG_E_ARG, who + "arc_begin must run from 0 to the number of arcs");
    for (int64_t s = 0; s < N; ++s) {
      const int64_t end = s + 1 < N ? arc_begin[s0 + s + 1] : A;
      if (arc_begin[s0 + s] > end) return khg_set_error(KHG_E_ARG, who + "arc_begin not monotone");
      if (frame[s0 + s] < 0 || (s > 0 && frame[s0 + s] < frame[s0 + s - 1])) return khg_set_error(KHG_E_ARG, who + "states must be ordered by frame");
    }
    if (start[u] < 0 || start[u] >= N) return khg_set_error(KHG_E_ARG, who + "start out of range");
    if (frame[s0 + start[u]] != 0) return khg_set_error(KHG_E_ARG, who + "start must be on frame 0");
    for (int64_t s = 0; s < N; ++s) {
      const int64_t end = s + 1 < N ? arc_begin[s0 + s + 1] : A;
      for (int64_t a = arc_begin[s0 + s]; a < end; ++a) {
        const int32_t k = nextstate[a0 + a];
        if (k < 0 || k >= N) return khg_set_error(KHG_E_ARG, who + "nextstate out of range");
        if (ilabel[a0 + a] != 0 && frame[s0 + k] != frame[s0 + s] + 1)
          return khg_set_error(KHG_E_ARG, who + "an emitting arc must go from frame f to frame f + 1 (arc " + std::to_string(a) + ")");
        if (ilabel[a0 + a] == 0 && frame[s0 + k] != frame[s0 + s])
          return khg_set_error(KHG_E_ARG, who + "an epsilon arc must stay in its frame (arc " + std::to_string(a) + ")");
      }
    }
  }
  return KHG_OK;
}

extern "C" int khg_lattices_num_utts(const khg_lattices* l, int32_t* n_utt) {
  if (!l || !n_utt) return khg_set_error(KHG_E_ARG, "khg_lattices_num_utts: bad arguments");
  *n_utt = l->U;
  return KHG_OK;
}
extern "C" int khg_lattices_num_chunks(const khg_lattices* l, int32_t* n_chunks) {
  if (!l || !n_chunks) return khg_set_error(KHG_E_ARG, "khg_lattices_num_chunks: bad arguments");
  *n_chunks = (int32_t)l->chunks.size();
  return KHG_OK;
}
extern "C" int khg_lattices_chunk_utts(const khg_lattices* l, int32_t* first_utt) {
  if (!l || !first_utt) return khg_set_error(KHG_E_ARG, "khg_lattices_chunk_utts: bad arguments");
  for (size_t c = 0; c < l->chunks.size(); ++c) first_utt[c] = l->chunks[c].u0;
  first_utt[l->chunks.size()] = l->chunks.empty() ? 0 : l->U;
  return KHG_OK;
}
extern "C" int khg_lattices_ali_layout(khg_ctx* ctx, const khg_lattices* lc, int64_t* ali_off_h) {
  if (ctx_dead(ctx) || !lc || !ali_off_h) return khg_set_error(KHG_E_ARG, "khg_lattices_ali_layout: bad arguments");
  khg_lattices* l = const_cast<khg_lattices*>(lc);
  int rc = lat_ready(ctx, l);
  if (rc) return rc;
  std::copy(l->ali_off.begin(), l->ali_off.end(), ali_off_h);
  return KHG_OK;
}

extern "C" int khg_lattices_upload(khg_ctx* ctx, int32_t n_utt, const int64_t* state_off, const int64_t* arc_off, const int32_t* frame,
                                   const int32_t* graph_state, const float* tot_cost, const float* extra_cost, const float* final_cost,
                                   const int32_t* arc_begin, const int32_t* ilabel, const int32_t* olabel, const float* graph_cost,
                                   const float* acoustic_cost, const int32_t* nextstate, const int32_t* start, khg_lattices** out) {
  if (ctx_dead(ctx) || !out) return khg_set_error(KHG_E_ARG, "khg_lattices_upload: bad arguments");
  *out = nullptr;
  int rc = khg_lattices_validate(n_utt, state_off, arc_off, frame, graph_state, tot_cost, extra_cost, final_cost, arc_begin, ilabel, olabel,
                                 graph_cost, acoustic_cost, nextstate, start);
  if (rc) return rc;
  LatPtr l;
  if ((rc = new_lattices(ctx, n_utt, &l))) return rc;
  l->state_off.assign(state_off, state_off + n_utt + 1);
  l->arc_off.assign(arc_off, arc_off + n_utt + 1);
  if (n_utt == 0) { *out = l.release(); return KHG_OK; }
  LatChunk ch;
  ch.u0 = 0; ch.n = n_utt; ch.ns = state_off[n_utt]; ch.na = arc_off[n_utt];
  if ((rc = lat_chunk_alloc(&ch, &l->bytes))) return rc;
  l->chunks.push_back(ch);
  rc = arena_flush(ctx);
  if (rc) return rc;
  const void* st_h[6] = {frame, graph_state, tot_cost, extra_cost, final_cost, arc_begin};
  const void* ar_h[5] = {ilabel, olabel, graph_cost, acoustic_cost, nextstate};
  for (int k = 0; k < 6; ++k) if (ch.ns) HIPCHK(hipMemcpyAsync(ch.buf + ch.st[k], st_h[k], 4 * (size_t)ch.ns, hipMemcpyHostToDevice, ctx->stream));
  for (int k = 0; k < 5; ++k) if (ch.na) HIPCHK(hipMemcpyAsync(ch.buf + ch.ar[k], ar_h[k], 4 * (size_t)ch.na, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(l->start_d, start, 4 * (size_t)n_utt, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));        // the host arrays are the caller's again
  *out = l.release();
  return KHG_OK;
}

extern "C" int khg_lattices_best_path(khg_ctx* ctx, const khg_lattices* lc, int32_t n_scales, const float* graph_scale, const float* acoustic_scale,
                                      int32_t* ali_h, int32_t* words_h, int64_t* words_off_h, int64_t words_cap, float* weight_h, int32_t* status_h) {
  if (ctx_dead(ctx) || !lc || n_scales < 1 || !graph_scale || !acoustic_scale) return khg_set_error(KHG_E_ARG, "khg_lattices_best_path: bad arguments");
  for (int k = 0; k < n_scales; ++k)
    if (bad_scale(graph_scale[k]) || bad_scale(acoustic_scale[k]))
      return khg_set_error(KHG_E_ARG, "khg_lattices_best_path: scale pair " + std::to_string(k) + ": graph_scale and acoustic_scale must be finite and >= 0");
  khg_lattices* l = const_cast<khg_lattices*>(lc);
  const int U = l->U, K = n_scales;
  if (words_off_h) std::fill(words_off_h, words_off_h + (int64_t)K * U + 1, 0);
  if (U == 0) return KHG_OK;
  int rc = lat_ready(ctx, l);
  if (rc) return rc;
  const int64_t KU = (int64_t)K * U, AT = l->ali_off[(size_t)U];
  DevBlocks dv;
  int32_t *ali_d, *nw_d, *status_d, *packed_d;
  float* weight_d;
  int64_t *ali_off_d, *woff_d;
  std::vector<LoArgs> pcs;
  if ((rc = dv.zeroed(ctx, std::max<int64_t>((int64_t)K * AT, 1), &ali_d)) || (rc = dv.alloc(KU, &nw_d)) || (rc = dv.alloc(KU, &status_d)) ||
      (rc = dv.alloc(2 * KU, &weight_d)) || (rc = best_path_args(ctx, l, K, graph_scale, acoustic_scale, nw_d, status_d, &dv, &pcs)) ||
      (rc = dv.upload(ctx, l->ali_off, &ali_off_d)) || (rc = dv.alloc(KU + 1, &woff_d)))
    return rc;
  for (LoArgs& p : pcs) {
    p.ali = ali_d; p.ali_off = ali_off_d; p.ali_total = AT; p.weight = weight_d;
    if ((rc = launch(ctx, "k2_lattice_best_path", k2_lattice_best_path, dim3((unsigned)p.n, (unsigned)((K + LO_NT - 1) / LO_NT)), dim3(LO_NT), (size_t)p.lds_bytes, p)))
      return rc;
  }
  // the words, packed on the device: a scan of the counts, one synchronisation to size the block, the copy
  std::vector<int64_t> woff((size_t)KU + 1, 0);
  std::vector<int32_t> packed, st;
  if (words_h && words_off_h) {
    if ((rc = launch(ctx, "k2_lattice_ops_words", k2_lattice_ops_scan, dim3(1), dim3(64), 0, nw_d, woff_d, KU)) || (rc = download(ctx, woff_d, KU + 1, &woff)))
      return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const int64_t NW = woff[(size_t)KU];
    if ((rc = dv.alloc(std::max<int64_t>(NW, 1), &packed_d))) return rc;
    if (NW > 0) {
      KernelTimer kt(ctx, "k2_lattice_ops_words");
      for (const LoArgs& p : pcs)
        KHG_LAUNCH(ctx, k2_lattice_ops_pack_words, dim3((unsigned)p.n, (unsigned)std::min(K, 64)), dim3(LO_NT), 0, ctx->stream, p, woff_d, packed_d);
      HIPCHK(hipGetLastError());
      if ((rc = download(ctx, packed_d, NW, &packed))) return rc;
    }
  }
  if (ali_h && AT) HIPCHK(hipMemcpyAsync(ali_h, ali_d, 4 * (size_t)((int64_t)K * AT), hipMemcpyDeviceToHost, ctx->stream));
  if (weight_h) HIPCHK(hipMemcpyAsync(weight_h, weight_d, 8 * (size_t)KU, hipMemcpyDeviceToHost, ctx->stream));
  if ((rc = download(ctx, status_d, KU, &st)) || (rc = check_err_flag(ctx, "khg_lattices_best_path"))) return rc;     // synchronises
  if (words_h && words_off_h &&       // (a path whose words do not fit: KHG_LAT_WORDS and none of them)
      (rc = pack_words("khg_lattices_best_path", st, &st, [&](size_t i) { return woff[i + 1] - woff[i]; },
                       [&](size_t i, int64_t) { return packed.begin() + woff[i]; }, words_h, words_off_h, words_cap)))
    return rc;
  if (status_h) std::copy(st.begin(), st.end(), status_h);
  return KHG_OK;
}

extern "C" int khg_lattices_prune(khg_ctx* ctx, const khg_lattices* lc, float graph_scale, float acoustic_scale, float beam, int32_t* status_h,
                                  khg_lattices** out) {
  if (ctx_dead(ctx) || !lc || !out) return khg_set_error(KHG_E_ARG, "khg_lattices_prune: bad arguments");
  *out = nullptr;
  if (bad_scale(graph_scale) || bad_scale(acoustic_scale))
    return khg_set_error(KHG_E_ARG, "khg_lattices_prune: graph_scale and acoustic_scale must be finite and >= 0");
  if (!(beam >= 0.0f)) return khg_set_error(KHG_E_ARG, "khg_lattices_prune: beam must be >= 0 (+inf allowed)");
  khg_lattices* l = const_cast<khg_lattices*>(lc);
  const int U = l->U;
  LatPtr res;
  int rc = new_lattices(ctx, U, &res);
  if (rc) return rc;
  if (U == 0) { *out = res.release(); return KHG_OK; }
  if ((rc = lat_ready(ctx, l))) return rc;
  DevBlocks dv;
  int32_t* status_d;
  if ((rc = dv.alloc(U, &status_d))) return rc;
  for (const LatChunk& c : l->chunks) {
    LoArgs p{};
    lat_chunk_args(l, c, &p);
    p.lds_bytes = lat_chunk_lds(ctx, l, c);
    p.K = 1; p.gs1 = graph_scale; p.as1 = acoustic_scale; p.beam = beam; p.status = status_d; p.o_start = res->start_d;
    const int64_t cells = std::max<int64_t>(c.ns, 1);
    if ((rc = dv.alloc(cells, &p.d1)) || (rc = dv.alloc(cells, &p.d2)) || (rc = dv.alloc(cells, &p.n1)) || (rc = dv.alloc(cells, &p.n2)) ||
        (rc = dv.alloc(cells, &p.e1)) || (rc = dv.alloc(cells, &p.e2)) || (rc = dv.alloc(cells, &p.bp)) || (rc = dv.alloc(cells, &p.pn)) ||
        (rc = dv.alloc(cells, &p.newid)) || (rc = dv.alloc(cells, &p.nab)) || (rc = dv.alloc(c.n, &p.limit)) ||
        (rc = dv.alloc(2 * (int64_t)c.n, &p.utt_tot)) || (rc = dv.alloc(2 * ((int64_t)c.n + 1), &p.utt_off)))
      return rc;
    LatChunk ch;
    if ((rc = launch(ctx, "k2_lattice_prune_mark", k2_lattice_prune_mark, dim3((unsigned)c.n), dim3(LO_NT), (size_t)p.lds_bytes, p)) ||
        (rc = size_out_chunk(ctx, "khg_lattices_prune", "k2_lattice_prune_scan", p.utt_tot, p.utt_off, c.u0, c.n, res.get(), &ch)))      // the one synchronisation that sizes the output
      return rc;
    lat_chunk_arrays(ch, &p.out);
    if ((rc = launch(ctx, "k2_lattice_prune_fill", k2_lattice_prune_fill, dim3((unsigned)c.n, stripes(chunk_max(l->state_off, c), LO_NT, c.n)), dim3(LO_NT), 0, p)))
      return rc;
  }
  std::vector<int32_t> st;
  if ((rc = download(ctx, status_d, U, &st)) || (rc = check_err_flag(ctx, "khg_lattices_prune"))) return rc;     // synchronises: the scratch goes with `dv`
  if (status_h) std::copy(st.begin(), st.end(), status_h);
  *out = res.release();
  return KHG_OK;
}

// ------------------------------------------------------------------------------------------
// K2P: forward-backward posteriors of device-resident lattices (khg_k2_lattice_post.hip.inc)
struct PostChunk {
  int u0 = 0, n = 0;
  int64_t nf = 0, ne = 0, na = 0;      // frames, entries, arcs
  double* arc_post = nullptr;          // [na], the lattice handle's arc order
  unsigned char* buf = nullptr;        // entry_begin int64 [nf + 1] (relative to the chunk) | weight double [ne] | tid int32 [ne]
  int64_t o_weight = 0, o_tid = 0;
};
struct khg_posteriors {
  int U = 0;
  std::vector<int64_t> frame_off, entry_off, arc_off;     // [U + 1]
  std::vector<PostChunk> chunks;
  int64_t bytes = 0;
  khg_ctx* ctx = nullptr;              // the context it was made on
  int32_t max_tid = -1;                // khg_posteriors_upload: the largest id (0: no entries); -1: made from lattices (the graph's labels)
  int64_t* frame_off_d = nullptr;      // [U + 1] frame_off on the device, made with the handle (posteriors_flatten reads it)
};

namespace {
struct PostFree { void operator()(khg_posteriors* p) const { (void)khg_posteriors_destroy(p); } };
using PostPtr = std::unique_ptr<khg_posteriors, PostFree>;
// an empty handle of U utterances: every offset 0
void new_posteriors(khg_ctx* ctx, int U, PostPtr* out) {
  out->reset(new khg_posteriors);
  (*out)->U = U; (*out)->ctx = ctx;
  (*out)->frame_off.assign((size_t)U + 1, 0);
  (*out)->entry_off.assign((size_t)U + 1, 0);
  (*out)->arc_off.assign((size_t)U + 1, 0);
}
// the entry block of a chunk whose nf and ne are set: entry_begin | weight | tid, each at a multiple of 256 bytes; its size is added to *bytes
int post_chunk_alloc(PostChunk* q, int64_t* bytes) {
  q->o_weight = (8 * (q->nf + 1) + 255) & ~int64_t(255);
  q->o_tid = q->o_weight + ((8 * q->ne + 255) & ~int64_t(255));
  const int64_t total = q->o_tid + 4 * q->ne;
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&q->buf), (size_t)std::max<int64_t>(total, 16)));
  *bytes += total;
  return KHG_OK;
}
struct PostArrays { int64_t* entry_begin; double* weight; int32_t* tid; };
PostArrays post_chunk_arrays(const PostChunk& c) {
  return {reinterpret_cast<int64_t*>(c.buf), reinterpret_cast<double*>(c.buf + c.o_weight), reinterpret_cast<int32_t*>(c.buf + c.o_tid)};
}

// The in-arc index block of a lattice chunk (int32): in_begin [ns + n] (N + 1 per utterance) | in_arc [na] | arc_src [na]
struct LatIndex { int32_t *in_begin, *in_arc, *arc_src; };
int64_t lat_index_words(const LatChunk& c) { return c.ns + c.n + 2 * c.na; }
LatIndex lat_index_arrays(int32_t* blk, const LatChunk& c) { return {blk, blk + c.ns + c.n, blk + c.ns + c.n + c.na}; }
// chunk c's block, as the next of l's; counted in l's bytes
int lat_index_alloc(khg_lattices* l, const LatChunk& c, int32_t** blk) {
  *blk = nullptr;
  HIPCHK(hipMalloc(reinterpret_cast<void**>(blk), (size_t)std::max<int64_t>(4 * lat_index_words(c), 16)));
  l->idx_d.push_back(*blk);
  l->bytes += 4 * lat_index_words(c);
  return KHG_OK;
}
// the in-arc index, once per handle
int lat_index(khg_ctx* ctx, khg_lattices* l) {
  if (l->idx_d.size() == l->chunks.size()) return KHG_OK;
  DevBlocks dv;
  for (size_t k = l->idx_d.size(); k < l->chunks.size(); ++k) {
    const LatChunk& c = l->chunks[k];
    int32_t *blk, *cur = nullptr;
    int rc = lat_index_alloc(l, c, &blk);
    if (!rc) rc = dv.alloc(std::max<int64_t>(c.ns, 1), &cur);
    if (rc) return rc;
    const LatIndex ix = lat_index_arrays(blk, c);
    LoArgs p{};
    lat_chunk_args(l, c, &p);
    if ((rc = launch(ctx, "k2_lattice_post_index", k2_lattice_post_index, dim3((unsigned)c.n), dim3(64), 0, p, ix.in_begin, ix.in_arc, ix.arc_src, cur))) return rc;
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));       // the cursors go with `dv`
  return KHG_OK;
}
// the handle's frame offsets on the device (not counted in its bytes: 8 (U + 1)); synchronous, so a handle either has them or is not made
int post_frame_off_upload(khg_ctx* ctx, khg_posteriors* p) {
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&p->frame_off_d), 8 * ((size_t)p->U + 1)));
  HIPCHK(hipMemcpyAsync(p->frame_off_d, p->frame_off.data(), 8 * ((size_t)p->U + 1), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return KHG_OK;
}
}  // namespace

extern "C" int khg_posteriors_destroy(khg_posteriors* p) {
  if (!p) return KHG_OK;
  for (PostChunk& c : p->chunks) {
    if (c.arc_post) (void)hipFree(c.arc_post);
    if (c.buf) (void)hipFree(c.buf);
  }
  if (p->frame_off_d) (void)hipFree(p->frame_off_d);
  delete p;
  return KHG_OK;
}
extern "C" int khg_posteriors_sizes(const khg_posteriors* p, int64_t* frame_off_h, int64_t* entry_off_h) {
  if (!p) return khg_set_error(KHG_E_ARG, "khg_posteriors_sizes: bad arguments");
  if (frame_off_h) std::copy(p->frame_off.begin(), p->frame_off.end(), frame_off_h);
  if (entry_off_h) std::copy(p->entry_off.begin(), p->entry_off.end(), entry_off_h);
  return KHG_OK;
}
extern "C" int khg_posteriors_device_bytes(const khg_posteriors* p, int64_t* bytes) {
  if (!p || !bytes) return khg_set_error(KHG_E_ARG, "khg_posteriors_device_bytes: bad arguments");
  *bytes = p->bytes;
  return KHG_OK;
}
extern "C" int khg_posteriors_download(khg_ctx* ctx, const khg_posteriors* p, int64_t* entry_begin_h, int32_t* tid_h, double* weight_h,
                                       double* arc_post_h) {
  if (ctx_dead(ctx) || !p) return khg_set_error(KHG_E_ARG, "khg_posteriors_download: bad arguments");
  if (entry_begin_h) entry_begin_h[0] = 0;
  for (const PostChunk& c : p->chunks) {
    const int64_t f0 = p->frame_off[(size_t)c.u0], e0 = p->entry_off[(size_t)c.u0], a0 = p->arc_off[(size_t)c.u0];
    if (entry_begin_h) HIPCHK(hipMemcpyAsync(entry_begin_h + f0, c.buf, 8 * ((size_t)c.nf + 1), hipMemcpyDeviceToHost, ctx->stream));
    if (weight_h && c.ne) HIPCHK(hipMemcpyAsync(weight_h + e0, c.buf + c.o_weight, 8 * (size_t)c.ne, hipMemcpyDeviceToHost, ctx->stream));
    if (tid_h && c.ne) HIPCHK(hipMemcpyAsync(tid_h + e0, c.buf + c.o_tid, 4 * (size_t)c.ne, hipMemcpyDeviceToHost, ctx->stream));
    if (arc_post_h && c.na) HIPCHK(hipMemcpyAsync(arc_post_h + a0, c.arc_post, 8 * (size_t)c.na, hipMemcpyDeviceToHost, ctx->stream));
    // a chunk's entry_begin counts from the chunk's first entry; chunk k + 1's first element lands on chunk k's last
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (entry_begin_h) for (int64_t f = 0; f <= c.nf; ++f) entry_begin_h[f0 + f] += e0;
  }
  return KHG_OK;
}

namespace {
// One call of khg_lattices_posteriors / khg_lattices_mpe_posteriors: what its chunks share.  Per chunk the caller runs post_chunk_begin,
// its own kernel (k2_lattice_post_fb, k2_lattice_post_mpe) under its own timer, and post_chunk_finish; post_run_finish ends the call.
struct PostRun {
  khg_ctx* ctx; khg_lattices* l;
  const char* who;                     // the call that the errors name
  double gs, as;
  PostPtr res;
  DevBlocks dv;                        // the call's scratch, every chunk's: freed on the way out
  int32_t* status_d = nullptr; double* tot_d = nullptr; int64_t* ali_off_d = nullptr;      // [U], [U], [U + 1]
};
// (U > 0, after lat_meta) the per-utterance results and the alignment layout on the device
int post_run_begin(PostRun& r) {
  const int U = r.l->U;
  int rc;
  if ((rc = r.dv.alloc(U, &r.status_d)) || (rc = r.dv.alloc(U, &r.tot_d))) return rc;
  return r.dv.upload(r.ctx, r.l->ali_off, &r.ali_off_d);
}
// chunk k's kernel arguments (*p zeroed by the caller) with the scratch both kernels need, and the result's chunk with its arc_post.
// per_state: the bytes a kernel keeps in LDS beside every staged state (its doubles: 24 or 40)
int post_chunk_begin(PostRun& r, size_t k, int64_t per_state, PoArgs* p) {
  khg_lattices* l = r.l;
  const LatChunk& c = l->chunks[k];
  lat_chunk_args(l, c, &p->lo);
  p->lo.lds_bytes = lat_chunk_lds(r.ctx, l, c, per_state);
  p->lo.status = r.status_d; p->lo.ali_off = r.ali_off_d; p->tot = r.tot_d;
  const LatIndex ix = lat_index_arrays(l->idx_d[k], c);
  p->in_begin = ix.in_begin; p->in_arc = ix.in_arc; p->arc_src = ix.arc_src;
  p->gs = r.gs; p->as = r.as;
  p->f_base = l->ali_off[(size_t)c.u0];
  const int64_t nfr = l->ali_off[(size_t)c.u0 + c.n] - p->f_base;
  const int64_t cells = std::max<int64_t>(c.ns, 1), arcs = std::max<int64_t>(c.na, 1);
  int rc;
  if ((rc = r.dv.alloc(cells, &p->alpha)) || (rc = r.dv.alloc(cells, &p->beta)) || (rc = r.dv.alloc(cells, &p->row)) || (rc = r.dv.alloc(arcs, &p->flag)) ||
      (rc = r.dv.alloc(arcs, &p->rank)) || (rc = r.dv.alloc(std::max<int64_t>(nfr, 1), &p->fcnt)) || (rc = r.dv.alloc(nfr + 2 * (int64_t)c.n, &p->fstate)) ||
      (rc = r.dv.alloc(2 * (int64_t)c.n, &p->lo.utt_tot)) || (rc = r.dv.alloc(2 * ((int64_t)c.n + 1), &p->lo.utt_off)))
    return rc;
  PostChunk pc;
  pc.u0 = c.u0; pc.n = c.n; pc.na = c.na;
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&pc.arc_post), (size_t)(8 * arcs)));
  r.res->chunks.push_back(pc);
  r.res->bytes += 8 * c.na;
  p->arc_post = pc.arc_post;
  return KHG_OK;
}
// after the chunk's kernel: the scan of its (frames, entries) pairs, the ONE synchronisation that sizes the entry block, the fill (which
// sums arc_post as the kernel left it)
int post_chunk_finish(PostRun& r, size_t k, PoArgs* p) {
  khg_ctx* ctx = r.ctx;
  const LatChunk& c = r.l->chunks[k];
  std::vector<int64_t> fo, eo;       // frames at [b], entries at [n + 1 + b]
  int rc = scan_pairs_and_read(ctx, "k2_lattice_post_scan", p->lo.utt_tot, p->lo.utt_off, c.n, &fo, &eo);
  if (!rc) rc = add_chunk_counts(r.who, c.u0, fo, eo, &r.res->frame_off, &r.res->entry_off);
  if (rc) return rc;
  PostChunk& q = r.res->chunks.back();
  q.nf = fo[(size_t)c.n]; q.ne = eo[(size_t)c.n];
  if ((rc = post_chunk_alloc(&q, &r.res->bytes))) return rc;
  const PostArrays pa = post_chunk_arrays(q);
  p->entry_begin = pa.entry_begin; p->weight = pa.weight; p->tid = pa.tid;
  return launch(ctx, "k2_lattice_post_fill", k2_lattice_post_fill, dim3((unsigned)c.n, stripes(chunk_max(r.l->arc_off, c), PO_NT, c.n)), dim3(PO_NT), 0, *p);
}
// the statuses and totals back -- and one more double per utterance, extra_d to extra_h, when the caller has one -- and the handle out
int post_run_finish(PostRun& r, int32_t* status_h, double* tot_like_h, const double* extra_d, double* extra_h, khg_posteriors** out) {
  const int64_t U = r.l->U;
  std::vector<int32_t> st;
  std::vector<double> tl, ex;
  int rc;
  if ((rc = download(r.ctx, r.status_d, U, &st)) || (rc = download(r.ctx, r.tot_d, U, &tl)) || (rc = download(r.ctx, extra_d, extra_d ? U : 0, &ex)) ||
      (rc = check_err_flag(r.ctx, r.who)))     // synchronises: the scratch goes with the run
    return rc;
  if (status_h) std::copy(st.begin(), st.end(), status_h);
  if (tot_like_h) std::copy(tl.begin(), tl.end(), tot_like_h);
  if (extra_h) std::copy(ex.begin(), ex.end(), extra_h);
  if ((rc = post_frame_off_upload(r.ctx, r.res.get()))) return rc;
  *out = r.res.release();
  return KHG_OK;
}
}  // namespace

extern "C" int khg_lattices_posteriors(khg_ctx* ctx, const khg_lattices* lc, float graph_scale, float acoustic_scale, int32_t* status_h,
                                       double* tot_like_h, khg_posteriors** out) {
  if (ctx_dead(ctx) || !lc || !out) return khg_set_error(KHG_E_ARG, "khg_lattices_posteriors: bad arguments");
  *out = nullptr;
  if (bad_scale(graph_scale) || bad_scale(acoustic_scale))
    return khg_set_error(KHG_E_ARG, "khg_lattices_posteriors: graph_scale and acoustic_scale must be finite and >= 0");
  PostRun r;
  r.ctx = ctx; r.l = const_cast<khg_lattices*>(lc); r.who = "khg_lattices_posteriors";
  r.gs = (double)graph_scale; r.as = (double)acoustic_scale;
  new_posteriors(ctx, r.l->U, &r.res);
  r.res->arc_off = r.l->arc_off;
  if (r.l->U == 0) { *out = r.res.release(); return KHG_OK; }
  int rc = lat_ready(ctx, r.l, kWithIndex);
  if (!rc) rc = post_run_begin(r);
  if (rc) return rc;
  for (size_t k = 0; k < r.l->chunks.size(); ++k) {
    PoArgs p{};
    if ((rc = post_chunk_begin(r, k, 24, &p)) ||       // alpha, beta and the Jacobi row (doubles) beside the staged lattice
        (rc = launch(ctx, "k2_lattice_post_fb", k2_lattice_post_fb, dim3((unsigned)r.l->chunks[k].n), dim3(PO_NT), (size_t)p.lo.lds_bytes, p)) ||
        (rc = post_chunk_finish(r, k, &p)))
      return rc;
  }
  return post_run_finish(r, status_h, tot_like_h, nullptr, nullptr, out);
}

// ------------------------------------------------------------------------------------------
// Posteriors from host arrays (ali-to-post, weight-silence-post, hand-made ones): one chunk in the layout of khg_lattices_posteriors',
// without arc posteriors.
extern "C" int khg_posteriors_validate(int32_t n_utt, const int64_t* frame_off_h, const int64_t* entry_begin_h, int64_t n_entries,
                                       const int32_t* tid_h, const double* weight_h) {
  const std::string who = "khg_posteriors_validate: ";
  if (n_utt < 0 || !frame_off_h || !entry_begin_h || n_entries < 0 || (n_entries > 0 && (!tid_h || !weight_h)))
    return khg_set_error(KHG_E_ARG, who + "bad arguments");
  int rc = check_offsets("khg_posteriors_validate", "frame_off", frame_off_h, n_utt, "utterance");
  if (rc) return rc;
  const int64_t F = frame_off_h[n_utt];
  if ((rc = check_offsets("khg_posteriors_validate", "entry_begin", entry_begin_h, F, "frame"))) return rc;
  if (entry_begin_h[F] != n_entries)
    return khg_set_error(KHG_E_ARG, who + "entry_begin ends at " + std::to_string(entry_begin_h[F]) + ", the entries number " + std::to_string(n_entries));
  for (int64_t e = 0; e < n_entries; ++e) {
    if (tid_h[e] < 1) return khg_set_error(KHG_E_ARG, who + "entry " + std::to_string(e) + " has transition-id " + std::to_string(tid_h[e]) + " (ids start at 1)");
    if (!std::isfinite(weight_h[e])) return khg_set_error(KHG_E_ARG, who + "entry " + std::to_string(e) + " has a weight that is not finite");
  }
  return KHG_OK;
}
extern "C" int khg_posteriors_upload(khg_ctx* ctx, int32_t n_utt, const int64_t* frame_off_h, const int64_t* entry_begin_h, const int32_t* tid_h,
                                     const double* weight_h, khg_posteriors** out) {
  if (ctx_dead(ctx) || !out) return khg_set_error(KHG_E_ARG, "khg_posteriors_upload: bad arguments");
  *out = nullptr;
  if (n_utt < 0 || !frame_off_h || !entry_begin_h || frame_off_h[0] != 0) return khg_set_error(KHG_E_ARG, "khg_posteriors_upload: bad arguments");
  int rc = check_offsets("khg_posteriors_upload", "frame_off", frame_off_h, n_utt, "utterance");      // (entry_begin's length comes from frame_off: checked before it is read)
  if (rc) return rc;
  const int64_t F = frame_off_h[n_utt], E = entry_begin_h[F];
  if ((rc = khg_posteriors_validate(n_utt, frame_off_h, entry_begin_h, E, tid_h, weight_h))) return rc;
  PostPtr res;
  new_posteriors(ctx, n_utt, &res);
  res->frame_off.assign(frame_off_h, frame_off_h + n_utt + 1);
  for (int u = 0; u <= n_utt; ++u) res->entry_off[(size_t)u] = entry_begin_h[frame_off_h[u]];
  res->max_tid = 0;
  for (int64_t e = 0; e < E; ++e) res->max_tid = std::max(res->max_tid, tid_h[e]);
  if (n_utt == 0) { *out = res.release(); return KHG_OK; }
  PostChunk q;
  q.u0 = 0; q.n = n_utt; q.nf = F; q.ne = E;
  if ((rc = post_chunk_alloc(&q, &res->bytes))) return rc;
  res->chunks.push_back(q);
  const PostArrays pa = post_chunk_arrays(q);
  HIPCHK(hipMemcpyAsync(pa.entry_begin, entry_begin_h, 8 * ((size_t)F + 1), hipMemcpyHostToDevice, ctx->stream));
  if (E) {
    HIPCHK(hipMemcpyAsync(pa.weight, weight_h, 8 * (size_t)E, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(pa.tid, tid_h, 4 * (size_t)E, hipMemcpyHostToDevice, ctx->stream));
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));        // the caller's arrays are free again
  if ((rc = post_frame_off_upload(ctx, res.get()))) return rc;
  *out = res.release();
  return KHG_OK;
}

// A handle of one entry per frame whose arrays the CALLER fills on the device (khg_posteriors_from_ali, khg_fmllr.hip): frame_off_h
// [n_utt + 1] as in khg_posteriors_upload; the three arrays of the single chunk (entry_begin [F + 1], weight / tid [F]) and the
// handle's frame offsets on the device come back.  max_tid = -1: the ids are checked where they are read, as a lattice's are.
int posteriors_make_unit(khg_ctx* ctx, int32_t n_utt, const int64_t* frame_off_h, int64_t** entry_begin_d, double** weight_d, int32_t** tid_d,
                         const int64_t** frame_off_d, khg_posteriors** out) {
  PostPtr res;
  new_posteriors(ctx, n_utt, &res);
  res->frame_off.assign(frame_off_h, frame_off_h + n_utt + 1);
  res->entry_off = res->frame_off;
  *entry_begin_d = nullptr; *weight_d = nullptr; *tid_d = nullptr; *frame_off_d = nullptr;
  if (n_utt == 0) { *out = res.release(); return KHG_OK; }
  PostChunk q;
  q.u0 = 0; q.n = n_utt; q.nf = q.ne = frame_off_h[n_utt];
  int rc = post_chunk_alloc(&q, &res->bytes);
  if (rc) return rc;
  res->chunks.push_back(q);
  if ((rc = post_frame_off_upload(ctx, res.get()))) return rc;
  const PostArrays pa = post_chunk_arrays(q);
  *entry_begin_d = pa.entry_begin; *weight_d = pa.weight; *tid_d = pa.tid; *frame_off_d = res->frame_off_d;
  *out = res.release();
  return KHG_OK;
}

// ------------------------------------------------------------------------------------------
// What khg_acc_stats_post (khg_k3.hip) reads of a handle: its sizes, and its entries flattened into three arrays.
void posteriors_info(const khg_posteriors* p, PostInfo* out) {
  out->ctx = p->ctx; out->U = p->U; out->max_tid = p->max_tid;
  out->frame_off = p->frame_off.data(); out->entry_off = p->entry_off.data();
}
struct PostFlatArgs {
  const int64_t* entry_begin;       // [nf + 1], relative to the chunk
  const double* weight; const int32_t* tid;
  const int64_t* post_frame_off;    // [n + 1] the handle's frame offsets of the chunk's utterances; [0] is the chunk's first frame
  const int64_t* set_frame_off;     // [n + 1] the utterance set's
  int64_t nf, ne;
  int32_t n, num_tids;
  double scale;
  int32_t sign;                     // khg_acc_stats_post2's selection: > 0 the positive weights as they are, < 0 the negative ones as |w|,
                                    // the others 0; 0: every weight as it is
  int32_t* e_row; int32_t* e_tid; float* e_w;      // at the chunk's first entry
  int32_t* err_flag;
};
// One thread per entry: its frame is the last f with entry_begin[f] <= e (empty frames repeat a value), its utterance the last b whose
// first frame is <= f (utterances without frames repeat one).  No atomics but the error word's.
__global__ __launch_bounds__(256) void k3_post_flatten(PostFlatArgs p) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int64_t f0 = p.post_frame_off[0];
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < p.ne; e += stride) {
    int64_t lo = 0, hi = p.nf;                       // entry_begin[lo] <= e < entry_begin[hi]
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (p.entry_begin[mid] <= e) lo = mid; else hi = mid;
    }
    const int64_t f = lo;
    int blo = 0, bhi = p.n;                          // post_frame_off[blo] - f0 <= f < post_frame_off[bhi] - f0
    while (bhi - blo > 1) {
      const int mid = (blo + bhi) >> 1;
      if (p.post_frame_off[mid] - f0 <= f) blo = mid; else bhi = mid;
    }
    const int64_t row = p.set_frame_off[blo] + (f - (p.post_frame_off[blo] - f0));
    int32_t tid = p.tid[e];
    float w = (float)(p.scale * p.weight[e]);        // one rounding
    if (tid < 1 || tid > p.num_tids) { atomicOr(p.err_flag, 4); tid = 0; w = 0.0f; }
    // |scale * w64| beyond float: an infinite weight would poison the block unseen (only ll is checked later): dropped like a bad id,
    // and the error word says overflow
    if (!(fabsf(w) <= 3.0e38f)) { atomicOr(p.err_flag, 1); tid = 0; w = 0.0f; }
    if (p.sign != 0) w = p.sign > 0 ? (w > 0.0f ? w : 0.0f) : (w < 0.0f ? -w : 0.0f);
    p.e_row[e] = (int32_t)row; p.e_tid[e] = tid; p.e_w[e] = w;
  }
}
int posteriors_flatten(khg_ctx* ctx, const khg_posteriors* p, const int64_t* set_frame_off_d, double scale, int32_t num_tids, int32_t* e_row,
                       int32_t* e_tid, float* e_w, int sign) {
  if (!p->frame_off_d) return KHG_OK;               // a handle of no utterances
  KernelTimer kt(ctx, "k3_post_flatten");
  for (const PostChunk& c : p->chunks) {
    if (c.ne == 0) continue;
    const int64_t e0 = p->entry_off[(size_t)c.u0];
    PostFlatArgs a;
    const PostArrays pa = post_chunk_arrays(c);
    a.entry_begin = pa.entry_begin; a.weight = pa.weight; a.tid = pa.tid;
    a.post_frame_off = p->frame_off_d + c.u0; a.set_frame_off = set_frame_off_d + c.u0;
    a.nf = c.nf; a.ne = c.ne; a.n = c.n; a.num_tids = num_tids; a.scale = scale; a.sign = (int32_t)sign;
    a.e_row = e_row + e0; a.e_tid = e_tid + e0; a.e_w = e_w + e0; a.err_flag = ctx->err_flag_d;
    KHG_LAUNCH(ctx, k3_post_flatten, dim3((unsigned)std::min<int64_t>(4096, (c.ne + 255) / 256)), dim3(256), 0, ctx->stream, a);
    HIPCHK(hipGetLastError());
  }
  return KHG_OK;
}

// ------------------------------------------------------------------------------------------
// K2X: rescoring and boosting (khg_k2_lattice_rescore.hip.inc, khg_k1_cells.hip.inc).  Both make a copy of the handle
// -- the utterances in `drop` left empty -- and then change one per-arc array of the copy in place.
namespace {
// A new handle with l's chunks; the lattice of an utterance u with drop[u] != 0 is left empty.  Whole arrays are copied on the device
// (a chunk with dropped utterances: the runs of kept ones).  Without a dropped utterance the offsets on the device, the alignment layout
// and the in-arc index go along when l has them: the structure is the same.
int lat_clone(khg_ctx* ctx, const khg_lattices* l, const std::vector<char>& drop, LatPtr* out) {
  const int U = l->U;
  LatPtr r;
  int rc = new_lattices(ctx, U, &r);
  if (rc) return rc;
  bool any = false;
  for (int u = 0; u < U; ++u) {
    const bool d = drop[(size_t)u] != 0;
    any = any || d;
    r->state_off[(size_t)u + 1] = r->state_off[(size_t)u] + (d ? 0 : l->state_off[(size_t)u + 1] - l->state_off[(size_t)u]);
    r->arc_off[(size_t)u + 1] = r->arc_off[(size_t)u] + (d ? 0 : l->arc_off[(size_t)u + 1] - l->arc_off[(size_t)u]);
  }
  if (U > 0) HIPCHK(hipMemcpyAsync(r->start_d, l->start_d, 4 * (size_t)U, hipMemcpyDeviceToDevice, ctx->stream));
  for (int u = 0; u < U; ++u)
    if (drop[(size_t)u]) HIPCHK(hipMemsetAsync(r->start_d + u, 0xFF, 4, ctx->stream));      // -1
  for (const LatChunk& c : l->chunks) {
    LatChunk ch;
    ch.u0 = c.u0; ch.n = c.n;
    ch.ns = r->state_off[(size_t)c.u0 + c.n] - r->state_off[(size_t)c.u0];
    ch.na = r->arc_off[(size_t)c.u0 + c.n] - r->arc_off[(size_t)c.u0];
    if ((rc = lat_chunk_alloc(&ch, &r->bytes))) return rc;
    r->chunks.push_back(ch);
    for (int ua = c.u0; ua < c.u0 + c.n;) {          // runs of kept utterances
      if (drop[(size_t)ua]) { ++ua; continue; }
      int ub = ua;
      while (ub < c.u0 + c.n && !drop[(size_t)ub]) ++ub;
      const int64_t ss = l->state_off[(size_t)ua] - l->state_off[(size_t)c.u0], ds = r->state_off[(size_t)ua] - r->state_off[(size_t)c.u0];
      const int64_t sa = l->arc_off[(size_t)ua] - l->arc_off[(size_t)c.u0], da = r->arc_off[(size_t)ua] - r->arc_off[(size_t)c.u0];
      const int64_t ns = l->state_off[(size_t)ub] - l->state_off[(size_t)ua], na = l->arc_off[(size_t)ub] - l->arc_off[(size_t)ua];
      for (int k = 0; k < 6 && ns > 0; ++k)
        HIPCHK(hipMemcpyAsync(ch.buf + ch.st[k] + 4 * ds, c.buf + c.st[k] + 4 * ss, 4 * (size_t)ns, hipMemcpyDeviceToDevice, ctx->stream));
      for (int k = 0; k < 5 && na > 0; ++k)
        HIPCHK(hipMemcpyAsync(ch.buf + ch.ar[k] + 4 * da, c.buf + c.ar[k] + 4 * sa, 4 * (size_t)na, hipMemcpyDeviceToDevice, ctx->stream));
      ua = ub;
    }
  }
  if (!any && U > 0) {
    if (l->off_d) {
      HIPCHK(hipMalloc(reinterpret_cast<void**>(&r->off_d), 16 * ((size_t)U + 1)));
      r->bytes += 16 * ((int64_t)U + 1);
      HIPCHK(hipMemcpyAsync(r->off_d, l->off_d, 16 * ((size_t)U + 1), hipMemcpyDeviceToDevice, ctx->stream));
      r->ali_off = l->ali_off;
    }
    if (!l->chunks.empty() && l->idx_d.size() == l->chunks.size()) {
      for (size_t k = 0; k < l->chunks.size(); ++k) {
        const LatChunk& c = l->chunks[k];
        int32_t* blk;
        if ((rc = lat_index_alloc(r.get(), c, &blk))) return rc;
        HIPCHK(hipMemcpyAsync(blk, l->idx_d[k], 4 * (size_t)lat_index_words(c), hipMemcpyDeviceToDevice, ctx->stream));
      }
    }
  }
  *out = std::move(r);
  return KHG_OK;
}
void k2x_chunk(const khg_lattices* l, const LatChunk& c, K2xChunk* p) {
  lat_chunk_arrays(c, &p->io);
  p->state_off = l->off_d; p->arc_off = l->off_d + l->U + 1;
  p->s_base = l->state_off[(size_t)c.u0]; p->a_base = l->arc_off[(size_t)c.u0]; p->na = c.na;
  p->u0 = c.u0; p->n = c.n;
}
unsigned k2x_grid(int64_t na) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(4096, (na + K2X_NT - 1) / K2X_NT)); }
// the statuses of a rescored / boosted handle: KHG_LAT_NO_REF where dropped, KHG_LAT_NO_PATH for an empty input
void k2x_status(const khg_lattices* in, const std::vector<char>& drop, khg_lattices* res) {
  res->op_status.resize((size_t)in->U);
  for (int u = 0; u < in->U; ++u)
    res->op_status[(size_t)u] = in->state_off[(size_t)u + 1] == in->state_off[(size_t)u] ? KHG_LAT_NO_PATH : drop[(size_t)u] ? KHG_LAT_NO_REF : KHG_LAT_SUCCEEDED;
}
}  // namespace

extern "C" int khg_lattices_op_status(const khg_lattices* l, int32_t* status_h) {
  if (!l || !status_h) return khg_set_error(KHG_E_ARG, "khg_lattices_op_status: bad arguments");
  if ((int)l->op_status.size() != l->U) return khg_set_error(KHG_E_ARG, "khg_lattices_op_status: the handle was not made by khg_lattices_rescore, khg_lattices_boost or khg_lattices_lm_rescore");
  std::copy(l->op_status.begin(), l->op_status.end(), status_h);
  return KHG_OK;
}

extern "C" int khg_lattices_rescore(khg_ctx* ctx, const khg_model* m, const khg_tm* tm, khg_utts* u, const khg_lattices* lc, float acoustic_scale,
                                    int mode, khg_rescore_stats* stats, khg_lattices** out) {
  const std::string name = "khg_lattices_rescore", who = name + ": ";      // (helpers take the name, the texts written here the prefix)
  if (ctx_dead(ctx) || !m || !tm || !u || !lc || !out) return khg_set_error(KHG_E_ARG, who + "bad arguments");
  *out = nullptr;
  { int rf = utts_foreign_ctx(ctx, u, name.c_str()); if (rf) return rf; }
  if (m->ctx != ctx || tm->ctx != ctx || u->ctx != ctx || lc->ctx != ctx) return other_ctx(name);
  if (mode != KHG_RESCORE_CELLS && mode != KHG_RESCORE_FROM_LL) return khg_set_error(KHG_E_ARG, who + "unknown mode " + std::to_string(mode));
  if (!std::isfinite(acoustic_scale)) return khg_set_error(KHG_E_ARG, who + "acoustic_scale must be finite");
  khg_lattices* l = const_cast<khg_lattices*>(lc);
  const int U = l->U;
  if (U != u->n_utt) return khg_set_error(KHG_E_ARG, who + "the lattices hold " + std::to_string(U) + " utterances, the set " + std::to_string(u->n_utt));
  if (m->D != u->D) return khg_set_error(KHG_E_ARG, who + "model / feature dimensions do not match");
  if (tm->max_pdf >= m->P) return khg_set_error(KHG_E_ARG, who + "transition model refers to pdf-ids the model does not have");
  if (mode == KHG_RESCORE_FROM_LL) {
    if (!u->ll_valid) return khg_set_error(KHG_E_ARG, who + "KHG_RESCORE_FROM_LL needs resident scores: call khg_loglikes first");
    if (u->ll_mode == 2) return khg_set_error(KHG_E_ARG, who + "the scores come from khg_loglikes_band; call khg_loglikes (every cell) first");
  }
  const int64_t NA = l->arc_off[(size_t)U];
  if (NA >= (int64_t)INT_MAX || u->N >= (int64_t)INT_MAX) return khg_set_error(KHG_E_UNSUPPORTED, who + "2^31 - 1 or more arcs or frames");
  int rc = lat_ready(ctx, l);
  if (rc) return rc;
  for (int i = 0; i < U; ++i) {
    if (l->state_off[(size_t)i + 1] == l->state_off[(size_t)i]) continue;
    const int64_t tl = l->ali_off[(size_t)i + 1] - l->ali_off[(size_t)i], ts = u->frame_off[(size_t)i + 1] - u->frame_off[(size_t)i];
    if (tl != ts)
      return khg_set_error(KHG_E_ARG, who + "utterance " + std::to_string(i) + ": the lattice spans " + std::to_string(tl) + " frames, the set has " + std::to_string(ts));
  }
  if (stats) { stats->arcs = NA; stats->emitting_arcs = 0; stats->cells = 0; }
  std::vector<char> drop((size_t)U, 0);
  LatPtr res;
  DevBlocks dv;
  if (mode == KHG_RESCORE_FROM_LL && NA > 0) {
    if ((rc = wait_ali(ctx, u))) return rc;
    int32_t* flag_d;
    if ((rc = dv.zeroed(ctx, U, &flag_d))) return rc;
    K2xLl p{};
    p.set_frame_off = u->frame_off_d; p.pdf_off = u->pdf_off_d; p.ll_off = u->ll_off_d; p.pdfs = u->pdfs_d; p.ll = u->ll_d;
    p.id2pdf = tm->id2pdf_d; p.num_tids = tm->num_tids; p.scale = acoustic_scale; p.flag = flag_d; p.err_flag = ctx->err_flag_d;
    {
      KernelTimer kt(ctx, "k2x_ll_check");
      for (const LatChunk& c : l->chunks) {
        if (c.na == 0) continue;
        k2x_chunk(l, c, &p.c);
        KHG_LAUNCH(ctx, k2x_ll<false>, dim3(k2x_grid(c.na)), dim3(K2X_NT), 0, ctx->stream, p);
        HIPCHK(hipGetLastError());
      }
    }
    std::vector<int32_t> flag;
    if ((rc = download(ctx, flag_d, U, &flag)) || (rc = check_err_flag(ctx, name.c_str()))) return rc;      // synchronises
    for (int i = 0; i < U; ++i) drop[(size_t)i] = flag[(size_t)i] != 0;
    if ((rc = lat_clone(ctx, l, drop, &res)) || (rc = lat_meta(ctx, res.get()))) return rc;
    KernelTimer kt(ctx, "k2x_ll_gather");
    for (const LatChunk& c : res->chunks) {
      if (c.na == 0) continue;
      k2x_chunk(res.get(), c, &p.c);
      KHG_LAUNCH(ctx, k2x_ll<true>, dim3(k2x_grid(c.na)), dim3(K2X_NT), 0, ctx->stream, p);
      HIPCHK(hipGetLastError());
    }
  } else {
    if ((rc = lat_clone(ctx, l, drop, &res))) return rc;
  }
  int64_t st[4] = {NA, 0, 0, 0};
  std::vector<int64_t> base;
  std::vector<float*> acp;
  if (mode == KHG_RESCORE_CELLS && NA > 0) {
    if ((rc = lat_meta(ctx, res.get())) || (rc = k1_cells_scratch(u, NA, m->P)) || (rc = arena_flush(ctx))) return rc;
    K2xFlat f{};
    f.set_frame_off = u->frame_off_d; f.id2pdf = tm->id2pdf_d; f.num_tids = tm->num_tids; f.P = m->P;
    f.keys = u->rc_keys_d; f.vals = u->rc_vals_d; f.err_flag = ctx->err_flag_d;
    {
      KernelTimer kt(ctx, "k2x_flatten");
      for (const LatChunk& c : res->chunks) {
        if (c.na == 0) continue;
        k2x_chunk(res.get(), c, &f.c);
        KHG_LAUNCH(ctx, k2x_flatten, dim3(k2x_grid(c.na)), dim3(K2X_NT), 0, ctx->stream, f);
        HIPCHK(hipGetLastError());
      }
    }
    for (const LatChunk& c : res->chunks) {
      base.push_back(res->arc_off[(size_t)c.u0]);
      acp.push_back(reinterpret_cast<float*>(c.buf + c.ar[3]));
    }
    base.push_back(NA);
    K1cTargets tg;
    int64_t* base_d; float** acp_d;
    if ((rc = dv.upload(ctx, base, &base_d)) || (rc = dv.upload(ctx, acp, &acp_d))) return rc;
    tg.base = base_d; tg.ac = acp_d; tg.n = (int32_t)acp.size();
    if ((rc = k1_cells_run(ctx, m, u, NA, acoustic_scale, tg, st))) return rc;
  }
  if ((rc = check_err_flag(ctx, "khg_lattices_rescore"))) return rc;      // synchronises: the scratch goes with `dv`
  if (stats) { stats->arcs = NA; stats->emitting_arcs = st[1]; stats->cells = st[2]; }
  k2x_status(l, drop, res.get());
  *out = res.release();
  return KHG_OK;
}

namespace {
// The reference of khg_lattices_boost and khg_lattices_mpe_posteriors: per utterance an alignment of transition-ids, from host arrays or
// resident in an utterance set, and the table 2 * class + (silence) per transition-id.  `drop` marks the utterances without a usable
// one: no alignment, one whose length is not the lattice's frame count, an id outside 1 .. num_tids.
struct LatRef {
  DevBlocks dv;
  const int32_t* ali_d = nullptr; const int64_t* aoff_d = nullptr;
  int32_t* tab_d = nullptr;
  std::vector<int32_t> tab;
  std::vector<char> drop;
};
// the host-only checks: every refusal is KHG_E_ARG before any launch.  cls_h[t] is the class of transition-id t (boost, MPFE: its phone)
int lat_ref_check(const std::string& name, khg_ctx* ctx, const khg_lattices* l, int32_t num_tids, const int32_t* cls_h, const int32_t* tid2phone_h, int32_t n_sil,
                  const int32_t* silence_phones_h, const int64_t* ali_off_h, const int32_t* ali_h, const khg_utts* ali_set, LatRef* r) {
  const std::string who = name + ": ";
  const bool host_ali = ali_off_h && ali_h;
  if ((ali_off_h != nullptr) != (ali_h != nullptr) || host_ali == (ali_set != nullptr))
    return khg_set_error(KHG_E_ARG, who + "give either the host alignment (ali_off_h and ali_h) or ali_set, not both and not neither");
  const int U = l->U;
  khg_utts* as = const_cast<khg_utts*>(ali_set);
  if (as) {
    { int rf = utts_foreign_ctx(ctx, as, name.c_str()); if (rf) return rf; }
    if (as->ctx != ctx) return other_ctx(name);
    if (as->n_utt != U) return khg_set_error(KHG_E_ARG, who + "the lattices hold " + std::to_string(U) + " utterances, ali_set " + std::to_string(as->n_utt));
    if (!as->ali_valid) return khg_set_error(KHG_E_ARG, who + "ali_set has no resident alignment: call khg_align (or khg_ali_upload) first");
  } else {
    int rc = check_offsets(name, "ali_off_h", ali_off_h, U, "utterance");
    if (rc) return rc;
  }
  // the class map and the silence set as one table: 2 * class + (silence)
  r->tab.assign((size_t)num_tids + 1, 0);
  for (int t = 1; t <= num_tids; ++t) {
    if (tid2phone_h[t] < 0 || tid2phone_h[t] > INT32_MAX / 2) return khg_set_error(KHG_E_ARG, who + "tid2phone[" + std::to_string(t) + "] out of range");
    if (cls_h[t] < 0 || cls_h[t] > INT32_MAX / 2) return khg_set_error(KHG_E_ARG, who + "tid2pdf[" + std::to_string(t) + "] out of range");
    r->tab[(size_t)t] = 2 * cls_h[t];
  }
  for (int k = 0; k < n_sil; ++k) {
    bool seen = false;
    for (int t = 1; t <= num_tids; ++t)
      if (tid2phone_h[t] == silence_phones_h[k]) { r->tab[(size_t)t] |= 1; seen = true; }
    if (!seen) return khg_set_error(KHG_E_ARG, who + "silence phone " + std::to_string(silence_phones_h[k]) + " is the phone of no transition-id");
  }
  r->drop.assign((size_t)U, 0);
  return KHG_OK;
}
// the device half (U > 0, after lat_meta): the table and the alignment on the device, the ids and the lattices' labels checked there
int lat_ref_device(const std::string& name, khg_ctx* ctx, khg_lattices* l, int32_t num_tids, const int64_t* ali_off_h, const int32_t* ali_h, const khg_utts* ali_set,
                   LatRef* r) {
  const int U = l->U;
  khg_utts* as = const_cast<khg_utts*>(ali_set);
  int rc = as ? wait_ali(ctx, as) : KHG_OK;
  if (rc) return rc;
  int32_t* flag_d;
  if ((rc = r->dv.zeroed(ctx, U + 1, &flag_d)) || (rc = r->dv.upload(ctx, r->tab, &r->tab_d))) return rc;      // [U]: the label word
  // what the host knows: the alignment's length against the lattice's frame count (and, of a host alignment, its ids)
  for (int i = 0; i < U; ++i) {
    const int64_t tl = l->ali_off[(size_t)i + 1] - l->ali_off[(size_t)i];
    const int64_t ta = as ? as->frame_off[(size_t)i + 1] - as->frame_off[(size_t)i] : ali_off_h[i + 1] - ali_off_h[i];
    if (ta == 0 || ta != tl) r->drop[(size_t)i] = 1;
    if (!as && !r->drop[(size_t)i])
      for (int64_t k = ali_off_h[i]; k < ali_off_h[i + 1]; ++k)
        if (ali_h[k] < 1 || ali_h[k] > num_tids) { r->drop[(size_t)i] = 1; break; }
  }
  if (as) {
    r->ali_d = as->ali_d; r->aoff_d = as->frame_off_d;
    if ((rc = launch(ctx, "k2x_ali_check", k2x_ali_check, dim3((unsigned)U), dim3(K2X_NT), 0, r->ali_d, r->aoff_d, num_tids, flag_d))) return rc;
  } else {
    int32_t* a_d; int64_t* o_d;
    if ((rc = r->dv.upload(ctx, ali_h, ali_off_h[U], &a_d)) || (rc = r->dv.upload(ctx, ali_off_h, U + 1, &o_d))) return rc;
    r->ali_d = a_d; r->aoff_d = o_d;
  }
  {
    KernelTimer kt(ctx, "k2x_label_check");
    for (const LatChunk& c : l->chunks) {
      if (c.na == 0) continue;
      K2xChunk kc;
      k2x_chunk(l, c, &kc);
      KHG_LAUNCH(ctx, k2x_label_check, dim3(k2x_grid(c.na)), dim3(K2X_NT), 0, ctx->stream, kc, num_tids, flag_d + U);
      HIPCHK(hipGetLastError());
    }
  }
  std::vector<int32_t> flag;
  if ((rc = download(ctx, flag_d, U + 1, &flag)) || (rc = check_err_flag(ctx, name.c_str()))) return rc;      // synchronises (the caller's arrays are free again)
  if (flag[(size_t)U]) return khg_set_error(KHG_E_ARG, name + ": a lattice arc carries an ilabel outside 0 .. num_tids = " + std::to_string(num_tids));
  for (int i = 0; i < U; ++i) r->drop[(size_t)i] = r->drop[(size_t)i] || flag[(size_t)i] != 0;
  return KHG_OK;
}
}  // namespace

extern "C" int khg_lattices_boost(khg_ctx* ctx, const khg_lattices* lc, int32_t num_tids, const int32_t* tid2phone_h, int32_t n_sil,
                                  const int32_t* silence_phones_h, const int64_t* ali_off_h, const int32_t* ali_h, const khg_utts* ali_set, float b,
                                  float max_silence_error, int32_t* status_h, khg_lattices** out) {
  const std::string name = "khg_lattices_boost", who = name + ": ";
  if (ctx_dead(ctx) || !lc || !out || num_tids < 0 || !tid2phone_h || n_sil < 0 || (n_sil > 0 && !silence_phones_h))
    return khg_set_error(KHG_E_ARG, who + "bad arguments");
  *out = nullptr;
  if (lc->ctx != ctx) return other_ctx(name);
  if (!std::isfinite(b) || !std::isfinite(max_silence_error)) return khg_set_error(KHG_E_ARG, who + "b and max_silence_error must be finite");
  khg_lattices* l = const_cast<khg_lattices*>(lc);
  const int U = l->U;
  LatRef ref;
  int rc = lat_ref_check(name, ctx, l, num_tids, tid2phone_h, tid2phone_h, n_sil, silence_phones_h, ali_off_h, ali_h, ali_set, &ref);
  if (rc) return rc;
  LatPtr res;
  if (U == 0) {
    if ((rc = lat_clone(ctx, l, ref.drop, &res))) return rc;
    *out = res.release();
    return KHG_OK;
  }
  if ((rc = lat_ready(ctx, l)) || (rc = lat_ref_device(name, ctx, l, num_tids, ali_off_h, ali_h, ali_set, &ref)) ||
      (rc = lat_clone(ctx, l, ref.drop, &res)) || (rc = lat_meta(ctx, res.get())))
    return rc;
  K2xBoost p{};
  p.ali = ref.ali_d; p.ali_off = ref.aoff_d; p.tab = ref.tab_d; p.neg_b = -b; p.max_sil_err = max_silence_error;
  {
    KernelTimer kt(ctx, "k2x_boost");
    for (const LatChunk& c : res->chunks) {
      if (c.na == 0) continue;
      k2x_chunk(res.get(), c, &p.c);
      KHG_LAUNCH(ctx, k2x_boost, dim3(k2x_grid(c.na)), dim3(K2X_NT), 0, ctx->stream, p);
      HIPCHK(hipGetLastError());
    }
  }
  if ((rc = check_err_flag(ctx, "khg_lattices_boost"))) return rc;      // synchronises: the scratch goes with `ref`
  k2x_status(l, ref.drop, res.get());
  if (status_h) std::copy(res->op_status.begin(), res->op_status.end(), status_h);
  *out = res.release();
  return KHG_OK;
}

// ------------------------------------------------------------------------------------------
// K2M: MPE / sMBR posteriors (khg_k2_lattice_mpe.hip.inc): khg_lattices_posteriors' chunk steps around k2_lattice_post_mpe
// in k2_lattice_post_fb's place; the handle's arc_post and weights are the signed values.
extern "C" int khg_lattices_mpe_posteriors(khg_ctx* ctx, const khg_lattices* lc, int32_t num_tids, const int32_t* tid2phone_h, const int32_t* tid2pdf_h,
                                           int32_t n_sil, const int32_t* silence_phones_h, const int64_t* ali_off_h, const int32_t* ali_h,
                                           const khg_utts* ali_set, int32_t criterion, int32_t one_silence_class, float graph_scale, float acoustic_scale,
                                           int32_t* status_h, double* tot_like_h, double* avg_acc_h, khg_posteriors** out) {
  const std::string name = "khg_lattices_mpe_posteriors", who = name + ": ";
  if (ctx_dead(ctx) || !lc || !out || num_tids < 0 || !tid2phone_h || n_sil < 0 || (n_sil > 0 && !silence_phones_h))
    return khg_set_error(KHG_E_ARG, who + "bad arguments");
  *out = nullptr;
  if (lc->ctx != ctx) return other_ctx(name);
  if (criterion != KHG_MPE_MPFE && criterion != KHG_MPE_SMBR) return khg_set_error(KHG_E_ARG, who + "unknown criterion " + std::to_string(criterion));
  if (criterion == KHG_MPE_SMBR && !tid2pdf_h) return khg_set_error(KHG_E_ARG, who + "KHG_MPE_SMBR needs tid2pdf_h");
  if (bad_scale(graph_scale) || bad_scale(acoustic_scale)) return khg_set_error(KHG_E_ARG, who + "graph_scale and acoustic_scale must be finite and >= 0");
  PostRun r;
  r.ctx = ctx; r.l = const_cast<khg_lattices*>(lc); r.who = "khg_lattices_mpe_posteriors";
  r.gs = (double)graph_scale; r.as = (double)acoustic_scale;
  khg_lattices* l = r.l;
  const int U = l->U;
  LatRef ref;
  int rc = lat_ref_check(name, ctx, l, num_tids, criterion == KHG_MPE_SMBR ? tid2pdf_h : tid2phone_h, tid2phone_h, n_sil, silence_phones_h, ali_off_h, ali_h,
                         ali_set, &ref);
  if (rc) return rc;
  new_posteriors(ctx, U, &r.res);
  r.res->arc_off = l->arc_off;
  if (U == 0) { *out = r.res.release(); return KHG_OK; }
  // (the in-arc index after the reference's checks: the order of the launches)
  if ((rc = lat_ready(ctx, l)) || (rc = lat_ref_device(name, ctx, l, num_tids, ali_off_h, ali_h, ali_set, &ref)) || (rc = lat_index(ctx, l)) ||
      (rc = post_run_begin(r)))
    return rc;
  int32_t* no_ref_d; double* avg_d;
  const std::vector<int32_t> no_ref(ref.drop.begin(), ref.drop.end());
  if ((rc = r.dv.alloc(U, &avg_d)) || (rc = r.dv.upload(ctx, no_ref, &no_ref_d))) return rc;
  for (size_t k = 0; k < l->chunks.size(); ++k) {
    const LatChunk& c = l->chunks[k];
    PoMpeArgs q{};
    if ((rc = post_chunk_begin(r, k, 40, &q.po))) return rc;       // alpha, beta, the Jacobi row, A and B (doubles) beside the staged lattice
    q.ref = ref.ali_d; q.ref_off = ref.aoff_d; q.tab = ref.tab_d; q.no_ref = no_ref_d; q.avg = avg_d; q.one_silence_class = one_silence_class != 0;
    const int64_t cells = std::max<int64_t>(c.ns, 1);
    if ((rc = r.dv.alloc(cells, &q.accA)) || (rc = r.dv.alloc(cells, &q.accB)) ||
        (rc = launch(ctx, "k2_lattice_post_mpe", k2_lattice_post_mpe, dim3((unsigned)c.n), dim3(PO_NT), (size_t)q.po.lo.lds_bytes, q)) ||
        (rc = post_chunk_finish(r, k, &q.po)))       // the fill sums arc_post: here the signed values
      return rc;
  }
  return post_run_finish(r, status_h, tot_like_h, avg_d, avg_acc_h, out);       // synchronises: the scratch goes with `r` and `ref`
}

// ------------------------------------------------------------------------------------------
// K2N: the backoff n-gram LM and lattice-lmrescore (khg_k2_lattice_lm.hip.inc)
struct khg_lm {
  khg_ctx* ctx = nullptr;
  int32_t n_states = 0, start = 0;
  int64_t n_arcs = 0, bytes = 0;
  unsigned char* buf = nullptr;       // backoff | backoff_cost | final_cost | arc_begin | word | cost | next, each at a multiple of 256 bytes
  LmDev dev;
};

extern "C" int khg_lm_validate(int32_t n_states, const int32_t* backoff, const float* backoff_cost, const int32_t* arc_begin, const int32_t* word,
                               const float* cost, const int32_t* next, const float* final_cost, int32_t start) {
  const std::string who = "khg_lm_validate: ";
  if (n_states < 1 || !backoff || !backoff_cost || !arc_begin || !final_cost) return khg_set_error(KHG_E_ARG, who + "bad arguments (at least the empty history, no NULL array)");
  if (arc_begin[0] != 0) return khg_set_error(KHG_E_ARG, who + "arc_begin must start at 0");
  for (int32_t h = 0; h < n_states; ++h)
    if (arc_begin[h + 1] < arc_begin[h]) return khg_set_error(KHG_E_ARG, who + "arc_begin not monotone at state " + std::to_string(h));
  if (arc_begin[n_states] > 0 && (!word || !cost || !next)) return khg_set_error(KHG_E_ARG, who + "bad arguments (an arc array is NULL)");
  if (start < 0 || start >= n_states) return khg_set_error(KHG_E_ARG, who + "start out of range");
  if (backoff[0] != -1) return khg_set_error(KHG_E_ARG, who + "backoff[0] must be -1 (the empty history backs off to nothing)");
  for (int32_t h = 0; h < n_states; ++h) {
    const std::string at = "state " + std::to_string(h) + ": ";
    if (h > 0 && (backoff[h] < 0 || backoff[h] >= h)) return khg_set_error(KHG_E_ARG, who + at + "backoff must name a lower state");
    if (!std::isfinite(backoff_cost[h])) return khg_set_error(KHG_E_ARG, who + at + "backoff_cost is not finite");
    if (!std::isfinite(final_cost[h])) return khg_set_error(KHG_E_ARG, who + at + "final_cost is not finite");
    for (int32_t a = arc_begin[h]; a < arc_begin[h + 1]; ++a) {
      const std::string arc = at + "arc " + std::to_string(a) + ": ";
      if (word[a] <= 0) return khg_set_error(KHG_E_ARG, who + arc + "word must be > 0");
      if (a > arc_begin[h] && word[a] <= word[a - 1]) return khg_set_error(KHG_E_ARG, who + arc + "words must ascend strictly inside a state");
      if (!std::isfinite(cost[a])) return khg_set_error(KHG_E_ARG, who + arc + "cost is not finite");
      if (next[a] < 0 || next[a] >= n_states) return khg_set_error(KHG_E_ARG, who + arc + "next out of range");
    }
  }
  return KHG_OK;
}

extern "C" int khg_lm_score(int32_t n_states, const int32_t* backoff, const float* backoff_cost, const int32_t* arc_begin, const int32_t* word,
                            const float* cost, const int32_t* next, const float* final_cost, int32_t start, int32_t n_words, const int32_t* words,
                            float* cost_out) {
  int rc = khg_lm_validate(n_states, backoff, backoff_cost, arc_begin, word, cost, next, final_cost, start);
  if (rc) return rc;
  if (n_words < 0 || (n_words > 0 && !words) || !cost_out) return khg_set_error(KHG_E_ARG, "khg_lm_score: bad arguments");
  int32_t h = start;
  volatile float total = 0.0f;       // (volatile: every sum is rounded to float where it is written)
  for (int32_t i = 0; i < n_words; ++i) {
    const int32_t w = words[i];
    if (w <= 0) return khg_set_error(KHG_E_ARG, "khg_lm_score: word " + std::to_string(i) + " is not > 0");
    volatile float c = 0.0f;
    for (;;) {
      const int32_t* lo = std::lower_bound(word + arc_begin[h], word + arc_begin[h + 1], w);
      if (lo != word + arc_begin[h + 1] && *lo == w) { c = c + cost[lo - word]; h = next[lo - word]; break; }
      if (h == 0) return khg_set_error(KHG_E_ARG, "khg_lm_score: word " + std::to_string(i) + " (" + std::to_string(w) + ") is out of vocabulary");
      c = c + backoff_cost[h];
      h = backoff[h];
    }
    total = total + c;
  }
  total = total + final_cost[h];
  *cost_out = total;
  return KHG_OK;
}

extern "C" int khg_lm_destroy(khg_lm* lm) {
  if (!lm) return KHG_OK;
  if (lm->buf) (void)hipFree(lm->buf);
  delete lm;
  return KHG_OK;
}
extern "C" int khg_lm_num_states(const khg_lm* lm, int32_t* n_states) {
  if (!lm || !n_states) return khg_set_error(KHG_E_ARG, "khg_lm_num_states: bad arguments");
  *n_states = lm->n_states;
  return KHG_OK;
}
extern "C" int khg_lm_device_bytes(const khg_lm* lm, int64_t* bytes) {
  if (!lm || !bytes) return khg_set_error(KHG_E_ARG, "khg_lm_device_bytes: bad arguments");
  *bytes = lm->bytes;
  return KHG_OK;
}

extern "C" int khg_lm_create(khg_ctx* ctx, int32_t n_states, const int32_t* backoff, const float* backoff_cost, const int32_t* arc_begin,
                             const int32_t* word, const float* cost, const int32_t* next, const float* final_cost, int32_t start, khg_lm** out) {
  if (ctx_dead(ctx) || !out) return khg_set_error(KHG_E_ARG, "khg_lm_create: bad arguments");
  *out = nullptr;
  int rc = khg_lm_validate(n_states, backoff, backoff_cost, arc_begin, word, cost, next, final_cost, start);
  if (rc) return rc;
  struct LmFree { void operator()(khg_lm* m) const { (void)khg_lm_destroy(m); } };
  std::unique_ptr<khg_lm, LmFree> lm(new khg_lm);
  lm->ctx = ctx; lm->n_states = n_states; lm->start = start; lm->n_arcs = arc_begin[n_states];
  const int64_t S = n_states, A = lm->n_arcs;
  const int64_t cnt[7] = {S, S, S, S + 1, A, A, A};
  const void* src[7] = {backoff, backoff_cost, final_cost, arc_begin, word, cost, next};
  int64_t o[7], total = 0;
  for (int k = 0; k < 7; ++k) { o[k] = total; total += (4 * cnt[k] + 255) & ~int64_t(255); }
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&lm->buf), (size_t)std::max<int64_t>(total, 16)));
  lm->bytes = total;
  if ((rc = arena_flush(ctx))) return rc;
  for (int k = 0; k < 7; ++k)
    if (cnt[k]) HIPCHK(hipMemcpyAsync(lm->buf + o[k], src[k], 4 * (size_t)cnt[k], hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));        // the host arrays are the caller's again
  auto i = [&](int k) { return reinterpret_cast<const int32_t*>(lm->buf + o[k]); };
  auto f = [&](int k) { return reinterpret_cast<const float*>(lm->buf + o[k]); };
  lm->dev.backoff = i(0); lm->dev.backoff_cost = f(1); lm->dev.fin = f(2); lm->dev.arc_begin = i(3); lm->dev.word = i(4); lm->dev.cost = f(5);
  lm->dev.next = i(6); lm->dev.start = start;
  *out = lm.release();
  return KHG_OK;
}

extern "C" int khg_lattices_lm_rescore(khg_ctx* ctx, const khg_lattices* lc, const khg_lm* lm, float scale, int32_t hist_factor, int32_t* status_h,
                                       khg_lm_rescore_stats* stats, khg_lattices** out) {
  const std::string name = "khg_lattices_lm_rescore", who = name + ": ";
  if (ctx_dead(ctx) || !lc || !lm || !out) return khg_set_error(KHG_E_ARG, who + "bad arguments");
  *out = nullptr;
  if (lc->ctx != ctx || lm->ctx != ctx) return other_ctx(name);
  if (!std::isfinite(scale)) return khg_set_error(KHG_E_ARG, who + "scale must be finite");
  if (hist_factor < 1) return khg_set_error(KHG_E_ARG, who + "hist_factor must be >= 1");
  khg_lattices* l = const_cast<khg_lattices*>(lc);
  const int U = l->U;
  LatPtr res;
  int rc = new_lattices(ctx, U, &res);
  if (rc) return rc;
  if (stats) *stats = khg_lm_rescore_stats{0, 0, 0, 0, 0};
  if (U == 0) { *out = res.release(); return KHG_OK; }
  if ((rc = lat_ready(ctx, l, kWithIndex))) return rc;
  DevBlocks dv;
  int32_t *status_d, *maxh_d;
  if ((rc = dv.alloc(U, &status_d)) || (rc = dv.alloc(U, &maxh_d))) return rc;
  for (size_t k = 0; k < l->chunks.size(); ++k) {
    const LatChunk& c = l->chunks[k];
    LmArgs p{};
    lat_chunk_args(l, c, &p.lo);
    p.lo.status = status_d; p.lo.o_start = res->start_d;
    p.lm = lm->dev; p.scale = scale; p.hist_factor = hist_factor; p.max_hist = maxh_d;
    const LatIndex ix = lat_index_arrays(l->idx_d[k], c);
    p.in_begin = ix.in_begin; p.in_arc = ix.in_arc; p.arc_src = ix.arc_src;
    const int64_t cells = std::max<int64_t>(c.ns, 1);
    if ((rc = dv.alloc((int64_t)hist_factor * cells, &p.arena)) || (rc = dv.alloc((int64_t)hist_factor * cells, &p.tmp)) ||
        (rc = dv.alloc(cells + c.n, &p.set_off)) || (rc = dv.alloc(cells, &p.arc_base)) || (rc = dv.alloc(2 * (int64_t)c.n, &p.lo.utt_tot)) ||
        (rc = dv.alloc(2 * ((int64_t)c.n + 1), &p.lo.utt_off)))
      return rc;
    LatChunk ch;
    if ((rc = launch(ctx, "k2_lattice_lm_mark", k2_lattice_lm_mark, dim3((unsigned)c.n), dim3(LM_NT), 0, p)) ||
        (rc = size_out_chunk(ctx, name, "k2_lattice_lm_scan", p.lo.utt_tot, p.lo.utt_off, c.u0, c.n, res.get(), &ch)))      // the one synchronisation that sizes the output
      return rc;
    lat_chunk_arrays(ch, &p.lo.out);
    if ((rc = launch(ctx, "k2_lattice_lm_fill", k2_lattice_lm_fill, dim3((unsigned)c.n, stripes(chunk_max(res->state_off, c), LM_NT, c.n)), dim3(LM_NT), 0, p)))
      return rc;
  }
  std::vector<int32_t> st, mh;
  if ((rc = download(ctx, status_d, U, &st)) || (rc = download(ctx, maxh_d, U, &mh)) || (rc = check_err_flag(ctx, name.c_str()))) return rc;     // synchronises: the scratch goes with `dv`
  res->op_status = st;
  if (status_h) std::copy(st.begin(), st.end(), status_h);
  if (stats) {
    stats->in_states = l->state_off[(size_t)U]; stats->in_arcs = l->arc_off[(size_t)U];
    stats->out_states = res->state_off[(size_t)U]; stats->out_arcs = res->arc_off[(size_t)U];
    for (int32_t m : mh) stats->max_hist = std::max<int64_t>(stats->max_hist, m);
  }
  *out = res.release();
  return KHG_OK;
}

// ------------------------------------------------------------------------------------------
// K2D: lattice-determinize-pruned (khg_k2_lattice_det.hip.inc): prune, split every state by the determinized states that
// hold it, prune again
extern "C" int khg_lattices_determinize(khg_ctx* ctx, const khg_lattices* lc, float graph_scale, float acoustic_scale, float beam, float delta,
                                        int32_t state_factor, int32_t* status_h, khg_det_stats* stats, khg_lattices** out) {
  const std::string name = "khg_lattices_determinize", who = name + ": ";
  if (ctx_dead(ctx) || !lc || !out) return khg_set_error(KHG_E_ARG, who + "bad arguments");
  *out = nullptr;
  if (lc->ctx != ctx) return other_ctx(name);
  if (bad_scale(graph_scale) || bad_scale(acoustic_scale)) return khg_set_error(KHG_E_ARG, who + "graph_scale and acoustic_scale must be finite and >= 0");
  if (!std::isfinite(beam) || beam < 0.0f) return khg_set_error(KHG_E_ARG, who + "beam must be finite and >= 0");
  if (!std::isfinite(delta) || delta < 0.0f) return khg_set_error(KHG_E_ARG, who + "delta must be finite and >= 0");
  if (state_factor < 1) return khg_set_error(KHG_E_ARG, who + "state_factor must be >= 1");
  khg_lattices* l = const_cast<khg_lattices*>(lc);
  const int U = l->U;
  if (stats) *stats = khg_det_stats{0, 0, 0, 0, 0, 0, 0, 0};
  if (U == 0) {
    LatPtr res;
    int rc = new_lattices(ctx, U, &res);
    if (rc) return rc;
    *out = res.release();
    return KHG_OK;
  }
  int rc = lat_ready(ctx, l);
  if (rc) return rc;
  DevBlocks dv;
  int32_t *status0_d, *status_d, *det_d, *maxk_d, *maxc_d;
  if ((rc = dv.alloc(U, &status0_d)) || (rc = dv.alloc(U, &status_d)) || (rc = dv.alloc(U, &det_d)) || (rc = dv.alloc(U, &maxk_d)) ||
      (rc = dv.alloc(U, &maxc_d)))
    return rc;
  // what is refused before anything else: an empty lattice, an arc that does not go to a higher state
  for (const LatChunk& c : l->chunks) {
    LoArgs q{};
    lat_chunk_args(l, c, &q);
    if ((rc = launch(ctx, "k2_lattice_det_check", k2_lattice_det_check, dim3((unsigned)c.n), dim3(DT_NT), 0, q, status0_d))) return rc;
  }
  std::vector<int32_t> st0, stx((size_t)U, 0);
  if ((rc = download(ctx, status0_d, U, &st0))) return rc;
  // 1. X
  khg_lattices* xp = nullptr;
  if ((rc = khg_lattices_prune(ctx, l, graph_scale, acoustic_scale, beam, stx.data(), &xp))) return rc;       // synchronises: st0 is there
  LatPtr X(xp);
  for (int u = 0; u < U; ++u)
    if (st0[(size_t)u] == 0 && stx[(size_t)u] != KHG_LAT_SUCCEEDED) st0[(size_t)u] = stx[(size_t)u];
  HIPCHK(hipMemcpyAsync(status0_d, st0.data(), 4 * (size_t)U, hipMemcpyHostToDevice, ctx->stream));
  // 2. to 5. Y
  LatPtr Y;
  if ((rc = new_lattices(ctx, U, &Y)) || (rc = lat_ready(ctx, X.get(), kWithIndex))) return rc;
  for (size_t k = 0; k < X->chunks.size(); ++k) {
    const LatChunk& c = X->chunks[k];
    DtArgs p{};
    lat_chunk_args(X.get(), c, &p.lo);
    p.lo.status = status_d; p.lo.o_start = Y->start_d;
    p.status0 = status0_d; p.gs = graph_scale; p.as = acoustic_scale; p.delta = delta; p.factor = state_factor;
    p.det_states = det_d; p.max_subset = maxk_d; p.max_closure = maxc_d;
    const LatIndex ix = lat_index_arrays(X->idx_d[k], c);
    p.in_begin = ix.in_begin; p.in_arc = ix.in_arc; p.arc_src = ix.arc_src;
    p.e_stride = (int64_t)state_factor * c.ns + c.n; p.s_stride = std::max<int64_t>(c.ns, 1); p.a_stride = std::max<int64_t>(c.na, 1);
    if ((rc = dv.alloc(DT_PER_E * p.e_stride, &p.per_e)) || (rc = dv.alloc(DT_PER_S * p.s_stride, &p.per_s)) ||
        (rc = dv.alloc(DT_PER_A * p.a_stride, &p.per_a)) || (rc = dv.alloc(std::max<int64_t>((int64_t)state_factor * c.na, 1), &p.slot)) ||
        (rc = dv.alloc(2 * (int64_t)c.n, &p.lo.utt_tot)) || (rc = dv.alloc(2 * ((int64_t)c.n + 1), &p.lo.utt_off)))
      return rc;
    LatChunk ch;
    if ((rc = launch(ctx, "k2_lattice_det_mark", k2_lattice_det_mark, dim3((unsigned)c.n), dim3(DT_NT), 0, p)) ||
        (rc = size_out_chunk(ctx, name, "k2_lattice_det_scan", p.lo.utt_tot, p.lo.utt_off, c.u0, c.n, Y.get(), &ch)))      // the one synchronisation that sizes Y
      return rc;
    lat_chunk_arrays(ch, &p.lo.out);
    if ((rc = launch(ctx, "k2_lattice_det_fill", k2_lattice_det_fill, dim3((unsigned)c.n, stripes(chunk_max(Y->state_off, c), DT_NT, c.n)), dim3(DT_NT), 0, p)))
      return rc;
  }
  std::vector<int32_t> st, nd, mk, mc;
  if ((rc = download(ctx, status_d, U, &st)) || (rc = download(ctx, det_d, U, &nd)) || (rc = download(ctx, maxk_d, U, &mk)) ||
      (rc = download(ctx, maxc_d, U, &mc)) || (rc = check_err_flag(ctx, name.c_str())))       // synchronises: the scratch goes with `dv`
    return rc;
  // 6. the result
  khg_lattices* rp = nullptr;
  if ((rc = khg_lattices_prune(ctx, Y.get(), graph_scale, acoustic_scale, beam, stx.data(), &rp))) return rc;
  LatPtr res(rp);
  for (int u = 0; u < U; ++u)
    if (st[(size_t)u] == KHG_LAT_SUCCEEDED) st[(size_t)u] = stx[(size_t)u];
  res->op_status = st;
  if (status_h) std::copy(st.begin(), st.end(), status_h);
  if (stats) {
    stats->in_states = l->state_off[(size_t)U]; stats->in_arcs = l->arc_off[(size_t)U];
    stats->out_states = res->state_off[(size_t)U]; stats->out_arcs = res->arc_off[(size_t)U];
    for (int u = 0; u < U; ++u) {
      if (st0[(size_t)u] == 0) stats->pruned_states += X->state_off[(size_t)u + 1] - X->state_off[(size_t)u];
      if (st[(size_t)u] != KHG_LAT_SUCCEEDED) continue;
      stats->det_states += nd[(size_t)u];
      stats->max_subset = std::max<int64_t>(stats->max_subset, mk[(size_t)u]);
      stats->max_closure = std::max<int64_t>(stats->max_closure, mc[(size_t)u]);
    }
  }
  *out = res.release();
  return KHG_OK;
}

// ------------------------------------------------------------------------------------------
// K2W: scoring (khg_k2_lattice_score.hip.inc): the word insertion penalty, the oracle path, the sweep of score.sh
namespace {
const int64_t kScoreScratch = int64_t(1) << 30;       // khg_lattices_oracle's tables per launch when the caller names no size
const int64_t kNbestArena = int64_t(1) << 30;        // khg_lattices_nbest: the lists of one launch's utterances (24 bytes per element) unless KHG_OPT_NBEST_ARENA names a size
const int64_t kScoreWerLds = 48 << 10;                // khg_lattices_wer: a (triple, utterance) table stays in LDS up to this many bytes

// the most dynamic LDS a workgroup of the current device may ask for: all 160 KiB of a gfx950 CU
int score_lds_cap(int64_t* cap) {
  int dev = 0, v = 0;
  HIPCHK(hipGetDevice(&dev));
  HIPCHK(hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
  *cap = std::min<int64_t>(160 << 10, v);
  return KHG_OK;
}
// the widest frame of every utterance, once per handle (after lat_meta)
int lat_width(khg_ctx* ctx, khg_lattices* l) {
  if (l->width_d || l->U == 0) return KHG_OK;
  const size_t U = (size_t)l->U;
  int32_t* w_d = nullptr;
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&w_d), 4 * U));
  l->width_d = w_d;
  l->bytes += 4 * (int64_t)U;
  for (const LatChunk& c : l->chunks) {
    LoArgs p{};
    lat_chunk_args(l, c, &p);
    KHG_LAUNCH(ctx, k2_lattice_score_width, dim3((unsigned)((c.n + 63) / 64)), dim3(64), 0, ctx->stream, p, w_d);
    HIPCHK(hipGetLastError());
  }
  int rc = download(ctx, w_d, (int64_t)U, &l->width);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return KHG_OK;
}
// the references of a scoring call: n_utt is the handle's, offsets from 0 and monotone, words > 0
int score_ref_check(const std::string& name, const khg_lattices* l, int32_t n_utt, const int32_t* ref_h, const int64_t* ref_off_h) {
  const std::string who = name + ": ";
  if (n_utt != l->U) return khg_set_error(KHG_E_ARG, who + "the lattices hold " + std::to_string(l->U) + " utterances, the references " + std::to_string(n_utt));
  int rc = check_offsets(name, "ref_off_h", ref_off_h, n_utt, "utterance", ref_h, "ref_h");
  if (rc) return rc;
  for (int u = 0; u < n_utt; ++u) {
    for (int64_t i = ref_off_h[u]; i < ref_off_h[u + 1]; ++i)
      if (ref_h[i] <= 0) return khg_set_error(KHG_E_ARG, who + "utterance " + std::to_string(u) + ": a reference word is not > 0");
    if ((l->state_off[(size_t)u + 1] - l->state_off[(size_t)u]) + (ref_off_h[u + 1] - ref_off_h[u]) >= (int64_t(1) << 29))
      return khg_set_error(KHG_E_ARG, who + "utterance " + std::to_string(u) + ": states + reference words reach 2^29");
  }
  return KHG_OK;
}
// the references on the device
int score_ref_upload(khg_ctx* ctx, int U, const int32_t* ref_h, const int64_t* ref_off_h, DevBlocks* dv, int32_t** ref_d, int64_t** ref_off_d) {
  int rc = dv->upload(ctx, ref_h, ref_off_h[U], ref_d);
  return rc ? rc : dv->upload(ctx, ref_off_h, U + 1, ref_off_d);
}
// Utterances whose tables share one scratch block, a launch at a time (khg_lattices_oracle, khg_lattices_mbr): a launch runs the n
// utterances list[first .. first + n) of chunk `chunk`; the table of list[j] starts tab_off[j] cells into the block; the launch's
// tables are `cells` together, the largest launch's max_cells.
struct TableLaunch { size_t chunk, first, n; int64_t cells; };
struct TableLaunches {
  std::vector<int32_t> list;
  std::vector<int64_t> tab_off;
  std::vector<TableLaunch> launches;
  int64_t max_cells = 1;
};
// Chunk by chunk, the utterances that run -- cells_of(u), called once per utterance in order: the cells of u's table, or < 0 when u does
// not run (no path, or a table that alone is over the budget: the caller's status) -- grouped into launches whose tables, cell_bytes
// a cell, fit `budget` bytes together.  (The decoders group scratch SLICES of a whole batch, by bytes and without skipping:
// split_by_budget.)
template <class F>
TableLaunches group_tables(const std::vector<LatChunk>& chunks, int64_t cell_bytes, int64_t budget, F cells_of) {
  TableLaunches g;
  for (size_t k = 0; k < chunks.size(); ++k) {
    const LatChunk& c = chunks[k];
    TableLaunch cur{k, g.list.size(), 0, 0};
    for (int u = c.u0; u < c.u0 + c.n; ++u) {
      const int64_t cells = cells_of(u);
      if (cells < 0) continue;
      if (cur.n > 0 && cell_bytes * (cur.cells + cells) > budget) { g.launches.push_back(cur); cur = TableLaunch{k, g.list.size(), 0, 0}; }
      g.list.push_back(u);
      g.tab_off.push_back(cur.cells);
      cur.cells += cells; ++cur.n;
    }
    if (cur.n > 0) g.launches.push_back(cur);
  }
  for (const TableLaunch& L : g.launches) g.max_cells = std::max(g.max_cells, L.cells);
  return g;
}
}  // namespace

extern "C" int khg_lattices_add_penalty(khg_ctx* ctx, const khg_lattices* lc, float word_ins_penalty, khg_lattices** out) {
  const std::string name = "khg_lattices_add_penalty", who = name + ": ";
  if (ctx_dead(ctx) || !lc || !out) return khg_set_error(KHG_E_ARG, who + "bad arguments");
  *out = nullptr;
  if (lc->ctx != ctx) return other_ctx(name);
  if (!std::isfinite(word_ins_penalty)) return khg_set_error(KHG_E_ARG, who + "word_ins_penalty must be finite");
  int rc = arena_flush(ctx);
  if (rc) return rc;
  LatPtr res;
  if ((rc = lat_clone(ctx, lc, std::vector<char>((size_t)lc->U, 0), &res))) return rc;
  {
    KernelTimer kt(ctx, "k2_lattice_score_add_penalty");
    for (const LatChunk& c : res->chunks) {
      if (c.na == 0) continue;
      KHG_LAUNCH(ctx, k2_lattice_score_add_penalty, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(4096, (c.na + 255) / 256))), dim3(256), 0, ctx->stream,
                 reinterpret_cast<float*>(c.buf + c.ar[2]), reinterpret_cast<const int32_t*>(c.buf + c.ar[1]), c.na, word_ins_penalty);
      HIPCHK(hipGetLastError());
    }
  }
  if ((rc = check_err_flag(ctx, name.c_str()))) return rc;      // synchronises
  *out = res.release();
  return KHG_OK;
}

extern "C" int khg_lattices_oracle(khg_ctx* ctx, const khg_lattices* lc, int32_t n_utt, const int32_t* ref_h, const int64_t* ref_off_h, int64_t scratch_bytes,
                                   int32_t* counts_h, int32_t* words_h, int64_t* words_off_h, int64_t words_cap, int32_t* ali_h, int32_t* status_h) {
  const std::string name = "khg_lattices_oracle", who = name + ": ";
  if (!lc) return khg_set_error(KHG_E_ARG, who + "bad arguments");
  int rc = score_ref_check(name, lc, n_utt, ref_h, ref_off_h);
  if (rc) return rc;
  if (scratch_bytes < 0) return khg_set_error(KHG_E_ARG, who + "scratch_bytes must be >= 0");
  if (ctx_dead(ctx)) return khg_set_error(KHG_E_ARG, who + "bad arguments");
  if (lc->ctx != ctx) return other_ctx(name);
  khg_lattices* l = const_cast<khg_lattices*>(lc);
  const int U = l->U;
  if (words_off_h) std::fill(words_off_h, words_off_h + U + 1, 0);
  if (U == 0) return KHG_OK;
  for (int u = 0; u < U; ++u)
    if (l->arc_off[(size_t)u + 1] - l->arc_off[(size_t)u] > (int64_t)INT32_MAX - 3)
      return khg_set_error(KHG_E_ARG, who + "utterance " + std::to_string(u) + ": more than 2^31 - 4 arcs");
  const int64_t budget = scratch_bytes ? scratch_bytes : kScoreScratch;
  int64_t lds_cap = 0;
  if ((rc = lat_ready(ctx, l, kWithIndex | kWithWidth)) || (rc = score_lds_cap(&lds_cap))) return rc;
  const int64_t AT = l->ali_off[(size_t)U];
  DevBlocks dv;
  int32_t *ref_d, *counts_d, *nw_d, *status_d, *ali_d, *list_d, *tab_d;
  int64_t *ref_off_d, *ali_off_d, *tab_off_d;
  // the utterances whose own table fits the budget, chunk by chunk, grouped into launches whose tables fit it together
  std::vector<char> too_big((size_t)U, 0);
  auto row = [&](int u) -> int64_t { return ref_off_h[u + 1] - ref_off_h[u] + 1; };       // the cells of a table's row: the reference and one
  const TableLaunches g = group_tables(l->chunks, 4, budget, [&](int u) -> int64_t {
    const int64_t N = l->state_off[(size_t)u + 1] - l->state_off[(size_t)u];
    const int64_t cells = 2 * N * row(u);
    if (4 * cells > budget) { too_big[(size_t)u] = 1; return -1; }
    return cells;
  });
  if ((rc = score_ref_upload(ctx, U, ref_h, ref_off_h, &dv, &ref_d, &ref_off_d)) || (rc = dv.alloc(4 * (int64_t)U, &counts_d)) || (rc = dv.alloc(U, &nw_d)) ||
      (rc = dv.zeroed(ctx, std::max<int64_t>(AT, 1), &ali_d)) || (rc = dv.zeroed(ctx, U, &status_d)) || (rc = dv.upload(ctx, l->ali_off, &ali_off_d)) ||
      (rc = dv.upload(ctx, g.list, &list_d)) || (rc = dv.upload(ctx, g.tab_off, &tab_off_d)) || (rc = dv.alloc(g.max_cells, &tab_d)))
    return rc;
  std::vector<int32_t*> words_d(l->chunks.size(), nullptr);
  for (size_t k = 0; k < l->chunks.size(); ++k)
    if ((rc = dv.alloc(std::max<int64_t>(l->chunks[k].ns, 1), &words_d[k]))) return rc;
  for (const TableLaunch& L : g.launches) {
    const LatChunk& c = l->chunks[L.chunk];
    int64_t lds = 0;       // the ring of rows of the launch's utterances in LDS: the largest that fits
    for (size_t j = L.first; j < L.first + L.n; ++j) {
      const int u = g.list[j];
      const int64_t ring = 8 * (int64_t)l->width[(size_t)u] * row(u);
      if (ctx->opt[KHG_OPT_LAT_OPS_LDS] != 1 && ring <= lds_cap) lds = std::max(lds, ring);
    }
    ScArgs p{};
    lat_chunk_args(l, c, &p.lo);
    p.lo.lds_bytes = (int32_t)lds;
    p.lo.status = status_d; p.lo.ali = ali_d; p.lo.ali_off = ali_off_d; p.lo.ali_total = AT; p.lo.words = words_d[L.chunk];
    const LatIndex ix = lat_index_arrays(l->idx_d[L.chunk], c);
    p.in_begin = ix.in_begin; p.in_arc = ix.in_arc; p.arc_src = ix.arc_src;
    p.list = list_d + L.first; p.tab_off = tab_off_d + L.first; p.tab = tab_d; p.width = l->width_d;
    p.ref = ref_d; p.ref_off = ref_off_d; p.counts = counts_d; p.nwords = nw_d;
    if ((rc = khg_lds_attribute((const void*)k2_lattice_score_oracle, (size_t)lds))) return rc;
    if ((rc = launch(ctx, "k2_lattice_score_oracle", k2_lattice_score_oracle, dim3((unsigned)L.n), dim3(SC_NT), (size_t)lds, p))) return rc;
  }
  std::vector<int32_t> counts, nw, st, words;
  if ((rc = download(ctx, counts_d, 4 * (int64_t)U, &counts)) || (rc = download(ctx, nw_d, U, &nw)) || (rc = download(ctx, status_d, U, &st))) return rc;
  if (ali_h && AT) HIPCHK(hipMemcpyAsync(ali_h, ali_d, 4 * (size_t)AT, hipMemcpyDeviceToHost, ctx->stream));
  const bool want_words = words_h && words_off_h;
  if (want_words) {
    words.resize((size_t)std::max<int64_t>(l->state_off[(size_t)U], 1));
    for (size_t k = 0; k < l->chunks.size(); ++k) {
      const LatChunk& c = l->chunks[k];
      if (c.ns) HIPCHK(hipMemcpyAsync(words.data() + l->state_off[(size_t)c.u0], words_d[k], 4 * (size_t)c.ns, hipMemcpyDeviceToHost, ctx->stream));
    }
  }
  rc = check_err_flag(ctx, name.c_str());     // synchronises: the scratch goes with `dv`
  if (rc) return rc;
  for (int u = 0; u < U; ++u) {
    if (!too_big[(size_t)u]) continue;
    const int32_t R = (int32_t)(ref_off_h[u + 1] - ref_off_h[u]);
    st[(size_t)u] = KHG_LAT_SCRATCH; nw[(size_t)u] = 0;
    counts[4 * (size_t)u] = R; counts[4 * (size_t)u + 1] = 0; counts[4 * (size_t)u + 2] = R; counts[4 * (size_t)u + 3] = 0;
  }
  // (a path whose words do not fit: KHG_LAT_WORDS and none of them; the kernel filled an utterance's slice from its end)
  if (want_words && (rc = pack_words(name, st, &st, [&](size_t u) { return nw[u]; },
                                     [&](size_t u, int64_t n) { return words.begin() + (l->state_off[u + 1] - n); }, words_h, words_off_h, words_cap)))
    return rc;
  if (counts_h) std::copy(counts.begin(), counts.end(), counts_h);
  if (status_h) std::copy(st.begin(), st.end(), status_h);
  return KHG_OK;
}

extern "C" int khg_lattices_wer(khg_ctx* ctx, const khg_lattices* lc, int32_t n_utt, const int32_t* ref_h, const int64_t* ref_off_h, int32_t n_points,
                                const float* graph_scale, const float* acoustic_scale, const float* word_ins_penalty, int32_t* counts_h, int32_t* nwords_h,
                                int32_t* status_h) {
  const std::string name = "khg_lattices_wer", who = name + ": ";
  if (!lc || n_points < 1 || !graph_scale || !acoustic_scale || !word_ins_penalty) return khg_set_error(KHG_E_ARG, who + "bad arguments");
  int rc = score_ref_check(name, lc, n_utt, ref_h, ref_off_h);
  if (rc) return rc;
  for (int k = 0; k < n_points; ++k)
    if (bad_scale(graph_scale[k]) || bad_scale(acoustic_scale[k]) || !std::isfinite(word_ins_penalty[k]))
      return khg_set_error(KHG_E_ARG, who + "point " + std::to_string(k) + ": graph_scale and acoustic_scale must be finite and >= 0, word_ins_penalty finite");
  if (ctx_dead(ctx)) return khg_set_error(KHG_E_ARG, who + "bad arguments");
  if (lc->ctx != ctx) return other_ctx(name);
  khg_lattices* l = const_cast<khg_lattices*>(lc);
  const int U = l->U, K = n_points;
  if (U == 0) return KHG_OK;
  if ((rc = lat_ready(ctx, l))) return rc;
  const int64_t KU = (int64_t)K * U;
  DevBlocks dv;
  int32_t *ref_d, *nw_d, *status_d, *counts_d;
  float* pen_d;
  int64_t *ref_off_d, *hb_off_d;
  unsigned char* hb_d;
  std::vector<LoArgs> pcs;
  if ((rc = score_ref_upload(ctx, U, ref_h, ref_off_h, &dv, &ref_d, &ref_off_d)) || (rc = dv.alloc(KU, &nw_d)) || (rc = dv.alloc(KU, &status_d)) ||
      (rc = dv.alloc(4 * KU, &counts_d)) || (rc = best_path_args(ctx, l, K, graph_scale, acoustic_scale, nw_d, status_d, &dv, &pcs)) ||
      (rc = dv.upload(ctx, word_ins_penalty, K, &pen_d)))
    return rc;
  for (const LoArgs& p : pcs) {
    ScBpArgs q{};
    q.lo = p; q.pen = pen_d;
    if ((rc = launch(ctx, "k2_lattice_score_best_path", k2_lattice_score_best_path, dim3((unsigned)p.n, (unsigned)((K + LO_NT - 1) / LO_NT)), dim3(LO_NT),
                     (size_t)p.lds_bytes, q)))
      return rc;
  }
  // the hypotheses' lengths size the tables: one synchronisation
  std::vector<int32_t> nw, st, counts;
  if ((rc = download(ctx, nw_d, KU, &nw)) || (rc = download(ctx, status_d, KU, &st)) || (rc = check_err_flag(ctx, name.c_str()))) return rc;
  std::vector<int64_t> hb_off((size_t)KU, -1);
  int64_t hb_total = 0, lds = 0;
  const bool no_lds = ctx->opt[KHG_OPT_LAT_OPS_LDS] == 1;
  for (int k = 0; k < K; ++k)
    for (int u = 0; u < U; ++u) {
      const size_t o = (size_t)k * U + u;
      const int64_t H = (st[o] & KHG_LAT_SUCCEEDED) ? nw[o] : 0, W = ref_off_h[u + 1] - ref_off_h[u] + 1;
      const int64_t need = 8 * W + (H + 1) * W;
      if (!no_lds && need <= kScoreWerLds) lds = std::max(lds, need);
      else { hb_off[o] = hb_total; hb_total += (need + 255) & ~int64_t(255); }
    }
  if ((rc = dv.alloc(std::max<int64_t>(hb_total, 1), &hb_d)) || (rc = dv.upload(ctx, hb_off, &hb_off_d))) return rc;
  for (const LoArgs& p : pcs) {
    ScWerArgs w{};
    w.lo = p; w.ref = ref_d; w.ref_off = ref_off_d; w.hb = hb_d; w.hb_off = hb_off_d; w.counts = counts_d;
    if ((rc = launch(ctx, "k2_lattice_score_wer", k2_lattice_score_wer, dim3((unsigned)p.n, (unsigned)K), dim3(SC_NT), (size_t)lds, w))) return rc;
  }
  if ((rc = download(ctx, counts_d, 4 * KU, &counts)) || (rc = check_err_flag(ctx, name.c_str()))) return rc;      // synchronises: the scratch goes with `dv`
  if (counts_h) std::copy(counts.begin(), counts.end(), counts_h);
  if (nwords_h) for (size_t o = 0; o < (size_t)KU; ++o) nwords_h[o] = (st[o] & KHG_LAT_SUCCEEDED) ? nw[o] : 0;
  if (status_h) std::copy(st.begin(), st.end(), status_h);
  return KHG_OK;
}

// compute-wer's core, on the host: the rule of khg_lattices_oracle on the chain of the hypothesis words, cell by cell as written
extern "C" int khg_edit_distance(int32_t n_pairs, const int32_t* ref_h, const int64_t* ref_off_h, const int32_t* hyp_h, const int64_t* hyp_off_h, int32_t* counts_h) {
  const std::string who = "khg_edit_distance: ";
  if (n_pairs < 0 || !ref_off_h || !hyp_off_h || (n_pairs > 0 && !counts_h) || ref_off_h[0] != 0 || hyp_off_h[0] != 0)
    return khg_set_error(KHG_E_ARG, who + "bad arguments (offsets start at 0)");
  for (int i = 0; i < n_pairs; ++i)
    if (ref_off_h[i + 1] < ref_off_h[i] || hyp_off_h[i + 1] < hyp_off_h[i]) return khg_set_error(KHG_E_ARG, who + "offsets decrease at pair " + std::to_string(i));
  if ((ref_off_h[n_pairs] > 0 && !ref_h) || (hyp_off_h[n_pairs] > 0 && !hyp_h)) return khg_set_error(KHG_E_ARG, who + "bad arguments (an array is NULL)");
  const int32_t INF = 1 << 30;
  std::vector<int32_t> prev, row;
  std::vector<unsigned char> mv;
  for (int i = 0; i < n_pairs; ++i) {
    const int32_t* ref = ref_h + ref_off_h[i];
    const int32_t* hyp = hyp_h + hyp_off_h[i];
    const int64_t R = ref_off_h[i + 1] - ref_off_h[i], H = hyp_off_h[i + 1] - hyp_off_h[i], W = R + 1;
    if (R + H >= (int64_t(1) << 29)) return khg_set_error(KHG_E_ARG, who + "pair " + std::to_string(i) + ": the two lengths reach 2^29");
    prev.assign((size_t)W, INF); row.assign((size_t)W, INF);
    mv.assign((size_t)((H + 1) * W), 0);
    for (int64_t h = 0; h <= H; ++h) {
      for (int64_t q = 0; q < W; ++q) {
        int32_t C = h == 0 && q == 0 ? 0 : INF;
        unsigned char m = 0;
        if (h > 0) {
          if (q > 0 && prev[(size_t)q - 1] < INF) { const int32_t c = prev[(size_t)q - 1] + (hyp[h - 1] != ref[q - 1] ? 1 : 0); if (c < C) { C = c; m = 1; } }
          if (prev[(size_t)q] < INF) { const int32_t c = prev[(size_t)q] + 1; if (c < C) { C = c; m = 2; } }
        }
        if (q > 0 && row[(size_t)q - 1] < INF && row[(size_t)q - 1] + 1 < C) { C = row[(size_t)q - 1] + 1; m = 3; }
        row[(size_t)q] = C;
        mv[(size_t)(h * W + q)] = m;
      }
      prev.swap(row);
    }
    int64_t h = H, q = R;
    int32_t ins = 0, del = 0, sub = 0;
    while (h > 0 || q > 0) {
      const unsigned char m = mv[(size_t)(h * W + q)];
      if (m == 1) { --h; --q; if (hyp[h] != ref[q]) ++sub; }
      else if (m == 2) { --h; ++ins; }
      else { --q; ++del; }
    }
    counts_h[4 * (size_t)i] = ins + del + sub; counts_h[4 * (size_t)i + 1] = ins; counts_h[4 * (size_t)i + 2] = del; counts_h[4 * (size_t)i + 3] = sub;
  }
  return KHG_OK;
}

// ------------------------------------------------------------------------------------------
// K2B: minimum Bayes risk decoding and word confidences (khg_k2_lattice_mbr.hip.inc)
struct khg_mbr {
  int U = 0;
  khg_ctx* ctx = nullptr;
  int64_t bytes = 0;
  std::vector<int64_t> state_off, arc_off;              // the lattice handle's
  std::vector<int32_t> status, iters, nwords, nvocab;   // [U]
  std::vector<double> risk;                             // [U]
  std::vector<int64_t> cap_off, gout_off;               // [U + 1]: the slots of an utterance's words / conf, and of its table
  double *arc_cond_d = nullptr, *final_cond_d = nullptr, *conf_d = nullptr, *gamma_d = nullptr;      // [arcs], [states], [cap_off[U]], [gout_off[U]]
  int32_t *vocab_d = nullptr, *hyp_d = nullptr;         // [arcs + U] (utterance u's slot at arc_off[u] + u), [2 * cap_off[U]]
};

namespace {
struct MbrFree { void operator()(khg_mbr* m) const { (void)khg_mbr_destroy(m); } };
using MbrPtr = std::unique_ptr<khg_mbr, MbrFree>;
template <class T>
int mbr_alloc(khg_mbr* m, int64_t count, T** out) {
  HIPCHK(hipMalloc(reinterpret_cast<void**>(out), (size_t)std::max<int64_t>(count * (int64_t)sizeof(T), 16)));
  m->bytes += count * (int64_t)sizeof(T);
  return KHG_OK;
}
}  // namespace

extern "C" int khg_mbr_destroy(khg_mbr* m) {
  if (!m) return KHG_OK;
  void* blocks[6] = {m->arc_cond_d, m->final_cond_d, m->conf_d, m->gamma_d, m->vocab_d, m->hyp_d};
  for (void* q : blocks) if (q) (void)hipFree(q);
  delete m;
  return KHG_OK;
}
extern "C" int khg_mbr_device_bytes(const khg_mbr* m, int64_t* bytes) {
  if (!m || !bytes) return khg_set_error(KHG_E_ARG, "khg_mbr_device_bytes: bad arguments");
  *bytes = m->bytes;
  return KHG_OK;
}
extern "C" int khg_mbr_sizes(const khg_mbr* m, int64_t* words_off_h, int64_t* vocab_off_h, int64_t* gamma_off_h) {
  if (!m) return khg_set_error(KHG_E_ARG, "khg_mbr_sizes: bad arguments");
  int64_t w = 0, v = 0, g = 0;
  for (int u = 0; u <= m->U; ++u) {
    if (words_off_h) words_off_h[u] = w;
    if (vocab_off_h) vocab_off_h[u] = v;
    if (gamma_off_h) gamma_off_h[u] = g;
    if (u == m->U || !(m->status[(size_t)u] & KHG_LAT_SUCCEEDED)) continue;
    const int64_t W = m->nwords[(size_t)u], V = m->nvocab[(size_t)u];
    w += W; v += V; g += (2 * W + 1) * V;
  }
  return KHG_OK;
}
extern "C" int khg_mbr_download(khg_ctx* ctx, const khg_mbr* m, int32_t* status_h, int32_t* iters_h, double* bayes_risk_h, int32_t* words_h, double* conf_h,
                                int32_t* vocab_h, double* gamma_h, double* arc_cond_h, double* final_cond_h) {
  if (ctx_dead(ctx) || !m) return khg_set_error(KHG_E_ARG, "khg_mbr_download: bad arguments");
  if (m->ctx != ctx) return other_ctx("khg_mbr_download");
  const size_t U = (size_t)m->U;
  if (status_h) std::copy(m->status.begin(), m->status.end(), status_h);
  if (iters_h) std::copy(m->iters.begin(), m->iters.end(), iters_h);
  if (bayes_risk_h) std::copy(m->risk.begin(), m->risk.end(), bayes_risk_h);
  if (U == 0) return KHG_OK;
  const int64_t NA = m->arc_off[U], NS = m->state_off[U];
  if (arc_cond_h && NA) HIPCHK(hipMemcpyAsync(arc_cond_h, m->arc_cond_d, 8 * (size_t)NA, hipMemcpyDeviceToHost, ctx->stream));
  if (final_cond_h && NS) HIPCHK(hipMemcpyAsync(final_cond_h, m->final_cond_d, 8 * (size_t)NS, hipMemcpyDeviceToHost, ctx->stream));
  // an utterance's results lie at the head of its slot: the slots come back in one copy per array and are packed here
  const int64_t CT = m->cap_off[U], GT = m->gout_off[U];
  std::vector<int32_t> hyp, voc;
  std::vector<double> conf, gam;
  int rc;
  if ((rc = download(ctx, m->hyp_d, words_h ? 2 * CT : 0, &hyp)) || (rc = download(ctx, m->vocab_d, vocab_h ? NA + (int64_t)U : 0, &voc)) ||
      (rc = download(ctx, m->conf_d, conf_h ? CT : 0, &conf)) || (rc = download(ctx, m->gamma_d, gamma_h ? GT : 0, &gam)))
    return rc;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  int64_t w = 0, v = 0, g = 0;
  for (size_t u = 0; u < U; ++u) {
    if (!(m->status[u] & KHG_LAT_SUCCEEDED)) continue;
    const int64_t W = m->nwords[u], V = m->nvocab[u], G = (2 * W + 1) * V;
    if (words_h) std::copy_n(hyp.begin() + 2 * m->cap_off[u], W, words_h + w);
    if (conf_h) std::copy_n(conf.begin() + m->cap_off[u], W, conf_h + w);
    if (vocab_h) std::copy_n(voc.begin() + m->arc_off[u] + (int64_t)u, V, vocab_h + v);
    if (gamma_h) std::copy_n(gam.begin() + m->gout_off[u], G, gamma_h + g);
    w += W; v += V; g += G;
  }
  return KHG_OK;
}

extern "C" int khg_lattices_mbr(khg_ctx* ctx, const khg_lattices* lc, float graph_scale, float acoustic_scale, int32_t decode_mbr, int32_t max_iter,
                                int32_t n_utt, const int32_t* init_h, const int64_t* init_off_h, const int32_t* init_given_h, int32_t max_words,
                                int64_t scratch_bytes, khg_mbr** out) {
  const std::string name = "khg_lattices_mbr", who = name + ": ";
  if (out) *out = nullptr;
  if (bad_scale(graph_scale) || bad_scale(acoustic_scale)) return khg_set_error(KHG_E_ARG, who + "graph_scale and acoustic_scale must be finite and >= 0");
  if (max_iter < 0) return khg_set_error(KHG_E_ARG, who + "max_iter must be >= 0");
  if (max_words < 0 || max_words > MB_MAX_WORDS) return khg_set_error(KHG_E_ARG, who + "max_words must lie in 0 .. " + std::to_string(MB_MAX_WORDS));
  if (scratch_bytes < 0) return khg_set_error(KHG_E_ARG, who + "scratch_bytes must be >= 0");
  if (!lc || !out) return khg_set_error(KHG_E_ARG, who + "bad arguments");
  khg_lattices* l = const_cast<khg_lattices*>(lc);
  const int U = l->U;
  if (n_utt != U) return khg_set_error(KHG_E_ARG, who + "the lattices hold " + std::to_string(U) + " utterances, the call names " + std::to_string(n_utt));
  if (init_off_h) {
    int rc = check_offsets(name, "init_off_h", init_off_h, U, "utterance", init_h, "init_h");
    if (rc) return rc;
    for (int u = 0; u < U; ++u)
      for (int64_t i = init_off_h[u]; i < init_off_h[u + 1]; ++i)
        if (init_h[i] <= 0) return khg_set_error(KHG_E_ARG, who + "utterance " + std::to_string(u) + ": an initial word is not > 0");
  }
  if (ctx_dead(ctx)) return khg_set_error(KHG_E_ARG, who + "bad arguments");
  if (l->ctx != ctx) return other_ctx(name);
  MbrPtr res(new khg_mbr);
  khg_mbr* m = res.get();
  m->U = U; m->ctx = ctx; m->state_off = l->state_off; m->arc_off = l->arc_off;
  m->status.assign((size_t)U, 0); m->iters.assign((size_t)U, 0); m->nwords.assign((size_t)U, 0); m->nvocab.assign((size_t)U, 0);
  m->risk.assign((size_t)U, std::numeric_limits<double>::infinity());
  m->cap_off.assign((size_t)U + 1, 0); m->gout_off.assign((size_t)U + 1, 0);
  if (U == 0) { *out = res.release(); return KHG_OK; }
  const int64_t budget = scratch_bytes ? scratch_bytes : kScoreScratch;
  const int64_t NS = l->state_off[(size_t)U], NA = l->arc_off[(size_t)U];
  // the initial hypotheses: the caller's, or the best path's words at the same pair
  std::vector<std::vector<int32_t>> init((size_t)U);
  bool need_best = false;
  for (int u = 0; u < U; ++u) {
    if (init_off_h && (!init_given_h || init_given_h[u])) init[(size_t)u].assign(init_h + init_off_h[u], init_h + init_off_h[u + 1]);
    else need_best = true;
  }
  if (need_best) {
    std::vector<int32_t> words((size_t)NS + 1), st((size_t)U);
    std::vector<int64_t> woff((size_t)U + 1, 0);
    int rc = khg_lattices_best_path(ctx, lc, 1, &graph_scale, &acoustic_scale, nullptr, words.data(), woff.data(), NS + 1, nullptr, st.data());
    if (rc) return rc;
    for (int u = 0; u < U; ++u)
      if (!(init_off_h && (!init_given_h || init_given_h[u])) && (st[(size_t)u] & KHG_LAT_SUCCEEDED))
        init[(size_t)u].assign(words.begin() + woff[(size_t)u], words.begin() + woff[(size_t)u + 1]);
  }
  int rc = lat_ready(ctx, l, kWithIndex);
  if (rc) return rc;
  if ((rc = mbr_alloc(m, NA, &m->arc_cond_d)) || (rc = mbr_alloc(m, NS, &m->final_cond_d)) || (rc = mbr_alloc(m, NA + U, &m->vocab_d))) return rc;
  DevBlocks dv;
  int32_t *nv_d, *mw_d, *widx_d;
  if ((rc = dv.alloc(U, &nv_d)) || (rc = dv.alloc(U, &mw_d)) || (rc = dv.alloc(std::max<int64_t>(NA, 1), &widx_d))) return rc;
  std::vector<int32_t> st, nv, mw;
  {
    // the weights: khg_lattices_posteriors' chunk steps around k2_lattice_mbr_weights (the run's own result handle is dropped)
    PostRun r;
    r.ctx = ctx; r.l = l; r.who = "khg_lattices_mbr";
    r.gs = (double)graph_scale; r.as = (double)acoustic_scale;
    new_posteriors(ctx, U, &r.res);
    if ((rc = post_run_begin(r))) return rc;
    for (size_t k = 0; k < l->chunks.size(); ++k) {
      const LatChunk& c = l->chunks[k];
      const int64_t cs0 = l->state_off[(size_t)c.u0], ca0 = l->arc_off[(size_t)c.u0];
      PoArgs p{};
      if ((rc = post_chunk_begin(r, k, 24, &p))) return rc;
      p.arc_post = m->arc_cond_d + ca0;
      int32_t *len_d, *first_d;
      const LatIndex ix = lat_index_arrays(l->idx_d[k], c);
      if ((rc = launch(ctx, "k2_lattice_mbr_weights", k2_lattice_mbr_weights, dim3((unsigned)c.n), dim3(PO_NT), (size_t)p.lo.lds_bytes, p, m->final_cond_d + cs0)) ||
          (rc = r.dv.alloc(std::max<int64_t>(c.ns, 1), &len_d)) || (rc = r.dv.alloc(std::max<int64_t>(c.na, 1), &first_d)) ||
          (rc = launch(ctx, "k2_lattice_mbr_prepare", k2_lattice_mbr_prepare, dim3((unsigned)c.n), dim3(MB_NT), 0, p.lo, ix.arc_src, len_d, first_d, m->vocab_d,
                       widx_d + ca0, nv_d, mw_d)))
        return rc;
    }
    if ((rc = download(ctx, r.status_d, U, &st)) || (rc = download(ctx, nv_d, U, &nv)) || (rc = download(ctx, mw_d, U, &mw)) ||
        (rc = check_err_flag(ctx, name.c_str())))      // synchronises: the run's scratch goes with `r`
      return rc;
  }
  // the caps, the slots, and the utterances that run, grouped into launches whose tables fit the budget together
  std::vector<int32_t> cap((size_t)U, 0), w0((size_t)U, 0);
  const TableLaunches g = group_tables(l->chunks, 8, budget, [&](int u) -> int64_t {
    const size_t su = (size_t)u;
    m->status[su] = st[su]; m->nvocab[su] = nv[su];
    m->cap_off[su + 1] = m->cap_off[su]; m->gout_off[su + 1] = m->gout_off[su];
    if (!(st[su] & KHG_LAT_SUCCEEDED)) return -1;
    const int64_t W0 = (int64_t)init[su].size();
    const int64_t cp = max_words > 0 ? max_words : std::max<int64_t>(W0, mw[su]);
    if (W0 > cp || cp > MB_MAX_WORDS) { m->status[su] = KHG_LAT_WORDS; return -1; }
    const int64_t N = l->state_off[su + 1] - l->state_off[su], C = 2 * cp + 2, cells = (2 * (N + 1) + nv[su]) * C;
    if (8 * cells > budget) { m->status[su] = KHG_LAT_SCRATCH; return -1; }
    cap[su] = (int32_t)cp; w0[su] = (int32_t)W0;
    m->cap_off[su + 1] += cp; m->gout_off[su + 1] += (2 * cp + 1) * nv[su];
    return cells;
  });
  const std::vector<int32_t>& list = g.list;
  const int64_t CT = m->cap_off[(size_t)U], GT = m->gout_off[(size_t)U];
  if ((rc = mbr_alloc(m, CT, &m->conf_d)) || (rc = mbr_alloc(m, GT, &m->gamma_d)) || (rc = mbr_alloc(m, 2 * CT, &m->hyp_d))) return rc;
  if (!list.empty()) {
    std::vector<int32_t> hyp((size_t)std::max<int64_t>(2 * CT, 1), 0);
    for (int u : list) std::copy(init[(size_t)u].begin(), init[(size_t)u].end(), hyp.begin() + 2 * m->cap_off[(size_t)u]);
    int32_t *cap_d, *w0_d, *status_d, *iters_d, *nw_d, *list_d;
    int64_t *cap_off_d, *gout_off_d, *tab_off_d;
    double *risk_d, *tab_d;
    HIPCHK(hipMemcpyAsync(m->hyp_d, hyp.data(), 4 * (size_t)(2 * CT), hipMemcpyHostToDevice, ctx->stream));
    if ((rc = dv.upload(ctx, cap, &cap_d)) || (rc = dv.upload(ctx, w0, &w0_d)) || (rc = dv.upload(ctx, m->cap_off, &cap_off_d)) ||
        (rc = dv.upload(ctx, m->gout_off, &gout_off_d)) || (rc = dv.upload(ctx, list, &list_d)) || (rc = dv.upload(ctx, g.tab_off, &tab_off_d)) ||
        (rc = dv.zeroed(ctx, U, &status_d)) || (rc = dv.alloc(U, &iters_d)) || (rc = dv.alloc(U, &nw_d)) || (rc = dv.alloc(U, &risk_d)) ||
        (rc = dv.alloc(g.max_cells, &tab_d)))
      return rc;
    for (const TableLaunch& L : g.launches) {
      const LatChunk& c = l->chunks[L.chunk];
      const int64_t cs0 = l->state_off[(size_t)c.u0], ca0 = l->arc_off[(size_t)c.u0];
      MbArgs p{};
      lat_chunk_args(l, c, &p.lo);
      const LatIndex ix = lat_index_arrays(l->idx_d[L.chunk], c);
      p.in_begin = ix.in_begin; p.in_arc = ix.in_arc; p.arc_src = ix.arc_src;
      p.list = list_d + L.first; p.tab_off = tab_off_d + L.first; p.tab = tab_d;
      p.arc_cond = m->arc_cond_d + ca0; p.final_cond = m->final_cond_d + cs0;
      p.widx = widx_d + ca0; p.vocab = m->vocab_d; p.nvocab = nv_d;
      p.cap = cap_d; p.w0 = w0_d; p.cap_off = cap_off_d; p.gout_off = gout_off_d;
      p.hyp = m->hyp_d; p.conf = m->conf_d; p.gamma_out = m->gamma_d;
      p.status = status_d; p.iters = iters_d; p.nwords = nw_d; p.risk = risk_d;
      p.decode_mbr = decode_mbr ? 1 : 0; p.max_iter = max_iter;
      if ((rc = launch(ctx, "k2_lattice_mbr", k2_lattice_mbr, dim3((unsigned)L.n), dim3(MB_NT), 0, p))) return rc;
    }
    std::vector<int32_t> st2, it, nw;
    std::vector<double> rk;
    if ((rc = download(ctx, status_d, U, &st2)) || (rc = download(ctx, iters_d, U, &it)) || (rc = download(ctx, nw_d, U, &nw)) ||
        (rc = download(ctx, risk_d, U, &rk)) || (rc = check_err_flag(ctx, name.c_str())))      // synchronises: the scratch goes with `dv`
      return rc;
    for (int u : list) {
      const size_t su = (size_t)u;
      m->status[su] = st2[su]; m->iters[su] = it[su];
      if (st2[su] & KHG_LAT_SUCCEEDED) { m->nwords[su] = nw[su]; m->risk[su] = rk[su]; }
    }
  }
  *out = res.release();
  return KHG_OK;
}

// ------------------------------------------------------------------------------------------
// K2N: the n best paths (khg_k2_lattice_nbest.hip.inc)
// The entries of the utterances u0 .. u0 + n, made by one launch of the fill: exactly-sized blocks, the utterances one after the other
struct NbBlock {
  int u0 = 0, n = 0;
  int64_t e0 = 0, ne = 0, w0 = 0, nw = 0, a0 = 0, na = 0;       // first entry / word / alignment cell in the handle's order, and how many
  int32_t *ali_d = nullptr, *words_d = nullptr, *nw_d = nullptr;
  float *weight_d = nullptr, *total_d = nullptr;
};
struct khg_nbest {
  int U = 0;
  khg_ctx* ctx = nullptr;
  int64_t bytes = 0;
  std::vector<int32_t> status;                          // [U]
  std::vector<int64_t> entry_off, words_off;            // [U + 1], [entries + 1]
  std::vector<NbBlock> blocks;
};

namespace {
struct NbFree { void operator()(khg_nbest* m) const { (void)khg_nbest_destroy(m); } };
using NbPtr = std::unique_ptr<khg_nbest, NbFree>;
template <class T>
int nb_alloc(khg_nbest* m, int64_t count, T** out) {
  HIPCHK(hipMalloc(reinterpret_cast<void**>(out), (size_t)std::max<int64_t>(count * (int64_t)sizeof(T), 16)));
  m->bytes += count * (int64_t)sizeof(T);
  return KHG_OK;
}
}  // namespace

extern "C" int khg_nbest_destroy(khg_nbest* m) {
  if (!m) return KHG_OK;
  for (NbBlock& b : m->blocks) {
    void* blocks[5] = {b.ali_d, b.words_d, b.nw_d, b.weight_d, b.total_d};
    for (void* q : blocks) if (q) (void)hipFree(q);
  }
  delete m;
  return KHG_OK;
}
extern "C" int khg_nbest_device_bytes(const khg_nbest* m, int64_t* bytes) {
  if (!m || !bytes) return khg_set_error(KHG_E_ARG, "khg_nbest_device_bytes: bad arguments");
  *bytes = m->bytes;
  return KHG_OK;
}
extern "C" int khg_nbest_sizes(const khg_nbest* m, int64_t* entry_off_h, int64_t* words_off_h) {
  if (!m) return khg_set_error(KHG_E_ARG, "khg_nbest_sizes: bad arguments");
  if (entry_off_h) std::copy(m->entry_off.begin(), m->entry_off.end(), entry_off_h);
  if (words_off_h) std::copy(m->words_off.begin(), m->words_off.end(), words_off_h);
  return KHG_OK;
}
extern "C" int khg_nbest_download(khg_ctx* ctx, const khg_nbest* m, int32_t* ali_h, int32_t* words_h, float* weight_h, float* total_h) {
  if (ctx_dead(ctx) || !m) return khg_set_error(KHG_E_ARG, "khg_nbest_download: bad arguments");
  if (m->ctx != ctx) return other_ctx("khg_nbest_download");
  for (const NbBlock& b : m->blocks) {
    if (ali_h && b.na) HIPCHK(hipMemcpyAsync(ali_h + b.a0, b.ali_d, 4 * (size_t)b.na, hipMemcpyDeviceToHost, ctx->stream));
    if (words_h && b.nw) HIPCHK(hipMemcpyAsync(words_h + b.w0, b.words_d, 4 * (size_t)b.nw, hipMemcpyDeviceToHost, ctx->stream));
    if (weight_h && b.ne) HIPCHK(hipMemcpyAsync(weight_h + 2 * b.e0, b.weight_d, 8 * (size_t)b.ne, hipMemcpyDeviceToHost, ctx->stream));
    if (total_h && b.ne) HIPCHK(hipMemcpyAsync(total_h + b.e0, b.total_d, 4 * (size_t)b.ne, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return KHG_OK;
}

extern "C" int khg_lattices_nbest(khg_ctx* ctx, const khg_lattices* lc, float graph_scale, float acoustic_scale, int32_t n, int32_t* status_h,
                                  khg_nbest** out) {
  const std::string name = "khg_lattices_nbest", who = name + ": ";
  if (ctx_dead(ctx) || !lc || !out) return khg_set_error(KHG_E_ARG, who + "bad arguments");
  *out = nullptr;
  if (lc->ctx != ctx) return other_ctx(name);
  if (bad_scale(graph_scale) || bad_scale(acoustic_scale)) return khg_set_error(KHG_E_ARG, who + "graph_scale and acoustic_scale must be finite and >= 0");
  if (n < 1 || n > KHG_NBEST_MAX) return khg_set_error(KHG_E_ARG, who + "n must lie in 1 .. " + std::to_string(KHG_NBEST_MAX));
  khg_lattices* l = const_cast<khg_lattices*>(lc);
  const int U = l->U;
  NbPtr res(new khg_nbest);
  khg_nbest* m = res.get();
  m->U = U; m->ctx = ctx;
  m->status.assign((size_t)U, 0); m->entry_off.assign((size_t)U + 1, 0); m->words_off.assign(1, 0);
  if (U == 0) { *out = res.release(); return KHG_OK; }
  int rc = lat_ready(ctx, l, kWithIndex);
  if (rc) return rc;
  // the running lists: in LDS when the device gives 52 n bytes (and KHG_OPT_LAT_OPS_LDS is not 1), else in HBM rows
  int64_t lds_cap = 0;
  if ((rc = score_lds_cap(&lds_cap))) return rc;
  const int64_t lds_need = 4 * (int64_t)NB_ROW_WORDS * n;
  const bool use_lds = ctx->opt[KHG_OPT_LAT_OPS_LDS] != 1 && lds_need <= lds_cap;
  const int64_t arena = ctx->opt[KHG_OPT_NBEST_ARENA] > 0 ? (int64_t)ctx->opt[KHG_OPT_NBEST_ARENA] << 10 : kNbestArena;
  DevBlocks dv;
  int32_t* status_d;
  int64_t* ali_off_d;
  if ((rc = dv.alloc(U, &status_d)) || (rc = dv.upload(ctx, l->ali_off, &ali_off_d))) return rc;
  std::vector<std::vector<int64_t>> ali_bases;      // (a launch's upload lives until the launch is done)
  std::vector<std::vector<int32_t>> nws;            // per block, the entries' word counts
  int64_t E = 0, W = 0, AL = 0;
  for (size_t k = 0; k < l->chunks.size(); ++k) {
    const LatChunk& c = l->chunks[k];
    NbArgs p{};
    lat_chunk_args(l, c, &p.lo);
    const LatIndex ix = lat_index_arrays(l->idx_d[k], c);
    p.in_begin = ix.in_begin; p.in_arc = ix.in_arc; p.arc_src = ix.arc_src;
    p.gs = graph_scale; p.as = acoustic_scale; p.nb = n; p.status = status_d; p.ali_off = ali_off_d;
    const int64_t cs = std::max<int64_t>(c.ns, 1);
    int64_t* utt_off;
    if ((rc = dv.alloc(cs, &p.len)) || (rc = dv.alloc(cs, &p.loff)) || (rc = dv.alloc(cs, &p.alen)) || (rc = dv.alloc(2 * (int64_t)c.n, &p.utt_tot)) ||
        (rc = dv.alloc(2 * ((int64_t)c.n + 1), &utt_off)) || (rc = dv.alloc(2 * (int64_t)c.n, &p.utt_tot2)))
      return rc;
    p.utt_off = utt_off;
    // 1. and 2. the bounds, and the one synchronisation that sizes the arena
    std::vector<int64_t> ro, so;
    if ((rc = launch(ctx, "k2_lattice_nbest_count", k2_lattice_nbest_count, dim3((unsigned)c.n), dim3(NB_NT), 0, p)) ||
        (rc = scan_pairs_and_read(ctx, "k2_lattice_nbest_scan", p.utt_tot, utt_off, c.n, &ro, &so)))
      return rc;
    const int64_t slots = std::max<int64_t>(so[(size_t)c.n], 1);
    if ((rc = dv.alloc(slots, &p.s_end)) || (rc = dv.alloc(slots, &p.s_rank)) || (rc = dv.alloc(slots, &p.s_nw)) || (rc = dv.alloc(slots, &p.s_woff)) ||
        (rc = dv.alloc(slots, &p.s_a)) || (rc = dv.alloc(slots, &p.s_b)) || (rc = dv.alloc(slots, &p.s_tot)))
      return rc;
    // the chunk's utterances in launches whose lists fit the budget together (an utterance above it is a launch of its own)
    for (size_t g0 = 0; g0 < (size_t)c.n;) {
      size_t g1 = g0 + 1;
      while (g1 < (size_t)c.n && 24 * (ro[g1 + 1] - ro[g0]) <= arena) ++g1;
      const int gn = (int)(g1 - g0);
      const int64_t R = ro[g1] - ro[g0], rows = std::max<int64_t>(R, 1);
      DevBlocks ga;       // the launch's arena
      int64_t* utt_off2;
      if ((rc = ga.alloc(rows, &p.r_t)) || (rc = ga.alloc(rows, &p.r_a)) || (rc = ga.alloc(rows, &p.r_b)) || (rc = ga.alloc(rows, &p.r_nw)) ||
          (rc = ga.alloc(rows, &p.r_e)) || (rc = ga.alloc(rows, &p.r_j)) || (rc = ga.alloc(2 * ((int64_t)gn + 1), &utt_off2)))
        return rc;
      p.rows = nullptr;
      if (!use_lds && (rc = ga.alloc((int64_t)gn * NB_ROW_WORDS * n, &p.rows))) return rc;
      p.b0 = (int)g0; p.gn = gn; p.arena_base = ro[g0]; p.arena_size = R; p.utt_off2 = utt_off2;
      // 3. the lists and the entries; 4. the scan of the entries and their words, with the synchronisation that sizes the block
      if (use_lds) {
        if ((rc = khg_lds_attribute(reinterpret_cast<const void*>(k2_lattice_nbest_fill<true>), (size_t)lds_need)) ||
            (rc = launch(ctx, "k2_lattice_nbest_fill", k2_lattice_nbest_fill<true>, dim3((unsigned)gn), dim3(NB_NT), (size_t)lds_need, p)))
          return rc;
      } else if ((rc = launch(ctx, "k2_lattice_nbest_fill", k2_lattice_nbest_fill<false>, dim3((unsigned)gn), dim3(NB_NT), 0, p))) {
        return rc;
      }
      std::vector<int64_t> eo, wo;
      if ((rc = scan_pairs_and_read(ctx, "k2_lattice_nbest_words", p.utt_tot2 + 2 * g0, utt_off2, gn, &eo, &wo))) return rc;
      NbBlock bl;
      bl.u0 = c.u0 + (int)g0; bl.n = gn; bl.e0 = E; bl.w0 = W; bl.a0 = AL; bl.ne = eo[(size_t)gn]; bl.nw = wo[(size_t)gn];
      ali_bases.emplace_back((size_t)gn, 0);
      std::vector<int64_t>& ab = ali_bases.back();
      for (int g = 0; g < gn; ++g) {
        const size_t u = (size_t)bl.u0 + (size_t)g;
        const int64_t cnt = eo[(size_t)g + 1] - eo[(size_t)g];
        ab[(size_t)g] = bl.na;
        bl.na += cnt * (l->ali_off[u + 1] - l->ali_off[u]);
        m->entry_off[u + 1] = m->entry_off[u] + cnt;
      }
      m->blocks.push_back(bl);
      NbBlock& B = m->blocks.back();
      if ((rc = nb_alloc(m, B.na, &B.ali_d)) || (rc = nb_alloc(m, B.nw, &B.words_d)) || (rc = nb_alloc(m, B.ne, &B.nw_d)) ||
          (rc = nb_alloc(m, 2 * B.ne, &B.weight_d)) || (rc = nb_alloc(m, B.ne, &B.total_d)))
        return rc;
      if (B.na) HIPCHK(hipMemsetAsync(B.ali_d, 0, 4 * (size_t)B.na, ctx->stream));
      int64_t* ab_d;
      if ((rc = ga.upload(ctx, ab, &ab_d))) return rc;
      p.ali_base = ab_d;
      p.o_ali = B.ali_d; p.o_words = B.words_d; p.o_nw = B.nw_d; p.o_weight = B.weight_d; p.o_total = B.total_d;
      p.o_ne = B.ne; p.o_nwords = B.nw; p.o_na = B.na;
      nws.emplace_back();
      if (B.ne > 0 &&
          ((rc = launch(ctx, "k2_lattice_nbest_trace", k2_lattice_nbest_trace, dim3((unsigned)gn, (unsigned)((n + NB_NT - 1) / NB_NT)), dim3(NB_NT), 0, p)) ||
           (rc = download(ctx, B.nw_d, B.ne, &nws.back()))))
        return rc;
      HIPCHK(hipStreamSynchronize(ctx->stream));       // the arena goes with `ga`
      E += B.ne; W += B.nw; AL += B.na;
      g0 = g1;
    }
  }
  if ((rc = download(ctx, status_d, U, &m->status)) || (rc = check_err_flag(ctx, name.c_str()))) return rc;     // synchronises: the scratch goes with `dv`
  m->words_off.reserve((size_t)E + 1);
  for (const std::vector<int32_t>& v : nws)
    for (int32_t w : v) m->words_off.push_back(m->words_off.back() + w);
  if (status_h) std::copy(m->status.begin(), m->status.end(), status_h);
  *out = res.release();
  return KHG_OK;
}
