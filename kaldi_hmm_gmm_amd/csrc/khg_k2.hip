// kaldi_hmm_gmm_amd/csrc/khg_k2.hip -- C-ABI (include/khg_hip.h): K2, Viterbi forced alignment (khg_align): the LDS budgets (k2_lds_*),
// kernel selection by graph shape (k2_plan), the kernel table (k2_insts) and its one launch (k2_launch), and khg_align as a list of
// steps -- checks, scratch, K2Args, the exact DP on the main stream, the order-faithful decoder on a side stream, the KHG_OPT_K2_PROF
// report, the download; the resident alignment (khg_ali_upload, khg_ali_download).  The lattice decoders and everything on lattices
// are khg_lattices.hip.  gfx950 only.
#include "khg_internal.hpp"

#include "khg_k2_hashlist.hip.inc"
#include "khg_k2_viterbi.hip.inc"

// ------------------------------------------------------------------------------------------
// K2
extern "C" void khg_align_config_default(khg_align_config* c) {
  c->beam = 200.0f; c->retry_beam = 0.0f; c->careful = 0; c->acoustic_scale = 1.0f;
  c->max_active = INT32_MAX; c->min_active = 20; c->beam_delta = 0.5f; c->hash_ratio = 2.0f;
  c->like_scale = 0.0f;
}

// The resident alignment.  Small sets with graphs keep everything khg_align hands back -- [status | like | num_words | words | ali] --
// in ONE block (of the context's arena: one download into its pinned mirror instead of five pageable copies).
static int ensure_ali(khg_ctx* ctx, khg_utts* u) {
  if (u->ali_d) return KHG_OK;
  if (u->small && u->has_graphs) {
    const size_t nu = (size_t)u->n_utt, nw = (size_t)u->words_off[u->n_utt];
    const size_t bytes = 4 * (3 * nu + nw + (size_t)u->N) + 64;
    int rc = u_alloc(u, &u->out_blk_d, bytes);
    if (rc) return rc;
    u->out_blk_bytes = bytes;
    int32_t* p = reinterpret_cast<int32_t*>(u->out_blk_d);
    u->status_d = p; u->like_d = reinterpret_cast<float*>(p + nu); u->num_words_d = p + 2 * nu; u->words_d = p + 3 * nu; u->ali_d = p + 3 * nu + nw;
    return KHG_OK;
  }
  return u_alloc(u, &u->ali_d, (size_t)u->N);
}

// ------------------------------------------------------------------------------------------
// The LDS budgets, in bytes, for the batch maxima: S states, A in-arcs, max_npdf score rows.  Each formula restates the carve-up at the
// top of its kernel (khg_k2_viterbi.hip.inc, which points back here by name): the two change together.
// k2_viterbi_dp: cur | nxt | reductions | arcs | in_off | wave minima/counts | flags | [align] | `tail`: max(score block (generic), trace-back block)
static size_t k2_lds_dp(size_t S, size_t A, size_t nwave, size_t tail) {
  return 16 * S + 8 * K2_MAXW + 8 * A + 4 * (S + 1) + 8 * K2_FB * nwave + 32 + 8 * K2_MAXW + 16 + tail + 64;
}
// trace-back block: fast = five groups of eight layers, one dword per lane and state slot (NS per thread; no score block)
// (fast: also the waves' strips of parked layer minima / counts, 2.5 KB each, in the same area during the forward pass)
static size_t k2_lds_dp_fast(size_t S, size_t A, size_t nthr, size_t NS) {
  return k2_lds_dp(S, A, nthr / 64, std::max<size_t>(5 * nthr * NS * 4, 2560 * (nthr / 64)));
}
// ... generic = 33 layers of bytes, or the score block of K2_SB frames where that is larger
static size_t k2_lds_dp_generic(size_t S, size_t A, size_t nwave, size_t max_npdf) {
  return k2_lds_dp(S, A, nwave, std::max<size_t>(4 * K2_SB * (max_npdf | 1), (K2_FB + 1) * ((S + 15) & ~size_t(15))));
}
// k2_viterbi_faithful: two elem pools | last / previous bucket (HB each) | work queue | GetCutoff's array | in_off | src, col, dst, w | ordinals
static size_t k2_lds_lane(size_t S, size_t A) {
  const size_t HB = std::max<size_t>(2 * S, 1000);
  return 32 * S + 8 * HB + 4 * (S + A) + 4 * S + 4 * (S + 1) + 16 * A + A + 64;
}
// k2_viterbi_faithful_wave, the per-frame tables: token costs x 2 | state keys | token states x 2, first, winner | GetCutoff's array |
// the score row | (exact slot prefix sums, odeg_w = 0: slot -> token, token -> first slot) | (state -> position) | (epsilon worklist) |
// survivor masks
static size_t k2_lds_wave_mut(size_t S, size_t A, size_t max_npdf, int odeg_w, bool use_pos, bool has_eps) {
  return 16 * S + 8 * S + 4 * 4 * S + 4 * S + 4 * max_npdf + (odeg_w ? 0 : 4 * A + 4 * S) + (use_pos ? 4 * S : 0) +
         (has_eps ? 4 * (S + A + 1) : 0) + 8 + 8 * ((std::max(A, S * (size_t)odeg_w) + 63) / 64 + 1);
}
// ... and its graph tables (LDS behind the per-frame tables, or the utterance's HBM scratch slice): in_off, out_off | src, col, w, dst,
// out-arc -> in-arc | (epsilon-input arcs: offsets, in-arc indices) | ordinals, flags
static size_t k2_lds_wave_graph(size_t S, size_t A, bool has_eps) {
  return 8 * (S + 1) + 5 * 4 * A + (has_eps ? 4 * (S + 1) + 4 * A : 0) + A + S + 64;
}
// k2_viterbi_faithful_chain<ODEG>.
// the frame loop's tables: token costs x 2 + state keys (24) | first / winner (8) | token states x 2 (4): 36 per state; per out-arc slot:
// parked cost (8) + record (8) + info (4, GetCutoff's array over it) + ordinal (1); the score row.  Over them, set-up and tail only:
// in-arc offsets (4 per state) + sources (2 per arc) + the trace-back's 9 rows.
static size_t k2_lds_chain(size_t S, size_t A, size_t max_npdf, int odeg) {
  const size_t S4 = (S + 3) & ~size_t(3);
  return std::max<size_t>(36 * S4 + 21 * S4 * (size_t)odeg + 4 * max_npdf, 4 * (S4 + 1) + 2 * A + 16 + 9 * ((S + 15) & ~size_t(15))) + 128;
}

// ------------------------------------------------------------------------------------------
// The ONE dispatch rule of khg_align: which instantiation of k2_viterbi_dp runs a set under the context's current options, its block
// size and dynamic LDS, and which order-faithful decoder follows for what the DP cannot certify, with its LDS and arguments.
// khg_align launches what this says and computes nothing about a launch itself; khg_utts_k2_plan hands the same answer to a test
// (nothing is launched or allocated here).
struct K2Plan {
  int KS = 1, DEG = 1;                       // k2_viterbi_dp<KS, DEG, FAST, GMEM, SC>
  bool FAST = false, GMEM = false, SC = false;
  bool LAD = false;                          // the ladder form of <1, 2, true, false, *> (an inner choice: same tables, same LDS, same block)
  int nthr = 64;
  size_t dp_bytes = 0, lds_dp = 0;           // the DP's tables; its dynamic LDS: the same, or (GMEM) 0 -- the tables are its slice of the HBM scratch
  size_t max_npdf = 0;
  int faithful = 0;                          // 0 one-lane LDS, 1 one-lane HBM, 2 wave LDS, 3 wave HBM, 4 chain
  size_t lds_faithful = 0;                   // ... and its dynamic LDS
  int odeg_c = 1, odeg_w = 0;                // the chain form's ODEG, in 1..4; the wave form's arguments
  bool has_eps = false;
  size_t gscratch_stride = 0;                // HBM scratch per utterance (0: none needed)
};

static K2Plan k2_plan(const khg_ctx* ctx, const khg_utts* u) {
  K2Plan p;
  const size_t S = (size_t)u->max_states, A = (size_t)u->max_inarcs;
  size_t max_npdf = 0;
  for (int i = 0; i < u->n_utt; ++i) max_npdf = std::max<size_t>(max_npdf, (size_t)(u->pdf_off[i + 1] - u->pdf_off[i]));
  p.max_npdf = max_npdf;
  // threads: one destination state each (up to 1024), KS states per thread beyond that
  int nthr = (int)std::min<size_t>(1024, (S + 63) / 64 * 64);
  const int ks_force = ctx->opt[KHG_OPT_K2_KS];   // experiment: states per thread on the register-resident path
  if (ks_force == 2 || ks_force == 4) nthr = (int)std::min<size_t>(1024, ((S + ks_force - 1) / ks_force + 63) / 64 * 64);
  p.nthr = nthr;
  const size_t nwave = nthr / 64;
  // register-resident path for the whole batch: in-degree <= 3 (up to 4 states per thread) or <= 6 (one state per thread)
  const bool deg6 = !u->has_eps && u->max_indeg > 3 && u->max_indeg <= 6 && S <= 1024;
  const bool fast = deg6 || (!u->has_eps && u->max_indeg <= 3 && S <= 4096);
  const int KSsel = !fast ? 0 : ((ks_force == 2 || ks_force == 4) && !deg6 && S <= (size_t)1024 * ks_force ? ks_force : (S <= 1024 ? 1 : (S <= 2048 ? 2 : 4)));
  const size_t lds_dp = fast ? k2_lds_dp_fast(S, A, (size_t)nthr, (size_t)KSsel) : k2_lds_dp_generic(S, A, nwave, max_npdf);
  // The order-faithful decoder for the utterances the DP cannot certify: the wave-parallel form with all its tables in LDS; with the
  // graph tables in an HBM scratch slice per utterance (> ~1600 states on a chain graph); the one-lane form beyond that.
  // KHG_K2_SERIAL = 1: always the one-lane form; 2: the HBM-graph wave form wherever its per-frame tables fit (tests, A/B).
  const size_t lds_f = k2_lds_lane(S, A);
  const int odeg_w = u->max_outdeg <= 8 ? std::max(1, (int)u->max_outdeg) : 0;     // 0: exact slot prefix sums
  const bool use_pos = u->has_eps || S > 1000;
  const size_t lds_w_mut = k2_lds_wave_mut(S, A, max_npdf, odeg_w, use_pos, u->has_eps), lds_w_graph = k2_lds_wave_graph(S, A, u->has_eps);
  const int fmode = ctx->opt[KHG_OPT_K2_SERIAL];
  // The chain form (k2_viterbi_faithful_chain: no epsilon-input arcs, <= 1000 states, out-degree <= 4 -- a linear transcript's training
  // graph): a third of the wave form's latency per frame.  KHG_K2_SERIAL = 3: the general wave form also where the chain form applies.
  const int odeg_c = (int)std::min<int32_t>(4, std::max<int32_t>(1, u->max_outdeg));     // (past 4 there is no chain form)
  const size_t lds_chain = k2_lds_chain(S, A, max_npdf, odeg_c);
  const bool chain = fmode == 0 && !u->has_eps && S <= 1000 && u->max_outdeg <= 4 && lds_chain <= 64 * 1024 && max_npdf <= 32767;
  const bool wave_lds = (fmode == 0 || fmode == 3) && S <= 65535 && lds_w_mut + lds_w_graph <= 160 * 1024;
  const bool wave_gm = fmode != 1 && !wave_lds && S <= 65535 && lds_w_mut <= 160 * 1024;
  const bool lane_gm = !wave_lds && !wave_gm && lds_f > 160 * 1024;
  p.faithful = chain ? 4 : wave_gm ? 3 : wave_lds ? 2 : lane_gm ? 1 : 0;
  p.lds_faithful = chain ? lds_chain : wave_gm ? lds_w_mut : wave_lds ? lds_w_mut + lds_w_graph : lane_gm ? 0 : lds_f;
  p.odeg_c = odeg_c; p.odeg_w = odeg_w; p.has_eps = u->has_eps;
  // Graphs whose DP tables exceed the 160 KB of LDS (a large decoding graph, not a training graph): the generic DP runs with its
  // tables carved out of the same HBM scratch slice.
  const bool gmem = lds_dp > 160 * 1024;
  p.dp_bytes = gmem ? k2_lds_dp_generic(S, A, nwave, max_npdf) : lds_dp;     // (the generic DP's carve-up: no register-resident path)
  p.lds_dp = gmem ? 0 : p.dp_bytes;
  if (gmem || wave_gm || lane_gm)
    p.gscratch_stride = (std::max(gmem ? p.dp_bytes : 0, std::max(wave_gm ? lds_w_graph : 0, lane_gm ? lds_f : 0)) + 255) & ~size_t(255);
  if (gmem) { p.GMEM = true; return p; }     // <1, 1, false, true>
  // in-degree <= 2 (a linear transcript's chain of HMM states: self-loop + forward arc): the two-slot instantiation, a sixth fewer
  // instructions per layer than the three-slot one (the layer loop is bound by VALU issue; every slot is evaluated, empty or not)
  const bool deg2 = fast && !deg6 && KSsel == 1 && u->max_indeg <= 2 && ctx->opt[KHG_OPT_K2_KS] != 3;
  // (KHG_K2_KS = 3: the general three-slot kernel, for the A/B)
  const bool sc2 = deg2 && u->same_col;     // ... and one score row per state: one score block / cost conversion per state
  const bool sc3 = fast && !deg6 && !deg2 && KSsel == 1 && u->same_col && ctx->opt[KHG_OPT_K2_KS] != 3;   // three slots, one score row per state
  // Two / four states per thread (graphs of more than 1024 / 2048 states): a block of 1024 threads leaves 128 registers per lane;
  // the three-slot form needs ~180 at two states per thread (84 registers spilled at the one-state kernels' budget of 96: a
  // transcript of > 340 phones ran 9x slower per frame than one of 330), the two-slot forms of chain graphs fit (round 4)
  const bool deg2m = fast && !deg6 && KSsel > 1 && u->max_indeg <= 2;
  auto form = [&](int ks, int deg, bool sc) { p.KS = ks; p.DEG = deg; p.FAST = true; p.SC = sc; };
  if (deg6) form(1, 6, false);
  else if (sc2) form(1, 2, true);
  else if (deg2) form(1, 2, false);
  else if (sc3) form(1, 3, true);
  else if (KSsel == 1) form(1, 3, false);
  else if (KSsel == 2 && deg2m && u->same_col) form(2, 2, true);
  else if (KSsel == 2 && deg2m) form(2, 2, false);
  else if (KSsel == 2) form(2, 3, false);
  else if (KSsel == 4 && deg2m && u->same_col) form(4, 2, true);
  else if (KSsel == 4 && deg2m) form(4, 2, false);
  else if (KSsel == 4) form(4, 3, false);
  // else: the generic LDS form <1, 1, false>
  // The ladder form of the two-slot, one-state-per-thread kernels: every graph of the batch in chain order (khg_utts::ladder) and at
  // most four waves.  KHG_K2_LADDER = off: the general body (A/B, tests).
  p.LAD = p.FAST && p.KS == 1 && p.DEG == 2 && u->ladder && nthr <= 256 && ctx->opt[KHG_OPT_K2_LADDER] == 0;
  return p;
}

extern "C" int khg_utts_k2_plan(khg_ctx* ctx, const khg_utts* u, int32_t out[8]) {
  if (ctx_dead(ctx) || !u || !out) return khg_set_error(KHG_E_ARG, "khg_utts_k2_plan: bad arguments");
  { int rf = utts_foreign_ctx(ctx, u, "khg_utts_k2_plan"); if (rf) return rf; }
  if (!u->has_graphs) return khg_set_error(KHG_E_ARG, "khg_utts_k2_plan: the utterance set has no decoding graphs");
  const K2Plan p = k2_plan(ctx, u);
  out[0] = p.KS; out[1] = p.DEG; out[2] = p.FAST ? 1 : 0; out[3] = p.GMEM ? 1 : 0; out[4] = p.SC ? 1 : 0;
  out[5] = p.nthr; out[6] = (int32_t)p.lds_dp; out[7] = p.faithful;
  return KHG_OK;
}

// Beside the plan: whether khg_align would run the ladder form of the kernel the plan names (1) or its general body (0).
extern "C" int khg_utts_k2_ladder(khg_ctx* ctx, const khg_utts* u, int32_t* out) {
  if (ctx_dead(ctx) || !u || !out) return khg_set_error(KHG_E_ARG, "khg_utts_k2_ladder: bad arguments");
  { int rf = utts_foreign_ctx(ctx, u, "khg_utts_k2_ladder"); if (rf) return rf; }
  if (!u->has_graphs) return khg_set_error(KHG_E_ARG, "khg_utts_k2_ladder: the utterance set has no decoding graphs");
  *out = k2_plan(ctx, u).LAD ? 1 : 0;
  return KHG_OK;
}

extern "C" int khg_utts_k2_tail(const khg_utts* u, int32_t* out, int64_t cap) {
  if (!u || !out) return khg_set_error(KHG_E_ARG, "khg_utts_k2_tail: bad arguments");
  if (u->k2_tail.empty()) return khg_set_error(KHG_E_ARG, "khg_utts_k2_tail: no khg_align under KHG_OPT_K2_PROF on this set yet");
  if (cap < (int64_t)u->k2_tail.size()) return khg_set_error(KHG_E_ARG, "khg_utts_k2_tail: cap too small");
  std::copy(u->k2_tail.begin(), u->k2_tail.end(), out);
  return KHG_OK;
}

// ------------------------------------------------------------------------------------------
// Every instantiation of K2's kernels, once -- k2_insts, one typed array per kernel signature: (KS of the DP or ODEG of the chain
// decoder, DEG, SC, LAD, GMEM) -> the kernel.  The DP's FAST is DEG > 1: <1, 1, false> is the generic form.
typedef void (*K2DpFn)(K2Args);                       // k2_viterbi_dp, and the one-lane k2_viterbi_faithful
typedef void (*K2WaveFn)(K2Args, int, int, int);      // has_eps, odeg_w, max_npdf
typedef void (*K2ChainFn)(K2Args, int);               // max_npdf
template <class Fn> struct K2Inst { int K, DEG; bool SC, LAD, GMEM; Fn fn; };
static const K2Inst<K2DpFn> k2_insts_dp[] = {
  {1, 1, false, false, false, k2_viterbi_dp<1, 1, false>},              {1, 1, false, false, true, k2_viterbi_dp<1, 1, false, true>},
  {1, 2, true, true, false, k2_viterbi_dp<1, 2, true, false, true, true>}, {1, 2, false, true, false, k2_viterbi_dp<1, 2, true, false, false, true>},
  {1, 2, true, false, false, k2_viterbi_dp<1, 2, true, false, true>},   {1, 2, false, false, false, k2_viterbi_dp<1, 2, true>},
  {1, 3, true, false, false, k2_viterbi_dp<1, 3, true, false, true>},   {1, 3, false, false, false, k2_viterbi_dp<1, 3, true>},
  {1, 6, false, false, false, k2_viterbi_dp<1, 6, true>},
  {2, 2, true, false, false, k2_viterbi_dp<2, 2, true, false, true>},   {2, 2, false, false, false, k2_viterbi_dp<2, 2, true>},
  {2, 3, false, false, false, k2_viterbi_dp<2, 3, true>},
  {4, 2, true, false, false, k2_viterbi_dp<4, 2, true, false, true>},   {4, 2, false, false, false, k2_viterbi_dp<4, 2, true>},
  {4, 3, false, false, false, k2_viterbi_dp<4, 3, true>},
};
static const K2Inst<K2DpFn> k2_insts_lane[] = {{0, 0, false, false, false, k2_viterbi_faithful<false>}, {0, 0, false, false, true, k2_viterbi_faithful<true>}};
static const K2Inst<K2WaveFn> k2_insts_wave[] = {{0, 0, false, false, false, k2_viterbi_faithful_wave<false>}, {0, 0, false, false, true, k2_viterbi_faithful_wave<true>}};
static const K2Inst<K2ChainFn> k2_insts_chain[] = {{1, 0, false, false, false, k2_viterbi_faithful_chain<1>}, {2, 0, false, false, false, k2_viterbi_faithful_chain<2>},
                                                   {3, 0, false, false, false, k2_viterbi_faithful_chain<3>}, {4, 0, false, false, false, k2_viterbi_faithful_chain<4>}};
static_assert(sizeof(k2_insts_dp) / sizeof(k2_insts_dp[0]) == 15 && sizeof(k2_insts_chain) / sizeof(k2_insts_chain[0]) == 4, "k2_insts: 15 DP forms, 2 one-lane, 2 wave and 4 chain decoders");
// A plan the table has no row for is an error that names the form -- never another form's kernel under this one's block and LDS.
template <class Fn, size_t N>
static int k2_find(Fn* fn, const K2Inst<Fn> (&insts)[N], const char* kernel, int K, int DEG, bool SC, bool LAD, bool GMEM) {
  for (const K2Inst<Fn>& i : insts)
    if (i.K == K && i.DEG == DEG && i.SC == SC && i.LAD == LAD && i.GMEM == GMEM) { *fn = i.fn; return KHG_OK; }
  return khg_set_error(KHG_E_UNSUPPORTED, std::string("khg_align: no ") + kernel + " kernel was built for the form (K " + std::to_string(K) + ", DEG " + std::to_string(DEG) +
                                          ", SC " + std::to_string(SC) + ", LAD " + std::to_string(LAD) + ", GMEM " + std::to_string(GMEM) + ")");
}
// the two kernels of a plan: the DP, and the one order-faithful decoder K2Plan::faithful names (the other two stay null)
struct K2Kernels { K2DpFn dp = nullptr, lane = nullptr; K2WaveFn wave = nullptr; K2ChainFn chain = nullptr; };
static int k2_kernels(const K2Plan& p, K2Kernels* k) {
  int rc = k2_find(&k->dp, k2_insts_dp, "k2_viterbi_dp", p.KS, p.DEG, p.SC, p.LAD, p.GMEM);
  if (rc) return rc;
  const bool gmem = p.faithful == 1 || p.faithful == 3;
  if (p.faithful == 4) return k2_find(&k->chain, k2_insts_chain, "k2_viterbi_faithful_chain", p.odeg_c, 0, false, false, false);
  if (p.faithful >= 2) return k2_find(&k->wave, k2_insts_wave, "k2_viterbi_faithful_wave", 0, 0, false, false, gmem);
  return k2_find(&k->lane, k2_insts_lane, "k2_viterbi_faithful", 0, 0, false, false, gmem);
}
// ... and the one launch of them, one workgroup per utterance, under the timer `name` on the launching stream
template <class... Params, class... Args>
static int k2_launch(khg_ctx* ctx, const char* name, void (*fn)(Params...), int grid, int nthr, size_t lds, hipStream_t s, const Args&... args) {
  if (!fn) return khg_set_error(KHG_E_UNSUPPORTED, "khg_align: no kernel of this form was built");
  int rc = khg_lds_attribute((const void*)fn, lds);
  if (rc) return rc;
  {
    KernelTimer kt(ctx, name, s);
    KHG_LAUNCH(ctx, fn, dim3(grid), dim3(nthr), lds, s, args...);
  }
  HIPCHK(hipGetLastError());
  return KHG_OK;
}

// ------------------------------------------------------------------------------------------
// khg_align, step by step, in the order the work is enqueued.
static int k2_check(khg_ctx* ctx, const khg_tm* tm, const khg_utts* u, const khg_align_config* cfg) {
  if (ctx_dead(ctx) || !tm || !u || !cfg) return khg_set_error(KHG_E_ARG, "khg_align: bad arguments");
  { int rf = utts_foreign_ctx(ctx, u, "khg_align"); if (rf) return rf; }
  if (!u->has_graphs) return khg_set_error(KHG_E_ARG, "khg_align: the utterance set has no decoding graphs");
  if (!u->ll_valid) return khg_set_error(KHG_E_ARG, "khg_align: call khg_loglikes first");
  // the exact DP's back-pointers are one byte and its arc sources 16 bits: khg_utts_create refuses such graphs, a khg_graph may hold one
  // (the lattice decoders have neither field).  Nothing was touched: the set stays usable.
  if (u->max_states > 65535)
    return khg_set_error(KHG_E_UNSUPPORTED, "khg_align: more than 65535 states in one decoding graph (" + std::to_string(u->max_states) + "); the aligner's limit");
  if (u->max_indeg > 254)
    return khg_set_error(KHG_E_UNSUPPORTED, "khg_align: a state has more than 254 incoming arcs (" + std::to_string(u->max_indeg) + "); the aligner's limit");
  // decoder-wrappers.cc:29-33
  if ((cfg->retry_beam != 0 && cfg->retry_beam <= cfg->beam) || cfg->beam <= 0.0)
    return khg_set_error(KHG_E_RUNTIME, "Beams do not make sense: beam " + std::to_string(cfg->beam) + ", retry-beam " + std::to_string(cfg->retry_beam));
  // faster-decoder.cc:24-27
  if (!(cfg->hash_ratio >= 1.0) || !(cfg->max_active > 1) || !(cfg->min_active >= 0 && cfg->min_active < cfg->max_active))
    return khg_set_error(KHG_E_RUNTIME, "FasterDecoderOptions assertion failed");
  return KHG_OK;
}

// Scratch, each group allocated on the set's first call that needs it.  The DP's back-pointers, layer certificates and paths; with
// them, where ensure_ali made no out block, the four separate output arrays
static int k2_dp_scratch(khg_utts* u) {
  if (u->bp_d) return KHG_OK;
  int rc = u_alloc(u, &u->bp_d, (size_t)u->bp_off[u->n_utt]);
  if (!rc) rc = u_alloc(u, &u->layer_best_d, (size_t)(u->N + u->n_utt));
  if (!rc) rc = u_alloc(u, &u->layer_cnt_d, (size_t)(u->N + u->n_utt));
  if (!rc) rc = u_alloc(u, &u->path_d, (size_t)u->path_off[u->n_utt]);
  if (!rc && !u->out_blk_d) {
    rc = u_alloc(u, &u->words_d, (size_t)u->words_off[u->n_utt]);
    if (!rc) rc = u_alloc(u, &u->num_words_d, (size_t)u->n_utt);
    if (!rc) rc = u_alloc(u, &u->status_d, (size_t)u->n_utt);
    if (!rc) rc = u_alloc(u, &u->like_d, (size_t)u->n_utt);
  }
  return rc;
}
// launch order of the DP kernel: longest utterances first (built once per set)
static int k2_launch_order(khg_ctx* ctx, khg_utts* u) {
  if (u->k2_order_d || u->n_utt <= 1) return KHG_OK;
  std::vector<int32_t> ord((size_t)u->n_utt);
  for (int i = 0; i < u->n_utt; ++i) ord[(size_t)i] = i;
  std::stable_sort(ord.begin(), ord.end(), [&](int32_t x, int32_t y) {
    return u->frame_off[x + 1] - u->frame_off[x] > u->frame_off[y + 1] - u->frame_off[y];
  });
  int rc = u_upload(ctx, u, &u->k2_order_d, ord);
  if (!rc) rc = sync_pageable(ctx);
  return rc;
}
// Split mode: nobody waits for the results here and the set is large -- the order-faithful decoders (side stream) write to ali2_d, the DP
// kernel leaves an uncertified utterance's range of ali_d zero, flags and counts it: khg_acc_stats can then accumulate the certified
// utterances while those decoders still run (khg_k3.hip); wait_ali merges.
static int k2_split_buffers(khg_ctx* ctx, khg_utts* u) {
  if (!u->ali2_d) {
    int rc = u_alloc(u, &u->ali2_d, (size_t)u->N);
    if (!rc) rc = u_alloc(u, &u->unc_d, (size_t)u->n_utt + 2);       // flags | [utterances, frames] the DP could not certify
    if (rc) return rc;
    u->unc_cnt_dev = u->unc_d + u->n_utt;
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&u->unc_cnt_h), 64, 0));   // pinned landing place of the two counters
  }
  HIPCHK(hipMemsetAsync(u->unc_d, 0, sizeof(int32_t) * ((size_t)u->n_utt + 2), ctx->stream));
  return KHG_OK;
}
// the HBM scratch of the forms whose tables do not fit LDS: one slice per utterance, grown on demand
static int k2_gscratch(khg_utts* u, const K2Plan& plan) {
  const size_t need = plan.gscratch_stride * (size_t)u->n_utt;
  if (need <= u->k2_gscratch_bytes) return KHG_OK;
  DEVFREE(u->k2_gscratch_d);
  int rc = u_alloc(u, &u->k2_gscratch_d, need);
  if (rc) return rc;
  u->k2_gscratch_bytes = need;
  return KHG_OK;
}

// KHG_OPT_K2_PROF, diagnostics: [U][8] DP stamps | [U][8] chain-decoder stamps, zeroed before the launches ...
static int k2_prof_begin(const khg_ctx* ctx, const khg_utts* u, long long** prof) {
  *prof = nullptr;
  if (ctx->opt[KHG_OPT_K2_PROF] == 0) return KHG_OK;
  HIPCHK(hipMalloc(reinterpret_cast<void**>(prof), sizeof(long long) * 16 * (size_t)u->n_utt));
  HIPCHK(hipMemset(*prof, 0, sizeof(long long) * 16 * (size_t)u->n_utt));
  return KHG_OK;
}
// ... and read behind them: average s_memtime ticks per phase of k2_viterbi_dp and of the chain decoder, and khg_utts::k2_tail
static int k2_prof_report(khg_ctx* ctx, khg_utts* u, const K2Plan& plan, long long* prof, hipStream_t side) {
  std::vector<long long> pr(16 * (size_t)u->n_utt);
  HIPCHK(hipStreamSynchronize(ctx->stream));
  HIPCHK(hipStreamSynchronize(side));
  HIPCHK(hipMemcpy(pr.data(), prof, pr.size() * 8, hipMemcpyDeviceToHost));
  (void)hipFree(prof);
  double ph[4] = {0, 0, 0, 0}, sT = 0, sS = 0, sf = 0; int n = 0;
  for (int i = 0; i < u->n_utt; ++i) if (pr[i * 8 + 4]) { for (int k = 0; k < 4; ++k) ph[k] += (double)(pr[i * 8 + k + 1] - pr[i * 8 + k]); sT += pr[i * 8 + 5]; sS += pr[i * 8 + 6]; sf += (double)(pr[i * 8 + 7] & 0xff); ++n; }
  // word 7: FAST | replay batches whose cost chain was scanned << 8 | those that took the serial loop << 32 (KHG_OPT_K2_TAIL)
  u->k2_tail.assign(2 * (size_t)u->n_utt, 0);
  long long bs = 0, bl = 0;
  for (int i = 0; i < u->n_utt; ++i) {
    u->k2_tail[2 * (size_t)i] = (int32_t)((pr[i * 8 + 7] >> 8) & 0xffffff); u->k2_tail[2 * (size_t)i + 1] = (int32_t)(pr[i * 8 + 7] >> 32);
    bs += u->k2_tail[2 * (size_t)i]; bl += u->k2_tail[2 * (size_t)i + 1];
  }
  if (n) fprintf(stderr, "[KHG_K2_PROF] %d utts, avg T %.1f S %.1f fast %.2f threads %d lds %zu | ticks: setup %.0f forward %.0f traceback %.0f replay %.0f | replay batches: %lld scanned, %lld serial\n",
                 n, sT / n, sS / n, sf / n, plan.nthr, plan.dp_bytes, ph[0] / n, ph[1] / n, ph[2] / n, ph[3] / n, bs, bl);
  const long long* pc = pr.data() + 8 * (size_t)u->n_utt;     // chain decoder: 0 start, 1 set-up done, 2 frames done (all attempts), 3 finished, 4 frames decoded
  double cs[3] = {0, 0, 0}, cf = 0, cp[3] = {0, 0, 0}; int nc = 0;
  for (int i = 0; i < u->n_utt; ++i) if (pc[i * 8 + 3]) { for (int k = 0; k < 3; ++k) { cs[k] += (double)(pc[i * 8 + k + 1] - pc[i * 8 + k]); cp[k] += (double)pc[i * 8 + 5 + k]; } cf += (double)pc[i * 8 + 4]; ++nc; }
  if (nc) fprintf(stderr, "[KHG_K2_PROF] chain decoder: %d utts, avg frames decoded %.1f | ticks: setup %.0f frames %.0f (%.1f per frame: GetCutoff %.1f, pass 1 %.1f, pass 2 %.1f, rest = row flush + score staging) finish %.0f\n",
                  nc, cf / nc, cs[0] / nc, cs[1] / nc, cs[1] / std::max(1.0, cf), cp[0] / std::max(1.0, cf), cp[1] / std::max(1.0, cf), cp[2] / std::max(1.0, cf), cs[2] / nc);
  return KHG_OK;
}

// the kernels' arguments, from the set, the transition table, the config and the plan (every scratch group is in place)
static K2Args k2_args(const khg_ctx* ctx, const khg_tm* tm, const khg_utts* u, const khg_align_config* cfg, const K2Plan& plan, bool split, long long* prof) {
  K2Args a;
  a.frame_off = u->frame_off_d; a.gidx = u->gidx_d; a.state_off = u->state_off_d; a.start = u->start_d;
  a.in_off = u->in_off_d; a.in_src = u->in_src_d; a.in_col = u->in_col_d; a.in_tid = u->in_tid_d;
  a.in_olabel = u->in_olabel_d; a.in_w = u->in_w_d; a.out_off = u->out_off_d; a.out_inidx = u->out_inidx_d;
  a.final_w = u->final_d; a.trans_cost = tm->has_trans_cost ? tm->trans_cost_d : nullptr;
  a.ll = u->ll_d; a.ll_off = u->ll_off_d;
  a.bp = u->bp_d; a.bp_off = u->bp_off_d; a.layer_best = u->layer_best_d; a.layer_cnt = u->layer_cnt_d;
  a.path = u->path_d; a.path_off = u->path_off_d;
  a.ali = u->ali_d; a.words = u->words_d; a.words_off = u->words_off_d; a.num_words = u->num_words_d;
  a.ali_fb = split ? u->ali2_d : u->ali_d; a.unc = split ? u->unc_d : nullptr; a.unc_cnt = split ? u->unc_cnt_dev : nullptr;
  a.like = u->like_d; a.status = u->status_d; a.err_flag = ctx->err_flag_d;
  a.prof = prof;
  a.tail_off = ctx->opt[KHG_OPT_K2_TAIL];
  a.order = ctx->opt[KHG_OPT_K2_INORDER] ? nullptr : u->k2_order_d;
  a.beam = cfg->beam; a.retry_beam = cfg->retry_beam; a.acoustic_scale = cfg->acoustic_scale;
  a.like_scale = cfg->like_scale != 0.0f ? cfg->like_scale : cfg->acoustic_scale;
  a.beam_delta = cfg->beam_delta; a.hash_ratio = cfg->hash_ratio;
  a.max_active = cfg->max_active; a.min_active = cfg->min_active;
  a.max_states = u->max_states; a.max_inarcs = u->max_inarcs;
  a.gscratch = plan.gscratch_stride ? u->k2_gscratch_d : nullptr; a.gscratch_stride = (int64_t)plan.gscratch_stride;
  return a;
}

// The order-faithful decoder for what the DP could not certify runs on a side stream, beside the main stream's next K1: the side
// stream waits for the DP (ev_dp); in split mode the two counters khg_acc_stats reads behind ev_dp are copied ahead of it.
static int k2_side_stream(khg_ctx* ctx, khg_utts* u, bool split, hipStream_t* side) {
  if (!u->ev_dp) { HIPCHK(hipEventCreateWithFlags(&u->ev_dp, hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&u->ev_ali, hipEventDisableTiming)); }
  if (split) HIPCHK(hipMemcpyAsync(u->unc_cnt_h, u->unc_cnt_dev, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));   // read by khg_acc_stats behind ev_dp
  HIPCHK(hipEventRecord(u->ev_dp, ctx->stream));
  *side = ctx->sides[ctx->next_side];
  ctx->side_dirty[ctx->next_side] = true;
  ctx->next_side = (ctx->next_side + 1) % khg_ctx::NSIDE;
  HIPCHK(hipStreamWaitEvent(*side, u->ev_dp, 0));
  return KHG_OK;
}
// the plan's order-faithful decoder, one wave per utterance; the signature picks the argument list
static int k2_run_faithful(khg_ctx* ctx, const khg_utts* u, const K2Plan& plan, const K2Kernels& k, const K2Args& a, hipStream_t side) {
  static const char* const name = "k2_viterbi_faithful";
  const int U = u->n_utt, maxp = (int)plan.max_npdf;
  if (k.chain) return k2_launch(ctx, name, k.chain, U, 64, plan.lds_faithful, side, a, maxp);
  if (k.wave) return k2_launch(ctx, name, k.wave, U, 64, plan.lds_faithful, side, a, plan.has_eps ? 1 : 0, plan.odeg_w, maxp);
  return k2_launch(ctx, name, k.lane, U, 64, plan.lds_faithful, side, a);
}

// The download of a call with host outputs.  words_h, packed: utterance i's words behind utterance i - 1's, words_off_h their bounds;
// nw / w: the device's counts and its words at the set's own offsets
static int k2_pack_words(const khg_utts* u, const int32_t* nw, const int32_t* w, int32_t* words_h, int64_t* words_off_h, int64_t words_cap) {
  int64_t o = 0;
  for (int i = 0; i < u->n_utt; ++i) {
    words_off_h[i] = o;
    const int64_t n = std::min<int64_t>(nw[i], u->words_off[i + 1] - u->words_off[i]);
    if (o + n > words_cap) return khg_set_error(KHG_E_ARG, "khg_align: words_cap too small");
    std::copy(w + u->words_off[i], w + u->words_off[i] + n, words_h + o);
    o += n;
  }
  words_off_h[u->n_utt] = o;
  return KHG_OK;
}
static int k2_download(khg_ctx* ctx, khg_utts* u, int32_t* ali_h, int32_t* words_h, int64_t* words_off_h, int64_t words_cap, float* like_h, int32_t* status_h) {
  int rc = wait_ali(ctx, u);
  if (rc) return rc;
  if (u->out_blk_d && ctx->arena.owns(u->out_blk_d)) {
    // one block, one copy into its pinned mirror; the error word's own copy and wait follow it on the stream
    char* hm = ctx->arena.mirror(u->out_blk_d);
    HIPCHK(hipMemcpyAsync(hm, u->out_blk_d, u->out_blk_bytes, hipMemcpyDeviceToHost, ctx->stream));
    rc = check_err_flag(ctx, "khg_align");  // synchronises
    if (rc) return rc;
    const size_t nu = (size_t)u->n_utt, nwt = (size_t)u->words_off[u->n_utt];
    const int32_t* hp = reinterpret_cast<const int32_t*>(hm);
    if (status_h) memcpy(status_h, hp, 4 * nu);
    if (like_h) memcpy(like_h, hp + nu, 4 * nu);
    if (ali_h && u->N) memcpy(ali_h, hp + 3 * nu + nwt, 4 * (size_t)u->N);
    return words_h && words_off_h ? k2_pack_words(u, hp + 2 * nu, hp + 3 * nu, words_h, words_off_h, words_cap) : KHG_OK;
  }
  rc = check_err_flag(ctx, "khg_align");  // synchronises
  if (rc) return rc;
  if (ali_h) HIPCHK(hipMemcpyAsync(ali_h, u->ali_d, sizeof(int32_t) * (size_t)u->N, hipMemcpyDeviceToHost, ctx->stream));
  if (like_h) HIPCHK(hipMemcpyAsync(like_h, u->like_d, sizeof(float) * (size_t)u->n_utt, hipMemcpyDeviceToHost, ctx->stream));
  if (status_h) HIPCHK(hipMemcpyAsync(status_h, u->status_d, sizeof(int32_t) * (size_t)u->n_utt, hipMemcpyDeviceToHost, ctx->stream));
  if (words_h && words_off_h) {
    std::vector<int32_t> w((size_t)u->words_off[u->n_utt]), nw((size_t)u->n_utt);
    if (!w.empty()) HIPCHK(hipMemcpyAsync(w.data(), u->words_d, sizeof(int32_t) * w.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(nw.data(), u->num_words_d, sizeof(int32_t) * nw.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    rc = k2_pack_words(u, nw.data(), w.data(), words_h, words_off_h, words_cap);
    if (rc) return rc;
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return KHG_OK;
}

extern "C" int khg_align(khg_ctx* ctx, const khg_tm* tm, khg_utts* u, const khg_align_config* cfg,
                         int32_t* ali_h, int32_t* words_h, int64_t* words_off_h, int64_t words_cap,
                         float* like_h, int32_t* status_h) {
  int rc = k2_check(ctx, tm, u, cfg);
  if (rc) return rc;
  // Host outputs: the caller waits for the results right here, nothing can overlap the order-faithful decoder, and it follows the DP
  // on the main stream without the two cross-stream events (the per-utterance call pattern: ~30 us of a ~300 us call).  Without
  // them and on a large set: split mode (k2_split_buffers).
  const bool sync_call = ali_h || like_h || status_h || words_h;
  const bool split = !sync_call && u->n_utt > 64 && !u->small && ctx->opt[KHG_OPT_K2_SPLIT] == 0;
  const K2Plan plan = k2_plan(ctx, u);
  K2Kernels k;                                    // the plan's two rows of k2_insts: nothing is enqueued for a plan without them
  long long* prof = nullptr;
  if ((rc = k2_kernels(plan, &k))) return rc;
  if ((rc = wait_ali(ctx, u))) return rc;
  if ((rc = k1_band_check(ctx, u))) return rc;      // BAND scores: their model must be alive and unchanged (khg_k1.hip)
  if ((rc = ensure_ali(ctx, u)) || (rc = k2_dp_scratch(u))) return rc;
  if ((rc = arena_flush(ctx))) return rc;            // an alignment staged by khg_ali_upload must not land on top of the cleared block
  HIPCHK(hipMemsetAsync(u->ali_d, 0, sizeof(int32_t) * (size_t)u->N, ctx->stream));
  if ((rc = k2_launch_order(ctx, u)) || (split && (rc = k2_split_buffers(ctx, u)))) return rc;
  if ((rc = k2_prof_begin(ctx, u, &prof)) || (rc = k2_gscratch(u, plan))) return rc;
  const K2Args a = k2_args(ctx, tm, u, cfg, plan, split, prof);
  if ((rc = k2_launch(ctx, "k2_viterbi_dp", k.dp, u->n_utt, plan.nthr, plan.lds_dp, ctx->stream, a))) return rc;
  hipStream_t side = ctx->stream;
  if (!sync_call && (rc = k2_side_stream(ctx, u, split, &side))) return rc;
  if ((rc = k1_band_repair(ctx, u, u->status_d, K2_ST_NEED_FALLBACK, side))) return rc;      // khg_k1.hip (BAND form of K1 only)
  if ((rc = k2_run_faithful(ctx, u, plan, k, a, side))) return rc;
  if (!sync_call) { HIPCHK(hipEventRecord(u->ev_ali, side)); u->ali_pending = true; }
  u->ali_split = split;
  u->ali_valid = true;
  if (prof && (rc = k2_prof_report(ctx, u, plan, prof, side))) return rc;
  if (!sync_call) return KHG_OK;   // asynchronous: errors surface at khg_ctx_sync / downloads
  return k2_download(ctx, u, ali_h, words_h, words_off_h, words_cap, like_h, status_h);
}

extern "C" int khg_ali_upload(khg_ctx* ctx, khg_utts* u, const int32_t* ali) {
  if (ctx_dead(ctx) || !u || !ali) return khg_set_error(KHG_E_ARG, "bad arguments");
  { int rf = utts_foreign_ctx(ctx, u, "khg_ali_upload"); if (rf) return rf; }
  int rc = wait_ali(ctx, u);
  if (!rc) rc = ensure_ali(ctx, u);
  if (rc) return rc;
  if (ctx->arena.owns(u->ali_d)) {          // staged: goes out with the next launch's flush
    if (u->N) { memcpy(ctx->arena.mirror(u->ali_d), ali, sizeof(int32_t) * (size_t)u->N); arena_mark_dirty(ctx, u->ali_d, sizeof(int32_t) * (size_t)u->N); }
  } else {
    HIPCHK(hipMemcpyAsync(u->ali_d, ali, sizeof(int32_t) * (size_t)u->N, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  u->ali_valid = true;
  return KHG_OK;
}

extern "C" int khg_ali_download(khg_ctx* ctx, khg_utts* u, int32_t* ali) {
  if (ctx_dead(ctx) || !u || !ali) return khg_set_error(KHG_E_ARG, "bad arguments");
  if (!u->ali_valid) return khg_set_error(KHG_E_ARG, "khg_ali_download: no resident alignment");
  { int rf = utts_foreign_ctx(ctx, u, "khg_ali_download"); if (rf) return rf; }
  int rc = wait_ali(ctx, u);
  if (!rc) rc = arena_flush(ctx);           // small sets: an uploaded alignment may still be staged in the pinned mirror
  if (!rc) rc = check_err_flag(ctx, "khg_align");
  if (rc) return rc;
  if (u->N) HIPCHK(hipMemcpyAsync(ali, u->ali_d, sizeof(int32_t) * (size_t)u->N, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return KHG_OK;
}
