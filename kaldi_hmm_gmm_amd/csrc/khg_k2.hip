// kaldi_hmm_gmm_amd/csrc/khg_k2.hip -- C-ABI (include/khg_hip.h): K2, Viterbi forced alignment (khg_align): kernel selection by graph
// shape, LDS budgets, the exact DP on the main stream and the order-faithful decoder on a side stream; and the lattice decoder
// (khg_decode_lattice_faster, khg_k2_lattice.hip.inc) and the data-parallel LatticeSimpleDecoder (khg_decode_lattice_simple,
// khg_k2_lattice_simple.hip.inc), each with its raw lattice (khg_decode_lattice_faster_raw, khg_k2_lattice_faster_raw.hip.inc;
// khg_decode_lattice_simple_raw, khg_k2_lattice_raw.hip.inc), the operations on resident lattices (khg_k2_lattice_ops.hip.inc) and their
// forward-backward posteriors (khg_lattices_posteriors, khg_k2_lattice_post.hip.inc).  gfx950 only.
#include "khg_internal.hpp"

#include <memory>

#include "khg_k2_viterbi.hip.inc"
#include "khg_k2_lattice.hip.inc"
#include "khg_k2_lattice_simple.hip.inc"
#include "khg_k2_lattice_raw.hip.inc"
#include "khg_k2_lattice_faster_raw.hip.inc"
#include "khg_k2_lattice_ops.hip.inc"
#include "khg_k2_lattice_post.hip.inc"

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

extern "C" int khg_align(khg_ctx* ctx, const khg_tm* tm, khg_utts* u, const khg_align_config* cfg,
                         int32_t* ali_h, int32_t* words_h, int64_t* words_off_h, int64_t words_cap,
                         float* like_h, int32_t* status_h) {
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
  int rc = wait_ali(ctx, u);
  if (!rc) rc = k1_band_check(ctx, u);      // BAND scores: their model must be alive and unchanged (khg_k1.hip)
  if (!rc) rc = ensure_ali(ctx, u);
  if (rc) return rc;
  if (!u->bp_d) {
    rc = u_alloc(u, &u->bp_d, (size_t)u->bp_off[u->n_utt]);
    if (!rc) rc = u_alloc(u, &u->layer_best_d, (size_t)(u->N + u->n_utt));
    if (!rc) rc = u_alloc(u, &u->layer_cnt_d, (size_t)(u->N + u->n_utt));
    if (!rc) rc = u_alloc(u, &u->path_d, (size_t)u->path_off[u->n_utt]);
    if (!rc && !u->out_blk_d) {
      rc = u_alloc(u, &u->words_d, (size_t)u->words_off[u->n_utt]);
      if (!rc) rc = u_alloc(u, &u->num_words_d, (size_t)u->n_utt);
      if (!rc) rc = u_alloc(u, &u->status_d, (size_t)u->n_utt);
      if (!rc) rc = u_alloc(u, &u->like_d, (size_t)u->n_utt);
    }
    if (rc) return rc;
  }
  rc = arena_flush(ctx);      // an alignment staged by khg_ali_upload must not land on top of the cleared block
  if (rc) return rc;
  HIPCHK(hipMemsetAsync(u->ali_d, 0, sizeof(int32_t) * (size_t)u->N, ctx->stream));
  K2Args a;
  a.frame_off = u->frame_off_d; a.gidx = u->gidx_d; a.state_off = u->state_off_d; a.start = u->start_d;
  a.in_off = u->in_off_d; a.in_src = u->in_src_d; a.in_col = u->in_col_d; a.in_tid = u->in_tid_d;
  a.in_olabel = u->in_olabel_d; a.in_w = u->in_w_d; a.out_off = u->out_off_d; a.out_inidx = u->out_inidx_d;
  a.final_w = u->final_d; a.trans_cost = tm->has_trans_cost ? tm->trans_cost_d : nullptr;
  a.ll = u->ll_d; a.ll_off = u->ll_off_d;
  a.bp = u->bp_d; a.bp_off = u->bp_off_d; a.layer_best = u->layer_best_d; a.layer_cnt = u->layer_cnt_d;
  a.path = u->path_d; a.path_off = u->path_off_d;
  a.ali = u->ali_d; a.ali_fb = u->ali_d; a.unc = nullptr; a.unc_cnt = nullptr; a.words = u->words_d; a.words_off = u->words_off_d; a.num_words = u->num_words_d;
  a.like = u->like_d; a.status = u->status_d; a.err_flag = ctx->err_flag_d;
  a.prof = nullptr;
  // launch order of the DP kernel: longest utterances first (built once per set)
  if (!u->k2_order_d && u->n_utt > 1) {
    std::vector<int32_t> ord((size_t)u->n_utt);
    for (int i = 0; i < u->n_utt; ++i) ord[(size_t)i] = i;
    std::stable_sort(ord.begin(), ord.end(), [&](int32_t x, int32_t y) {
      return u->frame_off[x + 1] - u->frame_off[x] > u->frame_off[y + 1] - u->frame_off[y];
    });
    int rc2 = u_upload(ctx, u, &u->k2_order_d, ord);
    if (!rc2) rc2 = sync_pageable(ctx);
    if (rc2) return rc2;
  }
  a.order = ctx->opt[KHG_OPT_K2_INORDER] ? nullptr : u->k2_order_d;
  // Split mode: nobody waits for the results here and the set is large -- the order-faithful decoders (side stream) write to ali2_d, the DP
  // kernel leaves an uncertified utterance's range of ali_d zero, flags and counts it: khg_acc_stats can then accumulate the certified
  // utterances while those decoders still run (khg_k3.hip); wait_ali merges.
  const bool split = !(ali_h || like_h || status_h || words_h) && u->n_utt > 64 && !u->small && ctx->opt[KHG_OPT_K2_SPLIT] == 0;
  if (split) {
    if (!u->ali2_d) {
      rc = u_alloc(u, &u->ali2_d, (size_t)u->N);
      if (!rc) rc = u_alloc(u, &u->unc_d, (size_t)u->n_utt + 2);       // flags | [utterances, frames] the DP could not certify
      if (rc) return rc;
      u->unc_cnt_dev = u->unc_d + u->n_utt;
      HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&u->unc_cnt_h), 64, 0));   // pinned landing place of the two counters
    }
    HIPCHK(hipMemsetAsync(u->unc_d, 0, sizeof(int32_t) * ((size_t)u->n_utt + 2), ctx->stream));
    a.ali_fb = u->ali2_d; a.unc = u->unc_d; a.unc_cnt = u->unc_cnt_dev;
  }
  const bool k2prof = ctx->opt[KHG_OPT_K2_PROF] != 0;
  if (k2prof) { HIPCHK(hipMalloc(reinterpret_cast<void**>(&a.prof), sizeof(long long) * 16 * (size_t)u->n_utt)); HIPCHK(hipMemset(a.prof, 0, sizeof(long long) * 16 * (size_t)u->n_utt)); }   // [U][8] DP stamps | [U][8] chain-decoder stamps
  a.beam = cfg->beam; a.retry_beam = cfg->retry_beam; a.acoustic_scale = cfg->acoustic_scale;
  a.like_scale = cfg->like_scale != 0.0f ? cfg->like_scale : cfg->acoustic_scale;
  a.beam_delta = cfg->beam_delta; a.hash_ratio = cfg->hash_ratio;
  a.max_active = cfg->max_active; a.min_active = cfg->min_active;
  a.max_states = u->max_states; a.max_inarcs = u->max_inarcs;
  const size_t S = (size_t)u->max_states, A = (size_t)u->max_inarcs;
  size_t max_npdf = 0;
  for (int i = 0; i < u->n_utt; ++i) max_npdf = std::max<size_t>(max_npdf, (size_t)(u->pdf_off[i + 1] - u->pdf_off[i]));
  // threads: one destination state each (up to 1024), KS states per thread beyond that
  int nthr = (int)std::min<size_t>(1024, (S + 63) / 64 * 64);
  const int ks_force = ctx->opt[KHG_OPT_K2_KS];   // experiment: states per thread on the register-resident path
  if (ks_force == 2 || ks_force == 4) nthr = (int)std::min<size_t>(1024, ((S + ks_force - 1) / ks_force + 63) / 64 * 64);
  const size_t nwave = nthr / 64;
  // register-resident path for the whole batch: in-degree <= 3 (up to 4 states per thread) or <= 6 (one state per thread)
  const bool deg6 = !u->has_eps && u->max_indeg > 3 && u->max_indeg <= 6 && S <= 1024;
  const bool fast = deg6 || (!u->has_eps && u->max_indeg <= 3 && S <= 4096);
  const int KSsel = !fast ? 0 : ((ks_force == 2 || ks_force == 4) && !deg6 && S <= (size_t)1024 * ks_force ? ks_force : (S <= 1024 ? 1 : (S <= 2048 ? 2 : 4)));
  const size_t NSl = fast ? KSsel : 1;
  // trace-back block: fast = five groups of eight layers, one dword per lane and state slot; generic = 33 layers of bytes
  // (fast: also the waves' strips of parked layer minima / counts, 2.5 KB each, in the same area during the forward pass)
  const size_t tb_bytes = fast ? std::max<size_t>(5 * (size_t)nthr * NSl * 4, 2560 * nwave) : (K2_FB + 1) * ((S + 15) & ~size_t(15));
  // cur | nxt | reductions | arcs | in_off | wave minima/counts | flags | [align] | max(score block (generic), trace-back block)
  size_t lds_dp = 16 * S + 8 * K2_MAXW + 8 * A + 4 * (S + 1) + 8 * K2_FB * nwave + 32 + 8 * K2_MAXW + 16 +
                  std::max<size_t>(fast ? 0 : 4 * K2_SB * (max_npdf | 1), tb_bytes) + 64;
  size_t HB = std::max<size_t>(2 * S, 1000);
  size_t lds_f = 32 * S + 8 * HB + 4 * (S + A) + 4 * S + 4 * (S + 1) + 16 * A + A + 64;
  // The order-faithful decoder for the utterances the DP cannot certify: the wave-parallel form with all its tables in LDS; with the
  // graph tables in an HBM scratch slice per utterance (> ~1600 states on a chain graph); the one-lane form beyond that.
  // KHG_K2_SERIAL = 1: always the one-lane form; 2: the HBM-graph wave form wherever its per-frame tables fit (tests, A/B).
  const int odeg_w = u->max_outdeg <= 8 ? std::max(1, (int)u->max_outdeg) : 0;     // 0: exact slot prefix sums
  const bool use_pos = u->has_eps || S > 1000;
  const size_t lds_w_mut = 16 * S + 8 * S + 4 * 4 * S + 4 * S + 4 * max_npdf + (odeg_w ? 0 : 4 * A + 4 * S) + (use_pos ? 4 * S : 0) +
                           (u->has_eps ? 4 * (S + A + 1) : 0) + 8 + 8 * ((std::max(A, S * (size_t)odeg_w) + 63) / 64 + 1);
  const size_t lds_w_graph = 8 * (S + 1) + 5 * 4 * A + (u->has_eps ? 4 * (S + 1) + 4 * A : 0) + A + S + 64;
  const int fmode = ctx->opt[KHG_OPT_K2_SERIAL];
  // The chain form (k2_viterbi_faithful_chain: no epsilon-input arcs, <= 1000 states, out-degree <= 4 -- a linear transcript's training
  // graph): a third of the wave form's latency per frame.  KHG_K2_SERIAL = 3: the general wave form also where the chain form applies.
  const int odeg_c = (int)std::max<int32_t>(1, u->max_outdeg);
  const size_t S4 = (S + 3) & ~size_t(3);
  // the frame loop's tables: token costs x 2 + state keys (24) | first / winner (8) | token states x 2 (4): 36 per state; per out-arc slot:
  // parked cost (8) + record (8) + info (4, GetCutoff's array over it) + ordinal (1); the score row.  Over them, set-up and tail only:
  // in-arc offsets (4 per state) + sources (2 per arc) + the trace-back's 9 rows.
  const size_t lds_chain = std::max<size_t>(36 * S4 + 21 * S4 * (size_t)odeg_c + 4 * max_npdf,
                                            4 * (S4 + 1) + 2 * A + 16 + 9 * ((S + 15) & ~size_t(15))) + 128;
  const bool chain = fmode == 0 && !u->has_eps && S <= 1000 && u->max_outdeg <= 4 && lds_chain <= 64 * 1024 && max_npdf <= 32767;
  const bool wave_lds = (fmode == 0 || fmode == 3) && S <= 65535 && lds_w_mut + lds_w_graph <= 160 * 1024;
  const bool wave_gm = fmode != 1 && !wave_lds && S <= 65535 && lds_w_mut <= 160 * 1024;
  const bool lane_gm = !wave_lds && !wave_gm && lds_f > 160 * 1024;
  // Graphs whose DP tables exceed the 160 KB of LDS (a large decoding graph, not a training graph): the generic DP runs with its
  // tables carved out of the same HBM scratch slice.
  const bool gmem = lds_dp > 160 * 1024;
  a.gscratch = nullptr; a.gscratch_stride = 0;
  if (gmem) // (the generic DP's carve-up: no register-resident path)
    lds_dp = 16 * S + 8 * K2_MAXW + 8 * A + 4 * (S + 1) + 8 * K2_FB * nwave + 32 + 8 * K2_MAXW + 16 +
             std::max<size_t>(4 * K2_SB * (max_npdf | 1), (K2_FB + 1) * ((S + 15) & ~size_t(15))) + 64;
  if (gmem || wave_gm || lane_gm) {
    const size_t stride = (std::max(gmem ? lds_dp : 0, std::max(wave_gm ? lds_w_graph : 0, lane_gm ? lds_f : 0)) + 255) & ~size_t(255);
    const size_t need = stride * (size_t)u->n_utt;
    if (need > u->k2_gscratch_bytes) {
      DEVFREE(u->k2_gscratch_d);
      { int rg = u_alloc(u, &u->k2_gscratch_d, need); if (rg) return rg; }
      u->k2_gscratch_bytes = need;
    }
    a.gscratch = u->k2_gscratch_d; a.gscratch_stride = (int64_t)stride;
  }
  if (gmem) {
    KernelTimer kt(ctx, "k2_viterbi_dp");
    KHG_LAUNCH(ctx, (k2_viterbi_dp<1, 1, false, true>), dim3(u->n_utt), dim3(nthr), 0, ctx->stream, a);
  } else {
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
#define K2_DP_CASES(X)                                                                                         \
    if (deg6) X((k2_viterbi_dp<1, 6, true>));                                                                  \
    else if (sc2) X((k2_viterbi_dp<1, 2, true, false, true>));                                                 \
    else if (deg2) X((k2_viterbi_dp<1, 2, true>));                                                             \
    else if (sc3) X((k2_viterbi_dp<1, 3, true, false, true>));                                                 \
    else if (KSsel == 1) X((k2_viterbi_dp<1, 3, true>));                                                       \
    else if (KSsel == 2 && deg2m && u->same_col) X((k2_viterbi_dp<2, 2, true, false, true>));                  \
    else if (KSsel == 2 && deg2m) X((k2_viterbi_dp<2, 2, true>));                                              \
    else if (KSsel == 2) X((k2_viterbi_dp<2, 3, true>));                                                       \
    else if (KSsel == 4 && deg2m && u->same_col) X((k2_viterbi_dp<4, 2, true, false, true>));                  \
    else if (KSsel == 4 && deg2m) X((k2_viterbi_dp<4, 2, true>));                                              \
    else if (KSsel == 4) X((k2_viterbi_dp<4, 3, true>));                                                       \
    else X((k2_viterbi_dp<1, 1, false>));
#define K2_SET_LDS(FN) HIPCHK(hipFuncSetAttribute((const void*)FN, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_dp))
#define K2_LAUNCH(FN) KHG_LAUNCH(ctx, FN, dim3(u->n_utt), dim3(nthr), lds_dp, ctx->stream, a)
    if (lds_dp > 48 * 1024) { K2_DP_CASES(K2_SET_LDS) }
    KernelTimer kt(ctx, "k2_viterbi_dp");
    K2_DP_CASES(K2_LAUNCH)
#undef K2_LAUNCH
#undef K2_SET_LDS
#undef K2_DP_CASES
  }
  HIPCHK(hipGetLastError());
  // The order-faithful decoder for what the DP could not certify runs on a side stream, beside the main stream's next K1 -- unless
  // the caller waits for the results right here (host outputs): then nothing can overlap it, and it follows the DP on the main
  // stream without the two cross-stream events (the per-utterance call pattern: ~30 us of a ~300 us call).
  const bool sync_call = ali_h || like_h || status_h || words_h;
  hipStream_t side = ctx->stream;
  if (!sync_call) {
    if (!u->ev_dp) { HIPCHK(hipEventCreateWithFlags(&u->ev_dp, hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&u->ev_ali, hipEventDisableTiming)); }
    if (split) HIPCHK(hipMemcpyAsync(u->unc_cnt_h, u->unc_cnt_dev, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));   // read by khg_acc_stats behind ev_dp
    HIPCHK(hipEventRecord(u->ev_dp, ctx->stream));
    side = ctx->sides[ctx->next_side];
    ctx->side_dirty[ctx->next_side] = true;
    ctx->next_side = (ctx->next_side + 1) % khg_ctx::NSIDE;
    HIPCHK(hipStreamWaitEvent(side, u->ev_dp, 0));
  }
  rc = k1_band_repair(ctx, u, u->status_d, K2_ST_NEED_FALLBACK, side);      // khg_k1.hip (BAND form of K1 only)
  if (rc) return rc;
  {
    KernelTimer kt(ctx, "k2_viterbi_faithful", side);
    if (chain) {
#define K2_CHAIN(OD)                                                                                                            \
  do {                                                                                                                          \
    if (lds_chain > 48 * 1024) HIPCHK(hipFuncSetAttribute((const void*)k2_viterbi_faithful_chain<OD>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_chain)); \
    KHG_LAUNCH(ctx, k2_viterbi_faithful_chain<OD>, dim3(u->n_utt), dim3(64), lds_chain, side, a, (int)max_npdf);                \
  } while (0)
      switch (odeg_c) { case 1: K2_CHAIN(1); break; case 2: K2_CHAIN(2); break; case 3: K2_CHAIN(3); break; default: K2_CHAIN(4); break; }
#undef K2_CHAIN
    } else if (wave_gm) {
      if (lds_w_mut > 48 * 1024) HIPCHK(hipFuncSetAttribute((const void*)k2_viterbi_faithful_wave<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_w_mut));
      KHG_LAUNCH(ctx, k2_viterbi_faithful_wave<true>, dim3(u->n_utt), dim3(64), lds_w_mut, side, a, u->has_eps ? 1 : 0, odeg_w, (int)max_npdf);
    } else if (wave_lds) {
      const size_t lds_w = lds_w_mut + lds_w_graph;
      if (lds_w > 48 * 1024) HIPCHK(hipFuncSetAttribute((const void*)k2_viterbi_faithful_wave<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_w));
      KHG_LAUNCH(ctx, k2_viterbi_faithful_wave<false>, dim3(u->n_utt), dim3(64), lds_w, side, a, u->has_eps ? 1 : 0, odeg_w, (int)max_npdf);
    } else if (lane_gm) {
      KHG_LAUNCH(ctx, k2_viterbi_faithful<true>, dim3(u->n_utt), dim3(64), 0, side, a);
    } else {
      if (lds_f > 48 * 1024) HIPCHK(hipFuncSetAttribute((const void*)k2_viterbi_faithful<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_f));
      KHG_LAUNCH(ctx, k2_viterbi_faithful<false>, dim3(u->n_utt), dim3(64), lds_f, side, a);
    }
  }
  HIPCHK(hipGetLastError());
  if (!sync_call) { HIPCHK(hipEventRecord(u->ev_ali, side)); u->ali_pending = true; }
  u->ali_split = split;
  u->ali_valid = true;
  if (k2prof) {  // diagnostics: average s_memtime ticks per phase of k2_viterbi_dp
    std::vector<long long> pr(16 * (size_t)u->n_utt);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipStreamSynchronize(side));
    HIPCHK(hipMemcpy(pr.data(), a.prof, pr.size() * 8, hipMemcpyDeviceToHost));
    (void)hipFree(a.prof);
    double ph[4] = {0, 0, 0, 0}, sT = 0, sS = 0, sf = 0; int n = 0;
    for (int i = 0; i < u->n_utt; ++i) if (pr[i * 8 + 4]) { for (int k = 0; k < 4; ++k) ph[k] += (double)(pr[i * 8 + k + 1] - pr[i * 8 + k]); sT += pr[i * 8 + 5]; sS += pr[i * 8 + 6]; sf += pr[i * 8 + 7]; ++n; }
    if (n) fprintf(stderr, "[KHG_K2_PROF] %d utts, avg T %.1f S %.1f fast %.2f threads %d lds %zu | ticks: setup %.0f forward %.0f traceback %.0f replay %.0f\n",
                   n, sT / n, sS / n, sf / n, nthr, lds_dp, ph[0] / n, ph[1] / n, ph[2] / n, ph[3] / n);
    const long long* pc = pr.data() + 8 * (size_t)u->n_utt;     // chain decoder: 0 start, 1 set-up done, 2 frames done (all attempts), 3 finished, 4 frames decoded
    double cs[3] = {0, 0, 0}, cf = 0, cp[3] = {0, 0, 0}; int nc = 0;
    for (int i = 0; i < u->n_utt; ++i) if (pc[i * 8 + 3]) { for (int k = 0; k < 3; ++k) { cs[k] += (double)(pc[i * 8 + k + 1] - pc[i * 8 + k]); cp[k] += (double)pc[i * 8 + 5 + k]; } cf += (double)pc[i * 8 + 4]; ++nc; }
    if (nc) fprintf(stderr, "[KHG_K2_PROF] chain decoder: %d utts, avg frames decoded %.1f | ticks: setup %.0f frames %.0f (%.1f per frame: GetCutoff %.1f, pass 1 %.1f, pass 2 %.1f, rest = row flush + score staging) finish %.0f\n",
                    nc, cf / nc, cs[0] / nc, cs[1] / nc, cs[1] / std::max(1.0, cf), cp[0] / std::max(1.0, cf), cp[1] / std::max(1.0, cf), cp[2] / std::max(1.0, cf), cs[2] / nc);
  }
  if (!ali_h && !like_h && !status_h && !words_h) return KHG_OK;   // asynchronous: errors surface at khg_ctx_sync / downloads
  rc = wait_ali(ctx, u);
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
    if (words_h && words_off_h) {
      const int32_t *nw = hp + 2 * nu, *w = hp + 3 * nu;
      int64_t o = 0;
      for (int i = 0; i < u->n_utt; ++i) {
        words_off_h[i] = o;
        const int64_t n = std::min<int64_t>(nw[i], u->words_off[i + 1] - u->words_off[i]);
        if (o + n > words_cap) return khg_set_error(KHG_E_ARG, "khg_align: words_cap too small");
        std::copy(w + u->words_off[i], w + u->words_off[i] + n, words_h + o);
        o += n;
      }
      words_off_h[u->n_utt] = o;
    }
    return KHG_OK;
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
    int64_t o = 0;
    for (int i = 0; i < u->n_utt; ++i) {
      words_off_h[i] = o;
      int64_t n = std::min<int64_t>(nw[i], u->words_off[i + 1] - u->words_off[i]);
      if (o + n > words_cap) return khg_set_error(KHG_E_ARG, "khg_align: words_cap too small");
      std::copy(w.begin() + u->words_off[i], w.begin() + u->words_off[i] + n, words_h + o);
      o += n;
    }
    words_off_h[u->n_utt] = o;
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return KHG_OK;
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

// ------------------------------------------------------------------------------------------
// The raw lattices of one batch (khg_decode_lattice_simple_raw, khg_decode_lattice_faster_raw): per chunk of scratch slices one exactly-sized
// device block holding
// the six per-state and five per-arc arrays of the chunk's utterances, one after the other.
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
};

// ------------------------------------------------------------------------------------------
// K2L: LatticeFasterDecoder (khg_k2_lattice.hip.inc)
extern "C" void khg_lattice_faster_config_default(khg_lattice_faster_config* c) {
  c->beam = 16.0f; c->max_active = INT32_MAX; c->min_active = 200; c->lattice_beam = 10.0f; c->prune_interval = 25;
  c->beam_delta = 0.5f; c->hash_ratio = 2.0f; c->prune_scale = 0.1f; c->acoustic_scale = 1.0f; c->allow_partial = 1;
  c->scratch_per_frame = 0;
}

// khg_decode_lattice_faster (lat_out == nullptr: nothing below about lattices runs, and the slices have no lattice rows) and
// khg_decode_lattice_faster_raw
static int decode_lattice_faster_impl(khg_ctx* ctx, const khg_tm* tm, khg_utts* u, const khg_lattice_faster_config* cfg,
                                      int32_t* ali_h, int32_t* words_h, int64_t* words_off_h, int64_t words_cap,
                                      double* like_h, int32_t* status_h, khg_lattices** lat_out) {
  const std::string who = lat_out ? "khg_decode_lattice_faster_raw" : "khg_decode_lattice_faster";      // the call the user made
  if (ctx_dead(ctx) || !tm || !u || !cfg) return khg_set_error(KHG_E_ARG, who + ": bad arguments");
  { int rf = utts_foreign_ctx(ctx, u, who.c_str()); if (rf) return rf; }
  if (!u->has_graphs) return khg_set_error(KHG_E_ARG, who + ": the utterance set has no decoding graphs");
  if (!u->ll_valid) return khg_set_error(KHG_E_ARG, who + ": call khg_loglikes first");
  // khg_loglikes_band leaves upper bounds in the cells past the band: a token of a partial (or pruned-late) path may read any cell
  if (u->ll_mode == 2)
    return khg_set_error(KHG_E_ARG, who + ": the scores come from khg_loglikes_band; call khg_loglikes (every cell) first");
  // LatticeFasterDecoderConfig::Check (csrc/lattice-faster-decoder.h:99-104)
  if (!(cfg->beam > 0.0f && cfg->max_active > 1 && cfg->lattice_beam > 0.0f && cfg->min_active <= cfg->max_active &&
        cfg->prune_interval > 0 && cfg->beam_delta > 0.0f && cfg->hash_ratio >= 1.0f && cfg->prune_scale > 0.0f && cfg->prune_scale < 1.0f) ||
      cfg->min_active < 0 || cfg->scratch_per_frame < 0)
    return khg_set_error(KHG_E_RUNTIME, "LatticeFasterDecoderConfig assertion failed");
  int rc = wait_ali(ctx, u);
  if (!rc) rc = k1_band_check(ctx, u);
  if (rc) return rc;
  const int U = u->n_utt;
  const bool lat = lat_out != nullptr;
  struct LatFree { void operator()(khg_lattices* l) const { (void)khg_lattices_destroy(l); } };
  std::unique_ptr<khg_lattices, LatFree> lats;
  if (lat) {
    lats.reset(new khg_lattices);
    lats->U = U;
    lats->state_off.assign((size_t)U + 1, 0);
    lats->arc_off.assign((size_t)U + 1, 0);
  }
  if (U == 0) { if (lat) *lat_out = lats.release(); return KHG_OK; }
  const int64_t hb = std::max<int64_t>(1000, (int64_t)((float)u->max_states * cfg->hash_ratio)) + 1;
  const int64_t Amax = u->max_inarcs;     // (the kernel lays every slice out with the same arc bound)
  std::vector<int64_t> wcap_off((size_t)U + 1, 0);
  for (int i = 0; i < U; ++i) wcap_off[(size_t)i + 1] = wcap_off[(size_t)i] + (u->frame_off[i + 1] - u->frame_off[i]) + utt_states(u, i) + 64;
  const int64_t N = u->N, NW = wcap_off[(size_t)U];
  struct Dev {
    std::vector<void*> p;
    ~Dev() { for (void* q : p) if (q) (void)hipFree(q); }
  } dv;
  auto dalloc = [&](size_t n, void** out) -> int {
    void* q = nullptr;
    HIPCHK(hipMalloc(&q, std::max<size_t>(n, 16)));
    dv.p.push_back(q);
    *out = q;
    return KHG_OK;
  };
  int32_t *ali_d, *words_d, *nw_d, *status_d; double* like_d; int64_t* woff_d;
  if ((rc = dalloc(4 * (size_t)std::max<int64_t>(N, 1), reinterpret_cast<void**>(&ali_d))) ||
      (rc = dalloc(4 * (size_t)std::max<int64_t>(NW, 1), reinterpret_cast<void**>(&words_d))) ||
      (rc = dalloc(4 * (size_t)U, reinterpret_cast<void**>(&nw_d))) || (rc = dalloc(4 * (size_t)U, reinterpret_cast<void**>(&status_d))) ||
      (rc = dalloc(8 * (size_t)U, reinterpret_cast<void**>(&like_d))) || (rc = dalloc(8 * ((size_t)U + 1), reinterpret_cast<void**>(&woff_d))))
    return rc;
  // (lattices) what a launch emitted: an exactly-sized block of the utterances list[ch.u0 .. ch.u0 + ch.n), with their offsets inside it;
  // a block not handed to the handle is freed on the way out
  struct EmitBlock { LatChunk ch; std::vector<int64_t> so, ao; };
  struct Blocks {
    std::vector<EmitBlock> v;
    ~Blocks() { for (EmitBlock& b : v) if (b.ch.buf) (void)hipFree(b.ch.buf); }
  } pass1, pass2;
  int64_t *lat_tot_d = nullptr, *lat_off_d = nullptr;
  if (lat) {
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&lats->start_d), 4 * (size_t)U));
    if ((rc = dalloc(16 * (size_t)U, reinterpret_cast<void**>(&lat_tot_d))) || (rc = dalloc(16 * ((size_t)U + 1), reinterpret_cast<void**>(&lat_off_d))))
      return rc;
  }
  rc = arena_flush(ctx);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(woff_d, wcap_off.data(), 8 * ((size_t)U + 1), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemsetAsync(ali_d, 0, 4 * (size_t)std::max<int64_t>(N, 1), ctx->stream));
  LatArgs a;
  a.frame_off = u->frame_off_d; a.gidx = u->gidx_d; a.state_off = u->state_off_d; a.start = u->start_d;
  a.in_off = u->in_off_d; a.in_col = u->in_col_d; a.in_tid = u->in_tid_d; a.in_olabel = u->in_olabel_d; a.in_w = u->in_w_d;
  a.out_off = u->out_off_d; a.out_inidx = u->out_inidx_d; a.final_w = u->final_d;
  a.trans_cost = tm->has_trans_cost ? tm->trans_cost_d : nullptr;
  a.ll = u->ll_d; a.ll_off = u->ll_off_d;
  a.hb = (int32_t)hb; a.amax = (int32_t)Amax;
  a.ali = ali_d; a.words = words_d; a.words_off = woff_d; a.num_words = nw_d; a.like = like_d; a.status = status_d;
  a.beam = cfg->beam; a.lattice_beam = cfg->lattice_beam; a.beam_delta = cfg->beam_delta; a.hash_ratio = cfg->hash_ratio;
  a.prune_scale = cfg->prune_scale; a.acoustic_scale = cfg->acoustic_scale;
  a.max_active = cfg->max_active; a.min_active = cfg->min_active; a.prune_interval = cfg->prune_interval; a.allow_partial = cfg->allow_partial ? 1 : 0;
  // One pass over a list of utterances: each gets a scratch slice of `per_frame` tokens / links per frame (0: the automatic size,
  // -1: the whole graph per frame, i.e. an utterance can never run out); slices are grouped into launches of <= 4 GiB of scratch.
  auto run = [&](const std::vector<int32_t>& list, int64_t per_frame, Blocks* blocks) -> int {
    const size_t L = list.size();
    std::vector<int32_t> tcap(L), lcap(L);
    std::vector<int64_t> bytes(L);
    for (size_t k = 0; k < L; ++k) {
      const int i = list[k];
      const int64_t T = u->frame_off[i + 1] - u->frame_off[i], S = utt_states(u, i), A = std::max<int64_t>(Amax, 1);
      const int64_t pt = per_frame > 0 ? per_frame : per_frame < 0 ? S : std::min<int64_t>(S, 256);
      const int64_t pl = per_frame > 0 ? per_frame : per_frame < 0 ? A : std::min<int64_t>(A, 1024);
      const int64_t tc = (T + 1) * pt + (per_frame > 0 ? 0 : S) + 1, lc = (T + 1) * pl + (per_frame > 0 ? 0 : A) + 1;
      if (tc > INT32_MAX / 2 || lc > INT32_MAX / 2) return khg_set_error(KHG_E_ARG, who + ": utterance too large for the scratch");
      tcap[k] = (int32_t)tc; lcap[k] = (int32_t)lc;
      bytes[k] = (lat_layout(T, S, Amax, hb, tc, lc, lat).total + 255) & ~int64_t(255);
    }
    const int64_t budget = int64_t(4) << 30;
    std::vector<size_t> cb{0};
    std::vector<int64_t> rel(L);
    int64_t acc = 0, max_chunk = 0;
    for (size_t k = 0; k < L; ++k) {
      if (acc > 0 && acc + bytes[k] > budget) { max_chunk = std::max(max_chunk, acc); cb.push_back(k); acc = 0; }
      rel[k] = acc;                    // relative to the launch's first slice
      acc += bytes[k];
    }
    max_chunk = std::max(max_chunk, acc);
    cb.push_back(L);
    unsigned char* scratch; int64_t* scr_off_d; int32_t *tcap_d, *lcap_d, *list_d;
    int r;
    if ((r = dalloc((size_t)max_chunk, reinterpret_cast<void**>(&scratch))) || (r = dalloc(8 * L, reinterpret_cast<void**>(&scr_off_d))) ||
        (r = dalloc(4 * L, reinterpret_cast<void**>(&tcap_d))) || (r = dalloc(4 * L, reinterpret_cast<void**>(&lcap_d))) ||
        (r = dalloc(4 * L, reinterpret_cast<void**>(&list_d))))
      return r;
    HIPCHK(hipMemcpyAsync(scr_off_d, rel.data(), 8 * L, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(tcap_d, tcap.data(), 4 * L, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(lcap_d, lcap.data(), 4 * L, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(list_d, list.data(), 4 * L, hipMemcpyHostToDevice, ctx->stream));
    a.scratch = scratch; a.scr_off = scr_off_d; a.tok_cap = tcap_d; a.link_cap = lcap_d; a.list = list_d;
    std::vector<int64_t> lat_off_h;
    for (size_t c = 0; c + 1 < cb.size(); ++c) {
      if (!lat) {
        KernelTimer kt(ctx, "k2_lattice_faster");
        KHG_LAUNCH(ctx, k2_lattice_faster, dim3((unsigned)(cb[c + 1] - cb[c])), dim3(64), 0, ctx->stream, a, (int)cb[c]);
        HIPCHK(hipGetLastError());
        continue;
      }
      // the launch's lattices, while its slices are alive: the decoder leaves the rows and the totals, one scan over the utterances,
      // ONE synchronisation to size the output, the fill
      const int n = (int)(cb[c + 1] - cb[c]), k0 = (int)cb[c];
      {
        KernelTimer kt(ctx, "k2_lattice_faster");
        KHG_LAUNCH(ctx, k2_lattice_faster_lat, dim3((unsigned)n), dim3(64), 0, ctx->stream, a, k0, lat_tot_d);
        HIPCHK(hipGetLastError());
      }
      {
        LrArgs sp;       // (K2R's scan over a launch's utterances: it reads n and the two arrays only)
        std::memset(&sp, 0, sizeof(sp));
        sp.n = n; sp.utt_tot = lat_tot_d; sp.utt_off = lat_off_d;
        KernelTimer kt(ctx, "k2_lattice_faster_raw_scan");
        KHG_LAUNCH(ctx, k2_lattice_raw_scan_utts, dim3(1), dim3(64), 0, ctx->stream, sp);
        HIPCHK(hipGetLastError());
      }
      lat_off_h.assign(2 * ((size_t)n + 1), 0);
      HIPCHK(hipMemcpyAsync(lat_off_h.data(), lat_off_d, 16 * ((size_t)n + 1), hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(hipStreamSynchronize(ctx->stream));
      blocks->v.emplace_back();
      EmitBlock& eb = blocks->v.back();
      LatChunk& ch = eb.ch;
      ch.u0 = k0; ch.n = n; ch.ns = lat_off_h[(size_t)n]; ch.na = lat_off_h[2 * (size_t)n + 1];
      eb.so.assign(lat_off_h.begin(), lat_off_h.begin() + n + 1);
      eb.ao.assign(lat_off_h.begin() + n + 1, lat_off_h.end());
      int64_t max_n = 0;
      for (int b = 0; b < n; ++b) {
        const int64_t ns = eb.so[(size_t)b + 1] - eb.so[(size_t)b], na = eb.ao[(size_t)b + 1] - eb.ao[(size_t)b];
        if (ns > INT32_MAX || na > INT32_MAX)
          return khg_set_error(KHG_E_ARG, who + ": the lattice of utterance " + std::to_string(list[(size_t)k0 + b]) +
                                              " has more than 2^31 - 1 states or arcs");
        max_n = std::max(max_n, ns);
      }
      int64_t o = 0;
      auto take = [&](int64_t cnt) { const int64_t r = o; o += (4 * cnt + 255) & ~int64_t(255); return r; };
      for (int j = 0; j < 6; ++j) ch.st[j] = take(ch.ns);
      for (int j = 0; j < 5; ++j) ch.ar[j] = take(ch.na);
      HIPCHK(hipMalloc(reinterpret_cast<void**>(&ch.buf), (size_t)std::max<int64_t>(o, 16)));
      LfrArgs p;
      std::memset(&p, 0, sizeof(p));
      p.a = a; p.n = n; p.utt_off = lat_off_d; p.start_out = lats->start_d;
      p.st_frame = reinterpret_cast<int32_t*>(ch.buf + ch.st[0]); p.st_gstate = reinterpret_cast<int32_t*>(ch.buf + ch.st[1]);
      p.st_tot = reinterpret_cast<float*>(ch.buf + ch.st[2]); p.st_extra = reinterpret_cast<float*>(ch.buf + ch.st[3]);
      p.st_final = reinterpret_cast<float*>(ch.buf + ch.st[4]); p.st_arc_begin = reinterpret_cast<int32_t*>(ch.buf + ch.st[5]);
      p.arc_ilabel = reinterpret_cast<int32_t*>(ch.buf + ch.ar[0]); p.arc_olabel = reinterpret_cast<int32_t*>(ch.buf + ch.ar[1]);
      p.arc_g = reinterpret_cast<float*>(ch.buf + ch.ar[2]); p.arc_ac = reinterpret_cast<float*>(ch.buf + ch.ar[3]);
      p.arc_next = reinterpret_cast<int32_t*>(ch.buf + ch.ar[4]);
      // state stripes go to workgroups of their own while the launch has few utterances (k2_lattice_prune_fill's rule)
      const unsigned gy = (unsigned)std::max<int64_t>(1, std::min<int64_t>((max_n + LFR_NT - 1) / LFR_NT, std::max<int64_t>(1, 4096 / n)));
      {
        KernelTimer kt(ctx, "k2_lattice_faster_raw_fill");
        KHG_LAUNCH(ctx, k2_lattice_faster_raw_fill, dim3((unsigned)n, gy), dim3(LFR_NT), 0, ctx->stream, p, k0);
        HIPCHK(hipGetLastError());
      }
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));    // the slices are freed with `dv` or reused by the next pass
    return KHG_OK;
  };
  std::vector<int32_t> all((size_t)U);
  for (int i = 0; i < U; ++i) all[(size_t)i] = i;
  rc = run(all, cfg->scratch_per_frame, &pass1);
  if (!rc) rc = check_err_flag(ctx, who.c_str());     // synchronises
  if (rc) return rc;
  std::vector<int32_t> st((size_t)U), nw((size_t)U), w((size_t)std::max<int64_t>(NW, 1));
  HIPCHK(hipMemcpy(st.data(), status_d, 4 * (size_t)U, hipMemcpyDeviceToHost));
  std::vector<int32_t> again;
  if (cfg->scratch_per_frame == 0) {
    // the automatic size ran out: those utterances again with room for every state and arc on every frame (a frame never holds more)
    for (int i = 0; i < U; ++i) if (st[(size_t)i] & KHG_LAT_SCRATCH) again.push_back(i);
    if (!again.empty()) {
      rc = run(again, -1, &pass2);
      if (!rc) rc = check_err_flag(ctx, who.c_str());
      if (rc) return rc;
      HIPCHK(hipMemcpy(st.data(), status_d, 4 * (size_t)U, hipMemcpyDeviceToHost));
    }
  }
  if (ali_h && N) HIPCHK(hipMemcpyAsync(ali_h, ali_d, 4 * (size_t)N, hipMemcpyDeviceToHost, ctx->stream));
  if (like_h) HIPCHK(hipMemcpyAsync(like_h, like_d, 8 * (size_t)U, hipMemcpyDeviceToHost, ctx->stream));
  if (words_h && words_off_h) {
    HIPCHK(hipMemcpyAsync(nw.data(), nw_d, 4 * (size_t)U, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(w.data(), words_d, 4 * (size_t)std::max<int64_t>(NW, 1), hipMemcpyDeviceToHost, ctx->stream));
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (status_h) std::copy(st.begin(), st.end(), status_h);
  if (words_h && words_off_h) {
    int64_t o = 0;
    for (int i = 0; i < U; ++i) {
      words_off_h[i] = o;
      const int64_t n = (st[(size_t)i] & KHG_LAT_SUCCEEDED) ? nw[(size_t)i] : 0;
      if (o + n > words_cap) return khg_set_error(KHG_E_ARG, who + ": words_cap too small");
      std::copy(w.begin() + wcap_off[(size_t)i], w.begin() + wcap_off[(size_t)i] + n, words_h + o);
      o += n;
    }
    words_off_h[U] = o;
  }
  if (!lat) return KHG_OK;
  // The handle: every utterance in utterance order, its chunks the first pass's launches.  Without a second pass the first pass's
  // blocks are the chunks.  With one, a chunk that holds a re-decoded utterance is rebuilt on the device from the blocks of both
  // passes (k2_lattice_faster_raw_gather); only offsets travel.
  // where every utterance's lattice is: block (first pass's, then second pass's), first state / arc there, sizes
  std::vector<int32_t> src_blk((size_t)U, 0);
  std::vector<int64_t> src_off(2 * (size_t)U, 0), ns_u((size_t)U, 0), na_u((size_t)U, 0);
  std::vector<EmitBlock*> blk;
  for (EmitBlock& b : pass1.v) blk.push_back(&b);
  for (EmitBlock& b : pass2.v) blk.push_back(&b);
  std::vector<char> redone((size_t)U, 0);
  for (int32_t i : again) redone[(size_t)i] = 1;
  for (size_t j = 0; j < blk.size(); ++j) {
    const bool second = j >= pass1.v.size();
    const EmitBlock& e = *blk[j];
    for (int b = 0; b < e.ch.n; ++b) {
      const int i = second ? again[(size_t)e.ch.u0 + b] : e.ch.u0 + b;
      if (!second && redone[(size_t)i]) continue;        // (empty there: the second pass's is the one)
      src_blk[(size_t)i] = (int32_t)j;
      src_off[2 * (size_t)i] = e.so[(size_t)b]; src_off[2 * (size_t)i + 1] = e.ao[(size_t)b];
      ns_u[(size_t)i] = e.so[(size_t)b + 1] - e.so[(size_t)b]; na_u[(size_t)i] = e.ao[(size_t)b + 1] - e.ao[(size_t)b];
    }
  }
  for (int i = 0; i < U; ++i) {
    lats->state_off[(size_t)i + 1] = lats->state_off[(size_t)i] + ns_u[(size_t)i];
    lats->arc_off[(size_t)i + 1] = lats->arc_off[(size_t)i] + na_u[(size_t)i];
  }
  LfrBlock* blocks_d = nullptr;
  std::vector<LfrBlock> blocks_h;
  std::vector<std::vector<int64_t>> dst_off_keep;      // (host sides of copies in flight until the synchronisation below)
  if (!again.empty()) {
    for (const EmitBlock* e : blk) {
      LfrBlock bd;
      for (int j = 0; j < 6; ++j) bd.st[j] = reinterpret_cast<const int32_t*>(e->ch.buf + e->ch.st[j]);
      for (int j = 0; j < 5; ++j) bd.ar[j] = reinterpret_cast<const int32_t*>(e->ch.buf + e->ch.ar[j]);
      blocks_h.push_back(bd);
    }
    if ((rc = dalloc(sizeof(LfrBlock) * blocks_h.size(), reinterpret_cast<void**>(&blocks_d)))) return rc;
    HIPCHK(hipMemcpyAsync(blocks_d, blocks_h.data(), sizeof(LfrBlock) * blocks_h.size(), hipMemcpyHostToDevice, ctx->stream));
  }
  lats->bytes += 4 * (int64_t)U;
  for (EmitBlock& e : pass1.v) {
    const int u0 = e.ch.u0, n = e.ch.n;
    bool rebuild = false;
    for (int b = 0; b < n; ++b) rebuild = rebuild || redone[(size_t)u0 + b];
    LatChunk ch;
    ch.u0 = u0; ch.n = n;
    if (!rebuild) {
      ch = e.ch;
      e.ch.buf = nullptr;        // the handle's from here on
    } else {
      dst_off_keep.emplace_back(2 * ((size_t)n + 1), 0);
      std::vector<int64_t>& dst_off = dst_off_keep.back();
      for (int b = 0; b < n; ++b) {
        dst_off[(size_t)b + 1] = dst_off[(size_t)b] + ns_u[(size_t)u0 + b];
        dst_off[(size_t)n + 2 + b] = dst_off[(size_t)n + 1 + b] + na_u[(size_t)u0 + b];
      }
      ch.ns = dst_off[(size_t)n]; ch.na = dst_off[2 * (size_t)n + 1];
      int64_t o = 0;
      auto take = [&](int64_t cnt) { const int64_t r = o; o += (4 * cnt + 255) & ~int64_t(255); return r; };
      for (int j = 0; j < 6; ++j) ch.st[j] = take(ch.ns);
      for (int j = 0; j < 5; ++j) ch.ar[j] = take(ch.na);
      HIPCHK(hipMalloc(reinterpret_cast<void**>(&ch.buf), (size_t)std::max<int64_t>(o, 16)));
    }
    lats->chunks.push_back(ch);
    for (int j = 0; j < 6; ++j) lats->bytes += (4 * ch.ns + 255) & ~int64_t(255);
    for (int j = 0; j < 5; ++j) lats->bytes += (4 * ch.na + 255) & ~int64_t(255);
    if (!rebuild) continue;
    LfrGather g;
    std::memset(&g, 0, sizeof(g));
    int32_t* src_blk_d; int64_t *src_off_d, *dst_off_d;
    if ((rc = dalloc(4 * (size_t)n, reinterpret_cast<void**>(&src_blk_d))) || (rc = dalloc(16 * (size_t)n, reinterpret_cast<void**>(&src_off_d))) ||
        (rc = dalloc(16 * ((size_t)n + 1), reinterpret_cast<void**>(&dst_off_d))))
      return rc;
    HIPCHK(hipMemcpyAsync(src_blk_d, src_blk.data() + u0, 4 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(src_off_d, src_off.data() + 2 * (size_t)u0, 16 * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(dst_off_d, dst_off_keep.back().data(), 16 * ((size_t)n + 1), hipMemcpyHostToDevice, ctx->stream));
    g.blocks = blocks_d; g.src_block = src_blk_d; g.src_off = src_off_d; g.dst_off = dst_off_d; g.n = n;
    for (int j = 0; j < 6; ++j) g.st[j] = reinterpret_cast<int32_t*>(ch.buf + ch.st[j]);
    for (int j = 0; j < 5; ++j) g.ar[j] = reinterpret_cast<int32_t*>(ch.buf + ch.ar[j]);
    int64_t max_n = 1;
    for (int b = 0; b < n; ++b) max_n = std::max(max_n, std::max(ns_u[(size_t)u0 + b], na_u[(size_t)u0 + b]));
    const unsigned gy = (unsigned)std::max<int64_t>(1, std::min<int64_t>((max_n + LFR_NT - 1) / LFR_NT, std::max<int64_t>(1, 4096 / n)));
    KernelTimer kt(ctx, "k2_lattice_faster_raw_gather");
    KHG_LAUNCH(ctx, k2_lattice_faster_raw_gather, dim3((unsigned)n, gy), dim3(LFR_NT), 0, ctx->stream, g);
    HIPCHK(hipGetLastError());
  }
  if (!again.empty()) {
    rc = check_err_flag(ctx, who.c_str());     // synchronises: the blocks the chunks were gathered from go now
    if (rc) return rc;
  }
  *lat_out = lats.release();
  return KHG_OK;
}

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

extern "C" int khg_lattices_destroy(khg_lattices* l) {
  if (!l) return KHG_OK;
  for (LatChunk& c : l->chunks) if (c.buf) (void)hipFree(c.buf);
  if (l->start_d) (void)hipFree(l->start_d);
  if (l->off_d) (void)hipFree(l->off_d);
  for (int32_t* q : l->idx_d) if (q) (void)hipFree(q);
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

// khg_decode_lattice_simple (lat_out == nullptr: nothing below about lattices runs) and khg_decode_lattice_simple_raw
static int decode_lattice_simple_impl(khg_ctx* ctx, const khg_tm* tm, khg_utts* u, const khg_lattice_simple_config* cfg,
                                      int32_t* ali_h, int32_t* words_h, int64_t* words_off_h, int64_t words_cap,
                                      double* like_h, int32_t* status_h, int32_t* err_frame_h, khg_lattices** lat_out) {
  if (ctx_dead(ctx) || !tm || !u || !cfg) return khg_set_error(KHG_E_ARG, "khg_decode_lattice_simple: bad arguments");
  { int rf = utts_foreign_ctx(ctx, u, "khg_decode_lattice_simple"); if (rf) return rf; }
  if (!u->has_graphs) return khg_set_error(KHG_E_ARG, "khg_decode_lattice_simple: the utterance set has no decoding graphs");
  if (!u->ll_valid) return khg_set_error(KHG_E_ARG, "khg_decode_lattice_simple: call khg_loglikes first");
  // khg_loglikes_band leaves upper bounds in the cells past the band: a token the beam keeps may read any cell
  if (u->ll_mode == 2)
    return khg_set_error(KHG_E_ARG, "khg_decode_lattice_simple: the scores come from khg_loglikes_band; call khg_loglikes (every cell) first");
  // LatticeSimpleDecoderConfig::Check (csrc/lattice-simple-decoder.h:76-78)
  if (!(cfg->beam > 0.0f && cfg->lattice_beam > 0.0f && cfg->prune_interval > 0) || cfg->scratch_per_frame < 0)
    return khg_set_error(KHG_E_RUNTIME, "LatticeSimpleDecoderConfig assertion failed");
  int rc = wait_ali(ctx, u);
  if (!rc) rc = k1_band_check(ctx, u);
  if (rc) return rc;
  const int U = u->n_utt;
  const bool lat = lat_out != nullptr;
  struct LatFree { void operator()(khg_lattices* l) const { (void)khg_lattices_destroy(l); } };
  std::unique_ptr<khg_lattices, LatFree> lats;
  if (lat) {
    lats.reset(new khg_lattices);
    lats->U = U;
    lats->state_off.assign((size_t)U + 1, 0);
    lats->arc_off.assign((size_t)U + 1, 0);
  }
  if (U == 0) { if (lat) *lat_out = lats.release(); return KHG_OK; }
  std::vector<int64_t> wcap_off((size_t)U + 1, 0);
  for (int i = 0; i < U; ++i) wcap_off[(size_t)i + 1] = wcap_off[(size_t)i] + (u->frame_off[i + 1] - u->frame_off[i]) + utt_states(u, i) + 64;
  const int64_t N = u->N, NW = wcap_off[(size_t)U];
  struct Dev {
    std::vector<void*> p;
    ~Dev() { for (void* q : p) if (q) (void)hipFree(q); }
  } dv;
  auto dalloc = [&](size_t n, void** out) -> int {
    void* q = nullptr;
    HIPCHK(hipMalloc(&q, std::max<size_t>(n, 16)));
    dv.p.push_back(q);
    *out = q;
    return KHG_OK;
  };
  int64_t *lat_tot_d = nullptr, *lat_off_d = nullptr;
  if (lat) {
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&lats->start_d), 4 * (size_t)U));
    lats->bytes += 4 * (int64_t)U;
    if ((rc = dalloc(16 * (size_t)U, reinterpret_cast<void**>(&lat_tot_d))) || (rc = dalloc(16 * ((size_t)U + 1), reinterpret_cast<void**>(&lat_off_d))))
      return rc;
  }
  int32_t *ali_d, *words_d, *nw_d, *status_d, *ef_d; double* like_d; int64_t* woff_d;
  if ((rc = dalloc(4 * (size_t)std::max<int64_t>(N, 1), reinterpret_cast<void**>(&ali_d))) ||
      (rc = dalloc(4 * (size_t)std::max<int64_t>(NW, 1), reinterpret_cast<void**>(&words_d))) ||
      (rc = dalloc(4 * (size_t)U, reinterpret_cast<void**>(&nw_d))) || (rc = dalloc(4 * (size_t)U, reinterpret_cast<void**>(&status_d))) ||
      (rc = dalloc(4 * (size_t)U, reinterpret_cast<void**>(&ef_d))) ||
      (rc = dalloc(8 * (size_t)U, reinterpret_cast<void**>(&like_d))) || (rc = dalloc(8 * ((size_t)U + 1), reinterpret_cast<void**>(&woff_d))))
    return rc;
  rc = arena_flush(ctx);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(woff_d, wcap_off.data(), 8 * ((size_t)U + 1), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemsetAsync(ali_d, 0, 4 * (size_t)std::max<int64_t>(N, 1), ctx->stream));
  LsArgs a;
  a.frame_off = u->frame_off_d; a.gidx = u->gidx_d; a.state_off = u->state_off_d; a.start = u->start_d;
  a.in_off = u->in_off_d; a.in_src = u->in_src_d; a.in_col = u->in_col_d; a.in_tid = u->in_tid_d; a.in_olabel = u->in_olabel_d;
  a.in_w = u->in_w_d; a.out_off = u->out_off_d; a.out_inidx = u->out_inidx_d; a.final_w = u->final_d;
  a.trans_cost = tm->has_trans_cost ? tm->trans_cost_d : nullptr;
  a.ll = u->ll_d; a.ll_off = u->ll_off_d;
  a.ali = ali_d; a.words = words_d; a.words_off = woff_d; a.num_words = nw_d; a.like = like_d; a.status = status_d; a.err_frame = ef_d;
  a.beam = cfg->beam; a.lattice_beam = cfg->lattice_beam; a.acoustic_scale = cfg->acoustic_scale;
  a.prune_interval = cfg->prune_interval; a.tok_cap = cfg->scratch_per_frame; a.amax = u->max_inarcs;
  a.hub = ctx->opt[KHG_OPT_K2S_HUB];
  // every utterance's dense rows, grouped into launches of <= 4 GiB of scratch (an utterance larger than that alone is refused)
  std::vector<int64_t> bytes((size_t)U);
  for (int i = 0; i < U; ++i) {
    const int64_t T = u->frame_off[i + 1] - u->frame_off[i], S = utt_states(u, i);
    bytes[(size_t)i] = ls_layout(T, S, u->max_inarcs, lat).total;     // (the kernel lays every slice out with the same arc bound)
  }
  const int64_t budget = int64_t(4) << 30;
  std::vector<size_t> cb{0};
  std::vector<int64_t> rel((size_t)U);
  int64_t acc = 0, max_chunk = 0;
  for (int i = 0; i < U; ++i) {
    if (bytes[(size_t)i] > budget)
      return khg_set_error(KHG_E_ARG, "khg_decode_lattice_simple: utterance " + std::to_string(i) + " needs more than 4 GiB of lattice scratch");
    if (acc > 0 && acc + bytes[(size_t)i] > budget) { max_chunk = std::max(max_chunk, acc); cb.push_back((size_t)i); acc = 0; }
    rel[(size_t)i] = acc;
    acc += bytes[(size_t)i];
  }
  max_chunk = std::max(max_chunk, acc);
  cb.push_back((size_t)U);
  unsigned char* scratch; int64_t* scr_off_d; int32_t* list_d;
  if ((rc = dalloc((size_t)max_chunk, reinterpret_cast<void**>(&scratch))) || (rc = dalloc(8 * (size_t)U, reinterpret_cast<void**>(&scr_off_d))) ||
      (rc = dalloc(4 * (size_t)U, reinterpret_cast<void**>(&list_d))))
    return rc;
  std::vector<int32_t> all((size_t)U);
  for (int i = 0; i < U; ++i) all[(size_t)i] = i;
  HIPCHK(hipMemcpyAsync(scr_off_d, rel.data(), 8 * (size_t)U, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(list_d, all.data(), 4 * (size_t)U, hipMemcpyHostToDevice, ctx->stream));
  a.scratch = scratch; a.scr_off = scr_off_d; a.list = list_d;
  // one wave for small graphs, up to four for larger ones (a lane owns states s = lane, lane + NT, ...)
  const int nt = u->max_states <= 64 ? 64 : u->max_states <= 128 ? 128 : LS_NT;
  int64_t max_T = 0;
  for (int i = 0; i < U; ++i) max_T = std::max<int64_t>(max_T, u->frame_off[i + 1] - u->frame_off[i]);
  std::vector<int64_t> lat_off_h;
  for (size_t c = 0; c + 1 < cb.size(); ++c) {
    {
      KernelTimer kt(ctx, "k2_lattice_simple");
      KHG_LAUNCH(ctx, k2_lattice_simple, dim3((unsigned)(cb[c + 1] - cb[c])), dim3(nt), 0, ctx->stream, a, (int)cb[c]);
      HIPCHK(hipGetLastError());
    }
    if (lat) {
      // the chunk's lattices, while its slices are alive: count, the two scans, ONE synchronisation to size the output, the fill
      const int n = (int)(cb[c + 1] - cb[c]), u0 = (int)cb[c];
      LrArgs p;
      std::memset(&p, 0, sizeof(p));
      p.a = a; p.n = n; p.utt_tot = lat_tot_d; p.utt_off = lat_off_d; p.start_out = lats->start_d;
      // frames are independent: stripes of them go to workgroups of their own while the chunk has few utterances
      const unsigned gy = (unsigned)std::min<int64_t>(max_T + 1, std::max<int64_t>(1, 1024 / n));
      {
        KernelTimer kt(ctx, "k2_lattice_raw_count");
        KHG_LAUNCH(ctx, k2_lattice_raw_count, dim3((unsigned)n, gy), dim3(nt), 0, ctx->stream, p, u0);
        HIPCHK(hipGetLastError());
      }
      {
        KernelTimer kt(ctx, "k2_lattice_raw_scan");
        KHG_LAUNCH(ctx, k2_lattice_raw_scan_frames, dim3((unsigned)n), dim3(64), 0, ctx->stream, p, u0);
        KHG_LAUNCH(ctx, k2_lattice_raw_scan_utts, dim3(1), dim3(64), 0, ctx->stream, p);
        HIPCHK(hipGetLastError());
      }
      lat_off_h.assign(2 * ((size_t)n + 1), 0);
      HIPCHK(hipMemcpyAsync(lat_off_h.data(), lat_off_d, 16 * ((size_t)n + 1), hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(hipStreamSynchronize(ctx->stream));
      LatChunk ch;
      ch.u0 = u0; ch.n = n; ch.ns = lat_off_h[(size_t)n]; ch.na = lat_off_h[2 * (size_t)n + 1];
      for (int b = 0; b < n; ++b) {
        const int64_t ns = lat_off_h[(size_t)b + 1] - lat_off_h[(size_t)b], na = lat_off_h[(size_t)n + 2 + b] - lat_off_h[(size_t)n + 1 + b];
        if (ns > INT32_MAX || na > INT32_MAX)
          return khg_set_error(KHG_E_ARG, "khg_decode_lattice_simple_raw: the lattice of utterance " + std::to_string(u0 + b) + " has more than 2^31 - 1 states or arcs");
        lats->state_off[(size_t)u0 + b + 1] = lats->state_off[(size_t)u0 + b] + ns;
        lats->arc_off[(size_t)u0 + b + 1] = lats->arc_off[(size_t)u0 + b] + na;
      }
      int64_t o = 0;
      auto take = [&](int64_t cnt) { const int64_t r = o; o += (4 * cnt + 255) & ~int64_t(255); return r; };
      for (int k = 0; k < 6; ++k) ch.st[k] = take(ch.ns);
      for (int k = 0; k < 5; ++k) ch.ar[k] = take(ch.na);
      HIPCHK(hipMalloc(reinterpret_cast<void**>(&ch.buf), (size_t)std::max<int64_t>(o, 16)));
      lats->chunks.push_back(ch);
      lats->bytes += o;
      p.st_frame = reinterpret_cast<int32_t*>(ch.buf + ch.st[0]); p.st_gstate = reinterpret_cast<int32_t*>(ch.buf + ch.st[1]);
      p.st_tot = reinterpret_cast<float*>(ch.buf + ch.st[2]); p.st_extra = reinterpret_cast<float*>(ch.buf + ch.st[3]);
      p.st_final = reinterpret_cast<float*>(ch.buf + ch.st[4]); p.st_arc_begin = reinterpret_cast<int32_t*>(ch.buf + ch.st[5]);
      p.arc_ilabel = reinterpret_cast<int32_t*>(ch.buf + ch.ar[0]); p.arc_olabel = reinterpret_cast<int32_t*>(ch.buf + ch.ar[1]);
      p.arc_g = reinterpret_cast<float*>(ch.buf + ch.ar[2]); p.arc_ac = reinterpret_cast<float*>(ch.buf + ch.ar[3]);
      p.arc_next = reinterpret_cast<int32_t*>(ch.buf + ch.ar[4]);
      {
        KernelTimer kt(ctx, "k2_lattice_raw_fill");
        KHG_LAUNCH(ctx, k2_lattice_raw_fill, dim3((unsigned)n, gy), dim3(nt), 0, ctx->stream, p, u0);
        HIPCHK(hipGetLastError());
      }
    }
    if (c + 2 < cb.size()) HIPCHK(hipStreamSynchronize(ctx->stream));     // the next launch reuses the slices
  }
  rc = check_err_flag(ctx, "khg_decode_lattice_simple");     // synchronises
  if (rc) return rc;
  std::vector<int32_t> st((size_t)U), nw((size_t)U), w((size_t)std::max<int64_t>(NW, 1));
  HIPCHK(hipMemcpy(st.data(), status_d, 4 * (size_t)U, hipMemcpyDeviceToHost));
  if (ali_h && N) HIPCHK(hipMemcpyAsync(ali_h, ali_d, 4 * (size_t)N, hipMemcpyDeviceToHost, ctx->stream));
  if (like_h) HIPCHK(hipMemcpyAsync(like_h, like_d, 8 * (size_t)U, hipMemcpyDeviceToHost, ctx->stream));
  if (err_frame_h) HIPCHK(hipMemcpyAsync(err_frame_h, ef_d, 4 * (size_t)U, hipMemcpyDeviceToHost, ctx->stream));
  if (words_h && words_off_h) {
    HIPCHK(hipMemcpyAsync(nw.data(), nw_d, 4 * (size_t)U, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(w.data(), words_d, 4 * (size_t)std::max<int64_t>(NW, 1), hipMemcpyDeviceToHost, ctx->stream));
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (status_h) std::copy(st.begin(), st.end(), status_h);
  if (words_h && words_off_h) {
    int64_t o = 0;
    for (int i = 0; i < U; ++i) {
      words_off_h[i] = o;
      const int64_t n = (st[(size_t)i] & KHG_LAT_SUCCEEDED) ? nw[(size_t)i] : 0;
      if (o + n > words_cap) return khg_set_error(KHG_E_ARG, "khg_decode_lattice_simple: words_cap too small");
      std::copy(w.begin() + wcap_off[(size_t)i], w.begin() + wcap_off[(size_t)i] + n, words_h + o);
      o += n;
    }
    words_off_h[U] = o;
  }
  if (lat) *lat_out = lats.release();
  return KHG_OK;
}

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
struct LatFree { void operator()(khg_lattices* l) const { (void)khg_lattices_destroy(l); } };
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
};
const int64_t kLatOpsLds = 48 << 10;        // an utterance's lattice is staged into LDS up to this many bytes

void lat_chunk_layout(LatChunk* ch, int64_t* total) {
  int64_t o = 0;
  auto take = [&](int64_t cnt) { const int64_t r = o; o += (4 * cnt + 255) & ~int64_t(255); return r; };
  for (int k = 0; k < 6; ++k) ch->st[k] = take(ch->ns);
  for (int k = 0; k < 5; ++k) ch->ar[k] = take(ch->na);
  *total = o;
}
void lat_chunk_args(const khg_lattices* l, const LatChunk& c, LoArgs* p) {
  p->st_frame = reinterpret_cast<const int32_t*>(c.buf + c.st[0]); p->st_gstate = reinterpret_cast<const int32_t*>(c.buf + c.st[1]);
  p->st_tot = reinterpret_cast<const float*>(c.buf + c.st[2]); p->st_extra = reinterpret_cast<const float*>(c.buf + c.st[3]);
  p->st_final = reinterpret_cast<const float*>(c.buf + c.st[4]); p->st_arc_begin = reinterpret_cast<const int32_t*>(c.buf + c.st[5]);
  p->arc_ilabel = reinterpret_cast<const int32_t*>(c.buf + c.ar[0]); p->arc_olabel = reinterpret_cast<const int32_t*>(c.buf + c.ar[1]);
  p->arc_g = reinterpret_cast<const float*>(c.buf + c.ar[2]); p->arc_ac = reinterpret_cast<const float*>(c.buf + c.ar[3]);
  p->arc_next = reinterpret_cast<const int32_t*>(c.buf + c.ar[4]);
  p->start = l->start_d; p->state_off = l->off_d; p->arc_off = l->off_d + l->U + 1;
  p->s_base = l->state_off[(size_t)c.u0]; p->a_base = l->arc_off[(size_t)c.u0];
  p->u0 = c.u0; p->n = c.n; p->U = l->U;
}
// the dynamic LDS a launch over chunk c asks for: the largest lattice of the chunk that still fits
int lat_chunk_lds(const khg_ctx* ctx, const khg_lattices* l, const LatChunk& c) {
  if (ctx->opt[KHG_OPT_LAT_OPS_LDS] == 1) return 0;
  int64_t best = 0;
  for (int u = c.u0; u < c.u0 + c.n; ++u) {
    const int64_t need = 4 * (3 * (l->state_off[(size_t)u + 1] - l->state_off[(size_t)u]) + 4 * (l->arc_off[(size_t)u + 1] - l->arc_off[(size_t)u]));
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
    LoArgs p;
    std::memset(&p, 0, sizeof(p));
    lat_chunk_args(l, c, &p);
    KHG_LAUNCH(ctx, k2_lattice_ops_last_frame, dim3((unsigned)((c.n + LO_NT - 1) / LO_NT)), dim3(LO_NT), 0, ctx->stream, p, t_d);
    HIPCHK(hipGetLastError());
  }
  std::vector<int32_t> t(U);
  HIPCHK(hipMemcpyAsync(t.data(), t_d, 4 * U, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  l->ali_off.assign(U + 1, 0);
  for (size_t u = 0; u < U; ++u) l->ali_off[u + 1] = l->ali_off[u] + std::max(t[u], 0);
  return KHG_OK;
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
  int rc = arena_flush(ctx);
  if (!rc) rc = lat_meta(ctx, l);
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
  std::unique_ptr<khg_lattices, LatFree> l(new khg_lattices);
  l->U = n_utt;
  l->state_off.assign(state_off, state_off + n_utt + 1);
  l->arc_off.assign(arc_off, arc_off + n_utt + 1);
  if (n_utt == 0) { *out = l.release(); return KHG_OK; }
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&l->start_d), 4 * (size_t)n_utt));
  l->bytes += 4 * (int64_t)n_utt;
  LatChunk ch;
  ch.u0 = 0; ch.n = n_utt; ch.ns = state_off[n_utt]; ch.na = arc_off[n_utt];
  int64_t total = 0;
  lat_chunk_layout(&ch, &total);
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&ch.buf), (size_t)std::max<int64_t>(total, 16)));
  l->chunks.push_back(ch);
  l->bytes += total;
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
  int rc = arena_flush(ctx);
  if (!rc) rc = lat_meta(ctx, l);
  if (rc) return rc;
  const int64_t KU = (int64_t)K * U, AT = l->ali_off[(size_t)U];
  DevBlocks dv;
  int32_t *ali_d, *nw_d, *status_d, *packed_d;
  float *weight_d, *gs_d, *as_d;
  int64_t *ali_off_d, *woff_d;
  if ((rc = dv.alloc(std::max<int64_t>((int64_t)K * AT, 1), &ali_d)) || (rc = dv.alloc(KU, &nw_d)) || (rc = dv.alloc(KU, &status_d)) ||
      (rc = dv.alloc(2 * KU, &weight_d)) || (rc = dv.alloc(K, &gs_d)) || (rc = dv.alloc(K, &as_d)) || (rc = dv.alloc(U + 1, &ali_off_d)) ||
      (rc = dv.alloc(KU + 1, &woff_d)))
    return rc;
  HIPCHK(hipMemsetAsync(ali_d, 0, 4 * (size_t)std::max<int64_t>((int64_t)K * AT, 1), ctx->stream));
  HIPCHK(hipMemcpyAsync(gs_d, graph_scale, 4 * (size_t)K, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(as_d, acoustic_scale, 4 * (size_t)K, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemcpyAsync(ali_off_d, l->ali_off.data(), 8 * ((size_t)U + 1), hipMemcpyHostToDevice, ctx->stream));
  std::vector<LoArgs> pcs;
  for (const LatChunk& c : l->chunks) {
    LoArgs p;
    std::memset(&p, 0, sizeof(p));
    lat_chunk_args(l, c, &p);
    p.lds_bytes = lat_chunk_lds(ctx, l, c);
    p.K = K; p.gs = gs_d; p.as = as_d; p.ali = ali_d; p.ali_off = ali_off_d; p.ali_total = AT;
    p.nwords = nw_d; p.weight = weight_d; p.status = status_d;
    const int64_t cells = std::max<int64_t>(c.ns * K, 1);
    if ((rc = dv.alloc(cells, &p.d1)) || (rc = dv.alloc(cells, &p.d2)) || (rc = dv.alloc(cells, &p.n1)) || (rc = dv.alloc(cells, &p.n2)) ||
        (rc = dv.alloc(cells, &p.bp)) || (rc = dv.alloc(cells, &p.words)))
      return rc;
    {
      KernelTimer kt(ctx, "k2_lattice_best_path");
      KHG_LAUNCH(ctx, k2_lattice_best_path, dim3((unsigned)c.n, (unsigned)((K + LO_NT - 1) / LO_NT)), dim3(LO_NT), (size_t)p.lds_bytes, ctx->stream, p);
      HIPCHK(hipGetLastError());
    }
    pcs.push_back(p);
  }
  // the words, packed on the device: a scan of the counts, one synchronisation to size the block, the copy
  std::vector<int64_t> woff((size_t)KU + 1, 0);
  std::vector<int32_t> packed, st((size_t)KU);
  if (words_h && words_off_h) {
    {
      KernelTimer kt(ctx, "k2_lattice_ops_words");
      KHG_LAUNCH(ctx, k2_lattice_ops_scan, dim3(1), dim3(64), 0, ctx->stream, nw_d, woff_d, KU);
      HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(woff.data(), woff_d, 8 * ((size_t)KU + 1), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const int64_t NW = woff[(size_t)KU];
    if ((rc = dv.alloc(std::max<int64_t>(NW, 1), &packed_d))) return rc;
    if (NW > 0) {
      KernelTimer kt(ctx, "k2_lattice_ops_words");
      for (const LoArgs& p : pcs)
        KHG_LAUNCH(ctx, k2_lattice_ops_pack_words, dim3((unsigned)p.n, (unsigned)std::min(K, 64)), dim3(LO_NT), 0, ctx->stream, p, woff_d, packed_d);
      HIPCHK(hipGetLastError());
      packed.resize((size_t)NW);
      HIPCHK(hipMemcpyAsync(packed.data(), packed_d, 4 * (size_t)NW, hipMemcpyDeviceToHost, ctx->stream));
    }
  }
  if (ali_h && AT) HIPCHK(hipMemcpyAsync(ali_h, ali_d, 4 * (size_t)((int64_t)K * AT), hipMemcpyDeviceToHost, ctx->stream));
  if (weight_h) HIPCHK(hipMemcpyAsync(weight_h, weight_d, 8 * (size_t)KU, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(st.data(), status_d, 4 * (size_t)KU, hipMemcpyDeviceToHost, ctx->stream));
  rc = check_err_flag(ctx, "khg_lattices_best_path");     // synchronises
  if (rc) return rc;
  if (words_h && words_off_h) {
    int64_t o = 0;
    for (int64_t i = 0; i < KU; ++i) {
      words_off_h[i] = o;
      int64_t n = (st[(size_t)i] & KHG_LAT_SUCCEEDED) ? woff[(size_t)i + 1] - woff[(size_t)i] : 0;
      if (o + n > words_cap) { st[(size_t)i] = KHG_LAT_WORDS; n = 0; }      // the path's words do not fit: none of them
      std::copy(packed.begin() + woff[(size_t)i], packed.begin() + woff[(size_t)i] + n, words_h + o);
      o += n;
    }
    words_off_h[KU] = o;
  }
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
  std::unique_ptr<khg_lattices, LatFree> res(new khg_lattices);
  res->U = U;
  res->state_off.assign((size_t)U + 1, 0);
  res->arc_off.assign((size_t)U + 1, 0);
  if (U == 0) { *out = res.release(); return KHG_OK; }
  int rc = arena_flush(ctx);
  if (!rc) rc = lat_meta(ctx, l);
  if (rc) return rc;
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&res->start_d), 4 * (size_t)U));
  res->bytes += 4 * (int64_t)U;
  DevBlocks dv;
  int32_t* status_d;
  if ((rc = dv.alloc(U, &status_d))) return rc;
  std::vector<int64_t> off_h;
  for (const LatChunk& c : l->chunks) {
    LoArgs p;
    std::memset(&p, 0, sizeof(p));
    lat_chunk_args(l, c, &p);
    p.lds_bytes = lat_chunk_lds(ctx, l, c);
    p.K = 1; p.gs1 = graph_scale; p.as1 = acoustic_scale; p.beam = beam; p.status = status_d; p.o_start = res->start_d;
    const int64_t cells = std::max<int64_t>(c.ns, 1);
    if ((rc = dv.alloc(cells, &p.d1)) || (rc = dv.alloc(cells, &p.d2)) || (rc = dv.alloc(cells, &p.n1)) || (rc = dv.alloc(cells, &p.n2)) ||
        (rc = dv.alloc(cells, &p.e1)) || (rc = dv.alloc(cells, &p.e2)) || (rc = dv.alloc(cells, &p.bp)) || (rc = dv.alloc(cells, &p.pn)) ||
        (rc = dv.alloc(cells, &p.newid)) || (rc = dv.alloc(cells, &p.nab)) || (rc = dv.alloc(c.n, &p.limit)) ||
        (rc = dv.alloc(2 * (int64_t)c.n, &p.utt_tot)) || (rc = dv.alloc(2 * ((int64_t)c.n + 1), &p.utt_off)))
      return rc;
    {
      KernelTimer kt(ctx, "k2_lattice_prune_mark");
      KHG_LAUNCH(ctx, k2_lattice_prune_mark, dim3((unsigned)c.n), dim3(LO_NT), (size_t)p.lds_bytes, ctx->stream, p);
      HIPCHK(hipGetLastError());
    }
    {
      KernelTimer kt(ctx, "k2_lattice_prune_scan");
      KHG_LAUNCH(ctx, k2_lattice_prune_scan, dim3(1), dim3(64), 0, ctx->stream, p);
      HIPCHK(hipGetLastError());
    }
    off_h.assign(2 * ((size_t)c.n + 1), 0);
    HIPCHK(hipMemcpyAsync(off_h.data(), p.utt_off, 16 * ((size_t)c.n + 1), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));        // the one synchronisation that sizes the output
    LatChunk ch;
    ch.u0 = c.u0; ch.n = c.n; ch.ns = off_h[(size_t)c.n]; ch.na = off_h[2 * (size_t)c.n + 1];
    for (int b = 0; b < c.n; ++b) {
      res->state_off[(size_t)c.u0 + b + 1] = res->state_off[(size_t)c.u0 + b] + (off_h[(size_t)b + 1] - off_h[(size_t)b]);
      res->arc_off[(size_t)c.u0 + b + 1] = res->arc_off[(size_t)c.u0 + b] + (off_h[(size_t)c.n + 2 + b] - off_h[(size_t)c.n + 1 + b]);
    }
    int64_t total = 0;
    lat_chunk_layout(&ch, &total);
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&ch.buf), (size_t)std::max<int64_t>(total, 16)));
    res->chunks.push_back(ch);
    res->bytes += total;
    p.o_frame = reinterpret_cast<int32_t*>(ch.buf + ch.st[0]); p.o_gstate = reinterpret_cast<int32_t*>(ch.buf + ch.st[1]);
    p.o_tot = reinterpret_cast<float*>(ch.buf + ch.st[2]); p.o_extra = reinterpret_cast<float*>(ch.buf + ch.st[3]);
    p.o_final = reinterpret_cast<float*>(ch.buf + ch.st[4]); p.o_arc_begin = reinterpret_cast<int32_t*>(ch.buf + ch.st[5]);
    p.o_ilabel = reinterpret_cast<int32_t*>(ch.buf + ch.ar[0]); p.o_olabel = reinterpret_cast<int32_t*>(ch.buf + ch.ar[1]);
    p.o_g = reinterpret_cast<float*>(ch.buf + ch.ar[2]); p.o_ac = reinterpret_cast<float*>(ch.buf + ch.ar[3]);
    p.o_next = reinterpret_cast<int32_t*>(ch.buf + ch.ar[4]);
    int64_t max_n = 0;
    for (int b = 0; b < c.n; ++b) max_n = std::max(max_n, l->state_off[(size_t)c.u0 + b + 1] - l->state_off[(size_t)c.u0 + b]);
    const unsigned gy = (unsigned)std::max<int64_t>(1, std::min<int64_t>((max_n + LO_NT - 1) / LO_NT, std::max<int64_t>(1, 4096 / c.n)));
    {
      KernelTimer kt(ctx, "k2_lattice_prune_fill");
      KHG_LAUNCH(ctx, k2_lattice_prune_fill, dim3((unsigned)c.n, gy), dim3(LO_NT), 0, ctx->stream, p);
      HIPCHK(hipGetLastError());
    }
  }
  std::vector<int32_t> st((size_t)U);
  HIPCHK(hipMemcpyAsync(st.data(), status_d, 4 * (size_t)U, hipMemcpyDeviceToHost, ctx->stream));
  rc = check_err_flag(ctx, "khg_lattices_prune");     // synchronises: the scratch goes with `dv`
  if (rc) return rc;
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
};

namespace {
struct PostFree { void operator()(khg_posteriors* p) const { (void)khg_posteriors_destroy(p); } };
// alpha, beta and the Jacobi row (doubles) beside the staged lattice
int64_t post_lds_need(const khg_lattices* l, int u) {
  const int64_t N = l->state_off[(size_t)u + 1] - l->state_off[(size_t)u], A = l->arc_off[(size_t)u + 1] - l->arc_off[(size_t)u];
  return 24 * N + 4 * (3 * N + 4 * A);
}
int post_chunk_lds(const khg_ctx* ctx, const khg_lattices* l, const LatChunk& c) {
  if (ctx->opt[KHG_OPT_LAT_OPS_LDS] == 1) return 0;
  int64_t best = 0;
  for (int u = c.u0; u < c.u0 + c.n; ++u) {
    const int64_t need = post_lds_need(l, u);
    if (need <= kLatOpsLds) best = std::max(best, need);
  }
  return (int)best;
}
// the in-arc index, once per handle
int lat_index(khg_ctx* ctx, khg_lattices* l) {
  if (l->idx_d.size() == l->chunks.size()) return KHG_OK;
  DevBlocks dv;
  for (size_t k = l->idx_d.size(); k < l->chunks.size(); ++k) {
    const LatChunk& c = l->chunks[k];
    const int64_t words = c.ns + c.n + 2 * c.na;
    int32_t* blk = nullptr;
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&blk), (size_t)std::max<int64_t>(4 * words, 16)));
    l->idx_d.push_back(blk);
    l->bytes += 4 * words;
    int32_t* cur = nullptr;
    int rc = dv.alloc(std::max<int64_t>(c.ns, 1), &cur);
    if (rc) return rc;
    LoArgs p;
    std::memset(&p, 0, sizeof(p));
    lat_chunk_args(l, c, &p);
    KernelTimer kt(ctx, "k2_lattice_post_index");
    KHG_LAUNCH(ctx, k2_lattice_post_index, dim3((unsigned)c.n), dim3(64), 0, ctx->stream, p, blk, blk + c.ns + c.n, blk + c.ns + c.n + c.na, cur);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));       // the cursors go with `dv`
  return KHG_OK;
}
}  // namespace

extern "C" int khg_posteriors_destroy(khg_posteriors* p) {
  if (!p) return KHG_OK;
  for (PostChunk& c : p->chunks) {
    if (c.arc_post) (void)hipFree(c.arc_post);
    if (c.buf) (void)hipFree(c.buf);
  }
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

extern "C" int khg_lattices_posteriors(khg_ctx* ctx, const khg_lattices* lc, float graph_scale, float acoustic_scale, int32_t* status_h,
                                       double* tot_like_h, khg_posteriors** out) {
  if (ctx_dead(ctx) || !lc || !out) return khg_set_error(KHG_E_ARG, "khg_lattices_posteriors: bad arguments");
  *out = nullptr;
  if (bad_scale(graph_scale) || bad_scale(acoustic_scale))
    return khg_set_error(KHG_E_ARG, "khg_lattices_posteriors: graph_scale and acoustic_scale must be finite and >= 0");
  khg_lattices* l = const_cast<khg_lattices*>(lc);
  const int U = l->U;
  std::unique_ptr<khg_posteriors, PostFree> res(new khg_posteriors);
  res->U = U;
  res->frame_off.assign((size_t)U + 1, 0);
  res->entry_off.assign((size_t)U + 1, 0);
  res->arc_off = l->arc_off;
  if (U == 0) { *out = res.release(); return KHG_OK; }
  int rc = arena_flush(ctx);
  if (!rc) rc = lat_meta(ctx, l);
  if (!rc) rc = lat_index(ctx, l);
  if (rc) return rc;
  DevBlocks dv;
  int32_t* status_d; double* tot_d; int64_t* ali_off_d;
  if ((rc = dv.alloc(U, &status_d)) || (rc = dv.alloc(U, &tot_d)) || (rc = dv.alloc(U + 1, &ali_off_d))) return rc;
  HIPCHK(hipMemcpyAsync(ali_off_d, l->ali_off.data(), 8 * ((size_t)U + 1), hipMemcpyHostToDevice, ctx->stream));
  std::vector<int64_t> off_h;
  for (size_t k = 0; k < l->chunks.size(); ++k) {
    const LatChunk& c = l->chunks[k];
    PoArgs p;
    std::memset(&p, 0, sizeof(p));
    lat_chunk_args(l, c, &p.lo);
    p.lo.lds_bytes = post_chunk_lds(ctx, l, c);
    p.lo.status = status_d; p.lo.ali_off = ali_off_d; p.tot = tot_d;
    p.in_begin = l->idx_d[k]; p.in_arc = l->idx_d[k] + c.ns + c.n; p.arc_src = l->idx_d[k] + c.ns + c.n + c.na;
    p.gs = (double)graph_scale; p.as = (double)acoustic_scale;
    p.f_base = l->ali_off[(size_t)c.u0];
    const int64_t nfr = l->ali_off[(size_t)c.u0 + c.n] - p.f_base;
    const int64_t cells = std::max<int64_t>(c.ns, 1), arcs = std::max<int64_t>(c.na, 1);
    if ((rc = dv.alloc(cells, &p.alpha)) || (rc = dv.alloc(cells, &p.beta)) || (rc = dv.alloc(cells, &p.row)) || (rc = dv.alloc(arcs, &p.flag)) ||
        (rc = dv.alloc(arcs, &p.rank)) || (rc = dv.alloc(std::max<int64_t>(nfr, 1), &p.fcnt)) || (rc = dv.alloc(nfr + 2 * (int64_t)c.n, &p.fstate)) ||
        (rc = dv.alloc(2 * (int64_t)c.n, &p.lo.utt_tot)) || (rc = dv.alloc(2 * ((int64_t)c.n + 1), &p.lo.utt_off)))
      return rc;
    PostChunk pc;
    pc.u0 = c.u0; pc.n = c.n; pc.na = c.na;
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&pc.arc_post), (size_t)(8 * arcs)));
    res->chunks.push_back(pc);
    res->bytes += 8 * c.na;
    p.arc_post = pc.arc_post;
    {
      KernelTimer kt(ctx, "k2_lattice_post_fb");
      KHG_LAUNCH(ctx, k2_lattice_post_fb, dim3((unsigned)c.n), dim3(PO_NT), (size_t)p.lo.lds_bytes, ctx->stream, p);
      HIPCHK(hipGetLastError());
    }
    {
      KernelTimer kt(ctx, "k2_lattice_post_scan");
      KHG_LAUNCH(ctx, k2_lattice_prune_scan, dim3(1), dim3(64), 0, ctx->stream, p.lo);     // frames at [b], entries at [n + 1 + b]
      HIPCHK(hipGetLastError());
    }
    off_h.assign(2 * ((size_t)c.n + 1), 0);
    HIPCHK(hipMemcpyAsync(off_h.data(), p.lo.utt_off, 16 * ((size_t)c.n + 1), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));        // the one synchronisation that sizes the output
    PostChunk& q = res->chunks.back();
    q.nf = off_h[(size_t)c.n]; q.ne = off_h[2 * (size_t)c.n + 1];
    for (int b = 0; b < c.n; ++b) {
      res->frame_off[(size_t)c.u0 + b + 1] = res->frame_off[(size_t)c.u0 + b] + (off_h[(size_t)b + 1] - off_h[(size_t)b]);
      res->entry_off[(size_t)c.u0 + b + 1] = res->entry_off[(size_t)c.u0 + b] + (off_h[(size_t)c.n + 2 + b] - off_h[(size_t)c.n + 1 + b]);
    }
    q.o_weight = (8 * (q.nf + 1) + 255) & ~int64_t(255);
    q.o_tid = q.o_weight + ((8 * q.ne + 255) & ~int64_t(255));
    const int64_t total = q.o_tid + 4 * q.ne;
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&q.buf), (size_t)std::max<int64_t>(total, 16)));
    res->bytes += total;
    p.entry_begin = reinterpret_cast<int64_t*>(q.buf); p.weight = reinterpret_cast<double*>(q.buf + q.o_weight);
    p.tid = reinterpret_cast<int32_t*>(q.buf + q.o_tid);
    int64_t max_a = 0;
    for (int b = 0; b < c.n; ++b) max_a = std::max(max_a, l->arc_off[(size_t)c.u0 + b + 1] - l->arc_off[(size_t)c.u0 + b]);
    const unsigned gy = (unsigned)std::max<int64_t>(1, std::min<int64_t>((max_a + PO_NT - 1) / PO_NT, std::max<int64_t>(1, 4096 / c.n)));
    {
      KernelTimer kt(ctx, "k2_lattice_post_fill");
      KHG_LAUNCH(ctx, k2_lattice_post_fill, dim3((unsigned)c.n, gy), dim3(PO_NT), 0, ctx->stream, p);
      HIPCHK(hipGetLastError());
    }
  }
  std::vector<int32_t> st((size_t)U);
  std::vector<double> tl((size_t)U);
  HIPCHK(hipMemcpyAsync(st.data(), status_d, 4 * (size_t)U, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(tl.data(), tot_d, 8 * (size_t)U, hipMemcpyDeviceToHost, ctx->stream));
  rc = check_err_flag(ctx, "khg_lattices_posteriors");     // synchronises: the scratch goes with `dv`
  if (rc) return rc;
  if (status_h) std::copy(st.begin(), st.end(), status_h);
  if (tot_like_h) std::copy(tl.begin(), tl.end(), tot_like_h);
  *out = res.release();
  return KHG_OK;
}
