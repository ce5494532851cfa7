// kaldi_hmm_gmm_amd/csrc/khg_utts.hip -- C-ABI (include/khg_hip.h): utterance sets = features + decoding graphs resident in HBM;
// host-side planning of the per-utterance pdf lists, first / last useful frames and the in-arc CSR K2 reads.  gfx950 only.
#include "khg_internal.hpp"

static void plan_ll(khg_utts* u) {
  u->ll_off.assign(u->n_utt + 1, 0);
  for (int i = 0; i < u->n_utt; ++i) {
    int64_t T = u->frame_off[i + 1] - u->frame_off[i];
    int64_t tpad = (T + 31) & ~int64_t(31);
    u->ll_off[i + 1] = u->ll_off[i] + (u->pdf_off[i + 1] - u->pdf_off[i]) * tpad;
  }
  u->ll_total = u->ll_off[u->n_utt];
}

// ---- planning of one decoding graph: shared by khg_utts_create (one graph per utterance) and khg_graph_create (one graph, once) ----
// The graph owns states [s0, s0 + S) of the caller's CSR-by-source arrays; its tables go to the same rows of the concatenated
// tables `gt` (sized for all graphs by the caller), its facts to `gf`.  Nothing here depends on the utterance's length: the last
// useful frame of a pdf is T - 1 - gf.pdf_dfin[j] (plan_pdf_last).  aligner_limits: the exact-DP aligner's one-byte back-pointers and
// 16-bit arc sources (<= 254 in-arcs per state, <= 65535 states), which khg_utts_create enforces for every set it builds.
struct GraphTables {
  std::vector<int64_t> in_off;
  std::vector<int32_t> in_src, in_col, in_tid, in_ol, out_inidx;
  std::vector<float> in_w;
  void size(int64_t NS, int64_t NA) {
    in_off.assign((size_t)NS + 1, 0);
    in_src.resize((size_t)NA); in_col.resize((size_t)NA); in_tid.resize((size_t)NA); in_ol.resize((size_t)NA); out_inidx.resize((size_t)NA);
    in_w.resize((size_t)NA);
  }
};
struct GraphFacts {
  int32_t max_indeg = 0, max_outdeg = 0;
  bool same_col = true, has_eps = false;
  bool ladder = true;            // states in chain order: every in-arc of state s comes from s or from s - 1 (K2's ladder form, khg_k2.hip)
  int64_t nwords = 0;
  std::vector<int32_t> pdfs, pdf_first, pdf_dfin;
};
static int plan_graph(const std::string& where, const khg_tm* tm, bool aligner_limits, int64_t s0, int64_t S, int32_t start,
                      const int64_t* arc_off, const int32_t* ilabel, const int32_t* olabel, const float* weight, const int32_t* nextstate,
                      const float* final_w, GraphTables* gt, GraphFacts* gf, std::string* msg) {
  auto fail = [&](int code, const std::string& m) { *msg = m; return code; };
  const int64_t a0 = arc_off[s0], a1 = arc_off[s0 + S], A = a1 - a0;
  if (S < 0 || A < 0) return fail(KHG_E_ARG, where + ": offsets not monotone");
  if (start >= S) return fail(KHG_E_ARG, where + ": start state out of range");
  if (aligner_limits && S > 65535) return fail(KHG_E_UNSUPPORTED, where + ": more than 65535 states in one decoding graph");
  if (S > INT32_MAX / 2 || A > INT32_MAX / 2) return fail(KHG_E_UNSUPPORTED, where + ": decoding graph too large");
  for (int64_t s = 0; s < S; ++s) gf->max_outdeg = std::max<int32_t>(gf->max_outdeg, (int32_t)(arc_off[s0 + s + 1] - arc_off[s0 + s]));
  // pdf list of this graph = distinct id2pdf[ilabel] over its arcs
  std::vector<int32_t>& tmp_pdfs = gf->pdfs;
  tmp_pdfs.clear();
  for (int64_t a = a0; a < a1; ++a) {
    int l = ilabel[a];
    if (l < 0 || l > tm->num_tids)
      return fail(KHG_E_RUNTIME, "AddTransitionProbs: invalid symbol " + std::to_string(l) + " on graph input side.");
    if (l >= 1) tmp_pdfs.push_back(tm->id2pdf[l]); else gf->has_eps = true;
    if (nextstate[a] < 0 || nextstate[a] >= S) return fail(KHG_E_ARG, where + ": nextstate out of range");
    if (olabel[a] != 0) ++gf->nwords;
  }
  std::sort(tmp_pdfs.begin(), tmp_pdfs.end());
  tmp_pdfs.erase(std::unique(tmp_pdfs.begin(), tmp_pdfs.end()), tmp_pdfs.end());
  if (tmp_pdfs.size() > 32767) return fail(KHG_E_UNSUPPORTED, where + ": more than 32767 distinct pdfs on one decoding graph");
  {
    // first frame each listed pdf can be needed at: a token can sit in state s after no fewer than
    // dmin[s] emitting arcs (0-1 BFS from the start state), so the score of an arc's pdf is first
    // read at frame dmin[src].  K1 may skip (pdf, frame) cells before that (khg_loglikes_reachable).
    std::vector<int32_t> dmin((size_t)S, INT32_MAX);
    if (start >= 0) {
      std::deque<int32_t> q;
      dmin[start] = 0; q.push_back(start);
      while (!q.empty()) {
        const int s = q.front(); q.pop_front();
        for (int64_t a = arc_off[s0 + s]; a < arc_off[s0 + s + 1]; ++a) {
          const int d = nextstate[a], wgt = ilabel[a] >= 1 ? 1 : 0;
          if (dmin[s] + wgt < dmin[d]) {
            dmin[d] = dmin[s] + wgt;
            if (wgt) q.push_back(d); else q.push_front(d);
          }
        }
      }
    }
    // ... and the last: from state d a final state is no fewer than dfin[d] emitting arcs away (0-1 BFS over the reversed
    // graph from the final states), so an arc into d consumed at frame t leaves T - 1 - t frames, enough iff t <= T - 1 - dfin[d].
    // A token past that can never reach a final state: the BAND form of K1 does not compute what only such tokens read.
    std::vector<int32_t> dfin((size_t)S, INT32_MAX);
    {
      std::vector<int64_t> roff((size_t)S + 1, 0);
      for (int64_t a = a0; a < a1; ++a) roff[(size_t)nextstate[a] + 1]++;
      for (int64_t s = 0; s < S; ++s) roff[(size_t)s + 1] += roff[(size_t)s];
      std::vector<int32_t> rsrc((size_t)A), rw((size_t)A), rc_((size_t)S, 0);
      for (int64_t s = 0; s < S; ++s)
        for (int64_t a = arc_off[s0 + s]; a < arc_off[s0 + s + 1]; ++a) {
          const size_t pos = (size_t)(roff[(size_t)nextstate[a]] + rc_[(size_t)nextstate[a]]++);
          rsrc[pos] = (int32_t)s; rw[pos] = ilabel[a] >= 1 ? 1 : 0;
        }
      std::deque<int32_t> q;
      for (int64_t s = 0; s < S; ++s)
        if (final_w[s0 + s] != std::numeric_limits<float>::infinity()) { dfin[(size_t)s] = 0; q.push_back((int32_t)s); }
      while (!q.empty()) {
        const int d = q.front(); q.pop_front();
        for (int64_t k = roff[(size_t)d]; k < roff[(size_t)d + 1]; ++k) {
          const int s = rsrc[(size_t)k], wgt = rw[(size_t)k];
          if (dfin[(size_t)d] + wgt < dfin[(size_t)s]) {
            dfin[(size_t)s] = dfin[(size_t)d] + wgt;
            if (wgt) q.push_back(s); else q.push_front(s);
          }
        }
      }
    }
    gf->pdf_first.assign(tmp_pdfs.size(), INT32_MAX);
    gf->pdf_dfin.assign(tmp_pdfs.size(), INT32_MAX);
    for (int64_t s = 0; s < S; ++s) {
      if (dmin[s] == INT32_MAX) continue;
      for (int64_t a = arc_off[s0 + s]; a < arc_off[s0 + s + 1]; ++a) {
        if (ilabel[a] < 1) continue;
        const size_t j = (size_t)(std::lower_bound(tmp_pdfs.begin(), tmp_pdfs.end(), tm->id2pdf[ilabel[a]]) - tmp_pdfs.begin());
        gf->pdf_first[j] = std::min(gf->pdf_first[j], dmin[s]);
        gf->pdf_dfin[j] = std::min(gf->pdf_dfin[j], dfin[(size_t)nextstate[a]]);
      }
    }
  }
  // in-arc CSR: stable bucketing by destination (ties in the DP then resolve to the lowest
  // original arc index, like a strict '<' scan over arcs in file order)
  std::vector<int64_t>& in_off = gt->in_off;
  for (int64_t a = a0; a < a1; ++a) in_off[s0 + nextstate[a] + 1]++;
  in_off[s0] = a0;
  for (int64_t s = 0; s < S; ++s) {
    if (aligner_limits && in_off[s0 + s + 1] > 254) return fail(KHG_E_UNSUPPORTED, where + ": a state has more than 254 incoming arcs");
    gf->max_indeg = std::max<int32_t>(gf->max_indeg, (int32_t)in_off[s0 + s + 1]);
    in_off[s0 + s + 1] += in_off[s0 + s];
  }
  std::vector<int32_t> cursor((size_t)S, 0);
  for (int64_t s = 0; s < S; ++s) {
    for (int64_t a = arc_off[s0 + s]; a < arc_off[s0 + s + 1]; ++a) {
      int d = nextstate[a];
      int64_t pos = in_off[s0 + d] + cursor[d]++;
      gt->in_src[pos] = (int32_t)s;
      gt->in_tid[pos] = ilabel[a];
      gt->in_ol[pos] = olabel[a];
      gt->in_w[pos] = weight[a];
      int col = -1;
      if (ilabel[a] >= 1)
        col = (int)(std::lower_bound(tmp_pdfs.begin(), tmp_pdfs.end(), tm->id2pdf[ilabel[a]]) - tmp_pdfs.begin());
      gt->in_col[pos] = col;
      gt->out_inidx[a] = (int32_t)(pos - a0);
    }
  }
  for (int64_t s = 0; s < S && gf->same_col; ++s)
    for (int64_t k = in_off[s0 + s] + 1; k < in_off[s0 + s + 1]; ++k)
      if (gt->in_col[k] != gt->in_col[in_off[s0 + s]]) { gf->same_col = false; break; }
  // ladder: no epsilon-input arc, at most two in-arcs per state, each from the state itself or from the one numbered just below it
  // (at most one of either: the kernel keeps one weight per kind)
  gf->ladder = !gf->has_eps;
  for (int64_t s = 0; s < S && gf->ladder; ++s) {
    const int64_t k0 = in_off[s0 + s], n = in_off[s0 + s + 1] - k0;
    if (n > 2 || (n == 2 && gt->in_src[k0] == gt->in_src[k0 + 1])) gf->ladder = false;
    for (int64_t k = k0; k < k0 + n && gf->ladder; ++k)
      if (gt->in_src[k] != s && gt->in_src[k] != s - 1) gf->ladder = false;
  }
  return KHG_OK;
}

// what one utterance of T frames on a planned graph of S states adds to the set: its pdf list with first / last useful frames,
// and the K2 scratch offsets
static void plan_utt_on_graph(khg_utts* u, int i, int64_t T, int64_t S, const GraphFacts& gf) {
  u->pdf_off[i + 1] = u->pdf_off[i] + (int64_t)gf.pdfs.size();
  u->pdfs.insert(u->pdfs.end(), gf.pdfs.begin(), gf.pdfs.end());
  u->pdf_first.insert(u->pdf_first.end(), gf.pdf_first.begin(), gf.pdf_first.end());
  for (size_t j = 0; j < gf.pdfs.size(); ++j) {
    const int32_t first = gf.pdf_first[j], df = gf.pdf_dfin[j];
    u->pdf_last.push_back(first == INT32_MAX || df == INT32_MAX ? -1 : (int32_t)std::max<int64_t>(-1, T - 1 - df));
  }
  // generic path: one byte per (layer, state); fast path: one dword per (group of eight layers, lane), whole waves
  u->bp_off[i + 1] = u->bp_off[i] + std::max<int64_t>((T + 1) * std::max<int64_t>((S + 15) & ~int64_t(15), 512), ((T >> 3) + 1) * (S + 256) * 4);
  u->path_off[i + 1] = u->path_off[i] + T + S + 8;
  u->words_off[i + 1] = u->words_off[i] + gf.nwords;
}

// everything of a set that does not depend on its graphs: the handle, the features, frame_off
static int utts_begin(const char* where, khg_ctx* ctx, int32_t n_utt, int32_t D, const int64_t* frame_off, const float* feats_h,
                      const float* feats_dv, bool small_graphs, khg_utts** out) {
  if (frame_off[0] != 0) return khg_set_error(KHG_E_ARG, std::string(where) + ": frame_off[0] != 0");
  for (int i = 0; i < n_utt; ++i)
    if (frame_off[i + 1] < frame_off[i]) return khg_set_error(KHG_E_ARG, std::string(where) + ": frame_off not monotone");
  khg_utts* u = new khg_utts();
  u->ctx = ctx; u->n_utt = n_utt; u->D = D;
  u->frame_off.assign(frame_off, frame_off + n_utt + 1);
  u->N = frame_off[n_utt];
  // the reference's per-utterance call pattern (one utterance per set, a new set per call): scratch from the context's arena, one
  // staged copy instead of a hipMalloc + pageable copy per table
  u->small = n_utt <= 16 && u->N <= 16384 && u->N * (int64_t)D <= (int64_t)(512 << 10) && small_graphs;
  int rc = KHG_OK;
  auto fail = [&](int code, const std::string& msg) { khg_utts_destroy(u); return khg_set_error(code, msg); };
  if (feats_dv) { u->feats_d = feats_dv; u->own_feats = false; }
  else {
    float* p = nullptr;
    rc = u_alloc(u, &p, (size_t)u->N * D);
    if (rc) { khg_utts_destroy(u); return rc; }
    u->feats_d = p; u->own_feats = true;
    if (u->N) {
      const size_t nb = sizeof(float) * (size_t)u->N * D;
      if (ctx->arena.owns(p)) { memcpy(ctx->arena.mirror(p), feats_h, nb); arena_mark_dirty(ctx, p, nb); }
      else {
        hipError_t e = hipMemcpyAsync(p, feats_h, nb, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) return fail(KHG_E_HIP, hipGetErrorString(e));
        ctx->pageable_pending = true;
      }
    }
    if (u->small && u->N > 0) {      // the column maxima the split K1 forms scale by: a pass over 48 kB here instead of a kernel + a download
      u->k1.xmax.assign((size_t)D, 0.0f);
      for (int64_t t = 0; t < u->N; ++t) {
        const float* x = feats_h + (size_t)t * D;
        for (int d = 0; d < D; ++d) {        // k1h_absmax's rule: -inf skipped, NaN / +inf come out as +inf
          const float v = x[d], m = u->k1.xmax[(size_t)d];
          if (v == -std::numeric_limits<float>::infinity()) continue;
          u->k1.xmax[(size_t)d] = (std::fabs(v) <= 3.0e38f) ? std::fmax(m, std::fabs(v)) : std::numeric_limits<float>::infinity();
        }
      }
    }
  }
  rc = u_upload(ctx, u, &u->frame_off_d, u->frame_off);
  if (rc) { khg_utts_destroy(u); return rc; }
  u->pdf_off.assign(n_utt + 1, 0);
  *out = u;
  return KHG_OK;
}
static int utts_finish(khg_ctx* ctx, khg_utts* u, khg_utts** out) {
  plan_ll(u);
  int rc = arena_flush(ctx);
  if (!rc) rc = sync_pageable(ctx);        // the caller's arrays and the planning vectors are free after this
  if (rc) { khg_utts_destroy(u); return rc; }
  *out = u;
  return KHG_OK;
}
// device bytes of the graph tables of NS states / NA arcs in `rows` graphs
static int64_t graph_table_bytes(int64_t rows, int64_t NS, int64_t NA) { return 8 * (rows + 1) + 4 * rows + 2 * 8 * (NS + 1) + 6 * 4 * NA + 4 * NS; }

extern "C" int khg_utts_create(khg_ctx* ctx, const khg_tm* tm, int32_t n_utt, int32_t D,
                               const int64_t* frame_off, const float* feats_h, const float* feats_dv,
                               const int64_t* state_off, const int32_t* start, const int64_t* arc_off,
                               const int32_t* ilabel, const int32_t* olabel, const float* weight,
                               const int32_t* nextstate, const float* final_w, khg_utts** out) {
  if (ctx_dead(ctx) || !out || n_utt <= 0 || D <= 0 || !frame_off || (!feats_h && !feats_dv))
    return khg_set_error(KHG_E_ARG, "khg_utts_create: bad arguments");
  khg_utts* u = nullptr;
  int rc = utts_begin("khg_utts_create", ctx, n_utt, D, frame_off, feats_h, feats_dv,
                      !state_off || (state_off[n_utt] <= 32768 && arc_off && arc_off[state_off[n_utt]] <= 65536), &u);
  if (rc) return rc;
  auto fail = [&](int code, const std::string& msg) { khg_utts_destroy(u); return khg_set_error(code, msg); };

  if (state_off && state_off[n_utt] > 0) {
    if (!tm || !start || !arc_off || !ilabel || !olabel || !weight || !nextstate || !final_w)
      return fail(KHG_E_ARG, "khg_utts_create: graph arrays / tm missing");
    u->has_graphs = true;
    u->state_off.assign(state_off, state_off + n_utt + 1);
    const int64_t NS = state_off[n_utt], NA = arc_off[NS];
    std::vector<int64_t> out_off(arc_off, arc_off + NS + 1);
    GraphTables gt;
    gt.size(NS, NA);
    u->bp_off.assign(n_utt + 1, 0); u->path_off.assign(n_utt + 1, 0); u->words_off.assign(n_utt + 1, 0);
    std::string msg;
    for (int i = 0; i < n_utt; ++i) {
      const int64_t s0 = state_off[i], S = state_off[i + 1] - s0;
      const int64_t T = frame_off[i + 1] - frame_off[i];
      GraphFacts gf;
      rc = plan_graph("khg_utts_create", tm, true, s0, S, start[i], arc_off, ilabel, olabel, weight, nextstate, final_w, &gt, &gf, &msg);
      if (rc) return fail(rc, msg);
      u->max_states = std::max<int64_t>(u->max_states, S);
      u->max_inarcs = std::max<int64_t>(u->max_inarcs, arc_off[s0 + S] - arc_off[s0]);
      u->max_outdeg = std::max(u->max_outdeg, gf.max_outdeg);
      u->max_indeg = std::max(u->max_indeg, gf.max_indeg);
      u->has_eps = u->has_eps || gf.has_eps;
      u->same_col = u->same_col && gf.same_col;
      u->ladder = u->ladder && gf.ladder;
      plan_utt_on_graph(u, i, T, S, gf);
    }
    gt.in_off[NS] = NA;
    std::vector<int32_t> startv(start, start + n_utt), gidx((size_t)n_utt);
    for (int i = 0; i < n_utt; ++i) gidx[(size_t)i] = i;
    std::vector<float> finalv(final_w, final_w + NS);
    rc = u_upload(ctx, u, &u->state_off_d, u->state_off);
    if (!rc) rc = u_upload(ctx, u, &u->start_d, startv);
    if (!rc) rc = u_upload(ctx, u, &u->gidx_d, gidx);
    if (!rc) rc = u_upload(ctx, u, &u->in_off_d, gt.in_off);
    if (!rc) rc = u_upload(ctx, u, &u->out_off_d, out_off);
    if (!rc) rc = u_upload(ctx, u, &u->in_src_d, gt.in_src);
    if (!rc) rc = u_upload(ctx, u, &u->in_col_d, gt.in_col);
    if (!rc) rc = u_upload(ctx, u, &u->in_tid_d, gt.in_tid);
    if (!rc) rc = u_upload(ctx, u, &u->in_olabel_d, gt.in_ol);
    if (!rc) rc = u_upload(ctx, u, &u->out_inidx_d, gt.out_inidx);
    if (!rc) rc = u_upload(ctx, u, &u->in_w_d, gt.in_w);
    if (!rc) rc = u_upload(ctx, u, &u->final_d, finalv);
    if (!rc) rc = u_upload(ctx, u, &u->bp_off_d, u->bp_off);
    if (!rc) rc = u_upload(ctx, u, &u->path_off_d, u->path_off);
    if (!rc) rc = u_upload(ctx, u, &u->words_off_d, u->words_off);
    if (rc) { khg_utts_destroy(u); return rc; }
    u->graph_bytes = graph_table_bytes(n_utt, NS, NA);
  }
  return utts_finish(ctx, u, out);
}

// ---- one decoding graph shared by many utterances (and by many sets) ---------------------------------------------------------
extern "C" int khg_graph_create(khg_ctx* ctx, const khg_tm* tm, int32_t num_states, int32_t start, const int64_t* arc_off,
                                const int32_t* ilabel, const int32_t* olabel, const float* weight, const int32_t* nextstate,
                                const float* final_w, khg_graph** out) {
  if (ctx_dead(ctx) || !out || num_states <= 0)
    return khg_set_error(KHG_E_ARG, "khg_graph_create: bad arguments");
  if (!tm || !arc_off || !ilabel || !olabel || !weight || !nextstate || !final_w)
    return khg_set_error(KHG_E_ARG, "khg_graph_create: graph arrays / tm missing");
  const int64_t S = num_states, A = arc_off[S] - arc_off[0];
  if (arc_off[0] != 0) return khg_set_error(KHG_E_ARG, "khg_graph_create: arc_off[0] != 0");
  for (int64_t s = 0; s < S; ++s)
    if (arc_off[s + 1] < arc_off[s]) return khg_set_error(KHG_E_ARG, "khg_graph_create: offsets not monotone");
  GraphTables gt;
  gt.size(S, A);
  GraphFacts gf;
  std::string msg;
  int rc = plan_graph("khg_graph_create", tm, false, 0, S, start, arc_off, ilabel, olabel, weight, nextstate, final_w, &gt, &gf, &msg);
  if (rc) return khg_set_error(rc, msg);
  gt.in_off[S] = A;
  khg_graph* g = new khg_graph();
  g->ctx = ctx; g->S = S; g->A = A; g->start = start; g->nwords = gf.nwords;
  g->max_indeg = gf.max_indeg; g->max_outdeg = gf.max_outdeg; g->same_col = gf.same_col; g->ladder = gf.ladder; g->has_eps = gf.has_eps;
  g->pdfs = gf.pdfs; g->pdf_first = gf.pdf_first; g->pdf_dfin = gf.pdf_dfin;
  std::vector<int64_t> so{0, S}, out_off(arc_off, arc_off + S + 1);
  std::vector<int32_t> startv{start};
  std::vector<float> finalv(final_w, final_w + S);
  rc = dev_upload(ctx, &g->state_off_d, so);
  if (!rc) rc = dev_upload(ctx, &g->start_d, startv);
  if (!rc) rc = dev_upload(ctx, &g->in_off_d, gt.in_off);
  if (!rc) rc = dev_upload(ctx, &g->out_off_d, out_off);
  if (!rc) rc = dev_upload(ctx, &g->in_src_d, gt.in_src);
  if (!rc) rc = dev_upload(ctx, &g->in_col_d, gt.in_col);
  if (!rc) rc = dev_upload(ctx, &g->in_tid_d, gt.in_tid);
  if (!rc) rc = dev_upload(ctx, &g->in_olabel_d, gt.in_ol);
  if (!rc) rc = dev_upload(ctx, &g->out_inidx_d, gt.out_inidx);
  if (!rc) rc = dev_upload(ctx, &g->in_w_d, gt.in_w);
  if (!rc) rc = dev_upload(ctx, &g->final_d, finalv);
  if (!rc) rc = sync_pageable(ctx);        // the caller's arrays and the vectors above are free after this
  if (rc) { khg_graph_release(g); return rc; }
  g->device_bytes = graph_table_bytes(1, S, A);
  *out = g;
  return KHG_OK;
}
void khg_graph_release(khg_graph* g) {
  if (!g || --g->refs > 0) return;
  DEVFREE(g->state_off_d); DEVFREE(g->start_d); DEVFREE(g->in_off_d); DEVFREE(g->out_off_d); DEVFREE(g->in_src_d); DEVFREE(g->in_col_d);
  DEVFREE(g->in_tid_d); DEVFREE(g->in_olabel_d); DEVFREE(g->out_inidx_d); DEVFREE(g->in_w_d); DEVFREE(g->final_d);
  delete g;
}
extern "C" int khg_graph_destroy(khg_graph* g) {
  khg_graph_release(g);
  return KHG_OK;
}
extern "C" int khg_graph_info(const khg_graph* g, int64_t* num_states, int64_t* num_arcs, int32_t* num_pdfs, int32_t* max_in_degree,
                              int64_t* device_bytes) {
  if (!g) return khg_set_error(KHG_E_ARG, "khg_graph_info: bad arguments");
  if (num_states) *num_states = g->S;
  if (num_arcs) *num_arcs = g->A;
  if (num_pdfs) *num_pdfs = (int32_t)g->pdfs.size();
  if (max_in_degree) *max_in_degree = g->max_indeg;
  if (device_bytes) *device_bytes = g->device_bytes;
  return KHG_OK;
}

extern "C" int khg_utts_create_on_graph(khg_ctx* ctx, const khg_tm* tm, khg_graph* g, int32_t n_utt, int32_t D, const int64_t* frame_off,
                                        const float* feats_h, const float* feats_dv, khg_utts** out) {
  (void)tm;      // (the graph was planned against its transition table)
  if (ctx_dead(ctx) || !out || !g || n_utt <= 0 || D <= 0 || !frame_off || (!feats_h && !feats_dv))
    return khg_set_error(KHG_E_ARG, "khg_utts_create_on_graph: bad arguments");
  if (g->ctx != ctx)
    return khg_set_error(KHG_E_ARG, "khg_utts_create_on_graph: a decoding graph must be used with the context that created it");
  khg_utts* u = nullptr;
  int rc = utts_begin("khg_utts_create_on_graph", ctx, n_utt, D, frame_off, feats_h, feats_dv, g->S <= 32768 && g->A <= 65536, &u);
  if (rc) return rc;
  u->has_graphs = true;
  u->graph = g; ++g->refs;
  u->state_off.assign({0, g->S});
  u->max_states = (int32_t)g->S; u->max_inarcs = (int32_t)g->A; u->max_indeg = g->max_indeg; u->max_outdeg = g->max_outdeg;
  u->has_eps = g->has_eps; u->same_col = g->same_col; u->ladder = g->ladder;
  u->bp_off.assign(n_utt + 1, 0); u->path_off.assign(n_utt + 1, 0); u->words_off.assign(n_utt + 1, 0);
  GraphFacts gf;
  gf.pdfs = g->pdfs; gf.pdf_first = g->pdf_first; gf.pdf_dfin = g->pdf_dfin; gf.nwords = g->nwords;
  for (int i = 0; i < n_utt; ++i) plan_utt_on_graph(u, i, frame_off[i + 1] - frame_off[i], g->S, gf);
  // the graph's tables, borrowed: khg_utts_destroy releases the reference instead of freeing them
  u->state_off_d = g->state_off_d; u->start_d = g->start_d; u->in_off_d = g->in_off_d; u->out_off_d = g->out_off_d;
  u->in_src_d = g->in_src_d; u->in_col_d = g->in_col_d; u->in_tid_d = g->in_tid_d; u->in_olabel_d = g->in_olabel_d;
  u->out_inidx_d = g->out_inidx_d; u->in_w_d = g->in_w_d; u->final_d = g->final_d;
  std::vector<int32_t> gidx((size_t)n_utt, 0);
  rc = u_upload(ctx, u, &u->gidx_d, gidx);
  if (!rc) rc = u_upload(ctx, u, &u->bp_off_d, u->bp_off);
  if (!rc) rc = u_upload(ctx, u, &u->path_off_d, u->path_off);
  if (!rc) rc = u_upload(ctx, u, &u->words_off_d, u->words_off);
  if (rc) { khg_utts_destroy(u); return rc; }
  return utts_finish(ctx, u, out);
}
extern "C" int khg_utts_graph_bytes(const khg_utts* u, int64_t* bytes) {
  if (!u || !bytes) return khg_set_error(KHG_E_ARG, "khg_utts_graph_bytes: bad arguments");
  *bytes = u->graph_bytes;
  return KHG_OK;
}

extern "C" int khg_utts_set_pdf_list(khg_utts* u, int32_t n, const int32_t* pdfs) {
  if (!u || n <= 0 || !pdfs) return khg_set_error(KHG_E_ARG, "khg_utts_set_pdf_list: bad arguments");
  if (u->has_graphs) return khg_set_error(KHG_E_ARG, "khg_utts_set_pdf_list: set has graphs; its pdf lists come from them");
  u->pdfs.clear();
  u->pdf_first.clear(); u->pdf_last.clear();     // no graphs behind an explicit list: every frame is needed
  for (int i = 0; i < u->n_utt; ++i) { u->pdf_off[i + 1] = u->pdf_off[i] + n; u->pdfs.insert(u->pdfs.end(), pdfs, pdfs + n); }
  plan_ll(u);
  DEVFREE(u->pdf_off_d); DEVFREE(u->pdfs_d); DEVFREE(u->ll_off_d); DEVFREE(u->ll_d);
  k1_lists_changed(u);
  u->pdfs_checked_P = -1;      // (the id range check is cached per model size)
  u->ll_valid = false;
  return KHG_OK;
}

// Borrowed device features were rewritten in place: drop everything derived from them (column maxima, the fp16 / bf16 planes of the
// split K1 forms, K3's split feature records); the next khg_loglikes / khg_acc_stats re-packs.  The fp32 K1 forms and every K3 form
// but k3_accumulate_wave16 on its records read feats_d live.
extern "C" int khg_utts_features_changed(khg_utts* u) {
  if (!u) return khg_set_error(KHG_E_ARG, "khg_utts_features_changed: bad arguments");
  k1_features_changed(u);
  u->k3x_key.clear();                 // (the buffer stays: same N, the next pass fills it again)
  u->ll_valid = false;
  return KHG_OK;
}

int utts_foreign_ctx(const khg_ctx* ctx, const khg_utts* u, const char* where) {
  if (u && u->small && u->ctx != ctx)
    return khg_set_error(KHG_E_ARG, std::string(where) + ": a small utterance set (<= 16 utterances: scratch in its context's arena) must be used with the context that created it");
  return KHG_OK;
}

extern "C" int khg_utts_destroy(khg_utts* u) {
  if (!u) return KHG_OK;
  if (u->small && u->ctx && khg_ctx_alive(u->ctx)) {      // (a handle may be destroyed after its context: nothing is in flight then)
    // arena scratch is reused by the next set at once (hipFree would have waited for the device): nothing of this set may be in flight
    khg_ctx* c = u->ctx;
    for (int i = 0; i < khg_ctx::NSIDE; ++i)
      if (c->side_dirty[i]) { (void)hipStreamSynchronize(c->sides[i]); c->side_dirty[i] = false; }
    (void)hipStreamSynchronize(c->stream);
    c->pageable_pending = false;
  }
  if (u->out_blk_d) {                      // ali / words / like / status live inside one block (small sets)
    u->ali_d = nullptr; u->words_d = nullptr; u->num_words_d = nullptr; u->status_d = nullptr; u->like_d = nullptr;
    DEVFREE(u->out_blk_d);
  }
  if (u->own_feats) DEVFREE(u->feats_d);
  if (u->graph) {                          // borrowed tables: the graph frees them with its last reference
    u->state_off_d = nullptr; u->start_d = nullptr; u->in_off_d = nullptr; u->out_off_d = nullptr; u->in_src_d = nullptr; u->in_col_d = nullptr;
    u->in_tid_d = nullptr; u->in_olabel_d = nullptr; u->out_inidx_d = nullptr; u->in_w_d = nullptr; u->final_d = nullptr;
    khg_graph_release(u->graph); u->graph = nullptr;
  }
  DEVFREE(u->gidx_d);
  DEVFREE(u->frame_off_d); DEVFREE(u->state_off_d); DEVFREE(u->pdf_off_d); DEVFREE(u->ll_off_d);
  DEVFREE(u->pdfs_d); DEVFREE(u->start_d); DEVFREE(u->in_off_d); DEVFREE(u->out_off_d);
  DEVFREE(u->in_src_d); DEVFREE(u->in_col_d); DEVFREE(u->in_tid_d); DEVFREE(u->in_olabel_d); DEVFREE(u->out_inidx_d);
  DEVFREE(u->in_w_d); DEVFREE(u->final_d); DEVFREE(u->ll_d);
  DEVFREE(u->bp_d); DEVFREE(u->bp_off_d); DEVFREE(u->path_off_d); DEVFREE(u->words_off_d);
  DEVFREE(u->ali2_d); DEVFREE(u->unc_d); DEVFREE(u->sub_off_d);
  if (u->unc_cnt_h) { (void)hipHostFree(u->unc_cnt_h); u->unc_cnt_h = nullptr; }
  DEVFREE(u->layer_best_d); DEVFREE(u->layer_cnt_d); DEVFREE(u->path_d); DEVFREE(u->k2_gscratch_d); DEVFREE(u->k2_order_d);
  DEVFREE(u->ali_d); DEVFREE(u->words_d); DEVFREE(u->num_words_d); DEVFREE(u->status_d); DEVFREE(u->like_d);
  DEVFREE(u->pdf_count_d); DEVFREE(u->pdf_cursor_d); DEVFREE(u->frame_ids_d); DEVFREE(u->pdf_start_d); DEVFREE(u->tid_count_d);
  DEVFREE(u->sort_keys_d); DEVFREE(u->sort_keys_out_d); DEVFREE(u->sort_vals_d); DEVFREE(u->sort_tmp_d); DEVFREE(u->cs_hist_d); DEVFREE(u->cs_tot_d);
  DEVFREE(u->k3x_d); DEVFREE(u->k3_part_d); DEVFREE(u->k3_llpart_d); DEVFREE(u->k3_items_d); DEVFREE(u->k3_item_off_d);
  DEVFREE(u->pe_row_d); DEVFREE(u->pe_tid_d); DEVFREE(u->pe_ids_d); DEVFREE(u->pe_w_d); DEVFREE(u->pe_keys_d); DEVFREE(u->pe_keys_out_d);
  DEVFREE(u->pe_vals_d); DEVFREE(u->pe_tmp_d); DEVFREE(u->pe_start_d);
  DEVFREE(u->rc_keys_d); DEVFREE(u->rc_keys_out_d); DEVFREE(u->rc_vals_d); DEVFREE(u->rc_vals_out_d); DEVFREE(u->rc_flag_d); DEVFREE(u->rc_inc_d);
  DEVFREE(u->rc_row_d); DEVFREE(u->rc_cell_d); DEVFREE(u->rc_tmp_d); DEVFREE(u->rc_cell_start_d); DEVFREE(u->rc_item_off_d); DEVFREE(u->rc_stats_d);
  k1_free(u);
  if (u->ev_dp) (void)hipEventDestroy(u->ev_dp);
  if (u->ev_ali) (void)hipEventDestroy(u->ev_ali);
  delete u;
  return KHG_OK;
}
extern "C" int khg_utts_num_pdfs(const khg_utts* u, int64_t* pdf_off) {
  if (!u || !pdf_off) return khg_set_error(KHG_E_ARG, "bad arguments");
  std::copy(u->pdf_off.begin(), u->pdf_off.end(), pdf_off);
  return KHG_OK;
}
extern "C" int khg_utts_pdfs(const khg_utts* u, int32_t* pdfs) {
  if (!u || !pdfs) return khg_set_error(KHG_E_ARG, "bad arguments");
  std::copy(u->pdfs.begin(), u->pdfs.end(), pdfs);
  return KHG_OK;
}

// the main stream must not touch ali / status / the ll buffer while the side-stream decoder runs
// split mode: the alignments the order-faithful decoders wrote to their own buffer go into the set's alignment
__global__ void k2_merge_fallback(const int32_t* __restrict__ unc, const int64_t* __restrict__ frame_off, const int32_t* __restrict__ ali2,
                                  int32_t* __restrict__ ali, int n_utt) {
  for (int u = blockIdx.x; u < n_utt; u += gridDim.x) {
    if (!unc[u]) continue;
    const int64_t f0 = frame_off[u], f1 = frame_off[u + 1];
    for (int64_t f = f0 + threadIdx.x; f < f1; f += blockDim.x) ali[f] = ali2[f];
  }
}
int wait_ali(khg_ctx* ctx, khg_utts* u) {
  if (u->ali_pending) { HIPCHK(hipStreamWaitEvent(ctx->stream, u->ev_ali, 0)); u->ali_pending = false; }
  if (u->ali_split) {
    u->ali_split = false;
    KHG_LAUNCH(ctx, k2_merge_fallback, dim3((unsigned)std::min(u->n_utt, 16384)), dim3(64), 0, ctx->stream, u->unc_d, u->frame_off_d, u->ali2_d, u->ali_d, u->n_utt);
    HIPCHK(hipGetLastError());
  }
  return KHG_OK;
}
