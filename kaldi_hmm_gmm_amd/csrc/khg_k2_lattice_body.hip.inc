// The body of k2_lattice_faster and k2_lattice_faster_lat (khg_k2_lattice.hip.inc includes it into both, with LAT false / true and
// utt_tot in scope, under `fp contract(off)`): the text of the decoder kernel once, so that the kernel without a lattice compiles exactly as before.
  // one lane runs the reference's serial token passing; the other lanes of the wave have nothing to do
  if (threadIdx.x != 0) return;
  const int k = u0 + (int)blockIdx.x;
  const int u = a.list[k];
  const int64_t f0 = a.frame_off[u];
  const int T = (int)(a.frame_off[u + 1] - f0);
  const int tpad = (T + 31) & ~31;
  const int64_t s0 = a.state_off[a.gidx[u]];
  const int S = (int)(a.state_off[a.gidx[u] + 1] - s0);
  const int64_t in0 = a.in_off[s0];
  const int A = (int)(a.in_off[s0 + S] - in0);
  const float* llu = a.ll + a.ll_off[u];
  const int TC = a.tok_cap[k], LC = a.link_cap[k];
  const LatLayout L = lat_layout(T, S, a.amax, a.hb, TC, LC, LAT);
  (void)A;
  unsigned char* base = a.scratch + a.scr_off[k];
  LatTok* tk = reinterpret_cast<LatTok*>(base + L.toks);
  LatLink* lk = reinterpret_cast<LatLink*>(base + L.links);
  LatElem* pools[2] = {reinterpret_cast<LatElem*>(base + L.elems0), reinterpret_cast<LatElem*>(base + L.elems1)};
  int32_t* b_last = reinterpret_cast<int32_t*>(base + L.blast);
  int32_t* b_prev = reinterpret_cast<int32_t*>(base + L.bprev);
  int32_t* queue = reinterpret_cast<int32_t*>(base + L.queue);
  float* tmp = reinterpret_cast<float*>(base + L.tmp);
  int32_t* dst = reinterpret_cast<int32_t*>(base + L.dst);
  int32_t* nieps = reinterpret_cast<int32_t*>(base + L.nieps);
  int32_t* fhead = reinterpret_cast<int32_t*>(base + L.fhead);
  int32_t* fflags = reinterpret_cast<int32_t*>(base + L.fflags);     // bit 0 must_prune_forward_links, bit 1 must_prune_tokens
  float* coff = reinterpret_cast<float*>(base + L.coff);
  int32_t* ord = reinterpret_cast<int32_t*>(base + L.ord);
  int32_t* rpb[2] = {reinterpret_cast<int32_t*>(base + L.rp0), reinterpret_cast<int32_t*>(base + L.rp1)};
  int32_t* slot = reinterpret_cast<int32_t*>(base + L.slot);
  int32_t* gst = reinterpret_cast<int32_t*>(base + L.gst);        // (LAT only, as the four below)
  int32_t* stok = reinterpret_cast<int32_t*>(base + L.stok);
  int32_t* sfr = reinterpret_cast<int32_t*>(base + L.sfr);
  int32_t* sarc = reinterpret_cast<int32_t*>(base + L.sarc);
  int32_t* fbase = reinterpret_cast<int32_t*>(base + L.fbase);
  if constexpr (LAT) { utt_tot[2 * (int64_t)blockIdx.x] = 0; utt_tot[2 * (int64_t)blockIdx.x + 1] = 0; }
  const float INF = __builtin_huge_valf();

  auto fail = [&](int st) {
    for (int t = 0; t < T; ++t) a.ali[f0 + t] = 0;
    a.num_words[u] = 0;
    a.like[u] = 0.0;
    a.status[u] = st;
  };
  // graph tables: destination of every in-arc, input-epsilon count of every state (fst_->NumInputEpsilons)
  for (int s = 0; s < S; ++s) {
    for (int64_t i = a.in_off[s0 + s]; i < a.in_off[s0 + s + 1]; ++i) dst[i - in0] = s;
    int n = 0;
    for (int64_t oa = a.out_off[s0 + s]; oa < a.out_off[s0 + s + 1]; ++oa) n += a.in_col[in0 + a.out_inidx[oa]] < 0;
    nieps[s] = n;
  }
  auto arc_w = [&](int ai) {
    float w = a.in_w[in0 + ai];
    const int tid = a.in_tid[in0 + ai];
    if (a.trans_cost && tid >= 1) w = w + a.trans_cost[tid];
    return w;
  };
  auto loglike = [&](int ai, int frame) { return a.acoustic_scale * llu[(int64_t)a.in_col[in0 + ai] * tpad + frame]; };

  // ---- pools (token_pool_ / forward_link_pool_) ----
  int tok_n = 0, tok_free = -1, link_n = 0, link_free = -1;
  bool oom = false;
  auto new_tok = [&](float tot, int frame) -> int {
    int t;
    if (tok_free >= 0) { t = tok_free; tok_free = tk[t].next; }
    else if (tok_n < TC) t = tok_n++;
    else { oom = true; return -1; }
    tk[t].tot = tot; tk[t].extra = 0.0f; tk[t].fcost = INF; tk[t].links = -1; tk[t].flags = 0;
    tk[t].next = fhead[frame]; fhead[frame] = t;     // put at the head of the frame's list
    return t;
  };
  auto free_tok = [&](int t) { tk[t].next = tok_free; tok_free = t; };
  auto new_link = [&](int from, int next_tok, int il, int ol, float g, float ac) -> bool {
    int l;
    if (link_free >= 0) { l = link_free; link_free = lk[l].next; }
    else if (link_n < LC) l = link_n++;
    else { oom = true; return false; }
    lk[l].next_tok = next_tok; lk[l].ilabel = il; lk[l].olabel = ol; lk[l].graph_cost = g; lk[l].acoustic_cost = ac;
    lk[l].next = tk[from].links; tk[from].links = l;
    return true;
  };
  auto delete_links = [&](int t) {
    for (int l = tk[t].links; l >= 0;) { int m = lk[l].next; lk[l].next = link_free; link_free = l; l = m; }
    tk[t].links = -1;
  };

  // ---- HashList (hash-list-inl.h) ----
  // (the HashList of khg_k2_viterbi.hip.inc, shared with k2_viterbi_faithful)
  int cur = 0;                             // pool of the list being built
  K2HashList<LatElem> hl{pools[0], 0, 1000, b_last, b_prev, -1, -1};   // :36 toks_.SetSize(1000)
  hl.init(a.hb);
  size_t& hash_size = hl.hash_size;
  int& list_head = hl.list_head;
  auto hl_insert = [&](int key, bool* is_new) -> int {     // FindOrAddToken's toks_.Insert(state, NULL)
    const int e = hl.insert(key, is_new);
    if (*is_new) hl.pool[e].val = -1;
    return e;
  };
  auto hl_clear = [&]() -> int { return hl.clear(); };

  // ProcessNonemitting (:840-905) on the list being built, tokens of frame `fp1`
  auto process_nonemitting = [&](float cutoff, int fp1) {
    LatElem* pool = pools[cur];
    int qn = 0;
    for (int e = list_head; e >= 0; e = pool[e].tail)
      if (nieps[pool[e].key] != 0) { if (qn < L.qcap) queue[qn++] = e; else oom = true; }
    while (qn && !oom) {
      const int e = queue[--qn];
      const int state = pool[e].key;
      const int tok = pool[e].val;
      const float cur_cost = tk[tok].tot;
      if (cur_cost >= cutoff) continue;
      delete_links(tok);                   // necessary when re-visiting
      for (int64_t oa = a.out_off[s0 + state]; oa < a.out_off[s0 + state + 1]; ++oa) {
        const int ai = a.out_inidx[oa];
        if (a.in_col[in0 + ai] >= 0) continue;      // propagate nonemitting only
        const float graph_cost = arc_w(ai), tot_cost = cur_cost + graph_cost;
        if (tot_cost < cutoff) {
          const int ns = dst[ai];
          bool is_new, changed;
          const int en = hl_insert(ns, &is_new);
          if (pool[en].val < 0) {
            const int nt = new_tok(tot_cost, fp1);
            if (nt < 0) return;
            if constexpr (LAT) gst[nt] = ns;
            pool[en].val = nt; changed = true;
          } else if (tk[pool[en].val].tot > tot_cost) {
            tk[pool[en].val].tot = tot_cost; changed = true;
          } else {
            changed = false;
          }
          if (!new_link(tok, pool[en].val, 0, a.in_olabel[in0 + ai], graph_cost, 0.0f)) return;
          if (changed && nieps[ns] != 0) { if (qn < L.qcap) queue[qn++] = en; else { oom = true; return; } }
        }
      }
    }
  };

  // PruneForwardLinks (:305-380) -> bit 0 extra_costs_changed, bit 1 links_pruned
  auto prune_forward_links = [&](int f, float delta) -> int {
    int res = 0;
    bool changed = true;
    while (changed) {
      changed = false;
      for (int t = fhead[f]; t >= 0; t = tk[t].next) {
        float tok_extra_cost = INF;
        int prev = -1;
        for (int l = tk[t].links; l >= 0;) {
          const int nt = lk[l].next_tok;
          float lec = tk[nt].extra + ((tk[t].tot + lk[l].acoustic_cost + lk[l].graph_cost) - tk[nt].tot);
          if (lec > a.lattice_beam) {
            const int nl = lk[l].next;
            if (prev >= 0) lk[prev].next = nl; else tk[t].links = nl;
            lk[l].next = link_free; link_free = l;
            l = nl;
            res |= 2;
          } else {
            if (lec < 0.0f) lec = 0.0f;
            if (lec < tok_extra_cost) tok_extra_cost = lec;
            prev = l;
            l = lk[l].next;
          }
        }
        if (fabsf(tok_extra_cost - tk[t].extra) > delta) changed = true;
        tk[t].extra = tok_extra_cost;
      }
      if (changed) res |= 1;
    }
    return res;
  };
  // PruneTokensForFrame (:492-513)
  auto prune_tokens_for_frame = [&](int f) {
    int prev = -1;
    for (int t = fhead[f], nx; t >= 0; t = nx) {
      nx = tk[t].next;
      if (tk[t].extra == INF) {
        if (prev >= 0) tk[prev].next = nx; else fhead[f] = nx;
        free_tok(t);
      } else {
        prev = t;
      }
    }
  };

  // ---- InitDecoding (:61-80) ----
  for (int f = 0; f <= T; ++f) { fhead[f] = -1; fflags[f] = 3; coff[f] = 0.0f; }
  {
    const int st = new_tok(0.0f, 0);
    if constexpr (LAT) gst[st] = a.start[a.gidx[u]];
    bool nw;
    const int e = hl_insert(a.start[a.gidx[u]], &nw);
    pools[cur][e].val = st;
    process_nonemitting(a.beam, 0);
  }
  // ---- AdvanceDecoding (:591-633) ----
  for (int frame = 0; frame < T && !oom; ++frame) {
    if (frame % a.prune_interval == 0) {    // PruneActiveTokens(lattice_beam * prune_scale) (:521-548)
      const float delta = a.lattice_beam * a.prune_scale;
      for (int f = frame - 1; f >= 0; --f) {
        if (fflags[f] & 1) {
          const int r = prune_forward_links(f, delta);
          if ((r & 1) && f > 0) fflags[f - 1] |= 1;
          if (r & 2) fflags[f] |= 2;
          fflags[f] &= ~1;
        }
        if (f + 1 < frame && (fflags[f + 1] & 2)) { prune_tokens_for_frame(f + 1); fflags[f + 1] &= ~2; }
      }
    }
    // ProcessEmitting (:730-825)
    LatElem* last = pools[cur];
    const int last_head = hl_clear();
    cur ^= 1; hl.pool = pools[cur]; hl.pool_n = 0;
    LatElem* pool = pools[cur];
    // GetCutoff (:657-727)
    float best_weight = INF;
    int best_elem = -1;
    int count = 0;
    float cur_cutoff, adaptive_beam;
    if (a.max_active == INT32_MAX && a.min_active == 0) {
      for (int e = last_head; e >= 0; e = last[e].tail, ++count) {
        const float w = tk[last[e].val].tot;
        if (w < best_weight) { best_weight = w; best_elem = e; }
      }
      adaptive_beam = a.beam;
      cur_cutoff = best_weight + a.beam;
    } else {
      for (int e = last_head; e >= 0; e = last[e].tail, ++count) {
        const float w = tk[last[e].val].tot;
        tmp[count] = w;
        if (w < best_weight) { best_weight = w; best_elem = e; }
      }
      const float beam_cutoff = best_weight + a.beam;
      float min_active_cutoff = INF, max_active_cutoff = INF;
      int limit = count;
      if (count > a.max_active) { max_active_cutoff = lat_kth(tmp, count, a.max_active); limit = a.max_active; }
      if (max_active_cutoff < beam_cutoff) {
        adaptive_beam = max_active_cutoff - best_weight + a.beam_delta;
        cur_cutoff = max_active_cutoff;
      } else {
        if (count > a.min_active) {
          if (a.min_active == 0) min_active_cutoff = best_weight;
          else min_active_cutoff = lat_kth(tmp, limit, a.min_active);
        }
        if (min_active_cutoff > beam_cutoff) {
          adaptive_beam = min_active_cutoff - best_weight + a.beam_delta;
          cur_cutoff = min_active_cutoff;
        } else {
          adaptive_beam = a.beam;
          cur_cutoff = beam_cutoff;
        }
      }
    }
    {   // PossiblyResizeHash (:221-228)
      const size_t new_sz = (size_t)((float)count * a.hash_ratio);
      if (new_sz > hash_size) hash_size = new_sz;
    }
    float next_cutoff = INF, cost_offset = 0.0f;
    if (best_elem >= 0) {
      const int state = last[best_elem].key;
      const float tot = tk[last[best_elem].val].tot;
      cost_offset = -tot;
      for (int64_t oa = a.out_off[s0 + state]; oa < a.out_off[s0 + state + 1]; ++oa) {
        const int ai = a.out_inidx[oa];
        if (a.in_col[in0 + ai] < 0) continue;
        const float new_weight = arc_w(ai) + cost_offset - loglike(ai, frame) + tot;
        if (new_weight + adaptive_beam < next_cutoff) next_cutoff = new_weight + adaptive_beam;
      }
    }
    coff[frame] = cost_offset;
    for (int e = last_head; e >= 0 && !oom; e = last[e].tail) {
      const int state = last[e].key;
      const int tok = last[e].val;
      if (!(tk[tok].tot <= cur_cutoff)) continue;
      for (int64_t oa = a.out_off[s0 + state]; oa < a.out_off[s0 + state + 1]; ++oa) {
        const int ai = a.out_inidx[oa];
        if (a.in_col[in0 + ai] < 0) continue;
        const float ac_cost = cost_offset - loglike(ai, frame), graph_cost = arc_w(ai), cur_cost = tk[tok].tot,
                    tot_cost = cur_cost + ac_cost + graph_cost;
        if (tot_cost >= next_cutoff) continue;
        else if (tot_cost + adaptive_beam < next_cutoff) next_cutoff = tot_cost + adaptive_beam;
        // FindOrAddToken (:254-299)
        const int ns = dst[ai];
        bool is_new;
        const int en = hl_insert(ns, &is_new);
        if (pool[en].val < 0) {
          const int nt = new_tok(tot_cost, frame + 1);
          if (nt < 0) break;
          if constexpr (LAT) gst[nt] = ns;
          pool[en].val = nt;
        } else if (tk[pool[en].val].tot > tot_cost) {
          tk[pool[en].val].tot = tot_cost;
        }
        if (!new_link(tok, pool[en].val, a.in_tid[in0 + ai], a.in_olabel[in0 + ai], graph_cost, ac_cost)) break;
      }
    }
    if (oom) break;
    process_nonemitting(next_cutoff, frame + 1);
  }
  if (oom) { fail(KHG_LAT_SCRATCH); return; }

  // ---- FinalizeDecoding (:639-653): PruneForwardLinksFinal with ComputeFinalCosts (:551-588) ----
  float final_relative_cost, final_best_cost;
  bool any_final = false;
  {
    LatElem* pool = pools[cur];
    float best_cost = INF, best_cost_with_final = INF;
    for (int e = list_head; e >= 0; e = pool[e].tail) {
      const float final_cost = a.final_w[s0 + pool[e].key];
      const int tok = pool[e].val;
      const float cost = tk[tok].tot, cost_with_final = cost + final_cost;
      best_cost = fminf(cost, best_cost);
      best_cost_with_final = fminf(cost_with_final, best_cost_with_final);
      if (final_cost != INF) { tk[tok].fcost = final_cost; any_final = true; }
    }
    final_relative_cost = (best_cost == INF && best_cost_with_final == INF) ? INF : best_cost_with_final - best_cost;
    final_best_cost = best_cost_with_final != INF ? best_cost_with_final : best_cost;
    hl_clear();
  }
  {
    bool changed = true;
    while (changed) {
      changed = false;
      for (int t = fhead[T]; t >= 0; t = tk[t].next) {
        const float final_cost = any_final ? tk[t].fcost : 0.0f;
        float tok_extra_cost = tk[t].tot + final_cost - final_best_cost;
        int prev = -1;
        for (int l = tk[t].links; l >= 0;) {
          const int nt = lk[l].next_tok;
          float lec = tk[nt].extra + ((tk[t].tot + lk[l].acoustic_cost + lk[l].graph_cost) - tk[nt].tot);
          if (lec > a.lattice_beam) {
            const int nl = lk[l].next;
            if (prev >= 0) lk[prev].next = nl; else tk[t].links = nl;
            lk[l].next = link_free; link_free = l;
            l = nl;
          } else {
            if (lec < 0.0f) lec = 0.0f;
            if (lec < tok_extra_cost) tok_extra_cost = lec;
            prev = l;
            l = lk[l].next;
          }
        }
        if (tok_extra_cost > a.lattice_beam) tok_extra_cost = INF;
        {   // ApproxEqual(extra, tok_extra_cost, 1e-5) (kaldi-math.h:102-110)
          const float x = tk[t].extra, y = tok_extra_cost;
          bool eq = x == y;
          if (!eq) {
            const float diff = fabsf(x - y);
            eq = !(diff == INF || diff != diff) && diff <= 1.0e-05f * (fabsf(x) + fabsf(y));
          }
          if (!eq) changed = true;
        }
        tk[t].extra = tok_extra_cost;
      }
    }
  }
  for (int f = T - 1; f >= 0; --f) {
    prune_forward_links(f, 0.0f);
    prune_tokens_for_frame(f + 1);
  }
  prune_tokens_for_frame(0);

  // ---- DecodeUtteranceLatticeFaster (decoder-wrappers.cc:186-224) ----
  if (fhead[T] < 0) { fail(KHG_LAT_NO_PATH); return; }                  // Decode() == false
  const bool reached = final_relative_cost != INF;
  if (!reached && !a.allow_partial) { fail(KHG_LAT_PARTIAL); return; }
  const int partial = reached ? 0 : KHG_LAT_PARTIAL;

  // ---- GetRawLattice + ShortestPath ----
  for (int f = 0; f <= T; ++f) {
    if (fhead[f] < 0) { fail(KHG_LAT_NO_TRACEBACK | partial); return; }    // "no tokens active on frame": empty lattice
    for (int t = fhead[f]; t >= 0; t = tk[t].next) tk[t].flags = 0;
  }
  float fd1 = INF, fd2 = INF;
  int f_parent = -1, start_tok = -1;
  int n_states = 0, n_arcs = 0;       // (LAT) GetRawLattice's states and arcs so far: the prefix sums the emission needs, for free
  for (int f = 0; f <= T; ++f) {
    if constexpr (LAT) fbase[f] = n_states;
    // TopSortTokens (:935-1013)
    int num = 0;
    for (int t = fhead[f]; t >= 0; t = tk[t].next) ++num;
    {
      int p = num;
      for (int t = fhead[f]; t >= 0; t = tk[t].next) { tk[t].pos = --p; ord[p] = t; }
    }
    int cur_pos = num, nrp = 0;
    int* rp = rpb[0];
    bool over = false;
    auto visit = [&](int t) {
      const int pos = tk[t].pos;
      for (int l = tk[t].links; l >= 0; l = lk[l].next) {
        if (lk[l].ilabel != 0) continue;
        const int nt = lk[l].next_tok;          // an epsilon link never leaves its frame
        if (tk[nt].pos < pos) {
          if (cur_pos >= L.slotcap) { over = true; return; }
          tk[nt].pos = cur_pos++;
          if (!(tk[nt].flags & LAT_F_RP)) {
            if (nrp >= L.rpcap) { over = true; return; }
            tk[nt].flags |= LAT_F_RP; tk[nt].rp_slot = nrp; rp[nrp++] = nt;
          }
        }
      }
    };
    for (int i = 0; i < num && !over; ++i) { const int t = ord[i]; visit(t); tk[t].flags &= ~LAT_F_RP; }
    // An acyclic frame settles in at most `num` reprocessing rounds (each round fixes the next token along the longest epsilon
    // chain); the reference stops at 1e6 rounds with "Epsilon loops exist in your decoding graph" -- more than num + 1 is that case.
    int loops = 0;
    bool eps_loop = false;
    while (!over) {
      if (loops > num + 1) { eps_loop = true; break; }
      int* vec = rpb[1];
      int nv = 0;
      for (int i = 0; i < nrp; ++i) {
        const int t = rp[i];
        if ((tk[t].flags & LAT_F_RP) && tk[t].rp_slot == i) { vec[nv++] = t; tk[t].flags &= ~LAT_F_RP; }
      }
      nrp = 0;
      if (nv == 0) break;
      for (int i = 0; i < nv && !over; ++i) visit(vec[i]);
      ++loops;
    }
    if (eps_loop) { fail(KHG_LAT_EPS_LOOP | partial); return; }
    if (over) { fail(KHG_LAT_SCRATCH | partial); return; }
    for (int i = 0; i < cur_pos; ++i) slot[i] = -1;
    for (int t = fhead[f]; t >= 0; t = tk[t].next) slot[tk[t].pos] = t;
    // ShortestPath: this frame's states in id order
    for (int i = 0; i < cur_pos; ++i) {
      const int t = slot[i];
      if (t < 0) continue;
      if constexpr (LAT) {
        // state n_states of the raw lattice: its token, frame and first arc; the token's rank in its frame takes the place of its
        // TopSortTokens position (read for the last time when `slot` was filled); final_costs_ empty: One() on the last frame
        tk[t].pos = n_states - fbase[f];
        stok[n_states] = t; sfr[n_states] = f; sarc[n_states] = n_arcs;
        ++n_states;
        if (f == T && !any_final) tk[t].fcost = 0.0f;
        if (!(tk[t].flags & LAT_F_DIST) && start_tok >= 0)
          for (int l = tk[t].links; l >= 0; l = lk[l].next) ++n_arcs;
      }
      if (start_tok < 0) { start_tok = t; tk[t].d1 = 0.0f; tk[t].d2 = 0.0f; tk[t].flags |= LAT_F_DIST; tk[t].plink = -1; }
      if (!(tk[t].flags & LAT_F_DIST)) continue;
      const float sd1 = tk[t].d1, sd2 = tk[t].d2;
      if (f == T) {
        const float fw = any_final ? tk[t].fcost : 0.0f;
        if (fw != INF) {
          const float w1 = sd1 + fw, w2 = sd2 + 0.0f;
          if (f_parent < 0 || lat_less(w1, w2, fd1, fd2)) { fd1 = w1; fd2 = w2; f_parent = t; }
        }
      }
      for (int l = tk[t].links; l >= 0; l = lk[l].next) {
        if constexpr (LAT) ++n_arcs;
        const int nt = lk[l].next_tok;
        const float ac = lk[l].ilabel != 0 ? lk[l].acoustic_cost - coff[f] : lk[l].acoustic_cost - 0.0f;
        const float w1 = sd1 + lk[l].graph_cost, w2 = sd2 + ac;
        if (!(tk[nt].flags & LAT_F_DIST) || lat_less(w1, w2, tk[nt].d1, tk[nt].d2)) {
          tk[nt].d1 = w1; tk[nt].d2 = w2; tk[nt].flags |= LAT_F_DIST; tk[nt].plink = l; tk[nt].ptok = t;
        }
      }
    }
  }
  if (f_parent < 0) { fail(KHG_LAT_NO_TRACEBACK | partial); return; }     // ShortestPath found no final state: empty output
  // backtrace: mark each token's successor link on the path (ptok chain), then walk forward
  for (int t = f_parent; t != start_tok; t = tk[t].ptok) tk[tk[t].ptok].rp_slot = tk[t].plink;
  float v1 = 0.0f, v2 = 0.0f;
  int frame = 0, nw = 0;
  const int64_t wcap = a.words_off[u + 1] - a.words_off[u];
  int32_t* words = a.words + a.words_off[u];
  for (int t = start_tok; t != f_parent;) {
    const int l = tk[t].rp_slot;
    const float ac = lk[l].ilabel != 0 ? lk[l].acoustic_cost - coff[frame] : lk[l].acoustic_cost - 0.0f;
    v1 = lk[l].graph_cost + v1;
    v2 = ac + v2;
    if (lk[l].ilabel != 0) { if (frame < T) a.ali[f0 + frame] = lk[l].ilabel; ++frame; }
    if (lk[l].olabel != 0) { if (nw < wcap) words[nw] = lk[l].olabel; ++nw; }
    t = lk[l].next_tok;
  }
  const float fw = any_final ? tk[f_parent].fcost : 0.0f;
  v1 = fw + v1;
  v2 = 0.0f + v2;
  if (frame != T) { fail(KHG_LAT_NO_TRACEBACK | partial); return; }
  if (nw > wcap) { fail(KHG_LAT_WORDS | partial); return; }
  a.num_words[u] = nw;
  a.like[u] = (double)(-(v1 + v2));
  a.status[u] = KHG_LAT_SUCCEEDED | partial;
  if constexpr (LAT) {
    fbase[T + 1] = n_states; sarc[n_states] = n_arcs;
    utt_tot[2 * (int64_t)blockIdx.x] = n_states; utt_tot[2 * (int64_t)blockIdx.x + 1] = n_arcs;
  }
