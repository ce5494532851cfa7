// K2F: the raw lattice of the order-faithful LatticeFasterDecoder (khg_decode_lattice_faster_raw), emitted from what k2_lattice_faster_lat
// leaves in an utterance's scratch slice: the surviving tokens and forward links, the cost offsets, and -- written by the decoder's lane
// in the per-frame walk that ends it (TopSortTokens + ShortestPath) -- per state its token, frame and first arc, per frame its first
// state, per token its graph state and its rank in its frame.
//
// Stands for (reference csrc/lattice-faster-decoder.cc) :101-192 GetRawLattice: a state per token of active_toks_, numbered by frame,
// then in TopSortTokens order with the gaps removed; an arc per forward link in the link list's order (head first): ilabel, olabel,
// LatticeWeight(graph_cost, acoustic_cost - cost_offsets_[frame] for an emitting link), nextstate; on the last frame final_costs_[tok]
// (One() when no final state was reached).  It is the FST whose best path the decoder kernel returns (DESIGN.md section 7f).
//
// The decoder's lane is serial, so the counts it keeps ARE the prefix sums inside the utterance: nothing is counted or scanned again
// per frame or per state.  Per launch of slices: the decoder, one scan of the utterances' totals (k2_lattice_scan_pairs, shared with
// K2R), the one synchronisation that sizes the output, the fill.  No atomics: every position is a prefix sum.  When a second decoding
// pass re-ran some utterances, k2_lattice_faster_raw_gather rebuilds a chunk from the blocks of both passes.

#define LFR_NT 256

struct LfrArgs {
  LatArgs a;             // the launch's decode: graph tables, slices (laid out with the lattice rows), status
  int32_t n;             // utterances of the launch (list positions u0 .. u0 + n)
  const int64_t* utt_off;    // [2 * (n + 1)]: exclusive prefix over the launch, states at [b], arcs at [n + 1 + b]
  LatArrays out;         // the launch's lattice arrays
  int32_t* start_out;    // [U]: the utterance's start state (-1: empty lattice)
};

// ---- fill: grid (utterance, state stripe); a lane takes a state, then walks that token's own link list ----
__global__ __launch_bounds__(LFR_NT) void k2_lattice_faster_raw_fill(LfrArgs p, int u0) {
#pragma clang fp contract(off)
  const LatArgs& a = p.a;
  const int b = (int)blockIdx.x, k = u0 + b;
  const int u = a.list[k];
  const int64_t so = p.utt_off[b], ao = p.utt_off[(int64_t)p.n + 1 + b];
  const int ns = (int)(p.utt_off[b + 1] - so);       // 0 unless the utterance succeeded
  if (blockIdx.y == 0 && threadIdx.x == 0) p.start_out[u] = ns > 0 ? 0 : -1;      // frame 0 starts at state 0
  if (ns == 0) return;
  const int T = (int)(a.frame_off[u + 1] - a.frame_off[u]);
  const int S = (int)(a.state_off[a.gidx[u] + 1] - a.state_off[a.gidx[u]]);
  const LatLayout L = lat_layout(T, S, a.amax, a.hb, a.tok_cap[k], a.link_cap[k], true);
  const unsigned char* base = a.scratch + a.scr_off[k];
  const LatTok* tk = reinterpret_cast<const LatTok*>(base + L.toks);
  const LatLink* lk = reinterpret_cast<const LatLink*>(base + L.links);
  const float* coff = reinterpret_cast<const float*>(base + L.coff);
  const int32_t* gst = reinterpret_cast<const int32_t*>(base + L.gst);
  const int32_t* stok = reinterpret_cast<const int32_t*>(base + L.stok);
  const int32_t* sfr = reinterpret_cast<const int32_t*>(base + L.sfr);
  const int32_t* sarc = reinterpret_cast<const int32_t*>(base + L.sarc);
  const int32_t* fbase = reinterpret_cast<const int32_t*>(base + L.fbase);
  for (int s = (int)(blockIdx.y * blockDim.x + threadIdx.x); s < ns; s += (int)(gridDim.y * blockDim.x)) {
    const int t = stok[s], f = sfr[s], ab = sarc[s];
    const int64_t sid = so + s;
    p.out.frame[sid] = f;
    p.out.gstate[sid] = gst[t];
    p.out.tot[sid] = tk[t].tot;
    p.out.extra[sid] = tk[t].extra;
    p.out.fin[sid] = tk[t].fcost;         // INF before the last frame and where final_costs_ has no entry
    p.out.arc_begin[sid] = ab;
    const float co = coff[f];
    const int base_eps = fbase[f], base_emit = fbase[f + 1];
    int64_t pos = ao + ab;
    for (int l = tk[t].links; l >= 0; l = lk[l].next, ++pos) {
      const bool emitting = lk[l].ilabel != 0;
      p.out.ilabel[pos] = lk[l].ilabel;
      p.out.olabel[pos] = lk[l].olabel;
      p.out.g[pos] = lk[l].graph_cost;
      p.out.ac[pos] = emitting ? lk[l].acoustic_cost - co : 0.0f;
      p.out.next[pos] = (emitting ? base_emit : base_eps) + tk[lk[l].next_tok].pos;      // (pos: the rank in its frame by now)
    }
  }
}

// ---- gather: a chunk's utterances, each from the block of the pass that decoded it; nothing is renumbered (arc_begin and nextstate
// are relative to the utterance) ----
struct LfrBlock {        // the eleven arrays of a block: frame, graph_state, tot, extra, final, arc_begin | ilabel, olabel, g, ac, next
  const int32_t* st[6];
  const int32_t* ar[5];
};
struct LfrGather {
  const LfrBlock* blocks;
  const int32_t* src_block;       // [n] of the chunk: which block holds the utterance
  const int64_t* src_off;         // [2 * n]: its first state / arc there
  const int64_t* dst_off;         // [2 * (n + 1)]: states at [b], arcs at [n + 1 + b], in the chunk
  int32_t n;
  int32_t* st[6];
  int32_t* ar[5];
};

__global__ __launch_bounds__(LFR_NT) void k2_lattice_faster_raw_gather(LfrGather g) {
  const int b = (int)blockIdx.x;
  const LfrBlock blk = g.blocks[g.src_block[b]];
  const int64_t s_src = g.src_off[2 * (int64_t)b], a_src = g.src_off[2 * (int64_t)b + 1];
  const int64_t s_dst = g.dst_off[b], a_dst = g.dst_off[(int64_t)g.n + 1 + b];
  const int64_t ns = g.dst_off[b + 1] - s_dst, na = g.dst_off[(int64_t)g.n + 2 + b] - a_dst;
  const int64_t step = (int64_t)gridDim.y * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.y * blockDim.x + threadIdx.x; i < ns; i += step)
    for (int j = 0; j < 6; ++j) g.st[j][s_dst + i] = blk.st[j][s_src + i];       // (floats travel as their bits)
  for (int64_t i = (int64_t)blockIdx.y * blockDim.x + threadIdx.x; i < na; i += step)
    for (int j = 0; j < 5; ++j) g.ar[j][a_dst + i] = blk.ar[j][a_src + i];
}
