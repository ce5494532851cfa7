// K2R: the raw lattice of the data-parallel LatticeSimpleDecoder (khg_decode_lattice_simple_raw), emitted from the rows that
// k2_lattice_simple leaves in an utterance's scratch slice: D (token costs), R (PruneCurrentTokens' survivors), pcut / ecut (the
// per-frame cutoffs) and X (FinalizeDecoding's exact extra costs).
//
// Stands for (reference csrc/lattice-simple-decoder.cc) :654-735 GetRawLattice: a state per token of active_toks_ (:684-690), an arc
// per forward link (:700-722: ilabel, olabel, LatticeWeight(graph_cost, acoustic_cost), nextstate), the final weights of the last
// frame's tokens (:723-733).  The reference's lattice depends on the order its unordered_maps are walked in (a link whose cost is at
// or above the frame's final fl(best + beam) is kept in some orders only); this is the order-independent lattice the decoder kernel
// already implies (DESIGN.md section 7d), a subset of every walk's:
//   state  (f, s), f in 0..T: D[f][s] != INF and X[f][s] != INF; numbered by frame, then by graph state
//   emitting link (f, m) -> (f + 1, k): tot = (D[f][m] + ac) + g < pcut[f + 1] and R[f + 1][k]
//   epsilon link  (f, m) -> (f, k):     D[f][m] + g < ecut[f]
//   either survives iff its link extra cost, in the decoder kernel's association order, is <= lattice_beam
//   arcs of a state in the order of the graph's arcs in that state
// Four launches per chunk of slices, behind the decoder's: count (per frame: the rank of every surviving state among its frame's, by
// ballot / wave prefix / LDS across waves; the surviving out-links of every state and their prefix), two scans (frames inside an
// utterance, int32; utterances across the chunk, int64: k2_lattice_scan_pairs), then -- after the one synchronisation that sizes the output -- the fill,
// straight into exactly-sized arrays.  No atomics: every position is a prefix sum, so the order never depends on timing.  Frames
// are independent in count and fill, so the grid is (utterance, frame stripe).  States above the hub threshold have their out-arcs
// counted and filled by a whole wave, 64 arcs at a time by ballot, in arc order: the same arrays at every threshold.

struct LrArgs {
  LsArgs a;              // the chunk's decode: graph tables, scores, slices (laid out with the lattice rows), status, configuration
  int32_t n;             // utterances of the chunk (list positions u0 .. u0 + n)
  int64_t* utt_tot;      // [2 * n]: states, arcs of utterance b of the chunk
  int64_t* utt_off;      // [2 * (n + 1)]: exclusive prefix over the chunk, states at [b], arcs at [n + 1 + b]
  LatArrays out;         // the chunk's lattice arrays (fill)
  int32_t* start_out;    // [U]: the utterance's start state (-1: empty lattice)
};

// an utterance's slice, as the decoder kernel left it
struct LrView {
  int u, T, S, tpad, start, nhub;
  int64_t s0, in0, hub_thr;
  const float* llu;
  const float *D, *X, *pcut, *ecut;
  const unsigned char* R;
  const int32_t *dst, *hub_out;
  int32_t *rank, *aoff, *ftok, *flink;
};

__device__ __forceinline__ LrView lr_view(const LsArgs& a, int k) {
  LrView v;
  v.u = a.list[k];
  const int64_t f0 = a.frame_off[v.u];
  v.T = (int)(a.frame_off[v.u + 1] - f0);
  v.tpad = (v.T + 31) & ~31;
  v.s0 = a.state_off[a.gidx[v.u]];
  v.S = (int)(a.state_off[a.gidx[v.u] + 1] - v.s0);
  v.in0 = a.in_off[v.s0];
  v.llu = a.ll + a.ll_off[v.u];
  v.start = a.start[a.gidx[v.u]];
  v.hub_thr = a.hub > 0 ? a.hub : INT64_MAX;
  v.nhub = 0;
  const LsLayout L = ls_layout(v.T, v.S, a.amax, true);
  unsigned char* base = a.scratch + a.scr_off[k];
  v.D = reinterpret_cast<const float*>(base + L.D);
  v.X = reinterpret_cast<const float*>(base + L.X);
  v.R = base + L.R;
  v.pcut = reinterpret_cast<const float*>(base + L.pcut);
  v.ecut = reinterpret_cast<const float*>(base + L.ecut);
  v.dst = reinterpret_cast<const int32_t*>(base + L.dst);
  v.hub_out = reinterpret_cast<const int32_t*>(base + L.hub) + v.S;
  v.rank = reinterpret_cast<int32_t*>(base + L.rank);
  v.aoff = reinterpret_cast<int32_t*>(base + L.aoff);
  v.ftok = reinterpret_cast<int32_t*>(base + L.ftok);
  v.flink = reinterpret_cast<int32_t*>(base + L.flink);
  return v;
}

// the hub states by out-degree were listed by the decoder kernel (state order); their number is counted again (workgroup-uniform)
__device__ __forceinline__ int lr_count_hubs(const LsArgs& a, const LrView& v) {
  if (a.hub <= 0) return 0;
  int n = 0;
  for (int sb = 0; sb < v.S; sb += (int)blockDim.x) {
    const int s = sb + (int)threadIdx.x;
    n += __syncthreads_count(s < v.S && a.out_off[v.s0 + s + 1] - a.out_off[v.s0 + s] > v.hub_thr);
  }
  return n;
}

// Out-arc `ai` (an in-arc index of the utterance's graph) of the live token (f, m) of cost dm: is it a surviving link?  pc =
// pcut[f + 1], ec = ecut[f].  -> graph cost, acoustic cost, destination state; emitting tells which frame the destination is on.
__device__ __forceinline__ bool lr_link(const LsArgs& a, const LrView& v, int f, float dm, int ai, float pc, float ec, float* g_out,
                                        float* ac_out, int* kk_out, bool* emitting) {
#pragma clang fp contract(off)
  float g = a.in_w[v.in0 + ai];
  const int t = a.in_tid[v.in0 + ai];
  if (a.trans_cost && t >= 1) g = g + a.trans_cost[t];
  const int kk = v.dst[ai];
  const int col = a.in_col[v.in0 + ai];
  float le, ac = 0.0f;
  if (col >= 0) {
    if (f == v.T) return false;                  // the last frame has no emitting links
    const int64_t rn = (int64_t)(f + 1) * v.S + kk;
    ac = -(a.acoustic_scale * v.llu[(int64_t)col * v.tpad + f]);
    const float tot = (dm + ac) + g;
    if (!(tot < pc) || !v.R[rn]) return false;
    le = v.X[rn] + (tot - v.D[rn]);
  } else {
    const int64_t rn = (int64_t)f * v.S + kk;
    if (!(dm + g < ec)) return false;
    le = v.X[rn] + (((dm + 0.0f) + g) - v.D[rn]);
  }
  if (!(le <= a.lattice_beam)) return false;       // excised
  *g_out = g; *ac_out = ac; *kk_out = kk; *emitting = col >= 0;
  return true;
}

// ---- count: per (utterance, frame) the surviving states with their ranks, the surviving links with their per-state prefix ----
__global__ __launch_bounds__(LS_NT) void k2_lattice_raw_count(LrArgs p, int u0) {
  __shared__ int sm[2][LS_NW];
  const LsArgs& a = p.a;
  const int NT = (int)blockDim.x, tid = (int)threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6, nwave = NT >> 6;
  LrView v = lr_view(a, u0 + (int)blockIdx.x);
  const float INF = __builtin_huge_valf();
  if (!(a.status[v.u] & KHG_LAT_SUCCEEDED)) {      // an empty lattice: the slice's rows may hold anything
    for (int f = (int)blockIdx.y * NT + tid; f <= v.T; f += (int)gridDim.y * NT) { v.ftok[f] = 0; v.flink[f] = 0; }
    return;
  }
  v.nhub = lr_count_hubs(a, v);
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int f = (int)blockIdx.y; f <= v.T; f += (int)gridDim.y) {
    const float* D = v.D + (int64_t)f * v.S;
    const float* X = v.X + (int64_t)f * v.S;
    int32_t* rank = v.rank + (int64_t)f * v.S;
    int32_t* aoff = v.aoff + (int64_t)f * v.S;
    const float pc = f < v.T ? v.pcut[f + 1] : INF, ec = v.ecut[f];
    // the hub states: a wave counts one state's links
    for (int h = wave; h < v.nhub; h += nwave) {
      const int m = v.hub_out[h];
      const float dm = D[m];
      int c = 0;
      if (dm != INF && X[m] != INF) {
        for (int64_t oa = a.out_off[v.s0 + m] + lane; oa < a.out_off[v.s0 + m + 1]; oa += 64) {
          float g, ac; int kk; bool em;
          c += lr_link(a, v, f, dm, a.out_inidx[oa], pc, ec, &g, &ac, &kk, &em) ? 1 : 0;
        }
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
      }
      if (lane == 0) aoff[m] = c;
    }
    if (v.nhub) __syncthreads();
    int tokbase = 0, arcbase = 0;
    for (int sb = 0; sb < v.S; sb += NT) {
      const int s = sb + tid;
      float dm = INF;
      bool alive = false;
      if (s < v.S) { dm = D[s]; alive = dm != INF && X[s] != INF; }
      int c = 0;
      if (alive) {
        const int64_t o0 = a.out_off[v.s0 + s], o1 = a.out_off[v.s0 + s + 1];
        if (o1 - o0 > v.hub_thr) c = aoff[s];
        else
          for (int64_t oa = o0; oa < o1; ++oa) {
            float g, ac; int kk; bool em;
            c += lr_link(a, v, f, dm, a.out_inidx[oa], pc, ec, &g, &ac, &kk, &em) ? 1 : 0;
          }
      }
      // ranks: ballot and popcount inside the wave; link prefix: a shuffle scan; both carried across waves through LDS
      const unsigned long long bal = __ballot(alive);
      int incl = c;
      for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o); if (lane >= o) incl += t; }
      if (lane == 63) { sm[0][wave] = __popcll(bal); sm[1][wave] = incl; }
      __syncthreads();
      int wt = 0, wa = 0, tt = 0, ta = 0;
      for (int j = 0; j < nwave; ++j) {
        if (j < wave) { wt += sm[0][j]; wa += sm[1][j]; }
        tt += sm[0][j]; ta += sm[1][j];
      }
      if (s < v.S) {
        rank[s] = alive ? tokbase + wt + __popcll(bal & below) : -1;
        aoff[s] = arcbase + wa + incl - c;
      }
      tokbase += tt; arcbase += ta;
      __syncthreads();
    }
    if (tid == 0) { v.ftok[f] = tokbase; v.flink[f] = arcbase; }
  }
}

// ---- scan: one wave per utterance, the frames' counts -> exclusive offsets in place (int32), the utterance's totals (int64) ----
__global__ __launch_bounds__(64) void k2_lattice_raw_scan_frames(LrArgs p, int u0) {
  const int lane = (int)threadIdx.x;
  const LrView v = lr_view(p.a, u0 + (int)blockIdx.x);
  long long ts = 0, ta = 0;
  for (int fb = 0; fb <= v.T; fb += 64) {
    const int f = fb + lane;
    const int c1 = f <= v.T ? v.ftok[f] : 0, c2 = f <= v.T ? v.flink[f] : 0;
    long long i1 = c1, i2 = c2;
    for (int o = 1; o < 64; o <<= 1) {
      const long long t1 = __shfl_up(i1, o), t2 = __shfl_up(i2, o);
      if (lane >= o) { i1 += t1; i2 += t2; }
    }
    if (f <= v.T) { v.ftok[f] = (int32_t)(ts + i1 - c1); v.flink[f] = (int32_t)(ta + i2 - c2); }   // (past int32: the host refuses the utterance)
    ts += __shfl(i1, 63); ta += __shfl(i2, 63);
  }
  if (lane == 0) { p.utt_tot[2 * (int64_t)blockIdx.x] = ts; p.utt_tot[2 * (int64_t)blockIdx.x + 1] = ta; }
}

// ---- fill: states and arcs, at the positions the prefix sums give ----
__global__ __launch_bounds__(LS_NT) void k2_lattice_raw_fill(LrArgs p, int u0) {
  const LsArgs& a = p.a;
  const int NT = (int)blockDim.x, tid = (int)threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6, nwave = NT >> 6;
  const int b = (int)blockIdx.x;
  LrView v = lr_view(a, u0 + b);
  const float INF = __builtin_huge_valf();
  if (!(a.status[v.u] & KHG_LAT_SUCCEEDED)) {
    if (blockIdx.y == 0 && tid == 0) p.start_out[v.u] = -1;
    return;
  }
  v.nhub = lr_count_hubs(a, v);
  const int64_t so = p.utt_off[b], ao = p.utt_off[(int64_t)p.n + 1 + b];
  if (blockIdx.y == 0 && tid == 0) p.start_out[v.u] = v.rank[v.start];      // frame 0 starts at state 0
  const unsigned long long below = (1ull << lane) - 1ull;
  auto put_arc = [&](int64_t pos, int ai, float g, float ac, int next) {
    p.out.ilabel[pos] = a.in_tid[v.in0 + ai];
    p.out.olabel[pos] = a.in_olabel[v.in0 + ai];
    p.out.g[pos] = g;
    p.out.ac[pos] = ac;
    p.out.next[pos] = next;
  };
  for (int f = (int)blockIdx.y; f <= v.T; f += (int)gridDim.y) {
    const float* D = v.D + (int64_t)f * v.S;
    const float* X = v.X + (int64_t)f * v.S;
    const int32_t* rank = v.rank + (int64_t)f * v.S;
    const int32_t* rank_n = rank + v.S;                    // (read only for emitting links, which the last frame has none of)
    const int32_t* aoff = v.aoff + (int64_t)f * v.S;
    const float pc = f < v.T ? v.pcut[f + 1] : INF, ec = v.ecut[f];
    const int tokbase = v.ftok[f], arcbase = v.flink[f], nextbase = f < v.T ? v.ftok[f + 1] : 0;
    for (int s = tid; s < v.S; s += NT) {
      const int r = rank[s];
      if (r < 0) continue;
      const int64_t sid = so + tokbase + r;
      const int ab = arcbase + aoff[s];
      const float dm = D[s];
      p.out.frame[sid] = f;
      p.out.gstate[sid] = s;
      p.out.tot[sid] = dm;
      p.out.extra[sid] = X[s];
      p.out.fin[sid] = f == v.T ? a.final_w[v.s0 + s] : INF;
      p.out.arc_begin[sid] = ab;
      const int64_t o0 = a.out_off[v.s0 + s], o1 = a.out_off[v.s0 + s + 1];
      if (o1 - o0 > v.hub_thr) continue;         // a hub state: below
      int64_t pos = ao + ab;
      for (int64_t oa = o0; oa < o1; ++oa) {
        const int ai = a.out_inidx[oa];
        float g, ac; int kk; bool em;
        if (!lr_link(a, v, f, dm, ai, pc, ec, &g, &ac, &kk, &em)) continue;
        put_arc(pos, ai, g, ac, em ? nextbase + rank_n[kk] : tokbase + rank[kk]);
        ++pos;
      }
    }
    for (int h = wave; h < v.nhub; h += nwave) {
      const int m = v.hub_out[h];
      if (rank[m] < 0) continue;
      const float dm = D[m];
      int64_t pos = ao + arcbase + aoff[m];
      const int64_t o0 = a.out_off[v.s0 + m], o1 = a.out_off[v.s0 + m + 1];
      for (int64_t ob = o0; ob < o1; ob += 64) {
        const int64_t oa = ob + lane;
        int ai = 0, kk = 0;
        float g = 0.0f, ac = 0.0f;
        bool em = false, ok = false;
        if (oa < o1) { ai = a.out_inidx[oa]; ok = lr_link(a, v, f, dm, ai, pc, ec, &g, &ac, &kk, &em); }
        const unsigned long long bal = __ballot(ok);
        if (ok) put_arc(pos + __popcll(bal & below), ai, g, ac, em ? nextbase + rank_n[kk] : tokbase + rank[kk]);
        pos += __popcll(bal);
      }
    }
  }
}
