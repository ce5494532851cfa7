// K2S: data-parallel LatticeSimpleDecoder + DecodeUtteranceLatticeSimple (khg_decode_lattice_simple), one workgroup per utterance,
// every lane owning destination states (a lane loops when the graph has more states than the workgroup has lanes).
//
// Restates (reference csrc/lattice-simple-decoder.cc, decoder-wrappers.cc), in float and in the reference's association order:
//   :40-66 InitDecoding  :68-142 ProcessNonemitting  :144-165 Decode  :174-219 FindOrAddToken  :224-309 PruneForwardLinks
//   :349-383 PruneActiveTokens  :385-426 ProcessEmitting  :431-461 PruneCurrentTokens  :466-582 FinalizeDecoding /
//   PruneForwardLinksFinal  :584-628 ComputeFinalCosts  :644-735 GetBestPath = GetRawLattice + ShortestPath
//   decoder-wrappers.cc:142-182 DecodeUtteranceLatticeSimple: (succeeded, alignment, words, like = -(graph + acoustic))
// The reference's answer does not depend on the order it walks its unordered_maps in (DESIGN.md section 7b), so every frame is a
// gather over in-arcs: no atomics, no hash, and the same answer on every run.  Three passes per utterance, over dense per-frame rows
// in the utterance's HBM scratch slice:
//   1. forward: token costs D[f][s] (INF: no live token), PruneCurrentTokens' survivors R[f][s], the cutoffs, Quirk 1, NaN links;
//   2. backward: the exact extra costs X[f][s] of FinalizeDecoding (delta = 0; the final frame with the final costs);
//   3. forward: OpenFst's ShortestPath over the links that survive, by the tie rule below, then the trace-back.
// Links are never stored: a link exists iff its arc passes the frame's cutoff from a live token into a token it can reach, and it
// survives iff its extra cost is <= lattice_beam, all of which the passes recompute from D, R, X and the cutoffs.
//
// Tie rule (the restatement, tests/lattice_simple_ref.py, uses the same): per frame, emitting in-links first, then epsilon in-links in
// Jacobi rounds (each round reads the previous round's distances); inside a round a destination takes its in-links in the in-arc
// CSR order of khg_utts_create (source state, then arc index) and changes only on a strictly better LatticeWeight (Value1 + Value2,
// then Value1).  The final state is the lowest-numbered one among exactly tied totals.
//
// Hub states (a.hub > 0): a state with more than a.hub in-arcs -- out-arcs in the backward pass -- (a word loop's loop state: one
// arc per word) does not have its arcs walked by the one lane that owns it; the waves of the workgroup take such states in turn,
// the 64 lanes stride over the arcs and combine by shuffles.  Every combination carries (key, position in the arc list) and prefers
// the lower position among equal keys, which is what the serial loop's strict comparisons keep: the same answer, bit for bit.

struct LsArgs {
  const int64_t* frame_off;   // [U+1]
  const int32_t* gidx;        // [U] the row of state_off / start an utterance decodes on (identity; zeros on a shared graph)
  const int64_t* state_off;   // [rows+1]
  const int32_t* start;       // [U]
  const int64_t* in_off;      // [sumS+1]
  const int32_t* in_src;
  const int32_t* in_col;      // -1: epsilon input
  const int32_t* in_tid;
  const int32_t* in_olabel;
  const float* in_w;
  const int64_t* out_off;     // [sumS+1]
  const int32_t* out_inidx;
  const float* final_w;
  const float* trans_cost;    // or nullptr
  const float* ll;
  const int64_t* ll_off;
  // workgroup b of a launch at list position u0 decodes utterance list[u0 + b], its slice at scratch + scr_off[u0 + b]
  const int32_t* list;
  unsigned char* scratch;
  const int64_t* scr_off;
  // outputs
  int32_t* ali;               // [sumT]
  int32_t* words;             // per utterance words_off[u+1] - words_off[u]
  const int64_t* words_off;
  int32_t* num_words;
  double* like;
  int32_t* status;
  int32_t* err_frame;
  // config
  float beam, lattice_beam, acoustic_scale;
  int32_t prune_interval, tok_cap;   // tok_cap: most live tokens on one frame (0: no limit)
  int32_t amax;               // arc bound the slices were laid out with (>= every utterance's arc count)
  int32_t hub;                // arc loops of states with more arcs than this are walked by a wave (0: never)
};

// the per-utterance slice: dense rows [T+1][S] of D, X, BP (best-path in-arc), R (byte), per-frame cutoffs, the graph tables, and
// six working rows of the best-path distances (frame f, frame f+1, Jacobi round buffer; Value1 and Value2 each).  lat (a raw lattice
// was asked for, khg_k2_lattice_raw.hip.inc): behind those, two more dense rows -- the rank of (f, s) among its frame's surviving
// states, the prefix of its surviving out-links -- and the per-frame state / link counts; the rows above stay where they are
struct LsLayout { int64_t D, X, BP, R, pcut, ecut, dst, nieps, w, hub, rank, aoff, ftok, flink, total; };
__host__ __device__ inline LsLayout ls_layout(int64_t T, int64_t S, int64_t A, bool lat = false) {
  LsLayout L;
  int64_t o = 0;
  auto take = [&](int64_t bytes) { int64_t r = o; o += (bytes + 255) & ~int64_t(255); return r; };
  const int64_t rows = (T + 1) * S;
  L.D = take(4 * rows);
  L.X = take(4 * rows);
  L.BP = take(4 * rows);
  L.R = take(rows);
  L.pcut = take(4 * (T + 1));
  L.ecut = take(4 * (T + 1));
  L.dst = take(4 * A);
  L.nieps = take(4 * S);
  L.w = take(4 * 6 * S);
  L.hub = take(4 * 2 * S);      // the hub states by in-degree, then by out-degree
  L.rank = L.aoff = L.ftok = L.flink = -1;
  if (lat) {
    L.rank = take(4 * rows);
    L.aoff = take(4 * rows);
    L.ftok = take(4 * (T + 2));
    L.flink = take(4 * (T + 2));
  }
  L.total = o;
  return L;
}

#define LS_NT 256
#define LS_NW (LS_NT / 64)

__device__ __forceinline__ float ls_block_min(float v, float* red) {
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = red[0];
  for (int i = 1; i < (int)(blockDim.x >> 6); ++i) r = fminf(r, red[i]);
  __syncthreads();
  return r;
}

__device__ __forceinline__ bool ls_less(float a1, float a2, float b1, float b2) {   // NaturalLess: (a1, a2) strictly better
  const float fa = a1 + a2, fb = b1 + b2;
  if (fa < fb) return true;
  if (fa > fb) return false;
  return a1 < b1;
}

#define LS_NONE 0x7fffffff
// over the wave: the least v and, among equal v, the least pos (the serial loop's strict `<` keeps the first of equals); identity (INF, LS_NONE)
__device__ __forceinline__ void ls_wave_min_first(float& v, int& pos) {
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o);
    const int op = __shfl_xor(pos, o);
    if (ov < v || (ov == v && op < pos)) { v = ov; pos = op; }
  }
}
// the same for LatticeWeight pairs under ls_less; pos == LS_NONE: no candidate
__device__ __forceinline__ void ls_wave_best_first(float& b1, float& b2, int& pos) {
  for (int o = 32; o > 0; o >>= 1) {
    const float o1 = __shfl_xor(b1, o), o2 = __shfl_xor(b2, o);
    const int op = __shfl_xor(pos, o);
    if (op != LS_NONE && (pos == LS_NONE || ls_less(o1, o2, b1, b2) || (!ls_less(b1, b2, o1, o2) && op < pos))) { b1 = o1; b2 = o2; pos = op; }
  }
}

__global__ __launch_bounds__(LS_NT) void k2_lattice_simple(LsArgs a, int u0) {
#pragma clang fp contract(off)
  __shared__ float red[LS_NW];
  __shared__ int hcnt[2][LS_NW];
  const int NT = (int)blockDim.x, tid = (int)threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6, nwave = NT >> 6;
  const int k = u0 + (int)blockIdx.x;
  const int u = a.list[k];
  const int64_t f0 = a.frame_off[u];
  const int T = (int)(a.frame_off[u + 1] - f0);
  const int tpad = (T + 31) & ~31;
  const int64_t s0 = a.state_off[a.gidx[u]];
  const int S = (int)(a.state_off[a.gidx[u] + 1] - s0);
  const int64_t in0 = a.in_off[s0];
  const float* llu = a.ll + a.ll_off[u];
  const LsLayout L = ls_layout(T, S, a.amax);
  unsigned char* base = a.scratch + a.scr_off[k];
  float* Drow = reinterpret_cast<float*>(base + L.D);
  float* Xrow = reinterpret_cast<float*>(base + L.X);
  int32_t* BProw = reinterpret_cast<int32_t*>(base + L.BP);
  unsigned char* Rrow = base + L.R;
  float* pcut = reinterpret_cast<float*>(base + L.pcut);
  float* ecut = reinterpret_cast<float*>(base + L.ecut);
  int32_t* dst = reinterpret_cast<int32_t*>(base + L.dst);
  int32_t* nieps = reinterpret_cast<int32_t*>(base + L.nieps);
  float* wrk = reinterpret_cast<float*>(base + L.w);
  int32_t* hub_in = reinterpret_cast<int32_t*>(base + L.hub);
  int32_t* hub_out = hub_in + S;
  const int64_t hub_thr = a.hub > 0 ? a.hub : INT64_MAX;
  const float INF = __builtin_huge_valf();
  const int start = a.start[a.gidx[u]];
  // khg_utts_create refuses start >= S only: a graph without a start state (kNoStateId, the reference's KHG_ASSERT at :52) has no path
  if (start < 0 || start >= S) {
    for (int t = tid; t < T; t += NT) a.ali[f0 + t] = 0;
    if (tid == 0) { a.num_words[u] = 0; a.like[u] = 0.0; a.status[u] = KHG_LAT_NO_PATH; a.err_frame[u] = -1; }
    return;
  }

  // the outcome of an utterance without output: every lane agrees on `st` (all decisions below are workgroup-uniform)
  auto fail = [&](int st, int frame) {
    for (int t = tid; t < T; t += NT) a.ali[f0 + t] = 0;
    if (tid == 0) { a.num_words[u] = 0; a.like[u] = 0.0; a.status[u] = st; a.err_frame[u] = frame; }
  };
  auto arc_w = [&](int ai) {
    float w = a.in_w[in0 + ai];
    const int t = a.in_tid[in0 + ai];
    if (a.trans_cost && t >= 1) w = w + a.trans_cost[t];
    return w;
  };
  // -1 * LogLikelihood(frame, ilabel) with DecodableAmDiagGmmScaled's scale (1 for scores uploaded already scaled)
  auto ac_cost = [&](int ai, int frame) { return -(a.acoustic_scale * llu[(int64_t)a.in_col[in0 + ai] * tpad + frame]); };

  // the hub states, in state order: in-degree above the threshold, then out-degree above it (the counts are workgroup-uniform)
  int nhub_in = 0, nhub_out = 0;
  if (a.hub > 0) {
    for (int sb = 0; sb < S; sb += NT) {
      const int s = sb + tid;
      const bool hi = s < S && a.in_off[s0 + s + 1] - a.in_off[s0 + s] > hub_thr;
      const bool ho = s < S && a.out_off[s0 + s + 1] - a.out_off[s0 + s] > hub_thr;
      const unsigned long long bi = __ballot(hi), bo = __ballot(ho);
      if (lane == 0) { hcnt[0][wave] = __popcll(bi); hcnt[1][wave] = __popcll(bo); }
      __syncthreads();
      int oi = nhub_in, oo = nhub_out;
      for (int j = 0; j < nwave; ++j) {
        if (j < wave) { oi += hcnt[0][j]; oo += hcnt[1][j]; }
        nhub_in += hcnt[0][j]; nhub_out += hcnt[1][j];
      }
      const unsigned long long below = (1ull << lane) - 1ull;
      if (hi) hub_in[oi + __popcll(bi & below)] = s;
      if (ho) hub_out[oo + __popcll(bo & below)] = s;
      __syncthreads();
    }
  }
  // graph tables: destination of every in-arc, fst_.NumInputEpsilons of every state
  for (int s = tid; s < S; s += NT) {
    Drow[s] = s == start ? 0.0f : INF;   // InitDecoding: the start token, cost 0
    const int64_t i0 = a.in_off[s0 + s], i1 = a.in_off[s0 + s + 1], o0 = a.out_off[s0 + s], o1 = a.out_off[s0 + s + 1];
    if (i1 - i0 <= hub_thr)
      for (int64_t i = i0; i < i1; ++i) dst[i - in0] = s;
    if (o1 - o0 > hub_thr) continue;
    int n = 0;
    for (int64_t oa = o0; oa < o1; ++oa) n += a.in_col[in0 + a.out_inidx[oa]] < 0;
    nieps[s] = n;
  }
  for (int h = wave; h < nhub_in; h += nwave) {
    const int s = hub_in[h];
    for (int64_t i = a.in_off[s0 + s] + lane; i < a.in_off[s0 + s + 1]; i += 64) dst[i - in0] = s;
  }
  for (int h = wave; h < nhub_out; h += nwave) {
    const int s = hub_out[h];
    int n = 0;
    for (int64_t oa = a.out_off[s0 + s] + lane; oa < a.out_off[s0 + s + 1]; oa += 64) n += a.in_col[in0 + a.out_inidx[oa]] < 0;
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
    if (lane == 0) nieps[s] = n;
  }
  __syncthreads();

  // ProcessNonemitting's closure on row D (frame f): with the cutoff fixed, the tokens and costs the reference's LIFO queue settles
  // on are the least fixpoint of the relaxation; in-place rounds reach it in any interleaving.  -> false on a negative-cost epsilon
  // cycle (no fixpoint within S + 1 rounds; the reference loops forever)
  auto closure = [&](float* D, float cut) -> bool {
    for (int round = 0;; ++round) {
      int changed = 0;
      for (int n = tid; n < S; n += NT) {
        const int64_t i0 = a.in_off[s0 + n], i1 = a.in_off[s0 + n + 1];
        if (i1 - i0 > hub_thr) continue;       // a hub state: below
        const float cur = D[n];
        float best = cur;
        for (int64_t i = i0; i < i1; ++i) {
          const int ai = (int)(i - in0);
          if (a.in_col[i] >= 0) continue;
          const float dm = D[a.in_src[i]];
          if (dm == INF) continue;
          const float tot = dm + arc_w(ai);
          if (tot < cut && tot < best) best = tot;
        }
        if (best < cur) { D[n] = best; changed = 1; }
      }
      for (int h = wave; h < nhub_in; h += nwave) {
        const int n = hub_in[h];
        const int64_t i0 = a.in_off[s0 + n], i1 = a.in_off[s0 + n + 1];
        const float cur = D[n];
        float best = INF;
        int pos = LS_NONE;
        for (int64_t i = i0 + lane; i < i1; i += 64) {
          if (a.in_col[i] >= 0) continue;
          const float dm = D[a.in_src[i]];
          if (dm == INF) continue;
          const float tot = dm + arc_w((int)(i - in0));
          if (tot < cut && tot < best) { best = tot; pos = (int)(i - i0); }
        }
        ls_wave_min_first(best, pos);
        if (lane == 0 && best < cur) { D[n] = best; changed = 1; }
      }
      if (!__syncthreads_or(changed)) return true;
      if (round > S) return false;
    }
  };

  // the most live tokens one frame may hold (scratch_per_frame; 0: no limit)
  auto over_cap = [&](const float* D) -> bool {
    if (a.tok_cap <= 0) return false;
    int live = 0;
    for (int n = tid; n < S; n += NT) live += D[n] != INF;
    return __syncthreads_count(live) > a.tok_cap;
  };

  // ---- pass 1: Decode (:144-158) ----
  // InitDecoding (:40-66): ProcessNonemitting at frame -1, the map holding the start token only
  if (nieps[start] == 0) { fail(KHG_LAT_NO_EPS_TOKEN, -1); return; }     // :95-101
  if (tid == 0) { pcut[0] = INF; ecut[0] = 0.0f + a.beam; }
  if (!closure(Drow, 0.0f + a.beam)) { fail(KHG_LAT_EPS_LOOP, -1); return; }
  if (over_cap(Drow)) { fail(KHG_LAT_SCRATCH, -1); return; }
  int nan_frame = -1;      // first frame with a NaN forward link (every such link is kept: `tot >= cutoff` is false for NaN)
  for (int t = 0; t < T; ++t) {
    // PruneActiveTokens (:349-383) never changes the search; it reaches PruneForwardLinks' NaN check (:261) on every frame with
    // links that it has not pruned before, which is every frame below the current one
    if (t % a.prune_interval == 0 && nan_frame >= 0 && nan_frame < t) { fail(KHG_LAT_NAN, -1); return; }
    const float* Dp = Drow + (int64_t)t * S;
    float* Dn = Drow + (int64_t)(t + 1) * S;
    unsigned char* Rn = Rrow + (int64_t)(t + 1) * S;
    // ProcessEmitting (:385-426): each state's cheapest in-arc from the map; the running cutoff never drops below
    // fl(best + beam), so exactly those arcs are kept
    float lmin = INF;
    int nan = 0;
    for (int n = tid; n < S; n += NT) {
      const int64_t i0 = a.in_off[s0 + n], i1 = a.in_off[s0 + n + 1];
      if (i1 - i0 > hub_thr) continue;       // a hub state: below
      float c = INF;
      for (int64_t i = i0; i < i1; ++i) {
        if (a.in_col[i] < 0) continue;
        const float dm = Dp[a.in_src[i]];
        if (dm == INF) continue;
        const int ai = (int)(i - in0);
        const float tot = (dm + ac_cost(ai, t)) + arc_w(ai);
        if (tot != tot) nan = 1;
        else if (tot < c) c = tot;
      }
      Dn[n] = c;
      lmin = fminf(lmin, c);
    }
    for (int h = wave; h < nhub_in; h += nwave) {
      const int n = hub_in[h];
      const int64_t i0 = a.in_off[s0 + n], i1 = a.in_off[s0 + n + 1];
      float c = INF;
      int pos = LS_NONE;
      for (int64_t i = i0 + lane; i < i1; i += 64) {
        if (a.in_col[i] < 0) continue;
        const float dm = Dp[a.in_src[i]];
        if (dm == INF) continue;
        const int ai = (int)(i - in0);
        const float tot = (dm + ac_cost(ai, t)) + arc_w(ai);
        if (tot != tot) nan = 1;
        else if (tot < c) { c = tot; pos = (int)(i - i0); }
      }
      ls_wave_min_first(c, pos);
      if (lane == 0) { Dn[n] = c; lmin = fminf(lmin, c); }
    }
    const float best = ls_block_min(lmin, red);
    if (__syncthreads_or(nan) && nan_frame < 0) nan_frame = t;
    // PruneCurrentTokens (:431-461): best_cost starts at 1e10
    const float pc = fminf(1.0e+10f, best) + a.beam;
    float lbest = INF;
    int eps = 0;
    for (int n = tid; n < S; n += NT) {
      const float c = Dn[n];
      const bool keep = c < pc;
      Rn[n] = keep ? 1 : 0;
      if (keep) { lbest = fminf(lbest, c); eps |= nieps[n] != 0; }
      else Dn[n] = INF;
    }
    const float best2 = ls_block_min(lbest, red);
    // ProcessNonemitting (:68-142) at frame t: the queue holds the map's states with an input-epsilon arc
    if (!__syncthreads_or(eps)) { fail(KHG_LAT_NO_EPS_TOKEN, t); return; }
    const float ec = best2 + a.beam;
    if (tid == 0) { pcut[t + 1] = pc; ecut[t + 1] = ec; }
    if (!closure(Dn, ec)) { fail(KHG_LAT_EPS_LOOP, t); return; }
    if (over_cap(Dn)) { fail(KHG_LAT_SCRATCH, -1); return; }
  }
  // FinalizeDecoding runs PruneForwardLinks on every frame: any NaN link left stops it (:261)
  if (nan_frame >= 0) { fail(KHG_LAT_NAN, -1); return; }

  // ---- pass 2: FinalizeDecoding (:466-478) ----
  const float* DT = Drow + (int64_t)T * S;
  // ComputeFinalCosts (:584-628) over the map
  float lb = INF, lbf = INF;
  int nfin = 0;
  for (int n = tid; n < S; n += NT) {
    const float d = DT[n];
    if (d == INF) continue;
    const float fc = a.final_w[s0 + n];
    lb = fminf(lb, d);
    lbf = fminf(lbf, d + fc);
    nfin += fc != INF;
  }
  const float best_cost = ls_block_min(lb, red), best_cost_with_final = ls_block_min(lbf, red);
  // Decode() returns !final_costs_.empty() (:164); DecodeUtteranceLatticeSimple stops there whatever allow_partial says
  if (!__syncthreads_or(nfin)) { fail(KHG_LAT_NO_PATH, -1); return; }
  if (T == 0) { fail(KHG_LAT_NO_TRACEBACK, -1); return; }       // GetRawLattice's KHG_ASSERT(num_frames > 0) (:680)
  const float final_best_cost = best_cost_with_final != INF ? best_cost_with_final : best_cost;
  const float beamL = a.lattice_beam;
  // the extra costs of one frame: the least fixpoint above zero (a new token's extra cost), which the reference's delta = 0 passes
  // reach from the lower values its interval pruning left; rounds stay in place.  Every value only rises (each is recomputed from
  // values no lower than the ones it was last computed from), so a round that changes anything raises some value strictly, within
  // the floats of [0, lattice_beam] and INF: the rounds end, as the reference's passes do -- after lattice_beam / w rounds or so on
  // an epsilon cycle of small positive weight w, never forever.  No cap, so no false report.
  auto extra_frame = [&](int f) {
    const float* D = Drow + (int64_t)f * S;
    float* X = Xrow + (int64_t)f * S;
    const bool last = f == T;
    const float* Dn = last ? nullptr : Drow + (int64_t)(f + 1) * S;
    const float* Xn = last ? nullptr : Xrow + (int64_t)(f + 1) * S;
    const unsigned char* Rn = last ? nullptr : Rrow + (int64_t)(f + 1) * S;
    for (int n = tid; n < S; n += NT) X[n] = D[n] == INF ? INF : 0.0f;
    __syncthreads();
    for (;;) {
      int changed = 0;
      for (int h = wave; h < nhub_out; h += nwave) {       // the hub states (by out-degree)
        const int m = hub_out[h];
        const float dm = D[m];
        if (dm == INF) continue;
        const int64_t o0 = a.out_off[s0 + m], o1 = a.out_off[s0 + m + 1];
        float te = INF;
        int pos = LS_NONE;
        for (int64_t oa = o0 + lane; oa < o1; oa += 64) {
          const int ai = a.out_inidx[oa];
          const int kk = dst[ai];
          const float g = arc_w(ai);
          float le;
          if (a.in_col[in0 + ai] >= 0) {
            if (last) continue;
            const float tot = (dm + ac_cost(ai, f)) + g;
            if (!(tot < pcut[f + 1]) || !Rn[kk]) continue;
            le = Xn[kk] + (tot - Dn[kk]);
          } else {
            if (!(dm + g < ecut[f])) continue;
            le = X[kk] + (((dm + 0.0f) + g) - D[kk]);
          }
          if (le > beamL) continue;
          if (le < 0.0f) le = 0.0f;
          if (le < te) { te = le; pos = (int)(oa - o0); }
        }
        ls_wave_min_first(te, pos);
        if (lane == 0) {
          if (last) {   // the final-cost term comes first in the serial order: it stays on a tie
            const float fc = a.final_w[s0 + m];
            const float ft = dm + fc - final_best_cost;
            if (!(te < ft)) te = ft;
            if (te > beamL) te = INF;
          }
          if (te != X[m]) { X[m] = te; changed = 1; }
        }
      }
      for (int m = tid; m < S; m += NT) {
        const float dm = D[m];
        if (dm == INF) continue;
        if (a.out_off[s0 + m + 1] - a.out_off[s0 + m] > hub_thr) continue;       // a hub state: above
        float te = INF;
        if (last) {   // PruneForwardLinksFinal (:483-582): a term for the final cost
          const float fc = a.final_w[s0 + m];
          te = dm + fc - final_best_cost;
        }
        for (int64_t oa = a.out_off[s0 + m]; oa < a.out_off[s0 + m + 1]; ++oa) {
          const int ai = a.out_inidx[oa];
          const int kk = dst[ai];
          const float g = arc_w(ai);
          float le;
          if (a.in_col[in0 + ai] >= 0) {
            if (last) continue;                  // the last frame has no emitting links
            const float tot = (dm + ac_cost(ai, f)) + g;
            if (!(tot < pcut[f + 1]) || !Rn[kk]) continue;
            le = Xn[kk] + (tot - Dn[kk]);
          } else {
            if (!(dm + g < ecut[f])) continue;
            le = X[kk] + (((dm + 0.0f) + g) - D[kk]);
          }
          if (le > beamL) continue;              // excised
          if (le < 0.0f) le = 0.0f;
          if (le < te) te = le;
        }
        if (last && te > beamL) te = INF;
        if (te != X[m]) { X[m] = te; changed = 1; }
      }
      if (!__syncthreads_or(changed)) return;
    }
  };
  for (int f = T; f >= 0; --f) extra_frame(f);

  // ---- pass 3: GetBestPath (:644-650): ShortestPath over the surviving links ----
  float* P1 = wrk;                 // frame f
  float* P2 = wrk + S;
  float* Q1 = wrk + 2 * (int64_t)S;    // frame f + 1
  float* Q2 = wrk + 3 * (int64_t)S;
  float* N1 = wrk + 4 * (int64_t)S;    // Jacobi round buffer
  float* N2 = wrk + 5 * (int64_t)S;
  // a surviving epsilon in-link i of n on frame f (D, X of that frame): its source is live, it passed the cutoff, it was not excised
  auto eps_ok = [&](int64_t i, const float* D, const float* X, float cut, int n, float* g_out) -> bool {
    const float dm = D[a.in_src[i]];
    if (dm == INF || D[n] == INF) return false;
    const float g = arc_w((int)(i - in0));
    if (!(dm + g < cut)) return false;
    const float le = X[n] + (((dm + 0.0f) + g) - D[n]);
    if (!(le <= beamL)) return false;
    *g_out = g;
    return true;
  };
  // epsilon rounds on frame f's distances (V1, V2) in place of B1 / B2, back-pointers into BP
  auto eps_rounds = [&](int f, float* B1, float* B2) -> bool {
    const float* D = Drow + (int64_t)f * S;
    const float* X = Xrow + (int64_t)f * S;
    int32_t* BP = BProw + (int64_t)f * S;
    for (int round = 0;; ++round) {
      int changed = 0;
      for (int h = wave; h < nhub_in; h += nwave) {        // the hub states
        const int n = hub_in[h];
        float b1 = INF, b2 = INF;
        int pos = LS_NONE;
        for (int64_t i = a.in_off[s0 + n] + lane; i < a.in_off[s0 + n + 1]; i += 64) {
          if (a.in_col[i] >= 0) continue;
          const int m = a.in_src[i];
          if (B1[m] == INF) continue;
          float g;
          if (!eps_ok(i, D, X, ecut[f], n, &g)) continue;
          const float c1 = B1[m] + g, c2 = B2[m] + 0.0f;
          if (pos == LS_NONE || ls_less(c1, c2, b1, b2)) { b1 = c1; b2 = c2; pos = (int)(i - in0); }
        }
        ls_wave_best_first(b1, b2, pos);
        if (lane == 0) {
          const float o1 = B1[n], o2 = B2[n];
          if (pos != LS_NONE && (o1 == INF || ls_less(b1, b2, o1, o2))) { N1[n] = b1; N2[n] = b2; BP[n] = pos; changed = 1; }
          else { N1[n] = o1; N2[n] = o2; }
        }
      }
      for (int n = tid; n < S; n += NT) {
        if (a.in_off[s0 + n + 1] - a.in_off[s0 + n] > hub_thr) continue;       // a hub state: above
        float b1 = B1[n], b2 = B2[n];
        int bp = -2;
        for (int64_t i = a.in_off[s0 + n]; i < a.in_off[s0 + n + 1]; ++i) {
          if (a.in_col[i] >= 0) continue;
          const int m = a.in_src[i];
          if (B1[m] == INF) continue;       // not reached (a reached distance is finite: the path survived pruning)
          float g;
          if (!eps_ok(i, D, X, ecut[f], n, &g)) continue;
          const float c1 = B1[m] + g, c2 = B2[m] + 0.0f;
          if (b1 == INF || ls_less(c1, c2, b1, b2)) { b1 = c1; b2 = c2; bp = (int)(i - in0); }
        }
        N1[n] = b1; N2[n] = b2;
        if (bp != -2) { BP[n] = bp; changed = 1; }
      }
      __syncthreads();
      for (int n = tid; n < S; n += NT) { B1[n] = N1[n]; B2[n] = N2[n]; }
      if (!__syncthreads_or(changed)) return true;
      if (round > S) return false;
    }
  };
  for (int n = tid; n < S; n += NT) {
    P1[n] = n == start && Xrow[n] != INF ? 0.0f : INF;
    P2[n] = n == start && Xrow[n] != INF ? 0.0f : INF;
    if (n == start) BProw[n] = -1;
  }
  __syncthreads();
  if (!eps_rounds(0, P1, P2)) { fail(KHG_LAT_EPS_LOOP, -1); return; }
  for (int f = 0; f < T; ++f) {
    const float* D = Drow + (int64_t)f * S;
    const float* Dn = Drow + (int64_t)(f + 1) * S;
    const float* Xn = Xrow + (int64_t)(f + 1) * S;
    const unsigned char* Rn = Rrow + (int64_t)(f + 1) * S;
    int32_t* BPn = BProw + (int64_t)(f + 1) * S;
    for (int h = wave; h < nhub_in; h += nwave) {          // the hub states
      const int n = hub_in[h];
      float b1 = INF, b2 = INF;
      int pos = LS_NONE;
      if (Rn[n] && Xn[n] != INF) {
        for (int64_t i = a.in_off[s0 + n] + lane; i < a.in_off[s0 + n + 1]; i += 64) {
          if (a.in_col[i] < 0) continue;
          const int m = a.in_src[i];
          if (P1[m] == INF) continue;
          const int ai = (int)(i - in0);
          const float ac = ac_cost(ai, f), g = arc_w(ai), tot = (D[m] + ac) + g;
          if (!(tot < pcut[f + 1])) continue;
          const float le = Xn[n] + (tot - Dn[n]);
          if (!(le <= beamL)) continue;
          const float c1 = P1[m] + g, c2 = P2[m] + ac;
          if (pos == LS_NONE || ls_less(c1, c2, b1, b2)) { b1 = c1; b2 = c2; pos = ai; }
        }
        ls_wave_best_first(b1, b2, pos);
      }
      if (lane == 0) {
        Q1[n] = b1; Q2[n] = b2;
        if (pos != LS_NONE) BPn[n] = pos;
      }
    }
    for (int n = tid; n < S; n += NT) {
      if (a.in_off[s0 + n + 1] - a.in_off[s0 + n] > hub_thr) continue;       // a hub state: above
      float b1 = INF, b2 = INF;
      if (Rn[n] && Xn[n] != INF) {
        for (int64_t i = a.in_off[s0 + n]; i < a.in_off[s0 + n + 1]; ++i) {
          if (a.in_col[i] < 0) continue;
          const int m = a.in_src[i];
          if (P1[m] == INF) continue;
          const int ai = (int)(i - in0);
          const float ac = ac_cost(ai, f), g = arc_w(ai), tot = (D[m] + ac) + g;
          if (!(tot < pcut[f + 1])) continue;
          const float le = Xn[n] + (tot - Dn[n]);
          if (!(le <= beamL)) continue;
          const float c1 = P1[m] + g, c2 = P2[m] + ac;
          if (b1 == INF || ls_less(c1, c2, b1, b2)) { b1 = c1; b2 = c2; BPn[n] = ai; }
        }
      }
      Q1[n] = b1; Q2[n] = b2;
    }
    __syncthreads();
    if (!eps_rounds(f + 1, Q1, Q2)) { fail(KHG_LAT_EPS_LOOP, -1); return; }
    float* t1 = P1; P1 = Q1; Q1 = t1;
    float* t2 = P2; P2 = Q2; Q2 = t2;
  }
  if (tid != 0) return;
  // the final state: strictly better totals in state order (ties: the lowest state)
  float fd1 = INF, fd2 = INF;
  int fp = -1;
  for (int n = 0; n < S; ++n) {
    if (P1[n] == INF || DT[n] == INF) continue;
    const float fc = a.final_w[s0 + n];
    if (fc == INF) continue;
    const float w1 = P1[n] + fc, w2 = P2[n] + 0.0f;
    if (fp < 0 || ls_less(w1, w2, fd1, fd2)) { fd1 = w1; fd2 = w2; fp = n; }
  }
  auto fail0 = [&](int st) {
    for (int t = 0; t < T; ++t) a.ali[f0 + t] = 0;
    a.num_words[u] = 0; a.like[u] = 0.0; a.status[u] = st; a.err_frame[u] = -1;
  };
  if (fp < 0) { fail0(KHG_LAT_NO_TRACEBACK); return; }
  // trace-back: the words come out last-first and are reversed in place
  const int64_t wcap = a.words_off[u + 1] - a.words_off[u];
  int32_t* words = a.words + a.words_off[u];
  int f = T, n = fp, nw = 0;
  const int64_t max_steps = (int64_t)(T + 1) * (S + 1);
  for (int64_t step = 0;; ++step) {
    const int bp = BProw[(int64_t)f * S + n];
    if (bp == -1 && f == 0 && n == start) break;
    if (bp < 0 || step > max_steps) { fail0(KHG_LAT_NO_TRACEBACK); return; }
    const int ol = a.in_olabel[in0 + bp];
    if (ol != 0) { if (nw < wcap) words[nw] = ol; ++nw; }
    if (a.in_col[in0 + bp] >= 0) {
      if (f == 0) { fail0(KHG_LAT_NO_TRACEBACK); return; }
      --f;
      a.ali[f0 + f] = a.in_tid[in0 + bp];
    }
    n = a.in_src[in0 + bp];
  }
  if (f != 0) { fail0(KHG_LAT_NO_TRACEBACK); return; }
  if (nw > wcap) { fail0(KHG_LAT_WORDS); return; }
  for (int i = 0, j = nw - 1; i < j; ++i, --j) { const int32_t w = words[i]; words[i] = words[j]; words[j] = w; }
  a.num_words[u] = nw;
  // GetLinearSymbolSequence multiplies the path's weights left to right from One(): the distance pairs above, plus the final weight
  a.like[u] = (double)(-(fd1 + fd2));
  a.status[u] = KHG_LAT_SUCCEEDED;
  a.err_frame[u] = -1;
}
