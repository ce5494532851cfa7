// K2W: scoring device-resident lattices (DESIGN.md section 7s; include/khg_hip.h states the rule in full): the word insertion penalty
// (khg_lattices_add_penalty: lattice-add-penalty), the oracle path against a reference (khg_lattices_oracle: lattice-oracle) and the
// sweep of score.sh (khg_lattices_wer: best path under (graph_scale, acoustic_scale, penalty) triples, then compute-wer's counts).
// Everything but the best path's float costs is int32 arithmetic, so host form, device form and restatement agree on every output.
//
// The oracle is a dynamic program over (lattice state, reference position): E[s][q], q = 0 .. R.  States depend on each other along the
// arcs, so an utterance is a serial loop over its states (every arc goes to a higher state); the width is the reference: ONE wave per
// utterance, lanes over q, 64 positions a segment.  A state takes its in-arcs in ascending arc number through the in-arc index of
// khg_lattices_posteriors (LatIndex); every lane reads the source's row at q and q - 1.  The deletion chain E[q] = min(C[q], E[q-1] + 1)
// is a wave prefix-min of C[q] - q with q added back (exact in integers; a carry goes from segment to segment), and "only when strictly
// smaller" is E < C.  Emitting arcs go one frame on and epsilon arcs stay in their frame, so a state reads rows of its own frame and the
// one before: those two frames' rows live in LDS as a ring of two halves when 2 * (widest frame) * (R + 1) * 4 bytes fit the launch's
// LDS; otherwise (or KHG_OPT_LAT_OPS_LDS = 1) the rows are read back from the HBM table.  Every row and its moves are written once to
// the HBM table [state][R + 1] for the trace-back, which lane 0 runs.  One wave per workgroup, so __syncthreads() is the only fence
// needed.  No atomics: nothing depends on timing.

#define SC_NT 64
#define SC_INF (1 << 30)
#define SC_MV_NONE (-1)                  // a move: the arc (EPS, DIAG), -3 - arc (INS), or one of these two
#define SC_MV_DEL (-2)

// ---- lattice-add-penalty, in place on a copy's graph costs ----
__global__ __launch_bounds__(256) void k2_lattice_score_add_penalty(float* g, const int32_t* olabel, int64_t na, float penalty) {
  for (int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x; a < na; a += (int64_t)gridDim.x * 256)
    if (olabel[a] != 0) g[a] = g[a] + penalty;
}

// the widest frame of every utterance of a chunk (states are ordered by frame): one lane per utterance, once per handle
__global__ __launch_bounds__(64) void k2_lattice_score_width(LoArgs p, int32_t* width) {
  const int b = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (b >= p.n) return;
  const int u = p.u0 + b;
  const int64_t s0 = p.state_off[u] - p.s_base;
  const int N = (int)(p.state_off[u + 1] - p.state_off[u]);
  int best = 0, run = 0;
  for (int s = 0; s < N; ++s) {
    run = s > 0 && p.in.frame[s0 + s] == p.in.frame[s0 + s - 1] ? run + 1 : 1;
    best = max(best, run);
  }
  width[u] = best;
}

struct ScArgs {
  LoArgs lo;                             // the chunk's lattices; ali / ali_off; status [U]; words [chunk states] (an utterance's from the END of its slice)
  const int32_t *in_begin, *in_arc, *arc_src;     // LatIndex
  const int32_t* list;                   // [launch] the utterances of the launch
  const int64_t* tab_off;                // [launch] the first cell of each one's table in `tab`: E [N][R + 1], then the moves [N][R + 1]
  int32_t* tab;
  const int32_t* width;                  // [U] the widest frame
  const int32_t* ref;                    // the references, one after the other
  const int64_t* ref_off;                // [U + 1]
  int32_t* counts;                       // [U][4] errors, insertions, deletions, substitutions
  int32_t* nwords;                       // [U]
};

// the inclusive prefix-min over the lanes
__device__ __forceinline__ int sc_prefix_min(int v, int lane) {
  for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(v, o); if (lane >= o) v = min(v, t); }
  return v;
}

// The rows of every state, in state order.  RING: ring [2][fw][W] holds the rows of the current frame and the one before.
template <bool RING>
__device__ __forceinline__ void sc_oracle_rows(int N, int W, int start, int fw, const int32_t* frame, const int32_t* ib, const int32_t* in_arc,
                                               const int32_t* arc_src, const int32_t* ol, const int32_t* ref, int32_t* E, int32_t* M, int32_t* ring) {
  const int lane = (int)threadIdx.x;
  int lo = 0, plo = 0, cur = 0;          // the current frame's states start at lo, the states of the one before at plo; cur: the current frame's half
  for (int s = 0; s < N; ++s) {
    if (s > 0 && frame[s] != frame[s - 1]) { plo = lo; lo = s; cur ^= 1; }
    const int j0 = ib[s], j1 = ib[s + 1];
    int carry = INT_MAX;
    for (int qb = 0; qb < W; qb += SC_NT) {
      const int q = qb + lane;
      const bool in = q < W;
      int C = s == start && q == 0 ? 0 : SC_INF, mv = SC_MV_NONE;
      for (int j = j0; j < j1; ++j) {
        const int a = in_arc[j], src = arc_src[a], w = ol[a];
        int e0 = SC_INF, e1 = SC_INF;
        if (in) {
          if (RING && src >= plo) {
            const int32_t* row = ring + ((int64_t)(src >= lo ? cur : cur ^ 1) * fw + (src - (src >= lo ? lo : plo))) * W;
            e0 = row[q];
            if (q > 0) e1 = row[q - 1];
          } else {
            const int32_t* row = E + (int64_t)src * W;
            e0 = row[q];
            if (q > 0) e1 = row[q - 1];
          }
        }
        if (w == 0) {
          if (e0 < C) { C = e0; mv = a; }                                      // EPS (an unreachable cell holds SC_INF: never < C)
        } else {
          if (e1 < SC_INF) { const int c = e1 + (w != ref[q - 1] ? 1 : 0); if (c < C) { C = c; mv = a; } }      // DIAG
          if (e0 < SC_INF) { const int c = e0 + 1; if (c < C) { C = c; mv = -3 - a; } }                         // INS
        }
      }
      // DEL: E[q] = min over j <= q of C[j] + (q - j)
      const int v = min(sc_prefix_min(in ? C - q : INT_MAX, lane), carry);
      carry = __shfl(v, 63);
      if (in) {
        const int e = v + q;
        if (e < C) mv = SC_MV_DEL;
        E[(int64_t)s * W + q] = e;
        M[(int64_t)s * W + q] = mv;
        if (RING) ring[((int64_t)cur * fw + (s - lo)) * W + q] = e;
      }
    }
    __syncthreads();
  }
}

// an utterance without an oracle path: the reference's words are all deleted
__device__ __forceinline__ void sc_fail(const ScArgs& p, int u, int R, int st) {
  p.lo.status[u] = st; p.nwords[u] = 0;
  p.counts[4 * (int64_t)u] = R; p.counts[4 * (int64_t)u + 1] = 0; p.counts[4 * (int64_t)u + 2] = R; p.counts[4 * (int64_t)u + 3] = 0;
}

__global__ __launch_bounds__(SC_NT) void k2_lattice_score_oracle(ScArgs p) {
  extern __shared__ int32_t sc_lds[];
  const int k = (int)blockIdx.x, u = p.list[k], b = u - p.lo.u0, lane = (int)threadIdx.x;
  const int64_t s0 = p.lo.state_off[u] - p.lo.s_base, a0 = p.lo.arc_off[u] - p.lo.a_base;
  const int N = (int)(p.lo.state_off[u + 1] - p.lo.state_off[u]), A = (int)(p.lo.arc_off[u + 1] - p.lo.arc_off[u]);
  const int R = (int)(p.ref_off[u + 1] - p.ref_off[u]), W = R + 1;
  const int32_t* frame = p.lo.in.frame + s0;
  const int32_t* next = p.lo.in.next + a0;
  const int32_t* ol = p.lo.in.olabel + a0;
  const int32_t* il = p.lo.in.ilabel + a0;
  const int32_t* ib = p.in_begin + s0 + b;
  const int32_t* in_arc = p.in_arc + a0;
  const int32_t* arc_src = p.arc_src + a0;
  const int32_t* ref = p.ref + p.ref_off[u];
  const int start = N ? p.lo.start[u] : -1;
  if (N == 0 || start < 0 || start >= N) { if (lane == 0) sc_fail(p, u, R, KHG_LAT_NO_PATH); return; }
  bool bad = false;
  for (int a = lane; a < A; a += SC_NT) bad = bad || next[a] <= arc_src[a];
  if (__ballot(bad)) { if (lane == 0) sc_fail(p, u, R, KHG_LAT_EPS_LOOP); return; }
  int32_t* E = p.tab + p.tab_off[k];
  int32_t* M = E + (int64_t)N * W;
  const int fw = p.width[u];
  if (8 * (int64_t)fw * W <= (int64_t)p.lo.lds_bytes) sc_oracle_rows<true>(N, W, start, fw, frame, ib, in_arc, arc_src, ol, ref, E, M, sc_lds);
  else sc_oracle_rows<false>(N, W, start, fw, frame, ib, in_arc, arc_src, ol, ref, E, M, nullptr);
  // the final state: the last frame's, the least E[f][R], the lowest state among ties
  const int T = frame[N - 1];
  long long best = LLONG_MAX;
  for (int s = N - 1 - lane; s >= 0 && frame[s] == T; s -= SC_NT) {
    if (p.lo.in.fin[s0 + s] == __builtin_huge_valf()) continue;
    const int e = E[(int64_t)s * W + R];
    if (e < SC_INF) best = min(best, ((long long)e << 32) | (long long)s);
  }
  for (int o = 32; o; o >>= 1) best = min(best, __shfl_xor(best, o));
  if (lane != 0) return;
  if (best == LLONG_MAX) { sc_fail(p, u, R, KHG_LAT_NO_PATH); return; }
  // the trace-back: the words come out last first, so they fill the utterance's slice from its end
  int32_t* ali = p.lo.ali + p.lo.ali_off[u];
  const int TA = (int)(p.lo.ali_off[u + 1] - p.lo.ali_off[u]);
  int32_t* words = p.lo.words + s0;
  int s = (int)(best & 0x7fffffffLL), q = R, nw = 0, ins = 0, del = 0, sub = 0;
  for (int64_t steps = 0;; ++steps) {
    const int mv = M[(int64_t)s * W + q];
    if (mv == SC_MV_NONE) break;
    if (steps > (int64_t)N + W) { sc_fail(p, u, R, KHG_LAT_NO_PATH); return; }
    if (mv == SC_MV_DEL) { ++del; --q; continue; }
    const int a = mv >= 0 ? mv : -3 - mv;
    const int w = ol[a], src = arc_src[a];
    if (mv < 0) ++ins;
    else if (w != 0) { --q; if (w != ref[q]) ++sub; }
    if (w != 0 && nw < N) { ++nw; words[N - nw] = w; }
    const int t = il[a], f = frame[src];
    if (t != 0 && f >= 0 && f < TA) ali[f] = t;
    s = src;
  }
  if (s != start || q != 0) { sc_fail(p, u, R, KHG_LAT_NO_PATH); return; }
  p.counts[4 * (int64_t)u] = ins + del + sub; p.counts[4 * (int64_t)u + 1] = ins; p.counts[4 * (int64_t)u + 2] = del; p.counts[4 * (int64_t)u + 3] = sub;
  p.nwords[u] = nw;
  p.lo.status[u] = KHG_LAT_SUCCEEDED;
}

// ---- the sweep: k2_lattice_best_path's walk with the penalty on the arcs that carry a word, one lane per triple ----
struct ScBpArgs {
  LoArgs lo;                             // as khg_lattices_best_path fills it (no ali, no weight)
  const float* pen;                      // [K]
};

// lo_forward with w1 = fl(fl(gs * graph_cost) + penalty) on an arc with olabel != 0 (ol: the utterance's olabels)
__device__ __forceinline__ int sc_forward(const LoView& v, const LoLane& L, float pen, const int32_t* ol, int* last_lo) {
#pragma clang fp contract(off)
  const float INF = __builtin_huge_valf();
  const int64_t K = L.K;
  for (int s = 0; s < v.N; ++s) { L.d1[s * K] = INF; L.d2[s * K] = INF; L.bp[s * K] = -1; }
  L.d1[v.start * K] = 0.0f; L.d2[v.start * K] = 0.0f;
  int lo = 0, plo = 0;
  while (lo < v.N) {
    const int f = v.frame[lo];
    int hi = lo + 1;
    while (hi < v.N && v.frame[hi] == f) ++hi;
    if (lo > 0)
      for (int m = plo; m < lo; ++m) {
        const float dm1 = L.d1[m * K];
        if (dm1 == INF) continue;
        const float dm2 = L.d2[m * K];
        const int ae = lo_aend(v, m);
        for (int a = v.abeg[m]; a < ae; ++a) {
          if (v.il[a] == 0) continue;
          const int n = v.next[a];
          float w1 = L.gs * v.gc[a];
          const float w2 = L.as * v.ac[a];
          if (ol[a] != 0) w1 = w1 + pen;
          const float c1 = dm1 + w1, c2 = dm2 + w2;
          const float b1 = L.d1[n * K];
          if (b1 == INF || lo_less(c1, c2, b1, L.d2[n * K])) { L.d1[n * K] = c1; L.d2[n * K] = c2; L.bp[n * K] = a; }
        }
      }
    for (int round = 0;; ++round) {
      bool changed = false;
      for (int n = lo; n < hi; ++n) { L.n1[n * K] = L.d1[n * K]; L.n2[n * K] = L.d2[n * K]; }
      for (int m = lo; m < hi; ++m) {
        const float dm1 = L.d1[m * K];
        if (dm1 == INF) continue;
        const float dm2 = L.d2[m * K];
        const int ae = lo_aend(v, m);
        for (int a = v.abeg[m]; a < ae; ++a) {
          if (v.il[a] != 0) continue;
          const int n = v.next[a];
          float w1 = L.gs * v.gc[a];
          if (ol[a] != 0) w1 = w1 + pen;
          const float c1 = dm1 + w1, c2 = dm2 + 0.0f;
          const float b1 = L.n1[n * K];
          if (b1 == INF || lo_less(c1, c2, b1, L.n2[n * K])) { L.n1[n * K] = c1; L.n2[n * K] = c2; L.bp[n * K] = a; changed = true; }
        }
      }
      if (!changed) break;
      for (int n = lo; n < hi; ++n) { L.d1[n * K] = L.n1[n * K]; L.d2[n * K] = L.n2[n * K]; }
      if (round > hi - lo) return KHG_LAT_EPS_LOOP;
    }
    plo = lo; lo = hi;
  }
  *last_lo = plo;
  return 0;
}

__device__ __forceinline__ void sc_bp_fail(const LoArgs& p, int64_t o, int st) { p.status[o] = st; p.nwords[o] = 0; }

__global__ __launch_bounds__(LO_NT) void k2_lattice_score_best_path(ScBpArgs q) {
#pragma clang fp contract(off)
  extern __shared__ int32_t lo_lds[];
  const LoArgs& p = q.lo;
  const int u = p.u0 + (int)blockIdx.x;
  const LoView v = lo_view(p, u, lo_lds);
  const int k = (int)blockIdx.y * LO_NT + (int)threadIdx.x;
  if (k >= p.K) return;
  const int64_t o = (int64_t)k * p.U + u;
  if (v.N == 0 || v.start < 0) { sc_bp_fail(p, o, KHG_LAT_NO_PATH); return; }
  const int64_t base = (p.state_off[u] - p.s_base) * p.K;
  const int32_t* ol = p.in.olabel + (p.arc_off[u] - p.a_base);
  LoLane L;
  L.gs = p.gs[k]; L.as = p.as[k]; L.K = p.K;
  L.d1 = p.d1 + base + k; L.d2 = p.d2 + base + k; L.n1 = p.n1 + base + k; L.n2 = p.n2 + base + k; L.bp = p.bp + base + k;
  int last_lo = 0;
  if (sc_forward(v, L, q.pen[k], ol, &last_lo)) { sc_bp_fail(p, o, KHG_LAT_EPS_LOOP); return; }
  float f1, f2;
  const int fin = lo_final(v, L, last_lo, &f1, &f2);
  if (fin < 0) { sc_bp_fail(p, o, KHG_LAT_NO_PATH); return; }
  int32_t* pn = reinterpret_cast<int32_t*>(L.n1);        // (the Jacobi rows are free now)
  const int steps = lo_chain(v, L, pn, fin);
  if (steps < 0) { sc_bp_fail(p, o, KHG_LAT_NO_PATH); return; }
  int32_t* words = p.words + base + (int64_t)k * v.N;
  int n = v.start, nw = 0;
  for (int i = 0; i < steps; ++i) {
    const int a = pn[n * L.K];
    const int w = ol[a];
    if (w != 0) { if (nw < v.N) words[nw] = w; ++nw; }
    n = v.next[a];
  }
  if (nw > v.N) { sc_bp_fail(p, o, KHG_LAT_WORDS); return; }
  p.nwords[o] = nw;
  p.status[o] = KHG_LAT_SUCCEEDED;
}

// ---- compute-wer's counts of one (triple, utterance): the oracle's rule on the chain of the hypothesis words.  One wave, lanes over q.
// The table -- two rows of E (int32) and the moves [H + 1][R + 1] (a byte each: 0 none, 1 DIAG, 2 INS, 3 DEL) -- lies in LDS when it
// fits the launch's, else at hb_off[o] (bytes, a multiple of 4) in `hb`.
struct ScWerArgs {
  LoArgs lo;                             // words / nwords / status as k2_lattice_score_best_path left them
  const int32_t* ref;
  const int64_t* ref_off;                // [U + 1]
  unsigned char* hb;
  const int64_t* hb_off;                 // [K * U]; -1: the table fits the LDS
  int32_t* counts;                       // [K * U][4]
};

// e: two rows of E; mvs: the moves.  Instantiated once for LDS and once for HBM, so that each uses its own address space's loads and
// stores (a pointer that may be either would make them flat ones, and a flat access is placed by its base register alone: &prev[q - 1]
// of lane 0 in the first LDS row lies below the LDS aperture)
template <class E, class M>
__device__ __forceinline__ void sc_wer_table(const ScWerArgs& p, int64_t o, int H, int W, const int32_t* hyp, const int32_t* ref, E e, M mvs) {
  const int lane = (int)threadIdx.x, R = W - 1;
  for (int i = 0; i <= H; ++i) {
    const int pr = (i + 1) & 1, cr = i & 1;
    const int w = i ? hyp[i - 1] : 0;
    int carry = INT_MAX;
    for (int qb = 0; qb < W; qb += SC_NT) {
      const int q = qb + lane;
      const bool in = q < W;
      int C = i == 0 && q == 0 ? 0 : SC_INF, mv = 0;
      if (in && i > 0) {
        const int e0 = e[(int64_t)pr * W + q], e1 = q > 0 ? e[(int64_t)pr * W + q - 1] : SC_INF;
        if (e1 < SC_INF) { const int c = e1 + (w != ref[q - 1] ? 1 : 0); if (c < C) { C = c; mv = 1; } }
        if (e0 < SC_INF) { const int c = e0 + 1; if (c < C) { C = c; mv = 2; } }
      }
      const int v = min(sc_prefix_min(in ? C - q : INT_MAX, lane), carry);
      carry = __shfl(v, 63);
      if (in) {
        const int ee = v + q;
        if (ee < C) mv = 3;
        e[(int64_t)cr * W + q] = ee;
        mvs[(int64_t)i * W + q] = (unsigned char)mv;
      }
    }
    __syncthreads();
  }
  if (lane != 0) return;
  int i = H, q = R, ins = 0, del = 0, sub = 0;
  while (i > 0 || q > 0) {
    const int mv = mvs[(int64_t)i * W + q];
    if (mv == 1 && i > 0 && q > 0) { --i; --q; if (hyp[i] != ref[q]) ++sub; }
    else if (mv == 2 && i > 0) { --i; ++ins; }
    else if (mv == 3 && q > 0) { --q; ++del; }
    else break;
  }
  p.counts[4 * o] = ins + del + sub; p.counts[4 * o + 1] = ins; p.counts[4 * o + 2] = del; p.counts[4 * o + 3] = sub;
}

__global__ __launch_bounds__(SC_NT) void k2_lattice_score_wer(ScWerArgs p) {
  extern __shared__ int32_t sc_lds[];
  const int u = p.lo.u0 + (int)blockIdx.x, k = (int)blockIdx.y;
  const int64_t o = (int64_t)k * p.lo.U + u;
  const int N = (int)(p.lo.state_off[u + 1] - p.lo.state_off[u]);
  const int W = (int)(p.ref_off[u + 1] - p.ref_off[u]) + 1;
  const int H = (p.lo.status[o] & KHG_LAT_SUCCEEDED) ? p.lo.nwords[o] : 0;
  const int32_t* ref = p.ref + p.ref_off[u];
  const int32_t* hyp = p.lo.words + (p.lo.state_off[u] - p.lo.s_base) * p.lo.K + (int64_t)k * N;
  const int64_t off = p.hb_off[o];
  if (off < 0) sc_wer_table(p, o, H, W, hyp, ref, sc_lds, reinterpret_cast<unsigned char*>(sc_lds + 2 * (int64_t)W));
  else sc_wer_table(p, o, H, W, hyp, ref, reinterpret_cast<int32_t*>(p.hb + off), p.hb + off + 8 * (int64_t)W);
}
