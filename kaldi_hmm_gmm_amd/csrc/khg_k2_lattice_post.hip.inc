// K2P: forward-backward posteriors of device-resident raw lattices (khg_lattices_posteriors: LatticeForwardBackward / lattice-to-post).
// The rule is DESIGN.md section 7g: the log-semiring pass in float64 under one (graph_scale, acoustic_scale) pair -- alpha, beta, the
// total log-likelihood, arc posteriors, and per frame the emitting arcs' posteriors merged by transition-id, ascending.
//
// One pair, so the width comes from the lattice: one workgroup (four waves) per utterance, lanes over the states of a frame (a state
// gathers its in-arcs through the handle's in-arc index; a state with more than PO_HUB arcs is taken by a whole wave), then lanes over
// arcs for the posteriors and the merge.  Inside a frame the epsilon arcs are closed by Jacobi rounds: every state's full sum is
// recomputed from the values of the round before (row -> alpha after a barrier) until no value's bits change; admissible lattices
// (every epsilon arc goes to a higher state: checked first, KHG_LAT_EPS_LOOP otherwise) settle after (longest chain + 1) rounds.
// Every sum is a max-then-sum log-sum-exp in a fixed order (lane: the arcs in order; wave: lane-strided, then a butterfly whose
// partners add the same two numbers), so results do not depend on timing or on the batch.  No atomics of any kind.
// The lattice is staged by lo_view and alpha / beta / the Jacobi row live in LDS when 24 N + 4 (3 N + 4 A) bytes fit the limit;
// otherwise (or KHG_OPT_LAT_OPS_LDS = 1) the same code reads the HBM arrays and HBM scratch [state].
// Every phase is a __device__ __forceinline__ piece (po_open, po_admissible, po_frames, po_sweep, po_alpha_total_beta, po_merge) that
// k2_lattice_post_mpe (khg_k2_lattice_mpe.hip.inc) calls as well: the two kernels' bit-equal likelihood part is one text.  All threads
// of the workgroup call a piece together; every early return inside one is workgroup-uniform.

#define PO_NT 256
#define PO_HUB 64

struct PoArgs {
  LoArgs lo;                                     // the chunk's lattice arrays; status, ali_off, utt_tot, utt_off
  const int32_t *in_begin, *in_arc, *arc_src;    // the handle's index: in_begin at [chunk state + utterance in chunk], N + 1 per utterance
  double gs, as;
  double *alpha, *beta, *row;                    // HBM scratch, [chunk states]
  double* arc_post;                              // [chunk arcs]
  int32_t *flag, *rank;                          // [chunk arcs]: 0 dead or epsilon, 1 live, 2 + r the first arc of its id in the frame, of rank r
  int32_t *fcnt, *fstate;                        // [chunk frames]: entries per frame, then their exclusive prefix; [chunk frames + 2 n]: first state of a frame
  int64_t f_base;                                // ali_off[u0]
  double* tot;                                   // [U]
  int64_t* entry_begin;                          // [chunk frames kept + 1]
  int32_t* tid;                                  // [chunk entries]
  double* weight;
};

// ---- the in-arc index: in_begin[N + 1], in_arc[A] (a state's in-arcs in global arc order), arc_src[A].  One wave per utterance walks
// the arcs in tiles of 64: a lane ranks its arc among the tile's arcs into the same state by shuffles, and the last lane of each group
// moves that state's cursor on, so every position is a function of the arc order alone. ----
__device__ __forceinline__ void po_tile_rank(int n, int lane, int* r, int* c) {
  int rr = 0, cc = 0;
  for (int j = 0; j < 64; ++j) {
    const int nj = __shfl(n, j);
    if (nj == n) { ++cc; if (j < lane) ++rr; }
  }
  *r = rr; *c = cc;
}

__global__ __launch_bounds__(64) void k2_lattice_post_index(LoArgs p, int32_t* in_begin, int32_t* in_arc, int32_t* arc_src, int32_t* cur) {
  const int b = (int)blockIdx.x, u = p.u0 + b, lane = (int)threadIdx.x;
  const int64_t s0 = p.state_off[u] - p.s_base, a0 = p.arc_off[u] - p.a_base;
  const int N = (int)(p.state_off[u + 1] - p.state_off[u]), A = (int)(p.arc_off[u + 1] - p.arc_off[u]);
  int32_t* ib = in_begin + s0 + b;
  int32_t* cu = cur + s0;
  const int32_t* abeg = p.in.arc_begin + s0;
  const int32_t* next = p.in.next + a0;
  for (int s = lane; s < N; s += 64) {
    const int ae = s + 1 < N ? abeg[s + 1] : A;
    for (int a = abeg[s]; a < ae; ++a) arc_src[a0 + a] = s;
    cu[s] = 0;
  }
  __syncthreads();
  for (int base = 0; base < A; base += 64) {          // in-degrees
    const int a = base + lane;
    const int n = a < A ? next[a] : -1 - lane;
    int r, c;
    po_tile_rank(n, lane, &r, &c);
    if (a < A && r == c - 1) cu[n] += c;
    __syncthreads();
  }
  int tot = 0;
  for (int sb = 0; sb < N; sb += 64) {                // exclusive prefix
    const int s = sb + lane;
    const int c = s < N ? cu[s] : 0;
    int incl = c;
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o); if (lane >= o) incl += t; }
    if (s < N) { ib[s] = tot + incl - c; cu[s] = tot + incl - c; }
    tot += __shfl(incl, 63);
  }
  if (lane == 0) ib[N] = tot;
  __syncthreads();
  for (int base = 0; base < A; base += 64) {          // placement
    const int a = base + lane;
    const int n = a < A ? next[a] : -1 - lane;
    int r, c;
    po_tile_rank(n, lane, &r, &c);
    if (a < A) {
      const int at = cu[n];
      in_arc[a0 + at + r] = a;
      if (r == c - 1) cu[n] = at + c;
    }
    __syncthreads();
  }
}

// ---- log-sum-exp of init and term(0 .. n - 1), max first: one lane in order, or one wave (all 64 lanes call it) ----
template <class Term>
__device__ __forceinline__ double po_lse_lane(double init, int n, Term term) {
#pragma clang fp contract(off)
  const double NINF = -__builtin_huge_val();
  double m = init;
  for (int i = 0; i < n; ++i) m = fmax(m, term(i));
  if (m == NINF) return NINF;
  double sum = exp(init - m);
  for (int i = 0; i < n; ++i) sum += exp(term(i) - m);
  return m + log(sum);
}
template <class Term>
__device__ __forceinline__ double po_lse_wave(double init, int n, Term term, int lane) {
#pragma clang fp contract(off)
  const double NINF = -__builtin_huge_val();
  double m = lane == 0 ? init : NINF;
  for (int i = lane; i < n; i += 64) m = fmax(m, term(i));
  for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o));
  if (m == NINF) return NINF;
  double sum = lane == 0 ? exp(init - m) : 0.0;
  for (int i = lane; i < n; i += 64) sum += exp(term(i) - m);
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  return m + log(sum);
}

// an arc's log-likelihood under the pair (the two products are exact in double: 24-bit factors)
__device__ __forceinline__ double po_w(const LoView& v, double gs, double as, int a) {
#pragma clang fp contract(off)
  const double g = gs * (double)v.gc[a];
  const double c = v.il[a] != 0 ? as * (double)v.ac[a] : 0.0;
  return -(g + c);
}

__device__ __forceinline__ bool po_differs(double a, double b) { return __double_as_longlong(a) != __double_as_longlong(b); }

// ---- one utterance of a launch, as every phase below sees it ----
struct PoView {
  LoView v;                                      // the lattice: staged in LDS, or the HBM arrays
  int b, u, N, A, T;                             // block, utterance; states, arcs; the last state's frame
  int64_t s0, a0;                                // the utterance's first state / arc in the chunk
  bool in_lds;                                   // workgroup-uniform: the doubles per state and the lattice are in LDS
  double *alpha, *beta, *row;                    // [N]
  const int32_t *asrc, *ib, *ia;                 // the in-arc index: arc_src [A], in_begin [N + 1], in_arc [A]
  int32_t *fs, *fc;                              // [T + 2]: frame f holds the states fs[f] .. fs[f + 1]; [T]: entries per frame
  int32_t *flag, *rank;                          // [A]
  double gs, as;
};
// All threads of the workgroup.  DOUBLES per state lie in front of the staged lattice (alpha, beta, row; an MPE launch: A and B behind
// them), in LDS when DOUBLES * 8 N + 4 (3 N + 4 A) bytes fit the launch's limit; ends with a barrier when it staged.
template <int DOUBLES>
__device__ __forceinline__ PoView po_open(const PoArgs& p, double* lds) {
  PoView w;
  w.b = (int)blockIdx.x; w.u = p.lo.u0 + w.b;
  w.s0 = p.lo.state_off[w.u] - p.lo.s_base; w.a0 = p.lo.arc_off[w.u] - p.lo.a_base;
  w.N = (int)(p.lo.state_off[w.u + 1] - p.lo.state_off[w.u]); w.A = (int)(p.lo.arc_off[w.u + 1] - p.lo.arc_off[w.u]);
  const int64_t need = 8 * DOUBLES * (int64_t)w.N + 4 * (3 * (int64_t)w.N + 4 * (int64_t)w.A);
  w.in_lds = need <= (int64_t)p.lo.lds_bytes;
  w.v = lo_view(p.lo, w.u, w.in_lds ? reinterpret_cast<int32_t*>(lds + DOUBLES * (size_t)w.N) : nullptr);
  w.alpha = w.in_lds ? lds : p.alpha + w.s0;
  w.beta = w.in_lds ? lds + w.N : p.beta + w.s0;
  w.row = w.in_lds ? lds + 2 * (size_t)w.N : p.row + w.s0;
  w.asrc = p.arc_src + w.a0; w.ib = p.in_begin + w.s0 + w.b; w.ia = p.in_arc + w.a0;
  const int64_t f0 = p.lo.ali_off[w.u] - p.f_base;
  w.T = (int)(p.lo.ali_off[w.u + 1] - p.lo.ali_off[w.u]);
  w.fs = p.fstate + f0 + 2 * (int64_t)w.b; w.fc = p.fcnt + f0;
  w.flag = p.flag + w.a0; w.rank = p.rank + w.a0;
  w.gs = p.gs; w.as = p.as;
  return w;
}

// admissible: every epsilon arc goes to a higher state (all threads: one barrier)
__device__ __forceinline__ bool po_admissible(const PoView& w) {
  int bad = 0;
  for (int a = (int)threadIdx.x; a < w.A; a += PO_NT) if (w.v.il[a] == 0 && w.v.next[a] <= w.asrc[a]) bad = 1;
  return !__syncthreads_or(bad);
}

// the frame table, alpha = beta = -inf and the frames' counts cleared; the caller's barrier follows
__device__ __forceinline__ void po_frames(const PoView& w) {
  const double NINF = -__builtin_huge_val();
  const int tid = (int)threadIdx.x;
  for (int s = tid; s < w.N; s += PO_NT) {
    const int f = w.v.frame[s], pf = s ? w.v.frame[s - 1] : -1;
    for (int g = pf + 1; g <= f; ++g) w.fs[g] = s;
    w.alpha[s] = NINF; w.beta[s] = NINF;
  }
  for (int t = tid; t < w.T; t += PO_NT) w.fc[t] = 0;
  if (tid == 0) w.fs[w.T + 1] = w.N;
}

// a state's arcs in a sweep's direction -- forward its in-arcs (through the index), backward its out-arcs -- as positions i0 .. i0 + deg;
// po_arc turns a position into the arc
template <bool FWD>
__device__ __forceinline__ void po_range(const PoView& w, int s, int* i0, int* deg) {
  if (FWD) { *i0 = w.ib[s]; *deg = w.ib[s + 1] - *i0; }
  else { *i0 = w.v.abeg[s]; *deg = lo_aend(w.v, s) - *i0; }
}
template <bool FWD>
__device__ __forceinline__ int po_arc(const PoView& w, int pos) { return FWD ? w.ia[pos] : pos; }

// ---- one pass over the frames, first to last (FWD) or last to first.  Inside a frame, Jacobi rounds: a lane takes a state of at most
// PO_HUB arcs, cur[s]'s next value being lane_val(s, f, i0, deg); a whole wave takes a hub state, wave_val(s, f, i0, deg, lane) (all 64
// lanes call it, lane 0 keeps it).  The values go to row, and to cur behind a barrier, until no value's bits change; a frame without
// epsilon arcs (seen in round 0) takes one round.  false: a frame did not settle (not reached on an admissible lattice). ----
template <bool FWD, class LaneVal, class WaveVal>
__device__ __forceinline__ bool po_sweep(const PoView& w, double* cur, LaneVal lane_val, WaveVal wave_val) {
#pragma clang fp contract(off)
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int k = 0; k <= w.T; ++k) {
    const int f = FWD ? k : w.T - k;
    const int lo = w.fs[f], hi = w.fs[f + 1];
    int has_eps = 0;
    for (int round = 0;; ++round) {
      int changed = 0, eps = 0;
      for (int s = lo + tid; s < hi; s += PO_NT) {                    // lanes over states
        int i0, deg;
        po_range<FWD>(w, s, &i0, &deg);
        if (deg > PO_HUB) continue;
        if (round == 0) for (int i = 0; i < deg; ++i) eps |= w.v.il[po_arc<FWD>(w, i0 + i)] == 0;
        const double val = lane_val(s, f, i0, deg);
        w.row[s] = val;
        changed |= po_differs(val, cur[s]);
      }
      for (int s = lo + wave; s < hi; s += PO_NT / 64) {              // hub states: the wave over a state's arcs
        int i0, deg;
        po_range<FWD>(w, s, &i0, &deg);
        if (deg <= PO_HUB) continue;
        if (round == 0) for (int i = lane; i < deg; i += 64) eps |= w.v.il[po_arc<FWD>(w, i0 + i)] == 0;
        const double val = wave_val(s, f, i0, deg, lane);
        if (lane == 0) { w.row[s] = val; changed |= po_differs(val, cur[s]); }
      }
      if (round == 0) has_eps = __syncthreads_or(eps);               // (the reduction gives 0 or 1: one call per flag)
      if (!__syncthreads_or(changed)) break;                          // no value's bits changed
      for (int s = lo + tid; s < hi; s += PO_NT) cur[s] = w.row[s];
      __syncthreads();
      if (!has_eps) break;
      if (round > hi - lo) return false;
    }
  }
  return true;
}

// ---- alpha, the total over the last frame's final states (through *sh_tot, a __shared__ of the kernel), beta.  *settled = false: the
// forward pass did not settle, nothing after it ran.  A total of -inf: no path, beta did not run. ----
__device__ __forceinline__ double po_alpha_total_beta(const PoView& w, double* sh_tot, bool* settled) {
#pragma clang fp contract(off)
  const double NINF = -__builtin_huge_val();
  const float FINF = __builtin_huge_valf();
  const LoView& v = w.v;
  const double gs = w.gs, as = w.as;
  const double *alpha = w.alpha, *beta = w.beta;
  const int lane = (int)threadIdx.x & 63;
  {
    auto init = [&](int s) { return s == v.start ? 0.0 : NINF; };
    auto term = [&](int pos) { const int a = w.ia[pos]; return alpha[w.asrc[a]] + po_w(v, gs, as, a); };
    *settled = po_sweep<true>(w, w.alpha,
                              [&](int s, int, int i0, int deg) { return po_lse_lane(init(s), deg, [&](int i) { return term(i0 + i); }); },
                              [&](int s, int, int i0, int deg, int ln) { return po_lse_wave(init(s), deg, [&](int i) { return term(i0 + i); }, ln); });
  }
  if (!*settled) return NINF;
  if (threadIdx.x < 64) {
    const int lo = w.fs[w.T];
    const double t = po_lse_wave(NINF, w.N - lo, [&](int i) { const float c = v.fin[lo + i]; return c == FINF ? NINF : alpha[lo + i] + -(gs * (double)c); }, lane);
    if (lane == 0) *sh_tot = t;
  }
  __syncthreads();
  const double tot = *sh_tot;
  if (tot == NINF) return tot;
  {                                                                   // backward: the same over out-arcs
    auto init = [&](int s, int f) { const float c = v.fin[s]; return f == w.T && c != FINF ? -(gs * (double)c) : NINF; };
    auto term = [&](int a) { return po_w(v, gs, as, a) + beta[v.next[a]]; };
    (void)po_sweep<false>(w, w.beta,
                          [&](int s, int f, int e0, int deg) { return po_lse_lane(init(s, f), deg, [&](int i) { return term(e0 + i); }); },
                          [&](int s, int f, int e0, int deg, int ln) { return po_lse_wave(init(s, f), deg, [&](int i) { return term(e0 + i); }, ln); });
  }
  return tot;
}

// ---- the per-frame merge's ranks and counts over the live flags (0 / 1 in flag, a barrier behind them), and the frames' exclusive
// prefix: the emitting arcs that leave frame f are the arc range of its states.  Returns the utterance's entry count in wave 0. ----
__device__ __forceinline__ int po_merge(const PoView& w) {
  const LoView& v = w.v;
  const int tid = (int)threadIdx.x, lane = tid & 63, N = w.N, A = w.A, T = w.T;
  int32_t *flag = w.flag, *rank = w.rank, *fs = w.fs, *fc = w.fc;
  // the first live arc of every id ...
  for (int a = tid; a < A; a += PO_NT) {
    int first = -1;
    if (flag[a]) {
      const int id = v.il[a], r0 = v.abeg[fs[v.frame[w.asrc[a]]]];
      first = 0;
      for (int k = r0; k < a; ++k) if (flag[k] && v.il[k] == id) { first = -1; break; }
    }
    rank[a] = first;
  }
  __syncthreads();
  // ... is ranked among the frame's ids, and the one with the highest id leaves the frame's count
  for (int a = tid; a < A; a += PO_NT) {
    if (rank[a] != 0) continue;
    const int id = v.il[a], f = v.frame[w.asrc[a]], r0 = v.abeg[fs[f]], hs = fs[f + 1], r1 = hs < N ? v.abeg[hs] : A;
    int r = 0, cnt = 0;
    for (int k = r0; k < r1; ++k) if (rank[k] == 0) { ++cnt; r += v.il[k] < id; }
    flag[a] = 2 + r;
    if (r == cnt - 1 && f < T) fc[f] = cnt;
  }
  __syncthreads();
  int sum = 0;
  if (tid < 64)                                                       // exclusive prefix of the frames' counts
    for (int tb = 0; tb < T; tb += 64) {
      const int t = tb + lane;
      const int c = t < T ? fc[t] : 0;
      int incl = c;
      for (int o = 1; o < 64; o <<= 1) { const int x = __shfl_up(incl, o); if (lane >= o) incl += x; }
      if (t < T) fc[t] = sum + incl - c;
      sum += __shfl(incl, 63);
    }
  return sum;
}
// what a kernel leaves for an utterance without SUCCEEDED (all threads) ...
__device__ __forceinline__ void po_fail(const PoArgs& p, const PoView& w, int st) {
  if (threadIdx.x == 0) {
    p.lo.status[w.u] = st; p.tot[w.u] = -__builtin_huge_val();
    p.lo.utt_tot[2 * (int64_t)w.b] = 0; p.lo.utt_tot[2 * (int64_t)w.b + 1] = 0;
  }
  for (int a = (int)threadIdx.x; a < w.A; a += PO_NT) p.arc_post[w.a0 + a] = 0.0;
}
// ... and for one that succeeded (thread 0, after po_merge)
__device__ __forceinline__ void po_done(const PoArgs& p, const PoView& w, int entries, double tot) {
  p.lo.utt_tot[2 * (int64_t)w.b] = w.T; p.lo.utt_tot[2 * (int64_t)w.b + 1] = entries;
  p.lo.status[w.u] = KHG_LAT_SUCCEEDED; p.tot[w.u] = tot;
}

// ---- forward, total, backward, arc posteriors, and the per-frame merge's counts and ranks ----
__global__ __launch_bounds__(PO_NT) void k2_lattice_post_fb(PoArgs p) {
#pragma clang fp contract(off)
  extern __shared__ double po_lds[];
  __shared__ double sh_tot;
  const double NINF = -__builtin_huge_val();
  const PoView w = po_open<3>(p, po_lds);
  const LoView& v = w.v;
  if (w.N == 0 || v.start < 0) { po_fail(p, w, KHG_LAT_NO_PATH); return; }
  if (!po_admissible(w)) { po_fail(p, w, KHG_LAT_EPS_LOOP); return; }
  po_frames(w);
  __syncthreads();
  bool settled;
  const double tot = po_alpha_total_beta(w, &sh_tot, &settled);
  if (!settled) { po_fail(p, w, KHG_LAT_EPS_LOOP); return; }
  if (tot == NINF) { po_fail(p, w, KHG_LAT_NO_PATH); return; }
  // arc posteriors; an arc is live when both of its ends are reached
  for (int a = (int)threadIdx.x; a < w.A; a += PO_NT) {
    const double al = w.alpha[w.asrc[a]], be = w.beta[v.next[a]];
    const bool live = al != NINF && be != NINF;
    p.arc_post[w.a0 + a] = live ? exp(((al + po_w(v, w.gs, w.as, a)) + be) - tot) : 0.0;
    w.flag[a] = live && v.il[a] != 0 && v.frame[w.asrc[a]] < w.T ? 1 : 0;
  }
  __syncthreads();
  const int entries = po_merge(w);
  if (threadIdx.x == 0) po_done(p, w, entries, tot);
}

// ---- fill: entry_begin per frame, and for every id of a frame its entry: the id, and its live arcs' posteriors summed in arc order ----
__global__ __launch_bounds__(PO_NT) void k2_lattice_post_fill(PoArgs p) {
#pragma clang fp contract(off)
  const int b = (int)blockIdx.x, u = p.lo.u0 + b;
  const int64_t n = p.lo.n;
  if (b == 0 && blockIdx.y == 0 && threadIdx.x == 0) p.entry_begin[p.lo.utt_off[n]] = p.lo.utt_off[2 * n + 1];
  const int64_t fo = p.lo.utt_off[b], eo = p.lo.utt_off[n + 1 + b];
  const int T = (int)(p.lo.utt_off[b + 1] - fo);
  if (T == 0) return;
  const LoView v = lo_view(p.lo, u, nullptr);
  const int64_t a0 = p.lo.arc_off[u] - p.lo.a_base, f0 = p.lo.ali_off[u] - p.f_base;
  const int32_t* fs = p.fstate + f0 + 2 * (int64_t)b;
  const int32_t* fc = p.fcnt + f0;
  const int32_t* flag = p.flag + a0;
  const int32_t* asrc = p.arc_src + a0;
  const int first = (int)blockIdx.y * PO_NT + (int)threadIdx.x, step = (int)gridDim.y * PO_NT;
  for (int t = first; t < T; t += step) p.entry_begin[fo + t] = eo + fc[t];
  for (int a = first; a < v.A; a += step) {
    const int fl = flag[a];
    if (fl < 2) continue;
    const int id = v.il[a], f = v.frame[asrc[a]], r0 = v.abeg[fs[f]], hs = fs[f + 1], r1 = hs < v.N ? v.abeg[hs] : v.A;
    double sum = 0.0;
    for (int k = r0; k < r1; ++k) if (flag[k] && v.il[k] == id) sum += p.arc_post[a0 + k];
    const int64_t pos = eo + fc[f] + (fl - 2);
    p.tid[pos] = id; p.weight[pos] = sum;
  }
}
