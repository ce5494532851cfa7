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

__device__ __forceinline__ void po_fail(const PoArgs& p, int u, int b, int64_t a0, int A, int st) {
  if (threadIdx.x == 0) {
    p.lo.status[u] = st; p.tot[u] = -__builtin_huge_val();
    p.lo.utt_tot[2 * (int64_t)b] = 0; p.lo.utt_tot[2 * (int64_t)b + 1] = 0;
  }
  for (int a = (int)threadIdx.x; a < A; a += PO_NT) p.arc_post[a0 + a] = 0.0;
}

// ---- forward, total, backward, arc posteriors, and the per-frame merge's counts and ranks ----
__global__ __launch_bounds__(PO_NT) void k2_lattice_post_fb(PoArgs p) {
#pragma clang fp contract(off)
  extern __shared__ double po_lds[];
  __shared__ double sh_tot;
  const double NINF = -__builtin_huge_val();
  const float FINF = __builtin_huge_valf();
  const int b = (int)blockIdx.x, u = p.lo.u0 + b, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t s0 = p.lo.state_off[u] - p.lo.s_base, a0 = p.lo.arc_off[u] - p.lo.a_base;
  const int N = (int)(p.lo.state_off[u + 1] - p.lo.state_off[u]), A = (int)(p.lo.arc_off[u + 1] - p.lo.arc_off[u]);
  const int64_t need = 24 * (int64_t)N + 4 * (3 * (int64_t)N + 4 * (int64_t)A);
  const bool in_lds = need <= (int64_t)p.lo.lds_bytes;                                   // workgroup-uniform
  const LoView v = lo_view(p.lo, u, in_lds ? reinterpret_cast<int32_t*>(po_lds + 3 * (size_t)N) : nullptr);
  if (N == 0 || v.start < 0) { po_fail(p, u, b, a0, A, KHG_LAT_NO_PATH); return; }
  double* alpha = in_lds ? po_lds : p.alpha + s0;
  double* beta = in_lds ? po_lds + N : p.beta + s0;
  double* row = in_lds ? po_lds + 2 * (size_t)N : p.row + s0;
  const int32_t* asrc = p.arc_src + a0;
  const int32_t* ib = p.in_begin + s0 + b;
  const int32_t* ia = p.in_arc + a0;
  const double gs = p.gs, as = p.as;
  // admissible: every epsilon arc goes to a higher state
  {
    int bad = 0;
    for (int a = tid; a < A; a += PO_NT) if (v.il[a] == 0 && v.next[a] <= asrc[a]) bad = 1;
    if (__syncthreads_or(bad)) { po_fail(p, u, b, a0, A, KHG_LAT_EPS_LOOP); return; }
  }
  const int64_t f0 = p.lo.ali_off[u] - p.f_base;
  const int T = (int)(p.lo.ali_off[u + 1] - p.lo.ali_off[u]);        // the last state's frame
  int32_t* fs = p.fstate + f0 + 2 * (int64_t)b;                       // [T + 2]: frame f holds the states fs[f] .. fs[f + 1]
  int32_t* fc = p.fcnt + f0;                                          // [T]
  for (int s = tid; s < N; s += PO_NT) {
    const int f = v.frame[s], pf = s ? v.frame[s - 1] : -1;
    for (int g = pf + 1; g <= f; ++g) fs[g] = s;
    alpha[s] = NINF; beta[s] = NINF;
  }
  for (int t = tid; t < T; t += PO_NT) fc[t] = 0;
  if (tid == 0) fs[T + 1] = N;
  __syncthreads();

  int broken = 0;
  for (int f = 0; f <= T && !broken; ++f) {                           // forward
    const int lo = fs[f], hi = fs[f + 1];
    int has_eps = 0;
    for (int round = 0;; ++round) {
      int changed = 0, eps = 0;
      for (int s = lo + tid; s < hi; s += PO_NT) {                    // lanes over states
        const int i0 = ib[s], deg = ib[s + 1] - i0;
        if (deg > PO_HUB) continue;
        if (round == 0) for (int i = 0; i < deg; ++i) eps |= v.il[ia[i0 + i]] == 0;
        const double val = po_lse_lane(s == v.start ? 0.0 : NINF, deg, [&](int i) { const int a = ia[i0 + i]; return alpha[asrc[a]] + po_w(v, gs, as, a); });
        row[s] = val;
        changed |= po_differs(val, alpha[s]);
      }
      for (int s = lo + wave; s < hi; s += PO_NT / 64) {              // hub states: the wave over a state's in-arcs
        const int i0 = ib[s], deg = ib[s + 1] - i0;
        if (deg <= PO_HUB) continue;
        if (round == 0) for (int i = lane; i < deg; i += 64) eps |= v.il[ia[i0 + i]] == 0;
        const double val = po_lse_wave(s == v.start ? 0.0 : NINF, deg, [&](int i) { const int a = ia[i0 + i]; return alpha[asrc[a]] + po_w(v, gs, as, a); }, lane);
        if (lane == 0) { row[s] = val; changed |= po_differs(val, alpha[s]); }
      }
      if (round == 0) has_eps = __syncthreads_or(eps);               // (the reduction gives 0 or 1: one call per flag)
      if (!__syncthreads_or(changed)) break;                          // no value's bits changed
      for (int s = lo + tid; s < hi; s += PO_NT) alpha[s] = row[s];
      __syncthreads();
      if (!has_eps) break;
      if (round > hi - lo) { broken = 1; break; }                     // (not reached on an admissible lattice)
    }
  }
  if (broken) { po_fail(p, u, b, a0, A, KHG_LAT_EPS_LOOP); return; }
  if (wave == 0) {                                                    // the total over the last frame's final states
    const int lo = fs[T];
    const double t = po_lse_wave(NINF, N - lo, [&](int i) { const float c = v.fin[lo + i]; return c == FINF ? NINF : alpha[lo + i] + -(gs * (double)c); }, lane);
    if (lane == 0) sh_tot = t;
  }
  __syncthreads();
  const double tot = sh_tot;
  if (tot == NINF) { po_fail(p, u, b, a0, A, KHG_LAT_NO_PATH); return; }

  for (int f = T; f >= 0; --f) {                                      // backward: the same over out-arcs
    const int lo = fs[f], hi = fs[f + 1];
    int has_eps = 0;
    for (int round = 0;; ++round) {
      int changed = 0, eps = 0;
      for (int s = lo + tid; s < hi; s += PO_NT) {
        const int e0 = v.abeg[s], deg = lo_aend(v, s) - e0;
        if (deg > PO_HUB) continue;
        if (round == 0) for (int i = 0; i < deg; ++i) eps |= v.il[e0 + i] == 0;
        const float c = v.fin[s];
        const double init = f == T && c != FINF ? -(gs * (double)c) : NINF;
        const double val = po_lse_lane(init, deg, [&](int i) { const int a = e0 + i; return po_w(v, gs, as, a) + beta[v.next[a]]; });
        row[s] = val;
        changed |= po_differs(val, beta[s]);
      }
      for (int s = lo + wave; s < hi; s += PO_NT / 64) {
        const int e0 = v.abeg[s], deg = lo_aend(v, s) - e0;
        if (deg <= PO_HUB) continue;
        if (round == 0) for (int i = lane; i < deg; i += 64) eps |= v.il[e0 + i] == 0;
        const float c = v.fin[s];
        const double init = f == T && c != FINF ? -(gs * (double)c) : NINF;
        const double val = po_lse_wave(init, deg, [&](int i) { const int a = e0 + i; return po_w(v, gs, as, a) + beta[v.next[a]]; }, lane);
        if (lane == 0) { row[s] = val; changed |= po_differs(val, beta[s]); }
      }
      if (round == 0) has_eps = __syncthreads_or(eps);
      if (!__syncthreads_or(changed)) break;
      for (int s = lo + tid; s < hi; s += PO_NT) beta[s] = row[s];
      __syncthreads();
      if (!has_eps || round > hi - lo) break;
    }
  }

  // arc posteriors; an arc is live when both of its ends are reached
  for (int a = tid; a < A; a += PO_NT) {
    const double al = alpha[asrc[a]], be = beta[v.next[a]];
    const bool live = al != NINF && be != NINF;
    p.arc_post[a0 + a] = live ? exp(((al + po_w(v, gs, as, a)) + be) - tot) : 0.0;
    p.flag[a0 + a] = live && v.il[a] != 0 && v.frame[asrc[a]] < T ? 1 : 0;
  }
  __syncthreads();
  // the merge: the emitting arcs that leave frame f are the arc range of its states; the first live arc of every id ...
  int32_t* flag = p.flag + a0;
  int32_t* rank = p.rank + a0;
  for (int a = tid; a < A; a += PO_NT) {
    int first = -1;
    if (flag[a]) {
      const int id = v.il[a], r0 = v.abeg[fs[v.frame[asrc[a]]]];
      first = 0;
      for (int k = r0; k < a; ++k) if (flag[k] && v.il[k] == id) { first = -1; break; }
    }
    rank[a] = first;
  }
  __syncthreads();
  // ... is ranked among the frame's ids, and the one with the highest id leaves the frame's count
  for (int a = tid; a < A; a += PO_NT) {
    if (rank[a] != 0) continue;
    const int id = v.il[a], f = v.frame[asrc[a]], r0 = v.abeg[fs[f]], hs = fs[f + 1], r1 = hs < N ? v.abeg[hs] : A;
    int r = 0, cnt = 0;
    for (int k = r0; k < r1; ++k) if (rank[k] == 0) { ++cnt; r += v.il[k] < id; }
    flag[a] = 2 + r;
    if (r == cnt - 1 && f < T) fc[f] = cnt;
  }
  __syncthreads();
  if (wave == 0) {                                                    // exclusive prefix of the frames' counts
    int sum = 0;
    for (int tb = 0; tb < T; tb += 64) {
      const int t = tb + lane;
      const int c = t < T ? fc[t] : 0;
      int incl = c;
      for (int o = 1; o < 64; o <<= 1) { const int x = __shfl_up(incl, o); if (lane >= o) incl += x; }
      if (t < T) fc[t] = sum + incl - c;
      sum += __shfl(incl, 63);
    }
    if (lane == 0) {
      p.lo.utt_tot[2 * (int64_t)b] = T; p.lo.utt_tot[2 * (int64_t)b + 1] = sum;
      p.lo.status[u] = KHG_LAT_SUCCEEDED; p.tot[u] = tot;
    }
  }
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
