// K2O: operations on device-resident raw lattices (khg_lattices): the best path under K (graph_scale, acoustic_scale) pairs at once
// (khg_lattices_best_path: lattice-scale | lattice-best-path, the language-model-weight sweep) and beam pruning under one pair
// (khg_lattices_prune: lattice-prune).  The rule is DESIGN.md section 7e: Lattice::ShortestPath's tie rule (khg_host_fst.cpp) with
// w1 = fl(gs * graph_cost), w2 = fl(as * acoustic_cost) in place of the raw costs, everything in float under fp contract(off).
//
// The shapes that exist (DESIGN.md 7d: 317 states, 634 arcs over 300 frames per utterance, one or two states per frame) make the
// frame recursion a dependent chain with no width, so the parallel axes are utterances and scale pairs: one workgroup (one wave)
// per utterance stages the utterance's lattice into LDS once, when it fits, and every lane walks it for one scale pair -- the K
// pairs of a sweep read the lattice from HBM once and run in lockstep (same arcs, same branches but for ties).  A lattice that does
// not fit (or KHG_OPT_LAT_OPS_LDS = 1) is read from the HBM arrays through the same code.  A lane walks the arcs in global arc order
// and replaces a value only by a strictly better one, which is the (source state, arc) in-link order of the rule without an in-arc
// index; a Jacobi round reads the values of the round before (n1 / n2).  No atomics: nothing depends on timing.  The per-(state, pair)
// values live in HBM scratch laid out [state][pair], so the lanes' accesses coalesce.
// Pruning: one lane per utterance runs forward, best path and backward; then the wave marks states and arcs, ranks them by ballot /
// shuffle prefix (count), one wave scans the utterances, and -- after the one synchronisation that sizes the output -- the fill writes
// exactly-sized arrays (as K2R does).

#define LO_NT 64

struct LoArgs {
  LatArraysIn in;                        // the chunk's lattice arrays (LatChunk); below, the utterances' ranges in them
  const int32_t* start;                  // [U]
  const int64_t *state_off, *arc_off;    // [U + 1] over the handle
  int64_t s_base, a_base;                // state_off[u0], arc_off[u0]
  int32_t u0, n, U;
  int32_t lds_bytes;                     // dynamic LDS of the launch (0: never stage)
  // scratch, [chunk states * K] each: element (s, k) of utterance u at ((state_off[u] - s_base) + s) * K + k
  float *d1, *d2, *n1, *n2, *e1, *e2;
  int32_t *bp, *pn;
  // best path
  int32_t K;
  const float *gs, *as;                  // [K]
  int32_t* ali;                          // [K][ali_total]
  const int64_t* ali_off;                // [U + 1]
  int64_t ali_total;
  int32_t* words;                        // [chunk states * K]: pair k of utterance u at (state_off[u] - s_base) * K + k * N_u
  int32_t* nwords;                       // [K * U]
  float* weight;                         // [K * U][2]
  int32_t* status;                       // [K * U]
  // prune
  float gs1, as1, beam;
  int32_t *newid, *nab;                  // [chunk states]
  float* limit;                          // [n]
  int64_t *utt_tot, *utt_off;            // [2 * n], [2 * (n + 1)]
  LatArrays out;                         // the pruned chunk's arrays
  int32_t* o_start;                      // [U]
};

// one utterance's lattice: in LDS (staged) or in the HBM arrays
struct LoView {
  int N, A, start;
  const int32_t *frame, *abeg, *il, *next;
  const float *fin, *gc, *ac;
};

__device__ __forceinline__ int lo_aend(const LoView& v, int s) { return s + 1 < v.N ? v.abeg[s + 1] : v.A; }

// all threads of the workgroup; ends with a barrier when it staged
__device__ __forceinline__ LoView lo_view(const LoArgs& p, int u, int32_t* lds) {
  LoView v;
  const int64_t s0 = p.state_off[u] - p.s_base, a0 = p.arc_off[u] - p.a_base;
  v.N = (int)(p.state_off[u + 1] - p.state_off[u]);
  v.A = (int)(p.arc_off[u + 1] - p.arc_off[u]);
  v.start = v.N ? p.start[u] : -1;
  v.frame = p.in.frame + s0; v.abeg = p.in.arc_begin + s0; v.fin = p.in.fin + s0;
  v.il = p.in.ilabel + a0; v.next = p.in.next + a0; v.gc = p.in.g + a0; v.ac = p.in.ac + a0;
  const int64_t need = 4 * (3 * (int64_t)v.N + 4 * (int64_t)v.A);
  if (lds == nullptr || need > (int64_t)p.lds_bytes) return v;          // workgroup-uniform
  int32_t* q = lds;
  int32_t* l_frame = q; q += v.N;
  int32_t* l_abeg = q; q += v.N;
  float* l_fin = reinterpret_cast<float*>(q); q += v.N;
  int32_t* l_il = q; q += v.A;
  int32_t* l_next = q; q += v.A;
  float* l_gc = reinterpret_cast<float*>(q); q += v.A;
  float* l_ac = reinterpret_cast<float*>(q);
  for (int s = (int)threadIdx.x; s < v.N; s += (int)blockDim.x) { l_frame[s] = v.frame[s]; l_abeg[s] = v.abeg[s]; l_fin[s] = v.fin[s]; }
  for (int a = (int)threadIdx.x; a < v.A; a += (int)blockDim.x) { l_il[a] = v.il[a]; l_next[a] = v.next[a]; l_gc[a] = v.gc[a]; l_ac[a] = v.ac[a]; }
  __syncthreads();
  v.frame = l_frame; v.abeg = l_abeg; v.fin = l_fin; v.il = l_il; v.next = l_next; v.gc = l_gc; v.ac = l_ac;
  return v;
}

// one lane's scale pair and its [state] columns (stride K)
struct LoLane {
  float gs, as;
  int64_t K;
  float *d1, *d2, *n1, *n2;
  int32_t* bp;
};

__device__ __forceinline__ bool lo_less(float a1, float a2, float b1, float b2) {
#pragma clang fp contract(off)
  const float fa = a1 + a2, fb = b1 + b2;
  if (fa < fb) return true;
  if (fa > fb) return false;
  return a1 < b1;
}

// the state whose arc range holds arc a
__device__ __forceinline__ int lo_src(const LoView& v, int a) {
  int l = 0, h = v.N;
  while (h - l > 1) {
    const int mid = (l + h) >> 1;
    if (v.abeg[mid] <= a) l = mid; else h = mid;
  }
  return l;
}

// forward pairs (d1, d2) and back-pointers; -> 0, or KHG_LAT_EPS_LOOP.  *last_lo: the first state of the last frame.
__device__ __forceinline__ int lo_forward(const LoView& v, const LoLane& L, int* last_lo) {
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
    if (lo > 0)              // emitting links out of the frame before (its states are [plo, lo)), in arc order
      for (int m = plo; m < lo; ++m) {
        const float dm1 = L.d1[m * K];
        if (dm1 == INF) continue;
        const float dm2 = L.d2[m * K];
        const int ae = lo_aend(v, m);
        for (int a = v.abeg[m]; a < ae; ++a) {
          if (v.il[a] == 0) continue;
          const int n = v.next[a];
          const float w1 = L.gs * v.gc[a], w2 = L.as * v.ac[a];
          const float c1 = dm1 + w1, c2 = dm2 + w2;
          const float b1 = L.d1[n * K];
          if (b1 == INF || lo_less(c1, c2, b1, L.d2[n * K])) { L.d1[n * K] = c1; L.d2[n * K] = c2; L.bp[n * K] = a; }
        }
      }
    for (int round = 0;; ++round) {       // epsilon links inside the frame: Jacobi rounds
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
          const float w1 = L.gs * v.gc[a];
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

// the final state (the lowest among exact ties) and its pair with the final weight; -1: none reached
__device__ __forceinline__ int lo_final(const LoView& v, const LoLane& L, int last_lo, float* f1o, float* f2o) {
#pragma clang fp contract(off)
  const float INF = __builtin_huge_valf();
  int fin = -1;
  float f1 = INF, f2 = INF;
  for (int n = last_lo; n < v.N; ++n) {
    const float d = L.d1[n * L.K], fc = v.fin[n];
    if (d == INF || fc == INF) continue;
    const float fw = L.gs * fc;
    const float w1 = d + fw, w2 = L.d2[n * L.K] + 0.0f;
    if (fin < 0 || lo_less(w1, w2, f1, f2)) { f1 = w1; f2 = w2; fin = n; }
  }
  *f1o = f1; *f2o = f2;
  return fin;
}

// the back-pointer chain from fin to the start, turned round: pn[s * K] = the arc the path leaves s by.  -> arcs on it, -1: broken
__device__ __forceinline__ int lo_chain(const LoView& v, const LoLane& L, int32_t* pn, int fin) {
  int n = fin, steps = 0;
  while (!(n == v.start && L.bp[n * L.K] < 0)) {
    const int a = L.bp[n * L.K];
    if (a < 0 || steps > v.A) return -1;
    ++steps;
    n = lo_src(v, a);
    pn[n * L.K] = a;
  }
  return steps;
}

// no path for (pair, utterance) entry o
__device__ __forceinline__ void lo_fail(const LoArgs& p, int64_t o, int st) {
  const float INF = __builtin_huge_valf();
  p.status[o] = st; p.nwords[o] = 0; p.weight[2 * o] = INF; p.weight[2 * o + 1] = INF;
}

__global__ __launch_bounds__(LO_NT) void k2_lattice_best_path(LoArgs p) {
#pragma clang fp contract(off)
  extern __shared__ int32_t lo_lds[];
  const int u = p.u0 + (int)blockIdx.x;
  const LoView v = lo_view(p, u, lo_lds);
  const int k = (int)blockIdx.y * LO_NT + (int)threadIdx.x;
  if (k >= p.K) return;
  const int64_t o = (int64_t)k * p.U + u;
  if (v.N == 0 || v.start < 0) { lo_fail(p, o, KHG_LAT_NO_PATH); return; }
  const int64_t base = (p.state_off[u] - p.s_base) * p.K;
  LoLane L;
  L.gs = p.gs[k]; L.as = p.as[k]; L.K = p.K;
  L.d1 = p.d1 + base + k; L.d2 = p.d2 + base + k; L.n1 = p.n1 + base + k; L.n2 = p.n2 + base + k; L.bp = p.bp + base + k;
  int last_lo = 0;
  if (lo_forward(v, L, &last_lo)) { lo_fail(p, o, KHG_LAT_EPS_LOOP); return; }
  float f1, f2;
  const int fin = lo_final(v, L, last_lo, &f1, &f2);
  if (fin < 0) { lo_fail(p, o, KHG_LAT_NO_PATH); return; }
  int32_t* pn = reinterpret_cast<int32_t*>(L.n1);        // (the Jacobi rows are free now)
  const int steps = lo_chain(v, L, pn, fin);
  if (steps < 0) { lo_fail(p, o, KHG_LAT_NO_PATH); return; }
  // left to right from One(): the two sums, the transition-ids by frame, the words
  int32_t* ali = p.ali + (int64_t)k * p.ali_total + p.ali_off[u];
  const int T = (int)(p.ali_off[u + 1] - p.ali_off[u]);
  int32_t* words = p.words + base + (int64_t)k * v.N;
  float v1 = 0.0f, v2 = 0.0f;
  int n = v.start, nw = 0;
  const int32_t* ol = p.in.olabel + (p.arc_off[u] - p.a_base);
  for (int i = 0; i < steps; ++i) {
    const int a = pn[n * L.K];
    const int il = v.il[a];
    const float w1 = L.gs * v.gc[a];
    float w2 = 0.0f;
    if (il != 0) {
      w2 = L.as * v.ac[a];
      const int f = v.frame[n];
      if (f >= 0 && f < T) ali[f] = il;
    }
    v1 = v1 + w1; v2 = v2 + w2;
    const int w = ol[a];
    if (w != 0) { if (nw < v.N) words[nw] = w; ++nw; }
    n = v.next[a];
  }
  if (nw > v.N) { lo_fail(p, o, KHG_LAT_WORDS); return; }
  const float fw = L.gs * v.fin[fin];
  v1 = v1 + fw; v2 = v2 + 0.0f;
  p.weight[2 * o] = v1; p.weight[2 * o + 1] = v2;
  p.nwords[o] = nw;
  p.status[o] = KHG_LAT_SUCCEEDED;
}

// exclusive prefix of cnt[0 .. n) -> off[0 .. n] (int64), one wave
__global__ __launch_bounds__(64) void k2_lattice_ops_scan(const int32_t* cnt, int64_t* off, int64_t n) {
  const int lane = (int)threadIdx.x;
  long long tot = 0;
  for (int64_t bb = 0; bb < n; bb += 64) {
    const int64_t b = bb + lane;
    const long long c = b < n ? cnt[b] : 0;
    long long incl = c;
    for (int o = 1; o < 64; o <<= 1) { const long long t = __shfl_up(incl, o); if (lane >= o) incl += t; }
    if (b < n) off[b] = tot + incl - c;
    tot += __shfl(incl, 63);
  }
  if (lane == 0) off[n] = tot;
}

// the words of every (pair, utterance), one after the other
__global__ __launch_bounds__(LO_NT) void k2_lattice_ops_pack_words(LoArgs p, const int64_t* woff, int32_t* packed) {
  const int u = p.u0 + (int)blockIdx.x;
  const int N = (int)(p.state_off[u + 1] - p.state_off[u]);
  const int64_t base = (p.state_off[u] - p.s_base) * p.K;
  for (int k = (int)blockIdx.y; k < p.K; k += (int)gridDim.y) {
    const int64_t o = (int64_t)k * p.U + u;
    const int nw = p.nwords[o];
    for (int i = (int)threadIdx.x; i < nw; i += (int)blockDim.x) packed[woff[o] + i] = p.words[base + (int64_t)k * N + i];
  }
}

// the frame of every utterance's last state (0 for an empty lattice)
__global__ __launch_bounds__(LO_NT) void k2_lattice_ops_last_frame(LoArgs p, int32_t* out) {
  const int b = (int)blockIdx.x * LO_NT + (int)threadIdx.x;
  if (b >= p.n) return;
  const int u = p.u0 + b;
  const int64_t s1 = p.state_off[u + 1], s0 = p.state_off[u];
  out[u] = s1 > s0 ? p.in.frame[s1 - 1 - p.s_base] : 0;
}

// is arc a of the kept state s kept?  (newid: >= 0 for a kept state)
__device__ __forceinline__ bool lo_keep_arc(const LoArgs& p, const LoView& v, int64_t s0, int s, int a, float limit) {
#pragma clang fp contract(off)
  const int k = v.next[a];
  if (p.newid[s0 + k] < 0) return false;
  if (p.pn[s0 + s] == a) return true;
  const float w1 = p.gs1 * v.gc[a];
  const float w2 = v.il[a] != 0 ? p.as1 * v.ac[a] : 0.0f;
  const float p1 = p.d1[s0 + s] + w1, p2 = p.d2[s0 + s] + w2;
  const float t1 = p1 + p.e1[s0 + k], t2 = p2 + p.e2[s0 + k];
  const float tot = t1 + t2;
  return tot <= limit;
}

// ---- prune, mark and count: forward / best path / backward on one lane, then the wave marks and ranks states and arcs ----
__global__ __launch_bounds__(LO_NT) void k2_lattice_prune_mark(LoArgs p) {
#pragma clang fp contract(off)
  extern __shared__ int32_t lo_lds[];
  __shared__ int sh_status, sh_fin;
  __shared__ float sh_limit;
  const int b = (int)blockIdx.x, u = p.u0 + b, lane = (int)threadIdx.x;
  const LoView v = lo_view(p, u, lo_lds);
  const float INF = __builtin_huge_valf();
  const int64_t s0 = p.state_off[u] - p.s_base;
  if (lane == 0) {
    int st = KHG_LAT_NO_PATH, fin = -1;
    float limit = INF;
    if (v.N > 0 && v.start >= 0) {
      LoLane L;
      L.gs = p.gs1; L.as = p.as1; L.K = 1;
      L.d1 = p.d1 + s0; L.d2 = p.d2 + s0; L.n1 = p.n1 + s0; L.n2 = p.n2 + s0; L.bp = p.bp + s0;
      int32_t* pn = p.pn + s0;
      for (int s = 0; s < v.N; ++s) pn[s] = -1;
      int last_lo = 0;
      st = lo_forward(v, L, &last_lo);
      if (!st) {
        float f1, f2;
        fin = lo_final(v, L, last_lo, &f1, &f2);
        st = fin >= 0 && lo_chain(v, L, pn, fin) >= 0 ? KHG_LAT_SUCCEEDED : KHG_LAT_NO_PATH;
        const float best = f1 + f2;
        limit = best + p.beam;
      }
      if (st == KHG_LAT_SUCCEEDED) {
        // backward pairs: frames T .. 0; a state takes its final weight, its emitting out-arcs, then epsilon out-arcs in Jacobi rounds
        float *e1 = p.e1 + s0, *e2 = p.e2 + s0;
        for (int s = 0; s < v.N; ++s) { e1[s] = INF; e2[s] = INF; }
        int hi = v.N;
        while (hi > 0 && st == KHG_LAT_SUCCEEDED) {
          const int f = v.frame[hi - 1];
          int lo = hi - 1;
          while (lo > 0 && v.frame[lo - 1] == f) --lo;
          for (int n = lo; n < hi; ++n) {
            float b1 = INF, b2 = INF;
            if (n >= last_lo && v.fin[n] != INF) { b1 = p.gs1 * v.fin[n]; b2 = 0.0f; }
            const int ae = lo_aend(v, n);
            for (int a = v.abeg[n]; a < ae; ++a) {
              const int k = v.next[a];
              if (v.il[a] == 0 || e1[k] == INF) continue;
              const float w1 = p.gs1 * v.gc[a], w2 = p.as1 * v.ac[a];
              const float c1 = w1 + e1[k], c2 = w2 + e2[k];
              if (b1 == INF || lo_less(c1, c2, b1, b2)) { b1 = c1; b2 = c2; }
            }
            e1[n] = b1; e2[n] = b2;
          }
          for (int round = 0;; ++round) {
            bool changed = false;
            for (int n = lo; n < hi; ++n) {
              float b1 = e1[n], b2 = e2[n];
              const int ae = lo_aend(v, n);
              for (int a = v.abeg[n]; a < ae; ++a) {
                const int k = v.next[a];
                if (v.il[a] != 0 || e1[k] == INF) continue;
                const float w1 = p.gs1 * v.gc[a];
                const float c1 = w1 + e1[k], c2 = 0.0f + e2[k];
                if (b1 == INF || lo_less(c1, c2, b1, b2)) { b1 = c1; b2 = c2; changed = true; }
              }
              L.n1[n] = b1; L.n2[n] = b2;
            }
            if (!changed) break;
            for (int n = lo; n < hi; ++n) { e1[n] = L.n1[n]; e2[n] = L.n2[n]; }
            if (round > hi - lo) { st = KHG_LAT_EPS_LOOP; break; }
          }
          hi = lo;
        }
      }
    }
    sh_status = st; sh_fin = fin; sh_limit = limit;
    p.status[u] = st;
    p.limit[b] = limit;
  }
  __syncthreads();
  const bool ok = sh_status == KHG_LAT_SUCCEEDED;
  const float limit = sh_limit;
  const int fin = sh_fin;
  // states: on the best path, or reached from both sides and within the beam
  for (int s = lane; s < v.N; s += LO_NT) {
    bool keep = false;
    if (ok) {
      keep = p.pn[s0 + s] >= 0 || s == fin;
      const float a1 = p.d1[s0 + s], b1 = p.e1[s0 + s];
      if (!keep && a1 != INF && b1 != INF) {
        const float t1 = a1 + b1, t2 = p.d2[s0 + s] + p.e2[s0 + s];
        const float tot = t1 + t2;
        keep = tot <= limit;
      }
    }
    p.newid[s0 + s] = keep ? 0 : -1;
  }
  __syncthreads();
  for (int s = lane; s < v.N; s += LO_NT) {
    int c = 0;
    if (p.newid[s0 + s] >= 0) {
      const int ae = lo_aend(v, s);
      for (int a = v.abeg[s]; a < ae; ++a) c += lo_keep_arc(p, v, s0, s, a, limit) ? 1 : 0;
    }
    p.nab[s0 + s] = c;
  }
  __syncthreads();
  // ranks: ballot and popcount for the states, a shuffle scan for the arcs, carried from tile to tile
  const unsigned long long below = (1ull << lane) - 1ull;
  int sbase = 0, abase = 0;
  for (int sb = 0; sb < v.N; sb += LO_NT) {
    const int s = sb + lane;
    const bool keep = s < v.N && p.newid[s0 + s] >= 0;
    const int c = s < v.N ? p.nab[s0 + s] : 0;
    const unsigned long long bal = __ballot(keep);
    int incl = c;
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o); if (lane >= o) incl += t; }
    if (s < v.N) {
      p.newid[s0 + s] = keep ? sbase + __popcll(bal & below) : -1;
      p.nab[s0 + s] = abase + incl - c;
    }
    sbase += __popcll(bal);
    abase += __shfl(incl, 63);
  }
  if (lane == 0) { p.utt_tot[2 * (int64_t)b] = sbase; p.utt_tot[2 * (int64_t)b + 1] = abase; }
}

// ---- prune, fill: the kept states and arcs at the positions the prefix sums give; costs as stored ----
__global__ __launch_bounds__(LO_NT) void k2_lattice_prune_fill(LoArgs p) {
  const int b = (int)blockIdx.x, u = p.u0 + b;
  const LoView v = lo_view(p, u, nullptr);
  const int64_t s0 = p.state_off[u] - p.s_base, a0 = p.arc_off[u] - p.a_base;
  const int64_t so = p.utt_off[b], ao = p.utt_off[(int64_t)p.n + 1 + b];
  const bool any = p.utt_off[b + 1] > so;
  if (blockIdx.y == 0 && threadIdx.x == 0) p.o_start[u] = any ? p.newid[s0 + v.start] : -1;
  if (!any) return;
  const float limit = p.limit[b];
  for (int s = (int)blockIdx.y * LO_NT + (int)threadIdx.x; s < v.N; s += (int)gridDim.y * LO_NT) {
    const int r = p.newid[s0 + s];
    if (r < 0) continue;
    const int64_t sid = so + r;
    p.out.frame[sid] = p.in.frame[s0 + s]; p.out.gstate[sid] = p.in.gstate[s0 + s]; p.out.tot[sid] = p.in.tot[s0 + s];
    p.out.extra[sid] = p.in.extra[s0 + s]; p.out.fin[sid] = p.in.fin[s0 + s];
    p.out.arc_begin[sid] = p.nab[s0 + s];
    int64_t pos = ao + p.nab[s0 + s];
    const int ae = lo_aend(v, s);
    for (int a = v.abeg[s]; a < ae; ++a) {
      if (!lo_keep_arc(p, v, s0, s, a, limit)) continue;
      p.out.ilabel[pos] = p.in.ilabel[a0 + a]; p.out.olabel[pos] = p.in.olabel[a0 + a];
      p.out.g[pos] = p.in.g[a0 + a]; p.out.ac[pos] = p.in.ac[a0 + a];
      p.out.next[pos] = p.newid[s0 + v.next[a]];
      ++pos;
    }
  }
}
