// K2D: determinizing device-resident lattices (khg_lattices_determinize: lattice-determinize-pruned).  The rule is DESIGN.md section 7u
// (include/khg_hip.h states it in full): between two khg_lattices_prune calls, every state s of the pruned lattice X is split by the
// determinized states D whose closure holds it, and an element (D, s) keeps its single best in-arc.  All in float under fp contract(off).
//
// Mark -> k2_lattice_scan_pairs -> fill, the shape of khg_lattices_lm_rescore.  A determinized state exists only once the ones before it
// have been expanded, so an utterance is a serial loop over its D, run by ONE wave (one workgroup: __syncthreads() is the only fence
// needed).  Per D the lanes take the word arcs that leave its closure (compacted by ballot, rank-sorted by (word, dest, cost, arc): the
// first of every (word, dest) run is the kept candidate); per word the lanes normalise the arrival, walk the closure state by state
// with the in-arcs of a state across the lanes (LatIndex; the best of a tile by a butterfly whose ties go to the lower arc), compare
// the arrival's K / R with the stored ones element-wise, and either find its D or append one to the utterance's arenas.  Every
// element (D, s) owns one slot per arc of s: the element its copy of the arc leads to, or -1; a slot has exactly one writer.  The new
// number of an element is base[s] + its rank among the elements of s, which are created in ascending D.  No atomics: nothing depends
// on timing.  Every arena write is checked against the arena's size (KHG_LAT_SCRATCH), every loop is bounded by a size.
// The fill runs one lane per new state: it copies the row and the arcs whose slot is set.

#define DT_NT 64
#define DT_PER_E 15       // arrays of [state_factor * chunk states + n] words
#define DT_PER_S 15       // arrays of [chunk states] words
#define DT_PER_A 12       // arrays of [chunk arcs] words

struct DtArgs {
  LoArgs lo;                             // the chunk of X: its lattices, status [U], utt_tot / utt_off, out, o_start
  const int32_t *in_begin, *in_arc, *arc_src;     // LatIndex of X
  const int32_t* status0;                // [U]: 0, or the status the utterance already has (its result is empty)
  float gs, as, delta;
  int32_t factor;
  // per utterance u of the chunk (b = u - u0, s0 / a0 its first state / arc in the chunk, N states, A arcs):
  int32_t* per_e;                        // DT_PER_E arrays of stride e_stride; u's slice starts at factor * s0 + b, factor * N + 1 words
  int32_t* per_s;                        // DT_PER_S arrays of stride s_stride; u's slice starts at s0
  int32_t* per_a;                        // DT_PER_A arrays of stride a_stride; u's slice starts at a0
  int32_t* slot;                         // [factor * chunk arcs]; u's slice starts at factor * a0
  int64_t e_stride, s_stride, a_stride;
  int32_t *det_states, *max_subset, *max_closure;      // [U]
};

// u's arrays
struct DtView {
  int N, A;
  const int32_t *abeg, *next, *ol, *il, *frame, *ib, *in_arc, *arc_src;
  const float *g, *ac, *fin;
  // elements, in the order they were made (D by D, ascending state inside a D)
  int32_t *e_s, *e_slot, *e_within, *e_d;
  float *e_a, *e_b;
  int32_t *k_s, *d_off, *d_koff, *d_hash, *d_fin, *y_elem, *y_abeg;
  float *k_a, *k_b;
  // per state of X
  int32_t *cl_stamp, *cl_idx, *in_stamp, *cnt, *t_s, *t_pred, *tk_s;
  float *cl_a, *cl_b, *in_a, *in_b, *t_a, *t_b, *tk_a, *tk_b;
  // per arc of X: the candidates of one D, unsorted (then: the kept ones) and sorted
  int32_t *u_w, *u_dest, *u_arc, *u_e, *s_w, *s_dest, *s_arc, *s_e;
  float *u_a, *u_b, *s_a, *s_b;
  int32_t* slot;
};

__device__ __forceinline__ DtView dt_view(const DtArgs& p, int b, int u) {
  DtView v;
  const int64_t s0 = p.lo.state_off[u] - p.lo.s_base, a0 = p.lo.arc_off[u] - p.lo.a_base;
  v.N = (int)(p.lo.state_off[u + 1] - p.lo.state_off[u]);
  v.A = (int)(p.lo.arc_off[u + 1] - p.lo.arc_off[u]);
  v.abeg = p.lo.in.arc_begin + s0; v.frame = p.lo.in.frame + s0; v.fin = p.lo.in.fin + s0;
  v.next = p.lo.in.next + a0; v.ol = p.lo.in.olabel + a0; v.il = p.lo.in.ilabel + a0; v.g = p.lo.in.g + a0; v.ac = p.lo.in.ac + a0;
  v.ib = p.in_begin + s0 + b; v.in_arc = p.in_arc + a0; v.arc_src = p.arc_src + a0;
  int32_t* e = p.per_e + (int64_t)p.factor * s0 + b;
  auto ei = [&](int k) { return e + (int64_t)k * p.e_stride; };
  auto ef = [&](int k) { return reinterpret_cast<float*>(e + (int64_t)k * p.e_stride); };
  v.e_s = ei(0); v.e_a = ef(1); v.e_b = ef(2); v.e_slot = ei(3); v.e_within = ei(4); v.e_d = ei(5); v.k_s = ei(6); v.k_a = ef(7); v.k_b = ef(8);
  v.d_off = ei(9); v.d_koff = ei(10); v.d_hash = ei(11); v.d_fin = ei(12); v.y_elem = ei(13); v.y_abeg = ei(14);
  int32_t* s = p.per_s + s0;
  auto si = [&](int k) { return s + (int64_t)k * p.s_stride; };
  auto sf = [&](int k) { return reinterpret_cast<float*>(s + (int64_t)k * p.s_stride); };
  v.cl_stamp = si(0); v.cl_a = sf(1); v.cl_b = sf(2); v.cl_idx = si(3); v.in_stamp = si(4); v.in_a = sf(5); v.in_b = sf(6); v.cnt = si(7);
  v.t_s = si(8); v.t_a = sf(9); v.t_b = sf(10); v.t_pred = si(11); v.tk_s = si(12); v.tk_a = sf(13); v.tk_b = sf(14);
  int32_t* a = p.per_a + a0;
  auto ai = [&](int k) { return a + (int64_t)k * p.a_stride; };
  auto af = [&](int k) { return reinterpret_cast<float*>(a + (int64_t)k * p.a_stride); };
  v.u_w = ai(0); v.u_dest = ai(1); v.u_arc = ai(2); v.u_a = af(3); v.u_b = af(4); v.u_e = ai(5);
  v.s_w = ai(6); v.s_dest = ai(7); v.s_arc = ai(8); v.s_a = af(9); v.s_b = af(10); v.s_e = ai(11);
  v.slot = p.slot + (int64_t)p.factor * a0;
  return v;
}

__device__ __forceinline__ int dt_aend(const DtView& v, int s) { return s + 1 < v.N ? v.abeg[s + 1] : v.A; }

// (a1, b1) strictly better than (a2, b2): khg_lattices_best_path's order
__device__ __forceinline__ bool dt_less(float a1, float b1, float a2, float b2) {
#pragma clang fp contract(off)
  const float f1 = a1 + b1, f2 = a2 + b2;
  if (f1 < f2) return true;
  if (f1 > f2) return false;
  return a1 < a2;
}
// the weight of arc a
__device__ __forceinline__ void dt_weight(const DtArgs& p, const DtView& v, int a, float* wa, float* wb) {
#pragma clang fp contract(off)
  *wa = p.gs * v.g[a];
  *wb = v.il[a] != 0 ? p.as * v.ac[a] : 0.0f;
}
// the best (a, b) among the lanes with `has`, ties to the lower idx (distinct among them); every lane gets it
__device__ __forceinline__ void dt_wave_best(bool* has, float* a, float* b, int* idx) {
  for (int o = 32; o; o >>= 1) {
    const int oh = __shfl_xor((int)*has, o), oi = __shfl_xor(*idx, o);
    const float oa = __shfl_xor(*a, o), ob = __shfl_xor(*b, o);
    const bool take = oh && (!*has || dt_less(oa, ob, *a, *b) || (!dt_less(*a, *b, oa, ob) && oi < *idx));
    if (take) { *has = true; *a = oa; *b = ob; *idx = oi; }
  }
}
// a float as an unsigned that orders as the float does (-0 as +0), so that a rank over it is a permutation whatever the bits
__device__ __forceinline__ uint32_t dt_ord(float x) {
#pragma clang fp contract(off)
  const float y = x + 0.0f;
  const uint32_t bits = __float_as_uint(y);
  return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}
__device__ __forceinline__ int dt_wave_max(int x) {
  for (int o = 32; o; o >>= 1) x = max(x, __shfl_xor(x, o));
  return x;
}
__device__ __forceinline__ uint32_t dt_wave_sum(uint32_t x) {
  for (int o = 32; o; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

// the utterance's running state (wave-uniform)
struct DtRun {
  int stamp, nD, max_k, max_c;
  int64_t used_s, used_a, used_k, cap_s, cap_a;
  int st;
};

// The arrival of the kept candidates u_*[g0 .. g1) (one word; dest ascending): its closure, K / R, its D (found or appended).  -> the
// number of the D, or -1 with r->st set.  Afterwards cl_idx / t_pred hold the arrival's own closure.  All lanes call it.
__device__ int dt_arrive(const DtArgs& p, const DtView& v, DtRun* r, int g0, int g1, int lane, int T) {
#pragma clang fp contract(off)
  const float INF = __builtin_huge_valf();
  // the best initial cost
  bool has = false;
  float ba = 0.0f, bb = 0.0f;
  int bi = 0x7fffffff;
  for (int i = g0 + lane; i < g1; i += DT_NT) {
    const float a = v.u_a[i], b = v.u_b[i];
    if (!has || dt_less(a, b, ba, bb)) { has = true; ba = a; bb = b; bi = i; }
  }
  dt_wave_best(&has, &ba, &bb, &bi);
  if (r->stamp == 0x7ffffffe) { r->st = KHG_LAT_SCRATCH; return -1; }
  const int stamp = ++r->stamp;
  for (int i = g0 + lane; i < g1; i += DT_NT) {
    const int s = v.u_dest[i];
    v.in_stamp[s] = stamp;
    v.in_a[s] = v.u_a[i] - ba; v.in_b[s] = v.u_b[i] - bb;
  }
  const int lo = v.u_dest[g0];
  int hi = v.u_dest[g1 - 1];
  __syncthreads();
  // the closure, state by state
  int tc = 0;
  int64_t arcs = 0;
  for (int s = lo; s <= hi; ++s) {
    bool in = v.in_stamp[s] == stamp;
    float ca = in ? v.in_a[s] : 0.0f, cb = in ? v.in_b[s] : 0.0f;
    int pr = -1;
    const int j1 = v.ib[s + 1];
    for (int jb = v.ib[s]; jb < j1; jb += DT_NT) {
      const int j = jb + lane;
      bool ok = false;
      float ta = 0.0f, tb = 0.0f;
      int a = 0x7fffffff;
      if (j < j1) {
        const int aa = v.in_arc[j];
        if (v.ol[aa] == 0) {
          const int q = v.arc_src[aa];
          if (v.cl_stamp[q] == stamp) {
            float wa, wb;
            dt_weight(p, v, aa, &wa, &wb);
            ta = v.cl_a[q] + wa; tb = v.cl_b[q] + wb; a = aa; ok = true;
          }
        }
      }
      dt_wave_best(&ok, &ta, &tb, &a);
      if (ok && (!in || dt_less(ta, tb, ca, cb))) { in = true; ca = ta; cb = tb; pr = a; }
    }
    if (!in) continue;
    if (lane == 0) {
      v.cl_stamp[s] = stamp; v.cl_a[s] = ca; v.cl_b[s] = cb; v.cl_idx[s] = tc;
      v.t_s[tc] = s; v.t_a[tc] = ca; v.t_b[tc] = cb; v.t_pred[tc] = pr;
    }
    ++tc;
    const int alo = v.abeg[s], ahi = dt_aend(v, s);
    arcs += ahi - alo;
    int m = hi;
    for (int a = alo + lane; a < ahi; a += DT_NT)
      if (v.ol[a] == 0) m = max(m, v.next[a]);
    hi = min(dt_wave_max(m), v.N - 1);
    __syncthreads();
  }
  // K / R: the initial states that no arc inside the closure beats, ascending
  int kc = 0;
  uint32_t hash = 0;
  for (int ib0 = g0; ib0 < g1; ib0 += DT_NT) {
    const int i = ib0 + lane;
    int s = 0;
    bool nd = false;
    if (i < g1) { s = v.u_dest[i]; nd = v.t_pred[v.cl_idx[s]] < 0; }
    const unsigned long long bal = __ballot(nd);
    if (nd) {
      const int k = kc + __popcll(bal & ((1ull << lane) - 1ull));
      v.tk_s[k] = s; v.tk_a[k] = v.cl_a[s]; v.tk_b[k] = v.cl_b[s];
      hash += (uint32_t)s * 2654435761u + 0x9e3779b9u;
    }
    kc += __popcll(bal);
  }
  hash = dt_wave_sum(hash);
  __syncthreads();
  // the lowest-numbered D with the same K and R within delta
  for (int db = 0; db < r->nD; db += DT_NT) {
    const int d = db + lane;
    const bool c = d < r->nD && v.d_koff[d + 1] - v.d_koff[d] == kc && (uint32_t)v.d_hash[d] == hash;
    unsigned long long mask = __ballot(c);
    while (mask) {
      const int dd = db + __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const int ko = v.d_koff[dd];
      bool differ = false;
      for (int i = lane; i < kc; i += DT_NT) {
        const float da = v.tk_a[i] - v.k_a[ko + i], dbv = v.tk_b[i] - v.k_b[ko + i];
        if (v.k_s[ko + i] != v.tk_s[i] || !(fabsf(da) <= p.delta) || !(fabsf(dbv) <= p.delta)) differ = true;
      }
      if (!__ballot(differ)) return dd;
    }
  }
  // a new D: its elements, their slots, its K / R, its final state
  if (r->used_s + tc > r->cap_s || r->used_a + arcs > r->cap_a) { r->st = KHG_LAT_SCRATCH; return -1; }
  const int me = r->nD, e0 = (int)r->used_s, k0 = (int)r->used_k;
  int64_t run = r->used_a;
  bool fh = false;
  float f1 = 0.0f, f2 = 0.0f;
  int fi = 0x7fffffff;
  for (int ib0 = 0; ib0 < tc; ib0 += DT_NT) {
    const int i = ib0 + lane;
    int s = 0, deg = 0;
    if (i < tc) { s = v.t_s[i]; deg = dt_aend(v, s) - v.abeg[s]; }
    long long incl = deg;
    for (int o = 1; o < 64; o <<= 1) { const long long t = __shfl_up(incl, o); if (lane >= o) incl += t; }
    if (i < tc) {
      const int64_t off = run + incl - deg;
      const int e = e0 + i;
      v.e_s[e] = s; v.e_a[e] = v.t_a[i]; v.e_b[e] = v.t_b[i]; v.e_slot[e] = (int32_t)off; v.e_d[e] = me;
      v.e_within[e] = v.cnt[s]; v.cnt[s] += 1;
      for (int k = 0; k < deg; ++k) v.slot[off + k] = -1;
      if (v.fin[s] != INF && v.frame[s] == T) {
        const float fw = p.gs * v.fin[s];
        const float v1 = v.t_a[i] + fw, v2 = v.t_b[i];
        if (!fh || dt_less(v1, v2, f1, f2)) { fh = true; f1 = v1; f2 = v2; fi = i; }
      }
    }
    run += __shfl(incl, 63);
  }
  dt_wave_best(&fh, &f1, &f2, &fi);
  for (int i = lane; i < kc; i += DT_NT) { v.k_s[k0 + i] = v.tk_s[i]; v.k_a[k0 + i] = v.tk_a[i]; v.k_b[k0 + i] = v.tk_b[i]; }
  if (lane == 0) {
    v.d_off[me + 1] = e0 + tc; v.d_koff[me + 1] = k0 + kc; v.d_hash[me] = (int32_t)hash; v.d_fin[me] = fh ? v.t_s[fi] : -1;
  }
  __syncthreads();       // the slots are cleared before the arcs inside the closure take theirs
  for (int i = lane; i < tc; i += DT_NT) {
    const int pr = v.t_pred[i];
    if (pr >= 0) {
      const int q = v.arc_src[pr];
      v.slot[(int64_t)v.e_slot[e0 + v.cl_idx[q]] + (pr - v.abeg[q])] = e0 + i;
    }
  }
  r->used_s += tc; r->used_a = run; r->used_k += kc; r->nD = me + 1;
  r->max_k = max(r->max_k, kc); r->max_c = max(r->max_c, tc);
  __syncthreads();
  return me;
}

// ---- mark: the determinized states of every utterance, the elements' new numbers and arc offsets, the totals, the status ----
__global__ __launch_bounds__(DT_NT) void k2_lattice_det_mark(DtArgs p) {
#pragma clang fp contract(off)
  const int b = (int)blockIdx.x, u = p.lo.u0 + b, lane = (int)threadIdx.x;
  const DtView v = dt_view(p, b, u);
  const int N = v.N, A = v.A;
  DtRun r;
  r.stamp = 0; r.nD = 0; r.max_k = 0; r.max_c = 0; r.used_s = 0; r.used_a = 0; r.used_k = 0;
  r.cap_s = (int64_t)p.factor * N < (int64_t)INT32_MAX ? (int64_t)p.factor * N : (int64_t)INT32_MAX;
  r.cap_a = (int64_t)p.factor * A < (int64_t)INT32_MAX ? (int64_t)p.factor * A : (int64_t)INT32_MAX;
  r.st = p.status0[u];
  if (r.st == 0 && N == 0) r.st = KHG_LAT_NO_PATH;
  int64_t n_arcs = 0;
  if (r.st == 0) {
    for (int s = lane; s < N; s += DT_NT) { v.cl_stamp[s] = 0; v.in_stamp[s] = 0; v.cnt[s] = 0; }
    const int T = v.frame[N - 1], start = p.lo.start[u];
    if (lane == 0) {
      v.d_off[0] = 0; v.d_koff[0] = 0;
      if (A > 0) { v.u_dest[0] = start; v.u_a[0] = 0.0f; v.u_b[0] = 0.0f; }       // (with A == 0 the per-arc slices are empty)
    }
    __syncthreads();
    if (A == 0) {
      // one state, no arc: D0 = {start}, nothing to expand
      if (r.cap_s < 1) r.st = KHG_LAT_SCRATCH;
      else {
        if (lane == 0) {
          v.e_s[0] = start; v.e_a[0] = 0.0f; v.e_b[0] = 0.0f; v.e_slot[0] = 0; v.e_d[0] = 0; v.e_within[0] = 0; v.cnt[start] = 1;
          v.d_off[1] = 1; v.d_koff[1] = 1; v.d_hash[0] = 0;
          v.d_fin[0] = v.fin[start] != __builtin_huge_valf() && v.frame[start] == T ? start : -1;
        }
        r.used_s = 1; r.nD = 1; r.max_k = 1; r.max_c = 1;
        __syncthreads();
      }
    } else {
      dt_arrive(p, v, &r, 0, 1, lane, T);
    }
    for (int d = 0; d < r.nD && r.st == 0 && A > 0; ++d) {
      // the word arcs that leave the closure of d
      int n = 0;
      const int e0 = v.d_off[d], e1 = v.d_off[d + 1];
      for (int eb = e0; eb < e1 && r.st == 0; eb += DT_NT) {
        const int e = eb + lane;
        int alo = 0, ahi = 0;
        float ea = 0.0f, ebv = 0.0f;
        if (e < e1) { const int q = v.e_s[e]; alo = v.abeg[q]; ahi = dt_aend(v, q); ea = v.e_a[e]; ebv = v.e_b[e]; }
        const int md = dt_wave_max(ahi - alo);
        for (int k = 0; k < md; ++k) {
          const int a = alo + k;
          const bool is = a < ahi && v.ol[a] != 0;
          const unsigned long long bal = __ballot(is);
          const int c = __popcll(bal);
          if (n + c > A) { r.st = KHG_LAT_SCRATCH; break; }
          if (is) {
            const int pos = n + __popcll(bal & ((1ull << lane) - 1ull));
            float wa, wb;
            dt_weight(p, v, a, &wa, &wb);
            v.u_w[pos] = v.ol[a]; v.u_dest[pos] = v.next[a]; v.u_arc[pos] = a; v.u_a[pos] = ea + wa; v.u_b[pos] = ebv + wb; v.u_e[pos] = e;
          }
          n += c;
        }
      }
      __syncthreads();
      if (r.st != 0) break;
      // rank-sorted by (word, dest, cost, arc): a permutation, the arcs being distinct
      for (int i = lane; i < n; i += DT_NT) {
        const int wi = v.u_w[i], di = v.u_dest[i], ai = v.u_arc[i];
        const float xa = v.u_a[i], xb = v.u_b[i];
        const uint32_t si = dt_ord(xa + xb), oi = dt_ord(xa);
        int rank = 0;
        for (int j = 0; j < n; ++j) {
          const int wj = v.u_w[j], dj = v.u_dest[j];
          bool less = wj < wi || (wj == wi && dj < di);
          if (wj == wi && dj == di) {
            const float ya = v.u_a[j], yb = v.u_b[j];
            const uint32_t sj = dt_ord(ya + yb), oj = dt_ord(ya);
            less = sj < si || (sj == si && (oj < oi || (oj == oi && v.u_arc[j] < ai)));
          }
          rank += less ? 1 : 0;
        }
        v.s_w[rank] = wi; v.s_dest[rank] = di; v.s_arc[rank] = ai; v.s_a[rank] = xa; v.s_b[rank] = xb; v.s_e[rank] = v.u_e[i];
      }
      __syncthreads();
      // the kept candidates: the first of every (word, dest) run, back into u_*
      int nw = 0;
      for (int ib0 = 0; ib0 < n; ib0 += DT_NT) {
        const int i = ib0 + lane;
        const bool first = i < n && (i == 0 || v.s_w[i - 1] != v.s_w[i] || v.s_dest[i - 1] != v.s_dest[i]);
        const unsigned long long bal = __ballot(first);
        if (first) {
          const int k = nw + __popcll(bal & ((1ull << lane) - 1ull));
          v.u_w[k] = v.s_w[i]; v.u_dest[k] = v.s_dest[i]; v.u_arc[k] = v.s_arc[i]; v.u_a[k] = v.s_a[i]; v.u_b[k] = v.s_b[i]; v.u_e[k] = v.s_e[i];
        }
        nw += __popcll(bal);
      }
      __syncthreads();
      // word by word
      for (int g0 = 0; g0 < nw && r.st == 0;) {
        const int w = v.u_w[g0];
        int g1 = nw;
        for (int t = g0; t < nw; t += DT_NT) {
          const bool same = t + lane < nw && v.u_w[t + lane] == w;
          const unsigned long long bal = __ballot(same);
          if (bal != ~0ull) { g1 = t + __ffsll((long long)~bal) - 1; break; }
        }
        const int d2 = dt_arrive(p, v, &r, g0, g1, lane, T);
        if (d2 < 0) break;
        const int t0 = v.d_off[d2], t1 = v.d_off[d2 + 1];
        bool lost = false;
        for (int i = g0 + lane; i < g1; i += DT_NT) {
          const int dest = v.u_dest[i];
          if (v.t_pred[v.cl_idx[dest]] >= 0) continue;       // dominated: the arc inside the closure is its in-arc
          int lo = t0, hi = t1;
          while (lo < hi) { const int mid = (lo + hi) >> 1; if (v.e_s[mid] < dest) lo = mid + 1; else hi = mid; }
          if (lo >= t1 || v.e_s[lo] != dest) { lost = true; continue; }
          const int e = v.u_e[i], q = v.e_s[e];
          v.slot[(int64_t)v.e_slot[e] + (v.u_arc[i] - v.abeg[q])] = lo;
        }
        if (__ballot(lost)) { r.st = KHG_LAT_SCRATCH; break; }
        g0 = g1;
        __syncthreads();
      }
    }
    __syncthreads();
    if (r.st == 0) {
      // base[s]: the first new number of the elements of s
      int tot = 0;
      for (int sb = 0; sb < N; sb += DT_NT) {
        const int s = sb + lane;
        const int c = s < N ? v.cnt[s] : 0;
        int incl = c;
        for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o); if (lane >= o) incl += t; }
        if (s < N) v.cnt[s] = tot + incl - c;
        tot += __shfl(incl, 63);
      }
      __syncthreads();
      const int NE = (int)r.used_s;
      for (int e = lane; e < NE; e += DT_NT) {
        const int s = v.e_s[e], id = v.cnt[s] + v.e_within[e];
        const int deg = dt_aend(v, s) - v.abeg[s];
        const int64_t off = v.e_slot[e];
        int kept = 0;
        for (int k = 0; k < deg; ++k) kept += v.slot[off + k] >= 0 ? 1 : 0;
        v.y_elem[id] = e; v.y_abeg[id] = kept;
      }
      __syncthreads();
      for (int ib0 = 0; ib0 < NE; ib0 += DT_NT) {
        const int i = ib0 + lane;
        const long long c = i < NE ? v.y_abeg[i] : 0;
        long long incl = c;
        for (int o = 1; o < 64; o <<= 1) { const long long t = __shfl_up(incl, o); if (lane >= o) incl += t; }
        if (i < NE) v.y_abeg[i] = (int32_t)(n_arcs + incl - c);
        n_arcs += __shfl(incl, 63);
      }
    }
  }
  if (lane == 0) {
    const bool ok = r.st == 0;
    p.lo.status[u] = ok ? KHG_LAT_SUCCEEDED : r.st;
    p.det_states[u] = ok ? r.nD : 0; p.max_subset[u] = ok ? r.max_k : 0; p.max_closure[u] = ok ? r.max_c : 0;
    p.lo.utt_tot[2 * (int64_t)b] = ok ? r.used_s : 0;
    p.lo.utt_tot[2 * (int64_t)b + 1] = ok ? n_arcs : 0;
  }
}

// ---- fill: one lane per new state; grid (utterance, stripes of new states) ----
__global__ __launch_bounds__(DT_NT) void k2_lattice_det_fill(DtArgs p) {
  const int b = (int)blockIdx.x, u = p.lo.u0 + b;
  const int64_t s0 = p.lo.state_off[u] - p.lo.s_base, a0 = p.lo.arc_off[u] - p.lo.a_base;
  const int64_t so_out = p.lo.utt_off[b], ao_out = p.lo.utt_off[(int64_t)p.lo.n + 1 + b];
  const int NS = (int)(p.lo.utt_off[b + 1] - so_out);
  const DtView v = dt_view(p, b, u);
  if (blockIdx.y == 0 && threadIdx.x == 0) p.lo.o_start[u] = NS > 0 ? v.cnt[p.lo.start[u]] : -1;       // (start, D0): the first element of all
  if (NS == 0) return;
  const float INF = __builtin_huge_valf();
  for (int r = (int)blockIdx.y * DT_NT + (int)threadIdx.x; r < NS; r += (int)gridDim.y * DT_NT) {
    const int e = v.y_elem[r], s = v.e_s[e];
    const int64_t sid = so_out + r;
    p.lo.out.frame[sid] = p.lo.in.frame[s0 + s]; p.lo.out.gstate[sid] = p.lo.in.gstate[s0 + s];
    p.lo.out.tot[sid] = p.lo.in.tot[s0 + s]; p.lo.out.extra[sid] = p.lo.in.extra[s0 + s];
    p.lo.out.fin[sid] = v.d_fin[v.e_d[e]] == s ? v.fin[s] : INF;
    p.lo.out.arc_begin[sid] = v.y_abeg[r];
    int64_t pos = ao_out + v.y_abeg[r];
    const int alo = v.abeg[s], ahi = dt_aend(v, s);
    const int64_t off = v.e_slot[e];
    for (int a = alo; a < ahi; ++a) {
      const int t = v.slot[off + (a - alo)];
      if (t < 0) continue;
      p.lo.out.ilabel[pos] = p.lo.in.ilabel[a0 + a]; p.lo.out.olabel[pos] = v.ol[a];
      p.lo.out.g[pos] = v.g[a]; p.lo.out.ac[pos] = v.ac[a];
      p.lo.out.next[pos] = v.cnt[v.e_s[t]] + v.e_within[t];
      ++pos;
    }
  }
}

// ---- check: what khg_lattices_determinize refuses before it prunes; one wave per utterance of the input ----
__global__ __launch_bounds__(DT_NT) void k2_lattice_det_check(LoArgs p, int32_t* status0) {
  const int b = (int)blockIdx.x, u = p.u0 + b, lane = (int)threadIdx.x;
  const int64_t s0 = p.state_off[u] - p.s_base, a0 = p.arc_off[u] - p.a_base;
  const int N = (int)(p.state_off[u + 1] - p.state_off[u]), A = (int)(p.arc_off[u + 1] - p.arc_off[u]);
  const int32_t* abeg = p.in.arc_begin + s0;
  const int32_t* next = p.in.next + a0;
  bool bad = false;
  for (int s = lane; s < N; s += DT_NT) {
    const int ae = s + 1 < N ? abeg[s + 1] : A;
    for (int a = abeg[s]; a < ae; ++a) bad = bad || next[a] <= s;
  }
  const bool any = __ballot(bad) != 0;
  if (lane == 0) status0[u] = N == 0 ? KHG_LAT_NO_PATH : any ? KHG_LAT_EPS_LOOP : 0;
}
