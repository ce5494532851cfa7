// K2N: the n best paths of device-resident lattices (khg_lattices_nbest: lattice-to-nbest | nbest-to-linear).  The rule is DESIGN.md
// section 7v (include/khg_hip.h states it in full): per state s, ascending, the list A[s] of the n least prefixes under the key
// (t', e, j) -- t' = fl(t + c) the scalar ordering key, e the in-arc, j the rank in the source's list -- and at the end the n least
// complete paths under (total, s, j).  All in float under fp contract(off).
//
// Count -> k2_lattice_scan_pairs -> fill -> k2_lattice_scan_pairs -> trace.  The count (one wave per utterance, the in-arcs of a state
// across the lanes) bounds every list: len[s] = min(n, sum of len[p]), which sizes an exact arena of SoA rows (t, a, b, nw, e, j).
// The fill (one wave per utterance, states ascending) keeps the running list and its successor as a ping-pong pair in LDS (or, when
// the device gives less LDS than 52 n bytes or KHG_OPT_LAT_OPS_LDS = 1, in HBM rows through the same code) and merges one in-arc at
// a time by rank: the in-arc index is in ascending arc order, which is the key's order, so the running list's elements come before
// equal keys of the arc (strict search on one side, non-strict on the other); t' is non-decreasing in j (x <= y implies
// fl(x + c) <= fl(y + c)), so the extended list is sorted as it stands and its dropped candidates (t' not < +inf) are its tail.
// A lane holding element i of one list binary-searches the other and writes to i + count when that is < n; lanes stride over ranks.
// The final selection is the same merge over the final states of frame T.  The trace runs one lane per entry from (end state, rank)
// back to the start through (e, j), writing the alignment by frame and the words from the back of the entry's slot: one writer per
// slot.  No atomics: nothing depends on timing.  Every loop is bounded by a size (states, arcs, n, 64), every arena write is checked
// against the arena's size: a defect ends in KHG_LAT_SCRATCH, not in a stray write.

#define NB_NT 64
#define NB_ROW_WORDS 13      // the fill's rows per utterance: two lists of 6 n words and n keys of the extended list

struct NbArgs {
  LoArgs lo;                             // the chunk: its lattices, start, state_off / arc_off, s_base / a_base, u0, n (utterances), U
  const int32_t *in_begin, *in_arc, *arc_src;     // LatIndex of the chunk
  float gs, as;
  int32_t nb;                            // n of the call
  int32_t b0, gn;                        // this launch takes the chunk's utterances b0 .. b0 + gn
  int32_t* status;                       // [U]
  // count: per state the bound of its list and where the list starts in the utterance's part of the arena
  int32_t *len, *loff;                   // [chunk states]
  int64_t* utt_tot;                      // [2 * chunk utterances]: (list elements, bound of the entries)
  const int64_t* utt_off;                // [2 * (chunk utterances + 1)]: their scan
  // fill
  int32_t* alen;                         // [chunk states]: the lists' lengths
  float *r_t, *r_a, *r_b;                // the arena's rows [arena_size]: the lists of the launch's utterances
  int32_t *r_nw, *r_e, *r_j;
  int64_t arena_base, arena_size;        // utt_off[b0]; elements
  int32_t* rows;                         // the HBM form's rows [gn][NB_ROW_WORDS * nb] (nullptr: LDS)
  int32_t *s_end, *s_rank, *s_nw, *s_woff;        // per entry slot of the chunk (utt_off's second column): end state, rank, words, first word
  float *s_a, *s_b, *s_tot;
  int64_t* utt_tot2;                     // [2 * chunk utterances]: (entries, words)
  // trace
  const int64_t* utt_off2;               // [2 * (gn + 1)]: the scan of utt_tot2 over the launch's utterances
  const int64_t* ali_base;               // [gn]: where the utterance's alignments start in o_ali
  const int64_t* ali_off;                // [U + 1]: the handle's alignment layout
  int32_t *o_ali, *o_words, *o_nw;       // [o_na], [o_nwords], [o_ne]
  float *o_weight, *o_total;             // [o_ne][2], [o_ne]
  int64_t o_ne, o_nwords, o_na;
};

struct NbList { float *t, *a, *b; int32_t *nw, *e, *j; };

__device__ __forceinline__ NbList nb_list(int32_t* q, int n) {
  NbList l;
  l.t = reinterpret_cast<float*>(q); l.a = l.t + n; l.b = l.a + n; l.nw = q + 3 * n; l.e = q + 4 * n; l.j = q + 5 * n;
  return l;
}
__device__ __forceinline__ int nb_wave_sum(int x) {
  for (int o = 32; o; o >>= 1) x += __shfl_xor(x, o);
  return x;
}
__device__ __forceinline__ long long nb_wave_sum64(long long x) {
  for (int o = 32; o; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

// ---- count: the bounds of the lists and of the entries, the structure's refusals; one wave per utterance ----
__global__ __launch_bounds__(NB_NT) void k2_lattice_nbest_count(NbArgs p) {
  const int b = (int)blockIdx.x, u = p.lo.u0 + b, lane = (int)threadIdx.x;
  const int64_t s0 = p.lo.state_off[u] - p.lo.s_base, a0 = p.lo.arc_off[u] - p.lo.a_base;
  const int N = (int)(p.lo.state_off[u + 1] - p.lo.state_off[u]), A = (int)(p.lo.arc_off[u + 1] - p.lo.arc_off[u]);
  const int32_t *abeg = p.lo.in.arc_begin + s0, *frame = p.lo.in.frame + s0, *next = p.lo.in.next + a0;
  const float* fin = p.lo.in.fin + s0;
  const int32_t *ib = p.in_begin + s0 + b, *in_arc = p.in_arc + a0, *arc_src = p.arc_src + a0;
  int32_t *len = p.len + s0, *loff = p.loff + s0;
  const float INF = __builtin_huge_valf();
  int st = 0;
  if (N == 0) st = KHG_LAT_NO_PATH;
  else {
    bool bad = false;
    for (int s = lane; s < N; s += NB_NT) {
      const int ae = s + 1 < N ? abeg[s + 1] : A;
      for (int a = abeg[s]; a < ae; ++a) bad = bad || next[a] <= s;
    }
    if (__ballot(bad)) st = KHG_LAT_EPS_LOOP;
  }
  long long tot = 0, ecap = 0;
  if (st == 0) {
    const int start = p.lo.start[u], T = frame[N - 1];
    for (int s = 0; s < N; ++s) {
      long long c = 0;
      if (s == start) c = 1;
      else {
        const int j1 = ib[s + 1];
        for (int j = ib[s] + lane; j < j1; j += NB_NT) c += len[arc_src[in_arc[j]]];
        c = nb_wave_sum64(c);
      }
      const int L = (int)(c < (long long)p.nb ? c : (long long)p.nb);
      if (lane == 0) { len[s] = L; loff[s] = (int32_t)tot; }
      tot += L;
      if (frame[s] == T && fabsf(fin[s]) < INF) ecap += L;
      __syncthreads();
    }
    if (tot > (long long)INT32_MAX) st = KHG_LAT_SCRATCH;
    else if (ecap == 0) st = KHG_LAT_NO_PATH;
  }
  if (lane == 0) {
    p.status[u] = st;
    p.utt_tot[2 * (int64_t)b] = st ? 0 : tot;
    p.utt_tot[2 * (int64_t)b + 1] = st ? 0 : (ecap < (long long)p.nb ? ecap : (long long)p.nb);
  }
}

// The running list P [Lc] merged with the list at the arena's xo .. xo + Lp extended by (c; wa, wb, dw; e) into Q, cut at n.
// -> the new length (the lists have changed places), or -1: nothing of the extended list enters and P stands.  All lanes call it.
__device__ __forceinline__ int nb_merge(const NbArgs& p, const NbList& P, const NbList& Q, float* xt, int Lc, int64_t xo, int Lp, float c, float wa,
                                        float wb, int dw, int e, int lane) {
#pragma clang fp contract(off)
  const float INF = __builtin_huge_valf();
  const int n = p.nb;
  int ok = 0;
  for (int k = lane; k < Lp; k += NB_NT) {
    const float t = p.r_t[xo + k] + c;
    xt[k] = t;
    ok += t < INF ? 1 : 0;
  }
  const int Lx = nb_wave_sum(ok);       // the candidates that stay are a prefix: t' does not decrease with the rank
  __syncthreads();
  const bool out = Lx == 0 || (Lc == n && !(xt[0] < P.t[n - 1]));        // wave-uniform
  __syncthreads();
  if (out) return -1;
  for (int i = lane; i < Lc; i += NB_NT) {
    const float key = P.t[i];
    int lo = 0, hi = Lx;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (xt[mid] < key) lo = mid + 1; else hi = mid; }
    const int pos = i + lo;
    if (pos < n) { Q.t[pos] = key; Q.a[pos] = P.a[i]; Q.b[pos] = P.b[i]; Q.nw[pos] = P.nw[i]; Q.e[pos] = P.e[i]; Q.j[pos] = P.j[i]; }
  }
  for (int k = lane; k < Lx; k += NB_NT) {
    const float key = xt[k];
    int lo = 0, hi = Lc;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (P.t[mid] <= key) lo = mid + 1; else hi = mid; }
    const int pos = k + lo;
    if (pos < n) {
      Q.t[pos] = key; Q.a[pos] = p.r_a[xo + k] + wa; Q.b[pos] = p.r_b[xo + k] + wb; Q.nw[pos] = p.r_nw[xo + k] + dw; Q.e[pos] = e; Q.j[pos] = k;
    }
  }
  __syncthreads();
  return Lc + Lx < n ? Lc + Lx : n;
}

// ---- fill: the lists of every state into the arena, the entries into their slots; one wave per utterance ----
template <bool kLds>
__global__ __launch_bounds__(NB_NT) void k2_lattice_nbest_fill(NbArgs p) {
#pragma clang fp contract(off)
  extern __shared__ int32_t nb_lds[];
  const int g = (int)blockIdx.x, b = p.b0 + g, u = p.lo.u0 + b, lane = (int)threadIdx.x;
  const int n = p.nb;
  int32_t* rows = kLds ? nb_lds : p.rows + (int64_t)g * NB_ROW_WORDS * n;
  NbList P = nb_list(rows, n), Q = nb_list(rows + 6 * n, n);
  float* xt = reinterpret_cast<float*>(rows + 12 * n);
  const int64_t s0 = p.lo.state_off[u] - p.lo.s_base, a0 = p.lo.arc_off[u] - p.lo.a_base;
  const int N = (int)(p.lo.state_off[u + 1] - p.lo.state_off[u]);
  const int32_t *frame = p.lo.in.frame + s0, *il = p.lo.in.ilabel + a0, *ol = p.lo.in.olabel + a0;
  const float *fin = p.lo.in.fin + s0, *gc = p.lo.in.g + a0, *ac = p.lo.in.ac + a0;
  const int32_t *ib = p.in_begin + s0 + b, *in_arc = p.in_arc + a0, *arc_src = p.arc_src + a0;
  const int32_t *len = p.len + s0, *loff = p.loff + s0;
  int32_t* alen = p.alen + s0;
  const int64_t ar0 = p.utt_off[b] - p.arena_base, arN = p.utt_off[b + 1] - p.utt_off[b];
  const int64_t sl0 = p.utt_off[(int64_t)p.lo.n + 1 + b], slN = p.utt_off[(int64_t)p.lo.n + 2 + b] - sl0;
  const float INF = __builtin_huge_valf();
  int st = p.status[u], ne = 0;
  long long words = 0;
  if (st == 0 && (ar0 < 0 || ar0 + arN > p.arena_size)) st = KHG_LAT_SCRATCH;
  if (st == 0) {
    const int start = p.lo.start[u], T = frame[N - 1];
    for (int s = 0; s < N && st == 0; ++s) {
      int Lc = 0;
      if (s == start) {
        if (lane == 0) { P.t[0] = 0.0f; P.a[0] = 0.0f; P.b[0] = 0.0f; P.nw[0] = 0; P.e[0] = -1; P.j[0] = 0; }
        Lc = 1;
        __syncthreads();
      } else {
        const int j1 = ib[s + 1];
        for (int i = ib[s]; i < j1; ++i) {
          const int e = in_arc[i], q = arc_src[e];
          const int Lp = alen[q];
          if (Lp == 0) continue;
          const float wa = p.gs * gc[e];
          const float wb = il[e] != 0 ? p.as * ac[e] : 0.0f;
          const float c = wa + wb;
          const int r = nb_merge(p, P, Q, xt, Lc, ar0 + loff[q], Lp, c, wa, wb, ol[e] != 0 ? 1 : 0, e, lane);
          if (r >= 0) { const NbList t = P; P = Q; Q = t; Lc = r; }
        }
      }
      if (Lc > len[s] || (int64_t)loff[s] + Lc > arN) { st = KHG_LAT_SCRATCH; break; }
      const int64_t o = ar0 + loff[s];
      for (int k = lane; k < Lc; k += NB_NT) {
        p.r_t[o + k] = P.t[k]; p.r_a[o + k] = P.a[k]; p.r_b[o + k] = P.b[k]; p.r_nw[o + k] = P.nw[k]; p.r_e[o + k] = P.e[k]; p.r_j[o + k] = P.j[k];
      }
      if (lane == 0) alen[s] = Lc;
      __syncthreads();
    }
    if (st == 0) {
      // the complete paths: the same merge over the final states of frame T, ascending
      int Lc = 0;
      for (int s = 0; s < N; ++s) {
        if (frame[s] != T) continue;
        const float fc = fin[s];
        const int Lp = alen[s];
        if (!(fabsf(fc) < INF) || Lp == 0) continue;
        const float fw = p.gs * fc;
        const int r = nb_merge(p, P, Q, xt, Lc, ar0 + loff[s], Lp, fw, fw, 0.0f, 0, s, lane);
        if (r >= 0) { const NbList t = P; P = Q; Q = t; Lc = r; }
      }
      if (Lc > slN) st = KHG_LAT_SCRATCH;
      else if (Lc == 0) st = KHG_LAT_NO_PATH;
      else {
        ne = Lc;
        for (int kb = 0; kb < ne; kb += NB_NT) {
          const int k = kb + lane;
          const int w = k < ne ? P.nw[k] : 0;
          long long incl = w;
          for (int o = 1; o < 64; o <<= 1) { const long long t = __shfl_up(incl, o); if (lane >= o) incl += t; }
          if (k < ne) {
            const int64_t sl = sl0 + k;
            p.s_end[sl] = P.e[k]; p.s_rank[sl] = P.j[k]; p.s_nw[sl] = w; p.s_woff[sl] = (int32_t)(words + incl - w);
            p.s_a[sl] = P.a[k]; p.s_b[sl] = P.b[k]; p.s_tot[sl] = P.t[k];
          }
          words += __shfl(incl, 63);
        }
        if (words > (long long)INT32_MAX) { st = KHG_LAT_SCRATCH; ne = 0; }
      }
    }
  }
  if (lane == 0) {
    const bool ok = st == 0;
    p.status[u] = ok ? KHG_LAT_SUCCEEDED : st;
    p.utt_tot2[2 * (int64_t)b] = ok ? ne : 0;
    p.utt_tot2[2 * (int64_t)b + 1] = ok ? words : 0;
  }
}

// ---- trace: one lane per entry; grid (utterance of the launch, stripes of entries) ----
__global__ __launch_bounds__(NB_NT) void k2_lattice_nbest_trace(NbArgs p) {
  const int g = (int)blockIdx.x, b = p.b0 + g, u = p.lo.u0 + b;
  const int64_t e0 = p.utt_off2[g], w0 = p.utt_off2[(int64_t)p.gn + 1 + g];
  const int ne = (int)(p.utt_off2[g + 1] - e0);
  const int64_t wN = p.utt_off2[(int64_t)p.gn + 2 + g] - w0;
  if (ne == 0) return;
  const int64_t s0 = p.lo.state_off[u] - p.lo.s_base, a0 = p.lo.arc_off[u] - p.lo.a_base;
  const int N = (int)(p.lo.state_off[u + 1] - p.lo.state_off[u]), A = (int)(p.lo.arc_off[u + 1] - p.lo.arc_off[u]);
  const int32_t *frame = p.lo.in.frame + s0, *il = p.lo.in.ilabel + a0, *ol = p.lo.in.olabel + a0, *arc_src = p.arc_src + a0;
  const int32_t *loff = p.loff + s0, *alen = p.alen + s0;
  const int64_t ar0 = p.utt_off[b] - p.arena_base;
  const int64_t sl0 = p.utt_off[(int64_t)p.lo.n + 1 + b];
  const int T = (int)(p.ali_off[u + 1] - p.ali_off[u]);
  for (int k = (int)blockIdx.y * NB_NT + (int)threadIdx.x; k < ne; k += (int)gridDim.y * NB_NT) {
    const int64_t sl = sl0 + k, eo = e0 + k, ab = p.ali_base[g] + (int64_t)k * T;
    if (eo >= p.o_ne || ab + T > p.o_na) continue;
    const int nw = p.s_nw[sl];
    const int64_t wb = w0 + p.s_woff[sl];
    p.o_weight[2 * eo] = p.s_a[sl]; p.o_weight[2 * eo + 1] = p.s_b[sl]; p.o_total[eo] = p.s_tot[sl]; p.o_nw[eo] = nw;
    int32_t* ali = p.o_ali + ab;
    int s = p.s_end[sl], j = p.s_rank[sl], pos = nw - 1;
    for (int steps = 0; steps < N; ++steps) {
      if (s < 0 || s >= N || j < 0 || j >= alen[s]) break;
      const int64_t o = ar0 + loff[s] + j;
      if (o < 0 || o >= p.arena_size) break;
      const int e = p.r_e[o];
      if (e < 0 || e >= A) break;       // the start's prefix
      const int q = arc_src[e];
      if (il[e] != 0) { const int f = frame[q]; if (f >= 0 && f < T) ali[f] = il[e]; }
      if (ol[e] != 0) {
        if (pos >= 0 && p.s_woff[sl] + (int64_t)pos < wN && wb + pos < p.o_nwords) p.o_words[wb + pos] = ol[e];
        --pos;
      }
      j = p.r_j[o]; s = q;
    }
  }
}
