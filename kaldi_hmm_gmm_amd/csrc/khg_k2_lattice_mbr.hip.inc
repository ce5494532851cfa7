// K2B: minimum Bayes risk decoding and word confidences of device-resident lattices (khg_lattices_mbr: lattice-mbr-decode and the
// confidence column of lattice-to-ctm-conf; Kaldi's MinimumBayesRisk).  The rule is written out at khg_lattices_mbr in
// include/khg_hip.h and repeated in DESIGN.md section 7t.  Three kernels:
//   k2_lattice_mbr_weights   the arc weights p_a and the final weights pf_f, from the forward body that khg_lattices_posteriors runs
//                            (po_alpha_total_beta): the ONLY place where exp enters.  One workgroup of four waves per utterance.
//   k2_lattice_mbr_prepare   per utterance the greatest number of words on a start -> final path (an int32 pass, lane 0), the distinct
//                            olabels ascending with 0 first, and every arc's index into them.  One wave per utterance.
//   k2_lattice_mbr           the whole loop -- forward, backward, pick, compaction, the next iteration -- for one utterance per wave,
//                            lanes over the positions q = 0 .. Q of the normalised hypothesis, 64 positions a segment.
// Everything in k2_lattice_mbr is +, *, < and <= on doubles under fp contract(off), in the order of the rule.  The two serial
// recurrences in q run as fixed-point iterations over the lanes: a3 (v_q = min(v_q, fl(v_{q-1} + ins))) and the backward carry along a
// run of move 3 (ba_q = fl(ba_{q+1} + t_q)); their fixed points are unique and are the serial values, whatever the number of rounds.
// A segment's carry-in of the a3 chain is kept in the lane of its number (at most 64 segments: Q + 1 <= 4096), so the backward pass,
// which takes the segments in descending order, first runs the chain upwards once.  AD, BD and gamma are HBM scratch (not staged in
// LDS): lane q owns column q of BD and of gamma, so there are no atomics and the AD rows -- read at q and q - 1 -- are fenced by one
// barrier per state (one wave per workgroup).

#define MB_NT 64
#define MB_DEL (1.0 + 1e-5)              // Kaldi's delta on a deletion
#define MB_MAX_WORDS 2047                // 2 W + 2 <= 64 segments of 64 positions

// ---- the weights ----
__global__ __launch_bounds__(PO_NT) void k2_lattice_mbr_weights(PoArgs p, double* final_cond) {
#pragma clang fp contract(off)
  extern __shared__ double po_lds[];
  __shared__ double sh_tot;
  const double NINF = -__builtin_huge_val();
  const float FINF = __builtin_huge_valf();
  const PoView w = po_open<3>(p, po_lds);
  const LoView& v = w.v;
  for (int s = (int)threadIdx.x; s < w.N; s += PO_NT) final_cond[w.s0 + s] = 0.0;
  if (w.N == 0 || v.start < 0) { po_fail(p, w, KHG_LAT_NO_PATH); return; }
  if (!po_admissible(w)) { po_fail(p, w, KHG_LAT_EPS_LOOP); return; }
  po_frames(w);
  __syncthreads();
  bool settled;
  const double tot = po_alpha_total_beta(w, &sh_tot, &settled);
  if (!settled) { po_fail(p, w, KHG_LAT_EPS_LOOP); return; }
  if (tot == NINF) { po_fail(p, w, KHG_LAT_NO_PATH); return; }
  for (int a = (int)threadIdx.x; a < w.A; a += PO_NT) {
    const double al = w.alpha[w.asrc[a]], ad = w.alpha[v.next[a]];
    p.arc_post[w.a0 + a] = al != NINF && ad != NINF ? exp((al + po_w(v, w.gs, w.as, a)) - ad) : 0.0;
  }
  for (int s = w.fs[w.T] + (int)threadIdx.x; s < w.N; s += PO_NT) {
    const float c = v.fin[s];
    const double al = w.alpha[s];
    if (c != FINF && al != NINF) final_cond[w.s0 + s] = exp((al + -(w.gs * (double)c)) - tot);
  }
  if (threadIdx.x == 0) { p.lo.status[w.u] = KHG_LAT_SUCCEEDED; p.tot[w.u] = tot; }
}

// ---- the longest path's words, the vocabulary, the arcs' indices into it ----
// len [chunk states] and first [chunk arcs] are scratch; vocab: utterance u's slot of A + 1 entries at arc_off[u] + u; widx [chunk arcs]
__global__ __launch_bounds__(MB_NT) void k2_lattice_mbr_prepare(LoArgs p, const int32_t* arc_src, int32_t* len, int32_t* first, int32_t* vocab, int32_t* widx,
                                                                int32_t* nvocab, int32_t* max_words) {
  const int b = (int)blockIdx.x, u = p.u0 + b, lane = (int)threadIdx.x;
  const int64_t s0 = p.state_off[u] - p.s_base, a0 = p.arc_off[u] - p.a_base;
  const int N = (int)(p.state_off[u + 1] - p.state_off[u]), A = (int)(p.arc_off[u + 1] - p.arc_off[u]);
  const int32_t* ol = p.in.olabel + a0;
  const int32_t* next = p.in.next + a0;
  const int32_t* src = arc_src + a0;
  int32_t* voc = vocab + p.arc_off[u] + u;
  int32_t* fst = first + a0;
  if (lane == 0) {
    int best = 0;
    const int start = N ? p.start[u] : -1;
    if (start >= 0 && start < N) {
      int32_t* L = len + s0;
      for (int s = 0; s < N; ++s) L[s] = -1;
      L[start] = 0;
      for (int a = 0; a < A; ++a) {        // arcs by source state; an arc that does not go up belongs to a refused lattice
        const int s = src[a], d = next[a];
        if (L[s] >= 0 && d > s) L[d] = max(L[d], L[s] + (ol[a] != 0 ? 1 : 0));
      }
      const int T = p.in.frame[s0 + N - 1];
      for (int s = N - 1; s >= 0 && p.in.frame[s0 + s] == T; --s)
        if (p.in.fin[s0 + s] != __builtin_huge_valf() && L[s] > best) best = L[s];
    }
    max_words[u] = best;
    voc[0] = 0;
  }
  int nfirst = 0;
  for (int ab = 0; ab < A; ab += MB_NT) {
    const int a = ab + lane;
    int f = 0;
    if (a < A && ol[a] != 0) {
      f = 1;
      const int w = ol[a];
      for (int k = 0; k < a; ++k) if (ol[k] == w) { f = 0; break; }
    }
    if (a < A) fst[a] = f;
    nfirst += __popcll(__ballot(f));
  }
  __syncthreads();
  for (int a = lane; a < A; a += MB_NT) {
    if (!fst[a]) continue;
    const int w = ol[a];
    int r = 0;
    for (int k = 0; k < A; ++k) r += fst[k] && ol[k] < w;
    voc[1 + r] = w;
  }
  if (lane == 0) nvocab[u] = 1 + nfirst;
  __syncthreads();
  const int V = 1 + nfirst;
  for (int a = lane; a < A; a += MB_NT) {
    const int w = ol[a];
    int l = 0, h = V;                      // voc[l] <= w < voc[h]
    while (h - l > 1) { const int mid = (l + h) >> 1; if (voc[mid] <= w) l = mid; else h = mid; }
    widx[a0 + a] = l;
  }
}

struct MbArgs {
  LoArgs lo;                             // the chunk's lattices
  const int32_t *in_begin, *in_arc, *arc_src;     // LatIndex
  const int32_t* list;                   // [launch] the utterances of the launch
  const int64_t* tab_off;                // [launch] the first cell of each one's table in `tab`: AD [N + 1][C], BD [N + 1][C], gamma [V][C]; C = 2 cap + 2
  double* tab;
  const double *arc_cond, *final_cond;   // [chunk arcs], [chunk states]
  const int32_t *widx, *vocab, *nvocab;  // [chunk arcs]; the handle's slots (arc_off[u] + u); [U]
  const int32_t *cap, *w0;               // [U] the cap on the words, the initial hypothesis's length
  const int64_t *cap_off, *gout_off;     // [U] utterance u: hyp at 2 * cap_off[u] (two halves of cap), conf at cap_off[u]; gamma_out at gout_off[u]
  int32_t* hyp;
  double *conf, *gamma_out;              // gamma_out: [Q][V] dense, in a slot of (2 cap + 1) * V
  int32_t *status, *iters, *nwords;      // [U]
  double* risk;                          // [U]
  int32_t decode_mbr, max_iter;
};

// one utterance's loop state, the same in every lane
struct MbView {
  int N, Q, C, lane, start, last_lo;
  const int32_t *ib, *in_arc, *arc_src, *ol, *widx;
  const double *arc_cond, *final_cond;
  double *AD, *BD, *G;
  const int32_t* h;
};

// in-arc j of state n (n == N: the virtual end state, one in-arc per state of the last frame): source, word, index of the word, weight
__device__ __forceinline__ void mb_in_arc(const MbView& m, int n, int j, int* s, int* w, int* wi, double* p) {
  if (n < m.N) {
    const int a = m.in_arc[m.ib[n] + j];
    *s = m.arc_src[a]; *w = m.ol[a]; *wi = m.widx[a]; *p = m.arc_cond[a];
  } else {
    *s = m.last_lo + j; *w = 0; *wi = 0; *p = m.final_cond[m.last_lo + j];
  }
}
__device__ __forceinline__ int mb_in_degree(const MbView& m, int n) { return n < m.N ? m.ib[n + 1] - m.ib[n] : m.N - m.last_lo; }

// r(q) of lane position q (0 outside 1 .. Q and at odd q)
__device__ __forceinline__ int mb_r(const MbView& m, int q) { return q >= 2 && q <= m.Q && (q & 1) == 0 ? m.h[(q >> 1) - 1] : 0; }

// One segment of an arc row: arc[q] and b[q] of lane position q = qb + lane from the source's row ADs, the arc's word w and the settled
// arc[qb - 1] (carry; unused at qb = 0).  A position past Q gets +inf and b = 0.
__device__ __forceinline__ double mb_arc_segment(const MbView& m, const double* ADs, int qb, int w, double carry, int* b_out) {
#pragma clang fp contract(off)
  const double INF = __builtin_huge_val();
  const int lane = m.lane, q = qb + lane;
  const bool in = q <= m.Q;
  const int rq = mb_r(m, q);
  const double insq = rq != 0 ? 1.0 : 0.0;
  const double delw = w != 0 ? MB_DEL : 0.0;
  double v = INF;
  int b = 0;
  if (in) {
    const double a2 = ADs[q] + delw;
    v = a2; b = 2;
    if (q > 0) {
      const double a1 = ADs[q - 1] + (w == rq ? 0.0 : 1.0);
      if (a1 <= a2) { v = a1; b = 1; }
    }
  }
  const double v12 = v;
  const bool chained = in && q > 0;
  for (int round = 0; round < MB_NT; ++round) {      // a chain over 64 lanes has settled after 64 rounds at the latest
    double up = __shfl_up(v, 1);
    if (lane == 0) up = carry;
    const double cand = up + insq;
    const bool take = chained && cand < v;
    if (take) v = cand;
    if (!__ballot(take)) break;
  }
  if (v < v12) b = 3;
  *b_out = b;
  return v;
}

// ba[q] = (b[q + 1] == 3 ? ba[q + 1] : 0) + t[q] over one segment; lane 63's upper neighbour is (up3, up_ba)
__device__ __forceinline__ double mb_carry_down(int lane, double t, bool next3, double up_ba) {
#pragma clang fp contract(off)
  double ba = t;
  for (int round = 0; round < MB_NT; ++round) {
    double nb = __shfl_down(ba, 1);
    if (lane == MB_NT - 1) nb = up_ba;
    const double nba = (next3 ? nb : 0.0) + t;
    const bool changed = __double_as_longlong(nba) != __double_as_longlong(ba);
    ba = nba;
    if (!__ballot(changed)) break;
  }
  return ba;
}

// AD of every state but the start's, in state order
__device__ __forceinline__ void mb_forward(const MbView& m) {
#pragma clang fp contract(off)
  for (int n = 0; n <= m.N; ++n) {
    if (n != m.start) {
      double* ADn = m.AD + (int64_t)n * m.C;
      const int deg = mb_in_degree(m, n);
      for (int j = 0; j < deg; ++j) {
        int s, w, wi; double p;
        mb_in_arc(m, n, j, &s, &w, &wi, &p);
        if (p == 0.0) continue;
        const double* ADs = m.AD + (int64_t)s * m.C;
        double carry = 0.0;
        for (int qb = 0; qb <= m.Q; qb += MB_NT) {
          int b;
          const double v = mb_arc_segment(m, ADs, qb, w, carry, &b);
          carry = __shfl(v, MB_NT - 1);
          const int q = qb + m.lane;
          if (q <= m.Q) { const double pv = p * v; ADn[q] = ADn[q] + pv; }
        }
      }
    }
    __syncthreads();
  }
}

// BD and gamma, states N down to 0 without the start, whose row is drained at the end
__device__ __forceinline__ void mb_backward(const MbView& m) {
#pragma clang fp contract(off)
  const int lane = m.lane;
  const int top = (m.Q / MB_NT) * MB_NT;           // the first position of the last segment
  for (int n = m.N; n >= 0; --n) {
    if (n == m.start) continue;
    const double* BDn = m.BD + (int64_t)n * m.C;
    const int deg = mb_in_degree(m, n);
    for (int j = 0; j < deg; ++j) {
      int s, w, wi; double p;
      mb_in_arc(m, n, j, &s, &w, &wi, &p);
      if (p == 0.0) continue;
      const double* ADs = m.AD + (int64_t)s * m.C;
      double* BDs = m.BD + (int64_t)s * m.C;
      // the a3 chain's carry into every segment: segment k's in lane k (when Q + 1 > 64 this runs the lower segments' rows a second time)
      double carries = 0.0, carry = 0.0;
      for (int qb = 0; qb < top; qb += MB_NT) {
        int b;
        const double v = mb_arc_segment(m, ADs, qb, w, carry, &b);
        carry = __shfl(v, MB_NT - 1);
        if (lane == qb / MB_NT + 1) carries = carry;
      }
      bool up3 = false;
      double up_ba = 0.0, up_t1 = 0.0;
      for (int qb = top; qb >= 0; qb -= MB_NT) {
        int b;
        (void)mb_arc_segment(m, ADs, qb, w, __shfl(carries, qb / MB_NT), &b);
        const int q = qb + lane;
        const bool in = q <= m.Q;
        double t = 0.0;
        if (in) t = p * BDn[q];
        int bn = __shfl_down(b, 1);
        if (lane == MB_NT - 1) bn = up3 ? 3 : 0;
        const double ba = mb_carry_down(lane, t, bn == 3, up_ba);
        const double term1 = in && b == 1 ? ba : 0.0;              // to cell q - 1
        const double term2 = in && b == 2 ? ba : 0.0;              // to cell q (position 0 is always move 2)
        if (in && b == 1) { double* g = m.G + (int64_t)wi * m.C + q; *g = *g + ba; }
        if (in && b == 3) { double* g = m.G + q; *g = *g + ba; }
        double t1 = __shfl_down(term1, 1);
        if (lane == MB_NT - 1) t1 = up_t1;
        if (in) { const double c = BDs[q] + t1; BDs[q] = c + term2; }
        up3 = __shfl(b, 0) == 3; up_ba = __shfl(ba, 0); up_t1 = __shfl(term1, 0);
      }
    }
  }
  // the start row: ba[q] = ba[q + 1] + BD[start][q], q = Q .. 1, all of it epsilon mass
  const double* BDst = m.BD + (int64_t)m.start * m.C;
  double up_ba = 0.0;
  for (int qb = top; qb >= 0; qb -= MB_NT) {
    const int q = qb + lane;
    const bool in = q >= 1 && q <= m.Q;
    const double t = in ? BDst[q] : 0.0;
    const double ba = mb_carry_down(lane, t, q + 1 <= m.Q, up_ba);
    if (in) { double* g = m.G + q; *g = *g + ba; }
    up_ba = __shfl(ba, 0);
  }
}

__global__ __launch_bounds__(MB_NT) void k2_lattice_mbr(MbArgs p) {
#pragma clang fp contract(off)
  const int k = (int)blockIdx.x, u = p.list[k], bu = u - p.lo.u0, lane = (int)threadIdx.x;
  const int64_t s0 = p.lo.state_off[u] - p.lo.s_base, a0 = p.lo.arc_off[u] - p.lo.a_base;
  const int N = (int)(p.lo.state_off[u + 1] - p.lo.state_off[u]);
  const int V = p.nvocab[u], cap = p.cap[u], C = 2 * cap + 2;
  const int32_t* voc = p.vocab + p.lo.arc_off[u] + u;
  const int32_t* frame = p.lo.in.frame + s0;
  MbView m;
  m.N = N; m.C = C; m.lane = lane; m.start = p.lo.start[u];
  m.ib = p.in_begin + s0 + bu; m.in_arc = p.in_arc + a0; m.arc_src = p.arc_src + a0; m.ol = p.lo.in.olabel + a0; m.widx = p.widx + a0;
  m.arc_cond = p.arc_cond + a0; m.final_cond = p.final_cond + s0;
  m.AD = p.tab + p.tab_off[k]; m.BD = m.AD + (int64_t)(N + 1) * C; m.G = m.BD + (int64_t)(N + 1) * C;
  int last_lo = N - 1;
  while (last_lo > 0 && frame[last_lo - 1] == frame[N - 1]) --last_lo;
  m.last_lo = last_lo;
  int32_t* ha = p.hyp + 2 * p.cap_off[u];
  int32_t* hb = ha + cap;
  int32_t *h = ha, *hn = hb;
  const int64_t cells = (2 * (int64_t)(N + 1) + V) * C;
  int W = p.w0[u], iters = 0, st = KHG_LAT_SUCCEEDED;
  double risk = 0.0;
  for (;;) {
    m.Q = 2 * W + 1; m.h = h;
    for (int64_t i = lane; i < cells; i += MB_NT) m.AD[i] = 0.0;
    __syncthreads();
    for (int q = lane; q <= m.Q; q += MB_NT) m.AD[(int64_t)m.start * C + q] = (double)(q >> 1);      // sums of ins(r): 0, 0, 1, 1, 2, ...
    if (lane == 0) m.BD[(int64_t)N * C + m.Q] = 1.0;
    __syncthreads();
    mb_forward(m);
    risk = m.AD[(int64_t)N * C + m.Q];
    mb_backward(m);
    __syncthreads();
    if (!p.decode_mbr) break;
    // the picks, and the ones that are words packed in order
    int Wn = 0, differs = 0;
    for (int qb = 0; qb <= m.Q; qb += MB_NT) {
      const int q = qb + lane;
      int word = 0;
      if (q >= 1 && q <= m.Q) {
        double best = m.G[q];
        int bi = 0;
        for (int x = 1; x < V; ++x) { const double g = m.G[(int64_t)x * C + q]; if (best < g) { best = g; bi = x; } }
        word = voc[bi];
      }
      const unsigned long long mask = __ballot(word != 0);
      const int idx = Wn + __popcll(mask & ((1ull << lane) - 1ull));
      if (word != 0) {
        if (idx < cap) hn[idx] = word;
        if (idx >= W || h[idx] != word) differs = 1;
      }
      Wn += __popcll(mask);
    }
    differs = __ballot(differs) != 0 || Wn != W;
    __syncthreads();
    if (!differs) break;
    if (iters == p.max_iter) { st |= KHG_LAT_NOT_CONVERGED; break; }
    if (Wn > cap) {
      if (lane == 0) { p.status[u] = KHG_LAT_WORDS; p.iters[u] = iters; p.nwords[u] = 0; p.risk[u] = __builtin_huge_val(); }
      return;
    }
    int32_t* t = h; h = hn; hn = t;
    W = Wn; ++iters;
  }
  // the outputs of the last accumulation: the words in the slot's first half, conf, the table [Q][V]
  if (h != ha) for (int i = lane; i < W; i += MB_NT) ha[i] = h[i];
  double* conf = p.conf + p.cap_off[u];
  for (int i = lane; i < W; i += MB_NT) {
    const int w = h[i];
    int l = 0, r = V;
    while (r - l > 1) { const int mid = (l + r) >> 1; if (voc[mid] <= w) l = mid; else r = mid; }
    conf[i] = voc[l] == w ? m.G[(int64_t)l * C + 2 * (i + 1)] : 0.0;
  }
  // (lanes over q, so a lane's stores are V doubles apart: uncoalesced, once per call, and V is small where Q is)
  double* out = p.gamma_out + p.gout_off[u];
  for (int q = 1 + lane; q <= m.Q; q += MB_NT)
    for (int x = 0; x < V; ++x) out[(int64_t)(q - 1) * V + x] = m.G[(int64_t)x * C + q];
  if (lane == 0) { p.status[u] = st; p.iters[u] = iters; p.nwords[u] = W; p.risk[u] = risk; }
}
