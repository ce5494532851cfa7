// K2N: rescoring device-resident lattices with a backoff n-gram language model (khg_lattices_lm_rescore: lattice-lmrescore).  The
// rule is DESIGN.md section 7r (include/khg_hip.h states it in full): every state s is split by the set H(s) of LM histories that
// reach it, every arc with a word takes fl(scale * cost of the word from the history) more graph cost, all in float under
// fp contract(off).
//
// Mark -> k2_lattice_scan_pairs -> fill, the shape of khg_lattices_prune.  The history sets depend on each other along the arcs, so an
// utterance is a serial loop over its states (every arc goes to a higher state); its width is the candidates of one state -- the
// in-arcs times the histories of their sources -- which the lanes of ONE wave per utterance take in rounds of 64 through the in-arc
// index of khg_lattices_posteriors (LatIndex).  A round is merged into the state's set by ballot and rank; the set is rank-sorted into
// the utterance's arena, where the sets lie one after the other in state order: the position of (s, h) in the arena IS the new state
// number.  One wave per workgroup, so __syncthreads() is the only fence needed.  No atomics: nothing depends on timing.
// The fill runs one lane per new state: it copies the row, repeats advance() for every labelled arc and finds the target history in
// H(d) by binary search.

#define LM_NT 64

// the LM automaton on the device (khg_lm)
struct LmDev {
  const int32_t *backoff, *arc_begin, *word, *next;
  const float *backoff_cost, *cost, *fin;
  int32_t start;
};

struct LmArgs {
  LoArgs lo;                             // the chunk's lattices, status [U], utt_tot / utt_off, out, o_start
  LmDev lm;
  const int32_t *in_begin, *in_arc, *arc_src;     // LatIndex
  float scale;
  int32_t hist_factor;
  // per utterance u of the chunk (b = u - u0, s0 = state_off[u] - s_base, N states):
  int32_t *arena, *tmp;                  // [hist_factor * chunk states]: the slice of u starts at hist_factor * s0
  int32_t* set_off;                      // [chunk states + n]: N + 1 offsets into the slice, at s0 + b
  int64_t* arc_base;                     // [chunk states]: the first new arc of the first copy of state s, at s0 + s
  int32_t* max_hist;                     // [U]
};

// advance(h, w): -> the next state and *c, or -1: out of vocabulary
__device__ __forceinline__ int lm_advance(const LmDev& m, int h, int w, float* c) {
#pragma clang fp contract(off)
  float acc = 0.0f;
  for (;;) {
    const int end = m.arc_begin[h + 1];
    int lo = m.arc_begin[h], hi = end;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (m.word[mid] < w) lo = mid + 1; else hi = mid;
    }
    if (lo < end && m.word[lo] == w) { *c = acc + m.cost[lo]; return m.next[lo]; }
    if (h == 0) { *c = acc; return -1; }
    acc = acc + m.backoff_cost[h];
    h = m.backoff[h];
  }
}

// One round of at most 64 candidates (valid lanes carry v >= 0) into the unsorted, duplicate-free list tmp[0 .. *cnt).  The list may grow
// to `room` entries; a round that would not fit sets *over and adds nothing.  All lanes call it; ends with a barrier.
__device__ __forceinline__ void lm_merge_round(int32_t* tmp, int* cnt, int64_t room, bool valid, int v, int lane, bool* over) {
  bool found = false;
  if (valid)
    for (int i = 0; i < *cnt; ++i)
      if (tmp[i] == v) { found = true; break; }
  int r, c;
  po_tile_rank(valid && !found ? v : -1 - lane, lane, &r, &c);
  const bool fresh = valid && !found && r == 0;
  const unsigned long long bal = __ballot(fresh);
  const int k = __popcll(bal);
  if ((int64_t)*cnt + k > room) *over = true;
  else {
    if (fresh) tmp[*cnt + __popcll(bal & ((1ull << lane) - 1ull))] = v;
    *cnt += k;
  }
  __syncthreads();
}

// ---- mark: the history sets of every state, the new states' and arcs' offsets, the totals and the status.  One wave per utterance ----
__global__ __launch_bounds__(LM_NT) void k2_lattice_lm_mark(LmArgs p) {
  const int b = (int)blockIdx.x, u = p.lo.u0 + b, lane = (int)threadIdx.x;
  const int64_t s0 = p.lo.state_off[u] - p.lo.s_base, a0 = p.lo.arc_off[u] - p.lo.a_base;
  const int N = (int)(p.lo.state_off[u + 1] - p.lo.state_off[u]), A = (int)(p.lo.arc_off[u + 1] - p.lo.arc_off[u]);
  const int32_t* abeg = p.lo.in.arc_begin + s0;
  const int32_t* next = p.lo.in.next + a0;
  const int32_t* ol = p.lo.in.olabel + a0;
  const int32_t* ib = p.in_begin + s0 + b;
  const int32_t* in_arc = p.in_arc + a0;
  const int32_t* arc_src = p.arc_src + a0;
  int32_t* so = p.set_off + s0 + b;
  int64_t* ab = p.arc_base + s0;
  int32_t* arena = p.arena + (int64_t)p.hist_factor * s0;
  int32_t* tmp = p.tmp + (int64_t)p.hist_factor * s0;
  const int64_t cap = (int64_t)p.hist_factor * N < (int64_t)INT32_MAX ? (int64_t)p.hist_factor * N : (int64_t)INT32_MAX;
  int st = 0;
  if (N == 0) st = KHG_LAT_NO_PATH;
  else {
    bool bad = false;
    for (int a = lane; a < A; a += LM_NT) bad = bad || next[a] <= arc_src[a];
    if (__ballot(bad)) st = KHG_LAT_EPS_LOOP;
  }
  const int start = N ? p.lo.start[u] : -1;
  int64_t off = 0, abase = 0;
  int maxh = 0;
  if (lane == 0) so[0] = 0;
  __syncthreads();
  for (int d = 0; d < N && st == 0; ++d) {
    int cnt = 0;
    bool oov = false, over = false;
    const int64_t room = cap - off;
    if (d == start) lm_merge_round(tmp, &cnt, room, lane == 0, p.lm.start, lane, &over);
    const int j1 = ib[d + 1];
    for (int jb = ib[d]; jb < j1; jb += LM_NT) {
      // a tile of in-arcs: the word, and where the source's set lies; then the tile's candidates, 64 at a time
      const int j = jb + lane;
      int w = 0, hb = 0;
      long long n = 0;
      if (j < j1) {
        const int a = in_arc[j], s = arc_src[a];
        w = ol[a]; hb = so[s]; n = so[s + 1] - hb;
      }
      long long incl = n;
      for (int o = 1; o < 64; o <<= 1) { const long long t = __shfl_up(incl, o); if (lane >= o) incl += t; }
      const long long tot = __shfl(incl, 63);
      for (long long cb = 0; cb < tot; cb += LM_NT) {
        const bool cv = cb + lane < tot;
        const long long cc = cv ? cb + lane : 0;
        int L = 0;              // the in-arc of candidate cc: the lanes before it hold incl <= cc
        for (int step = 32; step; step >>= 1) { const long long t = __shfl(incl, L + step - 1); if (t <= cc) L += step; }
        const long long first = __shfl(incl, L) - __shfl(n, L);
        const int hbL = __shfl(hb, L), wL = __shfl(w, L);
        int v = -1;
        if (cv) {
          const int h = arena[hbL + (int)(cc - first)];
          float c;
          v = wL == 0 ? h : lm_advance(p.lm, h, wL, &c);
          if (v < 0) oov = true;
        }
        lm_merge_round(tmp, &cnt, room, cv && v >= 0, v, lane, &over);
      }
    }
    if (__ballot(oov)) st = KHG_LAT_LM_OOV;
    else if (over) st = KHG_LAT_SCRATCH;
    else {
      for (int i = lane; i < cnt; i += LM_NT) {       // the ranks of distinct values are the sorted positions
        const int v = tmp[i];
        int r = 0;
        for (int k = 0; k < cnt; ++k) r += tmp[k] < v ? 1 : 0;
        arena[off + r] = v;
      }
      const int deg = (d + 1 < N ? abeg[d + 1] : A) - abeg[d];
      if (lane == 0) { ab[d] = abase; so[d + 1] = (int32_t)(off + cnt); }
      off += cnt;
      abase += (int64_t)cnt * deg;
      maxh = max(maxh, cnt);
    }
    __syncthreads();
  }
  if (lane == 0) {
    const bool ok = st == 0 && N > 0;
    p.lo.status[u] = ok ? KHG_LAT_SUCCEEDED : st;
    p.max_hist[u] = ok ? maxh : 0;
    p.lo.utt_tot[2 * (int64_t)b] = ok ? off : 0;
    p.lo.utt_tot[2 * (int64_t)b + 1] = ok ? abase : 0;
  }
}

// ---- fill: one lane per new state (its number is its set entry's place in the arena); grid (utterance, stripes of new states) ----
__global__ __launch_bounds__(LM_NT) void k2_lattice_lm_fill(LmArgs p) {
#pragma clang fp contract(off)
  const int b = (int)blockIdx.x, u = p.lo.u0 + b;
  const int64_t s0 = p.lo.state_off[u] - p.lo.s_base, a0 = p.lo.arc_off[u] - p.lo.a_base;
  const int N = (int)(p.lo.state_off[u + 1] - p.lo.state_off[u]), A = (int)(p.lo.arc_off[u + 1] - p.lo.arc_off[u]);
  const int64_t so_out = p.lo.utt_off[b], ao_out = p.lo.utt_off[(int64_t)p.lo.n + 1 + b];
  const int NS = (int)(p.lo.utt_off[b + 1] - so_out);
  const int32_t* so = p.set_off + s0 + b;
  if (blockIdx.y == 0 && threadIdx.x == 0) p.lo.o_start[u] = NS > 0 ? so[p.lo.start[u]] : -1;
  if (NS == 0) return;
  const float INF = __builtin_huge_valf();
  const int32_t* abeg = p.lo.in.arc_begin + s0;
  const int32_t* arena = p.arena + (int64_t)p.hist_factor * s0;
  for (int r = (int)blockIdx.y * LM_NT + (int)threadIdx.x; r < NS; r += (int)gridDim.y * LM_NT) {
    int s = 0, hi = N;          // the old state: the last s with so[s] <= r (so[0] = 0, so[N] = NS)
    while (hi - s > 1) {
      const int mid = (s + hi) >> 1;
      if (so[mid] <= r) s = mid; else hi = mid;
    }
    const int h = arena[r];
    const int64_t sid = so_out + r;
    p.lo.out.frame[sid] = p.lo.in.frame[s0 + s]; p.lo.out.gstate[sid] = p.lo.in.gstate[s0 + s];
    p.lo.out.tot[sid] = p.lo.in.tot[s0 + s]; p.lo.out.extra[sid] = p.lo.in.extra[s0 + s];
    const float f = p.lo.in.fin[s0 + s];
    float fo = INF;
    if (f != INF) { const float t = p.scale * p.lm.fin[h]; fo = f + t; }
    p.lo.out.fin[sid] = fo;
    const int alo = abeg[s], ahi = s + 1 < N ? abeg[s + 1] : A;
    int64_t pos = p.arc_base[s0 + s] + (int64_t)(r - so[s]) * (ahi - alo);
    p.lo.out.arc_begin[sid] = (int32_t)pos;
    pos += ao_out;
    for (int a = alo; a < ahi; ++a, ++pos) {
      const int d = p.lo.in.next[a0 + a], w = p.lo.in.olabel[a0 + a];
      float g = p.lo.in.g[a0 + a];
      int hh = h;
      if (w != 0) {
        float c;
        hh = lm_advance(p.lm, h, w, &c);
        const float t = p.scale * c;
        g = g + t;
      }
      int lo = so[d], hi2 = so[d + 1];          // hh is in H(d): the mark put it there
      while (lo < hi2) {
        const int mid = (lo + hi2) >> 1;
        if (arena[mid] < hh) lo = mid + 1; else hi2 = mid;
      }
      p.lo.out.ilabel[pos] = p.lo.in.ilabel[a0 + a]; p.lo.out.olabel[pos] = w;
      p.lo.out.g[pos] = g; p.lo.out.ac[pos] = p.lo.in.ac[a0 + a];
      p.lo.out.next[pos] = lo;
    }
  }
}
