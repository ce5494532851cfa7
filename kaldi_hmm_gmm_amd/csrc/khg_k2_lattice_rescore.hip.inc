// K2X (khg_lattices_rescore, khg_lattices_boost; DESIGN.md 7j): the per-arc kernels over a chunk of resident lattices.  One thread per
// arc finds its utterance (the last one whose first arc is not behind it) and its source state (the last state of that utterance whose
// arc_begin is not behind it) by binary search; the state's frame and the arc's transition-id name the (frame, pdf) cell.
//   k2x_flatten     CELLS mode: key = (pdf << 32) | feature row, val = the arc's number, for khg_k1_cells.hip.inc
//   k2x_ll_check    FROM_LL mode: flags the utterances with an arc whose pdf is not on their pdf list
//   k2x_ll_gather   FROM_LL mode: acoustic_cost = -(scale * ll[j * tpad + t]), in place
//   k2x_ali_check   boost: flags the utterances whose alignment holds an id outside 1 .. num_tids
//   k2x_label_check boost: raises a word when an arc's ilabel is outside 0 .. num_tids
//   k2x_boost       boost: graph_cost = fl(graph_cost + fl(-b * e)), in place
// No atomics but the error word's: a flag is a plain store of 1.

constexpr int K2X_NT = 256;
struct K2xChunk {
  LatArrays io;                     // the chunk's arrays (read; k2x_ll_gather writes ac, k2x_boost writes g)
  const int64_t *state_off, *arc_off;   // the handle's [U + 1], on the device
  int64_t s_base, a_base, na;       // the chunk's first state / arc in the handle's order, its arcs
  int32_t u0, n;
};
// chunk-local arc a -> its utterance (handle-wide number) and the frame of its source state
__device__ __forceinline__ void k2x_where(const K2xChunk& c, int64_t a, int32_t* utt, int32_t* frame) {
  const int64_t ga = c.a_base + a;
  int lo = 0, hi = c.n;                          // arc_off[u0 + lo] <= ga < arc_off[u0 + hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (c.arc_off[c.u0 + mid] <= ga) lo = mid; else hi = mid;
  }
  const int u = c.u0 + lo;
  const int32_t al = (int32_t)(ga - c.arc_off[u]);
  const int64_t s0 = c.state_off[u] - c.s_base;
  int32_t slo = 0, shi = (int32_t)(c.state_off[u + 1] - c.state_off[u]);      // arc_begin[slo] <= al < arc_begin[shi] (the end: all arcs)
  while (shi - slo > 1) {
    const int32_t mid = (slo + shi) >> 1;
    if (c.io.arc_begin[s0 + mid] <= al) slo = mid; else shi = mid;
  }
  *utt = u; *frame = c.io.frame[s0 + slo];
}

struct K2xFlat {
  K2xChunk c;
  const int64_t* set_frame_off;     // the utterance set's [U + 1]
  const int32_t* id2pdf; int32_t num_tids, P;
  uint64_t* keys; uint32_t* vals;   // at the handle's first arc
  int32_t* err_flag;
};
__global__ __launch_bounds__(K2X_NT) void k2x_flatten(K2xFlat p) {
  const int64_t stride = (int64_t)gridDim.x * K2X_NT;
  for (int64_t a = (int64_t)blockIdx.x * K2X_NT + threadIdx.x; a < p.c.na; a += stride) {
    const int32_t il = p.c.io.ilabel[a];
    uint64_t key = (uint64_t)p.P << 32;          // past every pdf: an epsilon arc
    if (il != 0) {
      if (il < 1 || il > p.num_tids) atomicOr(p.err_flag, 4);
      else {
        int32_t u, t;
        k2x_where(p.c, a, &u, &t);
        const int32_t pdf = p.id2pdf[il];
        if (pdf < 0 || pdf >= p.P) atomicOr(p.err_flag, 4);
        else key = ((uint64_t)pdf << 32) | (uint64_t)(uint32_t)(p.set_frame_off[u] + t);
      }
    }
    p.keys[p.c.a_base + a] = key; p.vals[p.c.a_base + a] = (uint32_t)(p.c.a_base + a);
  }
}

struct K2xLl {
  K2xChunk c;
  const int64_t *set_frame_off, *pdf_off, *ll_off;      // the set's [U + 1]
  const int32_t* pdfs; const float* ll;
  const int32_t* id2pdf; int32_t num_tids;
  float scale;
  int32_t* flag;                    // [U]
  int32_t* err_flag;
};
// the index of `pdf` in utterance u's sorted list, -1 when it is not there
__device__ __forceinline__ int32_t k2x_pdf_index(const K2xLl& p, int32_t u, int32_t pdf) {
  int64_t lo = p.pdf_off[u], hi = p.pdf_off[u + 1];
  const int64_t base = lo;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (p.pdfs[mid] < pdf) lo = mid + 1; else hi = mid;
  }
  return (lo < p.pdf_off[u + 1] && p.pdfs[lo] == pdf) ? (int32_t)(lo - base) : -1;
}
template <bool GATHER>
__global__ __launch_bounds__(K2X_NT) void k2x_ll(K2xLl p) {
  const int64_t stride = (int64_t)gridDim.x * K2X_NT;
  for (int64_t a = (int64_t)blockIdx.x * K2X_NT + threadIdx.x; a < p.c.na; a += stride) {
    const int32_t il = p.c.io.ilabel[a];
    if (il == 0) continue;
    if (il < 1 || il > p.num_tids) { if (!GATHER) atomicOr(p.err_flag, 4); continue; }
    int32_t u, t;
    k2x_where(p.c, a, &u, &t);
    const int32_t j = k2x_pdf_index(p, u, p.id2pdf[il]);
    if (!GATHER) {
      if (j < 0) p.flag[u] = 1;
      continue;
    }
    if (j < 0) continue;                         // (cannot be: such an utterance was left empty)
    const int64_t T = p.set_frame_off[u + 1] - p.set_frame_off[u], tpad = (T + 31) & ~int64_t(31);
    p.c.io.ac[a] = -__fmul_rn(p.scale, p.ll[p.ll_off[u] + (int64_t)j * tpad + t]);
  }
}

// one workgroup per utterance: flag[u] = 1 when its alignment holds an id outside 1 .. num_tids
__global__ __launch_bounds__(K2X_NT) void k2x_ali_check(const int32_t* __restrict__ ali, const int64_t* __restrict__ ali_off, int32_t num_tids, int32_t* __restrict__ flag) {
  const int u = (int)blockIdx.x;
  for (int64_t i = ali_off[u] + threadIdx.x; i < ali_off[u + 1]; i += K2X_NT)
    if (ali[i] < 1 || ali[i] > num_tids) flag[u] = 1;
}
__global__ __launch_bounds__(K2X_NT) void k2x_label_check(K2xChunk c, int32_t num_tids, int32_t* __restrict__ bad) {
  const int64_t stride = (int64_t)gridDim.x * K2X_NT;
  for (int64_t a = (int64_t)blockIdx.x * K2X_NT + threadIdx.x; a < c.na; a += stride)
    if (c.io.ilabel[a] < 0 || c.io.ilabel[a] > num_tids) *bad = 1;
}
struct K2xBoost {
  K2xChunk c;
  const int32_t* ali; const int64_t* ali_off;    // [U + 1]: utterance u's alignment, one id per frame
  const int32_t* tab;               // [num_tids + 1]: 2 * phone + (the phone is a silence phone)
  float neg_b, max_sil_err;
};
__global__ __launch_bounds__(K2X_NT) void k2x_boost(K2xBoost p) {
  const int64_t stride = (int64_t)gridDim.x * K2X_NT;
  for (int64_t a = (int64_t)blockIdx.x * K2X_NT + threadIdx.x; a < p.c.na; a += stride) {
    const int32_t il = p.c.io.ilabel[a];
    if (il == 0) continue;
    int32_t u, t;
    k2x_where(p.c, a, &u, &t);
    const int32_t mine = p.tab[il], ref = p.tab[p.ali[p.ali_off[u] + t]];
    const float e = (mine >> 1) == (ref >> 1) ? 0.0f : (mine & 1) ? p.max_sil_err : 1.0f;
    p.c.io.g[a] = __fadd_rn(p.c.io.g[a], __fmul_rn(p.neg_b, e));
  }
}
