// kaldi_hmm_gmm_amd/csrc/khg_tree_stats.hip.inc -- kernels of acc-tree-stats (DESIGN.md 7o): phone segments of the resident alignment,
// one 64-bit event key per frame, the distinct keys of the sorted list, the fixed-order gather sums and the key-union merge.
// Included by khg_tree.hip only.  No atomics anywhere: every sum is formed by one thread in a written order.

// per transition-id: phone | pdf-class << 16 | flags << 24
constexpr uint32_t TR_SELF = 1u << 24, TR_FINAL = 1u << 25, TR_CI = 1u << 26;
constexpr int TR_SLICE = 1024;          // entries of one work item of the gather
constexpr int TR_BAD_ALI = 1, TR_BAD_PHONE = 2, TR_BAD_END = 4;

struct TrArgs {
  const int32_t* ali; const int64_t* frame_off; int32_t n_utt;
  const uint32_t* tidinfo; int32_t num_tids;
  int32_t N, P, bp, bc;                 // context; bits of a phone / of a pdf-class in the sort key
  int32_t *tmp, *seg_start, *seg_end;   // [frames]
  int32_t* status;                      // [n_utt]
  uint64_t* keys; uint32_t* vals;       // [frames]
};
struct TrItem { int32_t key, e0, n, slot; };     // slot < 0: the key's only slice, written to the call's sums directly
struct TrRun { int32_t key, slot0, nslot, pad; };

__device__ __forceinline__ uint32_t tr_info(const TrArgs& a, int32_t tid) { return (tid >= 1 && tid <= a.num_tids) ? a.tidinfo[tid] : 0u; }

// inclusive max-scan over the 256 threads of the block; *total = the block's maximum.  Every thread calls it.
__device__ inline int tr_scan_max(int v, int* sh, int* total) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const int o = t >= off ? sh[t - off] : INT_MIN;
    __syncthreads();
    v = max(v, o);
    sh[t] = v;
    __syncthreads();
  }
  *total = sh[255];
  __syncthreads();
  return v;
}

// One utterance per block (blockIdx.x strides).  seg_start[f]: first frame of f's phone segment; seg_end[f]: first frame of the next
// segment, or the utterance's end.  A segment begins at the utterance's first frame and at every non-self-loop id whose nearest
// preceding non-self-loop id is final (SplitToPhones for reordered graphs).  status[u]: TR_BAD_* bits, 0 = the utterance counts.
__global__ __launch_bounds__(256) void k_tree_segments(TrArgs a) {
  __shared__ int sh[256];
  const int t = threadIdx.x;
  for (int u = blockIdx.x; u < a.n_utt; u += gridDim.x) {
    const int f0 = (int)a.frame_off[u], f1 = (int)a.frame_off[u + 1];
    int bad_ali = 0, bad_phone = 0, total;
    // A: tmp[f] = last non-self-loop frame <= f (-1: none)
    int carry = -1;
    for (int c0 = f0; c0 < f1; c0 += 256) {
      const int f = c0 + t;
      int v = -1;
      if (f < f1) {
        const int32_t id = a.ali[f];
        if (id < 1 || id > a.num_tids) bad_ali = 1;
        else if (!(a.tidinfo[id] & TR_SELF)) v = f;
      }
      v = max(tr_scan_max(v, sh, &total), carry);
      if (f < f1) a.tmp[f] = v;
      carry = max(carry, total);
    }
    __syncthreads();
    const int last_nsl = f1 > f0 ? a.tmp[f1 - 1] : -1;
    const int bad_end = (f1 > f0 && (last_nsl < 0 || !(tr_info(a, a.ali[last_nsl]) & TR_FINAL))) ? 1 : 0;
    // B: seg_start[f] = last segment boundary <= f
    carry = f0;
    for (int c0 = f0; c0 < f1; c0 += 256) {
      const int f = c0 + t;
      int v = -1;
      if (f == f0) v = f;
      else if (f < f1 && !(tr_info(a, a.ali[f]) & TR_SELF)) {
        const int p = a.tmp[f - 1];
        if (p >= 0 && (tr_info(a, a.ali[p]) & TR_FINAL)) v = f;
      }
      v = max(tr_scan_max(v, sh, &total), carry);
      if (f < f1) a.seg_start[f] = v;
      carry = max(carry, total);
    }
    __syncthreads();
    // C (backwards): tmp[f] = first segment boundary >= f (f1: none); thread t takes frame c1 - 1 - t, so the max-scan of -f runs towards lower frames
    carry = -f1;
    for (int c1 = f1; c1 > f0; c1 -= 256) {
      const int f = c1 - 1 - t;
      int v = INT_MIN;
      if (f >= f0 && a.seg_start[f] == f) v = -f;
      v = max(tr_scan_max(v, sh, &total), carry);
      if (f >= f0) a.tmp[f] = -v;
      carry = max(carry, total);
    }
    __syncthreads();
    // D: seg_end, and one phone per segment
    for (int f = f0 + t; f < f1; f += 256) {
      a.seg_end[f] = f + 1 < f1 ? a.tmp[f + 1] : f1;
      if ((tr_info(a, a.ali[f]) & 0xFFFFu) != (tr_info(a, a.ali[a.seg_start[f]]) & 0xFFFFu)) bad_phone = 1;
    }
    bad_ali = __syncthreads_or(bad_ali);
    bad_phone = __syncthreads_or(bad_phone);
    if (t == 0) a.status[u] = bad_ali ? TR_BAD_ALI : ((bad_phone ? TR_BAD_PHONE : 0) | (bad_end ? TR_BAD_END : 0));   // without ids there are no segments to judge
    __syncthreads();
  }
}

// The event of every frame as one key: window[0] .. window[N - 1] (bp bits each), then the pdf-class (bc bits) -- ascending keys are
// ascending (window, pdf-class) tuples.  Frames of a skipped utterance get the sentinel 1 << (N bp + bc), which sorts last.
__global__ __launch_bounds__(256) void k_tree_keys(TrArgs a) {
  const uint64_t sentinel = uint64_t(1) << (a.N * a.bp + a.bc);
  for (int u = blockIdx.x; u < a.n_utt; u += gridDim.x) {
    const int f0 = (int)a.frame_off[u], f1 = (int)a.frame_off[u + 1];
    const bool skip = a.status[u] != 0;
    for (int f = f0 + threadIdx.x; f < f1; f += 256) {
      a.vals[f] = (uint32_t)f;
      if (skip) { a.keys[f] = sentinel; continue; }
      const uint32_t own = a.tidinfo[a.ali[f]];
      const int s = a.seg_start[f], e = a.seg_end[f];
      const uint32_t cur = a.tidinfo[a.ali[s]];
      uint32_t ph[5] = {0, 0, cur & 0xFFFFu, 0, 0};     // segments i - 2 .. i + 2; 0 outside the utterance
      if (!(cur & TR_CI)) {
        if (s > f0) {
          const int s1 = a.seg_start[s - 1];
          ph[1] = a.tidinfo[a.ali[s1]] & 0xFFFFu;
          if (s1 > f0) ph[0] = a.tidinfo[a.ali[a.seg_start[s1 - 1]]] & 0xFFFFu;
        }
        if (e < f1) {
          ph[3] = a.tidinfo[a.ali[e]] & 0xFFFFu;
          const int e2 = a.seg_end[e];
          if (e2 < f1) ph[4] = a.tidinfo[a.ali[e2]] & 0xFFFFu;
        }
      }
      uint64_t k = 0;
      for (int j = 0; j < a.N; ++j) k = (k << a.bp) | ph[2 - a.P + j];
      a.keys[f] = (k << a.bc) | ((own >> 16) & 0xFFu);
    }
  }
}

__global__ __launch_bounds__(256) void k_tree_iota(uint32_t* v, int64_t n) {
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) v[i] = (uint32_t)i;
}

// head[i] = 1 where a new key begins in the sorted list (sentinels never do)
__global__ __launch_bounds__(256) void k_tree_heads(const uint64_t* __restrict__ keys, int64_t n, uint64_t sentinel, int32_t* __restrict__ head) {
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const uint64_t k = keys[i];
    head[i] = (k != sentinel && (i == 0 || keys[i - 1] != k)) ? 1 : 0;
  }
}

// inc: the inclusive scan of head.  kstart[j] = first sorted entry of distinct key j, kstart[K] = the end of the last; kkey[j] = that
// key in the handle's layout (16 bits a phone, 8 bits the pdf-class)
__global__ __launch_bounds__(256) void k_tree_starts(const uint64_t* __restrict__ keys, const int32_t* __restrict__ head, const int32_t* __restrict__ inc, int64_t n,
                                                     uint64_t sentinel, int32_t N, int32_t bp, int32_t bc, int32_t* __restrict__ kstart, uint64_t* __restrict__ kkey) {
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const uint64_t k = keys[i];
    if (k == sentinel) continue;
    if (head[i]) {
      const int o = inc[i] - 1;
      kstart[o] = (int32_t)i;
      uint64_t c = 0;
      for (int j = 0; j < N; ++j) c = (c << 16) | ((k >> (bc + bp * (N - 1 - j))) & ((uint64_t(1) << bp) - 1));
      kkey[o] = (c << 8) | (k & ((uint64_t(1) << bc) - 1));
    }
    if (i + 1 == n || keys[i + 1] == sentinel) kstart[inc[i]] = (int32_t)(i + 1);
  }
}

// The gather: one work item = <= TR_SLICE consecutive entries of one key's list.  dim <= 256: thread = (row lane r = tid / dim, element
// d = tid % dim), R = 256 / dim row lanes; lane r adds entries r, r + R, r + 2 R, .. of the slice in that order, then element d's R
// chains are added in lane order 0 .. R - 1.  dim > 256: one chain per element over the slice.  fp32 rows widened to fp64: v * v is
// exact, so each term costs one rounding (of the add).  The rows of four entries are in flight per lane.
__global__ __launch_bounds__(256) void k_tree_sum(const TrItem* __restrict__ items, const uint32_t* __restrict__ vals, const float* __restrict__ feats, int32_t D,
                                                  double* __restrict__ part, double* __restrict__ cx, double* __restrict__ cx2) {
  __shared__ double shx[256], shx2[256];
  const TrItem it = items[blockIdx.x];
  const uint32_t* v = vals + it.e0;
  double* ox = it.slot < 0 ? cx + (int64_t)it.key * D : part + (int64_t)it.slot * 2 * D;
  double* ox2 = it.slot < 0 ? cx2 + (int64_t)it.key * D : part + (int64_t)it.slot * 2 * D + D;
  if (D <= 256) {
    const int R = 256 / D, r = threadIdx.x / D, d = threadIdx.x % D;
    double sx = 0.0, sx2 = 0.0;
    if (r < R) {
      int j = r;
      for (; j + 3 * R < it.n; j += 4 * R) {
        const float x0 = feats[(int64_t)v[j] * D + d], x1 = feats[(int64_t)v[j + R] * D + d];
        const float x2 = feats[(int64_t)v[j + 2 * R] * D + d], x3 = feats[(int64_t)v[j + 3 * R] * D + d];
        sx += (double)x0; sx2 += (double)x0 * (double)x0;
        sx += (double)x1; sx2 += (double)x1 * (double)x1;
        sx += (double)x2; sx2 += (double)x2 * (double)x2;
        sx += (double)x3; sx2 += (double)x3 * (double)x3;
      }
      for (; j < it.n; j += R) {
        const float x0 = feats[(int64_t)v[j] * D + d];
        sx += (double)x0; sx2 += (double)x0 * (double)x0;
      }
    }
    shx[threadIdx.x] = sx; shx2[threadIdx.x] = sx2;
    __syncthreads();
    if (r == 0) {
      for (int q = 1; q < R; ++q) { sx += shx[q * D + d]; sx2 += shx2[q * D + d]; }
      ox[d] = sx; ox2[d] = sx2;
    }
  } else {
    for (int d = threadIdx.x; d < D; d += 256) {
      double sx = 0.0, sx2 = 0.0;
      for (int j = 0; j < it.n; ++j) {
        const float x0 = feats[(int64_t)v[j] * D + d];
        sx += (double)x0; sx2 += (double)x0 * (double)x0;
      }
      ox[d] = sx; ox2[d] = sx2;
    }
  }
}

// The same sums for keys of at most R = 256 / dim entries (dim <= 256), 256 / dim keys a workgroup: thread = (key of the group,
// element d).  With n <= R every chain of k_tree_sum holds one entry or none, so its result is 0 + x_0 + x_1 + .. + x_(n-1) in entry
// order (an empty chain adds +0, which changes no bit of a sum that began at +0): that sum is formed here by one thread, and the
// inventories of many short keys (uniform triphones: a median of 3 entries) no longer cost a workgroup a key.
__global__ __launch_bounds__(256) void k_tree_sum_short(const TrItem* __restrict__ items, int32_t nitems, const uint32_t* __restrict__ vals,
                                                        const float* __restrict__ feats, int32_t D, double* __restrict__ cx, double* __restrict__ cx2) {
  const int per = 256 / D, g = threadIdx.x / D, d = threadIdx.x % D;
  const int64_t i = (int64_t)blockIdx.x * per + g;
  if (g >= per || i >= nitems) return;
  const TrItem it = items[i];
  const uint32_t* v = vals + it.e0;
  double sx = 0.0, sx2 = 0.0;
  for (int j = 0; j < it.n; ++j) {
    const float x0 = feats[(int64_t)v[j] * D + d];
    sx += (double)x0; sx2 += (double)x0 * (double)x0;
  }
  cx[(int64_t)it.key * D + d] = sx;
  cx2[(int64_t)it.key * D + d] = sx2;
}

// the slices of a long key, added in slice order
__global__ __launch_bounds__(256) void k_tree_reduce(const TrRun* __restrict__ runs, int32_t nruns, const double* __restrict__ part, int32_t D, double* __restrict__ cx,
                                                     double* __restrict__ cx2) {
  const int64_t n = (int64_t)nruns * 2 * D;
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const TrRun r = runs[i / (2 * D)];
    const int c = (int)(i % (2 * D));
    double s = part[(int64_t)r.slot0 * 2 * D + c];
    for (int q = 1; q < r.nslot; ++q) s += part[(int64_t)(r.slot0 + q) * 2 * D + c];
    (c < D ? cx : cx2)[(int64_t)r.key * D + (c < D ? c : c - D)] = s;
  }
}
__global__ __launch_bounds__(256) void k_tree_counts(const int32_t* __restrict__ kstart, int32_t K, double* __restrict__ cnt) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < K; i += gridDim.x * 256) cnt[i] = (double)(kstart[i + 1] - kstart[i]);
}

// Key-union merge.  The sorted list holds the keys of a (sources 0 .. Ka - 1) and of b (Ka ..), a's first among equals (stable sort).
// Every distinct key gets a, scale b or a + scale b: one product and one add, never fused.  Columns: count | x[D] | x2[D].
struct TrSide { const double *cnt, *x, *x2; };
__device__ __forceinline__ double tr_col(const TrSide& s, int64_t row, int c, int D) {
  return c == 0 ? s.cnt[row] : (c <= D ? s.x[row * D + (c - 1)] : s.x2[row * D + (c - 1 - D)]);
}
__global__ __launch_bounds__(256) void k_tree_merge(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ src, const int32_t* __restrict__ head,
                                                    const int32_t* __restrict__ inc, int64_t M, int32_t Ka, TrSide A, TrSide B, double scale, int32_t D,
                                                    uint64_t* __restrict__ okey, double* __restrict__ ocnt, double* __restrict__ ox, double* __restrict__ ox2) {
  const int W = 2 * D + 1;
  const int64_t n = M * W;
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t e = i / W;
    const int c = (int)(i % W);
    if (!head[e]) continue;
    const int64_t o = inc[e] - 1;
    const uint32_t s1 = src[e];
    double v = s1 < (uint32_t)Ka ? tr_col(A, s1, c, D) : __dmul_rn(scale, tr_col(B, (int64_t)s1 - Ka, c, D));
    if (e + 1 < M && keys[e + 1] == keys[e]) v = __dadd_rn(v, __dmul_rn(scale, tr_col(B, (int64_t)src[e + 1] - Ka, c, D)));
    if (c == 0) { ocnt[o] = v; okey[o] = keys[e]; }
    else if (c <= D) ox[o * D + (c - 1)] = v;
    else ox2[o * D + (c - 1 - D)] = v;
  }
}
