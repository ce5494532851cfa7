// LDA statistics on spliced features (khg_acc_lda_stats_post, DESIGN.md 7n): Kaldi's LdaEstimate accumulators from posteriors resident on
// the device.  The spliced matrix z_t[k D + j] = x[clamp(t + k - L, 0, T - 1)][j] is never written to HBM: every kernel forms z by index
// arithmetic on the set's own rows.
//
// Pipeline per call: posteriors_flatten (khg_lattices.hip) -> e_row / e_tid / e_w [E] in utterance, frame, entry order ->
//   k_lda_rowutt   the first and last feature row of every row's utterance (the clamp's bounds)
//   k_lda_roww     W_t of every feature row: the double sum of the row's weights in entry order
//   k_lda_keys     (pdf, entry) pairs of ALL the call's entries; an entry that adds nothing gets key C -> stable radix sort (K3's path)
//   k_lda_bounds   the first sorted entry of every class (one word per class comes down: the slice plan is made on the host)
//   k_lda_class    one workgroup per slice of <= 1024 sorted entries of ONE class: one chain per element of [w | w z], in sorted order
//   k_lda_creduce  the slices of a class added in slice order onto the call's sums
//   per chunk of 1024-frame slices of the call's frame list: k_lda_posrow, k_lda_gram (the second-order sum of one slice on the fp64
//   matrix pipe, lower-triangle tiles only, parked per slice), k_lda_reduce (the slices added in slice order)
//   k_lda_axpy     the call's sums into the handle
// No atomics on any value.  The handle's block of doubles: zero_acc[C] | first_acc[C][Dz] | total_second_acc (Kaldi's packed lower
// triangle: (i, j <= i) at i (i + 1) / 2 + j).

constexpr int LD_SLICE = 1024;     // frames of one Gram work item / sorted entries of one class work item
constexpr int LD_TB = 64;          // frames staged in LDS at a time
constexpr int LD_CT = 8;           // column tiles a wave keeps accumulators for
constexpr int LD_CG = (KHG_LDA_MAX_SPLICED_DIM + 15) / 16 * 16 / 64 + 1;   // 64-lane column groups of a staged row of (16 tile rows) | 1 floats

struct LdSeg { int32_t row0, n, pos0, pad; };            // n feature rows from row0 sit at compact positions pos0 .. of their chunk
struct LdItem { int32_t pos0, n, slot, pad; };           // one slice: positions [pos0, pos0 + n) of its chunk, parked in slot `slot`
struct LdUnit { int32_t ti, tj0, ntj, pad; };            // one wave's share of the triangle: tile row ti, column tiles tj0 .. tj0 + ntj - 1 (<= ti)
struct LdCItem { int32_t cls, e0, n, slot; };            // one class slice: sorted entries [e0, e0 + n), parked in slot `slot` of its chunk
struct LdCRun { int32_t cls, slot0, nslot, pad; };       // the slices of one class inside one chunk

struct LdArgs {
  const float* feats; int32_t D, L, R, Dz, C; int64_t N;
  const int64_t* frame_off; int32_t n_utt;
  const int32_t* id2pdf; int32_t num_tids;
  const int32_t *e_row, *e_tid; const float* e_w; int64_t E;
  int32_t *row_lo, *row_hi;         // [N] first / last feature row of the row's utterance
  double* row_w;                    // [N] W_t
  int32_t* pos_row;                 // chunk scratch: compact position -> feature row
  double* part;                     // parked slice images
  int32_t* err_flag;
};

// blockIdx.x strides over the utterances
__global__ __launch_bounds__(256) void k_lda_rowutt(LdArgs p) {
  for (int u = blockIdx.x; u < p.n_utt; u += gridDim.x) {
    const int64_t f0 = p.frame_off[u], f1 = p.frame_off[u + 1];
    for (int64_t r = f0 + threadIdx.x; r < f1; r += 256) { p.row_lo[r] = (int32_t)f0; p.row_hi[r] = (int32_t)(f1 - 1); }
  }
}

// the class of an entry, or -1 when it adds nothing (dropped by the flatten pass, weight +-0, a pdf outside the handle's classes)
__device__ __forceinline__ int ld_entry_class(const LdArgs& p, int64_t i) {
  const int tid = p.e_tid[i];
  if (tid < 1 || tid > p.num_tids || p.e_w[i] == 0.0f) return -1;
  const int c = p.id2pdf[tid];
  if (c < 0 || c >= p.C) { atomicOr(p.err_flag, 4); return -1; }
  return c;
}

// W_t: the thread of a row's first entry walks the row's entries (rows ascend with the entries: posteriors_flatten's order); row_w was zeroed
__global__ __launch_bounds__(256) void k_lda_roww(LdArgs p) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < p.E; i += stride) {
    const int32_t r = p.e_row[i];
    if (r < 0 || (int64_t)r >= p.N) continue;
    if (i > 0 && p.e_row[i - 1] == r) continue;
    double w = 0.0;
    for (int64_t k = i; k < p.E && p.e_row[k] == r; ++k)
      if (ld_entry_class(p, k) >= 0) w += (double)p.e_w[k];
    p.row_w[r] = w;
  }
}

__global__ __launch_bounds__(256) void k_lda_keys(LdArgs p, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < p.E; i += stride) {
    int c = -1;
    const int32_t r = p.e_row[i];
    if (r >= 0 && (int64_t)r < p.N) c = ld_entry_class(p, i);
    keys[i] = (uint32_t)(c < 0 ? p.C : c);
    vals[i] = (uint32_t)i;
  }
}

// cstart[c], c = 0 .. C: the first sorted entry whose key is >= c (cstart[C]: the entries that count)
__global__ __launch_bounds__(256) void k_lda_bounds(const uint32_t* __restrict__ skeys, int64_t E, int32_t C, int32_t* __restrict__ cstart) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c > C) return;
  int64_t lo = 0, hi = E;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (skeys[mid] < (uint32_t)c) lo = mid + 1; else hi = mid;
  }
  cstart[c] = (int32_t)lo;
}

// One class slice: thread e (+ 256, ...) owns element e of [w | w z[0 .. Dz)] and adds the slice's entries in sorted order, each term
// (double)w * (double)z -- the product of two floats, exact -- with one rounding in the add.  The entries' rows, clamp bounds and
// weights are staged in LDS once.  Parked: slot x (Dz + 1) doubles.
__global__ __launch_bounds__(256) void k_lda_class(LdArgs p, const LdCItem* __restrict__ items, const uint32_t* __restrict__ svals) {
  __shared__ int32_t s_row[LD_SLICE], s_lo[LD_SLICE], s_hi[LD_SLICE];
  __shared__ float s_w[LD_SLICE];
  const LdCItem it = items[blockIdx.x];
  const int tid = threadIdx.x;
  for (int e = tid; e < it.n; e += 256) {
    const int64_t i = svals[(int64_t)it.e0 + e];
    const int32_t r = p.e_row[i];
    s_row[e] = r; s_lo[e] = p.row_lo[r]; s_hi[e] = p.row_hi[r]; s_w[e] = p.e_w[i];
  }
  __syncthreads();
  const int D = p.D, L = p.L, Dz = p.Dz;
  double* dst = p.part + (int64_t)it.slot * (Dz + 1);
  for (int el = tid; el <= Dz; el += 256) {
    double acc = 0.0;
    if (el == 0) {
      for (int e = 0; e < it.n; ++e) acc += (double)s_w[e];
    } else {
      const int k = (el - 1) / D, j = (el - 1) - k * D;
      for (int e = 0; e < it.n; ++e) {
        const int r = min(max(s_row[e] + k - L, s_lo[e]), s_hi[e]);
        acc += (double)s_w[e] * (double)p.feats[(int64_t)r * D + j];
      }
    }
    dst[el] = acc;
  }
}

// call[zero_acc | first_acc] += the parked slices of a class, in slice order
__global__ __launch_bounds__(256) void k_lda_creduce(const LdCRun* __restrict__ runs, const double* __restrict__ part, double* __restrict__ call,
                                                     int32_t C, int32_t Dz) {
  const LdCRun r = runs[blockIdx.x];
  for (int el = threadIdx.x; el <= Dz; el += 256) {
    double* d = el == 0 ? call + r.cls : call + C + (int64_t)r.cls * Dz + (el - 1);
    double v = *d;
    for (int k = 0; k < r.nslot; ++k) v += part[(int64_t)(r.slot0 + k) * (Dz + 1) + el];
    *d = v;
  }
}

__global__ __launch_bounds__(256) void k_lda_posrow(const LdSeg* __restrict__ segs, int32_t nseg, int32_t* __restrict__ pos_row) {
  for (int s = blockIdx.x; s < nseg; s += gridDim.x) {
    const LdSeg g = segs[s];
    for (int i = threadIdx.x; i < g.n; i += 256) pos_row[g.pos0 + i] = g.row0 + i;
  }
}

// The second-order kernel: S[i][j] = sum_t (W_t z_t[i]) z_t[j], j <= i, over the frames of one slice on v_mfma_f64_16x16x4_f64.
// blockIdx.x: the slice; blockIdx.y: four units of the triangle, one per wave.  A wave owns tile row ti and up to LD_CT column tiles of
// it: per four frames it forms a = W_t z_t[i] ONCE (one rounding in double) and feeds it to every column tile it keeps accumulators
// for -- on this chip an fp64 MFMA holds the SIMD's issue for its 64 cycles (khg_fmllr_stats.hip.inc), so nothing is formed twice and
// nothing hides.  Operand maps of the instruction (7l): A[row = lane & 15][k = lane >> 4], B[k = lane >> 4][col = lane & 15], C/D
// col = lane & 15, row = (lane >> 4) + 4 reg.  The sum over t runs in frame order, four frames per instruction: fixed by the slice.
// The LD_TB spliced rows of a block are staged in LDS (a block of a slice may straddle utterances, each with its own clamp: the spliced
// form keeps every index out of the inner loop).  Dynamic LDS: ws[LD_TB] doubles | zs[LD_TB][ZS] floats, ZS = (16 tile rows) | 1;
// columns >= Dz and rows >= the block's frames are zero.
typedef double ld_f64x4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void k_lda_gram(LdArgs p, const LdItem* __restrict__ items, const LdUnit* __restrict__ units, int32_t nunits, int32_t ZS,
                                                  int64_t SZ2) {
  extern __shared__ __attribute__((aligned(16))) double ld_lds[];
  double* ws = ld_lds;
  float* zs = reinterpret_cast<float*>(ld_lds + LD_TB);
  const LdItem it = items[blockIdx.x];
  const int D = p.D, L = p.L, Dz = p.Dz;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j16 = lane & 15, q = lane >> 4;
  const int un = blockIdx.y * 4 + ((wave + blockIdx.x) & 3);  // rotated by the slice: the widest unit does not always land on the same SIMD
  const bool live = un < nunits;                              // wave-uniform
  LdUnit u{0, 0, 0, 0};
  if (live) u = units[un];
  const int ntj = __builtin_amdgcn_readfirstlane(u.ntj);
  // this lane's columns lane + 64 m of a staged row: which neighbour k and which element j of it (k = -1: a padding column), once
  int ck[LD_CG], cj[LD_CG];
#pragma unroll
  for (int m = 0; m < LD_CG; ++m) {
    const int c = lane + 64 * m;
    ck[m] = -1; cj[m] = 0;
    if (c < Dz) { ck[m] = c / D; cj[m] = c - ck[m] * D; }
  }
  ld_f64x4 acc[LD_CT];
#pragma unroll
  for (int c = 0; c < LD_CT; ++c) acc[c] = ld_f64x4{0, 0, 0, 0};

  for (int t0 = 0; t0 < it.n; t0 += LD_TB) {
    const int nt = min(LD_TB, it.n - t0);
    __syncthreads();
    for (int t = wave; t < LD_TB; t += 4) {                  // a wave stages a frame: its row and clamp bounds are wave-uniform
      float* zr = zs + t * ZS;
      const bool in = t < nt;
      int32_t row = 0, lo = 0, hi = 0;
      if (in) { row = p.pos_row[it.pos0 + t0 + t]; lo = p.row_lo[row]; hi = p.row_hi[row]; }
#pragma unroll
      for (int m = 0; m < LD_CG; ++m) {
        const int c = lane + 64 * m;
        if (c >= ZS) break;
        float v = 0.0f;
        if (in && ck[m] >= 0) v = p.feats[(int64_t)min(max(row + ck[m] - L, lo), hi) * D + cj[m]];
        zr[c] = v;
      }
    }
    if (tid < LD_TB) ws[tid] = tid < nt ? p.row_w[p.pos_row[it.pos0 + t0 + tid]] : 0.0;
    __syncthreads();
    if (!live) continue;
    const float* zi = zs + 16 * u.ti + j16;
    const float* zj = zs + 16 * u.tj0 + j16;
    for (int tk = 0; tk < LD_TB; tk += 4) {
      if (tk >= nt) break;                                  // the rest of the block is zero rows
      const int t = tk + q;
      const double a = __dmul_rn(ws[t], (double)zi[t * ZS]);
#pragma unroll
      for (int c = 0; c < LD_CT; ++c)
        if (c < ntj) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, (double)zj[t * ZS + 16 * c], acc[c], 0, 0, 0);
    }
  }
  if (!live) return;
  double* dst = p.part + (int64_t)it.slot * SZ2;
#pragma unroll
  for (int c = 0; c < LD_CT; ++c) {
    if (c >= ntj) continue;
    const int j = 16 * (u.tj0 + c) + j16;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = 16 * u.ti + q + 4 * r;
      if (i < Dz && j <= i) dst[(int64_t)i * (i + 1) / 2 + j] = acc[c][r];
    }
  }
}

// call[e] += the parked slices 0 .. nslot - 1, in slice order
__global__ __launch_bounds__(256) void k_lda_reduce(const double* __restrict__ part, int32_t nslot, double* __restrict__ call, int64_t SZ2) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < SZ2; e += stride) {
    double v = call[e];
    for (int k = 0; k < nslot; ++k) v += part[(int64_t)k * SZ2 + e];
    call[e] = v;
  }
}

// dst += scale * src, one product and one add per element (the call's sums into the handle: scale 1; khg_lda_stats_add)
__global__ __launch_bounds__(256) void k_lda_axpy(double* __restrict__ dst, const double* __restrict__ src, double scale, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) dst[i] = __dadd_rn(dst[i], __dmul_rn(scale, src[i]));
}
