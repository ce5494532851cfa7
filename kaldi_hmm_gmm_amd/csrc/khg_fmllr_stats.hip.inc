// fMLLR statistics (khg_acc_fmllr_stats_post, DESIGN.md 7l): Kaldi's FmllrDiagGmmAccs per speaker from posteriors resident on the device.
//
// Pipeline per call: posteriors_flatten (khg_lattices.hip) -> e_row / e_tid / e_w [E] in utterance, frame, entry order ->
// k_fmllr_heads (the first entry of every feature row) -> per chunk of speaker slices: k_fmllr_posrow (compact position -> feature
// row), k_fmllr_frame (the frame vectors a_t, b_t, c_t), k_fmllr_gram (the weighted Gram matrices of one slice on the fp64 matrix
// pipe, parked per slice), k_fmllr_reduce (the slices of a speaker added in slice order into the call's sums) -> k_fmllr_axpy (the
// call's sums into the handle).  No atomics on any value: a speaker's statistics depend on its own frame list and nothing else.
//
// A speaker's block of doubles: K[D][D+1] | G[D][(D+1)(D+2)/2] (Kaldi's packed lower triangle per d: (i, j <= i) at i (i + 1) / 2 + j)
// | beta.

constexpr int FM_SLICE = 1024;     // frames of one work item: a speaker's frame list is cut every FM_SLICE frames, whatever else is in the call
constexpr int FM_TB = 64;          // frames staged in LDS at a time
constexpr int FM_TPW = 2;          // column tiles a wave keeps accumulators for
constexpr int FM_TPG = 4 * FM_TPW; // column tiles of one workgroup (tile group)

struct FmSeg { int32_t row0, n, pos0, pad; };            // n feature rows from row0 sit at compact positions pos0 .. of their chunk
struct FmItem { int32_t spk, pos0, n, slot; };           // one slice: positions [pos0, pos0 + n) of its chunk, parked in slot `slot` of the chunk
struct FmRun { int32_t spk, slot0, nslot, pad; };        // the slices of one speaker inside one chunk

struct FmArgs {
  const float* feats; int32_t D; int64_t N;
  // model
  const int32_t* gauss_off; const float *gconsts, *miv, *iv, *nhiv; int32_t P;
  const int32_t* id2pdf; int32_t num_tids;
  // entries
  const int32_t *e_row, *e_tid; const float* e_w; int64_t E;
  int32_t* row_first;               // [N] first entry of a feature row, -1 without one
  // chunk scratch
  int32_t* pos_row; float *a, *b; double* c;
  double* part; int64_t SZ;
  int32_t* err_flag;
};

// the first entry of every feature row that has one (rows ascend with the entries: posteriors_flatten's order)
__global__ __launch_bounds__(256) void k_fmllr_heads(FmArgs p) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < p.E; i += stride) {
    const int32_t r = p.e_row[i];
    if (r < 0 || (int64_t)r >= p.N) continue;
    if (i == 0 || p.e_row[i - 1] != r) p.row_first[r] = (int32_t)i;
  }
}

__global__ __launch_bounds__(256) void k_fmllr_posrow(const FmSeg* __restrict__ segs, int32_t nseg, int32_t* __restrict__ pos_row) {
  for (int s = blockIdx.x; s < nseg; s += gridDim.x) {
    const FmSeg g = segs[s];
    for (int i = threadIdx.x; i < g.n; i += 256) pos_row[g.pos0 + i] = g.row0 + i;
  }
}

// LDS written by some lanes of a wave and read by others: the wave's LDS operations complete in order, the fence keeps the compiler from
// moving them across
__device__ __forceinline__ void fm_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// One wave per frame (compact position): for every entry of the frame, in entry order, the component posteriors of the entry's pdf as
// the POST forms of K3 compute them -- per Gaussian the fp32 chain s = gconst; per pair of dimensions two fmaf with M, two with -V / 2
// on fl(x^2); e = exp(s - max); gamma = e * (w / sum) -- then ea[d] = sum_g gamma_g V[g][d], eb[d] = sum_g gamma_g M[g][d] in Gaussian
// order (one product and one add each, no contraction), ec = sum_g gamma_g; the frame's a_t / b_t are the float sums of the entries'
// vectors in entry order, c_t the double sum.  Lanes over Gaussians for the posteriors, over dimensions for the vectors.
// Dynamic LDS per wave: x[DP] | x2[DP] | gamma[GM].
__global__ __launch_bounds__(256) void k_fmllr_frame(FmArgs p, int32_t npos, int32_t DP, int32_t GM) {
  extern __shared__ __attribute__((aligned(16))) float fm_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* xs = fm_lds + (size_t)wave * (2 * DP + GM);
  float* x2 = xs + DP;
  float* gam = x2 + DP;
  const int D = p.D;
  for (int pos = blockIdx.x * 4 + wave; pos < npos; pos += gridDim.x * 4) {
    const int32_t row = p.pos_row[pos];
    for (int d = lane; d < D; d += 64) {
      const float v = p.feats[(int64_t)row * D + d];
      xs[d] = v; x2[d] = __fmul_rn(v, v);
    }
    fm_wave_sync();
    float at[2] = {0.0f, 0.0f}, bt[2] = {0.0f, 0.0f};      // dimensions lane and lane + 64 (D <= 80)
    double ct = 0.0;
    int32_t i = p.row_first[row];
    for (; i >= 0 && (int64_t)i < p.E && p.e_row[i] == row; ++i) {
      const int tid = p.e_tid[i];
      const float w = p.e_w[i];
      if (tid < 1 || tid > p.num_tids || w == 0.0f) continue;
      const int pdf = p.id2pdf[tid];
      if (pdf < 0 || pdf >= p.P) { if (lane == 0) atomicOr(p.err_flag, 4); continue; }
      const int g0 = p.gauss_off[pdf], G = p.gauss_off[pdf + 1] - g0;
      float mx = -INFINITY;
      for (int g = lane; g < G; g += 64) {
        const float* M = p.miv + (int64_t)(g0 + g) * D;
        const float* V = p.nhiv + (int64_t)(g0 + g) * D;
        float s = p.gconsts[g0 + g];
        int d = 0;
        for (; d + 1 < D; d += 2) {
          s = fmaf(M[d], xs[d], s); s = fmaf(M[d + 1], xs[d + 1], s);
          s = fmaf(V[d], x2[d], s); s = fmaf(V[d + 1], x2[d + 1], s);
        }
        if (d < D) { s = fmaf(M[d], xs[d], s); s = fmaf(V[d], x2[d], s); }
        gam[g] = s;
        mx = fmaxf(mx, s);
      }
      for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
      float sum = 0.0f;
      for (int g = lane; g < G; g += 64) { const float e = __expf(gam[g] - mx); gam[g] = e; sum += e; }
      for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
      const float llf = __logf(sum) + mx;
      if (!(fabsf(llf) <= 3.0e38f)) { if (lane == 0) atomicOr(p.err_flag, 1); continue; }     // diag-gmm.cc:385-387
      const float scale = w / sum;
      for (int g = lane; g < G; g += 64) gam[g] = gam[g] * scale;
      fm_wave_sync();
      float ea[2] = {0.0f, 0.0f}, eb[2] = {0.0f, 0.0f}, ec = 0.0f;
      for (int g = 0; g < G; ++g) {
        const float gg = gam[g];
        ec = __fadd_rn(ec, gg);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int d = lane + 64 * h;
          if (d < D) {
            ea[h] = __fadd_rn(ea[h], __fmul_rn(gg, p.iv[(int64_t)(g0 + g) * D + d]));
            eb[h] = __fadd_rn(eb[h], __fmul_rn(gg, p.miv[(int64_t)(g0 + g) * D + d]));
          }
        }
      }
#pragma unroll
      for (int h = 0; h < 2; ++h) { at[h] = __fadd_rn(at[h], ea[h]); bt[h] = __fadd_rn(bt[h], eb[h]); }
      ct += (double)ec;
      fm_wave_sync();
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int d = lane + 64 * h;
      if (d < D) { p.a[(int64_t)pos * D + d] = at[h]; p.b[(int64_t)pos * D + d] = bt[h]; }
    }
    if (lane == 0) p.c[pos] = ct;
    fm_wave_sync();
  }
}

// The Gram kernel: C[d][col] = sum_t A[t][d] Z[t][col] over the frames of one slice on v_mfma_f64_16x16x4_f64, where a column is either a
// pair (i, j <= i) -- A = a_t, Z = (double)x+[i] (double)x+[j], the product of two floats, exact -- or an index j of K -- A = b_t,
// Z = (double)x+[j] * 1.  blockIdx.x: the slice; blockIdx.y: a group of FM_TPG column tiles, FM_TPW per wave.  A wave forms the z of
// its column ONCE per frame and feeds it to the NDT row tiles (d in 16s) it keeps accumulators for: on this chip an fp64 MFMA holds the
// SIMD's issue for its 64 cycles (khg_k3_accstats.hip.inc, k3_accumulate_wave16), so nothing is formed twice and nothing hides.
// Operand maps of the instruction: A[row = lane & 15][k = lane >> 4], B[k = lane >> 4][col = lane & 15], C/D col = lane & 15,
// row = (lane >> 4) + 4 reg.  The sum over t runs in frame order, four frames per instruction: fixed by the slice alone.
// Dynamic LDS: xs[FM_TB][XS] | as[FM_TB][16 NDT] | bs[FM_TB][16 NDT] floats.
typedef double fm_f64x4 __attribute__((ext_vector_type(4)));
template <int NDT>
__global__ __launch_bounds__(256) void k_fmllr_gram(FmArgs p, const FmItem* __restrict__ items) {
  extern __shared__ __attribute__((aligned(16))) float fm_lds[];
  const FmItem it = items[blockIdx.x];
  const int D = p.D, D1 = D + 1, NP = D1 * (D1 + 1) / 2;
  const int NPT = (NP + 15) / 16, NKT = (D1 + 15) / 16, NT = NPT + NKT;
  constexpr int DP = 16 * NDT;
  const int XS = D1 | 1;                                    // odd row stride: the lanes' column reads spread over the banks
  float* xs = fm_lds;
  float* as = xs + FM_TB * XS;
  float* bs = as + FM_TB * DP;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j16 = lane & 15, q = lane >> 4;
  // this lane's column in each of the wave's tiles: the two x+ indices whose product is z, and which of a / b feeds the rows
  int ci[FM_TPW], cj[FM_TPW], tile[FM_TPW];
  bool isk[FM_TPW], live[FM_TPW];
#pragma unroll
  for (int s = 0; s < FM_TPW; ++s) {
    tile[s] = blockIdx.y * FM_TPG + s * 4 + wave;
    live[s] = tile[s] < NT;
    isk[s] = tile[s] >= NPT;
    ci[s] = D; cj[s] = D;                                   // padding columns: 1 * 1, never written
    if (live[s]) {
      if (isk[s]) {
        const int j = (tile[s] - NPT) * 16 + j16;
        if (j < D1) ci[s] = j;
      } else {
        const int c = tile[s] * 16 + j16;
        if (c < NP) {
          int i = (int)((sqrtf(8.0f * (float)c + 1.0f) - 1.0f) * 0.5f);
          while ((i + 1) * (i + 2) / 2 <= c) ++i;
          while (i * (i + 1) / 2 > c) --i;
          ci[s] = i; cj[s] = c - i * (i + 1) / 2;
        }
      }
    }
  }
  fm_f64x4 acc[FM_TPW][NDT];
#pragma unroll
  for (int s = 0; s < FM_TPW; ++s)
#pragma unroll
    for (int m = 0; m < NDT; ++m) acc[s][m] = fm_f64x4{0, 0, 0, 0};

  for (int t0 = 0; t0 < it.n; t0 += FM_TB) {
    const int nt = min(FM_TB, it.n - t0);
    __syncthreads();
    for (int e = tid; e < FM_TB * XS; e += 256) {
      const int t = e / XS, j = e - t * XS;
      float v = 0.0f;
      if (t < nt) {
        if (j < D) v = p.feats[(int64_t)p.pos_row[it.pos0 + t0 + t] * D + j];
        else if (j == D) v = 1.0f;
      }
      xs[e] = v;
    }
    for (int e = tid; e < FM_TB * DP; e += 256) {
      const int t = e / DP, d = e - t * DP;
      float va = 0.0f, vb = 0.0f;
      if (t < nt && d < D) {
        const int64_t o = (int64_t)(it.pos0 + t0 + t) * D + d;
        va = p.a[o]; vb = p.b[o];
      }
      as[e] = va; bs[e] = vb;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < FM_TPW; ++s) {
      if (!live[s]) continue;                               // wave-uniform
      const float* rows = isk[s] ? bs : as;
      for (int tk = 0; tk < FM_TB; tk += 4) {
        if (tk >= nt) break;                                // the rest of the block is zero rows
        const int t = tk + q;
        const double z = (double)xs[t * XS + ci[s]] * (double)xs[t * XS + cj[s]];
#pragma unroll
        for (int m = 0; m < NDT; ++m) {
          const double av = (double)rows[t * DP + 16 * m + j16];
          acc[s][m] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, z, acc[s][m], 0, 0, 0);
        }
      }
    }
  }
  // park the slice's image: K | G | beta
  double* dst = p.part + (int64_t)it.slot * p.SZ;
#pragma unroll
  for (int s = 0; s < FM_TPW; ++s) {
    if (!live[s]) continue;
    const int col = (isk[s] ? tile[s] - NPT : tile[s]) * 16 + j16;
    const int ncol = isk[s] ? D1 : NP;
    if (col >= ncol) continue;
#pragma unroll
    for (int m = 0; m < NDT; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int d = 16 * m + q + 4 * r;
        if (d < D) dst[isk[s] ? (int64_t)d * D1 + col : (int64_t)D * D1 + (int64_t)d * NP + col] = acc[s][m][r];
      }
  }
  if (blockIdx.y == 0 && wave == 0) {                       // beta of the slice: lanes strided over the frames, then a fixed shuffle tree
    double s = 0.0;
    for (int t = lane; t < it.n; t += 64) s += p.c[it.pos0 + t];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) dst[p.SZ - 1] = s;
  }
}

// the slices of a speaker inside this chunk, added in slice order onto the call's sum of that speaker
__global__ __launch_bounds__(256) void k_fmllr_reduce(const FmRun* __restrict__ runs, const double* __restrict__ part, double* __restrict__ call, int64_t SZ) {
  const FmRun r = runs[blockIdx.x];
  for (int64_t e = (int64_t)blockIdx.y * 256 + threadIdx.x; e < SZ; e += (int64_t)gridDim.y * 256) {
    double v = call[(int64_t)r.spk * SZ + e];
    for (int k = 0; k < r.nslot; ++k) v += part[(int64_t)(r.slot0 + k) * SZ + e];
    call[(int64_t)r.spk * SZ + e] = v;
  }
}

// dst += scale * src, one product and one add per element (the call's sums into the handle: scale 1; khg_fmllr_stats_add)
__global__ __launch_bounds__(256) void k_fmllr_axpy(double* __restrict__ dst, const double* __restrict__ src, double scale, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) dst[i] = __dadd_rn(dst[i], __dmul_rn(scale, src[i]));
}
