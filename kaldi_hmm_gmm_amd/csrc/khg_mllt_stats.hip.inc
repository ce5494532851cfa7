// MLLT statistics (khg_acc_mllt_stats_post, DESIGN.md 7m): Kaldi's MlltAccs from posteriors resident on the device, split into a frame
// side and a Gaussian side.
//
// Pipeline per call: khg_acc_stats_post with one work item per pdf into the handle's own accumulator block (occ_g, m_g) -> k_mllt_shift_part / k_mllt_shift (the
// shift c) -> the fMLLR plan (khg_fmllr_stats.hip.inc / khg_fmllr_entry.hip.inc: heads, posrow, bucket, entry vectors, frame sums) with
// k_mllt_gram in place of k_fmllr_gram, parked and reduced in slice order (k_fmllr_reduce) -> k_mllt_gauss per chunk of 1024-Gaussian
// slices, parked and reduced the same way -> k_mllt_fold (S - C into the handle).  No atomics in the kernels of this file; K3's closing fp64 atomics have one writer per cell in this call.
//
// The block of doubles: G[D][D (D + 1) / 2] (Kaldi's packed lower triangle per d: (i, j <= i) at i (i + 1) / 2 + j) | beta.

constexpr int MT_GSLICE = 1024;    // Gaussians of one work item of the Gaussian side: the model's (pdf, g) list is cut every MT_GSLICE
constexpr int MT_GB = 32;          // Gaussians staged in LDS at a time

// the column (i, j <= i) of packed index c
__device__ __forceinline__ void mt_pair(int c, int* pi, int* pj) {
  int i = (int)((sqrtf(8.0f * (float)c + 1.0f) - 1.0f) * 0.5f);
  while ((i + 1) * (i + 2) / 2 <= c) ++i;
  while (i * (i + 1) / 2 > c) --i;
  *pi = i; *pj = c - i * (i + 1) / 2;
}

// The shift: per slice of MT_GSLICE consecutive Gaussians the fp64 sum of mu_g[j] = means_invvars / inv_vars (one float division) in
// Gaussian order, one thread per dimension ...
__global__ __launch_bounds__(128) void k_mllt_shift_part(const float* __restrict__ miv, const float* __restrict__ iv, int64_t sumG, int32_t D,
                                                         double* __restrict__ part) {
  const int j = threadIdx.x;
  if (j >= D) return;
  const int64_t g0 = (int64_t)blockIdx.x * MT_GSLICE, g1 = min(g0 + (int64_t)MT_GSLICE, sumG);
  double s = 0.0;
  for (int64_t g = g0; g < g1; ++g) s += (double)__fdiv_rn(miv[g * D + j], iv[g * D + j]);
  part[(int64_t)blockIdx.x * D + j] = s;
}
// ... then the slices' sums in slice order, divided by the number of Gaussians, narrowed to float
__global__ __launch_bounds__(128) void k_mllt_shift(const double* __restrict__ part, int32_t nslice, int64_t sumG, int32_t D, float* __restrict__ c) {
  const int j = threadIdx.x;
  if (j >= D) return;
  double s = 0.0;
  for (int k = 0; k < nslice; ++k) s += part[(int64_t)k * D + j];
  c[j] = (float)(s / (double)sumG);
}

// The frame side's Gram kernel: k_fmllr_gram (khg_fmllr_stats.hip.inc; the same operand maps, the same NDT row tiles, z formed once per
// frame and fed to all of them) on x' = (double)x - (double)c -- the difference of two floats, exact in a double, so that the frame
// side and the Gaussian side are shifted by the SAME vector and the shift cancels to fp64 rounding (a float subtraction would leave
// 6e-8 of the uncancelled term: DESIGN.md 7m) --, with no b / K columns and no border column: C[d][pair] = sum_t a_t[d] (x'[i] x'[j])
// over the frames of one slice, four frames per instruction in frame order.  blockIdx.x: the slice; blockIdx.y: a group of FM_TPG
// column tiles, FM_TPW per wave.  A lane keeps the two shifts of its column in registers.
// Dynamic LDS: xs[FM_TB][XS] | as[FM_TB][16 NDT] floats; column D of xs is 0 (what a padding column reads; never written back).
template <int NDT>
__global__ __launch_bounds__(256) void k_mllt_gram(FmArgs p, const FmItem* __restrict__ items, const float* __restrict__ shift) {
  extern __shared__ __attribute__((aligned(16))) float fm_lds[];
  const FmItem it = items[blockIdx.x];
  const int D = p.D, NP = D * (D + 1) / 2, NT = (NP + 15) / 16;
  constexpr int DP = 16 * NDT;
  const int XS = (D + 1) | 1;
  float* xs = fm_lds;
  float* as = xs + FM_TB * XS;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j16 = lane & 15, q = lane >> 4;
  int ci[FM_TPW], cj[FM_TPW], tile[FM_TPW];
  double si[FM_TPW], sj[FM_TPW];
  bool live[FM_TPW];
#pragma unroll
  for (int s = 0; s < FM_TPW; ++s) {
    tile[s] = blockIdx.y * FM_TPG + s * 4 + wave;
    live[s] = tile[s] < NT;
    ci[s] = D; cj[s] = D; si[s] = 0.0; sj[s] = 0.0;
    const int c = tile[s] * 16 + j16;
    if (live[s] && c < NP) { mt_pair(c, &ci[s], &cj[s]); si[s] = (double)shift[ci[s]]; sj[s] = (double)shift[cj[s]]; }
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
      if (t < nt && j < D) v = p.feats[(int64_t)p.pos_row[it.pos0 + t0 + t] * D + j];
      xs[e] = v;
    }
    for (int e = tid; e < FM_TB * DP; e += 256) {
      const int t = e / DP, d = e - t * DP;
      as[e] = (t < nt && d < D) ? p.a[(int64_t)(it.pos0 + t0 + t) * D + d] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < FM_TPW; ++s) {
      if (!live[s]) continue;                               // wave-uniform
      for (int tk = 0; tk < FM_TB; tk += 4) {
        if (tk >= nt) break;                                // the rest of the block is zero rows
        const int t = tk + q;
        const double z = __dmul_rn(__dsub_rn((double)xs[t * XS + ci[s]], si[s]), __dsub_rn((double)xs[t * XS + cj[s]], sj[s]));
#pragma unroll
        for (int m = 0; m < NDT; ++m) {
          const double av = (double)as[t * DP + 16 * m + j16];
          acc[s][m] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, z, acc[s][m], 0, 0, 0);
        }
      }
    }
  }
  double* dst = p.part + (int64_t)it.slot * p.SZ;           // the slice's image: G | beta
#pragma unroll
  for (int s = 0; s < FM_TPW; ++s) {
    if (!live[s]) continue;
    const int col = tile[s] * 16 + j16;
    if (col >= NP) continue;
#pragma unroll
    for (int m = 0; m < NDT; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int d = 16 * m + q + 4 * r;
        if (d < D) dst[(int64_t)d * NP + col] = acc[s][m][r];
      }
  }
  if (blockIdx.y == 0 && wave == 0) {                       // beta of the slice, as k_fmllr_gram adds it
    double s = 0.0;
    for (int t = lane; t < it.n; t += 64) s += p.c[it.pos0 + t];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) dst[p.SZ - 1] = s;
  }
}

// The Gaussian side, the same GEMM shape on the fp64 matrix pipe: C[d][pair] = sum_g A[g][d] Z[g][pair] over one slice of MT_GSLICE
// consecutive Gaussians, A = (double)inv_var[g][d], Z[g][(i, j)] = (m'[i] mu'[j] + mu'[i] m'[j]) - (occ mu'[i]) mu'[j] with
// mu' = (double)mu_g - (double)c, m' = m_g - occ_g (double)c, each one fp64 operation.  blockIdx.x: the slice (slot blockIdx.x of the
// chunk, Gaussians from g_first + MT_GSLICE blockIdx.x); blockIdx.y: a group of FM_TPG column tiles.  A wave forms the Z of its
// column ONCE per Gaussian and feeds it to its NDT row tiles (an fp64 MFMA holds the SIMD's issue: khg_fmllr_stats.hip.inc).  The sum
// runs in Gaussian order, four Gaussians per instruction.
// Dynamic LDS: mus[MT_GB][XS] | ms[MT_GB][XS] | occ[MT_GB] doubles | ivs[MT_GB][16 NDT] floats; XS odd, column D is 0.
struct MtGaussArgs {
  const float *miv, *iv; const double *occ, *mean; const float* shift;
  int64_t sumG, g_first; int32_t D; double* part; int64_t SZ;
};
template <int NDT>
__global__ __launch_bounds__(256) void k_mllt_gauss(MtGaussArgs p) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double mt_lds[];
  const int D = p.D, NP = D * (D + 1) / 2, NT = (NP + 15) / 16;
  constexpr int DP = 16 * NDT;
  const int XS = (D + 1) | 1;
  double* mus = mt_lds;
  double* ms = mus + MT_GB * XS;
  double* occs = ms + MT_GB * XS;
  float* ivs = reinterpret_cast<float*>(occs + MT_GB);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j16 = lane & 15, q = lane >> 4;
  const int64_t gs0 = p.g_first + (int64_t)blockIdx.x * MT_GSLICE;
  const int ng_slice = (int)min((int64_t)MT_GSLICE, p.sumG - gs0);
  int ci[FM_TPW], cj[FM_TPW], tile[FM_TPW];
  bool live[FM_TPW];
#pragma unroll
  for (int s = 0; s < FM_TPW; ++s) {
    tile[s] = blockIdx.y * FM_TPG + s * 4 + wave;
    live[s] = tile[s] < NT;
    ci[s] = D; cj[s] = D;
    const int c = tile[s] * 16 + j16;
    if (live[s] && c < NP) mt_pair(c, &ci[s], &cj[s]);
  }
  fm_f64x4 acc[FM_TPW][NDT];
#pragma unroll
  for (int s = 0; s < FM_TPW; ++s)
#pragma unroll
    for (int m = 0; m < NDT; ++m) acc[s][m] = fm_f64x4{0, 0, 0, 0};

  for (int b0 = 0; b0 < ng_slice; b0 += MT_GB) {
    const int nb = min(MT_GB, ng_slice - b0);
    __syncthreads();
    for (int e = tid; e < MT_GB * XS; e += 256) {
      const int k = e / XS, j = e - k * XS;
      double mu = 0.0, mm = 0.0;
      if (k < nb && j < D) {
        const int64_t g = gs0 + b0 + k;
        const double cd = (double)p.shift[j];
        mu = (double)__fdiv_rn(p.miv[g * D + j], p.iv[g * D + j]) - cd;
        mm = p.mean[g * D + j] - p.occ[g] * cd;
      }
      mus[e] = mu; ms[e] = mm;
    }
    for (int e = tid; e < MT_GB * DP; e += 256) {
      const int k = e / DP, d = e - k * DP;
      ivs[e] = (k < nb && d < D) ? p.iv[(gs0 + b0 + k) * D + d] : 0.0f;
    }
    if (tid < MT_GB) occs[tid] = tid < nb ? p.occ[gs0 + b0 + tid] : 0.0;
    __syncthreads();
#pragma unroll
    for (int s = 0; s < FM_TPW; ++s) {
      if (!live[s]) continue;                               // wave-uniform
      for (int gk = 0; gk < MT_GB; gk += 4) {
        if (gk >= nb) break;                                // the rest of the block is zero rows
        const int k = gk + q;
        const double mui = mus[k * XS + ci[s]], muj = mus[k * XS + cj[s]];
        const double z = (ms[k * XS + ci[s]] * muj + mui * ms[k * XS + cj[s]]) - (occs[k] * mui) * muj;
#pragma unroll
        for (int m = 0; m < NDT; ++m) {
          const double av = (double)ivs[k * DP + 16 * m + j16];
          acc[s][m] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, z, acc[s][m], 0, 0, 0);
        }
      }
    }
  }
  double* dst = p.part + (int64_t)blockIdx.x * p.SZ;
#pragma unroll
  for (int s = 0; s < FM_TPW; ++s) {
    if (!live[s]) continue;
    const int col = tile[s] * 16 + j16;
    if (col >= NP) continue;
#pragma unroll
    for (int m = 0; m < NDT; ++m)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int d = 16 * m + q + 4 * r;
        if (d < D) dst[(int64_t)d * NP + col] = acc[s][m][r];
      }
  }
  if (blockIdx.y == 0 && tid == 0) dst[p.SZ - 1] = 0.0;     // the Gaussian side has no count
}

// the parked images of one chunk of Gaussian-side slices, added in slice order onto the call's C
__global__ __launch_bounds__(256) void k_mllt_greduce(const double* __restrict__ part, int32_t nslot, double* __restrict__ call, int64_t SZ) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < SZ; e += (int64_t)gridDim.x * 256) {
    double v = call[e];
    for (int k = 0; k < nslot; ++k) v += part[(int64_t)k * SZ + e];
    call[e] = v;
  }
}

// the call's sums into the handle: G += S - C (one subtraction, one addition), beta += the frame side's (C's is 0)
__global__ __launch_bounds__(256) void k_mllt_fold(double* __restrict__ dst, const double* __restrict__ s, const double* __restrict__ c, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) dst[i] = __dadd_rn(dst[i], __dsub_rn(s[i], c[i]));
}

// gmm-transform-means on the handle (khg_model_transform_means): one wave per Gaussian, lanes over d (lane and lane + 64).  M sits in
// LDS at an odd row stride; the wave's mu = means_invvars / inv_vars is staged beside it; every lane runs its own fmaf chain in j order,
// so no value crosses lanes.  means_invvars = y * inv_vars; then lane 0 recomputes the gconst as DiagGmm::ComputeGconsts does (float
// accumulator, double right-hand side, d in order: k4_gconst's arithmetic).
// Dynamic LDS (floats): Ms[D][MS] | per wave: mu[D] | nm[D].
__global__ __launch_bounds__(256) void k_model_transform_means(const float* __restrict__ M, int64_t sumG, int32_t D, const float* __restrict__ w,
                                                               const float* __restrict__ iv, float* __restrict__ miv, float* __restrict__ gc,
                                                               int32_t* __restrict__ bad) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float tm_lds[];
  const int MS = D | 1;
  float* Ms = tm_lds;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* mu = Ms + D * MS + wave * 2 * D;
  float* nm = mu + D;
  for (int e = tid; e < D * D; e += 256) { const int d = e / D, j = e - d * D; Ms[d * MS + j] = M[e]; }
  __syncthreads();
  const float offset = (float)(-0.5 * 1.8378770664093454835606594728112 * D);
  for (int64_t g = (int64_t)blockIdx.x * 4 + wave; g < sumG; g += (int64_t)gridDim.x * 4) {
    for (int d = lane; d < D; d += 64) mu[d] = __fdiv_rn(miv[g * D + d], iv[g * D + d]);
    fm_wave_sync();
    for (int d = lane; d < D; d += 64) {
      float y = 0.0f;
      for (int j = 0; j < D; ++j) y = fmaf(Ms[d * MS + j], mu[j], y);
      const float v = __fmul_rn(y, iv[g * D + d]);
      miv[g * D + d] = v; nm[d] = v;
    }
    fm_wave_sync();
    if (lane == 0) {
      float c = logf(w[g]) + offset;
      for (int d = 0; d < D; ++d) {
        const float ivf = iv[g * D + d];
        const double ivd = (double)ivf, mi = (double)nm[d];
        const double rhs = 0.5 * (double)logf(ivf) - 0.5 * mi * mi / ivd;
        c = (float)((double)c + rhs);
      }
      if (c != c) atomicOr(bad, 1);
      if (isinf(c) && c > 0) c = -c;
      gc[g] = c;
    }
    fm_wave_sync();
  }
}
