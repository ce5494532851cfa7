// The fMLLR estimate on the device (khg_fmllr_stats_estimate, DESIGN.md 7l): khg_fmllr_compute's arithmetic, operation for operation.
// k_fmllr_invg: one workgroup per (speaker, d) inverts G[d] by Gauss-Jordan without pivoting into HBM scratch.  k_fmllr_rows: one
// workgroup per speaker runs the sweeps -- A^T's Gauss-Jordan with lanes over elements, cg and W[d] with one lane per output element
// summing in index order, the scalars (pivot search, the quadratic's roots, the sums of Q) on one lane.  No cross-lane reduction is
// on a value path, and contraction is off: W, the statuses and the counts have the host form's bits (the two log calls decide the
// root only where the roots tie, and round objf_impr).  invG lives in HBM scratch (a workgroup's own: barriers order it); A^T and its
// inverse in LDS where they fit (D <= 59), else in HBM scratch too.
#pragma clang fp contract(off)

struct FeArgs {
  const double* stats; int64_t SZ; int32_t S, D;     // the handle's blocks: K | G | beta
  double min_count; int32_t num_iters;
  double* invg;      // [S][D][D1][D1]
  double* work;      // k_fmllr_invg: [S][D][D1][D1] the matrix being reduced; k_fmllr_rows: per speaker M | inv (D x D each) from its start
  double* W;         // [S][D][D1]
  int32_t* status;   // [S]
  double* impr;      // [S]
  float* Wf;         // [S][D][D1] narrowed (may be null)
};

__global__ __launch_bounds__(256) void k_fmllr_invg(FeArgs a) {
  const int D = a.D, D1 = D + 1, NP = D1 * (D1 + 1) / 2, tid = threadIdx.x;
  const int s = blockIdx.x / D, d = blockIdx.x % D;
  const double* blk = a.stats + (int64_t)s * a.SZ;
  if (blk[a.SZ - 1] < a.min_count) { if (tid == 0 && d == 0) a.status[s] = KHG_FMLLR_LOW_COUNT; return; }
  const double* g = blk + (int64_t)D * D1 + (int64_t)d * NP;
  double* M = a.work + ((int64_t)s * D + d) * D1 * D1;
  double* inv = a.invg + ((int64_t)s * D + d) * D1 * D1;
  __shared__ double fcol[KHG_FMLLR_MAX_DIM + 1];
  for (int e = tid; e < D1 * D1; e += 256) {
    const int i = e / D1, j = e - i * D1;
    M[e] = g[j <= i ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i];
    inv[e] = i == j ? 1.0 : 0.0;
  }
  __syncthreads();
  for (int p = 0; p < D1; ++p) {
    const double piv = M[p * D1 + p];
    if (!(isfinite(piv) && piv > 0.0)) { if (tid == 0) atomicMax(&a.status[s], KHG_FMLLR_SINGULAR); return; }     // uniform: every thread read the same pivot
    __syncthreads();
    for (int j = tid; j < D1; j += 256) { M[p * D1 + j] = M[p * D1 + j] / piv; inv[p * D1 + j] = inv[p * D1 + j] / piv; }
    __syncthreads();
    for (int r = tid; r < D1; r += 256) fcol[r] = M[r * D1 + p];
    __syncthreads();
    for (int e = tid; e < D1 * D1; e += 256) {
      const int r = e / D1, j = e - r * D1;
      if (r == p) continue;
      const double f = fcol[r];
      M[e] = M[e] - f * M[p * D1 + j];
      inv[e] = inv[e] - f * inv[p * D1 + j];
    }
    __syncthreads();
  }
}

// inv = M^-1 (D x D) by Gauss-Jordan with partial pivoting, as FmInvPiv (khg_host.cpp); *ld = sum of log |pivot| (thread 0's value);
// returns false (uniformly) on a pivot that is zero or not finite.  sh: fcol[D] | 2 scalars.
__device__ bool fe_inv_piv(int D, double* M, double* inv, double* sh_f, int* sh_i, double* ld_out) {
  const int tid = threadIdx.x;
  double ld = 0.0;
  for (int e = tid; e < D * D; e += 256) inv[e] = (e / D == e % D) ? 1.0 : 0.0;
  __syncthreads();
  for (int p = 0; p < D; ++p) {
    if (tid == 0) {
      int best = p;
      double bv = fabs(M[p * D + p]);
      for (int r = p + 1; r < D; ++r) { const double v = fabs(M[r * D + p]); if (v > bv) { bv = v; best = r; } }
      sh_i[0] = best;
    }
    __syncthreads();
    const int best = sh_i[0];
    if (best != p)
      for (int j = tid; j < D; j += 256) {
        double t = M[p * D + j]; M[p * D + j] = M[best * D + j]; M[best * D + j] = t;
        t = inv[p * D + j]; inv[p * D + j] = inv[best * D + j]; inv[best * D + j] = t;
      }
    __syncthreads();
    const double piv = M[p * D + p];
    if (!isfinite(piv) || piv == 0.0) return false;
    ld = ld + log(fabs(piv));
    __syncthreads();
    for (int j = tid; j < D; j += 256) { M[p * D + j] = M[p * D + j] / piv; inv[p * D + j] = inv[p * D + j] / piv; }
    __syncthreads();
    for (int r = tid; r < D; r += 256) sh_f[r] = M[r * D + p];
    __syncthreads();
    for (int e = tid; e < D * D; e += 256) {
      const int r = e / D, j = e - r * D;
      if (r == p) continue;
      const double f = sh_f[r];
      M[e] = M[e] - f * M[p * D + j];
      inv[e] = inv[e] - f * inv[p * D + j];
    }
    __syncthreads();
  }
  *ld_out = ld;
  return true;
}

// sum_d (W[d] . K[d] - 1/2 W[d] G[d] W[d]^T): one thread per d for the two terms, thread 0 adds them in d order (FmAuxf's order)
__device__ double fe_auxf_terms(int D, const double* K, const double* G, const double* W, double* term) {
  const int D1 = D + 1, NP = D1 * (D1 + 1) / 2;
  for (int d = threadIdx.x; d < D; d += 256) {
    const double* g = G + (int64_t)d * NP;
    const double* w = W + d * D1;
    double t1 = 0.0, t2 = 0.0;
    for (int i = 0; i < D1; ++i) t1 = t1 + w[i] * K[d * D1 + i];
    for (int i = 0; i < D1; ++i) {
      double r = 0.0;
      for (int j = 0; j < D1; ++j) r = r + g[j <= i ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i] * w[j];
      t2 = t2 + w[i] * r;
    }
    term[d] = t1 - 0.5 * t2;
  }
  __syncthreads();
  double acc = 0.0;
  if (threadIdx.x == 0)
    for (int d = 0; d < D; ++d) acc = acc + term[d];
  __syncthreads();
  return acc;      // thread 0's is the value
}

__global__ __launch_bounds__(256) void k_fmllr_rows(FeArgs a, int use_lds) {
  const int D = a.D, D1 = D + 1, tid = threadIdx.x, s = blockIdx.x;
  const double* blk = a.stats + (int64_t)s * a.SZ;
  const double* K = blk;
  const double* G = blk + (int64_t)D * D1;
  const double beta = blk[a.SZ - 1];
  double* W = a.W + (int64_t)s * D * D1;
  // A^T and its inverse (D x D each): in LDS where the launch gave room for them (use_lds: 2 D^2 doubles fit), else in the speaker's
  // share of k_fmllr_invg's work block in HBM, free by now.  Same operations either way.
  extern __shared__ __attribute__((aligned(16))) double fe_dyn[];
  double* M = use_lds ? fe_dyn : a.work + (int64_t)s * D * D1 * D1;
  double* inv = M + D * D;
  __shared__ double sh_vec[4 * (KHG_FMLLR_MAX_DIM + 1)];
  double* c = sh_vec;
  double *cg = c + D1, *v = cg + D1, *term = v + D1;
  __shared__ double sh_f[KHG_FMLLR_MAX_DIM + 1];
  __shared__ double sh_alpha;
  __shared__ int sh_i[2];
  int status = a.status[s];
  for (int e = tid; e < D * D1; e += 256) W[e] = (e / D1 == e % D1) ? 1.0 : 0.0;
  __syncthreads();
  double q0 = 0.0, q1 = 0.0;
  if (status == KHG_FMLLR_OK) {
    q0 = beta * 0.0 + fe_auxf_terms(D, K, G, W, term);
    for (int it = 0; it < a.num_iters && status == KHG_FMLLR_OK; ++it)
      for (int d = 0; d < D; ++d) {
        for (int e = tid; e < D * D; e += 256) M[e] = W[(e % D) * D1 + e / D];       // A^T
        __syncthreads();
        double ld;
        if (!fe_inv_piv(D, M, inv, sh_f, sh_i, &ld)) { status = KHG_FMLLR_SINGULAR; break; }
        for (int j = tid; j < D1; j += 256) c[j] = j < D ? inv[d * D + j] : 0.0;
        __syncthreads();
        const double* ig = a.invg + ((int64_t)s * D + d) * D1 * D1;
        const double* k = K + d * D1;
        for (int i = tid; i < D1; i += 256) {
          double r = 0.0;
          for (int j = 0; j < D1; ++j) r = r + ig[i * D1 + j] * c[j];
          cg[i] = r;
        }
        __syncthreads();
        if (tid == 0) {
          double e1 = 0.0, e2 = 0.0;
          for (int i = 0; i < D1; ++i) e1 = e1 + cg[i] * c[i];
          for (int i = 0; i < D1; ++i) e2 = e2 + cg[i] * k[i];
          const double disc = sqrt(e2 * e2 + (4.0 * e1) * beta);
          const double a1 = (-e2 + disc) / (2.0 * e1), a2 = (-e2 - disc) / (2.0 * e1);
          const double f1 = beta * log(fabs(a1 * e1 + e2)) - ((0.5 * a1) * a1) * e1;
          const double f2 = beta * log(fabs(a2 * e1 + e2)) - ((0.5 * a2) * a2) * e1;
          sh_alpha = f1 > f2 ? a1 : a2;
        }
        __syncthreads();
        const double alpha = sh_alpha;
        for (int i = tid; i < D1; i += 256) v[i] = alpha * c[i] + k[i];
        __syncthreads();
        for (int i = tid; i < D1; i += 256) {
          double r = 0.0;
          for (int j = 0; j < D1; ++j) r = r + ig[i * D1 + j] * v[j];
          W[d * D1 + i] = r;
        }
        __syncthreads();
      }
    if (status == KHG_FMLLR_OK) {
      for (int e = tid; e < D * D; e += 256) M[e] = W[(e % D) * D1 + e / D];
      __syncthreads();
      double ld = 0.0;
      if (!fe_inv_piv(D, M, inv, sh_f, sh_i, &ld)) status = KHG_FMLLR_SINGULAR;
      else q1 = beta * ld + fe_auxf_terms(D, K, G, W, term);
    }
  }
  __syncthreads();
  if (status != KHG_FMLLR_OK) {
    for (int e = tid; e < D * D1; e += 256) W[e] = (e / D1 == e % D1) ? 1.0 : 0.0;
    __syncthreads();
  }
  if (a.Wf)
    for (int e = tid; e < D * D1; e += 256) a.Wf[(int64_t)s * D * D1 + e] = (float)W[e];
  if (tid == 0) { a.status[s] = status; a.impr[s] = status == KHG_FMLLR_OK ? q1 - q0 : 0.0; }
}
