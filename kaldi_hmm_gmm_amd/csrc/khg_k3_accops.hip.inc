// khg_k3_accops.hip.inc -- elementwise operations on whole accumulator blocks (khg_accs_add / _scale / _smooth_with_accum): what
// Kaldi's gmm-sum-accs (AccumAmDiagGmm::Add / Scale, csrc/mle-am-diag-gmm.cc:119-138) and gmm-ismooth-stats
// (AccumDiagGmm::SmoothWithAccum, csrc/mle-diag-gmm.cc:209-226) do on files, on blocks that stay in HBM.  One fp64 operation per
// element in the host classes' order, contraction off: bit-identical to AccumDiagGmm::Add / Scale / SmoothWithAccum.  HBM-bound.
#pragma once

// dst[i] += s * src[i] (src may be dst)
__global__ __launch_bounds__(256) void k3_accs_add(double* dst, const double* src, double s, int64_t n) {
#pragma clang fp contract(off)
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) dst[i] = dst[i] + src[i] * s;
}
__global__ __launch_bounds__(256) void k3_accs_scale(double* dst, double f, int64_t n) {
#pragma clang fp contract(off)
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) dst[i] = dst[i] * f;
}
// One wave per Gaussian (4 per workgroup).  A wave touches its own Gaussian's count and rows only, and holds the source count `so` and
// the new destination count `dn` in registers before it writes anything: that is what lets dst == src (a block smoothed with itself)
// use the old count for every row.  (The barrier below is not needed for that; every thread reaches it before the range check returns.)
__global__ __launch_bounds__(256) void k3_accs_smooth(double* d_occ, double* d_mean, double* d_var, const double* s_occ, const double* s_mean,
                                                      const double* s_var, double tau, int64_t sumG, int D, int32_t* untouched) {
#pragma clang fp contract(off)
  const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const bool in = g < sumG;
  const double so = in ? s_occ[g] : 0.0;
  const double dn = in ? d_occ[g] + tau : 0.0;
  __syncthreads();
  if (!in) return;
  if (so != 0.0) {
    const int64_t row = g * D;
    for (int d = lane; d < D; d += 64) {
      d_mean[row + d] = d_mean[row + d] + s_mean[row + d] * tau / so;
      d_var[row + d] = d_var[row + d] + s_var[row + d] * tau / so;
    }
    if (lane == 0) d_occ[g] = dn;
  } else if (lane == 0 && untouched) {
    atomicAdd(untouched, 1);
  }
}
