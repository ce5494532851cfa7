// compute-cmvn-stats (khg_acc_cmvn_stats, DESIGN.md 7p): per speaker sum x, sum x x and the frame count in fp64, no atomics.
//   k_cmvn_slice    one workgroup per slice of <= CV_SLICE frames of ONE speaker's frame list: lanes go over (frame lane, column),
//                   every lane one fp64 chain per sum; the chains meet in LDS in a fixed order; the slice's image is parked
//   k_cmvn_reduce   a speaker's parked slices of the chunk added in slice order onto the call's sums
//   k_cmvn_axpy     dst += scale * src (the call's sums into the handle: scale 1; khg_cmvn_stats_add)
// The order of a slice of n frames at dimension D, with R = 256 / D chains (1 for D > 256): chain r starts at +0 and adds frames r,
// r + R, .. of the slice in order; column c's sum is chain 0 + chain 1 + .. + chain R - 1, left to right.  It depends on n and D only.
// The handle's block of doubles is Kaldi's layout [n_spk][2][D + 1].

constexpr int CV_SLICE = 1024;     // frames of one work item

struct CvSeg { int64_t row0; int32_t n, pos; };           // n feature rows from row0 sit at positions pos .. pos + n - 1 of their slice
struct CvItem { int32_t seg0, nseg, n, slot; };           // one slice: segments [seg0, seg0 + nseg) of the chunk, n frames, parked in slot `slot`
struct CvRun { int32_t spk, slot0, nslot, pad; double frames; };   // a speaker's slices in one chunk: slots [slot0, slot0 + nslot), their frames

// one chain's pass over a segment: frames p = first, first + R, .. < pos + n of the slice, in order
__device__ __forceinline__ void cv_chain(const float* __restrict__ x, const CvSeg sg, int first, int R, int D, double& s1, double& s2) {
  const int end = sg.n;
  const float* base = x + sg.row0 * D;                  // position p of the slice is row row0 + (p - pos)
  int p = first - sg.pos;
  for (; p + 3 * R < end; p += 4 * R) {                 // four loads in flight, added in order
    const double a = (double)base[(int64_t)p * D], b = (double)base[(int64_t)(p + R) * D];
    const double c = (double)base[(int64_t)(p + 2 * R) * D], d = (double)base[(int64_t)(p + 3 * R) * D];
    s1 += a; s2 += a * a;
    s1 += b; s2 += b * b;
    s1 += c; s2 += c * c;
    s1 += d; s2 += d * d;
  }
  for (; p < end; p += R) {
    const double a = (double)base[(int64_t)p * D];
    s1 += a; s2 += a * a;
  }
}

__global__ __launch_bounds__(256) void k_cmvn_slice(const float* __restrict__ feats, int32_t D, const CvSeg* __restrict__ segs,
                                                    const CvItem* __restrict__ items, double* __restrict__ part) {
  __shared__ double cv_s1[256], cv_s2[256];
  const CvItem it = items[blockIdx.x];
  const int tid = threadIdx.x;
  double* out = part + (int64_t)it.slot * 2 * D;
  if (D > 256) {                                          // one chain per column, the columns strided over the lanes
    for (int c = tid; c < D; c += 256) {
      double s1 = 0.0, s2 = 0.0;
      for (int k = 0; k < it.nseg; ++k) {
        const CvSeg sg = segs[it.seg0 + k];
        cv_chain(feats + c, sg, sg.pos, 1, D, s1, s2);
      }
      out[c] = s1; out[D + c] = s2;
    }
    return;
  }
  const int R = 256 / D;
  const int r = tid / D, c = tid - r * D;
  double s1 = 0.0, s2 = 0.0;
  if (r < R)
    for (int k = 0; k < it.nseg; ++k) {
      const CvSeg sg = segs[it.seg0 + k];
      const int m = (r - sg.pos) % R;                     // the first position >= pos that is r modulo R
      cv_chain(feats + c, sg, sg.pos + (m < 0 ? m + R : m), R, D, s1, s2);
    }
  cv_s1[tid] = s1; cv_s2[tid] = s2;
  __syncthreads();
  if (tid < D) {
    double t1 = cv_s1[tid], t2 = cv_s2[tid];
    for (int q = 1; q < R; ++q) { t1 += cv_s1[q * D + tid]; t2 += cv_s2[q * D + tid]; }
    out[tid] = t1; out[D + tid] = t2;
  }
}

// one thread per (run, element of the speaker's [2][D + 1] block): the run's slices in slot order onto the call's sums
__global__ __launch_bounds__(256) void k_cmvn_reduce(const CvRun* __restrict__ runs, int32_t nruns, const double* __restrict__ part,
                                                     double* __restrict__ call, int32_t D) {
  const int W = 2 * (D + 1);
  const int64_t total = (int64_t)nruns * W, stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const int run = (int)(i / W), e = (int)(i - (int64_t)run * W);
    const CvRun rn = runs[run];
    double* dst = call + (int64_t)rn.spk * W + e;
    if (e == D) { *dst += rn.frames; continue; }          // the count: whole numbers, exact
    if (e == 2 * D + 1) continue;                         // stats[s][1][D] stays 0
    const int col = e < D ? e : e - 1;                    // the parked image is [2][D]
    const double* p = part + (int64_t)rn.slot0 * 2 * D + col;
    double v = *dst;
    for (int k = 0; k < rn.nslot; ++k) v += p[(int64_t)k * 2 * D];
    *dst = v;
  }
}

__global__ __launch_bounds__(256) void k_cmvn_axpy(double* __restrict__ dst, const double* __restrict__ src, double scale, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) dst[i] = __dadd_rn(dst[i], __dmul_rn(scale, src[i]));
}
