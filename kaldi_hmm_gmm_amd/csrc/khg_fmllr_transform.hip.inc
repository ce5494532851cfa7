// transform-feats (khg_utts_transform_feats, DESIGN.md 7l): y = A x + b with W = [A | b] of the utterance's speaker, in float:
// y[d] = b[d]; then y[d] = fmaf(A[d][j], x[j], y[d]) for j = 0 .. D - 1.  One workgroup takes FT_ROWS consecutive rows of ONE utterance:
// its speaker's W and the rows are staged in LDS (coalesced dwords), every thread then owns outputs (row, d) of the row-major block, so
// the stores are coalesced too.  All reads of a block's rows come before its stores and blocks own disjoint rows: src == dst is allowed.
// An utterance without a speaker (utt2spk < 0) is copied (nothing to do in place).
constexpr int FT_ROWS = 64;
struct FtItem { int32_t utt, nrows; int64_t row0; };
// Dynamic LDS: W[D][D + 1] | x[FT_ROWS][D]
__global__ __launch_bounds__(256) void k_fmllr_transform(const FtItem* __restrict__ items, const int32_t* __restrict__ utt2spk, const float* __restrict__ W,
                                                         const float* src, float* dst, int32_t D) {
  extern __shared__ __attribute__((aligned(16))) float ft_lds[];
  const FtItem it = items[blockIdx.x];
  const int spk = utt2spk[it.utt];
  const int D1 = D + 1, tid = threadIdx.x;
  const int64_t base = it.row0 * D;
  const int n = it.nrows * D;
  if (spk < 0) {
    if (src != dst)
      for (int e = tid; e < n; e += 256) dst[base + e] = src[base + e];
    return;
  }
  float* Ws = ft_lds;
  float* xs = Ws + D * D1;
  for (int e = tid; e < D * D1; e += 256) Ws[e] = W[(int64_t)spk * D * D1 + e];
  for (int e = tid; e < n; e += 256) xs[e] = src[base + e];
  __syncthreads();
  for (int e = tid; e < n; e += 256) {
    const int r = e / D, d = e - r * D;
    const float* w = Ws + d * D1;
    const float* x = xs + r * D;
    float y = w[D];
    for (int j = 0; j < D; ++j) y = fmaf(w[j], x[j], y);
    dst[base + e] = y;
  }
}
