// splice-feats | transform-feats (khg_utts_splice_transform_feats, DESIGN.md 7n): y = M z (+ the offset column) of the spliced frame
// z_t[k D + j] = x[clamp(t + k - L, 0, T - 1)][j], in float by 7l's transform rule: y[r] = M[r][Dz] (0 without the column), then
// y[r] = fmaf(M[r][c], z[c], y[r]) for c = 0 .. Dz - 1.  One workgroup takes LT_ROWS consecutive rows of ONE utterance: M and the rows
// with their halo of L rows before and R after (clamped to the utterance, so the edge frames are replicated and no neighbour's row is
// read) are staged in LDS; local row l holds x[clamp(row0 - L + l)], so z_t[k D + j] of the block's frame t is xs[t + k][j].  Every
// thread owns whole chains (row, r) of the row-major output block: no value crosses lanes, the stores are coalesced.  Without M the
// same gather is copied out: splice-feats.
constexpr int LT_ROWS = 64;
struct LtItem { int64_t row0; int32_t nrows, lo, hi, pad; };   // rows [row0, row0 + nrows) of the utterance whose rows are lo .. hi
// Dynamic LDS: xs[LT_ROWS + L + R][D] | Ms[out_dim][MS], MS = (Dz + 1) | 1 (odd: the lanes' rows of M spread over the banks)
__global__ __launch_bounds__(256) void k_lda_splice_transform(const LtItem* __restrict__ items, const float* __restrict__ M, int32_t has_offset,
                                                              const float* __restrict__ src, float* __restrict__ dst, int32_t D, int32_t L, int32_t R,
                                                              int32_t out_dim, int32_t MS) {
  extern __shared__ __attribute__((aligned(16))) float lt_lds[];
  const LtItem it = items[blockIdx.x];
  const int tid = threadIdx.x, Dz = D * (L + R + 1), nh = it.nrows + L + R;
  float* xs = lt_lds;
  float* Ms = xs + (LT_ROWS + L + R) * D;
  for (int e = tid; e < nh * D; e += 256) {
    const int l = e / D, j = e - l * D;
    const int64_t r = min(max(it.row0 - L + l, (int64_t)it.lo), (int64_t)it.hi);
    xs[e] = src[r * D + j];
  }
  if (M) {
    const int MW = Dz + (has_offset ? 1 : 0);
    for (int e = tid; e < out_dim * MW; e += 256) {
      const int r = e / MW, c = e - r * MW;
      Ms[r * MS + c] = M[e];
    }
  }
  __syncthreads();
  const int n = it.nrows * out_dim;
  const int64_t base = it.row0 * out_dim;
  if (!M) {                                                  // out_dim == Dz: the spliced rows themselves
    for (int e = tid; e < n; e += 256) {
      const int t = e / Dz, c = e - t * Dz;                  // c = k D + j -> xs[(t + k) D + j] = xs[t D + c]
      dst[base + e] = xs[t * D + c];
    }
    return;
  }
  for (int e = tid; e < n; e += 256) {
    const int t = e / out_dim, r = e - t * out_dim;
    const float* m = Ms + r * MS;
    const float* z = xs + t * D;                             // z[c], c = 0 .. Dz - 1, is contiguous: (t + k) D + j = t D + c
    float y = has_offset ? m[Dz] : 0.0f;
    for (int c = 0; c < Dz; ++c) y = fmaf(m[c], z[c], y);
    dst[base + e] = y;
  }
}
