// apply-cmvn and add-deltas (khg_utts_apply_cmvn, khg_utts_add_deltas, DESIGN.md 7p) in one tile kernel on the pattern of
// k_lda_splice_transform.  One workgroup takes FT2_ROWS consecutive rows of ONE utterance and stages them with a halo of H = order x
// window rows each side, clamped to the utterance (edge frames are replicated, a neighbour's row is never read): local row l holds
// v[clamp(row0 - H + l)].  v is the row itself, or with a normaliser its CMVN value fl(fl(x scale) + offset) -- a product and a sum,
// each rounded, never fused (Kaldi's MulColsVec then AddVecToRows) -- formed while the tile is staged.  Block i of the output is the
// chain y = 0, y = fmaf(scales[i][j], v[t + j][d], y) over j = -i window .. i window with the zero coefficients skipped (7l's
// transform rule).  Every thread owns whole output elements -- the order + 1 blocks of one (frame, column) -- so no value crosses
// lanes; consecutive lanes write consecutive columns, then the next frame: runs of D floats per block.  apply-cmvn (`apply`: order 0,
// no halo, no LDS, any D) writes the staged value itself, so that a row without a speaker keeps its bytes (the chain would turn -0
// into +0); every element is read by the thread that writes it: that case alone may run in place.
constexpr int FT2_ROWS = 64;
struct Ft2Item { int64_t row0; int32_t nrows, spk; int64_t lo, hi; };   // rows [row0, row0 + nrows) of the utterance whose rows are lo .. hi; spk < 0: no normaliser

__device__ __forceinline__ float ft2_cmvn(float x, float scale, float offset) {
#pragma clang fp contract(off)
  const float t = x * scale;
  return t + offset;
}

// row and column of element e of a row-major [..][D] block without an integer division: (e + 0.5) fl(1 / D) lies within 2^-23 e / D of
// e / D + 0.5 / D, far inside the 0.5 / D to the next whole number for every e < 2^22 (a tile holds fewer than 2^14 elements)
__device__ __forceinline__ int ft2_row(int e, float invD) { return (int)(((float)e + 0.5f) * invD); }

// Dynamic LDS: xs[FT2_ROWS + 2 H][D].  scales: the tables one after the other, table i of 2 i window + 1 floats at i + window i (i - 1);
// a thread takes frame t and column d and walks the blocks i = 0 .. order, so the coefficient and its test against zero are the same
// for the whole wave (scalar loads, a scalar branch) and only the staged values come from LDS.
__global__ __launch_bounds__(256) void k_feat_cmvn_deltas(const Ft2Item* __restrict__ items, const float* __restrict__ norm, const float* __restrict__ scales,
                                                          const float* __restrict__ src, float* __restrict__ dst, int32_t D, int32_t order, int32_t window, int32_t apply) {
  extern __shared__ __attribute__((aligned(16))) float ft2_lds[];
  const Ft2Item it = items[blockIdx.x];
  const int tid = threadIdx.x, H = order * window, nh = it.nrows + 2 * H;
  const float invD = 1.0f / (float)D;
  float* xs = ft2_lds;
  const float* nm = (norm && it.spk >= 0) ? norm + (int64_t)it.spk * 2 * D : nullptr;    // [0][d] offset, [1][d] scale
  if (apply) {                                               // apply-cmvn: the staged value IS the output (a row without a speaker keeps its bytes)
    const int64_t base = it.row0 * D;
    for (int e = tid; e < it.nrows * D; e += 256) {
      const int d = e % D;                                     // (no tile bounds D here: the integer form)
      const float x = src[base + e];
      dst[base + e] = nm ? ft2_cmvn(x, nm[D + d], nm[d]) : x;
    }
    return;
  }
  for (int e = tid; e < nh * D; e += 256) {
    const int l = ft2_row(e, invD), d = e - l * D;
    const int64_t r = min(max(it.row0 - H + l, it.lo), it.hi);
    const float x = src[r * D + d];
    xs[e] = nm ? ft2_cmvn(x, nm[D + d], nm[d]) : x;
  }
  __syncthreads();
  const int OD = D * (order + 1), n = it.nrows * D;
  for (int e = tid; e < n; e += 256) {
    const int t = ft2_row(e, invD), d = e - t * D;
    const float* v = xs + (t + H) * D + d;                  // v[j D]: frame t + j of the block
    float* o = dst + (it.row0 + t) * OD + d;
    for (int i = 0; i <= order; ++i) {
      const int Hi = i * window;
      const float* s = scales + i + window * i * (i - 1) + Hi;    // s[j], j = -Hi .. Hi
      float y = 0.0f;
      for (int j = -Hi; j <= Hi; ++j) {
        const float a = s[j];
        if (a != 0.0f) y = fmaf(a, v[j * D], y);
      }
      o[i * D] = y;
    }
  }
}
