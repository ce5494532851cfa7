// K1C (khg_lattices_rescore, KHG_RESCORE_CELLS; DESIGN.md 7j): log-likelihoods of the distinct (feature row, pdf) cells a batch of
// lattices names, and nothing else.  The caller (khg_lattices.hip, which alone knows a lattice chunk) has flattened every arc into
//   key = (pdf << 32) | row      val = the arc's number in the handle's arc order      (an arc that names no cell: key = P << 32)
// in u->rc_keys_d / u->rc_vals_d.  From there, on the context's stream, without a synchronisation:
//   sort     hipcub::DeviceRadixSort::SortPairs on bits 0 .. 32 + bits(P): stable, so the result is reproducible
//   heads    flag = the key differs from its predecessor; an inclusive scan numbers the cells; the heads' rows are compacted; a lower
//            bound per pdf over the sorted keys gives the per-pdf bounds of the cell list and, scanned, the work items
//   score    one workgroup per (pdf, slice of K1C_CS of its cells): the pdf's rows staged into LDS once, a wave per cell (two cells
//            per wave where the pdf has <= 32 Gaussians), lanes over the Gaussians, the log-sum-exp across the wave
//   scatter  one thread per sorted entry: acoustic_cost[val] = -(acoustic_scale * cell[index])
// Count, scan, fill: no atomics but the error word's.
//
// The value of a cell.  Per Gaussian the chain of the strict-fp32 K1 (include/khg_hip.h, KHG_K1_FP32_PDF; oracle.loglikes(fma_order =
// True) bit for bit): s = gconst; for d in steps of two: fma(M[d], x[d]), fma(M[d+1], x[d+1]), fma(-V[d]/2, fl(x[d]^2)),
// fma(-V[d+1]/2, fl(x[d+1]^2)).  Gaussian g of the pdf sits on lane g % W, W = 32 for a pdf of <= 32 Gaussians and 64 otherwise; a
// lane folds its Gaussians g = lane, lane + W, ... in that order into a running (max, sum of exp); the lanes' pairs are combined by an
// xor butterfly (max, then the rescaled sums; offsets W/2 .. 1), whose additions are commutative pairs: every lane ends with the same
// bits.  The order depends on the pdf's number of Gaussians alone -- not on where the cell sits in its slice, not on the batch.
#include <hipcub/hipcub.hpp>

constexpr int K1C_NT = 256;        // threads of a scoring workgroup: four waves
constexpr int K1C_CS = 128;        // cells per work item
constexpr int K1C_LDS_MAX = 64 << 10;   // a pdf's rows are staged into LDS up to this many bytes; a larger pdf is read from HBM (same bits)

__global__ __launch_bounds__(256) void k1c_heads(const uint64_t* __restrict__ keys, int32_t n, uint64_t sentinel, int32_t* __restrict__ flag) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const uint64_t k = keys[i];
    flag[i] = (k < sentinel && (i == 0 || keys[i - 1] != k)) ? 1 : 0;
  }
}
__global__ __launch_bounds__(256) void k1c_fill(const uint64_t* __restrict__ keys, const int32_t* __restrict__ flag, const int32_t* __restrict__ inc,
                                               int32_t n, int32_t* __restrict__ cell_row) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride)
    if (flag[i]) cell_row[inc[i] - 1] = (int32_t)(uint32_t)(keys[i] & 0xffffffffu);
}
// One workgroup: cell_start[p] = cells of the pdfs before p (p = 0 .. P; [P] is the number of cells), item_off[p] = work items before
// p (slices of K1C_CS cells), stats = { entries, entries that name a cell, cells, work items }.
__global__ __launch_bounds__(1024) void k1c_bounds(const uint64_t* __restrict__ keys, const int32_t* __restrict__ inc, int32_t n, int32_t P,
                                                   int32_t* __restrict__ cell_start, int32_t* __restrict__ item_off, int64_t* __restrict__ stats) {
  __shared__ int32_t part[1024];
  const int t = (int)threadIdx.x;
  const int per = (P + 1 + 1023) / 1024;
  const int p0 = min(t * per, P + 1), p1 = min(p0 + per, P + 1);
  for (int p = p0; p < p1; ++p) {
    const uint64_t want = (uint64_t)p << 32;
    int32_t lo = 0, hi = n;                      // first entry with key >= want
    while (lo < hi) {
      const int32_t mid = lo + ((hi - lo) >> 1);
      if (keys[mid] < want) lo = mid + 1; else hi = mid;
    }
    cell_start[p] = lo == 0 ? 0 : inc[lo - 1];
    if (p == P) { stats[0] = n; stats[1] = lo; }
  }
  __syncthreads();
  int32_t sum = 0;
  for (int p = p0; p < p1 && p < P; ++p) sum += (cell_start[p + 1] - cell_start[p] + K1C_CS - 1) / K1C_CS;
  part[t] = sum;
  __syncthreads();
  if (t == 0) {
    int32_t acc = 0;
    for (int k = 0; k < 1024; ++k) { const int32_t v = part[k]; part[k] = acc; acc += v; }
    stats[2] = cell_start[P]; stats[3] = acc;
    item_off[P] = acc;
  }
  __syncthreads();
  int32_t acc = part[t];
  for (int p = p0; p < p1 && p < P; ++p) {
    item_off[p] = acc;
    acc += (cell_start[p + 1] - cell_start[p] + K1C_CS - 1) / K1C_CS;
  }
}

struct K1cScore {
  const float* feats; int32_t D, P;
  const int32_t* gauss_off; const float *gconsts, *miv, *iv;
  const int32_t *cell_start, *item_off, *cell_row;
  float* cell;
  int32_t lds_floats;           // dynamic LDS of the launch, in floats
  int32_t* err_flag;
};
// the chain of Gaussian g (row g0 + g of the model) on feature row x; STAGED: the pdf's rows in LDS as [d][G] M | [d][G] -V/2
template <bool STAGED>
__device__ __forceinline__ float k1c_chain(const K1cScore& a, const float* __restrict__ w, int g0, int G, int g, const float* __restrict__ x) {
  const int D = a.D;
  float s = a.gconsts[g0 + g];
  const float* pm = STAGED ? w + g : a.miv + (int64_t)(g0 + g) * D;
  const float* pv = STAGED ? w + (int64_t)G * D + g : a.iv + (int64_t)(g0 + g) * D;
  const int st = STAGED ? G : 1;
  for (int d = 0; d < D; d += 2) {
    const bool two = d + 1 < D;
    const float x0 = x[d], x1 = two ? x[d + 1] : 0.0f;
    const float m0 = pm[(int64_t)d * st], m1 = two ? pm[(int64_t)(d + 1) * st] : 0.0f;
    float v0 = pv[(int64_t)d * st], v1 = two ? pv[(int64_t)(d + 1) * st] : 0.0f;
    if (!STAGED) { v0 = -0.5f * v0; v1 = -0.5f * v1; }       // (exact)
    s = __fmaf_rn(m0, x0, s);
    if (two) s = __fmaf_rn(m1, x1, s);
    s = __fmaf_rn(v0, __fmul_rn(x0, x0), s);
    if (two) s = __fmaf_rn(v1, __fmul_rn(x1, x1), s);
  }
  return s;
}
// the cell (row, pdf) on the W lanes of one wave (W = 32: a half); `on`: this half has a cell (the other lanes run along, harmless)
template <bool STAGED, int W>
__device__ __forceinline__ float k1c_cell(const K1cScore& a, const float* __restrict__ w, int g0, int G, int gl, const float* __restrict__ x) {
  float mx = -INFINITY, sm = 0.0f;
  for (int g = gl; g < G; g += W) {            // (a lane without a Gaussian keeps (-inf, 0))
    const float v = k1c_chain<STAGED>(a, w, g0, G, g, x);
    const float nm = fmaxf(mx, v);
    sm = __fmaf_rn(sm, expf(mx - nm), expf(v - nm));
    mx = nm;
  }
  float M = mx;
#pragma unroll
  for (int o = W / 2; o >= 1; o >>= 1) M = fmaxf(M, __shfl_xor(M, o));
  float S = sm == 0.0f ? 0.0f : __fmul_rn(sm, expf(mx - M));
#pragma unroll
  for (int o = W / 2; o >= 1; o >>= 1) S = __fadd_rn(S, __shfl_xor(S, o));
  return __fadd_rn(M, logf(S));
}
__global__ __launch_bounds__(K1C_NT) void k1c_score(K1cScore a) {
  extern __shared__ float k1c_lds[];
  const int b = (int)blockIdx.x;
  if (b >= a.item_off[a.P]) return;
  int lo = 0, hi = a.P;                          // item_off[lo] <= b < item_off[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.item_off[mid] <= b) lo = mid; else hi = mid;
  }
  const int p = lo;
  const int g0 = a.gauss_off[p], G = a.gauss_off[p + 1] - g0, D = a.D;
  const int c0 = a.cell_start[p] + (b - a.item_off[p]) * K1C_CS, c1 = min(c0 + K1C_CS, a.cell_start[p + 1]);
  const bool staged = 2 * (int64_t)G * D <= (int64_t)a.lds_floats;
  if (staged) {
    for (int i = (int)threadIdx.x; i < G * D; i += K1C_NT) {
      const int g = i / D, d = i - g * D;
      k1c_lds[d * G + g] = a.miv[(int64_t)g0 * D + i];
      k1c_lds[G * D + d * G + g] = -0.5f * a.iv[(int64_t)g0 * D + i];
    }
  }
  __syncthreads();
  const int wv = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  constexpr int NW = K1C_NT / 64;
  if (G <= 32) {
    const int h = lane >> 5, gl = lane & 31;
    for (int c = c0 + 2 * wv; c < c1; c += 2 * NW) {
      const bool on = c + h < c1;
      const int cc = on ? c + h : c;
      const float* x = a.feats + (int64_t)a.cell_row[cc] * D;
      const float v = staged ? k1c_cell<true, 32>(a, k1c_lds, g0, G, gl, x) : k1c_cell<false, 32>(a, k1c_lds, g0, G, gl, x);
      if (on && gl == 0) {
        a.cell[cc] = v;
        if (!(fabsf(v) <= 3.0e38f)) atomicOr(a.err_flag, 1);
      }
    }
  } else {
    for (int c = c0 + wv; c < c1; c += NW) {
      const int row = __builtin_amdgcn_readfirstlane(a.cell_row[c]);      // uniform: the row's loads may stay scalar
      const float* x = a.feats + (int64_t)row * D;
      const float v = staged ? k1c_cell<true, 64>(a, k1c_lds, g0, G, lane, x) : k1c_cell<false, 64>(a, k1c_lds, g0, G, lane, x);
      if (lane == 0) {
        a.cell[c] = v;
        if (!(fabsf(v) <= 3.0e38f)) atomicOr(a.err_flag, 1);
      }
    }
  }
}

// where the arcs of the output handle are: chunk k holds the arcs base[k] .. base[k + 1] of the handle's arc order
struct K1cTargets { const int64_t* base; float* const* ac; int32_t n; };
__global__ __launch_bounds__(256) void k1c_scatter(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, const int32_t* __restrict__ inc,
                                                  const float* __restrict__ cell, int32_t n, uint64_t sentinel, float scale, K1cTargets t) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    if (keys[i] >= sentinel) continue;
    const int64_t arc = vals[i];
    int lo = 0, hi = t.n;                        // base[lo] <= arc < base[hi]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (t.base[mid] <= arc) lo = mid; else hi = mid;
    }
    t.ac[lo][arc - t.base[lo]] = -__fmul_rn(scale, cell[inc[i] - 1]);
  }
}

namespace {
// the scratch on the utterance set: by the arc count (kept, grown on demand) and by the model's pdfs
int k1_cells_scratch(khg_utts* u, int64_t NA, int32_t P) {
  int rc = KHG_OK;
  if ((size_t)NA > u->rc_cap) {
    DEVFREE(u->rc_keys_d); DEVFREE(u->rc_keys_out_d); DEVFREE(u->rc_vals_d); DEVFREE(u->rc_vals_out_d); DEVFREE(u->rc_flag_d); DEVFREE(u->rc_inc_d);
    DEVFREE(u->rc_row_d); DEVFREE(u->rc_cell_d);
    u->rc_cap = 0;
    const size_t n = (size_t)NA;
    if (!rc) rc = u_alloc(u, &u->rc_keys_d, n);
    if (!rc) rc = u_alloc(u, &u->rc_keys_out_d, n);
    if (!rc) rc = u_alloc(u, &u->rc_vals_d, n);
    if (!rc) rc = u_alloc(u, &u->rc_vals_out_d, n);
    if (!rc) rc = u_alloc(u, &u->rc_flag_d, n);
    if (!rc) rc = u_alloc(u, &u->rc_inc_d, n);
    if (!rc) rc = u_alloc(u, &u->rc_row_d, n);
    if (!rc) rc = u_alloc(u, &u->rc_cell_d, n);
    if (rc) return rc;
    u->rc_cap = n;
  }
  if (u->rc_P != P) {
    DEVFREE(u->rc_cell_start_d); DEVFREE(u->rc_item_off_d);
    u->rc_P = -1;
    rc = u_alloc(u, &u->rc_cell_start_d, (size_t)P + 1);
    if (!rc) rc = u_alloc(u, &u->rc_item_off_d, (size_t)P + 1);
    if (rc) return rc;
    u->rc_P = P;
  }
  if (!u->rc_stats_d) rc = u_alloc(u, &u->rc_stats_d, 4);
  return rc;
}

// sort .. scatter over the NA flattened arcs in u->rc_keys_d / u->rc_vals_d; stats_h[4] (pinned or pageable: the caller synchronises
// before it reads) = { entries, entries that name a cell, cells, work items }
int k1_cells_run(khg_ctx* ctx, const khg_model* m, khg_utts* u, int64_t NA, float scale, const K1cTargets& tg, int64_t* stats_h) {
  const int n = (int)NA, P = m->P;
  const uint64_t sentinel = (uint64_t)P << 32;
  int bits = 1;
  while ((1 << bits) <= P) ++bits;               // pdfs are 0 .. P
  const int gb = (int)std::min<int64_t>(4096, (NA + 255) / 256);
  size_t need_sort = 0, need_scan = 0;
  HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, need_sort, u->rc_keys_d, u->rc_keys_out_d, u->rc_vals_d, u->rc_vals_out_d, n, 0, 32 + bits, ctx->stream));
  HIPCHK(hipcub::DeviceScan::InclusiveSum(nullptr, need_scan, u->rc_flag_d, u->rc_inc_d, n, ctx->stream));
  const size_t need = std::max(need_sort, need_scan);
  if (need > u->rc_tmp_bytes) {
    DEVFREE(u->rc_tmp_d);
    u->rc_tmp_bytes = 0;
    int rt = u_alloc(u, reinterpret_cast<char**>(&u->rc_tmp_d), need);
    if (rt) return rt;
    u->rc_tmp_bytes = need;
  }
  {
    KernelTimer kt(ctx, "k1c_sort");
    need_sort = u->rc_tmp_bytes;
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(u->rc_tmp_d, need_sort, u->rc_keys_d, u->rc_keys_out_d, u->rc_vals_d, u->rc_vals_out_d, n, 0, 32 + bits, ctx->stream));
  }
  {
    KernelTimer kt(ctx, "k1c_heads");
    KHG_LAUNCH(ctx, k1c_heads, dim3(gb), dim3(256), 0, ctx->stream, u->rc_keys_out_d, n, sentinel, u->rc_flag_d);
    need_scan = u->rc_tmp_bytes;
    HIPCHK(hipcub::DeviceScan::InclusiveSum(u->rc_tmp_d, need_scan, u->rc_flag_d, u->rc_inc_d, n, ctx->stream));
    KHG_LAUNCH(ctx, k1c_fill, dim3(gb), dim3(256), 0, ctx->stream, u->rc_keys_out_d, u->rc_flag_d, u->rc_inc_d, n, u->rc_row_d);
    KHG_LAUNCH(ctx, k1c_bounds, dim3(1), dim3(1024), 0, ctx->stream, u->rc_keys_out_d, u->rc_inc_d, n, P, u->rc_cell_start_d, u->rc_item_off_d, u->rc_stats_d);
    HIPCHK(hipGetLastError());
  }
  {
    K1cScore a;
    a.feats = u->feats_d; a.D = m->D; a.P = P; a.gauss_off = m->gauss_off_d; a.gconsts = m->gconsts_d; a.miv = m->miv_d; a.iv = m->iv_d;
    a.cell_start = u->rc_cell_start_d; a.item_off = u->rc_item_off_d; a.cell_row = u->rc_row_d; a.cell = u->rc_cell_d; a.err_flag = ctx->err_flag_d;
    int64_t maxgd = 0;
    for (int p = 0; p < P; ++p) maxgd = std::max<int64_t>(maxgd, (int64_t)(m->gauss_off[(size_t)p + 1] - m->gauss_off[(size_t)p]) * m->D);
    const size_t lds = (size_t)std::min<int64_t>(K1C_LDS_MAX, 8 * maxgd);
    a.lds_floats = (int32_t)(lds / 4);
    { int rc = khg_lds_attribute((const void*)k1c_score, lds); if (rc) return rc; }
    // every pdf may leave one short slice: an upper bound from the arc count and P alone (the cell counts stay on the device); a
    // workgroup past the last item returns at once
    const int64_t max_items = (int64_t)P + NA / K1C_CS + 1;
    KernelTimer kt(ctx, "k1c_score");
    KHG_LAUNCH(ctx, k1c_score, dim3((unsigned)max_items), dim3(K1C_NT), lds, ctx->stream, a);
    HIPCHK(hipGetLastError());
  }
  {
    KernelTimer kt(ctx, "k1c_scatter");
    KHG_LAUNCH(ctx, k1c_scatter, dim3(gb), dim3(256), 0, ctx->stream, u->rc_keys_out_d, u->rc_vals_out_d, u->rc_inc_d, u->rc_cell_d, n, sentinel, scale, tg);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipMemcpyAsync(stats_h, u->rc_stats_d, 32, hipMemcpyDeviceToHost, ctx->stream));
  return KHG_OK;
}
}  // namespace
