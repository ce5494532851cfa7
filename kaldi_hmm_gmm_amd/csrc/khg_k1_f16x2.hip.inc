// K1 on the fp16 matrix cores at fp32 accuracy ("f16x2"): the same log-likelihoods as the other K1 forms with THREE
// partial products per term (the bf16x3 form of rounds 2-5, six products of three exact bf16 pieces, was removed in round 6).
//
// Reference: decodable-am-diag-gmm.cc:55-61, diag-gmm.cc:167-189, eigen.cc:14-18 (as in the other K1 forms).
//
// Arithmetic.  The contraction is  C[g][t] = gconst[g] + sum_k W[g][k] X[k][t],  W = [M | -0.5 V],  X = [x | fl(x^2)],
// K = 2 D.  Per k the two operands are rescaled by an exact power of two, w' = w 2^-e_k, x' = x 2^e_k (the products do not
// change), and each is written as
//     v = v1 + v2 2^-11,    v1 = fp16(v)  (round to nearest; fp16's significand is 11 bits: |v - v1| <= 2^-11 |v|),
//                           v2 = fp16((v - v1) 2^11)     -- the residual PRE-SCALED to v's own magnitude, so it is an
//                                                           ordinary fp16 number (no subnormal residuals for |v| >= 2^-13),
// which represents v to 2^-23 |v| (the residual has <= 13 significant bits on v's grid; rounding it to 11 loses at most the
// last one): 11 + 11 bits, one short of fp32's own rounding.  The term w x is evaluated as
//     acc_main  = gconst + sum w1 x1,      acc_cross = sum (w1 x2 + w2 x1),       C = acc_main + acc_cross 2^-11
// on v_mfma_f32_32x32x16_f16 (exact fp16 x fp16 products, fp32 accumulators); the dropped w2 x2 is <= 2^-22 of the term.
// Worst case |error| <= 2^-21 sum |w x| + the fp32 accumulation ("about 22-bit operands"; tests/test_split_arithmetic.py pins
// these bounds on the CPU).  tools/probe_f16x2.hip (profiles/r2_probe_f16x2.txt)
// measures |error| / B against fp64 on three kinds of data (the bench's model; variances 1e-3..1e2 with means +-50; features
// ~1e-3): max 3.0e-7, rms 5.1e-8 -- below the fp32 fmaf chain of the fp32-MFMA kernels (7.4e-7 / 1.1e-7) on every one.
// fp16 subnormal operands survive the MFMA (same probe), which only matters for |v'| < 2^-14.
//
// Since round 3 this is the SECOND choice: khg_k1_f16x2s.hip.inc (one accumulator, residuals not pre-scaled, feature tiles in
// LDS and pdfs dealt to waves) is the default and hands over to this form when the absolute part of its error bound is too
// large for the model at hand.
//
// Scaling.  2^e_k = sqrt(max_g |w_gk| / max_t |x_tk|) rounded to a power of two: both scaled operands then peak at
// sqrt(max|w| max|x|), far inside fp16's range (65504) for any model the form accepts (below).  The features' planes are
// packed once with the scales of the first model; a later model re-uses them while it still fits (the W image is re-packed
// with the model anyway), else the planes are re-packed (5 ms at 30 M frames).
//
// Domain.  The log-sum-exp evaluates 2^((c - max) log2 e) as exp2(fma(c, L2E, -fl(max L2E))) (one VALU instruction per
// Gaussian; k1_exp2_le1): the rounding of max L2E shifts every term alike -- harmless, 6e-8 |max| in the result -- as long
// as the shift stays inside fp32's exponent range, i.e. |c| well below 2^24 x 100.  The host therefore uses this form (and
// bf16x3) only while  max |gconst| + sum_k max |w_k| max |x_k| <= 2^28  (exact maxima of the model and of the utterance
// set; ~1e3 for ordinary models) and runs the fp32-MFMA forms, whose log-sum-exp subtracts first, for anything larger.
//
// Shape: utterance-major ( B fragments of <= 2 32-frame tiles per wave in registers; W tiles stream
// through two LDS slots by LDS-DMA, one workgroup barrier per group of tiles; online log-sum-exp of a chain interleaved with
// the MFMAs of the next).  A W tile is 2 x KS + 1 KiB (11 KiB at D <= 40, against 16), a chain 3 KS MFMAs (15, against 30).

#ifndef K1H_VHEAD
#define K1H_VHEAD 6      // VALU instructions of the previous chain's epilogue ahead of the first MFMA ...
#define K1H_VPER5 6      // ... and behind every MFMA (KS = 5: 15 MFMAs per chain; KS = 10: 30)
#define K1H_VPER10 3
#endif
#ifndef K1H_GROUP5
#define K1H_GROUP5 6     // W tiles per LDS slot / barrier interval: 66 KiB (KS = 5), 63 KiB (KS = 10)
#define K1H_GROUP10 3
#endif
typedef _Float16 k1h_f16x8 __attribute__((ext_vector_type(8)));

__host__ __device__ constexpr int k1h_tile_pieces(int KS) { return 2 * KS + 1; }        // 1-KiB pieces: 2 x KS fragments + [gconst 32 | pad]
__host__ __device__ constexpr int k1h_tile_bytes(int KS) { return k1h_tile_pieces(KS) * 1024; }
__host__ __device__ constexpr int k1h_group(int KS) { return KS == 5 ? K1H_GROUP5 : K1H_GROUP10; }
__host__ __device__ constexpr int k1h_lds_bytes(int KS) { return 2 * k1h_group(KS) * k1h_tile_bytes(KS); }

struct K1hArgs {
  const k1b_u32x4* xh;            // per 32-frame tile: [piece 2][step KS][lane 64] 16-byte B fragments
  const int64_t* utt_xtile_off;   // [U+1] first 32-frame tile of each utterance
  const int64_t* frame_off;       // [U+1]
  const K1bChunk* chunks;
  const char* wimg;               // k1h_tile_bytes(KS) per 32-Gaussian tile
  const int64_t* utt_tile_off;    // [U+1] offsets into utt_tiles
  const int32_t* utt_tiles;       // walk entries (see khg_k1_loglikes.hip.inc)
  float* ll;
  const int64_t* ll_off;
  int32_t* err_flag;
  int32_t dbg;                    // KHG_K1B_DBG (experiments): 2 = skip the log-sum-exp updates (wrong results), 8 = no shared remainder tiles
  uint64_t* tbuf;                 // -DK1H_TIMING builds: 8 counters per wave (see the end of k1h_wave), or null
};

__device__ __forceinline__ float k1_max3v(float a, float b, float c) { return __builtin_fmaxf(__builtin_fmaxf(a, b), c); }

__device__ __forceinline__ void k1h_split2(float v, _Float16& a, _Float16& b) {
  a = (_Float16)v;
  b = (_Float16)((v - (float)a) * 2048.0f);     // exact: the residual has <= 13 significant bits
}

// per-column max |value| of a row-major [n][D] matrix (D <= 128), as the bits of a non-negative float.  -inf is skipped (a
// zero-weight Gaussian's gconst); NaN / +inf come out as +inf.
__global__ __launch_bounds__(256) void k1h_absmax(const float* __restrict__ a, int64_t n, int D, uint32_t* __restrict__ out) {
  const int d = threadIdx.x & 127, sub = threadIdx.x >> 7;
  float m = 0.0f;
  if (d < D)
    for (int64_t r = (int64_t)blockIdx.x * 2 + sub; r < n; r += (int64_t)gridDim.x * 2) {
      const float v = a[r * D + d];
      if (v == -INFINITY) continue;
      m = (fabsf(v) <= 3.0e38f) ? fmaxf(m, fabsf(v)) : INFINITY;
    }
  if (d < D && m > 0.0f) atomicMax(out + d, __float_as_uint(m));
}

// k index of element e of lane's fragment at step s: 16 s + 8 (lane >> 5) + e;  k = 2 d + kind (kind 0: M . x, 1: -V/2 . x^2)

// model -> f16x2 W image, one workgroup per 32-Gaussian tile; ex[k]: the scale exponents (w' = w 2^-ex)
template <int KS>
__global__ __launch_bounds__(256) void k0h_pack_tiles(const float* __restrict__ gconsts, const float* __restrict__ miv,
                                                       const float* __restrict__ iv, const int32_t* __restrict__ gauss_off,
                                                       const int32_t* __restrict__ pdf_tile_off, const int32_t* __restrict__ tile_pdf,
                                                       int D, const int32_t* __restrict__ ex, char* __restrict__ wimg) {
  constexpr int TILEB = k1h_tile_bytes(KS);
  const int t = blockIdx.x, p = tile_pdf[t];
  const int g_first = gauss_off[p] + 32 * (t - pdf_tile_off[p]);
  const int nrow = min(32, gauss_off[p + 1] - g_first);
  char* img = wimg + (size_t)t * TILEB;
  for (int f = threadIdx.x; f < KS * 64; f += 256) {       // one (step, lane) fragment per thread: two 16-byte pieces
    const int s = f >> 6, lane = f & 63, g = lane & 31, kb = lane >> 5;
    k1h_f16x8 p0, p1;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int k = 16 * s + 8 * kb + e, d = k >> 1;
      float v = 0.0f;
      if (g < nrow && d < D) { const size_t src = (size_t)(g_first + g) * D + d; v = ldexpf((k & 1) ? -0.5f * iv[src] : miv[src], -ex[k]); }
      _Float16 a, b;
      k1h_split2(v, a, b);
      p0[e] = a; p1[e] = b;
    }
    *reinterpret_cast<k1h_f16x8*>(img + ((0 * KS + s) * 64 + lane) * 16) = p0;
    *reinterpret_cast<k1h_f16x8*>(img + ((1 * KS + s) * 64 + lane) * 16) = p1;
  }
  float* gc = reinterpret_cast<float*>(img + 2 * KS * 1024);
  for (int i = threadIdx.x; i < 256; i += 256) gc[i] = i < nrow ? gconsts[g_first + i] : (i < 32 ? -INFINITY : 0.0f);
}

// features -> f16x2 B fragments, one thread per (32-frame tile, step, lane); x' = x 2^ex
template <int KS>
__global__ void k1h_pack_x(const float* __restrict__ feats, const int64_t* __restrict__ frame_off,
                           const int64_t* __restrict__ utt_xtile_off, const int32_t* __restrict__ xtile_utt,
                           int64_t n_xtiles, int D, const int32_t* __restrict__ ex, k1b_u32x4* __restrict__ xh) {
  const int64_t nfrag = n_xtiles * (KS * 64);
  for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < nfrag; f += (int64_t)gridDim.x * blockDim.x) {
    const int64_t xt = f / (KS * 64);
    const int w = (int)(f - xt * (KS * 64)), s = w >> 6, lane = w & 63, col = lane & 31, kb = lane >> 5;
    const int u = xtile_utt[xt];
    const int64_t f0 = frame_off[u];
    const int T = (int)(frame_off[u + 1] - f0);
    int t = (int)(xt - utt_xtile_off[u]) * 32 + col;
    if (t > T - 1) t = T - 1;               // padded frames repeat the last one (their scores land in the row padding)
    const float* xp = feats + (f0 + t) * (int64_t)D;
    k1h_f16x8 p0, p1;
#pragma unroll
    for (int e = 0; e < 8; e += 2) {
      const int k = 16 * s + 8 * kb + e, d = k >> 1;
      const float x = d < D ? xp[d] : 0.0f;
      const float xx = x * x;               // rounded to fp32 like the reference's squared features
      _Float16 a, b;
      k1h_split2(ldexpf(x, ex[k]), a, b);      p0[e] = a; p1[e] = b;
      k1h_split2(ldexpf(xx, ex[k + 1]), a, b); p0[e + 1] = a; p1[e + 1] = b;
    }
    k1b_u32x4* dst = xh + xt * (2 * KS * 64);
    dst[(0 * KS + s) * 64 + lane] = __builtin_bit_cast(k1b_u32x4, p0);
    dst[(1 * KS + s) * 64 + lane] = __builtin_bit_cast(k1b_u32x4, p1);
  }
}

// One wave's walk with a compile-time number NT of slots (see k1b_wave: same dealing, same barriers).
template <int KS, int NT>
__device__ __forceinline__ void k1h_wave(const K1hArgs& a, const K1bChunk& ck, char* lds, const int wave, const K1bWork wk) {
  constexpr int TILEB = k1h_tile_bytes(KS);
  constexpr int PPT = k1h_tile_pieces(KS);
  constexpr int G = k1h_group(KS);             // W tiles per LDS slot / barrier interval
  constexpr int SLOTB = G * TILEB;
  constexpr int NX = NT > 0 ? NT : 1;
  constexpr int VPER = KS == 5 ? K1H_VPER5 : K1H_VPER10;
  constexpr float L2E = 1.44269504088896340736f, LN2 = 0.69314718055994530942f;
  const int lane = threadIdx.x & 63;
  const int col = lane & 31, kb = lane >> 5;
  const int u = ck.utt;
  const int64_t f0 = a.frame_off[u];
  const int T = (int)(a.frame_off[u + 1] - f0);
  const int tpad = (T + 31) & ~31;

  // ---- B operands of my tiles: resident in registers ----
  k1h_f16x8 xb[NX][2][KS];
#pragma unroll
  for (int f = 0; f < NT; ++f) {
    const k1b_u32x4* src = a.xh + (a.utt_xtile_off[u] + ck.tile0 + wk.tile[f]) * (int64_t)(2 * KS * 64) + lane;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int s = 0; s < KS; ++s) xb[f][p][s] = __builtin_bit_cast(k1h_f16x8, src[(p * KS + s) * 64]);
  }
  // complete before the loop, as far as the compiler's wait-count tracking goes (see k1b_wave)
#pragma unroll
  for (int f = 0; f < NT; ++f)
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int s = 0; s < KS; ++s) asm volatile("" ::"v"(xb[f][p][s]));
  float* llu = a.ll + a.ll_off[u];

  // LDS-DMA of one W tile: 1 KiB per wave-instruction; the PPT pieces of a tile are dealt to the 8 waves starting at a
  // wave that rotates with the tile's place in the group (PPT is not a multiple of 8)
  const uint32_t lane_b = (uint32_t)lane * 16u;
  auto dma_tile = [&](int tile, int slot, int sub) {
    const char* src = a.wimg + (int64_t)tile * TILEB;
    const int w0 = (wave + 3 * sub) & 7;
#pragma unroll
    for (int i = 0; i < (PPT + 7) / 8; ++i) {
      const int piece = w0 + 8 * i;
      if (piece < PPT)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + piece * 1024 + lane_b),
                                         (__attribute__((address_space(3))) void*)(lds + slot * SLOTB + sub * TILEB + piece * 1024), 16, 0, 0);
    }
  };

  // walk entries: wave-uniform scalar loads (inline asm; see k1b_wave)
  const int64_t tl0 = (int64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)a.utt_tile_off[u]) | ((int64_t)__builtin_amdgcn_readfirstlane((int)(a.utt_tile_off[u] >> 32)) << 32);
  const int ntl = __builtin_amdgcn_readfirstlane((int)(a.utt_tile_off[u + 1] - a.utt_tile_off[u]));
  const int32_t* tl = a.utt_tiles + tl0;
  auto sload = [&](int i) {                    // entry i (clamped); asynchronous
    const int32_t* ptr = tl + (i < ntl ? i : (ntl > 0 ? ntl - 1 : 0));
    int v;
    asm volatile("s_load_dword %0, %1, 0x0" : "=s"(v) : "s"(ptr));
    return v;
  };
  auto sload_wait = [&](int& v) { asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(v)::"memory"); };
  const int nit = (ntl + G - 1) / G;
  int eg[G], en[G];
  auto sload_group = [&](int g, int (&dst)[G]) {
#pragma unroll
    for (int t = 0; t < G; ++t) dst[t] = sload(G * g + t);
  };
  auto wait_group = [&](int (&v)[G]) {
#pragma unroll
    for (int t = 0; t < G; ++t) sload_wait(v[t]);
  };
  auto dma_group = [&](const int (&v)[G], int slot, int first) {
#pragma unroll
    for (int t = 0; t < G; ++t)
      if (first + t < ntl) dma_tile(v[t] & 0x3fffff, slot, t);
  };
  sload_group(0, eg);
  sload_group(1, en);
  wait_group(eg);
  wait_group(en);
  if (nit > 0) dma_group(eg, 0, 0);

  // Per wave, the work is a sequence of CHAINS: chain (W tile, my frame tile f) = 3 KS MFMAs into a main and a cross
  // accumulator.  The online log-sum-exp of a chain's result is issued INSIDE the next chain's MFMA stream.  Two
  // accumulator pairs alternate: with two frame tiles chain f writes pair f; with one, the pairs take turns.
  const bool epi_on = !(a.dbg & 2);
  float m_run[NX], s_run[NX];
#pragma unroll
  for (int f = 0; f < NX; ++f) { m_run[f] = K1_MFLOOR; s_run[f] = 0.0f; }
  k1b_f32x16 accm[2], accc[2];
  struct Pend { int live, last, jrow, ef; };   // the chain whose epilogue is still owed (wave-uniform); ef: its pdf's first needed 16-frame tile
  Pend pend{0, 0, 0, 0};

  // online log-sum-exp update of frame tile F from accumulator pair R (pure VALU, no memory: it is meant to be interleaved)
  auto lse_update = [&](auto r_c, auto f_c) {
    constexpr int R = decltype(r_c)::value, F = decltype(f_c)::value;
    k1b_f32x16 c;
#pragma unroll
    for (int i = 0; i < 16; ++i) c[i] = __builtin_fmaf(accc[R][i], 1.0f / 2048.0f, accm[R][i]);
    float m = k1_max3v(k1_max3v(c[0], c[1], c[2]), k1_max3v(c[3], c[4], c[5]), k1_max3v(c[6], c[7], c[8]));
    const float m2 = k1_max3v(k1_max3v(c[9], c[10], c[11]), k1_max3v(c[12], c[13], c[14]), c[15]);
    m = k1b_pair_max(k1_max3v(m, m2, K1_MFLOOR));
    const float mnew = __builtin_fmaxf(m_run[F], m);
    const float nm = -mnew * L2E;
    float ss0 = 0.0f, ss1 = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; i += 2) {
      ss0 += k1_exp2_le1(__builtin_fmaf(c[i], L2E, nm));
      ss1 += k1_exp2_le1(__builtin_fmaf(c[i + 1], L2E, nm));
    }
    const float sc = __builtin_amdgcn_exp2f((m_run[F] - mnew) * L2E);
    s_run[F] = __builtin_fmaf(s_run[F], sc, ss0 + ss1);
    m_run[F] = mnew;
  };
  // the pdf's last W tile went through lse_update: LL = max + log(sum), 32 consecutive floats per tile
  // (the 16 frames of a tile in front of the pdf's first needed 16-frame tile are not written: nobody reads them)
  auto finish = [&](auto f_c, int jrow, int ef) {
    constexpr int F = decltype(f_c)::value;
    const float st = k1b_pair_sum(s_run[F]);
    const float v = m_run[F] + __builtin_amdgcn_logf(st) * LN2;
    const int t = 32 * (ck.tile0 + wk.tile[F]) + col;
    if (kb == 0 && (t >> 4) >= ef) llu[(int64_t)jrow * tpad + t] = v;
    if (kb == 0 && t < T && !(fabsf(v) <= 3.0e38f) && epi_on) atomicOr(a.err_flag, 1);
    m_run[F] = K1_MFLOOR;
    s_run[F] = 0.0f;
  };
  constexpr bool UPFRONT = KS <= 5;               // KS = 10: fragments are read at their MFMA
  struct Frags { k1h_f16x8 A[2][KS]; const char* wt; };
  auto load_gconst = [&](const char* wt, k1b_f32x16& c) {
    const float* gc = reinterpret_cast<const float*>(wt + 2 * KS * 1024);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const f32x4 g = *reinterpret_cast<const f32x4*>(gc + 8 * i + 4 * kb);
      c[4 * i] = g[0]; c[4 * i + 1] = g[1]; c[4 * i + 2] = g[2]; c[4 * i + 3] = g[3];
    }
  };
  auto load_piece = [&](const char* wt, int pw, k1h_f16x8 (&dst)[KS]) {
#pragma unroll
    for (int s = 0; s < KS; ++s) dst[s] = *reinterpret_cast<const k1h_f16x8*>(wt + ((pw * KS + s) * 64 + lane) * 16);
  };
  // chain into pair W for frame tile FW, with the epilogue of pair 1 - W (frame tile FR) inside it
  auto chain = [&](const Frags& fr, auto w_c, auto fw_c, auto fr_c, bool with_epi) {
    constexpr int W = decltype(w_c)::value, FW = decltype(fw_c)::value;
    auto afrag = [&](int pw, int s) -> k1h_f16x8 {
      if constexpr (UPFRONT) return fr.A[pw][s];
      else return *reinterpret_cast<const k1h_f16x8*>(fr.wt + ((pw * KS + s) * 64 + lane) * 16);
    };
    // C input of the main accumulator = gconst[row], rows 8 i + 4 kb + j
    k1b_f32x16 cm, cc;
    load_gconst(fr.wt, cm);
#pragma unroll
    for (int i = 0; i < 16; ++i) cc[i] = 0.0f;
    auto mfmas = [&] {
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        cc = __builtin_amdgcn_mfma_f32_32x32x16_f16(afrag(0, s), xb[FW][1][s], cc, 0, 0, 0);
        cm = __builtin_amdgcn_mfma_f32_32x32x16_f16(afrag(0, s), xb[FW][0][s], cm, 0, 0, 0);
        cc = __builtin_amdgcn_mfma_f32_32x32x16_f16(afrag(1, s), xb[FW][0][s], cc, 0, 0, 0);
      }
    };
    if (with_epi) {
      lse_update(std::integral_constant<int, 1 - W>(), fr_c);
      mfmas();
      __builtin_amdgcn_sched_group_barrier(0x002, K1H_VHEAD, 0);
#pragma unroll
      for (int i = 0; i < 3 * KS; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, VPER, 0);
      }
    } else {
      mfmas();
    }
    accm[W] = cm;
    accc[W] = cc;
  };
  auto first_live = [&](int e) {               // tiles of mine the pdf does not need yet (first needed 32-frame tile = ef >> 1)
    const int need = ((e >> 22) & 0x7f) >> 1;
    int fs = 0;
#pragma unroll
    for (int f = 0; f < NT; ++f) fs += (ck.tile0 + wk.tile[f]) < need ? 1 : 0;
    return fs;
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;

  int par = 1;                                 // NT == 1: pair holding the owed result (the first chain writes pair 0)
  auto compute = [&](const Frags& fr, int e, int jrow, int fs, bool last_on) {
    const int last = e < 0 ? 1 : 0, ef = (e >> 22) & 0x7f;
    if constexpr (NT == 2) {
      const bool l0 = fs == 0, l1 = fs <= 1 && last_on;
      if (l0 && l1) {
        chain(fr, I0(), I0(), I1(), pend.live && epi_on);
        if (pend.live && pend.last) finish(I1(), pend.jrow, pend.ef);
        chain(fr, I1(), I1(), I0(), epi_on);
        if (last) finish(I0(), jrow, ef);
        pend = Pend{1, last, jrow, ef};
      } else if (l1) {
        if (pend.live) { if (epi_on) lse_update(I1(), I1()); if (pend.last) finish(I1(), pend.jrow, pend.ef); }
        chain(fr, I1(), I1(), I0(), false);
        pend = Pend{1, last, jrow, ef};
      } else if (l0) {
        chain(fr, I0(), I0(), I1(), pend.live && epi_on);
        if (pend.live && pend.last) finish(I1(), pend.jrow, pend.ef);
        if (epi_on) lse_update(I0(), I0());
        if (last) finish(I0(), jrow, ef);
        pend = Pend{0, 0, 0, 0};
      }
    } else if constexpr (NT == 1) {
      if (fs == 0 && last_on) {
        if (par) { chain(fr, I0(), I0(), I0(), pend.live && epi_on); }
        else { chain(fr, I1(), I0(), I0(), pend.live && epi_on); }
        par ^= 1;
        if (pend.live && pend.last) finish(I0(), pend.jrow, pend.ef);
        pend = Pend{1, last, jrow, ef};
      }
    }
  };

  int j = 0;                                   // local pdf index of the walk entry being consumed
#ifdef K1H_TIMING
  uint64_t tm_bar = 0, tm_lds = 0, tm_cmp = 0, tm_idle = 0, tm_n = 0, t_d = __builtin_readcyclecounter();
  const uint64_t t_0 = t_d;
#endif
  for (int it = 0; it < nit; ++it) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (it + 1 < nit) dma_group(en, (it + 1) & 1, G * (it + 1));
    int ec[G];
#pragma unroll
    for (int t = 0; t < G; ++t) { ec[t] = eg[t]; eg[t] = en[t]; }
    sload_group(it + 2, en);
#ifdef K1H_TIMING
    const uint64_t t_a = __builtin_readcyclecounter();
    tm_bar += t_a - t_d;
    uint64_t t_c = t_a;
#endif
    const char* slot_base = lds + (it & 1) * SLOTB;
    // (Requesting the first-piece fragments of tile t + 1 before the chains of tile t -- 20 more registers -- and pinning the
    // order of the LDS reads were both measured: no gain, see DESIGN.md K1 f16x2 "what was tried".)
#pragma unroll
    for (int t = 0; t < G; ++t) {
      if (G * it + t < ntl) {
        const int e = ec[t];
        if constexpr (NT > 0) {
          const int fs = first_live(e);
          const bool last_on = wk.pmode == 0 || (j & 1) == wk.pmode - 1;
          if (fs < NT - 1 || (fs == NT - 1 && last_on)) {
            Frags fr;
            fr.wt = slot_base + t * TILEB;
            if constexpr (UPFRONT) { load_piece(fr.wt, 0, fr.A[0]); load_piece(fr.wt, 1, fr.A[1]); }
#ifdef K1H_TIMING
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            const uint64_t t_b = __builtin_readcyclecounter();
            tm_lds += t_b - t_c;
#endif
            compute(fr, e, j, fs, last_on);
#ifdef K1H_TIMING
            t_c = __builtin_readcyclecounter();
            tm_cmp += t_c - t_b;
            tm_n += 1;
#endif
          }
        }
        j += e < 0 ? 1 : 0;
      }
    }
#ifdef K1H_TIMING
    t_d = __builtin_readcyclecounter();
    tm_idle += t_d - t_c;
#endif
    wait_group(en);
  }
  if constexpr (NT == 2) {
    if (pend.live) { if (epi_on) lse_update(I1(), I1()); if (pend.last) finish(I1(), pend.jrow, pend.ef); }
  } else if constexpr (NT == 1) {
    if (pend.live) {
      if (epi_on) { if (par) lse_update(I1(), I0()); else lse_update(I0(), I0()); }
      if (pend.last) finish(I0(), pend.jrow, pend.ef);
    }
  }
#ifdef K1H_TIMING
  // cycle stamps (s_memtime) of this wave: [barrier wait, fragment wait, chains, tail of the interval, tiles, total, NT]
  if (a.tbuf && lane == 0) {
    uint64_t* o = a.tbuf + ((size_t)blockIdx.x * 8 + wave) * 8;
    o[0] = tm_bar; o[1] = tm_lds; o[2] = tm_cmp; o[3] = tm_idle; o[4] = tm_n; o[5] = __builtin_readcyclecounter() - t_0; o[6] = NT; o[7] = nit;
  }
#endif
}

template <int KS, int NTMAX>
__global__ __launch_bounds__(512, 2) void k1h_loglikes(K1hArgs a) {
  extern __shared__ __attribute__((aligned(1024))) char k1h_lds[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const K1bChunk ck = a.chunks[blockIdx.x];
  if (ck.ntiles <= 0) return;
  // the dealing of k1b_loglikes: n = 4 q + r tiles, round k of SIMD s is tile 4 k + s, rounds alternate between the
  // SIMD's two waves, the r remainder tiles are shared by pdf parity
  const int n = ck.ntiles, q = n >> 2, r = n & 3, sd = wave & 3, hf = wave >> 2;
  const bool share = !(a.dbg & 8);
  auto deal = [&](int h, K1bWork& w) {          // what wave (sd, h) gets -> number of tiles
    int c = 0;
#pragma unroll
    for (int jj = 0; jj < NTMAX; ++jj) {
      const int k = 2 * jj + h;
      if (!share) { if (4 * k + sd < n) w.tile[c++] = 4 * k + sd; continue; }
      if (k < q) w.tile[c++] = 4 * k + sd;
      else if (k == q && r != 0) {
        if (r == 1) { if (sd < 2) { w.tile[c++] = 4 * q; w.pmode = 1 + sd; } }
        else if (r == 2) { w.tile[c++] = 4 * q + (sd >> 1); w.pmode = 1 + (sd & 1); }
        else if (sd < 2) w.tile[c++] = 4 * q + sd;
        else { w.tile[c++] = 4 * q + 2; w.pmode = 1 + (sd - 2); }
      }
    }
    return c;
  };
  K1bWork wk{{0, 0}, 0}, ws{{0, 0}, 0};
  int nt = deal(hf, wk);
  const int nts = deal(1 - hf, ws);
  // A SIMD whose second wave got nothing (utterances of < 8 tiles) would run one instruction stream with nobody to fill its
  // latencies: the two waves then BOTH hold the lone tile and split the pdfs of the walk by parity.
  if (share && !(a.dbg & 16)) {
    if (nt == 0 && nts == 1 && ws.pmode == 0) { wk = ws; wk.pmode = 1 + hf; nt = 1; }
    else if (nt == 1 && nts == 0 && wk.pmode == 0) wk.pmode = 1 + hf;
  }
  // (Telling the compiler that wk / nt are wave-uniform -- readfirstlane, scalar branches instead of exec-mask ones in the
  // walk -- measured 2-7 % SLOWER, tools/k1b_probe.py at T = 512 / 300 / 160: 13.5 / 15.7 / 17.9 ms against 13.3 / 15.2 / 16.7.)
  if (nt == 0) k1h_wave<KS, 0>(a, ck, k1h_lds, wave, wk);
  else if (nt == 1) k1h_wave<KS, 1>(a, ck, k1h_lds, wave, wk);
  else if constexpr (NTMAX >= 2) k1h_wave<KS, 2>(a, ck, k1h_lds, wave, wk);
}
