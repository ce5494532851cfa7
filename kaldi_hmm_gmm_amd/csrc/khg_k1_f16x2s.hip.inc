// K1 on the fp16 matrix cores, "f16x2s" (round 3; the default K1): the arithmetic of khg_k1_f16x2.hip.inc with ONE accumulator
// per chain, in a TRANSPOSED decomposition -- the utterance's feature tiles sit in LDS, every wave owns whole pdfs.
//
// Reference: decodable-am-diag-gmm.cc:55-61, diag-gmm.cc:167-189, eigen.cc:14-18 (as in the other K1 forms).
//
// Arithmetic.  C[g][t] = gconst[g] + sum_k W[g][k] X[k][t],  W = [M | -0.5 V],  X = [x | fl(x^2)],  K = 2 D.  Per k the operands
// are scaled by exact powers of two, x' = x 2^ex_k and w' = w 2^(S - ex_k), so that every feature column peaks in [2^14, 2^15)
// (ex_k: a property of the utterance set alone -- the planes are packed ONCE and never re-packed) and the largest weight column
// peaks in [2^14, 2^15) (S: one number per (model, set)).  Each scaled operand is split into two fp16 pieces WITHOUT rescaling
// the residual,
//     v' = v1 + v2,    v1 = fp16(v'),   v2 = fp16(v' - v1),
// so all three partial products  w1 x1 + w1 x2 + w2 x1  carry the same scale 2^S and go into ONE fp32 accumulator (whose C input
// is gconst 2^S) on v_mfma_f32_32x32x16_f16: 15 MFMAs per (32 Gaussians x 32 frames) at D <= 40 and no combine instructions; the
// log-sum-exp folds 2^-S into its constants.  Representation error per operand: max(2^-23 |v'|, 2^-25) -- 11 + 11 significant
// bits (fp16's significand is 11 bits: |v' - v1| <= 2^-11 |v'|; the residual has <= 13 significant bits on v's grid and loses
// at most the last one when it is a normal fp16 number, <= 2^-23 |v'|; below |v'| = 2^-2 the residual falls on fp16's subnormal
// grid 2^-24, absolute error <= 2^-25).  The dropped product w2 x2 is <= 2^-22 |w x|.  Worst case per term
//     |error| <= 2^-21 |w x| + 2^-25 (|w'| + |x'|) 2^-S,
// the second part being a FLOOR in absolute units that matters only for an operand more than 16 binades under its column's
// peak; its sum over k at the column maxima, 2^-25 sum_k (max|w'_k| + max|x'_k|) 2^-S (~1e-8 for ordinary models), is computed
// by the host, which runs this form only while it is <= 2e-6 (and the split forms' common domain holds, see
// khg_k1_f16x2.hip.inc), else the two-accumulator f16x2 form, else an fp32-MFMA form.  fp16 subnormal operands are not
// flushed by the MFMA (tools/probe_f16x2.hip).  tools/k1lab.hip measures max |error| / B = 2.1e-7 against fp64 for this form.
//
// Shape.  A workgroup (8 waves, two per SIMD) owns <= NMAX 32-frame tiles of one utterance (15 at D <= 40, 7 at D <= 80): their
// B fragments ([piece 2][step KS][lane 64] x 16 B = 2 KS KiB per tile) are copied into LDS once by LDS-DMA.  After that one
// barrier the waves never meet again: each takes pdfs of the utterance's list from an LDS counter (the last two pdfs are cut into
// four frame ranges each, so the waves finish together).  For a pdf it loads the
// A fragments + gconst of TPS = 2 (D <= 40; 1 at D <= 80) W tiles from the cache-resident image STRAIGHT INTO REGISTERS and
// runs over the frame tiles f the pdf needs: per f one chain of 3 KS MFMAs per W tile; the B fragments of tile f + 1 are read
// from LDS into the registers the last chain of f has finished with.  The online log-sum-exp of a chain is issued inside the
// NEXT chain, instruction by instruction behind its MFMAs (a fixed list of ~63 VALU instructions, hand-placed with
// sched_barrier: the compiler's own interleave front-loads them and leaves half the chain's MFMA gaps empty); the value of
// (pdf, f) is complete and stored inside chain (f + 1, 0).  No data-dependent branch, no workgroup barrier, no dealing of frame
// tiles to waves in the loop: an utterance of any number of tiles loads the four SIMDs alike (pdfs / 4 each).
// Pdfs of more than TPS tiles run as several PASSES over the frame tiles, a later pass combining its log-sum-exp with the
// value the earlier pass stored (same wave, same lanes).  Models whose pdfs all have <= 8 / <= 16 Gaussians run the PACKED kernel at
// the end of this file (4 / 2 pdfs per MFMA tile).
// Measured (tools/k1lab.hip, MI355X, 75-96 pdfs x 64 Gaussians): 26.4 / 27.4 / 27.8 / 30.7 ns per MFMA and SIMD at 14 / 10 / 8 / 5
// frame tiles, against 27.0 for the tile-major structure of khg_k1_f16x2.hip.inc at its best case (16 tiles, all slots
// full, hand-placed log-sum-exp) and ~37 for that kernel on the bench's ragged lengths; the bare dependent MFMA loop holds
// 20 ns (the chip clocks down to ~1.5-1.6 GHz under it: K1 is bound by power, so what counts is energy per chain).

typedef float k1s_f32x4 __attribute__((ext_vector_type(4)));
#ifndef K1S_NSPLIT
#define K1S_NSPLIT 2      // pdfs at the end of an utterance's list that are cut into ...
#define K1S_NPART 4       // ... this many frame ranges (work items)
#endif
#ifndef K1S_GAP0
#define K1S_GAP0 1        // first MFMA gap of a chain that carries owed log-sum-exp instructions
#endif
#ifndef K1S_KO
#define K1S_KO 0          // MEASUREMENT builds only (tools/ab_k1.sh; results are WRONG): knock-outs that price one part of the loop each --
#endif                    // 1 no score stores, 2 no band fills, 4 B fragments stay in registers (no LDS re-reads), 8 W tiles loaded once, 16 no log-sum-exp,
                          // 32 no chunk fill (the LDS-DMA copy of the chunk's frame tiles and its wait are skipped: the chains read whatever LDS holds;
                          //    timed as 33 against 1 -- without the score stores, so that nothing downstream reads those values)
#ifndef K1S_PRIO
#define K1S_PRIO 0        // 1: s_setprio 1 for the second-dispatched half of the workgroup (waves 4-7)
#endif

__host__ __device__ constexpr int k1s_tile_bytes(int KS) { return 2 * KS * 1024 + 128; }    // A fragments + gconst[32]
__host__ __device__ constexpr int k1s_xtile_bytes(int KS) { return 2 * KS * 1024; }
#ifndef K1S_NMAX5
#define K1S_NMAX5 15
#endif
__host__ __device__ constexpr int k1s_nmax(int KS) { return KS == 5 ? K1S_NMAX5 : 7; }       // frame tiles per workgroup (LDS)
__host__ __device__ constexpr int k1s_tps(int KS) { return KS == 5 ? 2 : 1; }                 // W tiles per pass (registers)

struct K1sChunk { int32_t utt, tile0, ntiles, pad; };
// one per (utterance, pdf of its list): first W tile; number of W tiles (bits 0-10) | SHIFT s of the band's tiles in frames (bits
// 11-15; 0 = tiles aligned on 32 frames) | first needed 32-frame tile, clamped to 255 (bits 16-23) | last needed 32-frame tile, 255 =
// no limit (bits 24-31: the BAND form, see K1sArgs::ubound)
struct K1sUnit { int32_t tile0; uint32_t info; };
#define K1S_NT_MASK 0x7ffu

struct K1sArgs {
  const k1b_u32x4* xs;            // per 32-frame tile: [piece 2][step KS][lane 64] 16-byte B fragments
  const int64_t* utt_xtile_off;   // [U+1]
  const int64_t* frame_off;       // [U+1]
  const K1sChunk* chunks;
  const char* wimg;               // k1s_tile_bytes(KS) per 32-Gaussian tile
  const int64_t* pdf_off;         // [U+1] offsets into units (= the utterances' pdf lists)
  const K1sUnit* units;
  float* ll;
  const int64_t* ll_off;
  float* dump;                    // >= 64 floats nobody reads
  int32_t* err_flag;
  float c1;                       // log2(e) 2^-S
  float inv_scale;                // 2^-S
  float mfloor;                   // floor of the running maximum, in accumulator units: -3e38 / max(1, c1), so that mfloor c1 stays finite
  // BAND form (khg_loglikes_band): a (pdf, 32-frame tile) behind the pdf's last needed tile -- every arc carrying the pdf leads to a
  // state from which no final state can be reached in the frames that remain -- is not computed; its 32 cells are FILLED with
  // ubound[first W tile of the pdf], an upper bound of the pdf's log-likelihood over all x (k0_model_stats, khg_ctx_model.hip).  A token that
  // reads such a cell can never reach a final state, so the best path is untouched; its DP cost only gets LOWER, which keeps
  // K2's beam certificate (exact frame minimum + beam) sound.  nullptr: every tile from the first needed one is computed.
  // SHIFTED TILES (round 4): a band [first, last] in frames whose end lies EARLIER inside its tile than its start (last % 32 <
  // first % 32: every second band) is covered by one 32-frame tile FEWER if its tiles start at frame `first` itself instead of on
  // the 32-frame grid.  The B fragment of a tile that starts s frames late is columns s..31 of tile f followed by columns 0..s-1
  // of tile f + 1 -- the same 16-byte LDS reads with a per-lane address (column (col + s) % 32, the next tile's block for
  // col + s >= 32), folded into the lane's base address once per pdf; nothing else changes in the chain.
  const float* ubound;
  // repair launch (khg_align, BAND form): only utterances whose status carries `repair_bit` (the beam certificate failed: the
  // order-faithful decoder is about to read EVERY cell a token can reach) are recomputed, without the band's upper limit
  const int32_t* repair_status;
  int32_t repair_bit;
  // KHG_OPT_K1_PROF: per chunk 8 words -- clock64() at entry | after the barrier | when the FIRST wave found the work-item counter
  // exhausted | when the LAST one did | (XCC << 16) | HW_ID bits 8-15 (shader engine, array, CU) | frame tiles; nullptr: no stamps
  long long* stamps;
};

// LDS behind the NMAX frame-tile slots: 16 control words (one-chunk launch: [0] the work-item counter; persistent launch: two
// banks of 8, see k1s_persistent), then two banks of stamp words {first, last, waves done} of 32 bytes (KHG_OPT_K1_PROF)
#define K1S_CTL_BYTES 128
struct K1sProf { unsigned long long first, last; int done, pad[3]; };

// (ubound[first tile of pdf p] = log sum_g exp(gconst_g + 0.5 sum_d mi_gd^2 / iv_gd) + margin -- every component at its own mean: an
//  upper bound of DiagGmm::LogLikelihood(x) for every x -- is computed by k0_model_stats, khg_ctx_model.hip, in fp64, once per
//  parameter version)

__device__ __forceinline__ void k1s_split(float v, _Float16& a, _Float16& b) {
  a = (_Float16)v;
  b = (_Float16)(v - (float)a);      // exact difference (<= 13 significant bits), rounded to fp16
}

// model -> f16x2s W image, one workgroup per 32-Gaussian tile; ew[k]: w' = w 2^ew[k]; gscale = 2^S
template <int KS>
__global__ __launch_bounds__(256) void k0s_pack_tiles(const float* __restrict__ gconsts, const float* __restrict__ miv,
                                                       const float* __restrict__ iv, const int32_t* __restrict__ gauss_off,
                                                       const int32_t* __restrict__ pdf_tile_off, const int32_t* __restrict__ tile_pdf,
                                                       int D, const int32_t* __restrict__ ew, float gscale, char* __restrict__ wimg) {
  constexpr int TILEB = k1s_tile_bytes(KS);
  const int t = blockIdx.x, p = tile_pdf[t];
  const int g_first = gauss_off[p] + 32 * (t - pdf_tile_off[p]);
  const int nrow = min(32, gauss_off[p + 1] - g_first);
  char* img = wimg + (size_t)t * TILEB;
  for (int f = threadIdx.x; f < KS * 64; f += 256) {
    const int s = f >> 6, lane = f & 63, g = lane & 31, kb = lane >> 5;
    k1h_f16x8 p0, p1;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int k = 16 * s + 8 * kb + e, d = k >> 1;
      float v = 0.0f;
      if (g < nrow && d < D) { const size_t src = (size_t)(g_first + g) * D + d; v = ldexpf((k & 1) ? -0.5f * iv[src] : miv[src], ew[k]); }
      _Float16 a, b;
      k1s_split(v, a, b);
      p0[e] = a; p1[e] = b;
    }
    *reinterpret_cast<k1h_f16x8*>(img + ((0 * KS + s) * 64 + lane) * 16) = p0;
    *reinterpret_cast<k1h_f16x8*>(img + ((1 * KS + s) * 64 + lane) * 16) = p1;
  }
  float* gc = reinterpret_cast<float*>(img + 2 * KS * 1024);
  if (threadIdx.x < 32) gc[threadIdx.x] = (int)threadIdx.x < nrow ? gconsts[g_first + threadIdx.x] * gscale : -INFINITY;
}

// features -> f16x2s B fragments, one thread per (32-frame tile, step, lane); x' = x 2^ex
template <int KS>
__global__ void k1s_pack_x(const float* __restrict__ feats, const int64_t* __restrict__ frame_off,
                           const int64_t* __restrict__ utt_xtile_off, const int32_t* __restrict__ xtile_utt,
                           int64_t n_xtiles, int D, const int32_t* __restrict__ ex, k1b_u32x4* __restrict__ xs) {
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
      k1s_split(ldexpf(x, ex[k]), a, b);      p0[e] = a; p1[e] = b;
      k1s_split(ldexpf(xx, ex[k + 1]), a, b); p0[e + 1] = a; p1[e + 1] = b;
    }
    k1b_u32x4* dst = xs + xt * (2 * KS * 64);
    dst[(0 * KS + s) * 64 + lane] = __builtin_bit_cast(k1b_u32x4, p0);
    dst[(1 * KS + s) * 64 + lane] = __builtin_bit_cast(k1b_u32x4, p1);
  }
}

// keeps a VALU result where it was written: without it the sums of the log-sum-exp are sunk to the end of the chain and
// re-associated into dependent v_pk_add_f32 chains
#define K1S_PIN(x) asm volatile("" : "+v"(x))

// frame tiles [f0, f1) of chunk `ck` -> base + f * XTB by LDS-DMA (1 KiB per wave-instruction), dealt to `nw` issuing waves of
// which this one is number `w`; the caller waits (vmcnt) and meets the barrier
template <int KS>
__device__ __forceinline__ void k1s_fill(const K1sArgs& a, const K1sChunk& ck, char* base, int f0, int f1, int w, int nw) {
  constexpr int XTB = k1s_xtile_bytes(KS);
  const int lane = threadIdx.x & 63;
  const char* src = reinterpret_cast<const char*>(a.xs) + (a.utt_xtile_off[ck.utt] + ck.tile0) * (int64_t)XTB;
  for (int i = f0 * 2 * KS + w; i < f1 * 2 * KS; i += nw)
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + (int64_t)i * 1024 + lane * 16),
                                     (__attribute__((address_space(3))) void*)(base + i * 1024), 16, 0, 0);
}

// KHG_OPT_K1_PROF: which CU this workgroup runs on -- (XCC_ID << 16) | HW_ID bits 8-15
__device__ __forceinline__ long long k1s_cu_id() {
  const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4), xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20);
  return (long long)(((xcc & 15u) << 16) | (hw & 0xff00u));
}
// ... a wave that found the work-item counter exhausted; the last of the 8 writes the chunk's record out
__device__ __forceinline__ void k1s_stamp_done(long long* rec, K1sProf* pf) {
  if ((threadIdx.x & 63) == 0) {
    const unsigned long long t = (unsigned long long)clock64();
    atomicMin(&pf->first, t);
    atomicMax(&pf->last, t);
    __threadfence_block();
    if (atomicAdd(&pf->done, 1) == 7) { rec[2] = (long long)atomicMin(&pf->first, ~0ull); rec[3] = (long long)atomicMax(&pf->last, 0ull); }
  }
}

// one chunk (<= NMAX frame tiles of one utterance) whose B fragments stand in LDS at `lds` (tile f at lds + f XTB), by one
// workgroup past its barrier; `ctr`: the chunk's work-item counter in LDS, zero
template <int KS>
__device__ __forceinline__ void k1s_body(const K1sArgs& a, const K1sChunk& ck, char* lds, int* ctr) {
  constexpr int XTB = k1s_xtile_bytes(KS), TILEB = k1s_tile_bytes(KS), TPS = k1s_tps(KS), NMF = 3 * KS;
  constexpr float LN2 = 0.69314718055994530942f;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63, col = lane & 31, kb = lane >> 5;
  const int n = ck.ntiles, u = ck.utt;
  const bool band = a.ubound != nullptr && a.repair_status == nullptr;
  const float c1 = a.c1, inv_scale = a.inv_scale, MFLOOR = a.mfloor;
  (void)wave;
  const int64_t T = a.frame_off[u + 1] - a.frame_off[u];
  const int tpad = (int)((T + 31) & ~(int64_t)31);
  float* llu = a.ll + a.ll_off[u] + 32 * ck.tile0;
  const int64_t p0 = a.pdf_off[u];
  const int npdf = (int)(a.pdf_off[u + 1] - p0);
  const K1sUnit* units = a.units + p0;

  // ---- state ----
  // The pipeline starts with an owed update on an accumulator of -inf against the state (0, 1): a no-op whose value, log 2,
  // goes to the dump line.
  float m_run = 0.0f, s_run = 1.0f;
  k1b_f32x16 acc0, acc1;
#pragma unroll
  for (int i = 0; i < 16; ++i) { acc0[i] = -INFINITY; acc1[i] = -INFINITY; }
  float* pend = a.dump;          // where the value whose log-sum-exp is still owed goes (lane 0's address)
  int pend_comb = 0;             // ... and whether it combines with an earlier pass's value stored there
  unsigned bad = 0;
  k1h_f16x8 B[2][KS];
  int btile = -1;                // the frame tile B holds (2 f + shift)
  int sh = 0;                    // this pdf's tiles start sh frames late (see K1sArgs::ubound)
  int lofs = lane * 16;          // the lane's byte offset inside a 1 KiB fragment block: its (shifted) column's
  auto load_b = [&](int f) {
    const char* src = lds + f * XTB + lofs;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int s = 0; s < KS; ++s) B[p][s] = *reinterpret_cast<const k1h_f16x8*>(src + (p * KS + s) * 1024);
    btile = 32 * f + sh;
  };

  struct Q { float t[5], u0, u1, m, mnew, nm, sc, a[16], e[16], ss0, ss1, st, v; };
  // The work owed for a finished chain, as an indexed list of single instructions:
  //   NEXT  (63): online log-sum-exp update of (m_run, s_run) with the accumulator c
  //   FIRST (59): the same on a fresh state (no rescale of the running sum)
  //   FIN    (7): the pdf's value for the pending (row, tile): max + log(sum) -> [combine] -> store; reset the state
  auto lse_core = [&](auto k_c, const k1b_f32x16& c, Q& q) {     // the 48 instructions of the exponentials: fma / exp / add, software-pipelined
    constexpr int K0 = decltype(k_c)::value;
    constexpr auto pick = [] {
      int nn = 0;
      for (int j = 0; j < 18; ++j)
        for (int sl = 0; sl < 3; ++sl) {
          const int idx = j - sl;
          if (idx < 0 || idx > 15) continue;
          if (nn == K0) return sl * 16 + idx;
          ++nn;
        }
      return -1;
    }();
    constexpr int SL = pick / 16, IDX = pick % 16;
    if constexpr (SL == 0) q.a[IDX] = __builtin_fmaf(c[IDX], c1, q.nm);
    else if constexpr (SL == 1) q.e[IDX] = k1_exp2_le1(q.a[IDX]);
    else if constexpr (IDX < 2) { if constexpr (IDX & 1) q.ss1 = q.e[IDX]; else q.ss0 = q.e[IDX]; }
    else { if constexpr (IDX & 1) { q.ss1 += q.e[IDX]; K1S_PIN(q.ss1); } else { q.ss0 += q.e[IDX]; K1S_PIN(q.ss0); } }
  };
  auto fin_op = [&](auto i_c, Q& q) {
    constexpr int I = decltype(i_c)::value;
    if constexpr (I == 0) q.st = k1b_pair_sum(s_run);
    else if constexpr (I == 1) q.st = __builtin_amdgcn_logf(q.st);
    else if constexpr (I == 2) q.v = q.st * LN2;
    else if constexpr (I == 3) q.v = __builtin_fmaf(m_run, inv_scale, q.v);
    else if constexpr (I == 4) {
      if (pend_comb) {            // a later pass of a pdf with more than TPS tiles: log(exp(old) + exp(v))
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const float old = pend[col];
        const float mx = fmaxf(old, q.v), mn = fminf(old, q.v);
        q.v = mx + __builtin_amdgcn_logf(1.0f + __builtin_amdgcn_exp2f((mn - mx) * 1.44269504088896340736f)) * LN2;
        if (!(mn > -INFINITY)) q.v = mx;
      }
    }
    else if constexpr (I == 5) { if (kb == 0 && !(K1S_KO & 1)) pend[col] = q.v; }
    else if constexpr (I == 6) { bad |= !(fabsf(q.v) <= 3.0e38f) ? 1u : 0u; m_run = MFLOOR; s_run = 0.0f; }
  };
  // KIND 0: NEXT + FIN (70 ops), 1: FIRST (59 ops), 2: NEXT (63 ops)
  auto op = [&](auto kind_c, auto i_c, const k1b_f32x16& c, Q& q) {
    constexpr int KIND = decltype(kind_c)::value, I = decltype(i_c)::value;
    if constexpr (I < 5) q.t[I] = k1_max3v(c[3 * I], c[3 * I + 1], c[3 * I + 2]);
    else if constexpr (I == 5) q.u0 = k1_max3v(q.t[0], q.t[1], q.t[2]);
    else if constexpr (I == 6) q.u1 = k1_max3v(q.t[3], q.t[4], c[15]);
    else if constexpr (I == 7) q.m = k1_max3v(q.u0, q.u1, MFLOOR);
    else if constexpr (I == 8) q.m = k1b_pair_max(q.m);
    else if constexpr (KIND == 1) {
      if constexpr (I == 9) { q.nm = -q.m * c1; }
      else if constexpr (I < 10 + 48) lse_core(std::integral_constant<int, I - 10>(), c, q);
      else if constexpr (I == 58) { s_run = q.ss0 + q.ss1; m_run = q.m; }
    } else {
      if constexpr (I == 9) q.mnew = __builtin_fmaxf(m_run, q.m);
      else if constexpr (I == 10) q.nm = -q.mnew * c1;
      else if constexpr (I == 11) q.sc = __builtin_fmaf(m_run, c1, q.nm);
      else if constexpr (I == 12) q.sc = __builtin_amdgcn_exp2f(q.sc);
      else if constexpr (I < 13 + 48) lse_core(std::integral_constant<int, I - 13>(), c, q);
      else if constexpr (I == 61) { q.ss0 += q.ss1; K1S_PIN(q.ss0); }
      else if constexpr (I == 62) { s_run = __builtin_fmaf(s_run, q.sc, q.ss0); m_run = q.mnew; }
      else if constexpr (KIND == 0) fin_op(std::integral_constant<int, I - 63>(), q);
    }
  };
  auto ops = [&](auto kind_c, auto lo_c, auto hi_c, const k1b_f32x16& c, Q& q) {
    constexpr int LO = decltype(lo_c)::value, HI = decltype(hi_c)::value;
    [&]<int... I>(std::integer_sequence<int, I...>) { (op(kind_c, std::integral_constant<int, LO + I>(), c, q), ...); }
    (std::make_integer_sequence<int, (HI > LO ? HI - LO : 0)>());
  };
  // One chain: acc = gconst + A . B (3 KS MFMAs), with the owed work of KIND on `prev` spread over the MFMA gaps (none behind
  // the first MFMA: the previous chain's last one is still in the pipe); ROLL: B[.][s] <- the tile at `nxt` once step s is done.
  auto chain = [&](k1b_f32x16& acc, const k1b_f32x16& gc, const k1h_f16x8 (&A)[2][KS], const k1b_f32x16& prev, auto kind_c, auto roll_c, const char* nxt) {
    constexpr int KIND = decltype(kind_c)::value;
    constexpr int NOPS = KIND == 0 ? 70 : KIND == 1 ? 59 : 63;
    constexpr bool ROLL = decltype(roll_c)::value;
    Q q;
    k1b_f32x16 cm = gc;
    [&]<int... I>(std::integer_sequence<int, I...>) {
      ([&] {
        constexpr int s = I / 3, jj = I % 3;
        cm = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[jj == 1 ? 1 : 0][s], B[jj == 0 ? 1 : 0][s], cm, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        constexpr int NG = NMF - K1S_GAP0;      // gaps that carry instructions
        constexpr int lo = I < K1S_GAP0 ? 0 : (I - K1S_GAP0) * NOPS / NG, hi = I < K1S_GAP0 ? 0 : (I - K1S_GAP0 + 1) * NOPS / NG;
        if constexpr (!(K1S_KO & 16)) ops(kind_c, std::integral_constant<int, lo>(), std::integral_constant<int, hi>(), prev, q);
        if constexpr (ROLL && jj == 2 && !(K1S_KO & 4)) {
          B[0][s] = *reinterpret_cast<const k1h_f16x8*>(nxt + lofs + (0 * KS + s) * 1024);
          B[1][s] = *reinterpret_cast<const k1h_f16x8*>(nxt + lofs + (1 * KS + s) * 1024);
        }
        __builtin_amdgcn_sched_barrier(0);
      }(), ...);
    }(std::make_integer_sequence<int, NMF>());
    acc = cm;
    if constexpr ((K1S_KO & 16) != 0) asm volatile("" ::"v"(prev));      // (keeps the previous chain's MFMAs alive without the log-sum-exp)
  };
  bool w_loaded = false;
  auto load_w = [&](int tile, k1h_f16x8 (&A)[2][KS], k1b_f32x16& gc) {
    if ((K1S_KO & 8) && w_loaded) return;
    const char* w = a.wimg + (int64_t)tile * TILEB;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int s = 0; s < KS; ++s) A[p][s] = *reinterpret_cast<const k1h_f16x8*>(w + ((p * KS + s) * 64 + lane) * 16);
    const float* g = reinterpret_cast<const float*>(w + 2 * KS * 1024);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const k1s_f32x4 x0 = *reinterpret_cast<const k1s_f32x4*>(g + 8 * i + 4 * kb);
#pragma unroll
      for (int jx = 0; jx < 4; ++jx) gc[4 * i + jx] = x0[jx];
    }
    // complete before the frame loop as far as the compiler's wait-count tracking goes: otherwise it waits vmcnt(0) at the first
    // use INSIDE the loop, i.e. in every iteration -- behind that iteration's score store
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int s = 0; s < KS; ++s) asm volatile("" ::"v"(A[p][s]));
    asm volatile("" ::"v"(gc));
  };
  using KN = std::integral_constant<int, 0>;    // NEXT + FIN
  using KF = std::integral_constant<int, 1>;    // FIRST

  k1h_f16x8 A0[2][KS], A1[TPS == 2 ? 2 : 1][TPS == 2 ? KS : 1];
  k1b_f32x16 gc0, gc1;
  auto unit_of = [&](int j) {                   // (tile0, info) of pdf j, wave-uniform
    const K1sUnit* pu = units + (j < npdf ? j : npdf - 1);
    K1sUnit r;
    r.tile0 = __builtin_amdgcn_readfirstlane(pu->tile0);
    r.info = __builtin_amdgcn_readfirstlane(pu->info);
    return r;
  };
  auto first_f = [&](const K1sUnit& un) { const int need = (int)((un.info >> 16) & 0xff) - ck.tile0; return need > 0 ? need : 0; };
  // one past the last frame tile of this chunk the pdf needs (BAND form; n otherwise)
  auto end_f = [&](const K1sUnit& un) {
    const int last = (int)(un.info >> 24);
    if (!band || last == 255) return n;
    const int e = last + 1 - ck.tile0;
    return e < 0 ? 0 : (e < n ? e : n);
  };

  // Work items, handed out by an LDS counter (a wave that gets less of its SIMD's matrix pipe simply takes fewer): item i is
  // pdf i with all its frame tiles, except that the last NSPLIT pdfs of the list are cut into NPART frame ranges each, so that
  // the waves of a workgroup finish within a fraction of a pdf of each other.
  constexpr int NSPLIT = K1S_NSPLIT, NPART = K1S_NPART;
  const int nsp = npdf < NSPLIT ? npdf : NSPLIT;
  const int nwhole = npdf - nsp, nitems = nwhole + nsp * NPART;
  auto grab = [&]() {
    int v = 0;
    if (lane == 0) v = __hip_atomic_fetch_add(ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return __builtin_amdgcn_readfirstlane(v);
  };
  auto pdf_of = [&](int i) { return i < nwhole ? i : nwhole + (i - nwhole) / NPART; };
  if constexpr (K1S_PRIO) { if (wave >= 4) __builtin_amdgcn_s_setprio(1); }
  int cur = grab();
  K1sUnit un = unit_of(pdf_of(cur));
  while (cur < nitems) {
    const int nxt_item = grab();                // one item ahead: the counter's latency and the next descriptor load are off the path
    const K1sUnit nu = unit_of(pdf_of(nxt_item));
    const int j = pdf_of(cur);
    const int ntile = (int)(un.info & K1S_NT_MASK);
    const int fb = first_f(un), fe0 = end_f(un);
    // shifted tiles: the band lies inside this chunk and the host found one tile to save
    sh = (int)((un.info >> 11) & 31u);
    if (!(band && sh && (int)(un.info >> 24) != 255 && (int)((un.info >> 16) & 0xff) >= ck.tile0 && (int)(un.info >> 24) + 1 - ck.tile0 <= n && fe0 - fb >= 2)) sh = 0;
    const int fe = fe0 - (sh ? 1 : 0);
    lofs = (((col + sh) & 31) + 32 * kb) * 16 + (col + sh >= 32 ? XTB : 0);
    int f_lo = fb, f_hi = fe;
    if (cur >= nwhole && fb < fe) {
      const int part = (cur - nwhole) % NPART, len = fe - fb;
      f_lo = fb + len * part / NPART;
      f_hi = fb + len * (part + 1) / NPART;
    }
    float* row = llu + (int64_t)j * tpad + sh;
    if (fe0 < n + (sh ? 1 : 0) && (cur < nwhole || (cur - nwhole) % NPART == NPART - 1)) {
      // BAND form: the tiles behind the pdf's last needed one get the pdf's upper bound (one 128-byte store each; a shifted band's
      // tiles end sh frames into tile fe0 - 1: the fill starts there, its last store is cut at the chunk's end)
      const float ub = a.ubound[un.tile0];
      for (int f = fe > fb ? fe : fb; f < n && !(K1S_KO & 2); ++f)
        if (kb == 0 && (f + 1 < n || col + sh < 32)) row[32 * f + col] = ub;
    }
    if (f_lo < f_hi) {
      for (int pt = 0; pt < ntile; pt += TPS) {
        const bool dual = TPS == 2 && pt + 1 < ntile;
        const int f_after = pt + TPS < ntile ? f_lo : 0;      // where B rolls to behind the last tile: this pdf's next pass, or (a guess) tile 0
        const int comb = pt > 0 ? 1 : 0;
        if (btile != 32 * f_lo + sh) load_b(f_lo);
        if constexpr (TPS == 2) {
          if (dual) {
            load_w(un.tile0 + pt, A0, gc0);
            load_w(un.tile0 + pt + 1, A1, gc1);
            if (K1S_KO & 8) w_loaded = true;
            for (int f = f_lo; f < f_hi; ++f) {
              const int fn = f + 1 < f_hi ? f + 1 : f_after;
              chain(acc0, gc0, A0, acc1, KN(), std::false_type(), nullptr);
              pend = row + 32 * f; pend_comb = comb;
              chain(acc1, gc1, A1, acc0, KF(), std::true_type(), lds + fn * XTB);
            }
            btile = 32 * f_after + sh;
            continue;
          }
        }
        // one W tile per pass: every chain closes a (pdf, tile); the two accumulators take turns, the owed one ends in acc1
        load_w(un.tile0 + pt, A0, gc0);
        int f = f_lo;
        for (; f + 1 < f_hi; f += 2) {
          chain(acc0, gc0, A0, acc1, KN(), std::true_type(), lds + (f + 1) * XTB);
          pend = row + 32 * f; pend_comb = comb;
          const int fn = f + 2 < f_hi ? f + 2 : f_after;
          chain(acc1, gc0, A0, acc0, KN(), std::true_type(), lds + fn * XTB);
          pend = row + 32 * (f + 1);
        }
        if (f < f_hi) {
          chain(acc0, gc0, A0, acc1, KN(), std::true_type(), lds + f_after * XTB);
          pend = row + 32 * f; pend_comb = comb;
          acc1 = acc0;
        }
        btile = 32 * f_after + sh;
      }
    }
    cur = nxt_item;
    un = nu;
  }
  // drain: the last chain's update and the last value
  {
    Q q;
    ops(KN(), std::integral_constant<int, 0>(), std::integral_constant<int, 70>(), acc1, q);
  }
  if (bad && !(K1S_KO & 32)) atomicOr(a.err_flag, 1);      // (no chunk fill: the values are whatever LDS held)
}

// one chunk by one workgroup, from nothing: the whole one-chunk kernel, as a function of the chunk's index
template <int KS>
__device__ __forceinline__ void k1s_chunk(const K1sArgs& a, const int chunk_index) {
  extern __shared__ __attribute__((aligned(1024))) char k1s_lds[];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const K1sChunk ck = a.chunks[chunk_index];
  const int n = ck.ntiles;
  if (n <= 0) return;
  if (a.repair_status && !(a.repair_status[ck.utt] & a.repair_bit)) return;     // repair launch: certified utterances keep their band
  int* ctr = reinterpret_cast<int*>(k1s_lds + k1s_nmax(KS) * k1s_xtile_bytes(KS));     // the work-item counter, behind the feature tiles
  K1sProf* pf = reinterpret_cast<K1sProf*>(k1s_lds + k1s_nmax(KS) * k1s_xtile_bytes(KS) + 64);
  long long* rec = a.stamps ? a.stamps + 8 * (int64_t)chunk_index : nullptr;
  if (rec && threadIdx.x == 0) { rec[0] = clock64(); rec[4] = k1s_cu_id(); rec[5] = n; pf->first = ~0ull; pf->last = 0; pf->done = 0; }
  // ---- the chunk's B fragments -> LDS, one barrier ----
  if constexpr (!(K1S_KO & 32)) k1s_fill<KS>(a, ck, k1s_lds, 0, n, wave, 8);
  if (threadIdx.x == 0) *ctr = 0;
  if constexpr (!(K1S_KO & 32)) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  if (rec && threadIdx.x == 0) rec[1] = clock64();
  k1s_body<KS>(a, ck, k1s_lds, ctr);
  if (rec) k1s_stamp_done(rec, pf);
}

template <int KS>
__global__ __launch_bounds__(512, 2) void k1s_loglikes(K1sArgs a) { k1s_chunk<KS>(a, (int)blockIdx.x); }

// The PERSISTENT launch (KHG_OPT_K1_LAUNCH): one workgroup per CU that can hold one takes chunks, in the launch order of the
// one-chunk kernel, from the global counter `next_chunk` (zero at launch), and fills the NEXT chunk's frame tiles into LDS under
// the tail of the current one.  The NMAX tile slots are used from both ends in turn: a chunk of n tiles stands at slots [0, n), the
// next one at [NMAX - n', NMAX), the one after at [0, n'') ... -- a chunk is always contiguous (tile f at base + f XTB: the chain
// code and the shifted-tile read of k1s_body are untouched) and the NMAX - n slots the current chunk leaves free all serve the
// next one.  The first wave that finds the work-item counter exhausted claims the next chunk (once per workgroup, through an LDS
// word), issues the LDS-DMA copies of those of its tiles whose slots are free, and publishes (chunk, base, the tile range [lo, hi) it
// requested); ONE barrier ends the chunk -- all waves done, all requested bytes landed.  Tiles outside [lo, hi) sit in slots the
// finished chunk was still reading: all waves copy them behind that barrier and meet a second one (no second barrier when
// everything fitted).  Control words in LDS, two banks of 8 used by alternating chunks, so that the claiming wave can reset the
// next chunk's bank while the current one is in use: [0] work-item counter, [1] claim flag, [2] the next chunk, [3] its base slot,
// [4] lo, [5] hi.  Every (pdf, tile) cell is computed by k1s_body exactly as in the one-chunk kernel: only which wave computes it
// when differs, scores are bit-identical.
template <int KS>
__global__ __launch_bounds__(512, 2) void k1s_persistent(K1sArgs a, int nchunks, int* next_chunk) {
  extern __shared__ __attribute__((aligned(1024))) char k1s_lds[];
  constexpr int XTB = k1s_xtile_bytes(KS), NMAX = k1s_nmax(KS);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  int* ctl = reinterpret_cast<int*>(k1s_lds + NMAX * XTB);
  K1sProf* prof = reinterpret_cast<K1sProf*>(k1s_lds + NMAX * XTB + 64);
  if (threadIdx.x == 0) {
    for (int i = 0; i < 16; ++i) ctl[i] = 0;
    ctl[8 + 2] = atomicAdd(next_chunk, 1);      // published as if by a chunk of bank 1: nothing resident, base 0
    for (int i = 0; i < 2; ++i) { prof[i].first = ~0ull; prof[i].last = 0; prof[i].done = 0; }
  }
  __syncthreads();
  int par = 1;
  for (;;) {
    const int c = __builtin_amdgcn_readfirstlane(ctl[8 * par + 2]);
    if (c >= nchunks) break;
    const int base = __builtin_amdgcn_readfirstlane(ctl[8 * par + 3]);
    const int have_lo = __builtin_amdgcn_readfirstlane(ctl[8 * par + 4]), have_hi = __builtin_amdgcn_readfirstlane(ctl[8 * par + 5]);
    par ^= 1;
    K1sChunk ck = a.chunks[c];
    ck.utt = __builtin_amdgcn_readfirstlane(ck.utt); ck.tile0 = __builtin_amdgcn_readfirstlane(ck.tile0);
    ck.ntiles = __builtin_amdgcn_readfirstlane(ck.ntiles);
    const int n = ck.ntiles > 0 ? ck.ntiles : 0;
    long long* rec = a.stamps ? a.stamps + 8 * (int64_t)c : nullptr;
    if (n > 0) {
      char* ldsc = k1s_lds + base * XTB;
      if (rec && threadIdx.x == 0) { rec[0] = clock64(); rec[4] = k1s_cu_id(); rec[5] = n; }
      if (have_hi - have_lo < n) {               // the tiles whose slots the previous chunk still held (all of them: the first chunk)
        k1s_fill<KS>(a, ck, ldsc, 0, have_lo, wave, 8);
        k1s_fill<KS>(a, ck, ldsc, have_hi, n, wave, 8);
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
      }
      if (rec && threadIdx.x == 0) rec[1] = clock64();
      k1s_body<KS>(a, ck, ldsc, &ctl[8 * par]);
      if (rec) k1s_stamp_done(rec, &prof[par]);
    }
    // the work-item counter is exhausted: the first wave here claims the workgroup's next chunk and requests what fits
    int first = 0;
    if (lane == 0) first = __hip_atomic_fetch_add(&ctl[8 * par + 1], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0 ? 1 : 0;
    if (__builtin_amdgcn_readfirstlane(first)) {
      int nc = 0;
      if (lane == 0) nc = atomicAdd(next_chunk, 1);
      nc = __builtin_amdgcn_readfirstlane(nc);
      K1sChunk nk = K1sChunk{0, 0, 0, 0};
      if (nc < nchunks) {
        nk = a.chunks[nc];
        nk.utt = __builtin_amdgcn_readfirstlane(nk.utt); nk.tile0 = __builtin_amdgcn_readfirstlane(nk.tile0);
        nk.ntiles = __builtin_amdgcn_readfirstlane(nk.ntiles);
      }
      const int nn = nk.ntiles > 0 ? (nk.ntiles < NMAX ? nk.ntiles : NMAX) : 0;
      int nbase, lo, hi;
      if (base == 0) { nbase = NMAX - nn; lo = n - nbase > 0 ? n - nbase : 0; hi = nn; }      // this chunk holds [0, n): the next one stands at the end
      else { nbase = 0; lo = 0; hi = nn < base ? nn : base; }                                  // this chunk holds [base, NMAX): ... at the front
      if (hi > lo) k1s_fill<KS>(a, nk, k1s_lds + nbase * XTB, lo, hi, 0, 1);
      if (lane == 0) {
        ctl[8 * par + 2] = nc; ctl[8 * par + 3] = nbase; ctl[8 * par + 4] = lo; ctl[8 * par + 5] = hi > lo ? hi : lo;
        ctl[8 * (par ^ 1) + 0] = 0; ctl[8 * (par ^ 1) + 1] = 0;
        prof[par ^ 1].first = ~0ull; prof[par ^ 1].last = 0; prof[par ^ 1].done = 0;
      }
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }
}

// The REPAIR launch of the band form (khg_align): the chunks of the few utterances whose status carries `repair_bit`, recomputed
// without the band's upper limit.  A launch of k1s_loglikes over all chunks would do it -- every other workgroup returns at once --
// but with one workgroup per CU (150 KB of LDS each) 100 000 returning workgroups still take 0.25 ms, on the path between K2 and
// K3.  Here <= 256 workgroups scan the chunk table 512 entries at a time, collect the flagged ones in LDS and run them.
template <int KS>
__global__ __launch_bounds__(512, 2) void k1s_repair(K1sArgs a, int nchunks) {
  extern __shared__ __attribute__((aligned(1024))) char k1s_lds[];
  int* list = reinterpret_cast<int*>(k1s_lds + k1s_nmax(KS) * k1s_xtile_bytes(KS) + K1S_CTL_BYTES);     // [1 + 512]: count, chunk indices
  for (int base = (int)blockIdx.x * 512; base < nchunks; base += (int)gridDim.x * 512) {
    if (threadIdx.x == 0) list[0] = 0;
    __syncthreads();
    const int c = base + (int)threadIdx.x;
    if (c < nchunks) {
      const K1sChunk ck = a.chunks[c];
      if (ck.ntiles > 0 && (a.repair_status[ck.utt] & a.repair_bit)) list[1 + atomicAdd(&list[0], 1)] = c;
    }
    __syncthreads();
    const int cnt = list[0];
    for (int i = 0; i < cnt; ++i) {
      const int cc = list[1 + i];
      __syncthreads();
      k1s_chunk<KS>(a, cc);
      __syncthreads();
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// PACKED form for models of small pdfs (every pdf <= 8 or <= 16 Gaussians, D <= 40): PACK = 4 or 2 pdfs share one 32-row MFMA
// tile instead of each filling a quarter / half of its own.  Nothing new is stored: pdf q of a group supplies rows
// q RB .. q RB + RB - 1 (RB = 32 / PACK) of the A operand from ITS OWN tile image -- the fragment loads take per-lane addresses --
// and in the accumulator layout (rows 8 i + 4 (lane >> 5) + j in registers 4 i + j) the rows of pdf q are exactly registers
// q 16 / PACK .. (q + 1) 16 / PACK - 1 of both half-waves: the log-sum-exp is SEGMENTED by register range, no lane movement
// beyond the usual half-wave exchange.  One chain gives PACK values per frame; a pdf is one tile, so there is no running state.
template <int KS, int PACK>
__global__ __launch_bounds__(512, 2) void k1s_loglikes_packed(K1sArgs a) {
  extern __shared__ __attribute__((aligned(1024))) char k1s_lds[];
  constexpr int XTB = k1s_xtile_bytes(KS), TILEB = k1s_tile_bytes(KS), NMF = 3 * KS;
  constexpr int RB = 32 / PACK, NR = 16 / PACK;          // rows / accumulator registers per pdf
  constexpr float LN2 = 0.69314718055994530942f;
  static_assert(PACK == 2 || PACK == 4, "2 or 4 pdfs per tile");
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63, col = lane & 31, kb = lane >> 5;
  const K1sChunk ck = a.chunks[blockIdx.x];
  const int n = ck.ntiles;
  if (n <= 0) return;
  const int u = ck.utt;
  const float c1 = a.c1, inv_scale = a.inv_scale, MFLOOR = a.mfloor;
  char* lds = k1s_lds;
  int* ctr = reinterpret_cast<int*>(k1s_lds + k1s_nmax(KS) * XTB);
  {
    const char* src = reinterpret_cast<const char*>(a.xs) + (a.utt_xtile_off[u] + ck.tile0) * (int64_t)XTB;
    for (int i = wave; i < n * 2 * KS; i += 8)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + (int64_t)i * 1024 + lane * 16),
                                       (__attribute__((address_space(3))) void*)(lds + i * 1024), 16, 0, 0);
    if (threadIdx.x == 0) *ctr = 0;
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }
  const int64_t T = a.frame_off[u + 1] - a.frame_off[u];
  const int tpad = (int)((T + 31) & ~(int64_t)31);
  float* llu = a.ll + a.ll_off[u] + 32 * ck.tile0;
  const int64_t p0 = a.pdf_off[u];
  const int npdf = (int)(a.pdf_off[u + 1] - p0);
  const K1sUnit* units = a.units + p0;
  (void)wave;

  k1b_f32x16 acc0, acc1;
#pragma unroll
  for (int i = 0; i < 16; ++i) { acc0[i] = 0.0f; acc1[i] = 0.0f; }     // the pipeline's first owed chain: finite values, stored to the dump line
  float* pend[PACK];
#pragma unroll
  for (int q = 0; q < PACK; ++q) pend[q] = a.dump;
  unsigned bad = 0;
  k1h_f16x8 B[2][KS];
  int btile = -1;
  auto load_b = [&](int f) {
    const char* src = lds + f * XTB;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int s = 0; s < KS; ++s) B[p][s] = *reinterpret_cast<const k1h_f16x8*>(src + ((p * KS + s) * 64 + lane) * 16);
    btile = f;
  };

  // the owed work for a finished chain: per pdf segment q the complete log-sum-exp of its NR registers and the store
  constexpr int NMAXOP = NR == 4 ? 2 : 4;                 // max tree
  constexpr int NCORE = 3 * NR - 1;                       // NR fma + NR exp + (NR - 1) adds
  constexpr int SEGOPS = NMAXOP + 2 + NCORE + 6;
  struct Q { float t[3], m, nm, a[NR], e[NR], ss0, ss1, st, v; };
  auto seg_op = [&](auto q_c, auto i_c, const k1b_f32x16& cc, Q& z) {
    constexpr int QS = decltype(q_c)::value, I = decltype(i_c)::value, R0 = QS * NR;
    if constexpr (I < NMAXOP) {
      if constexpr (NR == 4) {
        if constexpr (I == 0) z.t[0] = k1_max3v(cc[R0], cc[R0 + 1], cc[R0 + 2]);
        else z.m = k1_max3v(z.t[0], cc[R0 + 3], MFLOOR);
      } else {
        if constexpr (I == 0) z.t[0] = k1_max3v(cc[R0], cc[R0 + 1], cc[R0 + 2]);
        else if constexpr (I == 1) z.t[1] = k1_max3v(cc[R0 + 3], cc[R0 + 4], cc[R0 + 5]);
        else if constexpr (I == 2) z.t[2] = k1_max3v(cc[R0 + 6], cc[R0 + 7], MFLOOR);
        else z.m = k1_max3v(z.t[0], z.t[1], z.t[2]);
      }
    }
    else if constexpr (I == NMAXOP) z.m = k1b_pair_max(z.m);
    else if constexpr (I == NMAXOP + 1) z.nm = -z.m * c1;
    else if constexpr (I < NMAXOP + 2 + NCORE) {
      constexpr int K0 = I - (NMAXOP + 2);
      constexpr auto pick = [] {
        int nn = 0;
        for (int j = 0; j < NR + 2; ++j)
          for (int sl = 0; sl < 3; ++sl) {
            const int idx = j - sl;
            if (idx < 0 || idx > NR - 1) continue;
            if (sl == 2 && idx == 0) continue;          // the first value starts the sum: no add
            if (nn == K0) return sl * 16 + idx;
            ++nn;
          }
        return -1;
      }();
      constexpr int SL = pick / 16, IDX = pick % 16;
      if constexpr (SL == 0) z.a[IDX] = __builtin_fmaf(cc[R0 + IDX], c1, z.nm);
      else if constexpr (SL == 1) { z.e[IDX] = k1_exp2_le1(z.a[IDX]); if constexpr (IDX == 0) z.ss0 = z.e[0]; }
      else { z.ss0 += z.e[IDX]; K1S_PIN(z.ss0); }
    }
    else if constexpr (I == NMAXOP + 2 + NCORE) z.st = k1b_pair_sum(z.ss0);
    else if constexpr (I == NMAXOP + 3 + NCORE) z.st = __builtin_amdgcn_logf(z.st);
    else if constexpr (I == NMAXOP + 4 + NCORE) z.v = z.st * LN2;
    else if constexpr (I == NMAXOP + 5 + NCORE) z.v = __builtin_fmaf(z.m, inv_scale, z.v);
    else if constexpr (I == NMAXOP + 6 + NCORE) { if (kb == 0) pend[QS][col] = z.v; }
    else if constexpr (I == NMAXOP + 7 + NCORE) bad |= !(fabsf(z.v) <= 3.0e38f) ? 1u : 0u;
  };
  static_assert(SEGOPS == NMAXOP + 8 + NCORE, "op count");
  constexpr int NOPS = PACK * SEGOPS;
  auto ops = [&](auto lo_c, auto hi_c, const k1b_f32x16& cc, Q (&z)[PACK]) {
    constexpr int LO = decltype(lo_c)::value, HI = decltype(hi_c)::value;
    [&]<int... I>(std::integer_sequence<int, I...>) {
      (seg_op(std::integral_constant<int, (LO + I) / SEGOPS>(), std::integral_constant<int, (LO + I) % SEGOPS>(), cc, z[(LO + I) / SEGOPS]), ...);
    }(std::make_integer_sequence<int, (HI > LO ? HI - LO : 0)>());
  };
  auto chain = [&](k1b_f32x16& acc, const k1b_f32x16& gc, const k1h_f16x8 (&A)[2][KS], const k1b_f32x16& prev, const char* nxt) {
    Q z[PACK];
    k1b_f32x16 cm = gc;
    [&]<int... I>(std::integer_sequence<int, I...>) {
      ([&] {
        constexpr int s = I / 3, jj = I % 3;
        cm = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[jj == 1 ? 1 : 0][s], B[jj == 0 ? 1 : 0][s], cm, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        constexpr int NG = NMF - K1S_GAP0;
        constexpr int lo = I < K1S_GAP0 ? 0 : (I - K1S_GAP0) * NOPS / NG, hi = I < K1S_GAP0 ? 0 : (I - K1S_GAP0 + 1) * NOPS / NG;
        ops(std::integral_constant<int, lo>(), std::integral_constant<int, hi>(), prev, z);
        if constexpr (jj == 2) {
          B[0][s] = *reinterpret_cast<const k1h_f16x8*>(nxt + ((0 * KS + s) * 64 + lane) * 16);
          B[1][s] = *reinterpret_cast<const k1h_f16x8*>(nxt + ((1 * KS + s) * 64 + lane) * 16);
        }
        __builtin_amdgcn_sched_barrier(0);
      }(), ...);
    }(std::make_integer_sequence<int, NMF>());
    acc = cm;
  };

  const int nitems = (npdf + PACK - 1) / PACK;
  auto grab = [&]() {
    int v = 0;
    if (lane == 0) v = __hip_atomic_fetch_add(ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return __builtin_amdgcn_readfirstlane(v);
  };
  k1h_f16x8 A[2][KS];
  k1b_f32x16 gc;
  int cur = grab();
  while (cur < nitems) {
    const int nxt_item = grab();
    // the group's pdfs (the last group repeats the utterance's last pdf: the same values go to the same row twice)
    // (the group is computed from the earliest first needed tile among its pdfs; a pdf's own earlier tiles are not WRITTEN: their
    //  values go to the dump line, the cells nobody reads stay as they were, as in the one-pdf kernel)
    int tile[PACK], ndq[PACK], need = 255;
    float* row[PACK];
#pragma unroll
    for (int q = 0; q < PACK; ++q) {
      const int j = cur * PACK + q < npdf ? cur * PACK + q : npdf - 1;
      const K1sUnit* pu = units + j;
      tile[q] = __builtin_amdgcn_readfirstlane(pu->tile0);
      const int nd = (__builtin_amdgcn_readfirstlane(pu->info) >> 16) & 0xff;
      ndq[q] = nd - ck.tile0;
      need = nd < need ? nd : need;
      row[q] = llu + (int64_t)j * tpad;
    }
    const int f_lo = need - ck.tile0 > 0 ? need - ck.tile0 : 0;
    if (f_lo < n) {
      // A fragments: lane (row g, half kb) reads row g % RB of pdf g / RB's own tile; gconst likewise per register group
      {
        const int g = col, qs = g / RB;
        int tq = tile[0];
#pragma unroll
        for (int q = 1; q < PACK; ++q) tq = qs == q ? tile[q] : tq;
        const char* w = a.wimg + (int64_t)tq * TILEB + ((g % RB) + 32 * kb) * 16;
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
          for (int s = 0; s < KS; ++s) A[p][s] = *reinterpret_cast<const k1h_f16x8*>(w + (p * KS + s) * 1024);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int qi = (8 * i) / RB, r0 = (8 * i) % RB + 4 * kb;
          const float* gp = reinterpret_cast<const float*>(a.wimg + (int64_t)tile[qi] * TILEB + 2 * KS * 1024) + r0;
          const k1s_f32x4 x0 = *reinterpret_cast<const k1s_f32x4*>(gp);
#pragma unroll
          for (int jx = 0; jx < 4; ++jx) gc[4 * i + jx] = x0[jx];
        }
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
          for (int s = 0; s < KS; ++s) asm volatile("" ::"v"(A[p][s]));
        asm volatile("" ::"v"(gc));
      }
      if (btile != f_lo) load_b(f_lo);
      int f = f_lo;
      for (; f + 1 < n; f += 2) {
        chain(acc0, gc, A, acc1, lds + (f + 1) * XTB);
#pragma unroll
        for (int q = 0; q < PACK; ++q) pend[q] = f >= ndq[q] ? row[q] + 32 * f : a.dump;
        chain(acc1, gc, A, acc0, lds + (f + 2 < n ? f + 2 : 0) * XTB);
#pragma unroll
        for (int q = 0; q < PACK; ++q) pend[q] = f + 1 >= ndq[q] ? row[q] + 32 * (f + 1) : a.dump;
      }
      if (f < n) {
        chain(acc0, gc, A, acc1, lds);
#pragma unroll
        for (int q = 0; q < PACK; ++q) pend[q] = f >= ndq[q] ? row[q] + 32 * f : a.dump;
        acc1 = acc0;
      }
      btile = 0;
    }
    cur = nxt_item;
  }
  {
    Q z[PACK];
    ops(std::integral_constant<int, 0>(), std::integral_constant<int, NOPS>(), acc1, z);
  }
  if (bad) atomicOr(a.err_flag, 1);
}
