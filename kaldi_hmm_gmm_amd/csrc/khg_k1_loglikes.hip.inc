// K1: per-utterance diagonal-GMM log-likelihoods on fp32 MFMA (v_mfma_f32_16x16x4_f32).
//
// Replaces (reference, /root/reference/kaldi-hmm-gmm/csrc/):
//   decodable-am-diag-gmm.cc:55-61  loglikes = gconsts + means_invvars*x - 0.5*inv_vars*x^2 ; LogSumExp
//   diag-gmm.cc:167-176,177-189     DiagGmm::LogLikelihoods / LogLikelihoodsMatrix
//   eigen.cc:14-18                  LogSumExp
//
// Contraction: for 16 Gaussians x 16 frames,
//   C[g][t] = gconst[g] + sum_d ( M[g][d]*x[t][d] + (-0.5*V[g][d])*x[t][d]^2 )
// is a [16 x 2D]·[2D x 16] product.  MFMA step s consumes the k-quartet
//   (M[2s]·x[2s], M[2s+1]·x[2s+1], V'[2s]·x²[2s], V'[2s+1]·x²[2s+1])        V' = -0.5 V
// lane (r = lane&15, q = lane>>4) supplies A = plane_q[g = r][s] and B = xx_q[t = r][s], and the
// hardware evaluates the four products as a k-ordered fmaf chain on top of C, so the result is
// bit-for-bit   v = gconst; for s: v=fmaf(M[2s],x[2s],v); v=fmaf(M[2s+1],x[2s+1],v);
//                                  v=fmaf(V'[2s],x²[2s],v); v=fmaf(V'[2s+1],x²[2s+1],v)
// (tools/probe_mfma16.hip), which oracle/khg_oracle.c:orc_loglikes_fma_order restates.
//
// Why 16x16x4 and not 32x32x2 (same FLOP/clk): frame tiles of 16 let a ~300-frame utterance be
// dealt 5,5,5,4 over the workgroup's four waves instead of 3,3,2,2 tiles of 32 -- the 32-wide
// version measured 0.82 of the MFMA peak on perfectly divisible lengths but 0.64 at T = 300.
//
// C layout: column (lane&15) = frame, rows 4*(lane>>4)+reg = Gaussian, so the log-sum-exp over a
// pdf's Gaussians is an in-lane online reduction (8 registers per 32-Gaussian tile) and, once per
// pdf, a merge of the four lane quarters (lane^16, lane^32).
//
// Workgroup = 4 waves on one utterance chunk; wave w owns up to NF 16-frame tiles whose
// [x | x²] operands live in registers for the whole kernel; the W tiles of the utterance's pdfs
// stream through a double-buffered LDS image filled by LDS-DMA (global_load_lds_dwordx4).

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
// finite floor of the running max (all -inf tiles then need no special case: exp2(-inf) = 0)
#define K1_MFLOOR (-3.0e38f)
// v_max3_f32 without the canonicalising v_max the compiler adds around fmaxf of MFMA results
__device__ __forceinline__ float k1_max3(float a, float b, float c) {
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

struct K1Chunk {        // one workgroup
  int32_t utt;          // utterance index
  int32_t t0;           // first frame (within the utterance) of this chunk
  int32_t nframes;      // frames in this chunk (<= 4*NF*16)
  int32_t pad;
};

struct K1Args {
  const float* feats;            // [sumT][D]
  const int64_t* frame_off;      // [U+1]
  const K1Chunk* chunks;
  const float* wimg;             // tile images, khg_tile_floats(KQ) floats each
  const int64_t* utt_tile_off;   // [U+1] offsets into utt_tiles
  const int32_t* utt_tiles;      // per utterance, walk order: W-tile id (bits 0-21) | first needed 16-frame tile of the pdf (22-28) | last tile of its pdf (31)
  float* ll;                     // per utterance: [npdf_u][tpad_u]
  const int64_t* ll_off;         // [U+1] float offsets
  int32_t* err_flag;             // bit 0 set on a NaN/Inf log-likelihood (decodable-am-diag-gmm.cc:63-65)
  int32_t D;
  int32_t interleave;            // deal frame tiles to the waves round-robin (reachable-only walks) instead of contiguously
};

// KQ = ceil(D/4) rounded to 10 or 20; a plane row holds KH = 2*KQ floats (one per MFMA step),
// padded to an ODD number of 16-byte slots so ds_read_b128 of 16 consecutive rows is conflict free
__host__ __device__ constexpr int khg_row_floats(int KQ) { return 4 * ((KQ / 2) | 1); }
// tile image: [q=4][32][row] W planes + [32] gconst, rounded up to a multiple of 256 floats (1 KiB =
// one LDS-DMA wave-instruction) so the DMA never needs a partial wave
__host__ __device__ constexpr int khg_tile_floats(int KQ) {
  return ((4 * 32 * khg_row_floats(KQ) + 32) + 255) / 256 * 256;
}

// What one wave owns of a chunk (wave-uniform).  The chunk's n16 = 4b + rem frame tiles are dealt as
// b contiguous full tiles per wave; the rem remainder tiles are shared by GAUSSIAN HALF so that no
// wave carries more than half a tile above the others (rem = 1: two waves take one half each of the
// same frame tile; rem = 2: four halves, one per wave; rem = 3: two waves take a full tile, two a half).
struct K1Work {
  int first;       // full tile f of this wave is frame tile first + 4*f (tiles are dealt round-robin, so the
                   // leading tiles a pdf does not need yet -- see the walk entries -- thin out all four waves alike)
  int stride;      // 4 (round-robin, reachable-only runs) or 1 (contiguous: LL rows are then written 256 B at a time)
  int last_tile;   // frame-tile id of full tile NA-1 (first+stride*(NA-1), or a remainder tile)
  int half_tile;   // frame-tile id of the shared half tile (HALF instantiations)
  int hsel;        // Gaussian half (rows 16*hsel..) of every W tile this wave evaluates for half_tile
  int sidx;        // which of the workgroup's two shared-tile exchange areas
};

// One wave's whole walk with a compile-time number NA of full 16-frame tiles (+ one half tile when
// HALF).  NA == 0 && !HALF: the wave only helps with the LDS-DMA and the barriers.  Barrier counts
// are identical for every instantiation, so waves of one workgroup may run different ones.
template <int KQ, int NA, bool HALF, bool ALIGNED>
__device__ __forceinline__ void k1_wave(const K1Args& a, const K1Chunk& ck, float* lds, float* mrg, float* shr, const K1Work wk, const int wave) {
  constexpr int KH = 2 * KQ;                 // MFMA steps (k = 4 per step)
  constexpr int ROW = khg_row_floats(KQ);
  constexpr int TILE = khg_tile_floats(KQ);
  constexpr int NDMA = TILE / 256;           // 1 KiB pieces per tile
  constexpr int NX = NA > 0 ? NA : 1;
  constexpr bool WORK = NA > 0 || HALF;
  const int lane = threadIdx.x & 63;         // `wave` arrives wave-uniform (SGPR) from the kernel
  const int r = lane & 15, q = lane >> 4;
  const int u = ck.utt;
  const int64_t f0 = a.frame_off[u];
  const int T = (int)(a.frame_off[u + 1] - f0);
  const int tpad = (T + 31) & ~31;
  const int D = a.D;

  // ---- B operands: xx_q[t][s] for my frame tiles, resident in registers ----
  auto load_x = [&](int tile, float (&dst)[KH]) {
    int t = ck.t0 + tile * 16 + r;
    if (t > T - 1) t = T - 1;  // padded frames recompute the last frame (results land in the row padding)
    const float* xp = a.feats + (f0 + t) * (int64_t)D;
#pragma unroll
    for (int j = 0; j < KQ; ++j) {
      f32x4 v;
      if (ALIGNED) {
        v = (4 * j < D) ? *reinterpret_cast<const f32x4*>(xp + 4 * j) : f32x4{0, 0, 0, 0};
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = (4 * j + i < D) ? xp[4 * j + i] : 0.0f;
      }
      const float e0 = (q & 1) ? v[1] : v[0], e1 = (q & 1) ? v[3] : v[2];   // d = 4j + {0,2} + parity
      dst[2 * j] = (q & 2) ? e0 * e0 : e0;
      dst[2 * j + 1] = (q & 2) ? e1 * e1 : e1;
    }
  };
  float xb[NX][KH];
  float xh[KH];
#pragma unroll
  for (int f = 0; f < NA; ++f) load_x(f == NA - 1 ? wk.last_tile : wk.first + wk.stride * f, xb[f]);
  if (HALF) load_x(wk.half_tile, xh);

  float* llu = a.ll + a.ll_off[u];

  // LDS-DMA of one tile image: 1 KiB per wave-instruction, NDMA pieces dealt to the 4 waves
  // (uniform base in SGPRs + one 32-bit lane offset: the DMA needs no per-instruction address VALU)
  const uint32_t lane_b = (uint32_t)lane * 16u;
  auto dma_tile = [&](int tile, int buf) {
    const char* src = reinterpret_cast<const char*>(a.wimg + (int64_t)tile * TILE);
#pragma unroll
    for (int i = 0; i < (NDMA + 3) / 4; ++i) {
      const int piece = wave + 4 * i;
      if (piece < NDMA) {
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) void*)(src + piece * 1024 + lane_b),
            (__attribute__((address_space(3))) void*)(lds + buf * TILE + piece * 256), 16, 0, 0);
      }
    }
  };

  // flat walk over the utterance's W tiles (host-built list, pdf-major), two tiles per barrier (LDS
  // ring of two tile pairs).  The list is fetched 64 entries at a time into one VGPR (lane k holds
  // entry k) a block ahead and read with v_readlane: no memory latency sits on the walk.
  const int64_t tl0 = a.utt_tile_off[u];
  const int ntl = (int)(a.utt_tile_off[u + 1] - tl0);
  const int32_t* tl = a.utt_tiles + tl0;
  int ent_cur = lane < ntl ? tl[lane] : 0;
  int ent_nxt = 64 + lane < ntl ? tl[64 + lane] : 0;
  if (ntl > 0) {
    dma_tile(__builtin_amdgcn_readlane(ent_cur, 0) & 0x3fffff, 0);
    if (ntl > 1) dma_tile(__builtin_amdgcn_readlane(ent_cur, 1) & 0x3fffff, 1);
  }
  __syncthreads();

  float m_run[NX], s_run[NX];
#pragma unroll
  for (int f = 0; f < NX; ++f) { m_run[f] = K1_MFLOOR; s_run[f] = 0.0f; }
  float m_h = K1_MFLOOR, s_h = 0.0f;
  f32x4 acc[NX][2];
  f32x4 acch = f32x4{0, 0, 0, 0};

  // M: the MFMA phase of one W tile -> acc (both Gaussian halves of the full tiles, one of the half tile)
  // FS = first full tile this pdf needs (tiles 0..FS-1 of the wave lie wholly before the first frame a
  // decoder token can read the pdf at): a compile-time constant so the accumulators stay in registers
  auto mfma_phase = [&](int bufidx, auto fs_c) {
    constexpr int FS = decltype(fs_c)::value;
    const float* wt = lds + bufidx * TILE;
    const float* wrow0 = wt + (q * 32 + r) * ROW;        // Gaussians 0..15 of the tile
    const float* wrow1 = wrow0 + 16 * ROW;               // Gaussians 16..31
    const float* wrowh = wrow0 + wk.hsel * 16 * ROW;
    const float* gc = wt + 4 * 32 * ROW;
    // C input of the first step = gconst[row], rows 4*q + reg (+16 for the second block)
    f32x4 g0 = {0, 0, 0, 0}, g1 = g0, gh = g0, a0 = g0, a1 = g0, ah = g0;
    if (NA > FS) {
      g0 = *reinterpret_cast<const f32x4*>(gc + 4 * q);
      g1 = *reinterpret_cast<const f32x4*>(gc + 16 + 4 * q);
      a0 = *reinterpret_cast<const f32x4*>(wrow0);
      a1 = *reinterpret_cast<const f32x4*>(wrow1);
    }
    if (HALF) {
      gh = *reinterpret_cast<const f32x4*>(gc + 16 * wk.hsel + 4 * q);
      ah = *reinterpret_cast<const f32x4*>(wrowh);
    }
#pragma unroll
    for (int s4 = 0; s4 < KH / 4; ++s4) {
      f32x4 nn0 = a0, nn1 = a1, nnh = ah;
      if (s4 + 1 < KH / 4) {                             // A operands one 4-step group ahead
        if (NA > FS) {
          nn0 = *reinterpret_cast<const f32x4*>(wrow0 + 4 * (s4 + 1));
          nn1 = *reinterpret_cast<const f32x4*>(wrow1 + 4 * (s4 + 1));
        }
        if (HALF) nnh = *reinterpret_cast<const f32x4*>(wrowh + 4 * (s4 + 1));
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int f = FS; f < NA; ++f) {
          acc[f][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[i], xb[f][4 * s4 + i], (s4 == 0 && i == 0) ? g0 : acc[f][0], 0, 0, 0);
          acc[f][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[i], xb[f][4 * s4 + i], (s4 == 0 && i == 0) ? g1 : acc[f][1], 0, 0, 0);
        }
        if (HALF) acch = __builtin_amdgcn_mfma_f32_16x16x4f32(ah[i], xh[4 * s4 + i], (s4 == 0 && i == 0) ? gh : acch, 0, 0, 0);
      }
      a0 = nn0; a1 = nn1; ah = nnh;
    }
  };
  // E: online log-sum-exp, per LANE over the 8 (half tile: 4) Gaussians it holds of the tile in acc
  // (no cross-lane traffic per tile); the four lane quarters of a frame are merged once per pdf.
  // fp32 VALU work is NOT hidden behind fp32 MFMAs on CDNA4 (tools/mfma_coissue.hip: every VALU
  // instruction between MFMAs costs its ~4 issue cycles of MFMA time, a transcendental ~10), so
  // the epilogue is written for instruction count: v_max3, packed v_pk_{add,mul}_f32 for the
  // subtract / scale / sums, and a finite floor (-3e38) for the running max so that no -inf
  // guard is needed (exp2(-inf) = 0 covers padded Gaussians).
  auto epilogue_main = [&](auto fs_c) {
    constexpr int FS = decltype(fs_c)::value;
    const f32x2 l2e = f32x2{1.44269504088896340736f, 1.44269504088896340736f};
    // k1_max3 is inline asm: the compiler's MFMA->VALU hazard recognizer does not see its reads of
    // the accumulators.  Nothing may move across this point, and 12 wait states (> the 11 an
    // 8-pass MFMA result needs before a VALU read) pass before the first read.  The s_nops idle
    // only this wave; the SIMD's other wave keeps the MFMA pipe busy meanwhile.
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_nop 7\n\ts_nop 3");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int f = FS; f < NA; ++f) {
      const f32x4 c0 = acc[f][0], c1 = acc[f][1];
      const float mnew = k1_max3(k1_max3(c0[0], c0[1], c0[2]), k1_max3(c0[3], c1[0], c1[1]), k1_max3(c1[2], c1[3], m_run[f]));
      const f32x2 mm = f32x2{mnew, mnew};
      const f32x2 d0 = (f32x2{c0[0], c0[1]} - mm) * l2e, d1 = (f32x2{c0[2], c0[3]} - mm) * l2e;
      const f32x2 d2 = (f32x2{c1[0], c1[1]} - mm) * l2e, d3 = (f32x2{c1[2], c1[3]} - mm) * l2e;
      const f32x2 e0 = f32x2{__builtin_amdgcn_exp2f(d0[0]), __builtin_amdgcn_exp2f(d0[1])};
      const f32x2 e1 = f32x2{__builtin_amdgcn_exp2f(d1[0]), __builtin_amdgcn_exp2f(d1[1])};
      const f32x2 e2 = f32x2{__builtin_amdgcn_exp2f(d2[0]), __builtin_amdgcn_exp2f(d2[1])};
      const f32x2 e3 = f32x2{__builtin_amdgcn_exp2f(d3[0]), __builtin_amdgcn_exp2f(d3[1])};
      const f32x2 ss = (e0 + e1) + (e2 + e3);
      const float sc = __builtin_amdgcn_exp2f((m_run[f] - mnew) * 1.44269504088896340736f);
      s_run[f] = __builtin_fmaf(s_run[f], sc, ss[0] + ss[1]);
      m_run[f] = mnew;
    }
    if (HALF) {
      const f32x4 c0 = acch;
      const float mnew = k1_max3(k1_max3(c0[0], c0[1], c0[2]), c0[3], m_h);
      const f32x2 mm = f32x2{mnew, mnew};
      const f32x2 d0 = (f32x2{c0[0], c0[1]} - mm) * l2e, d1 = (f32x2{c0[2], c0[3]} - mm) * l2e;
      const f32x2 e0 = f32x2{__builtin_amdgcn_exp2f(d0[0]), __builtin_amdgcn_exp2f(d0[1])};
      const f32x2 e1 = f32x2{__builtin_amdgcn_exp2f(d1[0]), __builtin_amdgcn_exp2f(d1[1])};
      const f32x2 ss = e0 + e1;
      const float sc = __builtin_amdgcn_exp2f((m_h - mnew) * 1.44269504088896340736f);
      s_h = __builtin_fmaf(s_h, sc, ss[0] + ss[1]);
      m_h = mnew;
    }
  };
  // pdf finished: the 4 lane quarters' (max, sum) partials of every owned frame go through a
  // wave-private LDS transpose ([f][frame][quarter]) so that each LANE finishes one (tile, frame)
  // pair -- 64 pairs per round instead of 16 -- and the LL row is written 256 B contiguous.
  // LL = max + log(sum).
  // (efa: the pdf's first needed 16-frame tile of the utterance; tiles in front of it that were computed all the same -- the
  //  compiled variants skip at most KFS -- are not written: nobody reads them)
  auto epilogue_merge = [&](int wj, int fs, int efa) {
    float* mm_ = mrg;                             // [NX][16][4] maxima
    float* ms_ = mrg + ((NX + 3) / 4) * 256;      // [NX][16][4] sums (regions padded to whole rounds)
#pragma unroll
    for (int f = 0; f < NA; ++f) {
      mm_[f * 64 + r * 4 + q] = m_run[f];
      ms_[f * 64 + r * 4 + q] = s_run[f];
      m_run[f] = K1_MFLOOR;
      s_run[f] = 0.0f;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int rd = 0; rd < (NA + 3) / 4; ++rd) {
      // lane L finishes tile f = 4*rd + L/16, frame L%16: element index (f*16 + frame) = 64*rd + L
      const f32x4 m4 = *reinterpret_cast<const f32x4*>(mm_ + rd * 256 + lane * 4);
      const f32x4 s4 = *reinterpret_cast<const f32x4*>(ms_ + rd * 256 + lane * 4);
      const float M = k1_max3(k1_max3(m4[0], m4[1], m4[2]), m4[3], m4[3]);
      const f32x2 MM = f32x2{M, M};
      const f32x2 l2e = f32x2{1.44269504088896340736f, 1.44269504088896340736f};
      const f32x2 d0 = (f32x2{m4[0], m4[1]} - MM) * l2e, d1 = (f32x2{m4[2], m4[3]} - MM) * l2e;
      const f32x2 t0 = f32x2{s4[0], s4[1]} * f32x2{__builtin_amdgcn_exp2f(d0[0]), __builtin_amdgcn_exp2f(d0[1])};
      const f32x2 t1 = f32x2{s4[2], s4[3]} * f32x2{__builtin_amdgcn_exp2f(d1[0]), __builtin_amdgcn_exp2f(d1[1])};
      const f32x2 tt = t0 + t1;
      const float v = M + __builtin_amdgcn_logf(tt[0] + tt[1]) * 0.69314718055994530942f;
      const int f = 4 * rd + q;
      const bool live = f < NA && f >= fs;       // tiles the pdf does not need yet were skipped: nothing to write
      const int t = ck.t0 + (f == NA - 1 ? wk.last_tile : wk.first + wk.stride * f) * 16 + r;
      if (live && t < tpad && (t >> 4) >= efa) llu[(int64_t)wj * tpad + t] = v;
      if (live && t < T && !(fabsf(v) <= 3.0e38f)) atomicOr(a.err_flag, 1);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  };
  // half tile, pdf finished: publish my half's (max, sum) partials [frame][quarter] in the
  // workgroup's exchange area; the two owners take turns (by pdf) finishing the frames after the next barrier.
  // Slot = (shared tile, barrier interval parity, tile of the pair); layout [half][m|s][16][4].
  auto half_publish = [&](int par, int tip) {
    float* sl = shr + ((wk.sidx * 2 + par) * 2 + tip) * 256 + wk.hsel * 128;
    sl[r * 4 + q] = m_h;
    sl[64 + r * 4 + q] = s_h;
    m_h = K1_MFLOOR;
    s_h = 0.0f;
  };
  auto half_finish = [&](int par, int tip, int wj, int efa) {
    const float* sl = shr + ((wk.sidx * 2 + par) * 2 + tip) * 256;
    const f32x4 ma = *reinterpret_cast<const f32x4*>(sl + r * 4), sa = *reinterpret_cast<const f32x4*>(sl + 64 + r * 4);
    const f32x4 mb = *reinterpret_cast<const f32x4*>(sl + 128 + r * 4), sb = *reinterpret_cast<const f32x4*>(sl + 192 + r * 4);
    const float M = k1_max3(k1_max3(ma[0], ma[1], ma[2]), k1_max3(ma[3], mb[0], mb[1]), k1_max3(mb[2], mb[3], mb[3]));
    const f32x2 MM = f32x2{M, M};
    const f32x2 l2e = f32x2{1.44269504088896340736f, 1.44269504088896340736f};
    const f32x2 d0 = (f32x2{ma[0], ma[1]} - MM) * l2e, d1 = (f32x2{ma[2], ma[3]} - MM) * l2e;
    const f32x2 d2 = (f32x2{mb[0], mb[1]} - MM) * l2e, d3 = (f32x2{mb[2], mb[3]} - MM) * l2e;
    const f32x2 t0 = f32x2{sa[0], sa[1]} * f32x2{__builtin_amdgcn_exp2f(d0[0]), __builtin_amdgcn_exp2f(d0[1])};
    const f32x2 t1 = f32x2{sa[2], sa[3]} * f32x2{__builtin_amdgcn_exp2f(d1[0]), __builtin_amdgcn_exp2f(d1[1])};
    const f32x2 t2 = f32x2{sb[0], sb[1]} * f32x2{__builtin_amdgcn_exp2f(d2[0]), __builtin_amdgcn_exp2f(d2[1])};
    const f32x2 t3 = f32x2{sb[2], sb[3]} * f32x2{__builtin_amdgcn_exp2f(d3[0]), __builtin_amdgcn_exp2f(d3[1])};
    const f32x2 tt = (t0 + t1) + (t2 + t3);
    const float v = M + __builtin_amdgcn_logf(tt[0] + tt[1]) * 0.69314718055994530942f;
    const int t = ck.t0 + wk.half_tile * 16 + r;
    if (q == 0 && t < tpad && (t >> 4) >= efa) llu[(int64_t)wj * tpad + t] = v;
    if (q == 0 && t < T && !(fabsf(v) <= 3.0e38f)) atomicOr(a.err_flag, 1);
  };

  constexpr int KFS = NA > 2 ? 2 : (NA > 1 ? 1 : 0);   // largest compiled 'first needed tile'
  const int ef0 = ck.t0 >> 4;                 // chunks start on 16-frame boundaries
  int pair = 0;                               // which pair of LDS buffers holds the current two tiles
  int j = 0;                                  // local pdf index of tile `it`
  int pend0 = -1, pend1 = -1;                 // pdfs whose half-tile partials were published in the previous interval
  int pend0e = 0, pend1e = 0;                 // ... and their first needed 16-frame tiles
  for (int it = 0; it < ntl; it += 2) {
    // entries it, it+1 come from ent_cur; it+2, it+3 from ent_cur or (at a block edge) ent_nxt
    const int li = it & 63;
    const int e0 = __builtin_amdgcn_readlane(ent_cur, li);
    const int e1 = __builtin_amdgcn_readlane(ent_cur, li + 1);      // li is even, so li+1 <= 63
    const bool has1 = it + 1 < ntl;
    int f0e, f1e;
    if (li == 62) { f0e = __builtin_amdgcn_readlane(ent_nxt, 0); f1e = __builtin_amdgcn_readlane(ent_nxt, 1); }
    else { f0e = __builtin_amdgcn_readlane(ent_cur, li + 2); f1e = __builtin_amdgcn_readlane(ent_cur, li + 3); }
    if (it + 2 < ntl) dma_tile(f0e & 0x3fffff, 2 * (pair ^ 1));
    if (it + 3 < ntl) dma_tile(f1e & 0x3fffff, 2 * (pair ^ 1) + 1);
    if (li == 62) {                           // next block becomes current; fetch the one after it
      ent_cur = ent_nxt;
      const int nb = (it + 2) + 64 + lane;
      ent_nxt = nb < ntl ? tl[nb] : 0;
    }
    int cur0 = -1, cur1 = -1, cur0e = 0, cur1e = 0;
    if (WORK) {
      if (HALF) {                             // finish what both halves published before the last barrier
        if (pend0 >= 0 && (pend0 & 1) == wk.hsel) half_finish(pair ^ 1, 0, pend0, pend0e);   // the two owners alternate by pdf
        if (pend1 >= 0 && (pend1 & 1) == wk.hsel) half_finish(pair ^ 1, 1, pend1, pend1e);
      }
      // one W tile: MFMA phase + epilogue over the wave's tiles the pdf needs (full tile f is frame tile
      // first + stride*f of the chunk; needed iff it is not wholly before the pdf's first readable frame)
      auto step = [&](int e, int bufidx, int tip, int& cur, int& cure) {
        const int ef = ((e >> 22) & 0x7f) - ef0;                       // first needed frame tile, chunk-relative
        int fs = ef <= wk.first ? 0 : (wk.stride == 4 ? (ef - wk.first + 3) >> 2 : ef - wk.first);
        fs = fs > KFS ? KFS : fs;                                      // compiled variants: 0..KFS (less skipping is still correct)
        if (fs >= 2) { mfma_phase(bufidx, std::integral_constant<int, (NA > 2 ? 2 : 0)>()); epilogue_main(std::integral_constant<int, (NA > 2 ? 2 : 0)>()); }
        else if (fs == 1) { mfma_phase(bufidx, std::integral_constant<int, (NA > 1 ? 1 : 0)>()); epilogue_main(std::integral_constant<int, (NA > 1 ? 1 : 0)>()); }
        else { mfma_phase(bufidx, std::integral_constant<int, 0>()); epilogue_main(std::integral_constant<int, 0>()); }
        if (e < 0) {
          if (NA > 0) epilogue_merge(j, fs, (e >> 22) & 0x7f);
          if (HALF) { half_publish(pair, tip); cur = j; cure = (e >> 22) & 0x7f; }
          ++j;
        }
      };
      step(e0, 2 * pair, 0, cur0, cur0e);
      if (has1) step(e1, 2 * pair + 1, 1, cur1, cur1e);
    }
    pend0 = cur0; pend1 = cur1; pend0e = cur0e; pend1e = cur1e;
    __syncthreads();  // the next pair's DMA has landed (vmcnt(0) + barrier); this pair is free
    pair ^= 1;
  }
  if (HALF) {
    if (pend0 >= 0 && (pend0 & 1) == wk.hsel) half_finish(pair ^ 1, 0, pend0, pend0e);
    if (pend1 >= 0 && (pend1 & 1) == wk.hsel) half_finish(pair ^ 1, 1, pend1, pend1e);
  }
}

// NF = most 16-frame tiles a wave may own (chunks hold <= 4*NF*16 frames); WPS = waves per SIMD
// the register budget is sized for.
template <int KQ, int NF, bool ALIGNED, int WPS>
__global__ __launch_bounds__(256, WPS) void k1_loglikes(K1Args a) {
  constexpr int TILE = khg_tile_floats(KQ);
  __shared__ __attribute__((aligned(16))) float lds[4 * TILE];
  __shared__ __attribute__((aligned(16))) float s_mrg[4][2 * ((NF + 3) / 4) * 256];   // per-wave merge transpose
  __shared__ __attribute__((aligned(16))) float s_shr[2 * 2 * 2 * 256];                // half-tile exchange areas
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const K1Chunk ck = a.chunks[blockIdx.x];
  if (ck.nframes <= 0) return;
  // Which wave gets the remainder work is decided by the SIMD it actually runs on (HW_REG_HW_ID):
  // the two workgroups that share a CU put their heavy waves on complementary SIMDs (rank offset
  // by 2 for the workgroup in the odd wave slot), so per-SIMD MFMA work evens out.  Any bijection
  // wave -> rank is correct; if the four waves do not sit on four distinct SIMDs the rank falls
  // back to the wave index.
  __shared__ int s_hw[4];
  const int simd_id = __builtin_amdgcn_s_getreg((4) | (4 << 6) | (1 << 11));   // HW_ID[5:4]
  const int slot_id = __builtin_amdgcn_s_getreg((4) | (0 << 6) | (3 << 11));   // HW_ID[3:0]
  if ((threadIdx.x & 63) == 0) s_hw[wave] = simd_id | (slot_id << 8);
  __syncthreads();
  const int h0 = s_hw[0], h1 = s_hw[1], h2 = s_hw[2], h3 = s_hw[3];
  const int mask = (1 << (h0 & 3)) | (1 << (h1 & 3)) | (1 << (h2 & 3)) | (1 << (h3 & 3));
  const int rank = (mask == 0xF) ? ((simd_id + 2 * ((h0 >> 8) & 1)) & 3) : wave;
  // n16 = 4b + rem frame tiles: b full tiles per rank (rank, rank+4, ...), the remainder shared by Gaussian half
  const int n16 = (ck.nframes + 15) >> 4;
  const int b = n16 >> 2, rem = n16 & 3;
  K1Work wk;
  wk.stride = a.interleave ? 4 : 1;
  wk.first = a.interleave ? rank : rank * b; wk.last_tile = wk.first + wk.stride * (b - 1); wk.half_tile = 0; wk.hsel = 0; wk.sidx = 0;
  int na = b;
  bool half = false;
  if (rem == 1) { if (rank < 2) { half = true; wk.half_tile = 4 * b; wk.hsel = rank; } }
  else if (rem == 2) { half = true; wk.half_tile = 4 * b + (rank >> 1); wk.hsel = rank & 1; wk.sidx = rank >> 1; }
  else if (rem == 3) {
    if (rank < 2) { na = b + 1; wk.last_tile = 4 * b + rank; }
    else { half = true; wk.half_tile = 4 * b + 2; wk.hsel = rank - 2; }
  }
  float* mrg = s_mrg[wave];
#define K1_CASE(N)                                                                                      \
    case 2 * N: if constexpr (N <= NF) k1_wave<KQ, N, false, ALIGNED>(a, ck, lds, mrg, s_shr, wk, wave); break; \
    case 2 * N + 1: if constexpr (N < NF) k1_wave<KQ, N, true, ALIGNED>(a, ck, lds, mrg, s_shr, wk, wave); break;
  switch (2 * na + (half ? 1 : 0)) {
    K1_CASE(0) K1_CASE(1) K1_CASE(2) K1_CASE(3) K1_CASE(4) K1_CASE(5) K1_CASE(6)
    default: break;
  }
#undef K1_CASE
}
