// K2: batched Viterbi forced alignment, one workgroup per utterance.
//
// Replaces (reference, /root/reference/kaldi-hmm-gmm/csrc/):
//   decoder-wrappers.cc:16-108   AlignUtteranceWrapper (status / retry / like semantics)
//   faster-decoder.cc:41-240     InitDecoding / ProcessEmitting / ProcessNonemitting
//   faster-decoder.cc:243-335    GetCutoff (beam, min_active)
//   faster-decoder.cc:346-423    ReachedFinal / GetBestPath
//   decodable-am-diag-gmm.h:95-98  scale * LL(frame, id2pdf[tid])   (scores come from K1)
//   hmm-utils.cc:465-493         AddTransitionProbs (arc.w + trans_cost[tid], float add)
//
// Two kernels:
//  * k2_viterbi_dp   exact frame-synchronous min-plus DP in the reference's token arithmetic
//    (double path cost = (prev + double(arc.w)) + double(float(-(scale*ll))), faster-decoder.h:125).
//    It proves, per utterance, a *beam certificate*: every node of the optimal path lies
//    strictly inside `beam` of the exact frame minimum (or the frame has <= min_active live
//    states, where GetCutoff disables pruning).  The reference's token costs are >= the DP's,
//    so under the certificate FasterDecoder cannot prune that path in ANY HashList order and
//    returns exactly it.  No certificate, or any exact cost tie -> the utterance is handed to
//  * k2_viterbi_faithful   a serial, order-faithful emulation of FasterDecoder + HashList
//    (insertion-ordered token list, running next_weight_cutoff, float tmp_array_ in GetCutoff,
//    retry beam), run by one lane per utterance.

struct K2Args {
  // utterance set
  const int64_t* frame_off;   // [U+1]
  const int32_t* gidx;        // [U] the row of state_off / start an utterance decodes on (identity; zeros on a shared graph)
  const int64_t* state_off;   // [rows+1]
  const int32_t* start;       // [U]
  const int64_t* in_off;      // [sumS+1]  in-arcs (by destination), global offsets
  const int32_t* in_src;      // local source state
  const int32_t* in_col;      // column into the utterance's ll matrix; -1 for epsilon-input arcs
  const int32_t* in_tid;      // ilabel
  const int32_t* in_olabel;
  const float* in_w;          // base graph weight
  const int64_t* out_off;     // [sumS+1]  out-arcs (by source, original order) for the faithful kernel
  const int32_t* out_inidx;   // out-arc -> index of the same arc in the in-arc arrays (utterance-local)
  const float* final_w;       // [sumS]
  const float* trans_cost;    // [num_tids+1] or nullptr
  const float* ll;            // K1 output
  const int64_t* ll_off;      // [U+1]
  // scratch
  uint8_t* bp;                // per utterance [(T+1)][S]
  const int64_t* bp_off;      // [U+1]
  double* layer_best;         // per utterance [T+1]   (offset frame_off[u] + u)
  int32_t* layer_cnt;         // per utterance [T+1]
  int32_t* path;              // per utterance [T + S + 8] (offset path_off[u])
  const int64_t* path_off;    // [U+1]
  // outputs
  int32_t* ali;               // [sumT]
  // Split mode (khg_align without host outputs on a large set; khg_k2.hip): the order-faithful decoders write THEIR alignments to a
  // second buffer while K3 already accumulates the certified utterances from `ali` (khg_k3.hip); the DP kernel zero-fills the
  // range of an utterance it could not certify, flags it in unc[] and counts it (utterances, frames) in unc_cnt[] (device memory; the
  // host reads a copy behind the kernel).  Otherwise ali_fb == ali and unc == nullptr.
  int32_t* ali_fb;            // [sumT] where the order-faithful decoders write
  int32_t* unc;               // [U] or nullptr
  int32_t* unc_cnt;           // [2] or nullptr
  int32_t* words;             // per utterance capacity words_off[u+1]-words_off[u]
  const int64_t* words_off;   // [U+1]
  int32_t* num_words;         // [U]
  float* like;                // [U]
  int32_t* status;            // [U]
  int32_t* err_flag;          // bit 1: K1 NaN/Inf, bit 2: K2 internal overflow
  long long* prof;            // diagnostics (KHG_K2_PROF=1): [U][8] s_memtime stamps, else nullptr
  // config
  float beam, retry_beam, acoustic_scale, like_scale, beam_delta, hash_ratio;
  int32_t max_active, min_active;
  int32_t max_states, max_inarcs;  // LDS sizing (max over the batch)
  // graphs whose tables do not fit the 160 KB of LDS (a large decoding graph): the GMEM instantiations carve the same
  // tables out of a per-utterance slice of this HBM scratch instead (gscratch + utterance * gscratch_stride)
  unsigned char* gscratch;
  int64_t gscratch_stride;
  // k2_viterbi_dp: workgroup b takes utterance order[b] (longest first: the grid then drains on short utterances), or b
  const int32_t* order;
  // k2_viterbi_dp's tail (KHG_OPT_K2_TAIL): 0 the trace-back on packed source words and the scanned replay, 1 the loops they replaced
  int32_t tail_off;
};

#ifndef K2_WAVES_PER_EU
#define K2_WAVES_PER_EU 5          // register budget of the DP kernel: 5 waves per SIMD = 96 VGPRs (it used 104: four waves)
#endif
// measurement builds: either part of the tail (KHG_OPT_K2_TAIL) alone
#ifndef K2_TAIL_TRACE
#define K2_TAIL_TRACE 1
#endif
#ifndef K2_TAIL_REPLAY
#define K2_TAIL_REPLAY 1
#endif
#define K2_BP_NONE 255
#define K2_ST_NEED_FALLBACK 16   // internal: certificate failed, run the faithful kernel

__device__ __forceinline__ unsigned long long k2_d2key(double d) {
  unsigned long long b = (unsigned long long)__double_as_longlong(d);
  return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double k2_key2d(unsigned long long k) {
  unsigned long long b = (k & 0x8000000000000000ull) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)b);
}

// Shared tail of both kernels: trace back through bp[], then replay the path forward in the
// token arithmetic to produce alignment, words, `like` (decoder-wrappers.cc:93-95 via
// faster-decoder.cc:390-419) and, when `certify`, the beam certificate.
// Runs on ONE thread.  Returns status bits.
__device__ int k2_finish(const K2Args& a, int u, int best_state, const int32_t* s_in_off,
                         const int32_t* s_src, const int32_t* s_col, const float* s_w,
                         bool certify, bool* certified) {
  const int64_t f0 = a.frame_off[u];
  const int T = (int)(a.frame_off[u + 1] - f0);
  const int tpad = (T + 31) & ~31;
  const int S = (int)(a.state_off[a.gidx[u] + 1] - a.state_off[a.gidx[u]]);
  const int64_t in0 = a.in_off[a.state_off[a.gidx[u]]];
  const uint8_t* bp = a.bp + a.bp_off[u];
  int32_t* path = a.path + a.path_off[u];
  const int path_cap = (int)(a.path_off[u + 1] - a.path_off[u]);
  const float* llu = a.ll + a.ll_off[u];
  const double* lbest = a.layer_best + f0 + u;
  const int32_t* lcnt = a.layer_cnt + f0 + u;

  int n = 0, layer = T, s = best_state;
  bool overflow = false;
  while (true) {
    int ord = bp[(int64_t)layer * ((S + 15) & ~15) + s];
    if (ord == K2_BP_NONE) break;
    int ai = s_in_off[s] + ord;
    if (n >= path_cap) { overflow = true; break; }
    path[n++] = ai;
    if (s_col[ai] >= 0) --layer;
    s = s_src[ai];
  }
  if (overflow || layer != 0) return KHG_ALIGN_ERROR;

  double cost = 0.0;
  float v1 = 0.0f, v2 = 0.0f;
  int t = 0, nw = 0;
  const int64_t wcap = a.words_off[u + 1] - a.words_off[u];
  int32_t* words = a.words + a.words_off[u];
  bool ok = true;
  const double beam = (double)a.beam;
  auto node_ok = [&](double c, int L) {
    if (c < lbest[L] + beam) return true;
    return lcnt[L] <= a.min_active && (L == 0 || lcnt[L - 1] <= a.min_active);
  };
  if (certify) ok = node_ok(0.0, 0);
  for (int i = n - 1; i >= 0; --i) {
    int ai = path[i];
    float w = s_w[ai];
    double ncost;
    int col = s_col[ai];
    if (col >= 0) {
      float ac = -1 * (a.acoustic_scale * llu[(int64_t)col * tpad + t]);
      ncost = (cost + w) + ac;                       // faster-decoder.h:125
      a.ali_fb[f0 + t] = a.in_tid[in0 + ai];
      ++t;
    } else {
      ncost = cost + w;                              // faster-decoder.h:135
    }
    float tot_cost = (float)(ncost - cost);          // faster-decoder.cc:393
    float ac_cost = tot_cost - w;
    v1 = w + v1;                                     // LatticeWeight Times, path order
    v2 = ac_cost + v2;
    int ol = a.in_olabel[in0 + ai];
    if (ol != 0) { if (nw < wcap) words[nw] = ol; ++nw; }
    cost = ncost;
    if (certify && ok) ok = node_ok(cost, t);
  }
  v1 = a.final_w[a.state_off[a.gidx[u]] + best_state] + v1;  // faster-decoder.cc:415-417
  v2 = 0.0f + v2;
  a.num_words[u] = nw;
  a.like[u] = -(v1 + v2) / a.like_scale;         // decoder-wrappers.cc:95
  if (certified) *certified = ok;
  if (nw > wcap) return KHG_ALIGN_ERROR;
  return KHG_ALIGN_DONE;
}

// ---------------------------------------------------------------------------------------
// Exact DP: one workgroup per utterance, one destination state per thread (KS states when the
// graph has more than 1024 states).  A lone wave issues one instruction every 4-8 cycles, so the
// frame loop is issue bound: spreading the states over several waves (instead of striding them
// over one) is what fills the SIMDs.
//
// LDS holds the in-arc table, the two state-cost vectors and a 32-frame block of pre-scaled
// acoustic costs.  Fast path (no epsilon-input arcs, in-degree <= DEG): every thread keeps its
// in-arcs in registers and the back-pointers are 2 bits per state, packed with two ballots per
// wave and frame, parked in LDS and written to HBM once per 32 layers as whole lines -- no
// vector-memory instruction sits on the frame loop.  Generic path: CSR loop over LDS arcs, one
// back-pointer byte per state.
struct K2Arc { uint16_t src; int16_t col; float w; };   // 8 B (host checks S <= 65535, pdfs/utt <= 32767)

#define K2_FB 32   // layers per back-pointer / certificate block
#define K2_SB 16   // frames per staged score block (generic path)
#define K2_MAXW 16 // waves per workgroup

__device__ __forceinline__ void k2_lds_sync() {   // single-wave section: LDS visibility only
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ void k2_block_sync() { // workgroup barrier that does NOT drain vmcnt
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}
__device__ __forceinline__ void k2_global_sync() { // wave-local: global writes of other lanes visible
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}
// Wave-wide float minimum without LDS round trips: v_min_f32 with the DPP permutation applied to its first
// operand (row_ror 8,4,2,1, then row_bcast:15 / row_bcast:31 fold the four rows: six instructions; the inputs are
// never NaN, so no canonicalisation).  The wave minimum ends in LANE 63 only.  The s_nops are the VALU-write ->
// DPP-read wait states.
__device__ __forceinline__ float k2_wave_minf_lane63(float v) {
  asm volatile("s_nop 1\n\t"
               "v_min_f32_dpp %0, %0, %0 row_ror:8 row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"
               "v_min_f32_dpp %0, %0, %0 row_ror:4 row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"
               "v_min_f32_dpp %0, %0, %0 row_ror:2 row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"
               "v_min_f32_dpp %0, %0, %0 row_ror:1 row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"
               "v_min_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\ts_nop 1\n\t"
               "v_min_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\ts_nop 1"
               : "+v"(v));
  return v;
}
__device__ __forceinline__ double k2_wave_min(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { double t = __shfl_xor(v, o); v = t < v ? t : v; }
  return v;
}
// a double moved across lanes by DPP (two 32-bit moves); a lane whose source lane does not exist keeps `old`
template <int CTRL, int ROWMASK>
__device__ __forceinline__ double k2_dpp_d(double old, double v) {
  const int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(v), CTRL, ROWMASK, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(v), CTRL, ROWMASK, 0xf, false);
  return __hiloint2double(hi, lo);
}
// Inclusive wave scan of doubles by DPP, lane k <- v[0] + ... + v[k] in tree order: four shifts inside the rows of 16 lanes, then lane
// 15 of rows 0 / 2 into rows 1 / 3 and lane 31 into rows 2 and 3.  A lane without a source adds +0.  (The replay's cost chain, where
// every one of these additions is exact, and its running sum of magnitudes.)
__device__ __forceinline__ double k2_wave_scand(double v) {
  v += k2_dpp_d<0x111, 0xf>(0.0, v);      // row_shr:1
  v += k2_dpp_d<0x112, 0xf>(0.0, v);      // row_shr:2
  v += k2_dpp_d<0x114, 0xf>(0.0, v);      // row_shr:4
  v += k2_dpp_d<0x118, 0xf>(0.0, v);      // row_shr:8
  v += k2_dpp_d<0x142, 0xa>(0.0, v);      // row_bcast:15 -> rows 1, 3
  v += k2_dpp_d<0x143, 0xc>(0.0, v);      // row_bcast:31 -> rows 2, 3
  return v;
}
__device__ __forceinline__ double k2_readlane_d(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
__device__ __forceinline__ double k2_wave_sumd(double v) { return k2_readlane_d(k2_wave_scand(v), 63); }   // uniform
__device__ __forceinline__ unsigned k2_wave_minu(unsigned v) {                                             // uniform
  v = min(v, (unsigned)__builtin_amdgcn_update_dpp(-1, (int)v, 0x111, 0xf, 0xf, false));
  v = min(v, (unsigned)__builtin_amdgcn_update_dpp(-1, (int)v, 0x112, 0xf, 0xf, false));
  v = min(v, (unsigned)__builtin_amdgcn_update_dpp(-1, (int)v, 0x114, 0xf, 0xf, false));
  v = min(v, (unsigned)__builtin_amdgcn_update_dpp(-1, (int)v, 0x118, 0xf, 0xf, false));
  v = min(v, (unsigned)__builtin_amdgcn_update_dpp(-1, (int)v, 0x142, 0xa, 0xf, false));
  v = min(v, (unsigned)__builtin_amdgcn_update_dpp(-1, (int)v, 0x143, 0xc, 0xf, false));
  return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ int k2_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float k2_round_down(double d) {   // largest float <= d
  float f = (float)d;
  if ((double)f > d) f = __int_as_float(__float_as_int(f) + (f > 0.0f ? -1 : (f < 0.0f ? 1 : (int)0x80000001)));
  return f;
}

// back-pointer nibble of the register-resident path -> (in-arc ordinal or all ones = none, tie bit); see the layer loop for the two codes
template <int DEG, int NB>
__device__ __forceinline__ void k2_decode_nibble(int nib, int& ord, int& tie) {
  if constexpr (DEG == 2) { ord = (nib & 1) ? 0 : ((nib & 2) ? 1 : (1 << NB) - 1); tie = (nib & 3) == 3 ? 1 : 0; }
  else { ord = nib & ((1 << NB) - 1); tie = (nib >> NB) & 1; }
}

// SC: every state's in-arcs read the SAME score row (what AddSelfLoops with reorder = true leaves: the forward arc into a state and
// the state's self-loop carry transition-ids of one pdf) -- one score block and one cost conversion per state instead of one per slot.
// (one state per thread: K2_WAVES_PER_EU waves per SIMD; more: blocks of up to 1024 threads, four waves per SIMD = 128 registers)
//
// LAD, the ladder form of <1, 2, true, false, *> (chosen on the host, k2_plan: every graph of the batch has its states in chain
// order -- the in-arcs of state s come from s itself and from s - 1, at most one of either -- and at most 256 states): a layer needs no
// exchange through LDS.  The self-loop's source cost is the lane's own register, the forward arc's is the neighbouring lane's, one
// wave shift (DPP) away; only lane 0 of wave w > 0 needs a value of another wave, lane 63 of wave w - 1.  The waves therefore run one
// group of eight layers apart: wave w - 1 leaves its lane-63 cost of every layer of a group in an 8-entry LDS strip (two strips, by
// group parity), ONE workgroup barrier per group publishes it, and wave w reads the strip a group later -- off the dependent chain,
// as the `old` operand of the shift, which lane 0 keeps.  T / 8 + nwave barriers per utterance instead of T, and no LDS write,
// barrier and gather between a layer's minimum and the next layer's adds.  Same candidates, same association, same tie rule: the two
// in-arc slots are only re-slotted (self, previous) in registers, each keeping the nibble bit of its own slot.
template <int KS, int DEG, bool FAST, bool GMEM = false, bool SC = false, bool LAD = false>
__global__ __attribute__((amdgpu_waves_per_eu(KS == 1 ? K2_WAVES_PER_EU : 4))) void k2_viterbi_dp(K2Args a) {
  static_assert(!LAD || (FAST && KS == 1 && DEG == 2 && !GMEM), "the ladder form is a variant of <1, 2, true, false, *>");
  extern __shared__ __attribute__((aligned(16))) unsigned char k2_lds[];
  unsigned char* const smem = GMEM ? a.gscratch + (size_t)blockIdx.x * a.gscratch_stride : k2_lds;
  constexpr int NS = FAST ? KS : 1;
  constexpr int NSD = FAST ? KS * DEG : 1;
  constexpr int NB = DEG <= 3 ? 2 : 3;          // fast path: back-pointer bits per state (arc ordinal; all ones = none), + 1 tie bit
  constexpr int BNONE = (1 << NB) - 1;
  const int u = a.order ? a.order[blockIdx.x] : (int)blockIdx.x;
  // The block is launched for the batch's largest graph; an utterance with fewer states keeps only the waves it
  // has states for (one state per thread) -- the others leave before the first barrier, which then only counts
  // the remaining waves.  Every per-block quantity below (strides, reductions, the packed back-pointer pitch)
  // uses this utterance's own nthr / nwave.
  const int tid = threadIdx.x, lane = tid & 63;
  const int nthr = min((int)blockDim.x, max(64, (((int)(a.state_off[a.gidx[u] + 1] - a.state_off[a.gidx[u]]) + (FAST ? KS : 1) - 1) / (FAST ? KS : 1) + 63) & ~63));
  if (tid >= nthr) return;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nwave = nthr >> 6;
  const int64_t f0 = a.frame_off[u];
  const int T = (int)(a.frame_off[u + 1] - f0);
  const int tpad = (T + 31) & ~31;
  const int64_t s0 = a.state_off[a.gidx[u]];
  const int S = (int)(a.state_off[a.gidx[u] + 1] - s0);
  const int64_t in0 = a.in_off[s0];
  const int A = (int)(a.in_off[s0 + S] - in0);
  const int start = a.start[a.gidx[u]];
  const int npdf = (int)((a.ll_off[u + 1] - a.ll_off[u]) / (tpad > 0 ? tpad : 1));
  const int PP = npdf | 1;   // odd pitch: the frame-major score block is bank-conflict free
  const int Sp = (S + 15) & ~15;                       // generic back-pointer row pitch (bytes)
  // fast path: a state's back-pointers are packed BY ITS OWN LANE, one nibble per layer (NB ordinal bits, all ones =
  // none, + 1 tie bit), eight layers per dword: word (layer >> 3) * GW + state, nibble layer & 7
  const int GW = FAST ? nthr * KS : 0;                // dwords per group of eight layers
  const int LB = Sp;                                  // generic path: bytes per layer of the global back-pointer image

  // LDS carve-up (sized by the host for the batch maximum; FAST needs no score block)
  // (its byte count: k2_lds_dp / k2_lds_dp_fast / k2_lds_dp_generic, khg_k2.hip)
  double* cur = reinterpret_cast<double*>(smem);                          // [max_states]
  double* nxt = cur + a.max_states;
  double* s_red = nxt + a.max_states;                 // [K2_MAXW] best-final reduction
  K2Arc* s_arc = reinterpret_cast<K2Arc*>(s_red + K2_MAXW);               // [max_inarcs]
  int32_t* s_in_off = reinterpret_cast<int32_t*>(s_arc + a.max_inarcs);   // [max_states+1]
  float* s_wmin = reinterpret_cast<float*>(s_in_off + a.max_states + 1);  // [K2_FB][nwave] per-wave layer minima (rounded down)
  int32_t* s_wcnt = reinterpret_cast<int32_t*>(s_wmin + K2_FB * nwave);   // [K2_FB][nwave] per-wave live-state counts
  int32_t* s_flags = s_wcnt + K2_FB * nwave;                              // [8]: 0 tie, 1 has_eps, 2 changed
  int32_t* s_redi = s_flags + 8;                                          // [2*K2_MAXW]
  // 16-byte aligned tail: generic score block [K2_SB][PP], reused (both modes) as the trace-back block
  // (the offset is rounded, not the address: a pointer that went through an integer loses its address space and every access
  //  behind it becomes a flat_ instruction -- the per-layer parking of the certificate's minima was two of those)
  float* s_ac = reinterpret_cast<float*>(smem + (((reinterpret_cast<unsigned char*>(s_redi + 2 * K2_MAXW) - smem) + 15) & ~ptrdiff_t(15)));
  uint8_t* s_bp = reinterpret_cast<uint8_t*>(s_ac);

  if (tid == 0) { a.num_words[u] = 0; a.like[u] = 0.0f; }
  if (start < 0 || S == 0) {  // decoder-wrappers.cc:35-41 empty graph
    if (tid == 0) a.status[u] = KHG_ALIGN_ERROR;
    return;
  }
  if (a.prof && tid == 0) a.prof[u * 8 + 0] = clock64();
  if (tid < 8) s_flags[tid] = 0;
  for (int s = tid; s <= S; s += nthr) s_in_off[s] = (int32_t)(a.in_off[s0 + s] - in0);
  k2_block_sync();
  for (int i = tid; i < A; i += nthr) {
    int col = a.in_col[in0 + i];
    int tidl = a.in_tid[in0 + i];
    float w = a.in_w[in0 + i];
    if (a.trans_cost && tidl >= 1) w = w + a.trans_cost[tidl];  // Times(arc.weight, -scaled_log_prob)
    s_arc[i] = K2Arc{(uint16_t)a.in_src[in0 + i], (int16_t)col, w};
    if (col < 0) s_flags[1] = 1;
  }
  for (int s = tid; s < S; s += nthr) cur[s] = (s == start) ? 0.0 : INFINITY;
  if (LAD && tid < 8) s_red[tid] = INFINITY;          // wave 0's boundary strip: no state before state 0 (s_red is free until the loop ends)
  k2_block_sync();
  const bool has_eps = !FAST && s_flags[1] != 0;
  const float* llu = a.ll + a.ll_off[u];
  uint8_t* bp = a.bp + a.bp_off[u];
  double* lbest = a.layer_best + f0 + u;
  int32_t* lcnt = a.layer_cnt + f0 + u;

  // ---- FAST: the in-arcs of this thread's states live in registers ----
  // An empty slot (a state with fewer than DEG in-arcs, a lane without a state) gets weight +inf and column 0:
  // its candidate cost is +inf (or NaN), never below anything, so the per-layer loop needs no validity tests.
  int e_src[NSD], e_col[NSD];
  double e_w[NSD];
  const bool have_ll = npdf > 0 && T > 0;
  if (FAST) {
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const int sk = tid + nthr * k;
      const int ib = sk < S ? s_in_off[sk] : 0, ie = sk < S ? s_in_off[sk + 1] : 0;
#pragma unroll
      for (int j = 0; j < DEG; ++j) {
        const bool v = ib + j < ie;
        K2Arc ar = s_arc[v ? ib + j : 0];
        e_src[k * DEG + j] = v ? ar.src : 0;
        e_col[k * DEG + j] = v ? ar.col : 0;
        e_w[k * DEG + j] = v ? (double)ar.w : (double)INFINITY;
      }
    }
  } else {
    for (int s = tid; s < S; s += nthr) bp[s] = K2_BP_NONE;
  }
  // LAD: slot 0 becomes the self-loop, slot 1 the arc from state tid - 1 (an empty slot stays weight +inf, column 0); lad_bit[] is
  // the nibble bit each stands for, 1 << its own in-arc slot: the in-arc order and the tie rule are those of the general form
  int lad_bit[2] = {1, 2};
  if constexpr (LAD) {
    if (e_src[0] != tid) {             // slot 0 is the arc from tid - 1 (or both slots are empty)
      const double tw = e_w[0]; e_w[0] = e_w[1]; e_w[1] = tw;
      if (!SC) { const int tc = e_col[0]; e_col[0] = e_col[1]; e_col[1] = tc; }   // SC: one score row per state, slot 0 names it
      lad_bit[0] = 2; lad_bit[1] = 1;
    }
  }
  if (a.prof && tid == 0) a.prof[u * 8 + 1] = clock64();
  int tie = 0;
  // FAST: cur / nxt swap every layer and the layer loop is unrolled by four, so the buffer a layer reads is known
  // at compile time from its sub-index: gather and store addresses are formed once, not per layer
  const double* g_even[NSD]; const double* g_odd[NSD];
  double* st_even[NS]; double* st_odd[NS];       // where a layer of even / odd index WRITES (= the other buffer)
#pragma unroll
  for (int i = 0; i < NSD; ++i) { g_even[i] = cur + (FAST ? e_src[i] : 0); g_odd[i] = nxt + (FAST ? e_src[i] : 0); }
#pragma unroll
  for (int k = 0; k < NS; ++k) { const int sk = min(tid + nthr * k, S > 0 ? S - 1 : 0); st_even[k] = nxt + sk; st_odd[k] = cur + sk; }
  double mine[NS];   // FAST: current cost of this thread's states (mirror of cur[])
  unsigned bpw[NS];  // FAST: this lane's back-pointer nibbles of the current group of eight layers
#pragma unroll
  for (int k = 0; k < NS; ++k) bpw[k] = 0u;
#pragma unroll
  for (int k = 0; k < NS; ++k) mine[k] = (tid + nthr * k == start) ? 0.0 : INFINITY;
  int mine_live[NS];   // FAST: mine[k] != +inf, carried from the layer step that computed it (no second compare for the live count)
#pragma unroll
  for (int k = 0; k < NS; ++k) mine_live[k] = (tid + nthr * k == start) ? 1 : 0;
  // FAST: scores come straight from HBM/L2, 4 frames (one 16-byte load) per in-arc, one block ahead
  // Two named blocks used alternately (the layer loop is unrolled by eight): frames 8m..8m+3 live in sc_a, frames
  // 8m+4..8m+7 in sc_b; with several score rows per lane each is refilled for the block after next while the other is being consumed.
  constexpr int NSC = SC ? (FAST ? KS : 1) : NSD;          // score blocks held: per state (SC) or per in-arc slot
  f32x4 sc_a[NSC], sc_b[NSC];
  // One score row per lane (NSC == 1; round 6): the eight frames of a group -- one 32-byte sector of the row -- are requested in ONE
  // visit, at the group's fifth layer for the NEXT group: its first half into sc_a (free by then), its second half into sc_c, which
  // moves to sc_b when the group is entered.  Two visits per sector four layers apart left the second one to miss again whenever the
  // line had been evicted in between (scores are ~70 % of K2's bytes and the resident utterances' lines exceed an XCD's L2):
  // k2_viterbi_dp 8.22 -> 7.62 ms at the bench shape, L2 fetches - 9 %.  (More score rows per lane keep the two-buffer scheme: 4 more
  // registers per row do not fit their budgets.)
  constexpr bool SC3 = FAST && NSC == 1;
  f32x4 sc_c[NSC];
  if (FAST) {
#pragma unroll
    for (int i = 0; i < NSC; ++i) {
      sc_a[i] = have_ll ? *reinterpret_cast<const f32x4*>(llu + (int64_t)e_col[SC ? i * DEG : i] * tpad) : f32x4{0, 0, 0, 0};
      sc_b[i] = f32x4{0, 0, 0, 0};
      sc_c[i] = (SC3 && have_ll) ? *reinterpret_cast<const f32x4*>(llu + (int64_t)e_col[SC ? i * DEG : i] * tpad + 4) : f32x4{0, 0, 0, 0};   // tpad >= 32
    }
  }

  // FAST: the score requests of one layer step (SUB8 = layer & 7), shared by the general layer step and the ladder's
  auto score_fetch = [&](const int layer, auto subc) {
    constexpr int SUB8 = decltype(subc)::value;
    constexpr int SUB = SUB8 & 3;
    if constexpr (SC3) {
      if constexpr (SUB8 == 0) {
#pragma unroll
        for (int i = 0; i < NSC; ++i) sc_b[i] = sc_c[i];
      }
      if constexpr (SUB8 == 4) {
#pragma unroll
        for (int i = 0; i < NSC; ++i)
          if (have_ll && layer + 4 < tpad) {   // rows are padded to tpad (multiple of 32): the whole next group of eight frames is in bounds
            const float* src = llu + (int64_t)e_col[SC ? i * DEG : i] * tpad + layer + 4;
            sc_a[i] = *reinterpret_cast<const f32x4*>(src);
            sc_c[i] = *reinterpret_cast<const f32x4*>(src + 4);
          }
      }
    } else if (SUB == 0) {               // entering a block: request the NEXT block into the other buffer
#pragma unroll
      for (int i = 0; i < NSC; ++i)
        if (have_ll && layer + 4 < tpad) {   // rows are padded to tpad (multiple of 32)
          const f32x4 v = *reinterpret_cast<const f32x4*>(llu + (int64_t)e_col[SC ? i * DEG : i] * tpad + layer + 4);
          if constexpr ((SUB8 & 4) != 0) sc_a[i] = v; else sc_b[i] = v;
        }
    }
  };
  // One layer.  FAST instantiates it eight times (two 16-byte score blocks; SUB8 = layer & 7 is a compile-time
  // constant there: no dynamic vector indexing, no register shuffles, buffer parity and score block known statically).
  auto layer_step = [&](const int layer, auto subc) -> bool {
    constexpr int SUB8 = decltype(subc)::value;
    constexpr int SUB = SUB8 & 3;
    uint8_t* bpl = bp + (int64_t)layer * Sp;
    // ---- epsilon closure on cur (ProcessNonemitting without pruning), Jacobi sweeps ----
    if (has_eps) {
      for (int it = 0; it <= S + 1; ++it) {
        if (tid == 0) s_flags[2] = 0;
        k2_block_sync();
        for (int s = tid; s < S; s += nthr) {
          double best = cur[s];
          int barg = -1;
          for (int i = s_in_off[s]; i < s_in_off[s + 1]; ++i) {
            K2Arc ar = s_arc[i];
            if (ar.col >= 0) continue;
            double c = cur[ar.src];
            if (c == INFINITY) continue;
            double nw = c + ar.w;
            if (nw < best) { best = nw; barg = i - s_in_off[s]; }
            else if (nw == best && (barg >= 0 ? barg : (int)bpl[s]) != i - s_in_off[s]) tie = 1;
          }
          nxt[s] = best;
          if (barg >= 0) { bpl[s] = (uint8_t)barg; s_flags[2] = 1; }
        }
        k2_block_sync();
        for (int s = tid; s < S; s += nthr) cur[s] = nxt[s];
        const int changed = s_flags[2];
        k2_block_sync();
        if (!changed) break;
      }
    }
    // ---- per-layer minimum and live-state count (beam certificate) ----
    // The minimum is kept as a float rounded DOWN: a lower bound makes the certificate stricter,
    // never wrong.  One value per wave is parked in LDS; every K2_FB layers the block folds them.
    {
      double lm = INFINITY;
      int lc = 0;
      if (FAST) {
#pragma unroll
        for (int k = 0; k < NS; ++k) { lc += mine_live[k]; lm = k == 0 ? mine[0] : (mine[k] < lm ? mine[k] : lm); }   // +inf stays +inf
      } else {
        for (int s = tid; s < S; s += nthr) { double c = cur[s]; if (c != INFINITY) { ++lc; if (c < lm) lm = c; } }
      }
      // float rounding is monotone: min over lanes of (float)cost == (float)(min cost); the one-ulp step DOWN that
      // turns it into a lower bound is applied once per layer when the block folds the wave values (below)
      const int slot = layer & (K2_FB - 1);
      if constexpr (FAST) {
        // Every lane parks its value of this layer in the wave's own LDS strip [8 layers][64 lanes]; once per EIGHT layers the wave
        // folds the strip -- lane (layer slot ly = lane >> 3, sub = lane & 7) reads the eight values of lanes 8 sub .. 8 sub + 7 of
        // slot ly (two 16-byte reads), then three DPP steps over its 8-lane group -- instead of a six-step DPP reduction (plus
        // wait states) and two ballots in EVERY layer: the loop is bound by VALU issue, and this was ~10 of its ~47 instructions.
        float* pm = s_ac + wave * 640;                                    // [8][64] minima (floats) | [8][64] counts (bytes): 2.5 KB per wave
        uint8_t* pc = reinterpret_cast<uint8_t*>(pm + 512);
        pm[(layer & 7) * 64 + lane] = (float)lm;
        pc[(layer & 7) * 64 + lane] = (uint8_t)lc;
        if ((layer & 7) == 7 || layer == T) {
          k2_lds_sync();
          const int ly = lane >> 3, sub = lane & 7;
          const f32x4 m0 = *reinterpret_cast<const f32x4*>(pm + ly * 64 + sub * 8), m1 = *reinterpret_cast<const f32x4*>(pm + ly * 64 + sub * 8 + 4);
          const uint2 cb = *reinterpret_cast<const uint2*>(pc + ly * 64 + sub * 8);      // eight byte counts (<= KS each)
          // (the values are costs converted from double, never a signalling NaN: the bare instruction, without the v_max x, x the
          //  compiler puts in front of every operand of fminf -- eleven of them per fold)
          auto vmin = [](float x, float y) { float r; asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(y)); return r; };
          float m = vmin(vmin(vmin(m0[0], m0[1]), vmin(m0[2], m0[3])), vmin(vmin(m1[0], m1[1]), vmin(m1[2], m1[3])));
          int cn = (int)__builtin_amdgcn_sad_u8(cb.y, 0u, __builtin_amdgcn_sad_u8(cb.x, 0u, 0u));
          // the 8-lane group: xor 1, xor 2 (quad permutes), then the mirror image of the half row
          m = vmin(m, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(m), 0xB1, 0xf, 0xf, false)));
          cn += __builtin_amdgcn_update_dpp(0, cn, 0xB1, 0xf, 0xf, false);
          m = vmin(m, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(m), 0x4E, 0xf, 0xf, false)));
          cn += __builtin_amdgcn_update_dpp(0, cn, 0x4E, 0xf, 0xf, false);
          m = vmin(m, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(m), 0x141, 0xf, 0xf, false)));
          cn += __builtin_amdgcn_update_dpp(0, cn, 0x141, 0xf, 0xf, false);
          if (sub == 0 && ly <= (layer & 7)) {
            const int sl = (layer & ~7 & (K2_FB - 1)) + ly;               // this layer's slot in the 32-layer block
            s_wmin[sl * nwave + wave] = m; s_wcnt[sl * nwave + wave] = cn;
          }
          k2_lds_sync();
        }
      } else {
        const float wm = k2_wave_minf_lane63((float)lm);
        const int wc = k2_wave_sum(lc);
        if (lane == 63) { s_wmin[slot * nwave + wave] = wm; s_wcnt[slot * nwave + wave] = wc; }
      }
      if (slot == K2_FB - 1 || layer == T) {
        k2_block_sync();
        if (tid <= slot) {
          float m = INFINITY; int cn = 0;
          for (int w2 = 0; w2 < nwave; ++w2) { m = fminf(m, s_wmin[tid * nwave + w2]); cn += s_wcnt[tid * nwave + w2]; }
          // m = (float)(exact layer minimum), rounded to nearest: the next float below it is <= the exact minimum
          if (m == INFINITY) { if (cn > 0) m = 3.402823466e38f; }
          else m = __int_as_float(__float_as_int(m) + (m > 0.0f ? -1 : (m < 0.0f ? 1 : (int)0x80000001)));
          lbest[layer - slot + tid] = (double)m;
          lcnt[layer - slot + tid] = cn;
        }
      }
    }
    if (layer == T) return false;
    if (FAST) {
      // ---- emitting arcs: layer -> layer+1, one state per thread, everything in registers ----
      score_fetch(layer, subc);
      double cc[NSD];
#pragma unroll
      for (int i = 0; i < NSD; ++i) cc[i] = (SUB & 1) ? *g_odd[i] : *g_even[i];   // gathers issued back to back
#pragma unroll
      for (int k = 0; k < NS; ++k) {
        // Branch-free: a dead source (+inf) or an empty slot gives +inf or NaN (+inf + -inf when the score cell was
        // not computed: a finite source implies a readable, computed cell), neither is ever < best; a live
        // cell therefore sees exactly the candidates the reference's tokens produce.
        // The minimum first (v_min_f64 ignores a NaN candidate), then WHO attains it: the first arc that does is the one a strict
        // '<' scan keeps, two of them are a tie.  Three mins, three equality compares and a few selects per state instead of
        // a compare + four selects per candidate: the layer loop is bound by VALU issue.
        double nwv[DEG];
#pragma unroll
        for (int j = 0; j < DEG; ++j) {
          const int i = k * DEG + j;
          const int si = SC ? k : i;
          float sc;
          if constexpr ((SUB8 & 4) != 0) sc = sc_b[si][SUB]; else sc = sc_a[si][SUB];
          const float ac = -1 * (a.acoustic_scale * sc);   // decodable-am-diag-gmm.h:96, faster-decoder.cc:208
          nwv[j] = (cc[i] + e_w[i]) + ac;                                  // faster-decoder.h:125
        }
        double best = INFINITY;
#pragma unroll
        for (int j = 0; j < DEG; ++j) best = __builtin_fmin(best, nwv[j]);
        const bool live = __double2hiint(best) != 0x7FF00000;   // best != +inf (never NaN: the minimum started from +inf) as a 32-bit
                                                                // compare; +inf == +inf of a dead cell is neither an arc nor a tie
        // nibble of this cell: DEG == 2 stores WHICH of its two candidates attain the minimum (bit j: arc j does; both = a tie, the
        // first wins; none = dead cell) -- two selects and an or; the general form stores the first attainer's ordinal + a tie bit
        int code;
        if constexpr (DEG == 2) {
          const bool e0 = live && nwv[0] == best, e1 = live && nwv[1] == best;
          code = (e0 ? 1 : 0) | (e1 ? 2 : 0);
        } else {
          int barg = BNONE, neq = 0;
#pragma unroll
          for (int j = DEG - 1; j >= 0; --j) {
            const bool e = nwv[j] == best;
            barg = e ? j : barg;
            neq += e ? 1 : 0;
          }
          barg = live ? barg : BNONE;
          const int ctie = (live && neq > 1) ? 1 : 0;    // ctie: the winning cost is reached by two arcs
          code = barg | (ctie << NB);
        }
        const int sk = tid + nthr * k;
        if (sk < S) *((SUB & 1) ? st_odd[k] : st_even[k]) = best;
        mine[k] = best;
        mine_live[k] = live ? 1 : 0;
        // back-pointer nibble of layer+1, pushed in at the top of this lane's word (eight layers fill it, the
        // oldest ends at the bottom).  Only a tie at a cell ON the best path makes the reference's choice
        // order-dependent; the trace-back reads the tie bits of exactly those cells.
        bpw[k] = (bpw[k] >> 4) | ((unsigned)code << 28);
        const int lb = layer + 1;
        if ((lb & 7) == 7 || lb == T) {
          const unsigned wv = (lb & 7) == 7 ? bpw[k] : bpw[k] >> (4 * (7 - (lb & 7)));   // a partial last group is right-aligned
          reinterpret_cast<unsigned*>(bp)[(int64_t)(lb >> 3) * GW + sk] = wv;
        }
      }
    } else {
      // ---- generic: stage K2_SB frames of acoustic costs, s_ac[tt][col] = -(scale * ll) ----
      if ((layer & (K2_SB - 1)) == 0) {
        k2_block_sync();
        const int tt = tid & (K2_SB - 1), hh = tid / K2_SB, nh = nthr / K2_SB;
        for (int c0 = 0; c0 < npdf; c0 += 8 * nh) {
          float v[8];
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const int col = c0 + nh * k + hh;
            v[k] = col < npdf ? llu[(int64_t)col * tpad + layer + tt] : 0.0f;   // rows padded to tpad: in bounds
          }
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const int col = c0 + nh * k + hh;
            if (col < npdf) s_ac[tt * PP + col] = -1 * (a.acoustic_scale * v[k]);
          }
        }
        k2_block_sync();
      }
      const float* acr = s_ac + (layer & (K2_SB - 1)) * PP;
      uint8_t* bpn = bp + (int64_t)(layer + 1) * Sp;
      for (int s = tid; s < S; s += nthr) {
        double best = INFINITY;
        int barg = K2_BP_NONE;
        const int ib = s_in_off[s], ie = s_in_off[s + 1];
        for (int i = ib; i < ie; ++i) {
          K2Arc ar = s_arc[i];
          if (ar.col < 0) continue;
          double c = cur[ar.src];
          if (c == INFINITY) continue;
          double nw = (c + ar.w) + acr[ar.col];   // faster-decoder.h:125
          if (nw < best) { best = nw; barg = i - ib; }
          else if (nw == best) tie = 1;
        }
        nxt[s] = best;
        bpn[s] = (uint8_t)barg;
      }
    }
    k2_block_sync();
    double* tsw = cur; cur = nxt; nxt = tsw;
    return true;
  };
  if constexpr (LAD) {
    // ---- the ladder: wave w works on group (step - w) of eight layers; one workgroup barrier per step ----
    const int ngrp = (T >> 3) + 1;                                    // layers 0 .. T
    float* const pm = s_ac + wave * 640;                              // this wave's strip of parked minima / counts, as in layer_step
    uint8_t* const pc = reinterpret_cast<uint8_t*>(pm + 512);
    // Boundary strips, [2 group parities][8 layers] doubles each: wave w writes strip w (its lane-63 cost of every layer), wave w + 1
    // reads it one step later.  They lie over cur / nxt, which the ladder does not use before the loop ends (nwave - 1 strips of 128
    // bytes in 16 S bytes: S > 64 (nwave - 1)).  Wave 0 reads the eight +inf of s_red: state 0 has no state below it.
    const double* const bin = wave == 0 ? s_red : cur + (wave - 1) * 16;
    const int bpar = wave == 0 ? 0 : 8;
    double* const bout = cur + wave * 16;
    const bool pub = lane == 63 && wave + 1 < nwave;
    // Certificate: the waves deliver a layer one step apart, so the fold over waves is a running (minimum, count) per layer that
    // wave 0 starts, every later wave joins one step later and the LAST wave finishes and writes out -- the same minimum and the
    // same sum as the block-wide fold of the general form, then the same step down.  Four groups of eight slots (nwave <= 4).
    float* const acc_m = s_wmin;
    int32_t* const acc_c = s_wcnt;
    auto vmin = [](float x, float y) { float r; asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(y)); return r; };
    for (int step = 0; step < ngrp + nwave - 1; ++step) {
      const int g = step - wave;
      if (g >= 0 && g < ngrp) {                                       // wave-uniform
        const int base = 8 * g;
        const double* const bi = bin + (g & 1) * bpar;
        double* const bo = bout + (g & 1) * 8;
        // boundary values: written a step ago, requested two layers ahead of their use -- never on the dependent chain
        double bv[8];
        bv[0] = bi[0]; bv[1] = bi[1];
        auto lad_step = [&](auto subc) -> bool {
          constexpr int SUB8 = decltype(subc)::value;
          constexpr int SUB = SUB8 & 3;
          const int layer = base + SUB8;
          pm[SUB8 * 64 + lane] = (float)mine[0];
          pc[SUB8 * 64 + lane] = (uint8_t)mine_live[0];
          if (pub) bo[SUB8] = mine[0];
          if (layer == T) return false;
          if constexpr (SUB8 + 2 < 8) bv[SUB8 + 2] = bi[SUB8 + 2];
          score_fetch(layer, subc);
          float sc0, sc1;
          if constexpr ((SUB8 & 4) != 0) { sc0 = sc_b[0][SUB]; sc1 = sc_b[SC ? 0 : 1][SUB]; } else { sc0 = sc_a[0][SUB]; sc1 = sc_a[SC ? 0 : 1][SUB]; }
          const float ac0 = -1 * (a.acoustic_scale * sc0);            // decodable-am-diag-gmm.h:96, faster-decoder.cc:208
          const float ac1 = SC ? ac0 : -1 * (a.acoustic_scale * sc1);
          const double prev = k2_dpp_d<0x138, 0xf>(bv[SUB8], mine[0]);   // wave_shr:1 -- lane 0 keeps the boundary value
          const double n_self = (mine[0] + e_w[0]) + ac0;             // faster-decoder.h:125
          const double n_prev = (prev + e_w[1]) + ac1;
          double best = INFINITY;
          best = __builtin_fmin(best, n_self);
          best = __builtin_fmin(best, n_prev);
          const bool live = __double2hiint(best) != 0x7FF00000;
          const bool e_s = live && n_self == best, e_p = live && n_prev == best;
          const int code = (e_s ? lad_bit[0] : 0) | (e_p ? lad_bit[1] : 0);
          mine[0] = best;
          mine_live[0] = live ? 1 : 0;
          bpw[0] = (bpw[0] >> 4) | ((unsigned)code << 28);
          const int lb = layer + 1;
          if ((lb & 7) == 7 || lb == T) {
            const unsigned wv = (lb & 7) == 7 ? bpw[0] : bpw[0] >> (4 * (7 - (lb & 7)));   // a partial last group is right-aligned
            reinterpret_cast<unsigned*>(bp)[(int64_t)(lb >> 3) * GW + tid] = wv;
          }
          return true;
        };
        (void)(lad_step(std::integral_constant<int, 0>{}) && lad_step(std::integral_constant<int, 1>{}) &&
               lad_step(std::integral_constant<int, 2>{}) && lad_step(std::integral_constant<int, 3>{}) &&
               lad_step(std::integral_constant<int, 4>{}) && lad_step(std::integral_constant<int, 5>{}) &&
               lad_step(std::integral_constant<int, 6>{}) && lad_step(std::integral_constant<int, 7>{}));
        // fold this wave's strip (as layer_step does), join the running fold over waves
        const int lastsub = min(7, T - base);
        k2_lds_sync();
        const int ly = lane >> 3, sub = lane & 7;
        const f32x4 m0 = *reinterpret_cast<const f32x4*>(pm + ly * 64 + sub * 8), m1 = *reinterpret_cast<const f32x4*>(pm + ly * 64 + sub * 8 + 4);
        const uint2 cb = *reinterpret_cast<const uint2*>(pc + ly * 64 + sub * 8);
        float m = vmin(vmin(vmin(m0[0], m0[1]), vmin(m0[2], m0[3])), vmin(vmin(m1[0], m1[1]), vmin(m1[2], m1[3])));
        int cn = (int)__builtin_amdgcn_sad_u8(cb.y, 0u, __builtin_amdgcn_sad_u8(cb.x, 0u, 0u));
        m = vmin(m, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(m), 0xB1, 0xf, 0xf, false)));
        cn += __builtin_amdgcn_update_dpp(0, cn, 0xB1, 0xf, 0xf, false);
        m = vmin(m, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(m), 0x4E, 0xf, 0xf, false)));
        cn += __builtin_amdgcn_update_dpp(0, cn, 0x4E, 0xf, 0xf, false);
        m = vmin(m, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(m), 0x141, 0xf, 0xf, false)));
        cn += __builtin_amdgcn_update_dpp(0, cn, 0x141, 0xf, 0xf, false);
        if (sub == 0 && ly <= lastsub) {
          const int sl = (g & 3) * 8 + ly;
          if (wave > 0) { m = vmin(m, acc_m[sl]); cn += acc_c[sl]; }
          if (wave + 1 < nwave) {
            acc_m[sl] = m; acc_c[sl] = cn;
          } else {
            // m = (float)(exact layer minimum), rounded to nearest: the next float below it is <= the exact minimum
            if (m == INFINITY) { if (cn > 0) m = 3.402823466e38f; }
            else m = __int_as_float(__float_as_int(m) + (m > 0.0f ? -1 : (m < 0.0f ? 1 : (int)0x80000001)));
            lbest[base + ly] = (double)m;
            lcnt[base + ly] = cn;
          }
        }
      }
      k2_block_sync();
    }
    if (tid < S) cur[tid] = mine[0];                                  // for the best-final search below
  } else if constexpr (FAST) {
    for (int base = 0; base <= T; base += 8) {
      if (!layer_step(base, std::integral_constant<int, 0>{})) break;
      if (!layer_step(base + 1, std::integral_constant<int, 1>{})) break;
      if (!layer_step(base + 2, std::integral_constant<int, 2>{})) break;
      if (!layer_step(base + 3, std::integral_constant<int, 3>{})) break;
      if (!layer_step(base + 4, std::integral_constant<int, 4>{})) break;
      if (!layer_step(base + 5, std::integral_constant<int, 5>{})) break;
      if (!layer_step(base + 6, std::integral_constant<int, 6>{})) break;
      if (!layer_step(base + 7, std::integral_constant<int, 7>{})) break;
    }
  } else {
    for (int layer = 0; layer <= T; ++layer)
      if (!layer_step(layer, std::integral_constant<int, 0>{})) break;
  }
  // ---- best final state (faster-decoder.cc:373-382): minimum, exact ties flagged ----
  {
    double bc = INFINITY;
    int bs = INT32_MAX;
    for (int s = tid; s < S; s += nthr) {
      double c = cur[s] + a.final_w[s0 + s];
      if (c != INFINITY && c < bc) { bc = c; bs = s; }
    }
    const double g = k2_wave_min(bc);
    int nb = 0;
    if (g != INFINITY) {
      for (int s = tid; s < S; s += nthr) { double c = cur[s] + a.final_w[s0 + s]; if (c == g) { ++nb; if (s < bs || bc != g) { bs = s; bc = g; } } }
    }
    if (bc != g || g == INFINITY) bs = INT32_MAX;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { int t2 = __shfl_xor(bs, o); bs = t2 < bs ? t2 : bs; }
    nb = k2_wave_sum(nb);
    if (tie) s_flags[0] = 1;
    if (lane == 0) { s_red[wave] = g; s_redi[2 * wave] = bs; s_redi[2 * wave + 1] = nb; }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's back-pointer stores are done before wave 0 traces back
  k2_block_sync();
  if (a.prof && tid == 0) a.prof[u * 8 + 2] = clock64();
  if (wave != 0) return;          // trace-back and replay are single-wave work
  int best_state = -1;
  {
    double g = INFINITY;
    for (int w2 = 0; w2 < nwave; ++w2) if (s_red[w2] < g) g = s_red[w2];
    int nb = 0;
    if (g != INFINITY)
      for (int w2 = 0; w2 < nwave; ++w2) if (s_red[w2] == g) { nb += s_redi[2 * w2 + 1]; if (best_state < 0 || s_redi[2 * w2] < best_state) best_state = s_redi[2 * w2]; }
    tie = s_flags[0] != 0 || nb > 1;
  }
  if (best_state < 0) {
    // no final state reachable even without pruning: the reference fails for every beam
    for (int t = lane; t < T; t += 64) a.ali[f0 + t] = 0;
    if (lane == 0) a.status[u] = KHG_ALIGN_ERROR | (a.retry_beam != 0.0f ? KHG_ALIGN_RETRIED : 0);
    return;
  }
  int32_t* path = a.path + a.path_off[u];
  const int path_cap = (int)(a.path_off[u + 1] - a.path_off[u]);
  int n = 0, st = best_state, bad = 0, ptie = 0;   // ptie: a tie at a cell of the best path (fast path)
  k2_global_sync();
  // ---- trace back, fast path, graphs of <= 256 states: eight layers per step of the wave.  The walk itself is a serial chain
  // (the state at layer L-1 is the source of the arc the back-pointer of (L, state) names), but nothing ELSE in it has to be:
  // every lane holds up to four states and, for all eight layers of a back-pointer word at once, looks up where ITS states
  // come from (nibble -> arc -> source state: eight independent LDS reads in flight); the chain is then eight v_readlane hops
  // with the current state in a scalar register.  One lane walking alone stood on three dependent LDS reads and a global store
  // per layer: 344 k of an utterance's 842 k cycles (KHG_OPT_K2_PROF), more than a third of K2. ----
  bool traced = false;
  if constexpr (FAST) {
    if (S <= 256 && T <= path_cap) {
      traced = true;
      const unsigned* W = reinterpret_cast<const unsigned*>(bp);
      const uint32_t* arcw = reinterpret_cast<const uint32_t*>(s_arc);     // K2Arc: src in the low half of its first dword
      auto trace = [&](auto nslot_c) {
        constexpr int NSLOT = decltype(nslot_c)::value;
        int ioff[NSLOT];
        unsigned w[NSLOT], wn[NSLOT];
        int g = T >> 3;
#pragma unroll
        for (int q = 0; q < NSLOT; ++q) {
          const int sq = lane + 64 * q;
          ioff[q] = sq < S ? s_in_off[sq] : 0;
          w[q] = W[(int64_t)g * GW + min(sq, GW - 1)];
          wn[q] = 0u;
        }
        int sst = __builtin_amdgcn_readfirstlane(st);
        // The tail (KHG_OPT_K2_TAIL = 0), in-degree <= 3, one state per thread: the chain needs ONE thing of a cell, the source state
        // of the arc its nibble names.  The <= DEG candidates of a lane's state are loaded once per utterance into registers (already
        // shifted), a cell costs a bit-field extract, a select among them and an OR -- source << NBITS | raw nibble bits in one
        // register, no arc index, no flag packing, no LDS read -- and a hop is one v_readlane whose word is taken apart in scalar code
        // by k2_decode_nibble's rule.  Lane cnt keeps (state << NBITS | ordinal) of its step; the arc indices path[] holds are formed
        // after the eight hops, one LDS read per lane.  path[], n, bad, ptie and st are those of the loop below for every input.
        if constexpr (K2_TAIL_TRACE && DEG <= 3 && KS == 1) {
          if (!a.tail_off) {
            constexpr int NBITS = NB + 1;
            int srcr[NSLOT][DEG], srcx[NSLOT][DEG];
#pragma unroll
            for (int q = 0; q < NSLOT; ++q) {
              const int sq = lane + 64 * q;
              const int ib = sq < S ? s_in_off[sq] : 0, ie = sq < S ? s_in_off[sq + 1] : 0;
#pragma unroll
              for (int j = 0; j < DEG; ++j) srcr[q][j] = ib + j < ie ? (int)((arcw[2 * (ib + j)] & 0xffffu) << NBITS) : 0;
#pragma unroll
              for (int j = 0; j + 1 < DEG; ++j) srcx[q][j] = srcr[q][j] ^ srcr[q][DEG - 1];      // candidate j against the last one
            }
            for (; g >= 0 && !bad; --g) {
              if (g > 0) {
#pragma unroll
                for (int q = 0; q < NSLOT; ++q) wn[q] = W[(int64_t)(g - 1) * GW + min(lane + 64 * q, GW - 1)];  // next word: in flight under this one
              }
              int pk[8][NSLOT];
#pragma unroll
              for (int k = 0; k < 8; ++k)
#pragma unroll
                for (int q = 0; q < NSLOT; ++q) {
                  // (masks, not selects between array elements: those become indexed loads from a stack copy of srcr)
                  const int nib = (int)((w[q] >> (4 * k)) & (unsigned)((1 << NBITS) - 1));
                  int sel = srcr[q][0];
                  if constexpr (DEG == 2) sel = srcr[q][1] ^ (srcx[q][0] & -(nib & 1));
                  if constexpr (DEG == 3) { const int o = nib & BNONE; sel = srcr[q][2] ^ (srcx[q][0] & -(int)(o == 0)) ^ (srcx[q][1] & -(int)(o == 1)); }
                  pk[k][q] = sel | nib;
                }
              int pv = 0, cnt = 0;
#pragma unroll
              for (int k = 7; k >= 0; --k) {
                const int L = 8 * g + k;
                if (L <= T && L >= 1 && !bad) {
                  const int q = sst >> 6, l = sst & 63;
                  int pw = __builtin_amdgcn_readlane(pk[k][0], l);
#pragma unroll
                  for (int qq = 1; qq < NSLOT; ++qq)
                    if (q == qq) pw = __builtin_amdgcn_readlane(pk[k][qq], l);
                  int ord, tieb;
                  k2_decode_nibble<DEG, NB>(pw & ((1 << NBITS) - 1), ord, tieb);
                  if (ord == BNONE) {
                    bad = 1;                                 // a dead cell on the walk (cannot happen from a reachable final state)
                  } else {
                    ptie |= tieb;
                    pv = lane == cnt ? ((sst << NBITS) | ord) : pv;    // lane cnt keeps (state, ordinal) of this step
                    ++cnt;
                    sst = pw >> NBITS;
                  }
                }
              }
              if (lane < cnt) path[n + lane] = s_in_off[pv >> NBITS] + (pv & BNONE);     // coalesced, path order
              n += cnt;
#pragma unroll
              for (int q = 0; q < NSLOT; ++q) w[q] = wn[q];
            }
            st = sst;
            return;
          }
        }
        for (; g >= 0 && !bad; --g) {
          if (g > 0) {
#pragma unroll
            for (int q = 0; q < NSLOT; ++q) wn[q] = W[(int64_t)(g - 1) * GW + min(lane + 64 * q, GW - 1)];      // next word: in flight under this one
          }
          int aiv[8][NSLOT], srcv[8][NSLOT];
#pragma unroll
          for (int k = 0; k < 8; ++k)
#pragma unroll
            for (int q = 0; q < NSLOT; ++q) {
              const int nib = (int)((w[q] >> (4 * k)) & 15u);
              int ord, tieb;
              k2_decode_nibble<DEG, NB>(nib, ord, tieb);
              const int none = ord == BNONE;
              const int ai = ioff[q] + (none ? 0 : ord);
              aiv[k][q] = ai | (none << 30) | (tieb << 29);
              srcv[k][q] = (int)(arcw[2 * ai] & 0xffffu);
            }
          int pv = 0, cnt = 0;
#pragma unroll
          for (int k = 7; k >= 0; --k) {
            const int L = 8 * g + k;
            if (L <= T && L >= 1 && !bad) {
              const int q = sst >> 6, l = sst & 63;
              int av = __builtin_amdgcn_readlane(aiv[k][0], l), sv = __builtin_amdgcn_readlane(srcv[k][0], l);
#pragma unroll
              for (int qq = 1; qq < NSLOT; ++qq)
                if (q == qq) { av = __builtin_amdgcn_readlane(aiv[k][qq], l); sv = __builtin_amdgcn_readlane(srcv[k][qq], l); }
              if (av & (1 << 30)) {
                bad = 1;                                   // a dead cell on the walk (cannot happen from a reachable final state)
              } else {
                ptie |= (av >> 29) & 1;
                pv = lane == cnt ? (av & 0xffffff) : pv;      // lane cnt keeps the arc of this step (coalesced store below)
                ++cnt;
                sst = sv;
              }
            }
          }
          if (lane < cnt) path[n + lane] = pv;
          n += cnt;
#pragma unroll
          for (int q = 0; q < NSLOT; ++q) w[q] = wn[q];
        }
        st = sst;
      };
      if (S <= 64) trace(std::integral_constant<int, 1>{});
      else if (S <= 128) trace(std::integral_constant<int, 2>{});
      else trace(std::integral_constant<int, 4>{});
    }
  }
  // ---- trace back, general: one 32-layer block of back-pointers at a time through LDS, one lane walking ----
  for (int hi = traced ? -1 : T; hi >= 0 && !bad; ) {
    const int lo = hi > K2_FB ? hi - K2_FB : 0;          // layers lo..hi (hi-lo <= 32)
    const int glo = lo >> 3;                               // fast: first group of eight layers in this block
    if (FAST) {
      const int nw32 = ((hi >> 3) - glo + 1) * GW;         // <= 5 groups
      const unsigned* src = reinterpret_cast<const unsigned*>(bp) + (int64_t)glo * GW;
      unsigned* dst = reinterpret_cast<unsigned*>(s_bp);
      for (int i0 = 0; i0 < nw32; i0 += 256) {
        unsigned v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { const int i = i0 + 64 * k + lane; if (i < nw32) v[k] = src[i]; }
#pragma unroll
        for (int k = 0; k < 4; ++k) { const int i = i0 + 64 * k + lane; if (i < nw32) dst[i] = v[k]; }
      }
    } else {
      const int nv = (hi - lo + 1) * (LB >> 4);            // 16-byte vectors in this block
      const uint4* src = reinterpret_cast<const uint4*>(bp + (int64_t)lo * LB);
      uint4* dst = reinterpret_cast<uint4*>(s_bp);
      for (int i0 = 0; i0 < nv; i0 += 256) {
        uint4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { const int i = i0 + 64 * k + lane; if (i < nv) v[k] = src[i]; }
#pragma unroll
        for (int k = 0; k < 4; ++k) { const int i = i0 + 64 * k + lane; if (i < nv) dst[i] = v[k]; }
      }
    }
    k2_lds_sync();
    if (lane == 0) {
      int layer = hi;
      // consume layers hi .. lo+1 completely (an emitting arc leaves the layer); at `lo` only
      // epsilon hops, unless lo == 0 where the walk ends at the start state
      while (true) {
        int ord;
        if (FAST) {
          if (layer == 0) ord = K2_BP_NONE;
          else {
            const unsigned wv = reinterpret_cast<const unsigned*>(s_bp)[((layer >> 3) - glo) * GW + st];   // state st = lane tid + nthr*k: word index st
            const int nib = (int)((wv >> (4 * (layer & 7))) & 15u);
            int tieb;
            k2_decode_nibble<DEG, NB>(nib, ord, tieb);
            ptie |= tieb;
            if (ord == BNONE) ord = K2_BP_NONE;
          }
        } else {
          ord = s_bp[(layer - lo) * Sp + st];
        }
        if (ord == K2_BP_NONE) { if (layer != 0) bad = 1; layer = -1; break; }
        int ai = s_in_off[st] + ord;
        if (s_arc[ai].col >= 0 && layer == lo && lo != 0) break;   // continue in the next block
        if (n >= path_cap) { bad = 1; layer = -1; break; }
        path[n++] = ai;
        st = s_arc[ai].src;
        if (s_arc[ai].col >= 0) --layer;
      }
      hi = layer < 0 ? -1 : lo;
    }
    hi = __shfl(hi, 0); st = __shfl(st, 0); n = __shfl(n, 0); bad = __shfl(bad, 0); ptie = __shfl(ptie, 0);
    k2_lds_sync();
  }
  if (a.prof && tid == 0) a.prof[u * 8 + 3] = clock64();
  // ---- replay forward in the token arithmetic; 64 path entries per step ----
  double cost = 0.0;
  float v1 = 0.0f, v2 = 0.0f;
  int t = 0, nw = 0;
  bool ok = !bad;
  const double beam = (double)a.beam;
  const int64_t wcap = a.words_off[u + 1] - a.words_off[u];
  int32_t* words = a.words + a.words_off[u];
  k2_global_sync();   // path[] written by lane 0 is read by every lane below
  int nscan = 0, nserial = 0;     // replay batches whose cost chain ran as a wave scan / as the serial loop (KHG_OPT_K2_PROF)
  bool replayed = false;
  // ---- the tail's replay (KHG_OPT_K2_TAIL = 0), register-resident forms: no epsilon arcs, every entry emits (no col >= 0 tests), and
  // the fp64 cost chain ((cost + w) + ac per entry, 64 dependent iterations a batch) runs as a six-step wave scan of
  // d = (double)w + (double)ac seeded with the incoming cost in lane 0 -- WHERE THAT IS EXACT:
  //   let the addends of the utterance so far be the floats w_i, ac_i, e_min the smallest binary exponent among the non-zero ones
  //   (all normal, >= 2^-100, finite) and q = 2^(e_min - 23).  (1) Every addend is an integer multiple of q: a normal float of
  //   exponent e >= e_min is a multiple of 2^(e - 23).  (2) If sum |addend| <= 2^52 q, every sum of a subset of the addends, in any
  //   order and association, is an integer multiple of q of magnitude < 2^53 q: a binary64 number.  (3) So no addition of the
  //   reference's chain rounds, nor any of the scan's: both give the exact sums -- the same bits; a zero sum is +0 in both, since the
  //   chain starts from +0 and every scanned value includes lane 0's.
  // The running sum |addend| is itself rounded (relative error <= 2^-53 per add, a few thousand adds): the bound is 2^52 q, not
  // 2^53 q, a margin no such error reaches.  The first batch that fails the rule (NaN fails the comparison) and every later one of
  // the utterance take the serial loop: once an addition has rounded, the incoming cost is off the grid.  The float sums of the
  // LatticeWeight round at every step: they stay a serial chain, both in one packed add. ----
  if constexpr (FAST && K2_TAIL_REPLAY) {
    if (!bad && !a.tail_off) {
      replayed = true;
      ok = (0.0 < lbest[0] + beam) || lcnt[0] <= a.min_active;
      unsigned emin1 = 0xffffffffu;      // (bits of the smallest non-zero |addend| so far) - 1; all ones: none yet
      double sumabs = 0.0;               // running sum |addend|
      bool serial = false;
      f32x2 vv = {0.0f, 0.0f};
      for (int base = n - 1; base >= 0; base -= 64) {
        const int idx = base - lane;                     // lane k handles path[base-k] (forward order)
        const bool mine = idx >= 0;
        int ai = 0, col = 0, tidl = 0, ol = 0; float w = 0.0f, ac = 0.0f;
        if (mine) {
          ai = path[idx];
          K2Arc ar = s_arc[ai];
          col = ar.col; w = ar.w;
          tidl = a.in_tid[in0 + ai];
          ol = a.in_olabel[in0 + ai];
        }
        const int tf = t + lane;                         // every entry emits: entry k of the batch is frame t + k
        if (mine) {
          ac = -1 * (a.acoustic_scale * llu[(int64_t)col * tpad + tf]);
          a.ali[f0 + tf] = tidl;
        }
        const int cnt = base >= 63 ? 64 : base + 1;
        const int tl = tf + (mine ? 1 : 0);              // certificate operands of this entry's END node (layer tl)
        double lb = 0.0; int small = 0;
        if (mine) {
          lb = lbest[tl] + beam;
          small = lcnt[tl] <= a.min_active && (tl == 0 || lcnt[tl - 1] <= a.min_active);
        }
        const double cost_in = cost;
        double ca = 0.0;
        if (!serial) {
          const unsigned aw = __float_as_uint(w) & 0x7fffffffu, aa = __float_as_uint(ac) & 0x7fffffffu;
          const unsigned m1 = k2_wave_minu(min(aw - 1u, aa - 1u));          // zero -> all ones: not an addend
          emin1 = min(emin1, m1);
          sumabs += k2_wave_sumd((double)__uint_as_float(aw) + (double)__uint_as_float(aa));
          const unsigned eb = (emin1 + 1u) >> 23;                           // biased exponent of the smallest non-zero |addend|; 0: none
          const double bound = __hiloint2double((int)((eb + 925u) << 20), 0);   // 2^52 q = 2^(eb - 127 + 29)
          serial = !((emin1 == 0xffffffffu || eb >= 27u) && sumabs <= bound);
        }
        if (!serial) {
          ++nscan;
          double d = (double)w + (double)ac;
          d = lane == 0 ? cost_in + d : d;
          ca = k2_wave_scand(d);
          cost = k2_readlane_d(ca, cnt - 1);
        } else {
          ++nserial;
          for (int k = 0; k < cnt; ++k) {
            const float wk = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w), k));
            const float ack = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ac), k));
            const double ncost = (cost + wk) + ack;                          // faster-decoder.h:125
            ca = lane == k ? ncost : ca;
            cost = ncost;
          }
        }
        const double cb = k2_dpp_d<0x138, 0xf>(cost_in, ca);                 // wave_shr:1 -- the cost BEFORE this lane's entry
        const float tot_cost = (float)(ca - cb);                               // faster-decoder.cc:393
        const float ac_cost = tot_cost - w;
        if (__ballot(mine && !(ca < lb) && !small) != 0ull) ok = false;        // beam certificate of every entry's end node
        t += cnt;
        {
          const unsigned long long wm = __ballot(mine && ol != 0);             // word labels, path order
          if (mine && ol != 0) { const int pos = nw + __popcll(wm & ((1ull << lane) - 1ull)); if (pos < wcap) words[pos] = ol; }
          nw += __popcll(wm);
        }
        for (int k = 0; k < cnt; ++k) {                                        // LatticeWeight Times, path order
          const f32x2 r = {__int_as_float(__builtin_amdgcn_readlane(__float_as_int(w), k)), __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ac_cost), k))};
          vv = r + vv;
        }
      }
      v1 = vv[0]; v2 = vv[1];
    }
  }
  if (!bad && !replayed) {
    ok = (0.0 < lbest[0] + beam) || lcnt[0] <= a.min_active;
    for (int base = n - 1; base >= 0; base -= 64) {
      ++nserial;
      const int idx = base - lane;                     // lane k handles path[base-k] (forward order)
      int ai = 0, col = -1, tidl = 0, ol = 0; float w = 0.0f, ac = 0.0f;
      if (idx >= 0) {
        ai = path[idx];
        K2Arc ar = s_arc[ai];
        col = ar.col; w = ar.w;
        tidl = a.in_tid[in0 + ai];
        ol = a.in_olabel[in0 + ai];
      }
      // frame index of each entry = t + (number of emitting entries before it in this batch)
      const unsigned long long em = __ballot(idx >= 0 && col >= 0);
      const int before = __popcll(em & ((1ull << lane) - 1ull));
      const int tf = t + before;
      if (idx >= 0 && col >= 0) {
        ac = -1 * (a.acoustic_scale * llu[(int64_t)col * tpad + tf]);
        a.ali[f0 + tf] = tidl;
      }
      const int cnt = base >= 63 ? 64 : base + 1;
      // certificate operands of this entry's END node (layer tl), fetched by all lanes in parallel
      const int tl = tf + (idx >= 0 && col >= 0 ? 1 : 0);
      double lb = 0.0; int small = 0;
      if (idx >= 0) {
        lb = lbest[tl] + beam;
        small = lcnt[tl] <= a.min_active && (tl == 0 || lcnt[tl - 1] <= a.min_active);
      }
      // Only the token cost itself is a serial chain (fp64, one rounding per add: faster-decoder.h:125 / :135); it runs redundantly
      // and identically on every lane (uniform control flow, operands by v_readlane) and lane k keeps the cost AFTER its own
      // entry.  Everything derived from it -- the float cost pieces of GetBestPath, the beam certificate of the entry's end
      // node, the word labels -- is then per-lane work; the two float sums of the LatticeWeight are a second, shorter chain.
      // (One loop doing all of it per entry was ~24 vector instructions per path entry on a kernel bound by their issue.)
      const double cost_in = cost;
      double ca = 0.0;
      for (int k = 0; k < cnt; ++k) {
        const float wk = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w), k));
        const float ack = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ac), k));
        const int colk = __builtin_amdgcn_readlane(col, k);
        const double ncost = colk >= 0 ? (cost + wk) + ack : cost + wk;      // faster-decoder.h:125 / :135
        ca = lane == k ? ncost : ca;
        cost = ncost;
      }
      double cb = __shfl_up(ca, 1);                                          // the cost BEFORE this lane's entry
      if (lane == 0) cb = cost_in;
      const bool mine = idx >= 0;
      const float tot_cost = (float)(ca - cb);                               // faster-decoder.cc:393
      const float ac_cost = tot_cost - w;
      if (__ballot(mine && !(ca < lb) && !small) != 0ull) ok = false;        // beam certificate of every entry's end node
      t += __popcll(em);
      {
        const unsigned long long wm = __ballot(mine && ol != 0);             // word labels, path order
        if (mine && ol != 0) { const int pos = nw + __popcll(wm & ((1ull << lane) - 1ull)); if (pos < wcap) words[pos] = ol; }
        nw += __popcll(wm);
      }
      for (int k = 0; k < cnt; ++k) {                                        // LatticeWeight Times, path order
        v1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w), k)) + v1;
        v2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ac_cost), k)) + v2;
      }
    }
  }
  if (a.prof && tid == 0) { a.prof[u * 8 + 4] = clock64(); a.prof[u * 8 + 5] = T; a.prof[u * 8 + 6] = S; a.prof[u * 8 + 7] = (long long)FAST | ((long long)nscan << 8) | ((long long)nserial << 32); }   // word 7: FAST | replay batches scanned << 8 | serial << 32
  int stt = 0;
  if (lane == 0) {
    if (bad || nw > wcap) {
      stt = K2_ST_NEED_FALLBACK;
    } else {
      v1 = a.final_w[s0 + best_state] + v1;            // faster-decoder.cc:415-417
      v2 = 0.0f + v2;
      a.num_words[u] = nw;
      a.like[u] = -(v1 + v2) / a.like_scale;       // decoder-wrappers.cc:95
      stt = (ok && !tie && !ptie && a.max_active == INT32_MAX) ? (KHG_ALIGN_DONE | KHG_ALIGN_EXACT_DP) : K2_ST_NEED_FALLBACK;
    }
    a.status[u] = stt;
  }
  if (a.unc) {     // split mode: K3 starts on `ali` while the order-faithful decoders work -- it must not see this utterance there
    stt = __builtin_amdgcn_readfirstlane(stt);
    if (stt == K2_ST_NEED_FALLBACK) {
      k2_global_sync();      // the replay's stores to this range are complete before other lanes overwrite them
      for (int t2 = lane; t2 < T; t2 += 64) a.ali[f0 + t2] = 0;
      if (lane == 0) {
        a.unc[u] = 1;
        atomicAdd(&a.unc_cnt[0], 1);
        atomicAdd(&a.unc_cnt[1], T);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------
// Order-faithful FasterDecoder for the utterances k2_viterbi_dp could not certify.
// One thread per utterance does the token passing exactly in the reference's order.
//
// HashList (hash-list-inl.h:129-174) keeps ONE Elem per live state; its list order is "buckets
// in order of first occupation, insertion order inside a bucket".  Tokens form chains through
// prev_; because a layer is complete before it is expanded, the surviving chain is recovered
// from one back-pointer per (layer, state), exactly like the DP, and the token costs along it
// are re-derived by k2_finish in the same arithmetic.
struct K2Elem { double cost; int32_t key; int32_t tail; };  // tail: index of next elem, -1 = null

template <bool GMEM>
__global__ void k2_viterbi_faithful(K2Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char k2_lds[];
  unsigned char* const smem = GMEM ? a.gscratch + (size_t)blockIdx.x * a.gscratch_stride : k2_lds;
  const int u = blockIdx.x;
  if (a.status[u] != K2_ST_NEED_FALLBACK) return;
  if (threadIdx.x != 0) return;
  const int64_t f0 = a.frame_off[u];
  const int T = (int)(a.frame_off[u + 1] - f0);
  const int tpad = (T + 31) & ~31;
  const int64_t s0 = a.state_off[a.gidx[u]];
  const int S = (int)(a.state_off[a.gidx[u] + 1] - s0);
  const int64_t in0 = a.in_off[s0];
  const int A = (int)(a.in_off[s0 + S] - in0);
  const int start = a.start[a.gidx[u]];
  const float* llu = a.ll + a.ll_off[u];
  uint8_t* bp = a.bp + a.bp_off[u];

  // LDS: two elem pools (current / previous layer), bucket table, work queue, graph tables
  // (its byte count: k2_lds_lane, khg_k2.hip)
  const int HB = a.max_states * 2 > 1000 ? a.max_states * 2 : 1000;   // upper bound of hash_size
  K2Elem* pool0 = reinterpret_cast<K2Elem*>(smem);
  K2Elem* pool1 = pool0 + a.max_states;
  int32_t* b_last = reinterpret_cast<int32_t*>(pool1 + a.max_states);  // [HB] last elem of bucket, -1 empty
  int32_t* b_prev = b_last + HB;                                       // [HB] previous bucket in occupation order
  const int QCAP = a.max_states + a.max_inarcs;
  int32_t* queue = b_prev + HB;                                        // [QCAP] (elem indices)
  float* tmp = reinterpret_cast<float*>(queue + QCAP);                 // [max_states] GetCutoff tmp_array_
  int32_t* s_in_off = reinterpret_cast<int32_t*>(tmp + a.max_states);  // [max_states+1]
  int32_t* s_src = s_in_off + a.max_states + 1;
  int32_t* s_col = s_src + a.max_inarcs;
  int32_t* s_dst = s_col + a.max_inarcs;                               // destination state of the in-arc
  float* s_w = reinterpret_cast<float*>(s_dst + a.max_inarcs);
  uint8_t* s_ord = reinterpret_cast<uint8_t*>(s_w + a.max_inarcs);     // in-arc ordinal within its destination

  for (int s = 0; s <= S; ++s) s_in_off[s] = (int32_t)(a.in_off[s0 + s] - in0);
  for (int s = 0; s < S; ++s)
    for (int i = s_in_off[s]; i < s_in_off[s + 1]; ++i) {
      int tidl = a.in_tid[in0 + i];
      float w = a.in_w[in0 + i];
      if (a.trans_cost && tidl >= 1) w = w + a.trans_cost[tidl];
      s_src[i] = a.in_src[in0 + i];
      s_col[i] = a.in_col[in0 + i];
      s_w[i] = w;
      s_dst[i] = s;
      s_ord[i] = (uint8_t)(i - s_in_off[s]);
    }
  auto dest_of = [&](int ai) { return s_dst[ai]; };
  const int64_t o0 = a.out_off[s0];
  (void)A;

  K2HashList<K2Elem> hl{pool0, 0, 1000, b_last, b_prev, -1, -1};   // faster-decoder.cc:30 toks_.SetSize(1000)
  hl.init(HB);
  size_t& hash_size = hl.hash_size;
  int& list_head = hl.list_head;
  K2Elem*& pool = hl.pool;  // pool of the layer being built
  int& pool_n = hl.pool_n;

  // HashList::Insert (hash-list-inl.h:129-174); returns elem index; *is_new tells which case
  auto hl_insert = [&](int key, double cost, bool* is_new) -> int {
    const int e = hl.insert(key, is_new);
    if (*is_new) pool[e].cost = cost;
    return e;
  };
  auto hl_clear = [&]() -> int { return hl.clear(); };
  // ProcessNonemitting (faster-decoder.cc:58-118) on the layer being built
  auto process_nonemitting = [&](double cutoff, uint8_t* bpl) {
    int qn = 0;
    for (int e = list_head; e >= 0; e = pool[e].tail) queue[qn++] = e;
    while (qn) {
      int e = queue[--qn];
      int state = pool[e].key;
      double tcost = pool[e].cost;
      if (tcost > cutoff) continue;
      for (int64_t oa = a.out_off[s0 + state]; oa < a.out_off[s0 + state + 1]; ++oa) {
        int ai = a.out_inidx[oa];
        if (s_col[ai] >= 0) continue;           // ilabel != 0
        double ncost = tcost + s_w[ai];         // Token(arc, prev) :135
        if (ncost > cutoff) continue;           // :89-92
        int ns = dest_of(ai);
        bool is_new;
        int ef = hl_insert(ns, ncost, &is_new);
        if (is_new) { bpl[ns] = s_ord[ai]; if (qn < QCAP) queue[qn++] = ef; else atomicOr(a.err_flag, 2); continue; }
        if (pool[ef].cost > ncost) {            // :104
          pool[ef].cost = ncost; bpl[ns] = s_ord[ai];
          if (qn < QCAP) queue[qn++] = ef; else atomicOr(a.err_flag, 2);
        }
      }
    }
  };

  int status = KHG_ALIGN_ERROR;
  int best_state = -1;
  float beam = a.beam;
  for (int attempt = 0; attempt < 2; ++attempt) {
    // ---- InitDecoding (faster-decoder.cc:41-56) ----
    hl_clear();
    pool = pool0; pool_n = 0;
    for (int s = 0; s < S; ++s) bp[s] = K2_BP_NONE;
    { bool nw; hl_insert(start, 0.0, &nw); }
    process_nonemitting((double)3.402823466e+38f, bp);
    // ---- AdvanceDecoding ----
    for (int frame = 0; frame < T; ++frame) {
      K2Elem* last = pool;            // layer `frame`
      int last_head = hl_clear();
      pool = (last == pool0) ? pool1 : pool0;
      pool_n = 0;
      uint8_t* bpn = bp + (int64_t)(frame + 1) * ((S + 15) & ~15);
      for (int s = 0; s < S; ++s) bpn[s] = K2_BP_NONE;
      // GetCutoff (faster-decoder.cc:243-335)
      double best_cost = INFINITY;
      int best_elem = -1;
      size_t count = 0;
      double weight_cutoff;
      float adaptive_beam;
      if (a.max_active == INT32_MAX && a.min_active == 0) {
        for (int e = last_head; e >= 0; e = last[e].tail, ++count)
          if (last[e].cost < best_cost) { best_cost = last[e].cost; best_elem = e; }
        adaptive_beam = beam;
        weight_cutoff = best_cost + beam;
      } else {
        for (int e = last_head; e >= 0; e = last[e].tail, ++count) {
          double w = last[e].cost;
          tmp[count] = (float)w;
          if (w < best_cost) { best_cost = w; best_elem = e; }
        }
        double beam_cutoff = best_cost + beam;
        double min_active_cutoff = INFINITY, max_active_cutoff = INFINITY;
        size_t limit = count;
        // nth_element value == k-th order statistic: selection sort of the first k+1 minima
        auto kth = [&](size_t n, size_t k) -> float {
          for (size_t i = 0; i <= k; ++i) {
            size_t mi = i;
            for (size_t jj = i + 1; jj < n; ++jj) if (tmp[jj] < tmp[mi]) mi = jj;
            float tv = tmp[i]; tmp[i] = tmp[mi]; tmp[mi] = tv;
          }
          return tmp[k];
        };
        if (count > (size_t)a.max_active) { max_active_cutoff = kth(count, (size_t)a.max_active); limit = (size_t)a.max_active; }
        if (max_active_cutoff < beam_cutoff) {
          adaptive_beam = max_active_cutoff - best_cost + a.beam_delta;
          weight_cutoff = max_active_cutoff;
        } else {
          if (count > (size_t)a.min_active) {
            if (a.min_active == 0) min_active_cutoff = best_cost;
            else min_active_cutoff = kth(limit, (size_t)a.min_active);
          }
          if (min_active_cutoff > beam_cutoff) {
            adaptive_beam = min_active_cutoff - best_cost + a.beam_delta;
            weight_cutoff = min_active_cutoff;
          } else {
            adaptive_beam = beam;
            weight_cutoff = beam_cutoff;
          }
        }
      }
      // PossiblyResizeHash (:337-344)
      size_t new_sz = (size_t)((float)count * a.hash_ratio);
      if (new_sz > hash_size) hash_size = new_sz;
      double next_weight_cutoff = INFINITY;
      if (best_elem >= 0) {  // :175-188
        int state = last[best_elem].key;
        double tcost = last[best_elem].cost;
        for (int64_t oa = a.out_off[s0 + state]; oa < a.out_off[s0 + state + 1]; ++oa) {
          int ai = a.out_inidx[oa];
          int col = s_col[ai];
          if (col < 0) continue;
          float ac_cost = -1 * (a.acoustic_scale * llu[(int64_t)col * tpad + frame]);
          double new_weight = s_w[ai] + tcost + ac_cost;
          if (new_weight + adaptive_beam < next_weight_cutoff) next_weight_cutoff = new_weight + adaptive_beam;
        }
      }
      for (int e = last_head; e >= 0; e = last[e].tail) {  // :195-236
        int state = last[e].key;
        double tcost = last[e].cost;
        if (tcost < weight_cutoff) {
          for (int64_t oa = a.out_off[s0 + state]; oa < a.out_off[s0 + state + 1]; ++oa) {
            int ai = a.out_inidx[oa];
            int col = s_col[ai];
            if (col < 0) continue;
            float ac_cost = -1 * (a.acoustic_scale * llu[(int64_t)col * tpad + frame]);
            double new_weight = s_w[ai] + tcost + ac_cost;
            if (new_weight < next_weight_cutoff) {
              double tok_cost = (tcost + s_w[ai]) + ac_cost;   // Token ctor :125
              int ns = dest_of(ai);
              bool is_new;
              int ef = hl_insert(ns, tok_cost, &is_new);
              if (new_weight + adaptive_beam < next_weight_cutoff) next_weight_cutoff = new_weight + adaptive_beam;
              if (is_new) bpn[ns] = s_ord[ai];
              else if (pool[ef].cost > tok_cost) { pool[ef].cost = tok_cost; bpn[ns] = s_ord[ai]; }
            }
          }
        }
      }
      process_nonemitting(next_weight_cutoff, bpn);
    }
    // ---- ReachedFinal (:346-353) + best final token (:373-382) ----
    double bc = INFINITY;
    best_state = -1;
    bool reached = false;
    for (int e = list_head; e >= 0; e = pool[e].tail) {
      float fw = a.final_w[s0 + pool[e].key];
      if (pool[e].cost != INFINITY && fw != INFINITY) reached = true;
      double c = pool[e].cost + fw;
      if (c < bc && c != INFINITY) { bc = c; best_state = pool[e].key; }
    }
    if (reached) { status = (attempt ? KHG_ALIGN_RETRIED : 0); break; }
    if (attempt == 0 && a.retry_beam != 0.0f) { beam = a.retry_beam; continue; }  // decoder-wrappers.cc:55-67
    status = KHG_ALIGN_ERROR | (attempt ? KHG_ALIGN_RETRIED : 0);
    best_state = -1;
    break;
  }
  (void)o0;
  if (best_state < 0) {
    for (int t = 0; t < T; ++t) a.ali_fb[f0 + t] = 0;
    a.num_words[u] = 0; a.like[u] = 0.0f;
    a.status[u] = status | KHG_ALIGN_ERROR | KHG_ALIGN_FALLBACK;
    return;
  }
  int st = k2_finish(a, u, best_state, s_in_off, s_src, s_col, s_w, false, nullptr);
  if (st != KHG_ALIGN_DONE) {
    for (int t = 0; t < T; ++t) a.ali_fb[f0 + t] = 0;
    a.status[u] = KHG_ALIGN_ERROR | status | KHG_ALIGN_FALLBACK;
  } else {
    a.status[u] = status | KHG_ALIGN_FALLBACK;
  }
}

// ---------------------------------------------------------------------------------------
// Order-faithful FasterDecoder, WAVE-PARALLEL form (graphs of <= 1000 states, any out-degree, with or without
// epsilon-input arcs).  Same results as k2_viterbi_faithful, token for token; one wave per utterance.
//
// What makes the reference order dependent, and how each piece becomes a data-parallel primitive:
//  * ProcessEmitting walks the token list in HashList order and, per arc, prunes against
//    next_weight_cutoff, which it lowers as it goes (faster-decoder.cc:195-236).  The cutoff an arc is
//    tested against is min(initial, min over EARLIER arcs of new_weight + adaptive_beam) -- the update
//    only ever fires for arcs that also pass the test, so it is an exclusive prefix-min over the
//    flattened (token, arc) sequence: one wave scan per 64 arcs with a carried minimum.
//  * HashList::Insert keeps one Elem per state; a later token replaces it only if strictly cheaper
//    (:104/:226), so the survivor of a state is the FIRST arc that attains the minimum token cost: an LDS
//    atomicMin on the order-preserving key of the double cost, then an atomicMin of the arc index among
//    the arcs that attain it.
//  * The next list order is "buckets in order of first occupation, insertion order inside a bucket"
//    (hash-list-inl.h:129-174).  hash_size starts at 1000 and never shrinks, so with <= 1000 states every
//    state has its own bucket and the order is simply the order of FIRST insertion: compaction of the
//    per-arc "first survivor of its state" flags by a prefix count.
//  * GetCutoff's nth_element values (:243-335) are order statistics of the float costs: found by counting,
//    for every element, how many are smaller / not larger.
//  * The flattened (token, arc) sequence is exact, whatever the out-degrees: an exclusive prefix sum of the out-degrees of
//    the tokens inside weight_cutoff gives every token its slot range, a slot -> token map is written once per frame
//    (the slots of one layer never exceed the graph's arc count: every live token is a different state).
//  * ProcessNonemitting (:58-118) is a LIFO worklist over the whole list; what depends on its order is which of two
//    equal-cost epsilon paths sets the back-pointer and where a newly reached state enters the list.  Only tokens
//    whose state HAS an epsilon-input out-arc can do anything when popped, so the wave compacts those (in reverse list
//    order = pop order) and lane 0 runs the worklist on them alone, with a stack for the elements it pushes (a pushed
//    element is popped before the next original one, as in the reference's vector used as a stack); a new state is
//    appended to the list (its bucket is new) and found again through a state -> position table.
// Costs use the reference's exact expressions: new_weight = (arc.w + tok.cost) + ac_cost for the pruning test
// (:215), Token cost = (tok.cost + arc.w) + ac_cost (faster-decoder.h:125).
// eps: the set has epsilon-input arcs; odeg > 0: every state has <= odeg out-arcs and slots are token * odeg + arc (0: exact
// prefix sums); maxp: the largest number of score rows of an utterance (LDS sizing).
//
// More than 1000 states (round 4).  hash_size starts at 1000 and grows to hash_ratio x the token count of a frame
// (faster-decoder.cc:337-344; it never shrinks, not even between the two attempts of the retry beam), so states s and s + k hash_size
// SHARE a bucket and the list order is no longer the insertion order: elements are grouped by bucket, groups in order of their first
// element, insertion order inside a group (hash-list-inl.h:129-174).  `rerank` below turns an array in insertion order into that
// order with two counting passes (per element a walk over the <= S / hash_size states of its bucket; a prefix sum of the group sizes
// over the groups' first elements) -- no hash table, no sort.  GM: the graph tables (read-only after the set-up) are carved out of
// the utterance's HBM scratch slice instead of LDS, which is then left to the per-frame tables: ~3300 states on a chain graph
// instead of ~1600.
template <bool GM>
__global__ __launch_bounds__(64) void k2_viterbi_faithful_wave(K2Args a, int eps, int odeg, int maxp) {
  extern __shared__ __attribute__((aligned(16))) unsigned char k2_lds[];
  unsigned char* const smem = k2_lds;
  const int u = blockIdx.x;
  if (a.status[u] != K2_ST_NEED_FALLBACK) return;
  const int lane = threadIdx.x;
  const int64_t f0 = a.frame_off[u];
  const int T = (int)(a.frame_off[u + 1] - f0);
  const int tpad = (T + 31) & ~31;
  const int64_t s0 = a.state_off[a.gidx[u]];
  const int S = (int)(a.state_off[a.gidx[u] + 1] - s0);
  const int64_t in0 = a.in_off[s0];
  const int A = (int)(a.in_off[s0 + S] - in0);
  const int64_t o0 = a.out_off[s0];
  const int start = a.start[a.gidx[u]];
  const float* llu = a.ll + a.ll_off[u];
  uint8_t* bp = a.bp + a.bp_off[u];
  const int Sp = (S + 15) & ~15;
  const int MS = a.max_states, MA = a.max_inarcs;
  const int P = tpad > 0 ? (int)((a.ll_off[u + 1] - a.ll_off[u]) / tpad) : 0;   // score rows of this utterance
  const bool use_pos = eps || MS > 1000;      // state -> list position table: epsilon worklist, shared hash buckets

  // ---- per-frame tables (LDS) ----
  // (their byte count: k2_lds_wave_mut, the graph tables' below: k2_lds_wave_graph, khg_k2.hip)
  double* tkc0 = reinterpret_cast<double*>(smem);                       // token costs, list order (two layers)
  double* tkc1 = tkc0 + MS;
  unsigned long long* st_key = reinterpret_cast<unsigned long long*>(tkc1 + MS);   // per state: min token cost (ordered key)
  int32_t* tks0 = reinterpret_cast<int32_t*>(st_key + MS);              // token states, list order
  int32_t* tks1 = tks0 + MS;
  int32_t* st_first = tks1 + MS;                                        // per state: first surviving arc (flattened index)
  int32_t* st_win = st_first + MS;                                      // per state: first arc attaining the min cost
  float* tmp = reinterpret_cast<float*>(st_win + MS);                   // GetCutoff tmp_array_
  float* sc = tmp + MS;                                                 // [maxp] this frame's scores, one per score row
  int32_t* nxt = reinterpret_cast<int32_t*>(sc + maxp);
  // exact slot numbering only
  int32_t* s_tok = nxt;                                                 // [MA] flattened slot -> token (list position)
  int32_t* offs = s_tok + MA;                                           // [MS] token -> first slot
  if (odeg == 0) nxt = offs + MS;
  int32_t* st_pos = nxt;                                                // [MS] state -> list position in the layer being built
  if (use_pos) nxt = st_pos + MS;
  int32_t* stack = nxt;                                                 // [MS + MA + 1] epsilon worklist; last = shared count
  if (eps) nxt = stack + MS + MA + 1;
  unsigned long long* s_surv = reinterpret_cast<unsigned long long*>(
      (reinterpret_cast<uintptr_t>(nxt) + 7) & ~uintptr_t(7));          // survivor mask per 64-slot block
  unsigned char* const mut_end = reinterpret_cast<unsigned char*>(s_surv + ((MA > MS * odeg ? MA : MS * odeg) + 63) / 64 + 1);
  // ---- graph tables (LDS behind the per-frame tables, or the utterance's HBM scratch slice) ----
  unsigned char* const gbase = GM ? a.gscratch + (size_t)blockIdx.x * a.gscratch_stride : mut_end;
  int32_t* s_in_off = reinterpret_cast<int32_t*>(gbase);                // [MS+1]
  int32_t* s_out_off = s_in_off + MS + 1;                               // [MS+1]
  int32_t* s_src = s_out_off + MS + 1;                                  // in-arc order ...
  int32_t* s_col = s_src + MA;
  float* s_w = reinterpret_cast<float*>(s_col + MA);
  int32_t* s_dst = reinterpret_cast<int32_t*>(s_w + MA);
  int32_t* o_ai = s_dst + MA;                                           // out-arc order -> in-arc index
  // epsilon-input arcs only
  int32_t* e_off = o_ai + MA;                                           // [MS+1]
  int32_t* e_ai = e_off + MS + 1;                                       // [MA] epsilon-input out-arcs as in-arc indices
  uint8_t* s_ord = reinterpret_cast<uint8_t*>(eps ? e_ai + MA : e_off);
  uint8_t* s_eps = s_ord + MA;                                          // [MS] (eps) the state has an epsilon-input out-arc

  for (int s = lane; s <= S; s += 64) { s_in_off[s] = (int32_t)(a.in_off[s0 + s] - in0); s_out_off[s] = (int32_t)(a.out_off[s0 + s] - o0); }
  for (int i = lane; i < A; i += 64) {
    const int tidl = a.in_tid[in0 + i];
    float w = a.in_w[in0 + i];
    if (a.trans_cost && tidl >= 1) w = w + a.trans_cost[tidl];
    s_src[i] = a.in_src[in0 + i];
    s_col[i] = a.in_col[in0 + i];
    s_w[i] = w;
    o_ai[i] = a.out_inidx[o0 + i];
  }
  __syncthreads();
  for (int s = lane; s < S; s += 64) {
    for (int i = s_in_off[s]; i < s_in_off[s + 1]; ++i) { s_dst[i] = s; s_ord[i] = (uint8_t)(i - s_in_off[s]); }
  }
  // epsilon-input out-arcs per state, in arc order: e_off / e_ai (in-arc indices); maxeps = the largest count
  int maxeps = 1;
  if (eps) {
    int run = 0;
    for (int base = 0; base < S; base += 64) {
      const int s = base + lane;
      int ce = 0;
      if (s < S) for (int k = s_out_off[s]; k < s_out_off[s + 1]; ++k) ce += s_col[o_ai[k]] < 0;
      int inc = ce;
      for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o); if (lane >= o) inc += t; }
      if (s < S) {
        int e = run + inc - ce;
        e_off[s] = e;
        s_eps[s] = ce > 0;
        for (int k = s_out_off[s]; k < s_out_off[s + 1]; ++k) { const int ai = o_ai[k]; if (s_col[ai] < 0) e_ai[e++] = ai; }
      }
      run += __shfl(inc, 63);
      for (int o = 32; o > 0; o >>= 1) { const int t = __shfl_xor(ce, o); ce = t > ce ? t : ce; }
      maxeps = ce > maxeps ? ce : maxeps;
    }
    if (lane == 0) e_off[S] = run;
  }
  __syncthreads();

  // ProcessNonemitting (faster-decoder.cc:58-118) on the layer being built: kc / ks = its list (n0 elements), bpl = its
  // back-pointer row.  Returns the new element count.  Called by the whole wave.
  // The worklist pops the list's elements last to first and every element it pushes (a state it created or made cheaper)
  // before the next original one.  Only elements whose state has an epsilon-input out-arc do anything when popped.  While
  // no relaxation creates or improves such a state ("one level": the usual case, an epsilon arc leads into a chain of
  // emitting arcs), the pops are exactly the original epsilon-capable elements in reverse list order with their costs as
  // ProcessEmitting left them, and the relaxations form one flat sequence (element, epsilon arc): a state's final cost is
  // the minimum over the relaxations inside the cutoff and its own token, its back-pointer the FIRST relaxation that
  // attains a strictly cheaper minimum (:104 replaces on strict '<' only), and states without a token enter the list in
  // order of their first relaxation inside the cutoff -- the same atomic-minimum / first-index / prefix-count passes as
  // ProcessEmitting above.  The first pass also detects the other case (a relaxation that creates or improves an
  // epsilon-capable state) before anything is modified, and lane 0 then runs the worklist itself.
  // List order with shared hash buckets (see the header).  src: n elements in an order whose index is the insertion stamp (st_pos[state] =
  // index); dst: the same elements grouped by bucket (state % hs), groups in order of their first element, stamp order inside a group.
  // st_pos is updated to the new positions.
  auto rerank = [&](const double* src_c, const int32_t* src_s, double* dst_c, int32_t* dst_s, int n, int hs) {
    int32_t* gbase_of = reinterpret_cast<int32_t*>(tmp);        // per state, set for the first element of a group: the group's first position
    int run = 0;
    for (int base = 0; base < n; base += 64) {
      const int i = base + lane;
      int w = 0, st = 0;
      if (i < n) {
        st = src_s[i];
        int cnt = 0; bool lead = true;
        for (int m = st % hs; m < S; m += hs) { const int p = st_pos[m]; if (p >= 0) { ++cnt; if (p < i) lead = false; } }
        w = lead ? cnt : 0;
      }
      int inc = w;
      for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o); if (lane >= o) inc += t; }
      if (w) gbase_of[st] = run + inc - w;
      run += __shfl(inc, 63);
    }
    __syncthreads();
    for (int base = 0; base < n; base += 64) {
      const int i = base + lane;
      if (i < n) {
        const int st = src_s[i];
        int rank = 0, lp = i, ls = st;
        for (int m = st % hs; m < S; m += hs) { const int p = st_pos[m]; if (p >= 0) { if (p < i) ++rank; if (p < lp) { lp = p; ls = m; } } }
        const int pos = gbase_of[ls] + rank;
        dst_s[pos] = st; dst_c[pos] = src_c[i];
      }
    }
    __syncthreads();
    for (int i = lane; i < n; i += 64) st_pos[dst_s[i]] = i;
    __syncthreads();
  };

  // (kc, ks): the list; (okc, oks): the other layer's arrays, free at this point -- the re-ranked list goes there and the pairs swap
  auto process_nonemitting = [&](double cutoff, uint8_t* bpl, double*& kc, int32_t*& ks, double*& okc, int32_t*& oks, int n0, size_t hsz) -> int {
    int32_t* elist = reinterpret_cast<int32_t*>(tmp);
    auto relist = [&](int n) {                       // new elements were appended: their buckets may be occupied already
      if (n > n0 && hsz < (size_t)S) {
        rerank(kc, ks, okc, oks, n, (int)hsz);
        double* td = kc; kc = okc; okc = td; int32_t* ti = ks; ks = oks; oks = ti;
      }
    };
    int ne = 0;
    for (int base = 0; base < n0; base += 64) {          // pop order = reverse list order
      const int i = n0 - 1 - (base + lane);
      const bool cap = i >= 0 && s_eps[ks[i]];
      const unsigned long long m = __ballot(cap);
      if (cap) elist[ne + __popcll(m & ((1ull << lane) - 1ull))] = i;
      ne += __popcll(m);
    }
    if (ne == 0) return n0;
    for (int s = lane; s < S; s += 64) {
      const int p0 = st_pos[s];
      st_key[s] = p0 >= 0 ? k2_d2key(kc[p0]) : ~0ull;
      st_first[s] = INT32_MAX; st_win[s] = INT32_MAX;
    }
    __syncthreads();
    const int FE = ne * maxeps;
    auto earc = [&](int f, double& ncost, int& ai) -> bool {
      const int k = f / maxeps, j = f - k * maxeps;
      const int i = elist[k];
      const int st = ks[i];
      const int e = e_off[st] + j;
      if (e >= e_off[st + 1]) return false;
      const double tc = kc[i];
      if (tc > cutoff) return false;                            // :75-78
      ai = e_ai[e];
      ncost = tc + s_w[ai];                                     // Token(arc, prev) faster-decoder.h:135
      return !(ncost > cutoff);                                 // :89-92
    };
    bool multi = false;
    for (int base = 0; base < FE; base += 64) {
      const int f = base + lane;
      double nc = 0.0; int ai = 0;
      if (f < FE && earc(f, nc, ai)) {
        const int ns = s_dst[ai];
        const int p0 = st_pos[ns];
        if (s_eps[ns] && (p0 < 0 || nc < kc[p0])) multi = true;
        atomicMin(&st_key[ns], k2_d2key(nc));
        if (p0 < 0) atomicMin(&st_first[ns], f);
      }
    }
    const bool serial = __ballot(multi) != 0ull;
    __syncthreads();
    if (!serial) {
      for (int base = 0; base < FE; base += 64) {
        const int f = base + lane;
        double nc = 0.0; int ai = 0;
        if (f < FE && earc(f, nc, ai)) {
          const int ns = s_dst[ai];
          const int p0 = st_pos[ns];
          if (k2_d2key(nc) == st_key[ns] && (p0 < 0 || nc < kc[p0])) atomicMin(&st_win[ns], f);
        }
      }
      __syncthreads();
      int n = n0;
      for (int base = 0; base < FE; base += 64) {
        const int f = base + lane;
        double nc = 0.0; int ai = 0;
        bool first = false; int ns = 0;
        if (f < FE && earc(f, nc, ai)) {
          ns = s_dst[ai];
          first = st_first[ns] == f;                            // only states without a token have one
          if (st_win[ns] == f) { bpl[ns] = s_ord[ai]; if (!first) { const int p0 = st_pos[ns]; if (p0 >= 0 && p0 < n0) kc[p0] = nc; } }
        }
        const unsigned long long fm = __ballot(first);
        if (first) {
          const int pos = n + __popcll(fm & ((1ull << lane) - 1ull));
          ks[pos] = ns; kc[pos] = k2_key2d(st_key[ns]); st_pos[ns] = pos;
        }
        n += __popcll(fm);
      }
      __syncthreads();
      relist(n);
      return n;
    }
    if (lane == 0) {
      int n = n0, sp = 0;
      const int cap_sp = MS + MA;
      for (int k = 0; k < ne; ++k) {
        int pos = elist[k];
        for (;;) {
          const int state = ks[pos];
          const double tcost = kc[pos];
          if (!(tcost > cutoff)) {                                  // :75-78
            for (int e = e_off[state]; e < e_off[state + 1]; ++e) {
              const int ai = e_ai[e];
              const double ncost = tcost + s_w[ai];                 // Token(arc, prev) faster-decoder.h:135
              if (ncost > cutoff) continue;                         // :89-92
              const int ns = s_dst[ai];
              int p0 = st_pos[ns];
              bool push = false;
              if (p0 < 0) { p0 = n++; ks[p0] = ns; kc[p0] = ncost; st_pos[ns] = p0; bpl[ns] = s_ord[ai]; push = true; }
              else if (kc[p0] > ncost) { kc[p0] = ncost; bpl[ns] = s_ord[ai]; push = true; }   // :104
              if (push && s_eps[ns]) { if (sp < cap_sp) stack[sp++] = p0; else atomicOr(a.err_flag, 2); }
            }
          }
          if (!sp) break;
          pos = stack[--sp];
        }
      }
      stack[MS + MA] = n;
    }
    __syncthreads();
    const int n_after = stack[MS + MA];
    relist(n_after);
    return n_after;
  };

  // wave helpers (one wave per workgroup)
  auto wave_min_d = [&](double v) { for (int o = 32; o > 0; o >>= 1) { const double t = __shfl_xor(v, o); v = t < v ? t : v; } return v; };
  auto incl_prefix_min = [&](double v) {
    for (int o = 1; o < 64; o <<= 1) { const double t = __shfl_up(v, o); if (lane >= o && t < v) v = t; }
    return v;
  };

  int status = KHG_ALIGN_ERROR;
  int best_state = -1;
  float beam = a.beam;
  size_t hash_size = 1000;                         // faster-decoder.cc:30; the decoder object (and its hash size) outlives the first attempt
  for (int attempt = 0; attempt < 2; ++attempt) {
    double* tkc = tkc0; int32_t* tks = tks0;       // current layer
    double* nkc = tkc1; int32_t* nks = tks1;       // layer being built
    int n = 1;
    if (lane == 0) { tks[0] = start; tkc[0] = 0.0; }
    for (int s = lane; s < S; s += 64) { bp[s] = K2_BP_NONE; if (use_pos) st_pos[s] = s == start ? 0 : -1; }
    __syncthreads();
    if (eps) n = process_nonemitting((double)3.402823466e+38f, bp, tkc, tks, nkc, nks, n, hash_size);   // InitDecoding, faster-decoder.cc:54
    // a frame's scores go through LDS (every arc is looked at by three passes); rows lane and lane + 64 are requested one
    // frame ahead into registers, so the strided gather's latency lies under the previous frame's passes
    float pre0 = 0.0f, pre1 = 0.0f;
    if (T > 0) { if (lane < P) pre0 = llu[(int64_t)lane * tpad]; if (lane + 64 < P) pre1 = llu[(int64_t)(lane + 64) * tpad]; }
    for (int frame = 0; frame < T; ++frame) {
      uint8_t* bpn = bp + (int64_t)(frame + 1) * Sp;
      if (lane < P) sc[lane] = pre0;
      if (lane + 64 < P) sc[lane + 64] = pre1;
      for (int c = lane + 128; c < P; c += 64) sc[c] = llu[(int64_t)c * tpad + frame];
      if (frame + 1 < T) {
        if (lane < P) pre0 = llu[(int64_t)lane * tpad + frame + 1];
        if (lane + 64 < P) pre1 = llu[(int64_t)(lane + 64) * tpad + frame + 1];
      }
      for (int s = lane; s < S; s += 64) { bpn[s] = K2_BP_NONE; st_key[s] = ~0ull; st_first[s] = INT32_MAX; st_win[s] = INT32_MAX; if (use_pos) st_pos[s] = -1; }
      // ---- GetCutoff (faster-decoder.cc:243-335) ----
      double bc = INFINITY; int bi = INT32_MAX;
      for (int i = lane; i < n; i += 64) { const double c = tkc[i]; if (c < bc) { bc = c; bi = i; } }   // first minimum of my elements
      for (int o = 32; o > 0; o >>= 1) {
        const double c2 = __shfl_xor(bc, o); const int i2 = __shfl_xor(bi, o);
        if (c2 < bc || (c2 == bc && i2 < bi)) { bc = c2; bi = i2; }
      }
      const double best_cost = bc;
      const int best_elem = (bi == INT32_MAX) ? -1 : bi;
      const size_t count = (size_t)n;
      double weight_cutoff; float adaptive_beam;
      if (a.max_active == INT32_MAX && a.min_active == 0) {
        adaptive_beam = beam; weight_cutoff = best_cost + beam;
      } else {
        for (int i = lane; i < n; i += 64) tmp[i] = (float)tkc[i];
        __syncthreads();
        // k-th order statistic (0-based) of tmp[0..n) = the value nth_element leaves at position k: radix select on the
        // order-preserving integer image of the floats -- the largest key K with #{keys < K} <= k, one ballot count per
        // bit and 64 elements (the keys of the first 256 elements stay in registers)
        auto fkey = [](float x) { const unsigned b = __float_as_uint(x); return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u); };
        auto kth = [&](size_t k) -> float {
          unsigned kr[4];
#pragma unroll
          for (int b = 0; b < 4; ++b) { const int i = b * 64 + lane; kr[b] = i < n ? fkey(tmp[i]) : 0xFFFFFFFFu; }
          unsigned ans = 0;
          for (int bit = 31; bit >= 0; --bit) {
            const unsigned cand = ans | (1u << bit);
            int cnt = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) if (b * 64 < n) cnt += __popcll(__ballot(kr[b] < cand));
            for (int base = 256; base < n; base += 64) {
              const int i = base + lane;
              const unsigned key = i < n ? fkey(tmp[i]) : 0xFFFFFFFFu;
              cnt += __popcll(__ballot(key < cand));
            }
            if ((size_t)cnt <= k) ans = cand;
          }
          return __uint_as_float(ans ^ ((ans >> 31) ? 0x80000000u : 0xFFFFFFFFu));
        };
        const double beam_cutoff = best_cost + beam;
        double min_active_cutoff = INFINITY, max_active_cutoff = INFINITY;
        if (count > (size_t)a.max_active) max_active_cutoff = kth((size_t)a.max_active);
        if (max_active_cutoff < beam_cutoff) {
          adaptive_beam = max_active_cutoff - best_cost + a.beam_delta;
          weight_cutoff = max_active_cutoff;
        } else {
          if (count > (size_t)a.min_active) {
            if (a.min_active == 0) min_active_cutoff = best_cost;
            else min_active_cutoff = kth((size_t)a.min_active);
          }
          if (min_active_cutoff > beam_cutoff) {
            adaptive_beam = min_active_cutoff - best_cost + a.beam_delta;
            weight_cutoff = min_active_cutoff;
          } else {
            adaptive_beam = beam;
            weight_cutoff = beam_cutoff;
          }
        }
      }
      const size_t new_sz = (size_t)((float)count * a.hash_ratio);   // PossiblyResizeHash (:337-344): only ever grows
      if (new_sz > hash_size) hash_size = new_sz;
      // ---- initial next_weight_cutoff from the best token's arcs (:175-188), evaluated by every lane alike ----
      double next_weight_cutoff = INFINITY;
      if (best_elem >= 0) {
        const int state = tks[best_elem];
        const double tcost = tkc[best_elem];
        for (int k = s_out_off[state]; k < s_out_off[state + 1]; ++k) {
          const int ai = o_ai[k];
          const int col = s_col[ai];
          if (col < 0) continue;
          const float ac_cost = -1 * (a.acoustic_scale * sc[col]);
          const double new_weight = s_w[ai] + tcost + ac_cost;
          if (new_weight + adaptive_beam < next_weight_cutoff) next_weight_cutoff = new_weight + adaptive_beam;
        }
      }
      __syncthreads();
      // ---- ProcessEmitting (:195-236): pass 1 = pruning (prefix-min) + per-state minimum and first insertion ----
      // slots of the flattened (token, arc) sequence.  Small out-degrees (training graphs): slot = token * odeg + arc.
      // Otherwise exact: a prefix sum of the out-degrees, tokens outside weight_cutoff (:198) take none, slot -> token map.
      int F = n * odeg;
      if (odeg == 0) {
        for (int base = 0; base < n; base += 64) {
          const int i = base + lane;
          int dg = 0;
          if (i < n && tkc[i] < weight_cutoff) { const int st = tks[i]; dg = s_out_off[st + 1] - s_out_off[st]; }
          int inc = dg;
          for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o); if (lane >= o) inc += t; }
          const int first_slot = F + inc - dg;
          if (i < n) offs[i] = first_slot;
          for (int j = 0; j < dg; ++j) s_tok[first_slot + j] = i;
          F += __shfl(inc, 63);
        }
        __syncthreads();
      }
      double carry = next_weight_cutoff;
      auto arc_of = [&](int f, double& nw, double& tokc, int& ai) -> bool {
        int i, k;
        double tc;
        if (odeg) {
          i = f / odeg;
          const int jj = f - i * odeg;
          tc = tkc[i];
          if (!(tc < weight_cutoff)) return false;
          const int st = tks[i];
          k = s_out_off[st] + jj;
          if (k >= s_out_off[st + 1]) return false;
        } else {
          i = s_tok[f];
          tc = tkc[i];
          k = s_out_off[tks[i]] + (f - offs[i]);
        }
        ai = o_ai[k];
        const int col = s_col[ai];
        if (col < 0) return false;
        const float ac_cost = -1 * (a.acoustic_scale * sc[col]);
        nw = s_w[ai] + tc + ac_cost;               // :215 (pruning test)
        tokc = (tc + s_w[ai]) + ac_cost;           // Token constructor, faster-decoder.h:125
        return true;
      };
      for (int base = 0, blk = 0; base < F; base += 64, ++blk) {
        const int f = base + lane;
        double nw = INFINITY, tokc = INFINITY; int ai = 0;
        const bool valid = f < F && arc_of(f, nw, tokc, ai);
        const double cand = valid ? nw + adaptive_beam : INFINITY;
        const double inc = incl_prefix_min(cand);
        double ex = __shfl_up(inc, 1);
        if (lane == 0) ex = INFINITY;
        const double cutoff_before = carry < ex ? carry : ex;
        const bool surv = valid && nw < cutoff_before;
        const double tot = __shfl(inc, 63);
        carry = tot < carry ? tot : carry;
        const unsigned long long sm = __ballot(surv);
        if (lane == 0) s_surv[blk] = sm;
        if (surv) {
          const int dst = s_dst[ai];
          atomicMin(&st_key[dst], k2_d2key(tokc));
          atomicMin(&st_first[dst], f);
        }
      }
      __syncthreads();
      // pass 2: the first arc that attains each state's minimum (strict '<' replacement keeps the earliest)
      for (int base = 0, blk = 0; base < F; base += 64, ++blk) {
        const int f = base + lane;
        if ((s_surv[blk] >> lane) & 1ull) {
          double nw, tokc; int ai;
          arc_of(f, nw, tokc, ai);
          const int dst = s_dst[ai];
          if (k2_d2key(tokc) == st_key[dst]) atomicMin(&st_win[dst], f);
        }
      }
      __syncthreads();
      // pass 3: the new list in order of first insertion; back-pointers of the winners
      int nn = 0;
      for (int base = 0, blk = 0; base < F; base += 64, ++blk) {
        const int f = base + lane;
        bool first = false; int dst = 0, ai = 0;
        if ((s_surv[blk] >> lane) & 1ull) {
          double nw, tokc;
          arc_of(f, nw, tokc, ai);
          dst = s_dst[ai];
          first = st_first[dst] == f;
          if (st_win[dst] == f) bpn[dst] = s_ord[ai];
        }
        const unsigned long long fm = __ballot(first);
        if (first) {
          const int pos = nn + __popcll(fm & ((1ull << lane) - 1ull));
          nks[pos] = dst;
          nkc[pos] = k2_key2d(st_key[dst]);
          if (use_pos) st_pos[dst] = pos;
        }
        nn += __popcll(fm);
      }
      __syncthreads();
      n = nn;
      if (hash_size < (size_t)S && n > 1) rerank(nkc, nks, tkc, tks, n, (int)hash_size);   // shared buckets: into the old layer's arrays, no swap
      else { double* td = tkc; tkc = nkc; nkc = td; int32_t* ti = tks; tks = nks; nks = ti; }
      if (eps) n = process_nonemitting(carry, bpn, tkc, tks, nkc, nks, n, hash_size);    // :236 returns the running cutoff, :145 passes it on
    }
    // ---- ReachedFinal (:346-353) + best final token (:373-382): first minimum in list order ----
    double bc = INFINITY; int bi = INT32_MAX; bool reached = false;
    for (int i = lane; i < n; i += 64) {
      const float fw = a.final_w[s0 + tks[i]];
      if (tkc[i] != INFINITY && fw != INFINITY) reached = true;
      const double c = tkc[i] + fw;
      if (c < bc && c != INFINITY) { bc = c; bi = i; }
    }
    for (int o = 32; o > 0; o >>= 1) {
      const double c2 = __shfl_xor(bc, o); const int i2 = __shfl_xor(bi, o);
      if (c2 < bc || (c2 == bc && i2 < bi)) { bc = c2; bi = i2; }
    }
    reached = __ballot(reached) != 0ull;
    best_state = (bi == INT32_MAX) ? -1 : tks[bi];
    if (reached) { status = (attempt ? KHG_ALIGN_RETRIED : 0); break; }
    if (attempt == 0 && a.retry_beam != 0.0f) { beam = a.retry_beam; __syncthreads(); continue; }  // decoder-wrappers.cc:55-67
    status = KHG_ALIGN_ERROR | (attempt ? KHG_ALIGN_RETRIED : 0);
    best_state = -1;
    break;
  }
  (void)wave_min_d;
  __syncthreads();
  if (best_state < 0) {
    for (int t = lane; t < T; t += 64) a.ali_fb[f0 + t] = 0;
    if (lane == 0) { a.num_words[u] = 0; a.like[u] = 0.0f; a.status[u] = status | KHG_ALIGN_ERROR | KHG_ALIGN_FALLBACK; }
    return;
  }
  __threadfence_block();
  if (lane == 0) {
    const int st = k2_finish(a, u, best_state, s_in_off, s_src, s_col, s_w, false, nullptr);
    if (st != KHG_ALIGN_DONE) {
      for (int t = 0; t < T; ++t) a.ali_fb[f0 + t] = 0;
      a.status[u] = KHG_ALIGN_ERROR | status | KHG_ALIGN_FALLBACK;
    } else {
      a.status[u] = status | KHG_ALIGN_FALLBACK;
    }
  }
}

// ---------------------------------------------------------------------------------------
// Order-faithful FasterDecoder, CHAIN form (round 6): graphs WITHOUT epsilon-input arcs, <= 1000 states (every state owns its hash
// bucket for good: the list order is the order of first insertion, faster-decoder.cc:30 + hash-list-inl.h:129-174) and out-degree
// <= ODEG <= 4 -- the training graphs of linear transcripts.  Same answers as k2_viterbi_faithful_wave, token for token; what changed
// is the length of the dependent chains a frame costs (the decoder's time is T x that latency: one wave per utterance, every
// utterance in flight at once):
//  * one lane per TOKEN in pass 1: the token's <= ODEG out-arcs come from one static record table indexed by (state, arc) -- weight
//    with the transition cost folded in, score row, destination, ordinal -- so a slot costs three dependent LDS reads (token ->
//    record -> score) instead of six; the running next_weight_cutoff (an exclusive prefix-min over the flattened (token, arc)
//    sequence, :195-236) is a per-lane chain over the lane's own arcs + ONE wave scan of the lanes' minima on DPP row shifts
//    (v_mov_dpp + v_min_f64: ~20 instructions) instead of a ds_bpermute shuffle ladder per 64 slots;
//  * what pass 1 decided is parked per slot (token cost, destination | ordinal | survivor bit): pass 2, one lane per SLOT so that
//    lane order = insertion order, reads it back instead of re-deriving it, and does in one sweep what took two (the first arc
//    attaining a state's minimum: atomicMin of (slot << 8 | ordinal); the new list: compaction of the first survivors);
//  * the back-pointer row is assembled in LDS and leaves as whole dwords once per frame -- no byte scatter, no per-frame
//    re-initialisation of the row in HBM -- and NOTHING in the frame loop waits for a vector-memory operation except the score
//    gather issued a frame ahead (the wave form's __syncthreads() drained the byte stores six times per frame);
//  * GetCutoff (:243-335) takes nth_element's value only when it can matter: min_active_cutoff > beam_cutoff iff at most
//    min_active tokens lie at or below the beam cutoff -- one ballot count; the radix select runs in that case alone.
// k2_finish by a whole wave for graphs WITHOUT epsilon-input arcs (the chain decoder's tail; same arithmetic, same outputs): the
// trace-back walks 8-layer blocks of back-pointer rows staged in LDS by coalesced loads (one lane walking rows in HBM stood on a
// dependent global load per layer), the forward replay handles 64 path entries per step as k2_viterbi_dp's does -- only the fp64
// token cost is a serial chain -- and reads the arcs' weights / labels from the set's tables in HBM (64 independent gathers per
// step; the decoder's LDS holds only what its frame loop needs: it is bound by how many utterances a CU keeps in flight).
// stage: >= 9 * ((S + 15) & ~15) bytes of LDS, 16-byte aligned.  Returns the status bits on every lane.
#define K2_TB 8
__device__ int k2_finish_wave(const K2Args& a, int u, int best_state, const int32_t* s_in_off, const uint16_t* s_src, uint8_t* stage, int lane) {
  const int64_t f0 = a.frame_off[u];
  const int T = (int)(a.frame_off[u + 1] - f0);
  const int tpad = (T + 31) & ~31;
  const int S = (int)(a.state_off[a.gidx[u] + 1] - a.state_off[a.gidx[u]]);
  const int Sp = (S + 15) & ~15;
  const int64_t in0 = a.in_off[a.state_off[a.gidx[u]]];
  const uint8_t* bp = a.bp + a.bp_off[u];
  int32_t* path = a.path + a.path_off[u];
  const int path_cap = (int)(a.path_off[u + 1] - a.path_off[u]);
  const float* llu = a.ll + a.ll_off[u];
  if (T > path_cap) return KHG_ALIGN_ERROR;
  int st = best_state, bad = 0;
  for (int hi = T; hi > 0 && !bad; ) {
    const int lo = hi > K2_TB ? hi - K2_TB : 0;          // layers lo + 1 .. hi are consumed (every arc emits: one layer per step)
    const int nv = (hi - lo) * (Sp >> 4);                // 16-byte vectors of rows lo + 1 .. hi
    const uint4* src = reinterpret_cast<const uint4*>(bp + (int64_t)(lo + 1) * Sp);
    uint4* dst = reinterpret_cast<uint4*>(stage);
    for (int i0 = 0; i0 < nv; i0 += 256) {
      uint4 v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) { const int i = i0 + 64 * k + lane; if (i < nv) v[k] = src[i]; }
#pragma unroll
      for (int k = 0; k < 4; ++k) { const int i = i0 + 64 * k + lane; if (i < nv) dst[i] = v[k]; }
    }
    k2_lds_sync();
    // the walk is uniform work: every lane follows it (LDS broadcasts), lane (hi - layer) keeps the arc of its step
    int mine = 0;
    for (int layer = hi; layer > lo; --layer) {
      const int ord = stage[(layer - lo - 1) * Sp + st];
      if (ord == K2_BP_NONE) { bad = 1; break; }
      const int ai = s_in_off[st] + ord;
      if (lane == hi - layer) mine = ai;
      st = s_src[ai];
    }
    if (!bad && lane < hi - lo) path[T - hi + lane] = mine;      // path[k] = arc of layer T - k (backward order, as k2_finish leaves it)
    hi = lo;
    k2_lds_sync();
  }
  if (bad) return KHG_ALIGN_ERROR;
  const int n = T;
  k2_global_sync();   // path[] is read by other lanes below
  double cost = 0.0;
  float v1 = 0.0f, v2 = 0.0f;
  int nw = 0;
  const int64_t wcap = a.words_off[u + 1] - a.words_off[u];
  int32_t* words = a.words + a.words_off[u];
  for (int base = n - 1; base >= 0; base -= 64) {
    const int idx = base - lane;                     // lane k handles path[base - k] (forward order): frame tf
    const int tf = n - 1 - base + lane;
    int ol = 0; float w = 0.0f, ac = 0.0f;
    if (idx >= 0) {
      const int ai = path[idx];
      const int tidl = a.in_tid[in0 + ai];
      w = a.in_w[in0 + ai];
      if (a.trans_cost && tidl >= 1) w = w + a.trans_cost[tidl];          // Times(arc.weight, -scaled_log_prob), hmm-utils.cc:465-493
      ol = a.in_olabel[in0 + ai];
      ac = -1 * (a.acoustic_scale * llu[(int64_t)a.in_col[in0 + ai] * tpad + tf]);
      a.ali_fb[f0 + tf] = tidl;
    }
    const int cnt = base >= 63 ? 64 : base + 1;
    const double cost_in = cost;
    double ca = 0.0;
    for (int k = 0; k < cnt; ++k) {
      const float wk = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w), k));
      const float ack = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ac), k));
      const double ncost = (cost + wk) + ack;                              // faster-decoder.h:125
      ca = lane == k ? ncost : ca;
      cost = ncost;
    }
    double cb = __shfl_up(ca, 1);                                          // the cost BEFORE this lane's entry
    if (lane == 0) cb = cost_in;
    const bool mine = idx >= 0;
    const float tot_cost = (float)(ca - cb);                               // faster-decoder.cc:393
    const float ac_cost = tot_cost - w;
    {
      const unsigned long long wm = __ballot(mine && ol != 0);             // word labels, path order
      if (mine && ol != 0) { const int pos = nw + __popcll(wm & ((1ull << lane) - 1ull)); if (pos < wcap) words[pos] = ol; }
      nw += __popcll(wm);
    }
    for (int k = 0; k < cnt; ++k) {                                        // LatticeWeight Times, path order
      v1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w), k)) + v1;
      v2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ac_cost), k)) + v2;
    }
  }
  v1 = a.final_w[a.state_off[a.gidx[u]] + best_state] + v1;  // faster-decoder.cc:415-417
  v2 = 0.0f + v2;
  if (lane == 0) {
    a.num_words[u] = nw;
    a.like[u] = -(v1 + v2) / a.like_scale;           // decoder-wrappers.cc:95
  }
  return nw > wcap ? KHG_ALIGN_ERROR : KHG_ALIGN_DONE;
}

struct K2ChainArc { float w; int16_t col; uint16_t dst; };        // col < 0: the state has no such out-arc

// inclusive prefix-minimum over the 64 lanes (NaN candidates are ignored, like the reference's `x < cutoff` tests)
__device__ __forceinline__ double k2_scan_min_d(double v) {
  const double inf = INFINITY;
  v = __builtin_fmin(v, k2_dpp_d<0x111, 0xf>(inf, v));      // row_shr:1
  v = __builtin_fmin(v, k2_dpp_d<0x112, 0xf>(inf, v));      // row_shr:2
  v = __builtin_fmin(v, k2_dpp_d<0x114, 0xf>(inf, v));      // row_shr:4
  v = __builtin_fmin(v, k2_dpp_d<0x118, 0xf>(inf, v));      // row_shr:8
  v = __builtin_fmin(v, k2_dpp_d<0x142, 0xa>(inf, v));      // row_bcast:15 -> rows 1, 3
  v = __builtin_fmin(v, k2_dpp_d<0x143, 0xc>(inf, v));      // row_bcast:31 -> rows 2, 3
  return v;
}
__device__ __forceinline__ double k2_lane63_d(double v) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}
__device__ __forceinline__ int k2_wave_min_i(int v) {       // wave minimum, uniform result
  v = min(v, __builtin_amdgcn_update_dpp(INT32_MAX, v, 0x111, 0xf, 0xf, false));
  v = min(v, __builtin_amdgcn_update_dpp(INT32_MAX, v, 0x112, 0xf, 0xf, false));
  v = min(v, __builtin_amdgcn_update_dpp(INT32_MAX, v, 0x114, 0xf, 0xf, false));
  v = min(v, __builtin_amdgcn_update_dpp(INT32_MAX, v, 0x118, 0xf, 0xf, false));
  v = min(v, __builtin_amdgcn_update_dpp(INT32_MAX, v, 0x142, 0xa, 0xf, false));
  v = min(v, __builtin_amdgcn_update_dpp(INT32_MAX, v, 0x143, 0xc, 0xf, false));
  return __builtin_amdgcn_readlane(v, 63);
}

template <int ODEG>
__global__ __launch_bounds__(64) void k2_viterbi_faithful_chain(K2Args a, int maxp) {
  extern __shared__ __attribute__((aligned(16))) unsigned char k2_lds[];
  unsigned char* const smem = k2_lds;
  const int u = blockIdx.x;
  if (a.status[u] != K2_ST_NEED_FALLBACK) return;
  const int lane = threadIdx.x;
  const int64_t f0 = a.frame_off[u];
  const int T = (int)(a.frame_off[u + 1] - f0);
  const int tpad = (T + 31) & ~31;
  const int64_t s0 = a.state_off[a.gidx[u]];
  const int S = (int)(a.state_off[a.gidx[u] + 1] - s0);
  const int64_t in0 = a.in_off[s0];
  const int A = (int)(a.in_off[s0 + S] - in0);
  const int64_t o0 = a.out_off[s0];
  const int start = a.start[a.gidx[u]];
  const float* llu = a.ll + a.ll_off[u];
  uint8_t* bp = a.bp + a.bp_off[u];
  const int Sp = (S + 15) & ~15;
  const int MS = (a.max_states + 3) & ~3, MA = a.max_inarcs;
  const int P = tpad > 0 ? (int)((a.ll_off[u + 1] - a.ll_off[u]) / tpad) : 0;   // score rows of this utterance

  // ---- LDS (sized by the host for the batch maxima).  The frame loop's tables: 8-byte arrays first, then 4-byte, 2-byte, bytes.  What only
  // the set-up and the tail need (in-arc offsets and sources, the trace-back's rows) lies OVER them, from the start of the block: the
  // decoder is bound by how many utterances a CU keeps in flight, i.e. by LDS per utterance (10 KB at 121 states: 15 per CU) ----
  // (its byte count: k2_lds_chain, khg_k2.hip)
  double* tkc0 = reinterpret_cast<double*>(smem);                       // token costs, list order (two layers)
  double* tkc1 = tkc0 + MS;
  unsigned long long* st_key = reinterpret_cast<unsigned long long*>(tkc1 + MS);   // per state: min token cost (ordered key)
  double* sl_cost = reinterpret_cast<double*>(st_key + MS);             // [MS * ODEG] per slot: the token cost pass 1 computed
  K2ChainArc* oarc = reinterpret_cast<K2ChainArc*>(sl_cost + MS * ODEG);   // [MS * ODEG] out-arc records
  int32_t* sl_info = reinterpret_cast<int32_t*>(oarc + MS * ODEG);      // [MS * ODEG] per slot: dst | ordinal << 16 | survivor << 31
  float* tmp = reinterpret_cast<float*>(sl_info);                       // GetCutoff's array: over sl_info (dead between pass 2 and the next pass 1)
  int32_t* st_first = sl_info + MS * ODEG;                              // per state: first surviving slot
  int32_t* st_win = st_first + MS;                                      // per state: (first slot attaining the min cost) << 8 | ordinal
  float* sc = reinterpret_cast<float*>(st_win + MS);                    // [maxp] this frame's scores
  uint16_t* tks0 = reinterpret_cast<uint16_t*>(sc + maxp);              // token states, list order (<= 1000 states)
  uint16_t* tks1 = tks0 + MS;
  uint8_t* o_ord = reinterpret_cast<uint8_t*>(tks1 + MS);               // [MS * ODEG] ordinal of the out-arc among its destination's in-arcs
  // set-up and tail only (over tkc0 ...):
  int32_t* s_in_off = reinterpret_cast<int32_t*>(smem);                 // [MS + 1]
  uint16_t* s_src = reinterpret_cast<uint16_t*>(s_in_off + MS + 1);     // [MA] source state of the in-arc (the trace-back of k2_finish_wave)
  uint8_t* stage = smem + (((reinterpret_cast<unsigned char*>(s_src + MA) - smem) + 15) & ~ptrdiff_t(15));   // [(K2_TB + 1) * Sp] back-pointer rows of the trace-back
  long long* const prof = a.prof ? a.prof + 8 * ((size_t)gridDim.x + (size_t)u) : nullptr;      // second half of the stamp block
  int prof_frames = 0;
  long long pt[4] = {0, 0, 0, 0}, p0 = 0;      // KHG_K2_PROF: ticks in GetCutoff | pass 1 | pass 2 | row flush
#define K2C_STAMP(k) do { if (prof) { const long long now_ = clock64(); pt[k] += now_ - p0; p0 = now_; } } while (0)
  if (prof && lane == 0) prof[0] = clock64();
  for (int s = lane; s <= S; s += 64) s_in_off[s] = (int32_t)(a.in_off[s0 + s] - in0);
  k2_lds_sync();
  for (int s = lane; s < S; s += 64) {
    const int ob = (int)(a.out_off[s0 + s] - o0), oe = (int)(a.out_off[s0 + s + 1] - o0);
#pragma unroll
    for (int j = 0; j < ODEG; ++j) {
      K2ChainArc r{INFINITY, (int16_t)-1, (uint16_t)0};
      int ord = 0;
      if (ob + j < oe) {
        const int ai = a.out_inidx[o0 + ob + j];
        int lo = 0, hi = S - 1;                                          // destination of in-arc ai: the state whose in-arc range holds it
        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (s_in_off[mid] <= ai) lo = mid; else hi = mid - 1; }
        const int tidl = a.in_tid[in0 + ai];
        float w = a.in_w[in0 + ai];
        if (a.trans_cost && tidl >= 1) w = w + a.trans_cost[tidl];      // Times(arc.weight, -scaled_log_prob), hmm-utils.cc:465-493
        r = K2ChainArc{w, (int16_t)a.in_col[in0 + ai], (uint16_t)lo};
        ord = ai - s_in_off[lo];
      }
      oarc[s * ODEG + j] = r;
      o_ord[s * ODEG + j] = (uint8_t)ord;
    }
  }
  k2_lds_sync();

  auto fkey = [](float x) { const unsigned b = __float_as_uint(x); return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u); };
  // one dword of four back-pointer bytes per lane and step: states 4 l .. 4 l + 3 from st_win (INT32_MAX = none), which is reset with
  // st_key / st_first for the next frame in the same sweep
  auto flush_row = [&](uint8_t* row) {
    for (int sb = 4 * lane; sb < Sp; sb += 256) {          // (the four arrays are 16-byte aligned and padded to MS, a multiple of four)
      int4 wv = make_int4(INT32_MAX, INT32_MAX, INT32_MAX, INT32_MAX);
      if (sb < MS) {
        wv = *reinterpret_cast<const int4*>(st_win + sb);
        const int4 none = make_int4(INT32_MAX, INT32_MAX, INT32_MAX, INT32_MAX);
        *reinterpret_cast<int4*>(st_win + sb) = none;
        *reinterpret_cast<int4*>(st_first + sb) = none;
        const uint4 ones = make_uint4(~0u, ~0u, ~0u, ~0u);
        *reinterpret_cast<uint4*>(st_key + sb) = ones;
        *reinterpret_cast<uint4*>(st_key + sb + 2) = ones;
      }
      auto byte_of = [](int v) { return v == INT32_MAX ? (unsigned)K2_BP_NONE : ((unsigned)v & 0xffu); };
      *reinterpret_cast<unsigned*>(row + sb) = byte_of(wv.x) | (byte_of(wv.y) << 8) | (byte_of(wv.z) << 16) | (byte_of(wv.w) << 24);
    }
  };
  if (prof && lane == 0) prof[1] = clock64();
  int status = KHG_ALIGN_ERROR;
  int best_state = -1;
  float beam = a.beam;
  for (int attempt = 0; attempt < 2; ++attempt) {
    prof_frames += T;
    double* tkc = tkc0; uint16_t* tks = tks0;      // current layer
    double* nkc = tkc1; uint16_t* nks = tks1;      // layer being built
    int n = 1;
    if (lane == 0) { tks[0] = (uint16_t)start; tkc[0] = 0.0; }
    for (int s = lane; s < MS; s += 64) { st_win[s] = INT32_MAX; st_first[s] = INT32_MAX; st_key[s] = ~0ull; }
    k2_lds_sync();
    flush_row(bp);                                 // layer 0: no back-pointers (InitDecoding, faster-decoder.cc:41-56; no epsilon arcs)
    float pre0 = 0.0f, pre1 = 0.0f;
    if (T > 0) { if (lane < P) pre0 = llu[(int64_t)lane * tpad]; if (lane + 64 < P) pre1 = llu[(int64_t)(lane + 64) * tpad]; }
    for (int frame = 0; frame < T; ++frame) {
      if (lane < P) sc[lane] = pre0;
      if (lane + 64 < P) sc[lane + 64] = pre1;
      for (int c = lane + 128; c < P; c += 64) sc[c] = llu[(int64_t)c * tpad + frame];
      if (frame + 1 < T) {
        if (lane < P) pre0 = llu[(int64_t)lane * tpad + frame + 1];
        if (lane + 64 < P) pre1 = llu[(int64_t)(lane + 64) * tpad + frame + 1];
      }
      k2_lds_sync();
      if (prof) p0 = clock64();
      // ---- GetCutoff (faster-decoder.cc:243-335): the FIRST minimum in list order ----
      double bc = INFINITY; int bi = INT32_MAX;
      for (int i = lane; i < n; i += 64) { const double c = tkc[i]; if (c < bc) { bc = c; bi = i; } }
      const double best_cost = k2_lane63_d(k2_scan_min_d(bc));
      const int best_elem_raw = k2_wave_min_i(bc == best_cost ? bi : INT32_MAX);
      const int best_elem = best_elem_raw == INT32_MAX ? -1 : best_elem_raw;
      const size_t count = (size_t)n;
      double weight_cutoff; float adaptive_beam;
      if (a.max_active == INT32_MAX && a.min_active == 0) {
        adaptive_beam = beam; weight_cutoff = best_cost + beam;
      } else {
        const double beam_cutoff = best_cost + beam;
        // nth_element's answers are order statistics of the FLOAT costs (tmp_array_, :262).  The min_active branch can only fire when
        // its value exceeds beam_cutoff, i.e. when at most min_active floats lie at or below beam_cutoff: counted first, the select
        // (a radix select on the order-preserving integer image, one ballot count per bit) runs only then / for max_active.
        int le = 0;
        for (int base = 0; base < n; base += 64) {
          const int i = base + lane;
          le += __popcll(__ballot(i < n && (double)(float)tkc[i] <= beam_cutoff));
        }
        const bool need_max = count > (size_t)a.max_active;
        const bool need_min = count > (size_t)a.min_active && a.min_active != 0 && le <= a.min_active;
        unsigned* const tkey = reinterpret_cast<unsigned*>(tmp);          // the floats' order-preserving integer images
        if (need_max || need_min) {
          for (int i = lane; i < ((n + 3) & ~3); i += 64) tkey[i] = i < n ? fkey((float)tkc[i]) : 0xFFFFFFFFu;    // (padded to whole 16-byte reads)
          k2_lds_sync();
        }
        auto kth = [&](size_t k, size_t limit) -> float {     // k-th (0-based) smallest of the `limit` floats as nth_element leaves it (k < limit)
          unsigned ans = 0;
          if (limit <= 64) {
            // one element per lane: its rank = how many keys are smaller (the keys come back as LDS broadcasts, independent of each
            // other: no scalar round trip per step); the k-th smallest is the largest key of rank <= k
            const unsigned mykey = lane < (int)limit ? tkey[lane] : 0xFFFFFFFFu;
            int rank = 0;
            for (int j = 0; j < (int)limit; j += 4) {
              const uint4 q = *reinterpret_cast<const uint4*>(tkey + j);
              rank += (q.x < mykey ? 1 : 0) + (q.y < mykey ? 1 : 0) + (q.z < mykey ? 1 : 0) + (q.w < mykey ? 1 : 0);
            }
            unsigned v = (lane < (int)limit && (size_t)rank <= k) ? mykey : 0u;
            v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false));
            v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false));
            v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false));
            v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false));
            v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false));
            v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false));
            ans = (unsigned)__builtin_amdgcn_readlane((int)v, 63);
          } else {
            // radix select: the largest key K with #{keys < K} <= k, one ballot count per bit and 64 elements
            unsigned kr[2];                                     // (the keys of the first 128 elements stay in registers)
#pragma unroll
            for (int b = 0; b < 2; ++b) { const int i = b * 64 + lane; kr[b] = i < (int)limit ? tkey[i] : 0xFFFFFFFFu; }
            for (int bit = 31; bit >= 0; --bit) {
              const unsigned cand = ans | (1u << bit);
              int cnt = __popcll(__ballot(kr[0] < cand)) + __popcll(__ballot(kr[1] < cand));
              for (int base = 128; base < (int)limit; base += 64) {
                const int i = base + lane;
                const unsigned key = i < (int)limit ? tkey[i] : 0xFFFFFFFFu;
                cnt += __popcll(__ballot(key < cand));
              }
              if ((size_t)cnt <= k) ans = cand;
            }
          }
          return __uint_as_float(ans ^ ((ans >> 31) ? 0x80000000u : 0xFFFFFFFFu));
        };
        double min_active_cutoff = INFINITY, max_active_cutoff = INFINITY;
        if (need_max) max_active_cutoff = kth((size_t)a.max_active, count);
        if (max_active_cutoff < beam_cutoff) {
          adaptive_beam = max_active_cutoff - best_cost + a.beam_delta;
          weight_cutoff = max_active_cutoff;
        } else {
          if (count > (size_t)a.min_active) {
            if (a.min_active == 0) min_active_cutoff = best_cost;
            else if (need_min) min_active_cutoff = kth((size_t)a.min_active, count);
            else min_active_cutoff = -INFINITY;        // > min_active floats <= beam_cutoff: the (min_active)-th is <= beam_cutoff, value unused
          }
          if (min_active_cutoff > beam_cutoff) {
            adaptive_beam = min_active_cutoff - best_cost + a.beam_delta;
            weight_cutoff = min_active_cutoff;
          } else {
            adaptive_beam = beam;
            weight_cutoff = beam_cutoff;
          }
        }
      }
      K2C_STAMP(0);
      // ---- initial next_weight_cutoff from the best token's arcs (:175-188), evaluated by every lane alike ----
      double next_weight_cutoff = INFINITY;
      if (best_elem >= 0) {
        const int state = tks[best_elem];
        const double tcost = tkc[best_elem];
#pragma unroll
        for (int j = 0; j < ODEG; ++j) {
          const K2ChainArc r = oarc[state * ODEG + j];
          if (r.col < 0) continue;
          const float ac_cost = -1 * (a.acoustic_scale * sc[r.col]);
          const double new_weight = r.w + tcost + ac_cost;
          if (new_weight + adaptive_beam < next_weight_cutoff) next_weight_cutoff = new_weight + adaptive_beam;
        }
      }
      // ---- ProcessEmitting (:195-236), pass 1: one lane per token ----
      double carry = next_weight_cutoff;
      for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const bool have = i < n;
        const double tc = have ? tkc[i] : INFINITY;
        const int st = have ? tks[i] : 0;
        const bool act = have && tc < weight_cutoff;                    // :198
        double nwv[ODEG], tokc[ODEG], before[ODEG];
        int info[ODEG];
        bool val[ODEG];
        double run = INFINITY;
#pragma unroll
        for (int j = 0; j < ODEG; ++j) {
          const K2ChainArc r = oarc[st * ODEG + j];
          val[j] = act && r.col >= 0;
          const float ac_cost = -1 * (a.acoustic_scale * sc[val[j] ? r.col : 0]);
          nwv[j] = r.w + tc + ac_cost;                                  // :215 (pruning test)
          tokc[j] = (tc + r.w) + ac_cost;                               // Token constructor, faster-decoder.h:125
          info[j] = (int)r.dst | ((int)o_ord[st * ODEG + j] << 16);
          before[j] = run;
          run = __builtin_fmin(run, val[j] ? nwv[j] + adaptive_beam : (double)INFINITY);
        }
        const double inc = k2_scan_min_d(run);
        const double ex = k2_dpp_d<0x138, 0xf>((double)INFINITY, inc);  // wave_shr:1 -- the minimum over the lanes before this one
        const double cut0 = __builtin_fmin(carry, ex);
        carry = __builtin_fmin(carry, k2_lane63_d(inc));
#pragma unroll
        for (int j = 0; j < ODEG; ++j) {
          const bool surv = val[j] && nwv[j] < __builtin_fmin(cut0, before[j]);
          if (have) {
            const int f = i * ODEG + j;
            sl_cost[f] = tokc[j];
            sl_info[f] = info[j] | (surv ? (int)0x80000000 : 0);
            if (surv) {
              const int dst = info[j] & 0xffff;
              atomicMin(&st_key[dst], k2_d2key(tokc[j]));
              atomicMin(&st_first[dst], f);
            }
          }
        }
      }
      k2_lds_sync();
      K2C_STAMP(1);
      // pass 2: one lane per slot (lane order = insertion order): the first slot attaining each state's minimum (strict '<'
      // replacement keeps the earliest, :218-227) with its ordinal, and the new list in order of first insertion
      int nn = 0;
      const int F = n * ODEG;
      for (int base = 0; base < F; base += 64) {
        const int f = base + lane;
        const int inf_ = f < F ? sl_info[f] : 0;
        bool first = false; int dst = 0;
        if (inf_ < 0) {
          dst = inf_ & 0xffff;
          const unsigned long long key = st_key[dst];
          if (k2_d2key(sl_cost[f]) == key) atomicMin(&st_win[dst], (f << 8) | ((inf_ >> 16) & 0xff));
          first = st_first[dst] == f;
        }
        const unsigned long long fm = __ballot(first);
        if (first) {
          const int pos = nn + __popcll(fm & ((1ull << lane) - 1ull));
          nks[pos] = (uint16_t)dst;
          nkc[pos] = k2_key2d(st_key[dst]);
        }
        nn += __popcll(fm);
      }
      k2_lds_sync();
      K2C_STAMP(2);
      flush_row(bp + (int64_t)(frame + 1) * Sp);
      n = nn;
      { double* td = tkc; tkc = nkc; nkc = td; uint16_t* ti = tks; tks = nks; nks = ti; }
      k2_lds_sync();
      K2C_STAMP(3);
    }
    // ---- ReachedFinal (:346-353) + best final token (:373-382): first minimum in list order ----
    double bc = INFINITY; int bi = INT32_MAX; bool reached = false;
    for (int i = lane; i < n; i += 64) {
      const float fw = a.final_w[s0 + tks[i]];
      if (tkc[i] != INFINITY && fw != INFINITY) reached = true;
      const double c = tkc[i] + fw;
      if (c < bc && c != INFINITY) { bc = c; bi = i; }
    }
    for (int o = 32; o > 0; o >>= 1) {
      const double c2 = __shfl_xor(bc, o); const int i2 = __shfl_xor(bi, o);
      if (c2 < bc || (c2 == bc && i2 < bi)) { bc = c2; bi = i2; }
    }
    reached = __ballot(reached) != 0ull;
    best_state = (bi == INT32_MAX) ? -1 : tks[bi];
    if (reached) { status = (attempt ? KHG_ALIGN_RETRIED : 0); break; }
    if (attempt == 0 && a.retry_beam != 0.0f) { beam = a.retry_beam; k2_lds_sync(); continue; }  // decoder-wrappers.cc:55-67
    status = KHG_ALIGN_ERROR | (attempt ? KHG_ALIGN_RETRIED : 0);
    best_state = -1;
    break;
  }
  if (best_state < 0) {
    for (int t = lane; t < T; t += 64) a.ali_fb[f0 + t] = 0;
    if (lane == 0) { a.num_words[u] = 0; a.like[u] = 0.0f; a.status[u] = status | KHG_ALIGN_ERROR | KHG_ALIGN_FALLBACK; }
    return;
  }
  k2_global_sync();            // the back-pointer rows (all lanes' stores) before the trace-back reads them
  if (prof && lane == 0) { prof[2] = clock64(); prof[4] = prof_frames; prof[5] = pt[0]; prof[6] = pt[1]; prof[7] = pt[2]; }
#undef K2C_STAMP
  k2_lds_sync();               // (every lane is past its last read of the frame loop's tables)
  for (int s = lane; s <= S; s += 64) s_in_off[s] = (int32_t)(a.in_off[s0 + s] - in0);
  for (int i = lane; i < A; i += 64) s_src[i] = (uint16_t)a.in_src[in0 + i];
  k2_lds_sync();
  const int fst = k2_finish_wave(a, u, best_state, s_in_off, s_src, stage, lane);
  if (fst != KHG_ALIGN_DONE) {
    for (int t = lane; t < T; t += 64) a.ali_fb[f0 + t] = 0;
    if (lane == 0) a.status[u] = KHG_ALIGN_ERROR | status | KHG_ALIGN_FALLBACK;
  } else if (lane == 0) {
    a.status[u] = status | KHG_ALIGN_FALLBACK;
  }
  if (prof && lane == 0) prof[3] = clock64();
}
