// K3: sufficient-statistics accumulation from a resident alignment.
//
// Replaces (reference, /root/reference/):
//   scripts/gmm_acc_stats_ali.py:46-56          the per-frame Python loop
//   kaldi-hmm-gmm/csrc/mle-am-diag-gmm.cc:41-52 AccumAmDiagGmm::AccumulateForGmm
//   kaldi-hmm-gmm/csrc/mle-diag-gmm.cc:145-158  AccumulateFromDiag   (posteriors *= weight)
//   kaldi-hmm-gmm/csrc/mle-diag-gmm.cc:123-143  AccumulateFromPosteriors
//   kaldi-hmm-gmm/csrc/diag-gmm.cc:368-392      ComponentPosteriors (Softmax, eigen.cc:20-32)
//   kaldi-hmm-gmm/csrc/transition-model.h:183-189 Accumulate(prob=1, tid)
//
// Arithmetic kept from the reference: gamma*x and gamma*(x*x) are rounded to fp32 BEFORE being
// widened and added in fp64 (mle-diag-gmm.cc:135,138-140); occ adds double(gamma) (:132);
// total_log_like += float(ll*weight) (mle-am-diag-gmm.cc:49).  Only the fp64 summation ORDER
// differs (frames are grouped by pdf and chunks are merged with fp64 atomics).
//
// Pipeline: k3_count (histogram of frames per pdf + transition counts) -> host-free exclusive
// scan k3_scan -> k3_scatter (frame ids bucketed by pdf) -> k3_accumulate (grid = pdf x slice).

struct K3Args {
  const float* feats;          // [N][D]
  const int32_t* ali;          // [N] transition-ids, 0 = frame not aligned
  const int32_t* id2pdf;       // [num_tids+1]
  int32_t num_tids;
  int64_t N;
  int32_t P, D;
  // model, row-major as the reference stores it
  const int32_t* gauss_off;    // [P+1]
  const float* gconsts;
  const float* means_invvars;  // [sumG][D]
  const float* inv_vars;
  const float* nhalf_inv_vars; // -0.5 * inv_vars (exact), [sumG][D]
  // bucketing scratch
  int32_t* pdf_count;          // [P]
  int64_t* pdf_start;          // [P+1]
  int32_t* pdf_cursor;         // [P]
  int32_t* frame_ids;          // [N]
  unsigned long long* tid_count;  // [num_tids+1]
  // accumulators (fp64)
  double* occ; double* mean_acc; double* var_acc; double* trans_acc; double* scalars;  // scalars[0]=frames,[1]=loglike
  float weight;
  int32_t* err_flag;
  // wave form only: per-(pdf, slice) partial images when a pdf is cut into several blocks, per-pdf log-like partials
  double* part;                // [slots][NSUM + 1]: the images parked by the slices of a pdf that is cut into several blocks
  double* ll_part;             // [P]
  int32_t pdf0, npdf;          // the accumulate kernels of this launch cover pdfs pdf0 .. pdf0 + npdf - 1 (C1 overlaps K3 by pdf ranges)
  // work items of the accumulate kernels (k3_make_items): one block per item = slice y of ny of a pdf's bucket.  A pdf gets the form's
  // base number of slices, and more when its bucket is far above the average (silence in real transcripts: a hundred times the frames of
  // an average pdf -- one block per pdf would leave the whole chip waiting for three blocks).
  const struct K3Item* items;  // [item_off[P]]
  const int32_t* item_off;     // [P+1]
  // wave form with phase A on the fp16 matrix cores (k3_accumulate_wave<NB, true>): scale exponents that depend on the MODEL alone
  const int32_t* pa_ex;        // [80] per k = 2 d + kind: x' = x 2^ex, w' = w 2^(S - ex)
  int32_t pa_S;
  float pa_scale, pa_inv, pa_c1;   // 2^S, 2^-S, log2(e) 2^-S
  // k3_accumulate_wave16 (phase B on the fp16 matrix cores too): gamma' = gamma 2^SG, |weight| 2^SG in [2^13, 2^14)
  float pb_gscale;             // 2^SG
  int32_t pb_SG;
  // ... from the set's split feature records (k3_pack_x; the PLANES instantiation): [N + 1][K3_XREC] halves, record xrec_zero = N is zeros
  const _Float16* xrec;
  int32_t xrec_zero;
  // khg_acc_stats_post (khg_k3_post.hip.inc; the POST instantiations of k3_accumulate / k3_accumulate_mfma): `ali` holds the entries'
  // transition-ids, N is their number and the buckets (frame_ids) hold ENTRY numbers; entry e reads feature row e_row[e] and carries its
  // own weight e_w[e] where `weight` stands for an alignment
  const int32_t* e_row;        // [N]
  const float* e_w;            // [N]
};

struct K3Item { int32_t pdf, y, ny, slot; };      // slot: where slice y parks its image (wave forms, ny > 1), else -1

// block -> its work item; false: a block beyond the items of this launch's pdf range (the grid is an upper bound)
__device__ __forceinline__ bool k3_take_item(const K3Args& a, K3Item& it) {
  const int i = a.item_off[a.pdf0] + (int)blockIdx.x;
  if (i >= a.item_off[a.pdf0 + a.npdf]) return false;
  it = a.items[i];
  return true;
}

// Items from the bucket sizes: pdf p gets n_p = max(ny_base, ceil(frames_p / target_frames)) slices (<= K3_NYCAP).  One block; the
// pdfs in rounds of 1024 with a block-wide exclusive scan of (n_p, parked slices).  max_items / max_slots are what the host allocated
// (upper bounds from N, P, ny_base, target_frames alone); overflow raises the error flag and truncates.  Pdfs outside the launch's
// class (cls_lo < Gaussians <= cls_hi) and pdfs without frames get no item.
#define K3_NYCAP 4096
__global__ __launch_bounds__(1024) void k3_make_items(K3Args a, int ny_base, int target_frames, int max_items, int max_slots, K3Item* items, int32_t* item_off,
                                                      int cls_lo, int cls_hi) {
  __shared__ int s_n[1024], s_s[1024];
  __shared__ int s_run[2];
  const int tid = threadIdx.x;
  if (tid == 0) { s_run[0] = 0; s_run[1] = 0; }
  __syncthreads();
  for (int base = 0; base < a.P; base += 1024) {
    const int p = base + tid;
    int n = 0;
    if (p < a.P) {
      const int64_t nfr = a.pdf_start[p + 1] - a.pdf_start[p];
      const int64_t c = (nfr + target_frames - 1) / target_frames;
      n = (int)(c > ny_base ? (c > K3_NYCAP ? K3_NYCAP : c) : ny_base);
      const int Gp = a.gauss_off[p + 1] - a.gauss_off[p];              // the launch's class of pdfs (the form is chosen per pdf)
      if (Gp <= cls_lo || Gp > cls_hi || nfr == 0) n = 0;
    }
    const int sl = n > 1 ? n : 0;
    s_n[tid] = n; s_s[tid] = sl;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
      const int vn = tid >= o ? s_n[tid - o] : 0, vs = tid >= o ? s_s[tid - o] : 0;
      __syncthreads();
      s_n[tid] += vn; s_s[tid] += vs;
      __syncthreads();
    }
    const int i0 = s_run[0] + s_n[tid] - n, sl0 = s_run[1] + s_s[tid] - sl;
    if (p < a.P) {
      item_off[p] = i0 < max_items ? i0 : max_items;
      if (i0 + n > max_items || sl0 + sl > max_slots) atomicOr(a.err_flag, 8);
      else for (int y = 0; y < n; ++y) items[i0 + y] = K3Item{p, y, n, sl ? sl0 + y : -1};
    }
    __syncthreads();
    if (tid == 1023) { s_run[0] += s_n[1023]; s_run[1] += s_s[1023]; }
    __syncthreads();
  }
  if (tid == 0) item_off[a.P] = s_run[0] < max_items ? s_run[0] : max_items;
}

// Alignments come in runs (a state is held for several frames): each thread walks K3_SEG consecutive
// frames and issues one atomic per RUN of equal transition-id / pdf instead of one per frame.
#define K3_SEG 8
__global__ void k3_count(K3Args a) {
  const int64_t nseg = (a.N + K3_SEG - 1) / K3_SEG;
  int64_t sgi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; sgi < nseg; sgi += stride) {
    const int64_t i0 = sgi * K3_SEG;
    const int n = (int)min((int64_t)K3_SEG, a.N - i0);
    int ctid = -1, ntid = 0, cpdf = -1, npdf = 0;
    for (int k = 0; k < n; ++k) {
      const int tid = a.ali[i0 + k];
      if (tid < 1 || tid > a.num_tids) continue;
      const int pdf = a.id2pdf[tid];
      if (pdf < 0 || pdf >= a.P) { atomicOr(a.err_flag, 4); continue; }
      if (tid != ctid) {
        if (ntid) atomicAdd(&a.tid_count[ctid], (unsigned long long)ntid);
        ctid = tid; ntid = 0;
      }
      ++ntid;
      if (pdf != cpdf) {
        if (npdf) atomicAdd(&a.pdf_count[cpdf], npdf);
        cpdf = pdf; npdf = 0;
      }
      ++npdf;
    }
    if (ntid) atomicAdd(&a.tid_count[ctid], (unsigned long long)ntid);
    if (npdf) atomicAdd(&a.pdf_count[cpdf], npdf);
  }
}

// one workgroup: exclusive scan of pdf_count -> pdf_start; also folds the integer transition
// counts into the fp64 accumulator (exact: integer-valued sums)
__global__ void k3_scan(K3Args a) {
  __shared__ long long part[1024];
  const int tid = threadIdx.x, n = blockDim.x;
  const int per = (a.P + n - 1) / n;
  long long s = 0;
  for (int i = tid * per; i < (tid + 1) * per && i < a.P; ++i) s += a.pdf_count[i];
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    long long run = 0;
    for (int i = 0; i < n; ++i) { long long v = part[i]; part[i] = run; run += v; }
    a.pdf_start[a.P] = run;
  }
  __syncthreads();
  long long run = part[tid];
  for (int i = tid * per; i < (tid + 1) * per && i < a.P; ++i) {
    a.pdf_start[i] = run;
    a.pdf_cursor[i] = 0;
    run += a.pdf_count[i];
  }
  for (int i = tid; i <= a.num_tids; i += n) {
    unsigned long long c = a.tid_count[i];
    if (c) a.trans_acc[i] += (double)c * 1.0;  // transition-model.h:183-189 with prob = 1.0
  }
}

// Deterministic bucketing (default): key = pdf of the frame (P for a frame without a valid alignment), value = frame
// index; a stable radix sort of the pairs by key (rocPRIM through hipcub) leaves every pdf's frames in frame order, so
// the order in which K3 sums a pdf's frames -- and with it every bit of the statistics -- no longer depends on
// which thread won an atomic cursor.
// One pass over the alignment: the (pdf, frame) pairs AND the integer transition counts (one atomic per run of equal
// transition-ids, K3_SEG frames per thread), so the sort path needs no separate histogram kernel.
// Small transition models (<= K3_LDS_TIDS ids: a monophone system has a few hundred) count in a per-workgroup LDS histogram
// first: 30 M frames on ~300 counters in HBM serialise the global atomics (8.5 ms at 100 pdfs x 30 M frames, 1 ms this way).
// Larger transition models count straight into HBM, but through a small tagged cache in LDS (K3_HOT slots, first come first
// served): a transition-id that takes a large share of the frames (silence in real transcripts: 5 % of 30 M frames on six
// counters serialised the atomics, 1.6 ms) is seen early by every workgroup, owns its slot and is added to HBM once per workgroup.
#define K3_LDS_TIDS 4096
#define K3_HOT 1024
template <bool LDSHIST>
__global__ void k3_sort_keys(K3Args a, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  __shared__ unsigned int hist[LDSHIST ? K3_LDS_TIDS + 1 : K3_HOT];
  __shared__ int htag[LDSHIST ? 1 : K3_HOT];
  if constexpr (LDSHIST) {
    for (int i = threadIdx.x; i <= a.num_tids; i += blockDim.x) hist[i] = 0u;
  } else {
    for (int i = threadIdx.x; i < K3_HOT; i += blockDim.x) { hist[i] = 0u; htag[i] = 0; }
  }
  __syncthreads();
  // A wave takes 64 consecutive frames at a time -- coalesced reads of the alignment, coalesced writes of the pairs -- and counts a
  // RUN of equal transition-ids with one atomic: the run heads are a ballot, a head's run ends at the next set bit.  (One thread per
  // K3_SEG consecutive frames, the first form, made every load and store of a wave touch 64 cache lines: 0.74 ms for 360 MB.)
  const int lane = threadIdx.x & 63;
  const int64_t ngrp = (a.N + 63) / 64;
  const int64_t wstride = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; g < ngrp; g += wstride) {
    const int64_t i = g * 64 + lane;
    const bool in = i < a.N;
    const int tid = in ? a.ali[i] : 0;
    const bool valid = tid >= 1 && tid <= a.num_tids;
    int pdf = a.P;
    if (valid) {
      const int p = a.id2pdf[tid];
      if (p >= 0 && p < a.P) pdf = p; else atomicOr(a.err_flag, 4);
    }
    if (in) { keys[i] = (uint32_t)pdf; vals[i] = (uint32_t)i; }
    const int prev = __shfl_up(tid, 1);
    const bool head = lane == 0 || tid != prev;
    const unsigned long long heads = __ballot(head);
    if (head && valid) {
      const unsigned long long rest = lane == 63 ? 0ull : (heads >> (lane + 1));
      const int nrun = rest ? __ffsll((long long)rest) : 64 - lane;        // lanes past N carry tid 0: they end the last run
      if constexpr (LDSHIST) atomicAdd(&hist[tid], (unsigned int)nrun);
      else {
        const int slot = (int)(((unsigned)tid * 2654435761u) >> 22) & (K3_HOT - 1);
        int owner = htag[slot];
        if (owner == 0) { owner = atomicCAS(&htag[slot], 0, tid); if (owner == 0) owner = tid; }
        if (owner == tid) atomicAdd(&hist[slot], (unsigned int)nrun);
        else atomicAdd(&a.tid_count[tid], (unsigned long long)nrun);
      }
    }
  }
  __syncthreads();
  if constexpr (LDSHIST) {
    for (int i = threadIdx.x; i <= a.num_tids; i += blockDim.x) {
      const unsigned int c = hist[i];
      if (c) atomicAdd(&a.tid_count[i], (unsigned long long)c);
    }
  } else {
    for (int i = threadIdx.x; i < K3_HOT; i += blockDim.x) {
      const unsigned int c = hist[i];
      if (c) atomicAdd(&a.tid_count[htag[i]], (unsigned long long)c);
    }
  }
}

// ------------------------------------------------------------------------------------------
// The second pass of the split mode (khg_k3.hip: acc_stats_impl): the (pdf, frame) pairs of the FLAGGED utterances only -- those the
// exact DP left to the order-faithful decoders, whose alignments arrived after the first pass had started.  Utterances keep their
// order (positions from an exclusive sum of the flagged utterances' lengths), so the stable sort leaves every pdf's frames in frame
// order and the sums are as reproducible as the first pass's.
__global__ __launch_bounds__(1024) void k3_sub_scan(const int32_t* __restrict__ unc, const int64_t* __restrict__ frame_off, int n_utt, int64_t* __restrict__ sub_off) {
  __shared__ long long part[1024];
  const int tid = threadIdx.x;
  const int per = (n_utt + 1023) / 1024;
  const int u0 = tid * per, u1 = min(n_utt, u0 + per);
  long long s = 0;
  for (int u = u0; u < u1; ++u) if (unc[u]) s += frame_off[u + 1] - frame_off[u];
  part[tid] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const long long v = tid >= o ? part[tid - o] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  long long run = part[tid] - s;
  for (int u = u0; u < u1; ++u) { sub_off[u] = run; if (unc[u]) run += frame_off[u + 1] - frame_off[u]; }
  if (tid == 1023) sub_off[n_utt] = part[1023];
}
// one wave per flagged utterance, 64 consecutive frames at a time; transition-ids counted per run of equal ids (as k3_sort_keys)
__global__ __launch_bounds__(64) void k3_sub_keys(K3Args a, const int32_t* __restrict__ unc, const int64_t* __restrict__ frame_off,
                                                  const int64_t* __restrict__ sub_off, int n_utt, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const int lane = threadIdx.x;
  for (int u = blockIdx.x; u < n_utt; u += gridDim.x) {
    if (!unc[u]) continue;
    const int64_t f0 = frame_off[u], T = frame_off[u + 1] - f0, o0 = sub_off[u];
    for (int64_t b = 0; b < T; b += 64) {
      const int64_t t = b + lane;
      const bool in = t < T;
      const int tid = in ? a.ali[f0 + t] : 0;
      const bool valid = tid >= 1 && tid <= a.num_tids;
      int pdf = a.P;
      if (valid) {
        const int p = a.id2pdf[tid];
        if (p >= 0 && p < a.P) pdf = p; else atomicOr(a.err_flag, 4);
      }
      if (in && o0 + t < a.N) { keys[o0 + t] = (uint32_t)pdf; vals[o0 + t] = (uint32_t)(f0 + t); }
      const int prev = __shfl_up(tid, 1);
      const bool head = lane == 0 || tid != prev;
      const unsigned long long heads = __ballot(head);
      if (head && valid) {
        const unsigned long long rest = lane == 63 ? 0ull : (heads >> (lane + 1));
        const int nrun = rest ? __ffsll((long long)rest) : 64 - lane;        // lanes past T carry tid 0: they end the last run
        atomicAdd(&a.tid_count[tid], (unsigned long long)nrun);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// Bucketing without a library sort (option k3_bucket = 2, models of <= K3_CS_MAXP pdfs): a stable COUNTING sort of the frames by
// pdf, four small kernels.  Built in round 3 to take the one library call (rocPRIM's radix sort) off the path; measured at the bench
// size: hist 0.27 + scan 0.06 + starts 0.02 + place 0.85 = 1.2 ms against 0.27 (key pass) + 0.45 (radix sort) + 0.01: the placing
// pass -- per 64-frame group two LDS round trips for the run heads, 14 % of the groups through the pdf-by-pdf loop on a hash clash,
// scattered 14-byte stores -- does not beat the onesweep sort, so the radix sort stays the default.  The alignment is cut into blocks of CB consecutive frames.
//   k3_cs_hist   block b counts its frames per pdf in LDS (and the transition-ids, as k3_sort_keys) -> hist[b][0..P]
//   k3_cs_scan   per pdf: exclusive running sum over the blocks (in place), the pdf's total -> tot[p];
//   k3_cs_starts one workgroup: exclusive scan of the totals -> pdf_start[0..P] (+ the transition counts into the accumulator)
//   k3_cs_place  block b again, its waves on consecutive sub-ranges: per-wave counts in LDS -> each wave's first position
//                per pdf = pdf_start[p] + hist[b][p] + the earlier waves' counts -> the wave walks its 64-frame groups IN ORDER and
//                gives every frame the next position of its pdf (rank among the group's equal keys by ballot).
// Every frame's position is a pure function of the alignment: exactly the order a stable sort by pdf produces (frames of a pdf in
// frame order), so the statistics are bit-identical to the rocPRIM path's (tests/test_gpu_parity.py).
#define K3_CS_MAXP 16383

struct K3CsArgs {
  int32_t* hist;          // [nblk][P+1], overwritten by its exclusive running sum over blocks
  int64_t* tot;           // [P+1]
  int32_t CB;             // frames per block (multiple of 64 * waves)
  int32_t nblk;
};

__device__ __forceinline__ int k3_cs_pdf_of(const K3Args& a, int tid) {        // P for a frame without a valid alignment
  int pdf = a.P;
  if (tid >= 1 && tid <= a.num_tids) {
    const int p = a.id2pdf[tid];
    if (p >= 0 && p < a.P) pdf = p; else atomicOr(a.err_flag, 4);
  }
  return pdf;
}
__device__ __forceinline__ int k3_cs_key(const K3Args& a, int64_t i, bool in, int* tid_out) {
  const int tid = in ? a.ali[i] : 0;
  *tid_out = tid;
  return k3_cs_pdf_of(a, tid);
}
// The frames [w0, w1) of one wave, 64 at a time and IN ORDER, with the alignment of group g + 2 and the pdf lookup of group g + 1
// in flight while group g is processed (a lone wave per SIMD would otherwise stand on two dependent loads per group).
template <class F>
__device__ __forceinline__ void k3_cs_walk(const K3Args& a, int64_t w0, int64_t w1, int lane, F&& body) {
  auto tid_at = [&](int64_t g0) { const int64_t i = g0 + lane; return (g0 < w1 && i < w1) ? a.ali[i] : 0; };
  int tid0 = tid_at(w0), tid1 = tid_at(w0 + 64);
  int pdf0 = k3_cs_pdf_of(a, tid0);
  for (int64_t g0 = w0; g0 < w1; g0 += 64) {
    const int tid2 = tid_at(g0 + 128);
    const int pdf1 = k3_cs_pdf_of(a, tid1);
    body(g0, tid0, pdf0);
    tid0 = tid1; tid1 = tid2; pdf0 = pdf1;
  }
}

template <bool LDSHIST>
__global__ void k3_cs_hist(K3Args a, K3CsArgs c) {
  extern __shared__ unsigned int k3cs_lds[];          // [P+1] pdf counts (+ [num_tids+1] transition counts, LDSHIST)
  unsigned int* ph = k3cs_lds;
  unsigned int* th = k3cs_lds + a.P + 1;
  for (int i = threadIdx.x; i <= a.P; i += blockDim.x) ph[i] = 0u;
  if constexpr (LDSHIST) for (int i = threadIdx.x; i <= a.num_tids; i += blockDim.x) th[i] = 0u;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t b0 = (int64_t)blockIdx.x * c.CB, b1 = min(a.N, b0 + c.CB);
  const int64_t perw = (int64_t)c.CB / (blockDim.x >> 6);
  const int64_t hw0 = min(b1, b0 + (int64_t)(threadIdx.x >> 6) * perw), hw1 = min(b1, hw0 + perw);
  k3_cs_walk(a, hw0, hw1, lane, [&](int64_t g0, int tid, int pdf) {
    const int64_t i = g0 + lane;
    const bool in = i < hw1;
    const bool valid = tid >= 1 && tid <= a.num_tids;
    // runs of equal transition-ids (and with them of equal pdfs): one atomic per run and counter
    const int prev = __shfl_up(tid, 1);
    const bool head = lane == 0 || tid != prev;
    const unsigned long long heads = __ballot(head);
    if (head && in) {
      const unsigned long long rest = lane == 63 ? 0ull : (heads >> (lane + 1));
      int nrun = rest ? __ffsll((long long)rest) : 64 - lane;
      nrun = (int)min((int64_t)nrun, hw1 - i);
      atomicAdd(&ph[pdf], (unsigned int)nrun);
      if (valid) {
        if constexpr (LDSHIST) atomicAdd(&th[tid], (unsigned int)nrun);
        else atomicAdd(&a.tid_count[tid], (unsigned long long)nrun);
      }
    }
  });
  __syncthreads();
  int32_t* row = c.hist + (int64_t)blockIdx.x * (a.P + 1);
  for (int i = threadIdx.x; i <= a.P; i += blockDim.x) row[i] = (int32_t)ph[i];
  if constexpr (LDSHIST)
    for (int i = threadIdx.x; i <= a.num_tids; i += blockDim.x) {
      const unsigned int v = th[i];
      if (v) atomicAdd(&a.tid_count[i], (unsigned long long)v);
    }
}

__global__ void k3_cs_scan(K3Args a, K3CsArgs c) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p > a.P) return;
  const int64_t P1 = a.P + 1;
  int64_t run = 0;
  constexpr int U = 16;             // sixteen independent loads in flight per thread: the loop is latency bound otherwise
  int b = 0;
  for (; b + U <= c.nblk; b += U) {
    int32_t v[U];
#pragma unroll
    for (int j = 0; j < U; ++j) v[j] = c.hist[(int64_t)(b + j) * P1 + p];
#pragma unroll
    for (int j = 0; j < U; ++j) { c.hist[(int64_t)(b + j) * P1 + p] = (int32_t)run; run += v[j]; }   // < 2^31: N < INT_MAX on this path
  }
  for (; b < c.nblk; ++b) {
    const int32_t v = c.hist[(int64_t)b * P1 + p];
    c.hist[(int64_t)b * P1 + p] = (int32_t)run;
    run += v;
  }
  c.tot[p] = run;
}

__global__ __launch_bounds__(1024) void k3_cs_starts(K3Args a, K3CsArgs c) {
  __shared__ int64_t part[1024];
  const int tid = threadIdx.x, n = a.P + 1;
  const int per = (n + 1023) / 1024;
  const int lo = min(n, tid * per), hi = min(n, lo + per);
  int64_t s = 0;
  for (int p = lo; p < hi; ++p) s += c.tot[p];
  part[tid] = s;
  __syncthreads();
  if (tid == 0) { int64_t r = 0; for (int i = 0; i < 1024; ++i) { const int64_t v = part[i]; part[i] = r; r += v; } }
  __syncthreads();
  int64_t r = part[tid];
  for (int p = lo; p < hi; ++p) { a.pdf_start[p] = r; r += c.tot[p]; }      // pdf_start[P] = number of aligned frames
  for (int i = tid; i <= a.num_tids; i += 1024) {
    const unsigned long long cnt = a.tid_count[i];
    if (cnt) a.trans_acc[i] += (double)cnt * 1.0;    // transition-model.h:183-189 with prob = 1.0
  }
}

__global__ void k3_cs_place(K3Args a, K3CsArgs c) {
  extern __shared__ unsigned int k3cs_lds[];          // [waves][P+1]
  const int nw = blockDim.x >> 6, lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int P1 = a.P + 1;
  for (int i = threadIdx.x; i < nw * P1; i += blockDim.x) k3cs_lds[i] = 0u;
  __syncthreads();
  const int64_t b0 = (int64_t)blockIdx.x * c.CB, b1 = min(a.N, b0 + c.CB);
  const int64_t per = (int64_t)(c.CB / nw);                          // a multiple of 64
  const int64_t w0 = min(b1, b0 + wave * per), w1 = min(b1, w0 + per);
  unsigned int* mine = k3cs_lds + wave * P1;
  // (1) this wave's counts per pdf
  k3_cs_walk(a, w0, w1, lane, [&](int64_t g0, int, int pdf) {
    const int64_t i = g0 + lane;
    const bool in = i < w1;
    const int prev = __shfl_up(pdf, 1);
    const bool head = lane == 0 || pdf != prev;
    const unsigned long long heads = __ballot(head);
    if (head && in) {
      const unsigned long long rest = lane == 63 ? 0ull : (heads >> (lane + 1));
      int nrun = rest ? __ffsll((long long)rest) : 64 - lane;
      nrun = (int)min((int64_t)nrun, w1 - i);
      atomicAdd(&mine[pdf], (unsigned int)nrun);
    }
  });
  __syncthreads();
  // (2) counts -> first position of every wave per pdf
  const int32_t* row = c.hist + (int64_t)blockIdx.x * P1;
  for (int p = threadIdx.x; p < P1; p += blockDim.x) {
    unsigned int r = (unsigned int)(a.pdf_start[min(p, a.P)] + row[p]);      // key P (not aligned) is never placed
    for (int w = 0; w < nw; ++w) { const unsigned int v = k3cs_lds[w * P1 + p]; k3cs_lds[w * P1 + p] = r; r += v; }
  }
  __syncthreads();
  // (3) place, group by group in frame order.  The frames of a group come in runs of one pdf; when no pdf heads two runs of the
  // group (checked through a stamped 1024-slot hash table: a collision only sends the group to the general loop) every run takes
  // its pdf's next positions at once: its head reads the counter, the run's lanes follow it, the head adds the run length.
  // Otherwise pdf by pdf, the frames of one pdf ranked by ballot.
  unsigned int* tag = k3cs_lds + nw * P1 + wave * 1024;
  for (int i = lane; i < 1024; i += 64) tag[i] = 0xffffffffu;
  unsigned int stamp = 0;
  k3_cs_walk(a, w0, w1, lane, [&](int64_t g0, int, int pdf) {
    const int64_t i = g0 + lane;
    const bool in = i < w1;
    const bool live = in && pdf < a.P;
    const int prev = __shfl_up(pdf, 1);
    const bool head = lane == 0 || pdf != prev;
    const unsigned long long heads = __ballot(head);
    const bool lhead = head && live;
    const unsigned int mark = (stamp << 6) | (unsigned int)lane;
    const unsigned int slot = ((unsigned int)pdf * 2654435761u) >> 22;
    if (lhead) tag[slot] = mark;
    __builtin_amdgcn_wave_barrier();
    const bool clash = lhead && tag[slot] != mark;
    if (!__ballot(clash)) {
      const unsigned int base = lhead ? mine[pdf] : 0u;
      const unsigned long long below = heads & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));
      const int hl = 63 - __clzll((long long)below);                  // the head of this lane's run (lane 0 is always a head)
      const unsigned int hb = __shfl(base, hl);
      if (live) a.frame_ids[hb + (unsigned int)(lane - hl)] = (int32_t)i;
      if (lhead) {
        const unsigned long long rest = lane == 63 ? 0ull : (heads >> (lane + 1));
        int nrun = rest ? __ffsll((long long)rest) : 64 - lane;
        nrun = (int)min((int64_t)nrun, w1 - i);
        mine[pdf] = base + (unsigned int)nrun;
      }
      __builtin_amdgcn_wave_barrier();
      ++stamp;
      return;
    }
    ++stamp;
    unsigned long long todo = __ballot(live);
    while (todo) {
      const int l = __ffsll((long long)todo) - 1;
      const int k = __shfl(pdf, l);
      const unsigned long long same = __ballot(pdf == k) & todo;
      const unsigned int base = mine[k];
      if ((same >> lane) & 1ull) a.frame_ids[base + __popcll(same & ((1ull << lane) - 1ull))] = (int32_t)i;
      __builtin_amdgcn_wave_barrier();
      if (lane == l) mine[k] = base + (unsigned int)__popcll(same);
      __builtin_amdgcn_wave_barrier();
      todo &= ~same;
    }
  });
}

// After the sort: pdf_start[p] = first position of key p (binary search per pdf; pdf_start[P] = number of aligned
// frames), and the integer transition counts folded into the fp64 accumulator (exact).
__global__ void k3_bounds(K3Args a, const uint32_t* __restrict__ sorted_keys) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p <= a.P; p += stride) {
    int64_t lo = 0, hi = a.N;                    // first i with sorted_keys[i] >= p
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (sorted_keys[mid] < (uint32_t)p) lo = mid + 1; else hi = mid;
    }
    a.pdf_start[p] = lo;
  }
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= a.num_tids; i += stride) {
    const unsigned long long c = a.tid_count[i];
    if (c) a.trans_acc[i] += (double)c * 1.0;    // transition-model.h:183-189 with prob = 1.0
  }
}

__global__ void k3_scatter(K3Args a) {
  const int64_t nseg = (a.N + K3_SEG - 1) / K3_SEG;
  int64_t sgi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; sgi < nseg; sgi += stride) {
    const int64_t i0 = sgi * K3_SEG;
    const int n = (int)min((int64_t)K3_SEG, a.N - i0);
    int pdfs[K3_SEG];
#pragma unroll
    for (int k = 0; k < K3_SEG; ++k) {
      pdfs[k] = -1;
      if (k < n) {
        const int tid = a.ali[i0 + k];
        if (tid >= 1 && tid <= a.num_tids) {
          const int pdf = a.id2pdf[tid];
          if (pdf >= 0 && pdf < a.P) pdfs[k] = pdf;
        }
      }
    }
    // one cursor bump per run of equal pdfs, then the run's frame ids go out consecutively
    int k = 0;
    while (k < n) {
      const int pdf = pdfs[k];
      int e = k + 1;
      while (e < n && pdfs[e] == pdf) ++e;
      if (pdf >= 0) {
        const int pos = atomicAdd(&a.pdf_cursor[pdf], e - k);
        int32_t* dst = a.frame_ids + a.pdf_start[pdf] + pos;
        for (int j = k; j < e; ++j) dst[j - k] = (int32_t)(i0 + j);
      }
      k = e;
    }
  }
}

// frames of one pdf are processed in chunks of K3_CHUNK; within a chunk:
//  A. each wave takes frames round-robin; lane g evaluates Gaussian g's log-like with the same
//     fmaf chain as K1, then a wave-level softmax gives gamma[f][g]  (kept in LDS)
//  B. each thread owns a strip of K3_DS feature dims of one Gaussian and adds
//     fl32(gamma*x), fl32(gamma*x^2) into fp64 registers over the chunk's frames, then flushes
//     with fp64 atomics.
#define K3_CHUNK 64
#define K3_DS 10

template <int KQ, bool POST = false>
__global__ __launch_bounds__(256) void k3_accumulate(K3Args a) {
  extern __shared__ __attribute__((aligned(16))) float k3s[];
  // padded feature-row pitch in LDS (zero filled beyond D); KQ = 0 is the any-dimension form (D > 80): odd runtime pitch,
  // phase A reads its frame's row from LDS instead of holding [x | x^2] in registers
  constexpr int XPC = KQ > 0 ? 4 * KQ : 4;
  const int XP = KQ > 0 ? XPC : (a.D | 1);
  K3Item it;
  if (!k3_take_item(a, it)) return;
  const int pdf = it.pdf;
  const int64_t beg = a.pdf_start[pdf];
  const int nfr = (int)(a.pdf_start[pdf + 1] - beg);
  if (nfr == 0) return;
  const int D = a.D;
  const int g0 = a.gauss_off[pdf], G = a.gauss_off[pdf + 1] - g0;
  const int GP = G | 1;                   // odd pitch: gam[f][g] is conflict free both ways
  float* xs = k3s;                        // [K3_CHUNK][XP]
  float* gam = xs + K3_CHUNK * XP;        // [K3_CHUNK][GP]
  float* red = gam + K3_CHUNK * GP;       // [4][K3_CHUNK] cross-wave max / sum
  [[maybe_unused]] float* wts = red + 4 * K3_CHUNK;   // POST: [K3_CHUNK] the chunk's entries' weights
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nchunk = (nfr + K3_CHUNK - 1) / K3_CHUNK;
  const int SG = (D + K3_DS - 1) / K3_DS;   // strips per Gaussian
  const int nstrip = G * SG;
  const bool persist = nstrip <= 256;       // one strip per thread: keep fp64 sums in registers
  const int Gq = (G + 3) >> 2;              // Gaussians per wave in phase A
  const int gbeg = wave * Gq, gend = min(G, gbeg + Gq);
  double tot_ll = 0.0;
  [[maybe_unused]] double tot_w = 0.0;
  double am[K3_DS], av[K3_DS], ao = 0.0;
#pragma unroll
  for (int k = 0; k < K3_DS; ++k) { am[k] = 0.0; av[k] = 0.0; }

  auto flush = [&](int st) {
    const int g = st / SG, d0 = (st - g * SG) * K3_DS;
    const int nd = min(K3_DS, D - d0);
    double* mo = a.mean_acc + (int64_t)(g0 + g) * D + d0;
    double* vo = a.var_acc + (int64_t)(g0 + g) * D + d0;
#pragma unroll
    for (int k = 0; k < K3_DS; ++k)
      if (k < nd) { atomicAdd(mo + k, am[k]); atomicAdd(vo + k, av[k]); am[k] = 0.0; av[k] = 0.0; }
    if (d0 == 0) { atomicAdd(a.occ + g0 + g, ao); ao = 0.0; }
  };

  for (int c = it.y; c < nchunk; c += it.ny) {
    const int cf = min(K3_CHUNK, nfr - c * K3_CHUNK);
    __syncthreads();
    // stage the chunk's feature rows (gathered by frame id), zero padded to XP
    for (int i = tid; i < K3_CHUNK * XP; i += 256) {
      int f = i / XP, d = i - f * XP;
      // always-valid addresses (last frame of the chunk, last dim), zero fill by select: the loads of the loop issue back to back
      int row = a.frame_ids[beg + c * K3_CHUNK + min(f, cf - 1)];
      if constexpr (POST) row = a.e_row[row];
      const float raw = a.feats[(int64_t)row * D + min(d, D - 1)];
      xs[i] = (f < cf && d < D) ? raw : 0.0f;
    }
    if constexpr (POST) { if (tid < K3_CHUNK) wts[tid] = tid < cf ? a.e_w[a.frame_ids[beg + c * K3_CHUNK + tid]] : 0.0f; }
    __syncthreads();
    // ---- phase A: lane <-> frame ([x | x^2] in registers), wave <-> a quarter of the pdf's
    // Gaussians whose parameters are wave-uniform (scalar loads); no cross-lane traffic ----
    {
      float xr[XPC], x2[XPC];
      if constexpr (KQ > 0) {
        const f32x4* x4 = reinterpret_cast<const f32x4*>(xs + lane * XP);
#pragma unroll
        for (int q = 0; q < KQ; ++q) {
          const f32x4 v = x4[q];
#pragma unroll
          for (int i = 0; i < 4; ++i) { xr[4 * q + i] = v[i]; x2[4 * q + i] = v[i] * v[i]; }
        }
      }
      float m = -INFINITY;
      for (int g = gbeg; g < gend; ++g) {
        const float* mi = a.means_invvars + (int64_t)(g0 + g) * D;
        const float* nh = a.nhalf_inv_vars + (int64_t)(g0 + g) * D;
        float s = a.gconsts[g0 + g];
        if constexpr (KQ > 0) {
#pragma unroll
          for (int d = 0; d < XPC; ++d) {
            if (d < D) {
              s = fmaf(mi[d], xr[d], s);   // same chain as K1's MFMA (k = 2d, 2d+1)
              s = fmaf(nh[d], x2[d], s);
            }
          }
        } else {
          const float* xrow = xs + lane * XP;
          for (int d = 0; d < D; ++d) {
            const float xv = xrow[d];
            s = fmaf(mi[d], xv, s);
            s = fmaf(nh[d], xv * xv, s);
          }
        }
        gam[lane * GP + g] = s;
        m = fmaxf(m, s);
      }
      red[wave * K3_CHUNK + lane] = m;
      __syncthreads();
      m = fmaxf(fmaxf(red[lane], red[K3_CHUNK + lane]), fmaxf(red[2 * K3_CHUNK + lane], red[3 * K3_CHUNK + lane]));
      __syncthreads();
      float ssum = 0.0f;
      for (int g = gbeg; g < gend; ++g) {
        float e = __expf(gam[lane * GP + g] - m);   // Softmax: (v - max).exp()  (eigen.cc:23)
        gam[lane * GP + g] = e;
        ssum += e;
      }
      red[wave * K3_CHUNK + lane] = ssum;
      __syncthreads();
      ssum = (red[lane] + red[K3_CHUNK + lane]) + (red[2 * K3_CHUNK + lane] + red[3 * K3_CHUNK + lane]);
      const float ll = __logf(ssum) + m;            // eigen.cc:28
      float wf = a.weight;                          // POST: the entry's own weight
      if constexpr (POST) wf = wts[lane];
      if (lane < cf) {
        if (!(fabsf(ll) <= 3.0e38f)) atomicOr(a.err_flag, 1);  // diag-gmm.cc:385-387
        if (wave == 0) tot_ll += (double)(ll * wf);            // mle-am-diag-gmm.cc:49
        if constexpr (POST) { if (wave == 0) tot_w += (double)wf; }   // :50
      }
      for (int g = gbeg; g < gend; ++g) {
        float p = gam[lane * GP + g] / ssum;        // eigen.cc:31
        gam[lane * GP + g] = lane < cf ? p * wf : 0.0f;        // mle-diag-gmm.cc:153
      }
    }
    __syncthreads();
    // ---- phase B: thread <-> (Gaussian, strip of K3_DS dims); fp32 products, fp64 sums ----
    for (int st = tid; st < nstrip; st += 256) {
      const int g = st / SG, d0 = (st - g * SG) * K3_DS;
      const int nd = min(K3_DS, D - d0);
      for (int f = 0; f < cf; ++f) {
        const float p = gam[f * GP + g];
        const float* x = xs + f * XP + d0;
        if (d0 == 0) ao += (double)p;            // mle-diag-gmm.cc:132
#pragma unroll
        for (int k = 0; k < K3_DS; ++k) {
          if (k < nd) {
            float xv = x[k];
            float pm = p * xv;                    // :135  fp32 product, then widened
            float xx = xv * xv;
            float pv = p * xx;                    // :138-140
            am[k] += (double)pm;
            av[k] += (double)pv;
          }
        }
      }
      if (!persist) flush(st);
    }
  }
  if (persist && tid < nstrip) flush(tid);
  // wave 0's lanes hold per-frame partial sums of float(ll*weight): reduce and publish
  if (wave == 0) {
    for (int o = 32; o > 0; o >>= 1) tot_ll += __shfl_xor(tot_ll, o);
    if (lane == 0 && tot_ll != 0.0) atomicAdd(&a.scalars[1], tot_ll);
  }
  if constexpr (POST) {
    // the sum of the weights of this block's entries, where an alignment has frames x weight
    if (wave == 0) {
      for (int o = 32; o > 0; o >>= 1) tot_w += __shfl_xor(tot_w, o);
      if (lane == 0 && tot_w != 0.0) atomicAdd(&a.scalars[0], tot_w);
    }
  } else {
    if (tid == 0 && it.y == 0) atomicAdd(&a.scalars[0], (double)nfr * (double)a.weight);  // :50
  }
}

// ------------------------------------------------------------------------------------------
// MFMA form of k3_accumulate (pdfs with <= 64*NBW Gaussians): both contractions on the matrix pipes.
//   phase A  ll[f][g]  = gconst[g] + [x | x²][f]·W[g]        v_mfma_f32_16x16x4_f32, A = frames, B = Gaussians:
//            the same k-ordered fmaf chain as K1, so ll is bit-identical to K1's per-Gaussian value;
//            C puts the Gaussian on lane&15 and frames 4*(lane>>4)+reg in the registers,
//   phase B  acc[g][d'] += sum_f gamma[f][g]·[x | x²][f][d']   v_mfma_f64_16x16x4_f64, A = gamma^T, B = X:
//            MFMA step s takes frame 4*(lane>>4)+s from every lane quarter, i.e. register s of phase A's
//            result IS the A operand -- no transpose, no LDS round trip for gamma.
// A wave owns 16-Gaussian blocks (w, w+4, ...) for all 64 frames of a chunk, so its fp64
// accumulators (16 Gaussians x 2*XP columns) live in registers for the whole block and no cross-wave
// sum is needed.  The softmax over the pdf's Gaussians combines the waves through LDS.
// Products gamma*x are exact in fp64 here; the reference rounds each product to fp32 before
// widening (mle-diag-gmm.cc:135,138-140), a relative difference <= 2^-24 per term.
typedef double f64x4 __attribute__((ext_vector_type(4)));

// max / sum over the 16 lanes of a DPP row: the row rotation is applied to the first operand of the arithmetic
// instruction itself (four instructions per reduction; the inputs are never NaN).  The s_nops are the
// VALU-write -> DPP-read wait states.
__device__ __forceinline__ float k3_row_max(float v) {
  asm volatile("s_nop 1\n\t"
               "v_max_f32_dpp %0, %0, %0 row_ror:8 row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"
               "v_max_f32_dpp %0, %0, %0 row_ror:4 row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"
               "v_max_f32_dpp %0, %0, %0 row_ror:2 row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"
               "v_max_f32_dpp %0, %0, %0 row_ror:1 row_mask:0xf bank_mask:0xf\n\ts_nop 1"
               : "+v"(v));
  return v;
}
__device__ __forceinline__ float k3_row_sum(float v) {
  asm volatile("s_nop 1\n\t"
               "v_add_f32_dpp %0, %0, %0 row_ror:8 row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"
               "v_add_f32_dpp %0, %0, %0 row_ror:4 row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"
               "v_add_f32_dpp %0, %0, %0 row_ror:2 row_mask:0xf bank_mask:0xf\n\ts_nop 1\n\t"
               "v_add_f32_dpp %0, %0, %0 row_ror:1 row_mask:0xf bank_mask:0xf\n\ts_nop 1"
               : "+v"(v));
  return v;
}

// workgroup barrier that orders LDS traffic only: __syncthreads() also drains vmcnt, i.e. it would wait for the NEXT chunk's feature
// gather (two dependent HBM loads, requested a chunk ahead precisely so that nobody waits for them) at the first barrier behind it
__device__ __forceinline__ void k3_block_sync() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

template <int KQ, int NBW, bool POST = false>
__global__ __launch_bounds__(256) void k3_accumulate_mfma(K3Args a) {
  extern __shared__ __attribute__((aligned(16))) float k3s[];
  constexpr int XP = 4 * KQ;       // padded feature-row pitch (zero filled beyond D)
  constexpr int KH = 2 * KQ;       // phase-A MFMA steps
  constexpr int NDB = KQ / 2;      // 16-column blocks of [x | x²] (2*XP columns)
  K3Item it;
  if (!k3_take_item(a, it)) return;
  const int pdf = it.pdf;
  const int64_t beg = a.pdf_start[pdf];
  const int nfr = (int)(a.pdf_start[pdf + 1] - beg);
  if (nfr == 0) return;
  const int D = a.D;
  const int g0 = a.gauss_off[pdf], G = a.gauss_off[pdf + 1] - g0;
  // LDS: the chunk's features as four planes [q][64 frames][KH]: q = 0/1: x at even/odd d, q = 2/3: x² at
  // even/odd d (element s <-> d = 2s + (q&1)) -- exactly what lane quarter q feeds the fp32 MFMA, so the
  // phase-A operands are plain 16-byte LDS reads (row pitch KH = 5 or 10 slots... KH floats)
  float* xq = k3s;                          // [4][64][KH]
  float* red = xq + 4 * K3_CHUNK * KH;      // [4][64] per-wave per-frame max / sum
  float* fin = red + 4 * K3_CHUNK;          // [64] combined value per frame
  [[maybe_unused]] float* wts = fin + K3_CHUNK;       // POST: [64] the chunk's entries' weights
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j16 = lane & 15, q = lane >> 4;
  const int nchunk = (nfr + K3_CHUNK - 1) / K3_CHUNK;

  // ---- per block: this wave's Gaussians (block b = wave + 4*k), W planes as phase-A B operands ----
  float wq[NBW][KH], gcv[NBW];
  bool gvalid[NBW];
#pragma unroll
  for (int k = 0; k < NBW; ++k) {
    const int g = 16 * (wave + 4 * k) + j16;
    gvalid[k] = g < G;
    const float* mi = a.means_invvars + (int64_t)(g0 + (gvalid[k] ? g : 0)) * D;
    const float* nh = a.nhalf_inv_vars + (int64_t)(g0 + (gvalid[k] ? g : 0)) * D;
    gcv[k] = gvalid[k] ? a.gconsts[g0 + g] : -INFINITY;
#pragma unroll
    for (int s = 0; s < KH; ++s) {
      const int d = 2 * s + (q & 1);
      wq[k][s] = (gvalid[k] && d < D) ? ((q & 2) ? nh[d] : mi[d]) : 0.0f;
    }
  }
  f64x4 acc[NBW][NDB];
  double occ[NBW];
#pragma unroll
  for (int k = 0; k < NBW; ++k) {
    occ[k] = 0.0;
#pragma unroll
    for (int db = 0; db < NDB; ++db) acc[k][db] = f64x4{0, 0, 0, 0};
  }
  double tot_ll = 0.0;
  [[maybe_unused]] double tot_w = 0.0;

  // The NEXT chunk's features are requested into registers as soon as this chunk's are parked in LDS (always-valid addresses:
  // last frame of the chunk, last dim; zero fill by select at the staging), so the two dependent HBM loads of the gather
  // (frame id, then row) are covered by this chunk's two MFMA phases instead of standing at the head of every chunk.
  constexpr int NI = K3_CHUNK * XP / 256;
  constexpr bool PF = NBW < 4;           // four blocks per wave (193..256 Gaussians) leave no registers for the prefetch: it would spill
  float pre[NI];
  [[maybe_unused]] float prew = 0.0f;    // POST: the weight of entry `lane` of the requested chunk
  auto request = [&](int c) {
    const int cfn = min(K3_CHUNK, nfr - c * K3_CHUNK);
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int i = tid + 256 * j, f = i / XP, d = i - f * XP;
      int row = a.frame_ids[beg + c * K3_CHUNK + min(f, cfn - 1)];
      if constexpr (POST) row = a.e_row[row];
      pre[j] = a.feats[(int64_t)row * D + min(d, D - 1)];
    }
    if constexpr (POST) prew = a.e_w[a.frame_ids[beg + c * K3_CHUNK + min(lane, cfn - 1)]];
  };
  if (PF && it.y < nchunk) request(it.y);
  for (int c = it.y; c < nchunk; c += it.ny) {
    const int cf = min(K3_CHUNK, nfr - c * K3_CHUNK);
    k3_block_sync();
    if (!PF) request(c);
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int i = tid + 256 * j, f = i / XP, d = i - f * XP;
      const float v = (f < cf && d < D) ? pre[j] : 0.0f;
      float* dst = xq + ((d & 1) * K3_CHUNK + f) * KH + (d >> 1);
      dst[0] = v;
      dst[2 * K3_CHUNK * KH] = v * v;
    }
    if constexpr (POST) { if (tid < K3_CHUNK) wts[tid] = tid < cf ? prew : 0.0f; }
    if (PF && c + it.ny < nchunk) request(c + it.ny);
    k3_block_sync();
    // ---- phase A: ll[k][ft][reg] for Gaussian 16*(wave+4k)+j16, frame 16*ft + 4*q + reg.  Operands: lane (frame 16*ft + j16,
    // quarter q) holds xx_q[f][s]; two frame tiles at a time (2 x NBW independent accumulation chains keep the pipe full, and
    // the operand block is 2*KH registers instead of 4*KH: room for the prefetched next chunk) ----
    f32x4 ll[NBW][4];
#pragma unroll
    for (int k = 0; k < NBW; ++k)
#pragma unroll
      for (int ft = 0; ft < 4; ++ft) ll[k][ft] = f32x4{gcv[k], gcv[k], gcv[k], gcv[k]};
#pragma unroll
    for (int fp = 0; fp < 4; fp += 2) {
      float xa[2][KH];
#pragma unroll
      for (int f2 = 0; f2 < 2; ++f2) {
        const f32x4* x4 = reinterpret_cast<const f32x4*>(xq + (q * K3_CHUNK + 16 * (fp + f2) + j16) * KH);
#pragma unroll
        for (int jj = 0; jj < KH / 4; ++jj) {
          const f32x4 v = x4[jj];
          xa[f2][4 * jj] = v[0]; xa[f2][4 * jj + 1] = v[1]; xa[f2][4 * jj + 2] = v[2]; xa[f2][4 * jj + 3] = v[3];
        }
      }
#pragma unroll
      for (int s = 0; s < KH; ++s)
#pragma unroll
        for (int k = 0; k < NBW; ++k)
#pragma unroll
          for (int f2 = 0; f2 < 2; ++f2)
            ll[k][fp + f2] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[f2][s], wq[k][s], ll[k][fp + f2], 0, 0, 0);
    }
    // ---- softmax over the pdf's Gaussians, frame by frame (eigen.cc:20-32) ----
    // per-wave maximum of each frame: over this wave's blocks (in lane) and its 16 Gaussians (DPP row)
#pragma unroll
    for (int ft = 0; ft < 4; ++ft)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float m = ll[0][ft][r];
#pragma unroll
        for (int k = 1; k < NBW; ++k) m = fmaxf(m, ll[k][ft][r]);
        m = k3_row_max(m);
        if (j16 == 0) red[wave * K3_CHUNK + 16 * ft + 4 * q + r] = m;
      }
    k3_block_sync();
    if (tid < K3_CHUNK)
      fin[tid] = fmaxf(fmaxf(red[tid], red[K3_CHUNK + tid]), fmaxf(red[2 * K3_CHUNK + tid], red[3 * K3_CHUNK + tid]));
    k3_block_sync();
    float mx[4][4];
#pragma unroll
    for (int ft = 0; ft < 4; ++ft)
#pragma unroll
      for (int r = 0; r < 4; ++r) mx[ft][r] = fin[16 * ft + 4 * q + r];
    k3_block_sync();
#pragma unroll
    for (int ft = 0; ft < 4; ++ft)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < NBW; ++k) {
          const float e = __expf(ll[k][ft][r] - mx[ft][r]);   // (v - max).exp(); exp(-inf) = 0 for padding
          ll[k][ft][r] = e;
          s += e;
        }
        s = k3_row_sum(s);
        if (j16 == 0) red[wave * K3_CHUNK + 16 * ft + 4 * q + r] = s;
      }
    k3_block_sync();
    if (tid < K3_CHUNK)
      fin[tid] = (red[tid] + red[K3_CHUNK + tid]) + (red[2 * K3_CHUNK + tid] + red[3 * K3_CHUNK + tid]);
    k3_block_sync();
    // frame log-likelihood = log(sum) + max (eigen.cc:28): lanes j16 == 0 of wave 0 hold each frame once
#pragma unroll
    for (int ft = 0; ft < 4; ++ft)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = 16 * ft + 4 * q + r;
        const float ssum = fin[f];
        float wf = a.weight;                                          // POST: the entry's own weight
        if constexpr (POST) wf = wts[f];
        if (wave == 0 && j16 == 0 && f < cf) {
          const float llf = __logf(ssum) + mx[ft][r];
          if (!(fabsf(llf) <= 3.0e38f)) atomicOr(a.err_flag, 1);      // diag-gmm.cc:385-387
          tot_ll += (double)(llf * wf);                               // mle-am-diag-gmm.cc:49
          if constexpr (POST) tot_w += (double)wf;                    // :50
        }
        // eigen.cc:31 (e / sum) and mle-diag-gmm.cc:153 (* weight) as ONE correctly rounded division per frame
        // and a multiply per Gaussian (<= 1 ulp from the reference's per-element division)
        const float scale = f < cf ? wf / ssum : 0.0f;
#pragma unroll
        for (int k = 0; k < NBW; ++k) ll[k][ft][r] = ll[k][ft][r] * scale;
      }
    // ---- phase B: acc[k][db] += gamma^T · [x | x²] on fp64 MFMA ----
#pragma unroll
    for (int ft = 0; ft < 4; ++ft) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int fr = 16 * ft + 4 * q + s;                      // B operand row: frame 16*ft + 4*q + s
        double ga[NBW];
#pragma unroll
        for (int k = 0; k < NBW; ++k) { ga[k] = (double)ll[k][ft][s]; occ[k] += ga[k]; }   // mle-diag-gmm.cc:132
#pragma unroll
        for (int db = 0; db < NDB; ++db) {
          const int col = 16 * db + j16;                          // column of [x | x²]: d = col (x) or col - XP (x²)
          const int d = col < XP ? col : col - XP;
          const double bv = (double)xq[(((col < XP ? 0 : 2) + (d & 1)) * K3_CHUNK + fr) * KH + (d >> 1)];
#pragma unroll
          for (int k = 0; k < NBW; ++k)
            acc[k][db] = __builtin_amdgcn_mfma_f64_16x16x4f64(ga[k], bv, acc[k][db], 0, 0, 0);
        }
      }
    }
  }
  // ---- flush: C layout of the fp64 MFMA: column = lane&15 (d'), rows (lane>>4) + 4*reg (Gaussian) ----
#pragma unroll
  for (int k = 0; k < NBW; ++k) {
    const int gb = 16 * (wave + 4 * k);
#pragma unroll
    for (int db = 0; db < NDB; ++db) {
      const int col = 16 * db + j16;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int g = gb + q + 4 * r;
        if (g < G) {
          if (col < D) atomicAdd(a.mean_acc + (int64_t)(g0 + g) * D + col, acc[k][db][r]);
          else if (col >= XP && col - XP < D) atomicAdd(a.var_acc + (int64_t)(g0 + g) * D + (col - XP), acc[k][db][r]);
        }
      }
    }
    // occupancy: this lane summed gamma of Gaussian gb + j16 over frames 4*q + s; fold the 4 quarters
    double o = occ[k];
    o += __shfl_xor(o, 16);
    o += __shfl_xor(o, 32);
    if (q == 0 && gb + j16 < G) atomicAdd(a.occ + g0 + gb + j16, o);
  }
  if (wave == 0) {
    for (int o2 = 32; o2 > 0; o2 >>= 1) tot_ll += __shfl_xor(tot_ll, o2);
    if (lane == 0 && tot_ll != 0.0) atomicAdd(&a.scalars[1], tot_ll);
  }
  if constexpr (POST) {
    // the sum of the weights of this block's entries, where an alignment has frames x weight
    if (wave == 0) {
      for (int o2 = 32; o2 > 0; o2 >>= 1) tot_w += __shfl_xor(tot_w, o2);
      if (lane == 0 && tot_w != 0.0) atomicAdd(&a.scalars[0], tot_w);
    }
  } else {
    if (tid == 0 && it.y == 0) atomicAdd(&a.scalars[0], (double)nfr * (double)a.weight);  // mle-am-diag-gmm.cc:50
  }
}

// one global fp64 atomic per accumulator cell from a folded image [NB*16][2*XP] + occ[NB*16] (XP = 40)
// (the per-dimension feature envelope max_g |mean| + 8 sigma the fp16 phase A scales by is read by k0_model_stats, khg_ctx_model.hip,
//  in the one pass per parameter version that also reads the column maxima)
typedef _Float16 k3_f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 k3_f16x4 __attribute__((ext_vector_type(4)));
typedef __fp16 k3_fp16x4 __attribute__((__vector_size__(4 * sizeof(__fp16))));
typedef __attribute__((address_space(3))) k3_fp16x4 k3_lds_h4;     // an LDS operand of ds_read_b64_tr_b16
__device__ __forceinline__ k3_f16x4 k3_read_tr16(k3_lds_h4* p) { return __builtin_bit_cast(k3_f16x4, __builtin_amdgcn_ds_read_tr16_b64_v4f16(p)); }
#define K3_XH_ROW 104          // fp16 elements per frame row of the split planes (96 used; 208 B: conflict-free 16-byte reads)

template <int NB>
__device__ __forceinline__ void k3_wave_flush(const K3Args& a, const double* sum, int g0, int G, int D, int tid) {
  constexpr int XP = 40;
  for (int i = tid; i < NB * 16 * 2 * XP; i += 256) {
    const int g = i / (2 * XP), col = i - g * (2 * XP);
    if (g < G) {
      if (col < D) atomicAdd(a.mean_acc + (int64_t)(g0 + g) * D + col, sum[i]);
      else if (col >= XP && col - XP < D) atomicAdd(a.var_acc + (int64_t)(g0 + g) * D + (col - XP), sum[i]);
    }
  }
  if (tid < NB * 16 && tid < G) atomicAdd(a.occ + g0 + tid, sum[NB * 16 * 2 * XP + tid]);
}

__device__ __forceinline__ void k3_lds_sync() {   // wave-local LDS ordering: no workgroup barrier
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// ------------------------------------------------------------------------------------------
// Wave-local form of k3_accumulate_mfma for pdfs of <= 64 Gaussians and D <= 40 (the benchmark's shape).
// Same two MFMA phases and the same arithmetic, but a wave owns 16-FRAME tiles and ALL of the pdf's Gaussian
// blocks (NB <= 4) instead of 16 Gaussians of a 64-frame chunk: the softmax over the pdf's Gaussians is then
// an in-lane fold over the blocks plus one DPP row reduction -- no cross-wave exchange, so the tile loop
// has no workgroup barrier at all (the block form needs seven per chunk) and the four waves of a block, and
// the blocks sharing a CU, overlap each other's gathers and MFMA phases freely.
//   W (both planes of every Gaussian) sits in LDS in B-operand order: one ds_read_b32 per fp32 MFMA;
//   each wave stages its tile's [x | x²] planes in its own LDS area (wave-local ordering only);
//   the fp64 accumulators of all NB blocks stay in registers (NB*40 VGPRs) for the whole block; at the end
//   the four waves fold them, in wave order, into one LDS image, flushed with one fp64 atomic per cell.
// F16A: phase A on the fp16 matrix cores in the f16x2s arithmetic of K1s (khg_k1_f16x2s.hip.inc): per contraction index the
// operands are scaled by exact powers of two (exponents a.pa_ex, derived from the MODEL alone so that the statistics do not
// depend on how the utterances are sharded), split into two fp16 pieces each, and the three partial products w1 x1 + w1 x2 +
// w2 x1 accumulate in fp32 on v_mfma_f32_16x16x32_f16 with gconst 2^S as the C input: 9 MFMAs of 16 cycles per 16-Gaussian block
// and tile instead of 20 of 32 (fp32 MFMAs and vector instructions add up on gfx950, 16-bit MFMAs run under vector work).
// Measured error of the arithmetic against fp64: 2.1e-7 B (the fp32 chain: 7.4e-7 B).  Phase B is unchanged.
template <int NB, bool F16A = false>
__global__ __launch_bounds__(256, NB <= 2 ? 2 : 1) void k3_accumulate_wave(K3Args a) {
  extern __shared__ __attribute__((aligned(16))) float k3s[];
  constexpr int KQ = 10, XP = 4 * KQ, KH = 2 * KQ, NDB = KQ / 2, TF = 16;
  K3Item it;
  if (!k3_take_item(a, it)) return;
  const int pdf = it.pdf;
  const int64_t beg = a.pdf_start[pdf];
  const int nfr = (int)(a.pdf_start[pdf + 1] - beg);
  if (nfr == 0) return;
  const int D = a.D;
  const int g0 = a.gauss_off[pdf], G = a.gauss_off[pdf + 1] - g0;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j16 = lane & 15, q = lane >> 4;
  float* Wl = k3s;                                          // [NB][KH][64]   (fp32 phase A)
  float* xw = (F16A ? k3s : Wl + NB * KH * 64) + wave * (4 * TF * KH);     // this wave's planes [4][16][KH]
  _Float16* xh = reinterpret_cast<_Float16*>(k3s + 4 * (4 * TF * KH)) + wave * (2 * TF * K3_XH_ROW);   // F16A: [piece 2][frame 16][K3_XH_ROW]
  float gcv[NB];
#pragma unroll
  for (int k = 0; k < NB; ++k) gcv[k] = (16 * k + j16 < G) ? a.gconsts[g0 + 16 * k + j16] : -INFINITY;
  float wq[F16A ? 1 : NB][F16A ? 1 : KH];
  k3_f16x8 w1[F16A ? NB : 1][3], w2[F16A ? NB : 1][3];
  if constexpr (!F16A) {
    // ---- W into LDS, once ----
    for (int idx = tid; idx < NB * KH * 64; idx += 256) {
      const int l = idx & 63, s = (idx >> 6) % KH, k = idx / (64 * KH);
      const int g = 16 * k + (l & 15), qq = l >> 4, d = 2 * s + (qq & 1);
      float v = 0.0f;
      if (g < G && d < D) v = (qq & 2) ? a.nhalf_inv_vars[(int64_t)(g0 + g) * D + d] : a.means_invvars[(int64_t)(g0 + g) * D + d];
      Wl[idx] = v;
    }
    __syncthreads();
    // the B operands of phase A stay in registers for the whole block (one wave per SIMD: the file is there).  (Reading them from
    // LDS at their MFMA to fit two waves per SIMD was tried in round 3: 256 VGPRs, no AGPR split, 64 spilled dwords -> 16.2 ms.)
#pragma unroll
    for (int k = 0; k < NB; ++k)
#pragma unroll
      for (int s = 0; s < KH; ++s) wq[k][s] = Wl[(k * KH + s) * 64 + lane];
  } else {
    // the scaled, split W operands of this lane (Gaussian 16 k + j16; contraction index k' = 32 st + 8 q + e: k' < 40 the mean
    // plane of dim k', 40 <= k' < 80 the variance plane of dim k' - 40, then zero padding), straight from the model's rows
#pragma unroll
    for (int k = 0; k < NB; ++k)
#pragma unroll
      for (int st = 0; st < 3; ++st) {
        k3_f16x8 p1, p2;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int kp = 32 * st + 8 * q + e, var = kp >= XP, d = var ? kp - XP : kp, g = 16 * k + j16;
          float v = 0.0f;
          if (kp < 2 * XP && g < G && d < D) {
            const float w = var ? a.nhalf_inv_vars[(int64_t)(g0 + g) * D + d] : a.means_invvars[(int64_t)(g0 + g) * D + d];
            v = ldexpf(w, a.pa_S - a.pa_ex[2 * d + var]);
          }
          const _Float16 h1 = (_Float16)v;
          p1[e] = h1; p2[e] = (_Float16)(v - (float)h1);
        }
        w1[k][st] = p1; w2[k][st] = p2;
      }
#pragma unroll
    for (int k = 0; k < NB; ++k) gcv[k] = gcv[k] * a.pa_scale;        // the C input carries the common scale 2^S (-inf stays -inf)
    for (int i = lane; i < 2 * TF * K3_XH_ROW; i += 64) xh[i] = (_Float16)0.0f;   // the padding columns stay zero
    k3_lds_sync();
  }
  (void)Wl; (void)wq; (void)w1; (void)w2;

  f64x4 acc[NB][NDB];
  double occ[NB];
#pragma unroll
  for (int k = 0; k < NB; ++k) {
    occ[k] = 0.0;
#pragma unroll
    for (int db = 0; db < NDB; ++db) acc[k][db] = f64x4{0, 0, 0, 0};
  }
  double tot_ll = 0.0;
  const int ntile = (nfr + TF - 1) / TF;
  // lane -> the (frame, dim) cells it gathers: i = lane + 64*j, frame i / XP, dim i % XP.  The NEXT tile's
  // features are requested (into registers) as soon as this tile's are parked in LDS, so their HBM latency is
  // covered by this tile's two MFMA phases.
  constexpr int NG = TF * XP / 64;
  const int tstride = 4 * it.ny;
  float pre[NG];
  float sx[F16A ? NG : 1], sx2[F16A ? NG : 1];              // F16A: 2^ex of the (frame, dim) cells this lane stages
  if constexpr (F16A) {
#pragma unroll
    for (int j = 0; j < NG; ++j) {
      const int d = min((lane + 64 * j) % XP, D - 1);
      sx[j] = ldexpf(1.0f, a.pa_ex[2 * d]); sx2[j] = ldexpf(1.0f, a.pa_ex[2 * d + 1]);
    }
  }
  (void)sx; (void)sx2;
  // Tile t of the loop is tile (t + rot) mod ntile of the bucket: the buckets are in frame order, and the blocks of
  // neighbouring pdfs (consecutive HMM states: their frames are neighbours in memory) would otherwise sweep the
  // feature matrix in lock-step through the same HBM channels.  A fixed per-pdf rotation keeps the order a pure
  // function of the input.
  const int rot = (int)(((unsigned)pdf * 2654435761u) % (unsigned)ntile);
  auto tile_of = [&](int t) { const int x = t + rot; return x >= ntile ? x - ntile : x; };
  // The frame ids of a tile are loaded ONE TILE AHEAD of its features (two ahead of its use): the features' addresses depend on
  // them, and a dependent pair of HBM loads inside one request left the wave waiting ~2.5k of every ~10k cycles (SQ_WAIT_ANY 0.28).
  auto fid_of = [&](int tl) -> int {
    if (tl >= ntile) return 0;
    const int t = tile_of(tl);
    return (lane < min(TF, nfr - t * TF)) ? a.frame_ids[beg + t * TF + lane] : 0;
  };
  // All NG loads of a request are issued back to back from always-valid addresses (a lane past the tile's end carries frame id 0,
  // a padding dim reads dim D-1): the zero fill happens when the tile is parked in LDS.  (Selecting at the load made every one of
  // the NG gathers its own branch region with an LDS wait for its shuffle: ~1.5k of a tile's ~13k cycles.)
  auto request = [&](int tl, int myfid) {
    (void)tl;
    int fidv[NG];
#pragma unroll
    for (int j = 0; j < NG; ++j) fidv[j] = __shfl(myfid, (lane + 64 * j) / XP);
#pragma unroll
    for (int j = 0; j < NG; ++j) {
      const int i = lane + 64 * j, f = i / XP, d = i - f * XP;
      pre[j] = a.feats[(int64_t)fidv[j] * D + min(d, D - 1)];
    }
  };
  int t = it.y * 4 + wave;
  int fid_next = 0;
  if (t < ntile) { request(t, fid_of(t)); fid_next = fid_of(t + tstride); }
  for (; t < ntile; t += tstride) {
    const int cf = min(TF, nfr - tile_of(t) * TF);
#pragma unroll
    for (int j = 0; j < NG; ++j) {
      const int i = lane + 64 * j, f = i / XP, d = i - f * XP;
      float* dst = xw + ((d & 1) * TF + f) * KH + (d >> 1);
      const float v = (f < cf && d < D) ? pre[j] : 0.0f;
      dst[0] = v;
      dst[2 * TF * KH] = v * v;
      if constexpr (F16A) {
        const float s1 = v * sx[j], s2 = (v * v) * sx2[j];        // fl(x^2) first, as the planes of phase B (and the reference's squares)
        const _Float16 h1 = (_Float16)s1, g1 = (_Float16)s2;
        _Float16* r1 = xh + f * K3_XH_ROW + d;
        r1[0] = h1; r1[TF * K3_XH_ROW] = (_Float16)(s1 - (float)h1);
        r1[XP] = g1; r1[TF * K3_XH_ROW + XP] = (_Float16)(s2 - (float)g1);
      }
    }
    if (t + tstride < ntile) { request(t + tstride, fid_next); fid_next = fid_of(t + 2 * tstride); }
    k3_lds_sync();
    // ---- phase A ----
    f32x4 ll[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) ll[k] = f32x4{gcv[k], gcv[k], gcv[k], gcv[k]};
    if constexpr (!F16A) {
      float xa[KH];
      {
        const f32x4* x4 = reinterpret_cast<const f32x4*>(xw + (q * TF + j16) * KH);
#pragma unroll
        for (int jj = 0; jj < KH / 4; ++jj) {
          const f32x4 v = x4[jj];
          xa[4 * jj] = v[0]; xa[4 * jj + 1] = v[1]; xa[4 * jj + 2] = v[2]; xa[4 * jj + 3] = v[3];
        }
      }
#pragma unroll
      for (int s = 0; s < KH; ++s)          // the NB accumulation chains advance together (per Gaussian: s in order, as K1)
#pragma unroll
        for (int k = 0; k < NB; ++k)
          ll[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[s], wq[k][s], ll[k], 0, 0, 0);
    } else {
#pragma unroll
      for (int st = 0; st < 3; ++st) {
        const k3_f16x8 x1 = *reinterpret_cast<const k3_f16x8*>(xh + j16 * K3_XH_ROW + 32 * st + 8 * q);
        const k3_f16x8 x2 = *reinterpret_cast<const k3_f16x8*>(xh + (TF + j16) * K3_XH_ROW + 32 * st + 8 * q);
#pragma unroll
        for (int k = 0; k < NB; ++k) {
          ll[k] = __builtin_amdgcn_mfma_f32_16x16x32_f16(x2, w1[k][st], ll[k], 0, 0, 0);
          ll[k] = __builtin_amdgcn_mfma_f32_16x16x32_f16(x1, w2[k][st], ll[k], 0, 0, 0);
          ll[k] = __builtin_amdgcn_mfma_f32_16x16x32_f16(x1, w1[k][st], ll[k], 0, 0, 0);
        }
      }
    }
    // ---- softmax over the pdf's Gaussians (eigen.cc:20-32): blocks in lane, Gaussians of a block in the DPP row ----
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float m = ll[0][r];
#pragma unroll
      for (int k = 1; k < NB; ++k) m = fmaxf(m, ll[k][r]);
      m = k3_row_max(m);
      float ssum = 0.0f;
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        const float e = __builtin_amdgcn_exp2f((ll[k][r] - m) * (F16A ? a.pa_c1 : 1.44269504088896340736f));   // as K1's epilogue; exp2(-inf) = 0 for padding Gaussians
        ll[k][r] = e;
        ssum += e;
      }
      ssum = k3_row_sum(ssum);
      const int f = 4 * q + r;
      if (j16 == 0 && f < cf) {
        const float llf = __logf(ssum) + (F16A ? m * a.pa_inv : m);        // eigen.cc:28
        if (!(fabsf(llf) <= 3.0e38f)) atomicOr(a.err_flag, 1);             // diag-gmm.cc:385-387
        tot_ll += (double)(llf * a.weight);                                // mle-am-diag-gmm.cc:49
      }
      const float scale = f < cf ? a.weight / ssum : 0.0f;                 // one division per frame, as the block form
#pragma unroll
      for (int k = 0; k < NB; ++k) ll[k][r] = ll[k][r] * scale;
    }
    // ---- phase B: acc[k][db] += gamma^T . [x | x²] on fp64 MFMA ----
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int fr = 4 * q + s;
      double ga[NB];
#pragma unroll
      for (int k = 0; k < NB; ++k) { ga[k] = (double)ll[k][s]; occ[k] += ga[k]; }          // mle-diag-gmm.cc:132
#pragma unroll
      for (int db = 0; db < NDB; ++db) {
        const int col = 16 * db + j16;
        const int d = col < XP ? col : col - XP;
        const double bv = (double)xw[(((col < XP ? 0 : 2) + (d & 1)) * TF + fr) * KH + (d >> 1)];
#pragma unroll
        for (int k = 0; k < NB; ++k)
          acc[k][db] = __builtin_amdgcn_mfma_f64_16x16x4f64(ga[k], bv, acc[k][db], 0, 0, 0);
      }
    }
    k3_lds_sync();    // this tile's LDS reads are done before the next gather overwrites the planes
  }
  // ---- fold the four waves through LDS in wave order, then ONE global fp64 atomic per accumulator cell and launch
  //      (directly with one block per pdf, through k3_wave_finalize otherwise): every sum has a fixed order, the
  //      statistics are run-to-run reproducible ----
  __syncthreads();
  double* sum = reinterpret_cast<double*>(k3s);             // [NB*16][2*XP] + occ [NB*16]
  constexpr int NSUM = NB * 16 * 2 * XP + NB * 16;
  for (int i = tid; i < NSUM; i += 256) sum[i] = 0.0;
  __syncthreads();
#pragma unroll 1
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int k = 0; k < NB; ++k) {
#pragma unroll
        for (int db = 0; db < NDB; ++db) {
          const int col = 16 * db + j16;                    // C layout of the fp64 MFMA: column lane&15, rows (lane>>4) + 4*reg
#pragma unroll
          for (int r = 0; r < 4; ++r) atomicAdd(&sum[(16 * k + q + 4 * r) * (2 * XP) + col], acc[k][db][r]);   // ds_add_f64: no return value, no extra registers; one wave at a time, so the order is fixed
        }
        double o = occ[k];
        o += __shfl_xor(o, 16);
        o += __shfl_xor(o, 32);
        if (q == 0) atomicAdd(&sum[NB * 16 * 2 * XP + 16 * k + j16], o);
      }
    }
    __syncthreads();
  }
  // this block's share of total_log_like: lanes by a fixed shuffle tree, waves in order
  __shared__ double s_ll[4];
  for (int o2 = 32; o2 > 0; o2 >>= 1) tot_ll += __shfl_xor(tot_ll, o2);
  if (lane == 0) s_ll[wave] = tot_ll;
  __syncthreads();
  const double block_ll = ((s_ll[0] + s_ll[1]) + s_ll[2]) + s_ll[3];
  if (it.ny == 1) {
    k3_wave_flush<NB>(a, sum, g0, G, D, tid);
    if (tid == 0) a.ll_part[pdf] = block_ll;
  } else {
    // several blocks per pdf: park the image; k3_wave_finalize adds the slices in order
    double* dst = a.part + (int64_t)it.slot * (NSUM + 1);
    for (int i = tid; i < NSUM; i += 256) dst[i] = sum[i];
    if (tid == 0) dst[NSUM] = block_ll;
  }
}

// ------------------------------------------------------------------------------------------
// k3_accumulate_wave16 (round 4): the wave form with BOTH phases on the fp16 matrix cores.
// Why: on gfx950 a v_mfma_f64_16x16x4_f64 takes 64 cycles AND holds the SIMD's vector issue for all of them (measured twice in
// round 4, profiles/r4_k1_ab_lse.txt: neither a second wave per SIMD nor a software pipeline gets anything to run under it), so
// the 20 NB fp64 MFMAs of phase B (5 120 cycles per 16-frame tile at NB = 4) simply add to the ~4 900 cycles of everything else.
// The 16-bit MFMAs take 16 cycles and DO run under vector work.  Phase B here:
//   * two 16-frame tiles (32 frames) per step: K = 32 of v_mfma_f32_16x16x32_f16, A = gamma^T (16 Gaussians x 32 frames),
//     B = [x' | x^2'] (32 frames x 16 columns), D = fp32 partial sums of the 32 frames;
//   * both operands are split into two fp16 pieces WITHOUT rescaling the residual (khg_k1_f16x2s.hip.inc): gamma' = gamma 2^SG
//     (SG from the accumulation weight alone: |weight| 2^SG in [2^13, 2^14)), x' = x 2^ex / fl(x^2) 2^ex as phase A stages them
//     (exponents from the MODEL alone); the three partial products g1 x1 + g1 x2 + g2 x1 go into one fp32 accumulator:
//     60 MFMAs of 16 cycles per 32 frames at NB = 4 -- 480 cycles per tile instead of 5 120, hidden under the vector work;
//   * the 32-frame partial sums are widened and added to fp64 accumulators (registers, scaled units; 2^-(SG + ex) applied once at
//     the end: exact), so long sums still accumulate in fp64 as the reference's do (mle-diag-gmm.cc:135-140).
// What changes against the fp64 form: a product gamma x carries 22 + 22 significant bits instead of 24 + 24 (the reference rounds
// each product to fp32, 2^-24, before widening it: mle-diag-gmm.cc:135,138-140) and 32 of them are summed in fp32 before the
// fp64 add -- relative differences of ~1e-7 in a cell, far inside the 2e-5 the statistics are compared at; the sums depend on how
// frames fall into 32-frame groups, so N ranks' statistics add up to the one-rank statistics to ~1e-7, not 1e-12.  occ, the
// transition counts and the log-likelihood are computed exactly as in the fp64 form.  Run-to-run reproducible (fixed order).
// ONE LDS image serves both phases: the split planes are staged frame-major ([piece][frame][K3_X16_ROW]); phase A reads a frame's
// row (ds_read_b128), phase B reads the same rows through ds_read_b64_tr_b16, which hands lane 16 q + n column n of the four frames
// 4 q .. 4 q + 3 -- the K-slot order (q, e) of the B operand.  Rows of 224 B: the eight rows a 32-lane half of a transposed read
// touches start 56 banks apart (eight distinct 32-byte slots of the 256-byte bank row), and the 16-lane groups of the 16-byte row
// reads see sixteen distinct 16-byte slots (14 j + q mod 16 over a group's lanes); at 208 B the transposed reads are two-way.
// The instruction needs EXEC all ones and 8-byte addresses: every lane's address lies inside the image (rows 0..15, columns < 80)
// and the pair loop is wave-uniform.
// PLANES (KHG_OPT_K3_PLANES): the image is copied from the set's split feature records (k3_pack_x: 320 B per frame, made once per
// (set, exponents)) by 16-byte loads and ds_write_b128 -- no conversion in the loop; record N (zeros) stands for the frames past a
// tile's end.  Without them the loop splits the raw features itself, as it always did: same bits either way.
#define K3_X16_ROW 112        // fp16 elements per frame row of k3_accumulate_wave16's image (96 used; 224 B)
#define K3_XREC 160           // fp16 elements of a split feature record: [x'1 (40) | x^2'1 (40) | x'2 (40) | x^2'2 (40)]
__device__ __forceinline__ void k3_split_cell(float v, float sx, float sx2, _Float16& h1, _Float16& h2, _Float16& g1, _Float16& g2) {
  const float s1 = v * sx, s2 = (v * v) * sx2;        // fl(x^2) first (the reference's squares)
  h1 = (_Float16)s1; g1 = (_Float16)s2;
  h2 = (_Float16)(s1 - (float)h1); g2 = (_Float16)(s2 - (float)g1);
}
// The records of frames [0, N) and the zero record N: one thread per (record, 8 dims) writes its 16 bytes of each of the four parts
__global__ __launch_bounds__(256) void k3_pack_x(const float* __restrict__ feats, int64_t N, int D, const int32_t* __restrict__ ex, _Float16* __restrict__ rec) {
  const int64_t n = (N + 1) * 5;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t f = i / 5;
    const int d0 = 8 * (int)(i - 5 * f);
    k3_f16x8 h1, h2, g1, g2;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int d = d0 + e, dc = min(d, D - 1);
      const float v = (f < N && d < D) ? feats[f * D + dc] : 0.0f;
      _Float16 a1, a2, b1, b2;
      k3_split_cell(v, ldexpf(1.0f, ex[2 * dc]), ldexpf(1.0f, ex[2 * dc + 1]), a1, a2, b1, b2);
      h1[e] = a1; h2[e] = a2; g1[e] = b1; g2[e] = b2;
    }
    _Float16* r = rec + f * K3_XREC + d0;
    *reinterpret_cast<k3_f16x8*>(r) = h1; *reinterpret_cast<k3_f16x8*>(r + 40) = g1;
    *reinterpret_cast<k3_f16x8*>(r + 80) = h2; *reinterpret_cast<k3_f16x8*>(r + 120) = g2;
  }
}
template <int NB, bool PLANES = false>
__global__ __launch_bounds__(256, 1) void k3_accumulate_wave16(K3Args a) {
  extern __shared__ __attribute__((aligned(16))) float k3s[];
  constexpr int KQ = 10, XP = 4 * KQ, NDB = KQ / 2, TF = 16, ROW = K3_X16_ROW;
  constexpr int XHH = 2 * TF * ROW;                // halves of one tile's planes [piece 2][frame 16][ROW]
  K3Item it;
  if (!k3_take_item(a, it)) return;
  const int pdf = it.pdf;
  const int64_t beg = a.pdf_start[pdf];
  const int nfr = (int)(a.pdf_start[pdf + 1] - beg);
  if (nfr == 0) return;
  const int D = a.D;
  const int g0 = a.gauss_off[pdf], G = a.gauss_off[pdf + 1] - g0;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j16 = lane & 15, q = lane >> 4;
  _Float16* xh = reinterpret_cast<_Float16*>(k3s) + wave * (2 * XHH);               // this wave's planes of the pair's two tiles
  float gcv[NB];
#pragma unroll
  for (int k = 0; k < NB; ++k) gcv[k] = ((16 * k + j16 < G) ? a.gconsts[g0 + 16 * k + j16] : -INFINITY) * a.pa_scale;
  // phase A's split W operands ([block][step][piece][lane] x 16 B = 6 NB KiB, shared by the four waves) sit in LDS behind the waves'
  // planes: the fp64 totals, two tiles' posteriors and the split gamma operands leave no room for 24 NB more registers
  char* wl16 = reinterpret_cast<char*>(reinterpret_cast<_Float16*>(k3s) + 4 * (2 * XHH));
  for (int e0 = tid; e0 < NB * 3 * 64; e0 += 256) {
    const int l = e0 & 63, st = (e0 >> 6) % 3, k = e0 / (3 * 64), jl = l & 15, ql = l >> 4;
    k3_f16x8 p1, p2;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int kp = 32 * st + 8 * ql + e, var = kp >= XP, d = var ? kp - XP : kp, g = 16 * k + jl;
      float v = 0.0f;
      if (kp < 2 * XP && g < G && d < D) {
        const float w = var ? a.nhalf_inv_vars[(int64_t)(g0 + g) * D + d] : a.means_invvars[(int64_t)(g0 + g) * D + d];
        v = ldexpf(w, a.pa_S - a.pa_ex[2 * d + var]);
      }
      const _Float16 h1 = (_Float16)v;
      p1[e] = h1; p2[e] = (_Float16)(v - (float)h1);
    }
    *reinterpret_cast<k3_f16x8*>(wl16 + (((k * 3 + st) * 2 + 0) * 64 + l) * 16) = p1;
    *reinterpret_cast<k3_f16x8*>(wl16 + (((k * 3 + st) * 2 + 1) * 64 + l) * 16) = p2;
  }
  {                                                                         // padding columns / padding dims stay zero
    static_assert((2 * XHH) % 8 == 0 && ROW % 8 == 0, "the wave's planes and their rows are whole 16-byte words");
    const k3_f16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = lane; i < (2 * XHH) / 8; i += 64) reinterpret_cast<k3_f16x8*>(xh)[i] = z;
  }
  __syncthreads();

  f64x4 acc[NB][NDB];          // fp64 totals in scaled units: column n = lane & 15 of block db, Gaussians 4 (lane >> 4) + r of block k
  double occ[NB];
#pragma unroll
  for (int k = 0; k < NB; ++k) {
    occ[k] = 0.0;
#pragma unroll
    for (int db = 0; db < NDB; ++db) acc[k][db] = f64x4{0, 0, 0, 0};
  }
  double tot_ll = 0.0;
  unsigned bad = 0;
  const int ntile = (nfr + TF - 1) / TF, npair = (ntile + 1) / 2;
  // A lane stages 2 x 2 MICRO-TILES (two adjacent frames x two adjacent dims) of the pair's 2 x 16 x 40 cells: micro-tile
  // i = lane + 64 j, j < NM = 5: tile i / 160, frame pair (i % 160) / 20, dim pair i % 20.  The kernel is bound by the LDS
  // pipe (SQ_ACTIVE_INST_LDS = busy cycles with one cell per lane and eight 2-byte writes per cell): a micro-tile's four cells go
  // out as 4-byte writes -- two dims of one frame are neighbours in the frame-major planes --, half the lane shuffles for the frame
  // ids, 8-byte feature loads.
  // PLANES: a lane copies 16-byte chunks of the pair's 32 records: chunk i = lane + 64 j, j < NR = 10: frame slot i / 20 (tile 0:
  // j < 5), chunk i % 20 of its record (piece (i % 20) / 10, columns 8 ((i % 20) % 10) ..) -- a record is read by 20 neighbouring lanes.
  constexpr int NM = 2 * TF * XP / (4 * 64), NR = 2 * TF * (K3_XREC / 8) / 64;
  static_assert(NM * 4 * 64 == 2 * TF * XP, "micro-tiles cover the pair exactly");
  static_assert(NR * 64 == 2 * TF * (K3_XREC / 8) && (NR & 1) == 0, "record chunks cover the pair exactly, a tile per half of them");
  const int pstride = 4 * it.ny;
  float pre[NM][4];                       // [micro-tile][frame 2][dim 2]
  float sx[NM][2], sx2[NM][2];            // 2^ex of the micro-tile's two dims (x', x^2')
  k1b_u32x4 rec[NR];                      // PLANES: the pair's record chunks
  const bool even_d = (D & 1) == 0;       // 8-byte feature loads need even row lengths
  if constexpr (!PLANES) {
#pragma unroll
    for (int j = 0; j < NM; ++j)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int d = min(2 * ((lane + 64 * j) % 20) + c, D - 1);
        sx[j][c] = ldexpf(1.0f, a.pa_ex[2 * d]); sx2[j][c] = ldexpf(1.0f, a.pa_ex[2 * d + 1]);
      }
  }
  const int fid_none = PLANES ? a.xrec_zero : 0;      // what a lane past a tile's end asks for: the zero record / any valid row
  const float gs = a.pb_gscale;
  // pair p of the loop is pair (p + rot) mod npair of the bucket (see k3_accumulate_wave: neighbouring pdfs' blocks would otherwise
  // sweep the feature matrix in lock-step); its tiles are 2 p and 2 p + 1
  const int rot = (int)(((unsigned)pdf * 2654435761u) % (unsigned)npair);
  auto pair_of = [&](int p) { const int x = p + rot; return x >= npair ? x - npair : x; };
  auto cf_of = [&](int pl, int tau) { if (pl >= npair) return 0; const int t = 2 * pair_of(pl) + tau; return t < ntile ? min(TF, nfr - t * TF) : 0; };
  auto fid_of = [&](int pl, int tau) -> int {
    const int n = cf_of(pl, tau);
    const int t = pl < npair ? 2 * pair_of(pl) + tau : 0;
    return lane < n ? a.frame_ids[beg + t * TF + lane] : fid_none;
  };
  // the pair's features into pre[]: fid0 / fid1 = this lane's frame id of tile 0 / tile 1 (lane < 16); always-valid addresses (a lane past
  // a tile's end carries frame id 0, a padding dim reads dim D - 1), the zero fill happens when the pair is parked in LDS
  // (PLANES: the pair's record chunks into rec[]; a lane past a tile's end carries the zero record)
  auto request = [&](int fid0, int fid1) {
    if constexpr (PLANES) {
      const k1b_u32x4* src = reinterpret_cast<const k1b_u32x4*>(a.xrec);
#pragma unroll
      for (int j = 0; j < NR; ++j) {
        const int i = lane + 64 * j, fs = i / 20, kk = i - 20 * fs;
        const int fid = __shfl(j < NR / 2 ? fid0 : fid1, fs & (TF - 1));
        rec[j] = src[(int64_t)fid * (K3_XREC / 8) + kk];
      }
      return;
    }
    int fa[NM], fb[NM];
#pragma unroll
    for (int j = 0; j < NM; ++j) {
      const int i = lane + 64 * j, tau = i / 160, fp = (i % 160) / 20;
      // (the shuffle returns the SOURCE lane's register: micro-tiles 0, 1 of every lane lie in tile 0, 3, 4 in tile 1, and j = 2 is
      //  split between the half-waves -- there both ids are fetched and the reader picks)
      if (j < 2) { fa[j] = __shfl(fid0, 2 * fp); fb[j] = __shfl(fid0, 2 * fp + 1); }
      else if (j > 2) { fa[j] = __shfl(fid1, 2 * fp); fb[j] = __shfl(fid1, 2 * fp + 1); }
      else {
        const int a0 = __shfl(fid0, 2 * fp), a1 = __shfl(fid1, 2 * fp), b0 = __shfl(fid0, 2 * fp + 1), b1 = __shfl(fid1, 2 * fp + 1);
        fa[j] = tau ? a1 : a0; fb[j] = tau ? b1 : b0;
      }
    }
#pragma unroll
    for (int j = 0; j < NM; ++j) {
      const int d0 = 2 * ((lane + 64 * j) % 20);
      if (even_d) {
        typedef float f2 __attribute__((ext_vector_type(2)));
        const int dd = min(d0, D - 2);
        const f2 va = *reinterpret_cast<const f2*>(a.feats + (int64_t)fa[j] * D + dd), vb = *reinterpret_cast<const f2*>(a.feats + (int64_t)fb[j] * D + dd);
        pre[j][0] = va[0]; pre[j][1] = va[1]; pre[j][2] = vb[0]; pre[j][3] = vb[1];
      } else {
        const int da = min(d0, D - 1), db = min(d0 + 1, D - 1);
        pre[j][0] = a.feats[(int64_t)fa[j] * D + da]; pre[j][1] = a.feats[(int64_t)fa[j] * D + db];
        pre[j][2] = a.feats[(int64_t)fb[j] * D + da]; pre[j][3] = a.feats[(int64_t)fb[j] * D + db];
      }
    }
  };
  int p = it.y * 4 + wave;
  int fidn0 = 0, fidn1 = 0;
  if (p < npair) { request(fid_of(p, 0), fid_of(p, 1)); fidn0 = fid_of(p + pstride, 0); fidn1 = fid_of(p + pstride, 1); }
  for (; p < npair; p += pstride) {
    const int cf[2] = {cf_of(p, 0), cf_of(p, 1)};
    // ---- stage both tiles: the split planes, frame-major ([piece][frame][column]) ----
    if constexpr (PLANES) {
#pragma unroll
      for (int j = 0; j < NR; ++j) {
        const int i = lane + 64 * j, fs = i / 20, kk = i - 20 * fs, pc = kk >= K3_XREC / 16, tau = j >= NR / 2;
        *reinterpret_cast<k1b_u32x4*>(xh + tau * XHH + (pc * TF + (fs & (TF - 1))) * ROW + 8 * (kk - pc * (K3_XREC / 16))) = rec[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < NM; ++j) {
        typedef _Float16 h2v __attribute__((ext_vector_type(2)));
        const int i = lane + 64 * j, tau = i / 160, r = i % 160, f0 = 2 * (r / 20), d0 = 2 * (r % 20);
        const int cft = tau ? cf[1] : cf[0];
        _Float16 h1[4], h2[4], g1[4], g2[4];                        // [frame 2][dim 2]: the two pieces of x' and of x^2'
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int f = f0 + (e >> 1), d = d0 + (e & 1);
          const float v = (f < cft && d < D) ? pre[j][e] : 0.0f;
          k3_split_cell(v, sx[j][e & 1], sx2[j][e & 1], h1[e], h2[e], g1[e], g2[e]);
        }
        // dims d0, d0 + 1 of one frame are neighbours
#pragma unroll
        for (int ff = 0; ff < 2; ++ff) {
          _Float16* r1 = xh + tau * XHH + (f0 + ff) * ROW + d0;
          *reinterpret_cast<h2v*>(r1) = h2v{h1[2 * ff], h1[2 * ff + 1]};
          *reinterpret_cast<h2v*>(r1 + TF * ROW) = h2v{h2[2 * ff], h2[2 * ff + 1]};
          *reinterpret_cast<h2v*>(r1 + XP) = h2v{g1[2 * ff], g1[2 * ff + 1]};
          *reinterpret_cast<h2v*>(r1 + TF * ROW + XP) = h2v{g2[2 * ff], g2[2 * ff + 1]};
        }
      }
    }
    if (p + pstride < npair) { request(fidn0, fidn1); fidn0 = fid_of(p + 2 * pstride, 0); fidn1 = fid_of(p + 2 * pstride, 1); }
    k3_lds_sync();
    // ---- phase A + softmax, tile by tile (as k3_accumulate_wave<NB, true>) ----
    f32x4 ll[2][NB];
#pragma unroll
    for (int tau = 0; tau < 2; ++tau)
#pragma unroll
      for (int k = 0; k < NB; ++k) ll[tau][k] = f32x4{gcv[k], gcv[k], gcv[k], gcv[k]};
#pragma unroll
    for (int st = 0; st < 3; ++st) {          // a W operand is read once for both tiles (per Gaussian the steps stay in order)
      k3_f16x8 x1[2], x2[2];
#pragma unroll
      for (int tau = 0; tau < 2; ++tau) {
        x1[tau] = *reinterpret_cast<const k3_f16x8*>(xh + tau * XHH + j16 * ROW + 32 * st + 8 * q);
        x2[tau] = *reinterpret_cast<const k3_f16x8*>(xh + tau * XHH + (TF + j16) * ROW + 32 * st + 8 * q);
      }
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        const k3_f16x8 wa = *reinterpret_cast<const k3_f16x8*>(wl16 + (((k * 3 + st) * 2 + 0) * 64 + lane) * 16);
        const k3_f16x8 wb = *reinterpret_cast<const k3_f16x8*>(wl16 + (((k * 3 + st) * 2 + 1) * 64 + lane) * 16);
#pragma unroll
        for (int tau = 0; tau < 2; ++tau) {
          ll[tau][k] = __builtin_amdgcn_mfma_f32_16x16x32_f16(x2[tau], wa, ll[tau][k], 0, 0, 0);
          ll[tau][k] = __builtin_amdgcn_mfma_f32_16x16x32_f16(x1[tau], wb, ll[tau][k], 0, 0, 0);
          ll[tau][k] = __builtin_amdgcn_mfma_f32_16x16x32_f16(x1[tau], wa, ll[tau][k], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int tau = 0; tau < 2; ++tau) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float m = ll[tau][0][r];
#pragma unroll
        for (int k = 1; k < NB; ++k) m = fmaxf(m, ll[tau][k][r]);
        m = k3_row_max(m);
        float ssum = 0.0f;
#pragma unroll
        for (int k = 0; k < NB; ++k) {
          const float e = __builtin_amdgcn_exp2f((ll[tau][k][r] - m) * a.pa_c1);
          ll[tau][k][r] = e;
          ssum += e;
        }
        ssum = k3_row_sum(ssum);
        const int f = 4 * q + r;
        const bool counts = (j16 == 0) & (f < cf[tau]);
        const float llf = __logf(ssum) + m * a.pa_inv;                          // eigen.cc:28
        bad |= (counts & !(fabsf(llf) <= 3.0e38f)) ? 1u : 0u;                   // diag-gmm.cc:385-387
        tot_ll += counts ? (double)(llf * a.weight) : 0.0;                      // mle-am-diag-gmm.cc:49
        const float scale = f < cf[tau] ? a.weight / ssum : 0.0f;
#pragma unroll
        for (int k = 0; k < NB; ++k) ll[tau][k][r] = ll[tau][k][r] * scale;
      }
    }
    // ---- phase B on the fp16 matrix cores: part[k][db] = sum over the 32 frames of gamma'^T . [x' | x^2'] ----
    k3_f16x8 ga1[NB], ga2[NB];
    f32x4 prev[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float g = e < 4 ? ll[0][k][e] : ll[1][k][e - 4];                  // K slot (q, e): frame 4 q + (e & 3) of tile e >> 2
        occ[k] += (double)g;                                                    // mle-diag-gmm.cc:132
        const float gsc = g * gs;
        const _Float16 h1 = (_Float16)gsc;
        ga1[k][e] = h1; ga2[k][e] = (_Float16)(gsc - (float)h1);
      }
    }
#pragma unroll
    for (int db = 0; db < NDB; ++db) {
      // transposed reads of the frame-major image: lane 4 qq + pp of a 16-lane group names row qq of the group's block (frame 4 q + qq),
      // columns 4 pp .. of the column block; lane 16 q + j16 receives column 16 db + j16 of frames 4 q .. 4 q + 3 -- tile 0, then tile 1
      k3_lds_h4* cb = (k3_lds_h4*)(xh + (4 * q + (j16 >> 2)) * ROW + 16 * db + 4 * (j16 & 3));
      k3_f16x8 xb1, xb2;
      {
        typedef k3_f16x4 h4;
        constexpr int T1 = XHH / 4, P2 = TF * ROW / 4;                            // tile 1, piece 2: in 8-byte words
        const h4 a0 = k3_read_tr16(cb), a1 = k3_read_tr16(cb + T1);
        const h4 b0 = k3_read_tr16(cb + P2), b1 = k3_read_tr16(cb + T1 + P2);
#pragma unroll
        for (int e = 0; e < 4; ++e) { xb1[e] = a0[e]; xb1[4 + e] = a1[e]; xb2[e] = b0[e]; xb2[4 + e] = b1[e]; }
      }
      f32x4 cur[NB];
#pragma unroll
      for (int k = 0; k < NB; ++k) {
        f32x4 c = f32x4{0, 0, 0, 0};
        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(ga1[k], xb2, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(ga2[k], xb1, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x32_f16(ga1[k], xb1, c, 0, 0, 0);
        cur[k] = c;
      }
      // the PREVIOUS column block's partial sums into the fp64 totals, under this block's MFMAs
      if (db > 0) {
#pragma unroll
        for (int k = 0; k < NB; ++k)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[k][db - 1][r] += (double)prev[k][r];
      }
#pragma unroll
      for (int k = 0; k < NB; ++k) prev[k] = cur[k];
    }
#pragma unroll
    for (int k = 0; k < NB; ++k)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[k][NDB - 1][r] += (double)prev[k][r];
    k3_lds_sync();    // this pair's LDS reads are done before the next gather overwrites the planes
  }
  // ---- fold the four waves through LDS in wave order, unscaling on the way (powers of two: exact) ----
  __syncthreads();
  double* sum = reinterpret_cast<double*>(k3s);             // [NB*16][2*XP] + occ [NB*16]
  constexpr int NSUM = NB * 16 * 2 * XP + NB * 16;
  for (int i = tid; i < NSUM; i += 256) sum[i] = 0.0;
  __syncthreads();
  int unscale[NDB];
#pragma unroll
  for (int db = 0; db < NDB; ++db) {
    const int col = 16 * db + j16, var = col >= XP, d = min(var ? col - XP : col, D - 1);
    unscale[db] = -(a.pb_SG + a.pa_ex[2 * d + var]);
  }
  // In phase ph wave w adds its totals of Gaussian block (w + ph) mod 4: all four waves add in every phase, to different cells, and
  // every cell receives the waves in one fixed order (w = k, k - 1, k - 2, k - 3 mod 4): run-to-run reproducible, a quarter of the
  // time of four waves taking turns (round 5: the fold is a fixed cost per workgroup -- it shows at the 8-GPU shard size).
#pragma unroll 1
  for (int ph = 0; ph < 4; ++ph) {
    const int kk = (wave + ph) & 3;
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      if (k != kk) continue;
#pragma unroll
      for (int db = 0; db < NDB; ++db) {
        const int col = 16 * db + j16;                    // C layout of the 16x16 fp32 MFMA: column lane & 15, rows 4 (lane >> 4) + reg
#pragma unroll
        for (int r = 0; r < 4; ++r) atomicAdd(&sum[(16 * k + 4 * q + r) * (2 * XP) + col], ldexp(acc[k][db][r], unscale[db]));
      }
      double o = occ[k];                                  // this lane's Gaussian j16 of block k, its quarter of the frames
      o += __shfl_xor(o, 16);
      o += __shfl_xor(o, 32);
      if (q == 0) atomicAdd(&sum[NB * 16 * 2 * XP + 16 * k + j16], o);
    }
    __syncthreads();
  }
  if (bad) atomicOr(a.err_flag, 1);
  __shared__ double s_ll[4];
  for (int o2 = 32; o2 > 0; o2 >>= 1) tot_ll += __shfl_xor(tot_ll, o2);
  if (lane == 0) s_ll[wave] = tot_ll;
  __syncthreads();
  const double block_ll = ((s_ll[0] + s_ll[1]) + s_ll[2]) + s_ll[3];
  if (it.ny == 1) {
    k3_wave_flush<NB>(a, sum, g0, G, D, tid);
    if (tid == 0) a.ll_part[pdf] = block_ll;
  } else {
    double* dst = a.part + (int64_t)it.slot * (NSUM + 1);
    for (int i = tid; i < NSUM; i += 256) dst[i] = sum[i];
    if (tid == 0) dst[NSUM] = block_ll;
  }
}

// ------------------------------------------------------------------------------------------
// k3_accumulate_block16 (round 6): the chunk-per-block form with BOTH phases on the fp16 matrix cores -- pdfs of 65..128 Gaussians at
// 40 < D <= 80 (BASELINE config #5: 10 000 pdfs x 128 Gaussians, D = 80), where a wave cannot hold the fp64 totals of a whole pdf.
// k3_accumulate_mfma spends ~10 k cycles per 64-frame chunk in fp32 MFMAs (phase A) and ~20 k in fp64 MFMAs (phase B: 64 cycles
// each, holding the SIMD's vector issue): 0.46 of the fp32 / fp64 matrix roofline was all there was to get (63 ms at 125 000 utterances).
// Here, as in k3_accumulate_wave16:
//   * phase A: ll[g][f] = gconst' + W' . [x' | x^2'] on v_mfma_f32_16x16x32_f16, operands scaled by exponents of the MODEL alone
//     (K3Args::pa_ex, pa_S) and split into two fp16 pieces without rescaling the residual (khg_k1_f16x2s.hip.inc), three partial
//     products into one fp32 accumulator.  A wave owns the Gaussian blocks w, w + 4, ... (16 Gaussians each): their W operands
//     stay in registers (40 per block), the chunk's feature planes sit in LDS once for the four waves;
//   * the softmax over the pdf's Gaussians combines the waves through LDS exactly as the fp32 form does;
//   * phase B: gamma'^T . [x' | x^2'] per 32 frames (K = 32: two 16-frame tiles), three partial products, the chunk's 64 frames
//     summed in the MFMA's fp32 accumulator, then widened into the wave's fp64 totals (registers, scaled units; 2^-(SG + ex)
//     applied at the flush: exact).
// 240 MFMAs of 16 cycles per chunk and wave instead of 320 + 320 of 32 / 64.  Numerics: as k3_accumulate_wave16 (products carry
// 22 + 22 bits; 64 of them are summed in fp32 before the fp64 add: ~1e-7 of a cell, inside the 2e-5 the statistics are held to).
// KQ = 20 (D <= 80, 160 columns = 5 k-steps) or 10 (D <= 40, 80 columns padded to 96 = 3 k-steps).
#ifndef K3B16_KO
#define K3B16_KO 0        // MEASUREMENT builds only (results are WRONG): knock-outs that price one part of k3_accumulate_block16 each --
#endif                    // 1 no phase B, 2 no phase A MFMAs, 4 no staging, 8 no feature gather, 32 no flush atomics, 64 no W set-up
template <int KQ, int NBW, int NWV>
__global__ __launch_bounds__(64 * NWV, 1) void k3_accumulate_block16(K3Args a) {
  constexpr int NT = 64 * NWV;                     // threads: NWV waves, wave w owns the Gaussian blocks w, w + NWV, ...
  extern __shared__ __attribute__((aligned(16))) float k3s[];
  constexpr int XP = 4 * KQ;                       // padded feature-row pitch (zero filled beyond D)
  constexpr int K2 = 2 * XP;                       // columns of [x | x^2] = contraction length of phase A
  constexpr int KPAD = (K2 + 31) / 32 * 32, KST = KPAD / 32;
  constexpr int NDB = K2 / 16;                     // 16-column blocks
  constexpr int XROW = KPAD + 8;                   // halves per frame row of phase A's planes (an odd number of 16-byte words)
  constexpr int XTR = K3_CHUNK + 8;                // halves per column row of phase B's planes
  constexpr int XHH = K3_CHUNK * XROW, XTH = K2 * XTR;    // halves per piece
  static_assert((XROW / 8) % 2 == 1 && (XTR / 8) % 2 == 1, "row pitches are odd multiples of 16 bytes");
  K3Item it;
  if (!k3_take_item(a, it)) return;
  const int pdf = it.pdf;
  const int64_t beg = a.pdf_start[pdf];
  const int nfr = (int)(a.pdf_start[pdf + 1] - beg);
  if (nfr == 0) return;
  const int D = a.D;
  const int g0 = a.gauss_off[pdf], G = a.gauss_off[pdf + 1] - g0;
  _Float16* xh = reinterpret_cast<_Float16*>(k3s);            // [piece 2][frame 64][XROW]
  _Float16* xt = xh + 2 * XHH;                                 // [piece 2][column K2][XTR]
  float* red = reinterpret_cast<float*>(xt + 2 * XTH);         // [NWV][64] per-wave per-frame max / sum
  float* fin = red + NWV * K3_CHUNK;                           // [64]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j16 = lane & 15, q = lane >> 4;
  const int nchunk = (nfr + K3_CHUNK - 1) / K3_CHUNK;

  // ---- this wave's Gaussians: block b = wave + NWV k; W' pieces as phase A's B operands (lane: Gaussian j16, k = 32 st + 8 q + e).
  // The pdf's parameter rows come into LDS by coalesced loads first (the planes' area, not yet in use): read straight from HBM, a lane's
  // 8 KST values are 32-byte pieces of 16 different rows -- 19 us per workgroup, 0.75 of 5.2 ms (profiles/r6_k3_block16_knockouts.txt) ----
  constexpr int GP = 16 * NBW * NWV;                            // Gaussians the workgroup has lanes for
  k3_f16x8 w1[NBW][KST], w2[NBW][KST];
  float gcv[NBW];
  {
    const int WP = D | 1;                                       // odd row pitch: a lane group's 16 rows fall on 16 banks
    float* wl = k3s;                                            // [2][GP][WP]: means_invvars | -0.5 inv_vars
    int* ewl = reinterpret_cast<int*>(wl + 2 * GP * WP);        // [K2] S - ex per column
    for (int idx = tid; idx < G * D; idx += NT) {
      const int g = idx / D, d = idx - g * D;
      float mi = 0.0f, nh = 0.0f;
      if (!(K3B16_KO & 64)) { mi = a.means_invvars[(int64_t)g0 * D + idx]; nh = a.nhalf_inv_vars[(int64_t)g0 * D + idx]; }
      wl[g * WP + d] = mi; wl[(GP + g) * WP + d] = nh;
    }
    for (int kp = tid; kp < K2; kp += NT) {
      const int var = kp >= XP, d = var ? kp - XP : kp;
      ewl[kp] = d < D ? a.pa_S - a.pa_ex[2 * d + var] : 0;
    }
    k3_block_sync();
#pragma unroll
    for (int k = 0; k < NBW; ++k) {
      const int g = 16 * (wave + NWV * k) + j16;
      const bool gv = g < G;
      gcv[k] = (gv ? a.gconsts[g0 + g] : -INFINITY) * a.pa_scale;
#pragma unroll
      for (int st = 0; st < KST; ++st) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int kp = 32 * st + 8 * q + e, var = kp >= XP, d = var ? kp - XP : kp;
          float v = 0.0f;
          if (kp < K2 && gv && d < D) v = ldexpf(wl[(var * GP + g) * WP + d], ewl[kp]);
          const _Float16 h1 = (_Float16)v;
          w1[k][st][e] = h1; w2[k][st][e] = (_Float16)(v - (float)h1);
        }
      }
    }
    k3_block_sync();
  }
  {                                                             // padding columns of phase A's planes stay zero
    const k3_f16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = tid; i < 2 * XHH / 8; i += NT) reinterpret_cast<k3_f16x8*>(xh)[i] = z;
  }
  f64x4 acc[NBW][NDB];         // fp64 totals in scaled units: column lane & 15 of block db, Gaussians 4 (lane >> 4) + r of block wave + NWV k
  double occ[NBW];
#pragma unroll
  for (int k = 0; k < NBW; ++k) {
    occ[k] = 0.0;
#pragma unroll
    for (int db = 0; db < NDB; ++db) acc[k][db] = f64x4{0, 0, 0, 0};
  }
  double tot_ll = 0.0;
  unsigned bad = 0;
  const float gs = a.pb_gscale;

  // A thread stages 2 x 2 micro-tiles (two adjacent frames x two adjacent dims) of the chunk's 64 x XP cells: micro-tile i = tid + NT j:
  // frame pair i / (XP / 2), dim pair i % (XP / 2).  The NEXT chunk's features are requested into registers as soon as this chunk's are
  // parked in LDS (always-valid addresses; the zero fill happens at the staging).
  constexpr int NMT = K3_CHUNK * XP / 4, NM = (NMT + NT - 1) / NT;    // micro-tiles of a chunk, per thread (the last round is partial at XP = 40)
  float pre[NM][4];                       // [micro-tile][frame 2][dim 2]
  float sx[NM][2], sx2[NM][2];            // 2^ex of the micro-tile's two dims (x', x^2')
  const bool even_d = (D & 1) == 0;
#pragma unroll
  for (int j = 0; j < NM; ++j)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int d = min(2 * (min(tid + NT * j, NMT - 1) % (XP / 2)) + c, D - 1);
      sx[j][c] = ldexpf(1.0f, a.pa_ex[2 * d]); sx2[j][c] = ldexpf(1.0f, a.pa_ex[2 * d + 1]);
    }
  // The gather is two dependent loads (frame id, then the feature row).  Both are requested AHEAD and in separate steps -- the ids of the
  // chunk after next while the next chunk's rows are requested with ids that arrived a chunk ago -- so that neither latency stands in a
  // chunk (asked for in one step, the rows' request itself waited ~1 us per chunk for the ids: 1.1 of 5.2 ms, profiles/r6_k3_block16_knockouts.txt).
  int fidn[NM][2];
  auto request_ids = [&](int c) {
    const int cfn = min(K3_CHUNK, nfr - c * K3_CHUNK);
#pragma unroll
    for (int j = 0; j < NM; ++j) {
      const int i = min(tid + NT * j, NMT - 1), f0 = 2 * (i / (XP / 2));
      fidn[j][0] = a.frame_ids[beg + c * K3_CHUNK + min(f0, cfn - 1)];
      fidn[j][1] = a.frame_ids[beg + c * K3_CHUNK + min(f0 + 1, cfn - 1)];
    }
  };
  auto request_rows = [&]() {
    if constexpr ((K3B16_KO & 8) != 0) { for (int j = 0; j < NM; ++j) for (int e = 0; e < 4; ++e) pre[j][e] = 1.0f; return; }
#pragma unroll
    for (int j = 0; j < NM; ++j) {
      const int i = min(tid + NT * j, NMT - 1), d0 = 2 * (i % (XP / 2));
      const int64_t fa = fidn[j][0], fb = fidn[j][1];
      if (even_d) {
        typedef float f2 __attribute__((ext_vector_type(2)));
        const int dd = min(d0, D - 2);
        const f2 va = *reinterpret_cast<const f2*>(a.feats + fa * D + dd), vb = *reinterpret_cast<const f2*>(a.feats + fb * D + dd);
        pre[j][0] = va[0]; pre[j][1] = va[1]; pre[j][2] = vb[0]; pre[j][3] = vb[1];
      } else {
        const int da = min(d0, D - 1), db = min(d0 + 1, D - 1);
        pre[j][0] = a.feats[fa * D + da]; pre[j][1] = a.feats[fa * D + db];
        pre[j][2] = a.feats[fb * D + da]; pre[j][3] = a.feats[fb * D + db];
      }
    }
  };
  if (it.y < nchunk) { request_ids(it.y); request_rows(); if (it.y + it.ny < nchunk) request_ids(it.y + it.ny); }
  k3_block_sync();
  for (int c = it.y; c < nchunk; c += it.ny) {
    const int cf = min(K3_CHUNK, nfr - c * K3_CHUNK);
    // ---- stage the chunk: the split planes in phase A's layout (frame rows) and in phase B's (column rows) ----
#pragma unroll
    for (int j = 0; j < NM; ++j) {
      typedef _Float16 h2v __attribute__((ext_vector_type(2)));
      const int i = tid + NT * j, f0 = 2 * (i / (XP / 2)), d0 = 2 * (i % (XP / 2));
      if (NM * NT != NMT && i >= NMT) continue;
      if constexpr ((K3B16_KO & 4) != 0) { asm volatile("" ::"v"(pre[j][0]), "v"(pre[j][1]), "v"(pre[j][2]), "v"(pre[j][3])); continue; }
      _Float16 h1[4], h2[4], g1[4], g2[4];                        // [frame 2][dim 2]: the two pieces of x' and of x^2'
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int f = f0 + (e >> 1), d = d0 + (e & 1);
        const float v = (f < cf && d < D) ? pre[j][e] : 0.0f;
        const float s1 = v * sx[j][e & 1], s2 = (v * v) * sx2[j][e & 1];        // fl(x^2) first (the reference's squares)
        h1[e] = (_Float16)s1; g1[e] = (_Float16)s2;
        h2[e] = (_Float16)(s1 - (float)h1[e]); g2[e] = (_Float16)(s2 - (float)g1[e]);
      }
#pragma unroll
      for (int ff = 0; ff < 2; ++ff) {                            // phase A's layout: [piece][frame][column]
        _Float16* r1 = xh + (f0 + ff) * XROW + d0;
        *reinterpret_cast<h2v*>(r1) = h2v{h1[2 * ff], h1[2 * ff + 1]};
        *reinterpret_cast<h2v*>(r1 + XHH) = h2v{h2[2 * ff], h2[2 * ff + 1]};
        *reinterpret_cast<h2v*>(r1 + XP) = h2v{g1[2 * ff], g1[2 * ff + 1]};
        *reinterpret_cast<h2v*>(r1 + XHH + XP) = h2v{g2[2 * ff], g2[2 * ff + 1]};
      }
#pragma unroll
      for (int dd = 0; dd < 2; ++dd) {                            // phase B's layout: [piece][column][frame]
        _Float16* c1 = xt + (d0 + dd) * XTR + f0;
        *reinterpret_cast<h2v*>(c1) = h2v{h1[dd], h1[2 + dd]};
        *reinterpret_cast<h2v*>(c1 + XTH) = h2v{h2[dd], h2[2 + dd]};
        *reinterpret_cast<h2v*>(c1 + XP * XTR) = h2v{g1[dd], g1[2 + dd]};
        *reinterpret_cast<h2v*>(c1 + XTH + XP * XTR) = h2v{g2[dd], g2[2 + dd]};
      }
    }
    if (c + it.ny < nchunk) { request_rows(); if (c + 2 * it.ny < nchunk) request_ids(c + 2 * it.ny); }
    k3_block_sync();
    // ---- phase A: ll[k][ft][r] for Gaussian 16 (wave + 4 k) + j16, frame 16 ft + 4 q + r (scaled units 2^S) ----
    f32x4 ll[NBW][4];
#pragma unroll
    for (int k = 0; k < NBW; ++k)
#pragma unroll
      for (int ft = 0; ft < 4; ++ft) ll[k][ft] = f32x4{gcv[k], gcv[k], gcv[k], gcv[k]};
#pragma unroll
    for (int st = 0; st < ((K3B16_KO & 2) ? 0 : KST); ++st) {
#pragma unroll
      for (int ft = 0; ft < 4; ++ft) {
        const k3_f16x8 x1 = *reinterpret_cast<const k3_f16x8*>(xh + (16 * ft + j16) * XROW + 32 * st + 8 * q);
        const k3_f16x8 x2 = *reinterpret_cast<const k3_f16x8*>(xh + XHH + (16 * ft + j16) * XROW + 32 * st + 8 * q);
#pragma unroll
        for (int k = 0; k < NBW; ++k) {
          ll[k][ft] = __builtin_amdgcn_mfma_f32_16x16x32_f16(x2, w1[k][st], ll[k][ft], 0, 0, 0);
          ll[k][ft] = __builtin_amdgcn_mfma_f32_16x16x32_f16(x1, w2[k][st], ll[k][ft], 0, 0, 0);
          ll[k][ft] = __builtin_amdgcn_mfma_f32_16x16x32_f16(x1, w1[k][st], ll[k][ft], 0, 0, 0);
        }
      }
    }
    // ---- softmax over the pdf's Gaussians, frame by frame (eigen.cc:20-32): this wave's blocks in lane + DPP row, the waves through LDS ----
#pragma unroll
    for (int ft = 0; ft < 4; ++ft)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float m = ll[0][ft][r];
#pragma unroll
        for (int k = 1; k < NBW; ++k) m = fmaxf(m, ll[k][ft][r]);
        m = k3_row_max(m);
        if (j16 == 0) red[wave * K3_CHUNK + 16 * ft + 4 * q + r] = m;
      }
    k3_block_sync();
    if (tid < K3_CHUNK) {
      float v = red[tid];
#pragma unroll
      for (int w2 = 1; w2 < NWV; ++w2) v = fmaxf(v, red[w2 * K3_CHUNK + tid]);
      fin[tid] = v;
    }
    k3_block_sync();
    float mx[4][4];
#pragma unroll
    for (int ft = 0; ft < 4; ++ft)
#pragma unroll
      for (int r = 0; r < 4; ++r) mx[ft][r] = fin[16 * ft + 4 * q + r];
    k3_block_sync();
#pragma unroll
    for (int ft = 0; ft < 4; ++ft)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float ssum = 0.0f;
#pragma unroll
        for (int k = 0; k < NBW; ++k) {
          const float e = __builtin_amdgcn_exp2f((ll[k][ft][r] - mx[ft][r]) * a.pa_c1);   // (v - max).exp(); exp(-inf) = 0 for padding
          ll[k][ft][r] = e;
          ssum += e;
        }
        ssum = k3_row_sum(ssum);
        if (j16 == 0) red[wave * K3_CHUNK + 16 * ft + 4 * q + r] = ssum;
      }
    k3_block_sync();
    if (tid < K3_CHUNK) {
      float v = red[tid];
#pragma unroll
      for (int w2 = 1; w2 < NWV; ++w2) v += red[w2 * K3_CHUNK + tid];
      fin[tid] = v;
    }
    k3_block_sync();
#pragma unroll
    for (int ft = 0; ft < 4; ++ft)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = 16 * ft + 4 * q + r;
        const float ssum = fin[f];
        if (wave == 0 && j16 == 0 && f < cf) {
          const float llf = __logf(ssum) + mx[ft][r] * a.pa_inv;                 // eigen.cc:28
          bad |= !(fabsf(llf) <= 3.0e38f) ? 1u : 0u;                             // diag-gmm.cc:385-387
          tot_ll += (double)(llf * a.weight);                                    // mle-am-diag-gmm.cc:49
        }
        // eigen.cc:31 (e / sum) and mle-diag-gmm.cc:153 (* weight) as ONE correctly rounded division per frame and a multiply per Gaussian
        const float scale = f < cf ? a.weight / ssum : 0.0f;
#pragma unroll
        for (int k = 0; k < NBW; ++k) ll[k][ft][r] = ll[k][ft][r] * scale;
      }
    // ---- phase B: part[k][db] = sum over the chunk's 64 frames of gamma'^T . [x' | x^2'], then into the fp64 totals ----
    k3_f16x8 ga1[NBW][2], ga2[NBW][2];
#pragma unroll
    for (int k = 0; k < NBW; ++k)
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float g = e < 4 ? ll[k][2 * h][e] : ll[k][2 * h + 1][e - 4];      // K slot (q, e): frame 4 q + (e & 3) of tile 2 h + (e >> 2)
          occ[k] += (double)g;                                                    // mle-diag-gmm.cc:132
          const float gsc = g * gs;
          const _Float16 h1 = (_Float16)gsc;
          ga1[k][h][e] = h1; ga2[k][h][e] = (_Float16)(gsc - (float)h1);
        }
    f32x4 prev[NBW];
#pragma unroll
    for (int db = 0; db < ((K3B16_KO & 1) ? 0 : NDB); ++db) {
      const _Float16* cb = xt + (16 * db + j16) * XTR + 4 * q;                  // this lane's column: frames 4 q .. 4 q + 3 of each 16-frame tile
      f32x4 cur[NBW];
#pragma unroll
      for (int k = 0; k < NBW; ++k) cur[k] = f32x4{0, 0, 0, 0};
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        typedef _Float16 h4 __attribute__((ext_vector_type(4)));
        const h4 a0 = *reinterpret_cast<const h4*>(cb + 32 * h), a1 = *reinterpret_cast<const h4*>(cb + 32 * h + 16);
        const h4 b0 = *reinterpret_cast<const h4*>(cb + XTH + 32 * h), b1 = *reinterpret_cast<const h4*>(cb + XTH + 32 * h + 16);
        k3_f16x8 xb1, xb2;
#pragma unroll
        for (int e = 0; e < 4; ++e) { xb1[e] = a0[e]; xb1[4 + e] = a1[e]; xb2[e] = b0[e]; xb2[4 + e] = b1[e]; }
#pragma unroll
        for (int k = 0; k < NBW; ++k) {
          cur[k] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ga1[k][h], xb2, cur[k], 0, 0, 0);
          cur[k] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ga2[k][h], xb1, cur[k], 0, 0, 0);
          cur[k] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ga1[k][h], xb1, cur[k], 0, 0, 0);
        }
      }
      if (db > 0) {                                                             // the PREVIOUS column block's sums into the fp64 totals, under this block's MFMAs
#pragma unroll
        for (int k = 0; k < NBW; ++k)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[k][db - 1][r] += (double)prev[k][r];
      }
#pragma unroll
      for (int k = 0; k < NBW; ++k) prev[k] = cur[k];
    }
    if constexpr ((K3B16_KO & 1) == 0) {
#pragma unroll
    for (int k = 0; k < NBW; ++k)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[k][NDB - 1][r] += (double)prev[k][r];
    } else { asm volatile("" ::"v"(ga1[0][0]), "v"(ga2[0][0]), "v"(ga1[0][1]), "v"(ga2[0][1])); }
    k3_block_sync();          // this chunk's LDS reads are done before the next staging overwrites the planes
  }
  // ---- flush: one fp64 atomic per cell, unscaling on the way (powers of two: exact).  C layout of the 16x16 MFMA: column lane & 15,
  //      rows 4 (lane >> 4) + reg (Gaussian within the block) ----
#pragma unroll
  for (int k = 0; k < NBW; ++k) {
    const int gb = 16 * (wave + NWV * k);
#pragma unroll
    for (int db = 0; db < NDB; ++db) {
      const int col = 16 * db + j16, var = col >= XP, d = var ? col - XP : col;
      if (d < D) {
        const int unscale = -(a.pb_SG + a.pa_ex[2 * d + var]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int g = gb + 4 * q + r;
          if (g < G && !((K3B16_KO & 32) && acc[k][db][r] != -1.0)) atomicAdd((var ? a.var_acc : a.mean_acc) + (int64_t)(g0 + g) * D + d, ldexp(acc[k][db][r], unscale));
        }
      }
    }
    double o = occ[k];                                  // this lane's Gaussian j16 of the block, its quarter of the frames
    o += __shfl_xor(o, 16);
    o += __shfl_xor(o, 32);
    if (q == 0 && gb + j16 < G) atomicAdd(a.occ + g0 + gb + j16, o);
  }
  if (bad) atomicOr(a.err_flag, 1);
  if (wave == 0) {
    for (int o2 = 32; o2 > 0; o2 >>= 1) tot_ll += __shfl_xor(tot_ll, o2);
    if (lane == 0 && tot_ll != 0.0) atomicAdd(&a.scalars[1], tot_ll);
  }
  if (tid == 0 && it.y == 0) atomicAdd(&a.scalars[0], (double)nfr * (double)a.weight);  // mle-am-diag-gmm.cc:50
}

// Pdfs cut into several slices (small models: all of them; large ones: the pdfs far above the average): add the parked slices in
// slice order, then flush like a single block.
template <int NB>
__global__ __launch_bounds__(256) void k3_wave_finalize(K3Args a) {
  constexpr int XP = 40, NSUM = NB * 16 * 2 * XP + NB * 16;
  __shared__ double sum[NSUM];
  const int pdf = a.pdf0 + blockIdx.x, tid = threadIdx.x;
  if (a.pdf_start[pdf + 1] == a.pdf_start[pdf]) return;       // the accumulate blocks of an empty pdf returned early
  const int i0 = a.item_off[pdf], ny = a.item_off[pdf + 1] - i0;
  if (ny <= 1) return;                                        // its one block flushed by itself
  const double* src = a.part + (int64_t)a.items[i0].slot * (NSUM + 1);
  for (int i = tid; i < NSUM; i += 256) {
    double v = 0.0;
    for (int y = 0; y < ny; ++y) v += src[(int64_t)y * (NSUM + 1) + i];
    sum[i] = v;
  }
  __syncthreads();
  const int g0 = a.gauss_off[pdf], G = a.gauss_off[pdf + 1] - g0;
  k3_wave_flush<NB>(a, sum, g0, G, a.D, tid);
  if (tid == 0) {
    double v = 0.0;
    for (int y = 0; y < ny; ++y) v += src[(int64_t)y * (NSUM + 1) + NSUM];
    a.ll_part[pdf] = v;
  }
}

// total_frames and total_log_like of the wave form: per-pdf values folded by one block in a fixed order
// (strided partial sums, then a tree), one atomic each -- reproducible, unlike per-block atomics on one double.
__global__ __launch_bounds__(1024) void k3_wave_scalars(K3Args a, int cls_lo, int cls_hi) {
  __shared__ double s_l[1024], s_f[1024];
  const int tid = threadIdx.x;
  double l = 0.0, f = 0.0;
  for (int p = tid; p < a.P; p += 1024) {
    const int Gp = a.gauss_off[p + 1] - a.gauss_off[p];
    if (Gp <= cls_lo || Gp > cls_hi) continue;                         // the other class's form counts its own frames
    l += a.ll_part[p];
    f += (double)(a.pdf_start[p + 1] - a.pdf_start[p]) * (double)a.weight;     // mle-am-diag-gmm.cc:50
  }
  s_l[tid] = l; s_f[tid] = f;
  __syncthreads();
  for (int s = 512; s > 0; s >>= 1) {
    if (tid < s) { s_l[tid] += s_l[tid + s]; s_f[tid] += s_f[tid + s]; }
    __syncthreads();
  }
  if (tid == 0) {
    if (s_l[0] != 0.0) atomicAdd(&a.scalars[1], s_l[0]);
    if (s_f[0] != 0.0) atomicAdd(&a.scalars[0], s_f[0]);
  }
}
