// K3 from posteriors (khg_acc_stats_post, DESIGN.md 7h): gmm-acc-stats.  Every entry (feature row, transition-id, weight) of a
// khg_posteriors handle adds what one weighted frame of an alignment adds:
//   kaldi-hmm-gmm/csrc/mle-am-diag-gmm.cc:41-52   AccumulateForGmm(model, data, pdf, weight)
//   kaldi-hmm-gmm/csrc/transition-model.h:183-189 Accumulate(prob = weight, tid)
//
// Pipeline: k3_post_flatten (khg_lattices.hip, which knows the handle's layout) -> e_row / e_tid / e_w [E] in utterance, frame, entry
// order -> k3_post_keys (the (pdf, entry) pairs and the weighted transition statistics) -> the stable radix sort and k3_bounds of the
// alignment path, on the entries -> the POST instantiations of k3_accumulate_mfma / k3_accumulate (khg_k3_accstats.hip.inc), whose
// buckets hold entry numbers: a block gathers feats[e_row[e]] and e_w[e], and the entry's weight stands where the call's one weight
// stands for an alignment.  Stability keeps a pdf's entries in entry order, so the statistics are reproducible run to run.

// key = pdf of the entry's id (P: an entry the flatten pass dropped, or one whose weight is +-0: it adds nothing), value = the entry's
// number; trans_acc[tid] += (double)w per entry.  The sum of widened floats does not depend on its order anywhere near the
// statistics' tolerance, so the adds are fp64 atomics: into a per-workgroup histogram in LDS where the transition model is small
// (LDSHIST: num_tids <= K3_LDS_TIDS, dynamic LDS of (num_tids + 1) doubles), flushed once per workgroup, else straight into the block.
template <bool LDSHIST>
__global__ __launch_bounds__(256) void k3_post_keys(K3Args a, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  extern __shared__ __attribute__((aligned(16))) double k3p_hist[];
  if constexpr (LDSHIST) {
    for (int i = threadIdx.x; i <= a.num_tids; i += 256) k3p_hist[i] = 0.0;
    __syncthreads();
  }
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.N; i += stride) {
    const int tid = a.ali[i];
    const float w = a.e_w[i];
    int pdf = a.P;
    if (tid >= 1 && tid <= a.num_tids) {
      const int p = a.id2pdf[tid];
      if (p >= 0 && p < a.P) {
        if (w != 0.0f) {
          pdf = p;
          if constexpr (LDSHIST) atomicAdd(&k3p_hist[tid], (double)w);
          else atomicAdd(&a.trans_acc[tid], (double)w);
        }
      } else atomicOr(a.err_flag, 4);
    }
    keys[i] = (uint32_t)pdf; vals[i] = (uint32_t)i;
  }
  if constexpr (LDSHIST) {
    __syncthreads();
    for (int i = threadIdx.x; i <= a.num_tids; i += 256) {
      const double c = k3p_hist[i];
      if (c != 0.0) atomicAdd(&a.trans_acc[i], c);
    }
  }
}
