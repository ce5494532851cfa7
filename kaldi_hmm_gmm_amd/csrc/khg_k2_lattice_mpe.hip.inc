// K2M: MPE / sMBR posteriors of device-resident raw lattices (khg_lattices_mpe_posteriors: LatticeForwardBackwardMpeVariants /
// lattice-to-mpe-post, lattice-to-smbr-post).  The rule is DESIGN.md section 7k.  The likelihood part -- the admissibility check,
// alpha, the total, beta -- and the merge are section 7g's: the device functions k2_lattice_post_fb itself calls
// (khg_k2_lattice_post.hip.inc), which makes tot_like, the statuses, the live flags and the list structure bit-equal to
// khg_lattices_posteriors'.  Two more passes through the same sweep run in the linear domain: the forward expected accuracy A and the
// backward one B, a state's sum taken over its arcs in order (a hub state: lane-strided, then the butterfly).  The signed value
// d = g (A[src] + acc + B[next] - avg) goes where k2_lattice_post_fb puts g, so k2_lattice_post_fill merges it as it is.  An arc's
// frame accuracy (0 or 1) waits in the `rank` words, which nothing else uses before the merge.  No atomics.  LDS holds five doubles per
// state beside the staged lattice when 40 N + 4 (3 N + 4 A) bytes fit the limit; otherwise (or KHG_OPT_LAT_OPS_LDS = 1) the same code
// runs on HBM scratch.

struct PoMpeArgs {
  PoArgs po;
  double *accA, *accB;                 // HBM scratch, [chunk states]
  const int32_t* ref;                  // the reference alignments, utterance u's at ref_off[u] (one id in 1 .. num_tids per frame)
  const int64_t* ref_off;              // [U + 1]
  const int32_t* tab;                  // [num_tids + 1]: 2 * class + (the id's phone is a silence phone); class = phone (MPFE) or pdf (SMBR)
  const int32_t* no_ref;               // [U]: != 0 -> KHG_LAT_NO_REF
  double* avg;                         // [U]
  int32_t one_silence_class;
};

__device__ __forceinline__ void po_mpe_fail(const PoMpeArgs& p, const PoView& w, int st) {
  if (threadIdx.x == 0) p.avg[w.u] = 0.0;
  po_fail(p.po, w, st);
}

// ---- sum of add(sum, i) over i = 0 .. n - 1 from 0: one lane in order, or one wave (all 64 lanes call it: lane-strided, then a
// butterfly whose partners add the same two numbers) ----
template <class Add>
__device__ __forceinline__ double po_sum_lane(int n, Add add) {
#pragma clang fp contract(off)
  double sum = 0.0;
  for (int i = 0; i < n; ++i) sum = add(sum, i);
  return sum;
}
template <class Add>
__device__ __forceinline__ double po_sum_wave(int n, Add add, int lane) {
#pragma clang fp contract(off)
  double sum = 0.0;
  for (int i = lane; i < n; i += 64) sum = add(sum, i);
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  return sum;
}

__global__ __launch_bounds__(PO_NT) void k2_lattice_post_mpe(PoMpeArgs q) {
#pragma clang fp contract(off)
  extern __shared__ double po_lds[];
  __shared__ double sh_tot, sh_avg;
  const PoArgs& p = q.po;
  const double NINF = -__builtin_huge_val();
  const float FINF = __builtin_huge_valf();
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const PoView w = po_open<5>(p, po_lds);
  const LoView& v = w.v;
  const int u = w.u, N = w.N, A = w.A, T = w.T;
  if (N == 0 || v.start < 0) { po_mpe_fail(q, w, KHG_LAT_NO_PATH); return; }
  if (q.no_ref[u] != 0) { po_mpe_fail(q, w, KHG_LAT_NO_REF); return; }
  double* fwd = w.in_lds ? po_lds + 3 * (size_t)N : q.accA + w.s0;
  double* bwd = w.in_lds ? po_lds + 4 * (size_t)N : q.accB + w.s0;
  const double *alpha = w.alpha, *beta = w.beta;
  const int32_t *asrc = w.asrc, *rank = w.rank;
  const double gs = w.gs, as = w.as;
  if (!po_admissible(w)) { po_mpe_fail(q, w, KHG_LAT_EPS_LOOP); return; }
  po_frames(w);
  for (int s = tid; s < N; s += PO_NT) { fwd[s] = 0.0; bwd[s] = 0.0; }
  // the frame accuracy of every arc (the reference has T ids: no_ref otherwise)
  {
    const int32_t* ref = q.ref + q.ref_off[u];
    for (int a = tid; a < A; a += PO_NT) {
      const int il = v.il[a], t = v.frame[asrc[a]];
      int acc = 0;
      if (il != 0 && t < T) {
        const int mine = q.tab[il], r = q.tab[ref[t]];
        const bool match = (mine >> 1) == (r >> 1);
        acc = q.one_silence_class ? (match || ((mine & 1) && (r & 1))) : (match && !(mine & 1));
      }
      w.rank[a] = acc;
    }
  }
  __syncthreads();

  bool settled;
  const double tot = po_alpha_total_beta(w, &sh_tot, &settled);
  if (!settled) { po_mpe_fail(q, w, KHG_LAT_EPS_LOOP); return; }
  if (tot == NINF) { po_mpe_fail(q, w, KHG_LAT_NO_PATH); return; }

  // the forward accuracy: A[s] = sum over the in-arcs from reached states of exp((alpha[src] + w) - alpha[s]) (A[src] + acc)
  {
    auto count = [&](int s, double mine, int deg) { return s != v.start && mine != NINF ? deg : 0; };
    auto add = [&](double sum, double mine, int pos) {
      const int a = w.ia[pos], src = asrc[a];
      const double al = alpha[src];
      if (al != NINF) sum += exp((al + po_w(v, gs, as, a)) - mine) * (fwd[src] + (double)rank[a]);
      return sum;
    };
    (void)po_sweep<true>(w, fwd,
                         [&](int s, int, int i0, int deg) {
                           const double mine = alpha[s];
                           return po_sum_lane(count(s, mine, deg), [&](double sum, int i) { return add(sum, mine, i0 + i); });
                         },
                         [&](int s, int, int i0, int deg, int ln) {
                           const double mine = alpha[s];
                           return po_sum_wave(count(s, mine, deg), [&](double sum, int i) { return add(sum, mine, i0 + i); }, ln);
                         });
  }
  if (tid < 64) {                                                     // the criterion: the expected accuracy of a path
    const int lo = w.fs[T];
    const double sum = po_sum_wave(N - lo, [&](double sum, int i) {
      const float c = v.fin[lo + i];
      const double al = alpha[lo + i];
      if (c != FINF && al != NINF) sum += exp((al + -(gs * (double)c)) - tot) * fwd[lo + i];
      return sum;
    }, lane);
    if (lane == 0) sh_avg = sum;
  }
  __syncthreads();
  const double avg = sh_avg;

  // the backward accuracy: B[s] = sum over the out-arcs to states that reach the end of exp((w + beta[next]) - beta[s]) (acc + B[next])
  {
    auto count = [&](double mine, int deg) { return mine != NINF ? deg : 0; };
    auto add = [&](double sum, double mine, int a) {
      const int nx = v.next[a];
      const double be = beta[nx];
      if (be != NINF) sum += exp((po_w(v, gs, as, a) + be) - mine) * ((double)rank[a] + bwd[nx]);
      return sum;
    };
    (void)po_sweep<false>(w, bwd,
                          [&](int s, int, int e0, int deg) {
                            const double mine = beta[s];
                            return po_sum_lane(count(mine, deg), [&](double sum, int i) { return add(sum, mine, e0 + i); });
                          },
                          [&](int s, int, int e0, int deg, int ln) {
                            const double mine = beta[s];
                            return po_sum_wave(count(mine, deg), [&](double sum, int i) { return add(sum, mine, e0 + i); }, ln);
                          });
  }

  // the signed arc values; an arc is live when both of its ends are reached
  for (int a = tid; a < A; a += PO_NT) {
    const int src = asrc[a], nx = v.next[a];
    const double al = alpha[src], be = beta[nx];
    const bool live = al != NINF && be != NINF;
    double d = 0.0;
    if (live) {
      const double g = exp(((al + po_w(v, gs, as, a)) + be) - tot);
      d = g * (((fwd[src] + (double)rank[a]) + bwd[nx]) - avg);
    }
    p.arc_post[w.a0 + a] = d;
    w.flag[a] = live && v.il[a] != 0 && v.frame[src] < T ? 1 : 0;
  }
  __syncthreads();
  const int entries = po_merge(w);
  if (tid == 0) { po_done(p, w, entries, tot); q.avg[u] = avg; }
}
