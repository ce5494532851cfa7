// K2M: MPE / sMBR posteriors of device-resident raw lattices (khg_lattices_mpe_posteriors: LatticeForwardBackwardMpeVariants /
// lattice-to-mpe-post, lattice-to-smbr-post).  The rule is DESIGN.md section 7k.  The likelihood part -- the admissibility check,
// alpha, the total, beta, and the plain arc posterior g -- is section 7g's, statement for statement k2_lattice_post_fb's (kept as a
// copy here so that the kernel khg_lattices_posteriors launches stays the code it was), which makes tot_like, the statuses, the live
// flags and the list structure bit-equal to khg_lattices_posteriors'.  Two more passes of the same shape run in the linear domain:
// the forward expected accuracy A and the backward one B, a state's sum taken over its arcs in order (a hub state: lane-strided, then
// the butterfly), the epsilon arcs inside a frame closed by the same Jacobi rounds.  The signed value d = g (A[src] + acc + B[next] -
// avg) goes where k2_lattice_post_fb puts g, so k2_lattice_post_fill merges it as it is.  An arc's frame accuracy (0 or 1) waits in
// the `rank` words, which nothing else uses before the merge.  No atomics.  LDS holds five doubles per state beside the staged lattice
// when 40 N + 4 (3 N + 4 A) bytes fit the limit; otherwise (or KHG_OPT_LAT_OPS_LDS = 1) the same code runs on HBM scratch.

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

__device__ __forceinline__ void po_mpe_fail(const PoMpeArgs& p, int u, int b, int64_t a0, int A, int st) {
  if (threadIdx.x == 0) p.avg[u] = 0.0;
  po_fail(p.po, u, b, a0, A, st);
}

__global__ __launch_bounds__(PO_NT) void k2_lattice_post_mpe(PoMpeArgs q) {
#pragma clang fp contract(off)
  extern __shared__ double po_lds[];
  __shared__ double sh_tot, sh_avg;
  const PoArgs& p = q.po;
  const double NINF = -__builtin_huge_val();
  const float FINF = __builtin_huge_valf();
  const int b = (int)blockIdx.x, u = p.lo.u0 + b, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t s0 = p.lo.state_off[u] - p.lo.s_base, a0 = p.lo.arc_off[u] - p.lo.a_base;
  const int N = (int)(p.lo.state_off[u + 1] - p.lo.state_off[u]), A = (int)(p.lo.arc_off[u + 1] - p.lo.arc_off[u]);
  const int64_t need = 40 * (int64_t)N + 4 * (3 * (int64_t)N + 4 * (int64_t)A);
  const bool in_lds = need <= (int64_t)p.lo.lds_bytes;                                   // workgroup-uniform
  const LoView v = lo_view(p.lo, u, in_lds ? reinterpret_cast<int32_t*>(po_lds + 5 * (size_t)N) : nullptr);
  if (N == 0 || v.start < 0) { po_mpe_fail(q, u, b, a0, A, KHG_LAT_NO_PATH); return; }
  if (q.no_ref[u] != 0) { po_mpe_fail(q, u, b, a0, A, KHG_LAT_NO_REF); return; }
  double* alpha = in_lds ? po_lds : p.alpha + s0;
  double* beta = in_lds ? po_lds + N : p.beta + s0;
  double* row = in_lds ? po_lds + 2 * (size_t)N : p.row + s0;
  double* fwd = in_lds ? po_lds + 3 * (size_t)N : q.accA + s0;
  double* bwd = in_lds ? po_lds + 4 * (size_t)N : q.accB + s0;
  const int32_t* asrc = p.arc_src + a0;
  const int32_t* ib = p.in_begin + s0 + b;
  const int32_t* ia = p.in_arc + a0;
  const double gs = p.gs, as = p.as;
  // admissible: every epsilon arc goes to a higher state
  {
    int bad = 0;
    for (int a = tid; a < A; a += PO_NT) if (v.il[a] == 0 && v.next[a] <= asrc[a]) bad = 1;
    if (__syncthreads_or(bad)) { po_mpe_fail(q, u, b, a0, A, KHG_LAT_EPS_LOOP); return; }
  }
  const int64_t f0 = p.lo.ali_off[u] - p.f_base;
  const int T = (int)(p.lo.ali_off[u + 1] - p.lo.ali_off[u]);        // the last state's frame
  int32_t* fs = p.fstate + f0 + 2 * (int64_t)b;                       // [T + 2]: frame f holds the states fs[f] .. fs[f + 1]
  int32_t* fc = p.fcnt + f0;                                          // [T]
  int32_t* flag = p.flag + a0;
  int32_t* rank = p.rank + a0;
  for (int s = tid; s < N; s += PO_NT) {
    const int f = v.frame[s], pf = s ? v.frame[s - 1] : -1;
    for (int g = pf + 1; g <= f; ++g) fs[g] = s;
    alpha[s] = NINF; beta[s] = NINF; fwd[s] = 0.0; bwd[s] = 0.0;
  }
  for (int t = tid; t < T; t += PO_NT) fc[t] = 0;
  if (tid == 0) fs[T + 1] = N;
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
      rank[a] = acc;
    }
  }
  __syncthreads();

  int broken = 0;
  for (int f = 0; f <= T && !broken; ++f) {                           // forward
    const int lo = fs[f], hi = fs[f + 1];
    int has_eps = 0;
    for (int round = 0;; ++round) {
      int changed = 0, eps = 0;
      for (int s = lo + tid; s < hi; s += PO_NT) {                    // lanes over states
        const int i0 = ib[s], deg = ib[s + 1] - i0;
        if (deg > PO_HUB) continue;
        if (round == 0) for (int i = 0; i < deg; ++i) eps |= v.il[ia[i0 + i]] == 0;
        const double val = po_lse_lane(s == v.start ? 0.0 : NINF, deg, [&](int i) { const int a = ia[i0 + i]; return alpha[asrc[a]] + po_w(v, gs, as, a); });
        row[s] = val;
        changed |= po_differs(val, alpha[s]);
      }
      for (int s = lo + wave; s < hi; s += PO_NT / 64) {              // hub states: the wave over a state's in-arcs
        const int i0 = ib[s], deg = ib[s + 1] - i0;
        if (deg <= PO_HUB) continue;
        if (round == 0) for (int i = lane; i < deg; i += 64) eps |= v.il[ia[i0 + i]] == 0;
        const double val = po_lse_wave(s == v.start ? 0.0 : NINF, deg, [&](int i) { const int a = ia[i0 + i]; return alpha[asrc[a]] + po_w(v, gs, as, a); }, lane);
        if (lane == 0) { row[s] = val; changed |= po_differs(val, alpha[s]); }
      }
      if (round == 0) has_eps = __syncthreads_or(eps);               // (the reduction gives 0 or 1: one call per flag)
      if (!__syncthreads_or(changed)) break;                          // no value's bits changed
      for (int s = lo + tid; s < hi; s += PO_NT) alpha[s] = row[s];
      __syncthreads();
      if (!has_eps) break;
      if (round > hi - lo) { broken = 1; break; }                     // (not reached on an admissible lattice)
    }
  }
  if (broken) { po_mpe_fail(q, u, b, a0, A, KHG_LAT_EPS_LOOP); return; }
  if (wave == 0) {                                                    // the total over the last frame's final states
    const int lo = fs[T];
    const double t = po_lse_wave(NINF, N - lo, [&](int i) { const float c = v.fin[lo + i]; return c == FINF ? NINF : alpha[lo + i] + -(gs * (double)c); }, lane);
    if (lane == 0) sh_tot = t;
  }
  __syncthreads();
  const double tot = sh_tot;
  if (tot == NINF) { po_mpe_fail(q, u, b, a0, A, KHG_LAT_NO_PATH); return; }

  for (int f = T; f >= 0; --f) {                                      // backward: the same over out-arcs
    const int lo = fs[f], hi = fs[f + 1];
    int has_eps = 0;
    for (int round = 0;; ++round) {
      int changed = 0, eps = 0;
      for (int s = lo + tid; s < hi; s += PO_NT) {
        const int e0 = v.abeg[s], deg = lo_aend(v, s) - e0;
        if (deg > PO_HUB) continue;
        if (round == 0) for (int i = 0; i < deg; ++i) eps |= v.il[e0 + i] == 0;
        const float c = v.fin[s];
        const double init = f == T && c != FINF ? -(gs * (double)c) : NINF;
        const double val = po_lse_lane(init, deg, [&](int i) { const int a = e0 + i; return po_w(v, gs, as, a) + beta[v.next[a]]; });
        row[s] = val;
        changed |= po_differs(val, beta[s]);
      }
      for (int s = lo + wave; s < hi; s += PO_NT / 64) {
        const int e0 = v.abeg[s], deg = lo_aend(v, s) - e0;
        if (deg <= PO_HUB) continue;
        if (round == 0) for (int i = lane; i < deg; i += 64) eps |= v.il[e0 + i] == 0;
        const float c = v.fin[s];
        const double init = f == T && c != FINF ? -(gs * (double)c) : NINF;
        const double val = po_lse_wave(init, deg, [&](int i) { const int a = e0 + i; return po_w(v, gs, as, a) + beta[v.next[a]]; }, lane);
        if (lane == 0) { row[s] = val; changed |= po_differs(val, beta[s]); }
      }
      if (round == 0) has_eps = __syncthreads_or(eps);
      if (!__syncthreads_or(changed)) break;
      for (int s = lo + tid; s < hi; s += PO_NT) beta[s] = row[s];
      __syncthreads();
      if (!has_eps || round > hi - lo) break;
    }
  }

  // the forward accuracy: A[s] = sum over the in-arcs from reached states of exp((alpha[src] + w) - alpha[s]) (A[src] + acc)
  for (int f = 0; f <= T; ++f) {
    const int lo = fs[f], hi = fs[f + 1];
    int has_eps = 0;
    for (int round = 0;; ++round) {
      int changed = 0, eps = 0;
      for (int s = lo + tid; s < hi; s += PO_NT) {
        const int i0 = ib[s], deg = ib[s + 1] - i0;
        if (deg > PO_HUB) continue;
        if (round == 0) for (int i = 0; i < deg; ++i) eps |= v.il[ia[i0 + i]] == 0;
        const double mine = alpha[s];
        double sum = 0.0;
        if (s != v.start && mine != NINF)
          for (int i = 0; i < deg; ++i) {
            const int a = ia[i0 + i], src = asrc[a];
            const double al = alpha[src];
            if (al != NINF) sum += exp((al + po_w(v, gs, as, a)) - mine) * (fwd[src] + (double)rank[a]);
          }
        row[s] = sum;
        changed |= po_differs(sum, fwd[s]);
      }
      for (int s = lo + wave; s < hi; s += PO_NT / 64) {
        const int i0 = ib[s], deg = ib[s + 1] - i0;
        if (deg <= PO_HUB) continue;
        if (round == 0) for (int i = lane; i < deg; i += 64) eps |= v.il[ia[i0 + i]] == 0;
        const double mine = alpha[s];
        double sum = 0.0;
        if (s != v.start && mine != NINF)
          for (int i = lane; i < deg; i += 64) {
            const int a = ia[i0 + i], src = asrc[a];
            const double al = alpha[src];
            if (al != NINF) sum += exp((al + po_w(v, gs, as, a)) - mine) * (fwd[src] + (double)rank[a]);
          }
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        if (lane == 0) { row[s] = sum; changed |= po_differs(sum, fwd[s]); }
      }
      if (round == 0) has_eps = __syncthreads_or(eps);
      if (!__syncthreads_or(changed)) break;
      for (int s = lo + tid; s < hi; s += PO_NT) fwd[s] = row[s];
      __syncthreads();
      if (!has_eps || round > hi - lo) break;
    }
  }
  if (wave == 0) {                                                    // the criterion: the expected accuracy of a path
    const int lo = fs[T];
    double sum = 0.0;
    for (int i = lane; i < N - lo; i += 64) {
      const float c = v.fin[lo + i];
      const double al = alpha[lo + i];
      if (c != FINF && al != NINF) sum += exp((al + -(gs * (double)c)) - tot) * fwd[lo + i];
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) sh_avg = sum;
  }
  __syncthreads();
  const double avg = sh_avg;

  // the backward accuracy: B[s] = sum over the out-arcs to states that reach the end of exp((w + beta[next]) - beta[s]) (acc + B[next])
  for (int f = T; f >= 0; --f) {
    const int lo = fs[f], hi = fs[f + 1];
    int has_eps = 0;
    for (int round = 0;; ++round) {
      int changed = 0, eps = 0;
      for (int s = lo + tid; s < hi; s += PO_NT) {
        const int e0 = v.abeg[s], deg = lo_aend(v, s) - e0;
        if (deg > PO_HUB) continue;
        if (round == 0) for (int i = 0; i < deg; ++i) eps |= v.il[e0 + i] == 0;
        const double mine = beta[s];
        double sum = 0.0;
        if (mine != NINF)
          for (int i = 0; i < deg; ++i) {
            const int a = e0 + i, nx = v.next[a];
            const double be = beta[nx];
            if (be != NINF) sum += exp((po_w(v, gs, as, a) + be) - mine) * ((double)rank[a] + bwd[nx]);
          }
        row[s] = sum;
        changed |= po_differs(sum, bwd[s]);
      }
      for (int s = lo + wave; s < hi; s += PO_NT / 64) {
        const int e0 = v.abeg[s], deg = lo_aend(v, s) - e0;
        if (deg <= PO_HUB) continue;
        if (round == 0) for (int i = lane; i < deg; i += 64) eps |= v.il[e0 + i] == 0;
        const double mine = beta[s];
        double sum = 0.0;
        if (mine != NINF)
          for (int i = lane; i < deg; i += 64) {
            const int a = e0 + i, nx = v.next[a];
            const double be = beta[nx];
            if (be != NINF) sum += exp((po_w(v, gs, as, a) + be) - mine) * ((double)rank[a] + bwd[nx]);
          }
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        if (lane == 0) { row[s] = sum; changed |= po_differs(sum, bwd[s]); }
      }
      if (round == 0) has_eps = __syncthreads_or(eps);
      if (!__syncthreads_or(changed)) break;
      for (int s = lo + tid; s < hi; s += PO_NT) bwd[s] = row[s];
      __syncthreads();
      if (!has_eps || round > hi - lo) break;
    }
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
    p.arc_post[a0 + a] = d;
    flag[a] = live && v.il[a] != 0 && v.frame[src] < T ? 1 : 0;
  }
  __syncthreads();
  // the merge's counts and ranks, as k2_lattice_post_fb has them
  for (int a = tid; a < A; a += PO_NT) {
    int first = -1;
    if (flag[a]) {
      const int id = v.il[a], r0 = v.abeg[fs[v.frame[asrc[a]]]];
      first = 0;
      for (int k = r0; k < a; ++k) if (flag[k] && v.il[k] == id) { first = -1; break; }
    }
    rank[a] = first;
  }
  __syncthreads();
  for (int a = tid; a < A; a += PO_NT) {
    if (rank[a] != 0) continue;
    const int id = v.il[a], f = v.frame[asrc[a]], r0 = v.abeg[fs[f]], hs = fs[f + 1], r1 = hs < N ? v.abeg[hs] : A;
    int r = 0, cnt = 0;
    for (int k = r0; k < r1; ++k) if (rank[k] == 0) { ++cnt; r += v.il[k] < id; }
    flag[a] = 2 + r;
    if (r == cnt - 1 && f < T) fc[f] = cnt;
  }
  __syncthreads();
  if (wave == 0) {                                                    // exclusive prefix of the frames' counts
    int sum = 0;
    for (int tb = 0; tb < T; tb += 64) {
      const int t = tb + lane;
      const int c = t < T ? fc[t] : 0;
      int incl = c;
      for (int o = 1; o < 64; o <<= 1) { const int x = __shfl_up(incl, o); if (lane >= o) incl += x; }
      if (t < T) fc[t] = sum + incl - c;
      sum += __shfl(incl, 63);
    }
    if (lane == 0) {
      p.lo.utt_tot[2 * (int64_t)b] = T; p.lo.utt_tot[2 * (int64_t)b + 1] = sum;
      p.lo.status[u] = KHG_LAT_SUCCEEDED; p.tot[u] = tot; q.avg[u] = avg;
    }
  }
}
