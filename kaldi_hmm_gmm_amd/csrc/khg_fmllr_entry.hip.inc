// The per-entry vectors of the fMLLR accumulation, bucketed by pdf (DESIGN.md 7l, kernels 3a-3e).  Per chunk of frames:
//   k_fmllr_count   entries of every frame of the chunk -> k_fmllr_scan (exclusive sum: the frame's first COMPACT entry number)
//   k_fmllr_keys    per compact entry: its number in the call's flattened arrays, the (pdf, compact entry) pair; an entry that adds
//                   nothing (dropped by the flatten pass, weight +-0, a pdf the model lacks) and the unused tail get key P
//   stable radix sort of the pairs (K3's path: a pdf's entries stay in entry order)
//   k_fmllr_entry   one workgroup per FE_EB consecutive SORTED entries: for every run of one pdf inside them the pdf's rows are staged
//                   in LDS ONCE (coalesced; tiles of Gaussians when a pdf does not fit) and shared by the run's entries; per entry
//                   the component posteriors as K3's POST forms compute them, then ea / eb / ec in Gaussian order -- written per
//                   entry, no atomics
//   k_fmllr_fsum    a frame's a_t / b_t: the float sums of its entries' vectors in entry order; c_t their double sum
// The arithmetic of an entry and the order of every sum are the rule's, so the statistics keep the bits they had without the bucketing.
struct FeEntArgs {
  FmArgs f;
  int32_t npos, capE;
  int32_t* cnt;        // [npos + 1] entries per frame, then their exclusive sum in place
  int32_t* ent_id;     // [capE] compact entry -> flattened entry
  uint32_t *keys, *vals;            // [capE] the pairs before the sort
  const uint32_t *skeys, *svals;    // ... and after
  float *ea, *eb, *ec;              // [capE][D], [capE][D], [capE]
  int32_t EB, GT, DS, GS;           // entries per workgroup, Gaussians per staged tile, row stride of the tile (odd), ll row stride
};

__global__ __launch_bounds__(256) void k_fmllr_count(FeEntArgs a) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t pos = (int64_t)blockIdx.x * 256 + threadIdx.x; pos < a.npos; pos += stride) {
    const int32_t row = a.f.pos_row[pos];
    int n = 0;
    for (int32_t i = a.f.row_first[row]; i >= 0 && (int64_t)i < a.f.E && a.f.e_row[i] == row; ++i) ++n;
    a.cnt[pos] = n;
  }
}
// exclusive sum of cnt[0 .. n) in place, the total at cnt[n]: one workgroup, every thread a contiguous piece, the pieces' sums scanned in LDS
__global__ __launch_bounds__(1024) void k_fmllr_scan(int32_t* __restrict__ cnt, int32_t n) {
  __shared__ int32_t part[1024];
  const int tid = threadIdx.x;
  const int64_t per = ((int64_t)n + 1023) / 1024, lo = tid * per < n ? tid * per : n, hi = lo + per < n ? lo + per : n;
  int32_t s = 0;
  for (int64_t i = lo; i < hi; ++i) s += cnt[i];
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    int32_t run = 0;
    for (int i = 0; i < 1024; ++i) { const int32_t v = part[i]; part[i] = run; run += v; }
    cnt[n] = run;
  }
  __syncthreads();
  int32_t run = part[tid];
  for (int64_t i = lo; i < hi; ++i) { const int32_t v = cnt[i]; cnt[i] = run; run += v; }
}
__global__ __launch_bounds__(256) void k_fmllr_keys(FeEntArgs a) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int32_t total = a.cnt[a.npos];
  for (int64_t ce = total + (int64_t)blockIdx.x * 256 + threadIdx.x; ce < a.capE; ce += stride) { a.keys[ce] = (uint32_t)a.f.P; a.vals[ce] = (uint32_t)ce; }
  for (int64_t pos = (int64_t)blockIdx.x * 256 + threadIdx.x; pos < a.npos; pos += stride) {
    const int32_t row = a.f.pos_row[pos];
    int32_t ce = a.cnt[pos];
    for (int32_t i = a.f.row_first[row]; i >= 0 && (int64_t)i < a.f.E && a.f.e_row[i] == row; ++i, ++ce) {
      if (ce >= a.capE) break;                               // (cannot happen: capE bounds the chunk's entries)
      const int tid = a.f.e_tid[i];
      int pdf = a.f.P;
      if (tid >= 1 && tid <= a.f.num_tids && a.f.e_w[i] != 0.0f) {
        const int p = a.f.id2pdf[tid];
        if (p >= 0 && p < a.f.P) pdf = p; else atomicOr(a.f.err_flag, 4);
      }
      a.ent_id[ce] = i; a.keys[ce] = (uint32_t)pdf; a.vals[ce] = (uint32_t)ce;
      a.ec[ce] = 0.0f;                                       // an entry that adds nothing: fsum reads only its ec (0) flag-free
      if (pdf == a.f.P) {
        for (int d = 0; d < a.f.D; ++d) { a.ea[(int64_t)ce * a.f.D + d] = 0.0f; a.eb[(int64_t)ce * a.f.D + d] = 0.0f; }
      }
    }
  }
}

// Dynamic LDS (floats): Mt[GT][DS] | Vt[GT][DS] | ll[EB][GS] | xs[EB][D] | gc[GT]
__global__ __launch_bounds__(256) void k_fmllr_entry(FeEntArgs a) {
  extern __shared__ __attribute__((aligned(16))) float fe_lds[];
  const FmArgs& p = a.f;
  const int D = p.D, EB = a.EB, GT = a.GT, DS = a.DS, GS = a.GS;
  float* Mt = fe_lds;
  float* Vt = Mt + GT * DS;
  float* ll = Vt + GT * DS;
  float* xs = ll + EB * GS;
  float* gct = xs + EB * D;
  __shared__ int s_pdf[64], s_ent[64], s_ce[64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t base = (int64_t)blockIdx.x * EB;
  if (base >= a.capE) return;
  const int nb = (int)min((int64_t)EB, a.capE - base);
  if (tid < nb) {
    const int pdf = (int)a.skeys[base + tid], ce = (int)a.svals[base + tid];
    s_pdf[tid] = pdf; s_ce[tid] = ce; s_ent[tid] = pdf < p.P ? a.ent_id[ce] : -1;
  }
  __syncthreads();
  if (s_pdf[0] >= p.P) return;                               // sorted: nothing but the tail here
  for (int e = tid; e < nb * D; e += 256) {
    const int k = e / D, d = e - k * D;
    xs[e] = s_ent[k] >= 0 ? p.feats[(int64_t)p.e_row[s_ent[k]] * D + d] : 0.0f;
  }
  int r0 = 0;
  while (r0 < nb && s_pdf[r0] < p.P) {
    const int pdf = s_pdf[r0];
    int r1 = r0 + 1;
    while (r1 < nb && s_pdf[r1] == pdf) ++r1;
    const int g0 = p.gauss_off[pdf], G = p.gauss_off[pdf + 1] - g0;
    const int ntile = (G + GT - 1) / GT;
    // ---- phase A: the per-Gaussian log-likelihoods of the run's entries, tile by tile ----
    for (int t = 0; t < ntile; ++t) {
      const int t0 = t * GT, ng = min(GT, G - t0);
      __syncthreads();
      for (int e = tid; e < ng * D; e += 256) {
        const int g = e / D, d = e - g * D;
        Mt[g * DS + d] = p.miv[(int64_t)(g0 + t0) * D + e];
        Vt[g * DS + d] = p.nhiv[(int64_t)(g0 + t0) * D + e];
      }
      for (int g = tid; g < ng; g += 256) gct[g] = p.gconsts[g0 + t0 + g];
      __syncthreads();
      for (int k = r0 + wave; k < r1; k += 4) {
        const float* x = xs + k * D;
        for (int g = lane; g < ng; g += 64) {
          const float* M = Mt + g * DS;
          const float* V = Vt + g * DS;
          float s = gct[g];
          int d = 0;
          for (; d + 1 < D; d += 2) {
            const float x0 = x[d], x1 = x[d + 1];
            s = fmaf(M[d], x0, s); s = fmaf(M[d + 1], x1, s);
            s = fmaf(V[d], __fmul_rn(x0, x0), s); s = fmaf(V[d + 1], __fmul_rn(x1, x1), s);
          }
          if (d < D) { const float x0 = x[d]; s = fmaf(M[d], x0, s); s = fmaf(V[d], __fmul_rn(x0, x0), s); }
          ll[k * GS + t0 + g] = s;
        }
      }
    }
    __syncthreads();
    // ---- the posteriors: max, exp, sum, one division per entry (K3's POST forms) ----
    for (int k = r0 + wave; k < r1; k += 4) {
      float* l = ll + k * GS;
      float mx = -INFINITY;
      for (int g = lane; g < G; g += 64) mx = fmaxf(mx, l[g]);
      for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
      float sum = 0.0f;
      for (int g = lane; g < G; g += 64) { const float e = __expf(l[g] - mx); l[g] = e; sum += e; }
      for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
      const float llf = __logf(sum) + mx;
      float scale = p.e_w[s_ent[k]] / sum;
      if (!(fabsf(llf) <= 3.0e38f)) { if (lane == 0) atomicOr(p.err_flag, 1); scale = 0.0f; for (int g = lane; g < G; g += 64) l[g] = 0.0f; }   // diag-gmm.cc:385-387: the entry adds nothing
      for (int g = lane; g < G; g += 64) l[g] = l[g] * scale;
    }
    // ---- phase B: ea / eb / ec in Gaussian order, from the staged rows (inv_var = -2 x its staged half, exact) ----
    for (int t = 0; t < ntile; ++t) {
      const int t0 = t * GT, ng = min(GT, G - t0);
      if (ntile > 1) {
        __syncthreads();
        for (int e = tid; e < ng * D; e += 256) {
          const int g = e / D, d = e - g * D;
          Mt[g * DS + d] = p.miv[(int64_t)(g0 + t0) * D + e];
          Vt[g * DS + d] = p.nhiv[(int64_t)(g0 + t0) * D + e];
        }
      }
      __syncthreads();
      for (int k = r0 + wave; k < r1; k += 4) {
        const float* l = ll + k * GS + t0;
        const int64_t o = (int64_t)s_ce[k] * D;
        float ea[2] = {0.0f, 0.0f}, eb[2] = {0.0f, 0.0f}, ec = 0.0f;
        if (t > 0) {
          ec = a.ec[s_ce[k]];
#pragma unroll
          for (int h = 0; h < 2; ++h) { const int d = lane + 64 * h; if (d < D) { ea[h] = a.ea[o + d]; eb[h] = a.eb[o + d]; } }
        }
        for (int g = 0; g < ng; ++g) {
          const float gg = l[g];
          ec = __fadd_rn(ec, gg);
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int d = lane + 64 * h;
            if (d < D) {
              ea[h] = __fadd_rn(ea[h], __fmul_rn(gg, -2.0f * Vt[g * DS + d]));
              eb[h] = __fadd_rn(eb[h], __fmul_rn(gg, Mt[g * DS + d]));
            }
          }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) { const int d = lane + 64 * h; if (d < D) { a.ea[o + d] = ea[h]; a.eb[o + d] = eb[h]; } }
        if (lane == 0) a.ec[s_ce[k]] = ec;
      }
    }
    __syncthreads();
    r0 = r1;
  }
}

// a_t / b_t / c_t of every frame of the chunk: its entries' vectors added in entry order
__global__ __launch_bounds__(256) void k_fmllr_fsum(FeEntArgs a) {
  const int D = a.f.D;
  const int64_t n = (int64_t)a.npos * D, stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const int64_t pos = i / D;
    const int d = (int)(i - pos * D);
    const int e0 = a.cnt[pos], e1 = a.cnt[pos + 1];
    float at = 0.0f, bt = 0.0f;
    for (int e = e0; e < e1; ++e) { at = __fadd_rn(at, a.ea[(int64_t)e * D + d]); bt = __fadd_rn(bt, a.eb[(int64_t)e * D + d]); }
    a.f.a[i] = at; a.f.b[i] = bt;
    if (d == 0) {
      double ct = 0.0;
      for (int e = e0; e < e1; ++e) ct += (double)a.ec[e];
      a.f.c[pos] = ct;
    }
  }
}
