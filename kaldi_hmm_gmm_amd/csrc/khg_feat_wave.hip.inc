// MFCC and filterbank features from waveforms (khg_frontend_compute, DESIGN.md 7q): one tile kernel.  One workgroup of four waves takes
// FE_TILE consecutive frames of ONE utterance and stages their sample span -- (frames - 1) S + L samples, int16 widened exactly, an
// index outside the utterance reflected back into it, a neighbour's sample never read -- and the tables (window, twiddles, mel
// weights and runs) in LDS once.  Then one wave works on one frame at a time, four frames abreast: the mean and the energies as 64
// strided chains closed by a butterfly over the lanes, pre-emphasis and window read straight from the staged span (w[i] and w[i - 1]
// are both x - mean, so nothing is exchanged), the real FFT as a complex radix-2 FFT of N / 2 points in the wave's own LDS buffer
// (bit-reversed on the way in, log2(N / 2) in-place stages) with the split post-pass forming the power spectrum, one lane per mel
// filter walking its own run of the spectrum in ascending order, one lane per cepstrum walking the log-mel values.  The rows of the
// tile are assembled in LDS and leave as one contiguous run.  Every operation is rounded on its own (fp contract off): the host form
// (kaldi_hmm_gmm_amd/wave.py) repeats them one by one.  The only transcendental functions are the final log and, for the magnitude
// spectrum, a correctly rounded sqrt.  No atomics; vector stores only.
constexpr int FE_TILE = KHG_FE_TILE_FRAMES;
constexpr int FE_WAVES = 4;
constexpr int FE_LM = 128;                                   // floats of a wave's log-mel buffer (num_mel_bins <= 128)
struct FeItem { int64_t s0, n, row0; int32_t t0, nfr; };     // the utterance's first sample and length, the tile's first row, its first frame of the utterance, its frames
struct FeParams {
  int32_t L, S, N, logM, B, C, out_dim, n_w;
  int32_t mfcc, remove_dc, snip, use_energy, raw_energy, use_log, use_power, i16, has_floor;
  float preemph, inv_L, log_floor;
};

// the floats of LDS a launch needs (the int32 runs of the filters are kept in the same block)
static inline int64_t fe_lds_floats(const FeParams& p) {
  const int64_t M = p.N / 2;
  return ((int64_t)(FE_TILE - 1) * p.S + p.L) + p.L + p.N + p.n_w + 3 * (int64_t)p.B + FE_WAVES * (3 * M + FE_LM) + (int64_t)FE_TILE * p.out_dim;
}

// p[l] + p[l ^ 32], then ^ 16 .. ^ 1: every lane ends with the same sum (a + b and b + a are the same float)
__device__ __forceinline__ float fe_wave_sum(float v) {
#pragma clang fp contract(off)
  for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ float fe_log_floor(float e) {
  const float f = e < FLT_EPSILON ? FLT_EPSILON : e;         // a NaN stays a NaN
  return logf(f);
}

__global__ __launch_bounds__(256) void k_fe_wave(const FeItem* __restrict__ items, const FeParams p, const void* __restrict__ samples, const float* __restrict__ tab,
                                                 const int32_t* __restrict__ runs, const float* __restrict__ dctT, const float* __restrict__ lifter,
                                                 float* __restrict__ out) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float fe_lds[];
  const FeItem it = items[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int L = p.L, S = p.S, N = p.N, M = N >> 1, logM = p.logM, B = p.B;
  const int span = (it.nfr - 1) * S + L;
  float* smp = fe_lds;                                       // [(FE_TILE - 1) S + L]
  float* win = smp + (FE_TILE - 1) * S + L;                  // [L]
  float* tw = win + L;                                       // [N / 2][2]: cos, -sin of 2 pi k / N
  float* melw = tw + N;                                      // [n_w]
  int32_t* run = reinterpret_cast<int32_t*>(melw + p.n_w);   // [3][B]: first bin, length, first weight
  float* zr = reinterpret_cast<float*>(run + 3 * B) + wv * (3 * M + FE_LM);      // the wave's own: [M] real parts
  float* zi = zr + M;                                        // [M] imaginary parts
  float* pw = zi + M;                                        // [M] the spectrum
  float* lm = pw + M;                                        // [FE_LM] the mel energies or their logs
  float* rows = reinterpret_cast<float*>(run + 3 * B) + FE_WAVES * (3 * M + FE_LM);      // [FE_TILE][out_dim]

  for (int i = tid; i < L; i += 256) win[i] = tab[i];
  for (int i = tid; i < N; i += 256) tw[i] = tab[L + i];
  for (int i = tid; i < p.n_w; i += 256) melw[i] = tab[L + N + i];
  for (int i = tid; i < 3 * B; i += 256) run[i] = runs[i];
  {
    const int64_t first = (int64_t)it.t0 * S + (p.snip ? 0 : S / 2 - L / 2);
    const int16_t* s16 = static_cast<const int16_t*>(samples) + it.s0;
    const float* s32 = static_cast<const float*>(samples) + it.s0;
    for (int i = tid; i < span; i += 256) {
      int64_t j = first + i;
      if (j < 0 || j >= it.n) {                              // i < 0 -> -i - 1, i >= n -> 2 n - 1 - i until inside: period 2 n
        const int64_t m2 = 2 * it.n;
        j %= m2;
        if (j < 0) j += m2;
        if (j >= it.n) j = m2 - 1 - j;
      }
      smp[i] = p.i16 ? (float)s16[j] : s32[j];
    }
  }
  __syncthreads();

  const float c = p.preemph;
  for (int f0 = 0; f0 < it.nfr; f0 += FE_WAVES) {            // the same trips for the four waves: the barriers below are the block's
    const int f = f0 + wv;
    const bool live = f < it.nfr;
    const float* x = smp + (live ? f : 0) * S;               // a wave without a frame recomputes frame 0 and writes nothing
    float mean = 0.0f;
    if (p.remove_dc) {
      float a = 0.0f;
      for (int i = lane; i < L; i += 64) a = a + x[i];
      mean = fe_wave_sum(a) * p.inv_L;
    }
    float e_raw = 0.0f;
    if (p.use_energy && p.raw_energy) {
      float a = 0.0f;
      for (int i = lane; i < L; i += 64) { const float w = x[i] - mean; a = a + w * w; }
      e_raw = fe_wave_sum(a);
    }
    float e_win = 0.0f;
    for (int i = lane; i < N; i += 64) {
      float v = 0.0f;
      if (i < L) {
        v = x[i] - mean;
        if (c != 0.0f) { const float w1 = x[i ? i - 1 : 0] - mean; v = v - c * w1; }
        v = v * win[i];
        e_win = e_win + v * v;
      }
      const int r = (int)(__brev((unsigned)(i >> 1)) >> (32 - logM));
      ((i & 1) ? zi : zr)[r] = v;
    }
    if (p.use_energy && !p.raw_energy) e_win = fe_wave_sum(e_win);
    __syncthreads();
    for (int s = 0; s < logM; ++s) {
      const int half = 1 << s;
      for (int q = lane; q < (M >> 1); q += 64) {
        const int k = q & (half - 1), a = ((q >> s) << (s + 1)) + k, b = a + half;
        const int j = k << (logM - 1 - s);                   // W_M^j = W_N^(2 j)
        const float wr = tw[4 * j], wi = tw[4 * j + 1];
        const float br = zr[b], bi = zi[b], ar = zr[a], ai = zi[a];
        const float tr = wr * br - wi * bi, ti = wr * bi + wi * br;
        zr[a] = ar + tr; zi[a] = ai + ti;
        zr[b] = ar - tr; zi[b] = ai - ti;
      }
      __syncthreads();
    }
    for (int k = lane; k < M; k += 64) {                     // X[k] = E[k] + W_N^k O[k] from Z[k] and conj(Z[M - k]); bins 0 .. N / 2 - 1
      float P;
      if (k == 0) {
        const float a = zr[0] + zi[0];
        P = a * a;
      } else {
        const float xr = zr[k], xi = zi[k], yr = zr[M - k], yi = zi[M - k];
        const float er = 0.5f * (xr + yr), ei = 0.5f * (xi - yi), pr = 0.5f * (xi + yi), pi = 0.5f * (yr - xr);
        const float wr = tw[2 * k], wi = tw[2 * k + 1];
        const float re = er + (wr * pr - wi * pi), im = ei + (wr * pi + wi * pr);
        P = re * re + im * im;
      }
      // the correctly rounded root: a double root is within an ulp of the real one, and the root of a float lies more than 2^-26 of
      // itself away from the midpoint of two floats, so narrowing it rounds as the real one would
      pw[k] = p.use_power ? P : (float)sqrt((double)P);
    }
    __syncthreads();
    for (int b = lane; b < B; b += 64) {
      const int off = run[b], len = run[B + b];
      const float* w = melw + run[2 * B + b];
      float a = 0.0f;
      for (int k = 0; k < len; ++k) a = a + w[k] * pw[off + k];
      lm[b] = p.use_log ? fe_log_floor(a) : a;
    }
    __syncthreads();
    float energy = 0.0f;
    if (p.use_energy) {
      energy = fe_log_floor(p.raw_energy ? e_raw : e_win);
      if (p.has_floor && energy < p.log_floor) energy = p.log_floor;
    }
    if (live) {
      float* o = rows + f * p.out_dim;
      if (p.mfcc) {
        for (int cc = lane; cc < p.C; cc += 64) {
          float a = 0.0f;
          for (int b = 0; b < B; ++b) a = a + dctT[b * p.C + cc] * lm[b];
          a = a * lifter[cc];
          o[cc] = (p.use_energy && cc == 0) ? energy : a;
        }
      } else {
        const int e0 = p.use_energy ? 1 : 0;
        if (e0 && lane == 0) o[0] = energy;
        for (int b = lane; b < B; b += 64) o[e0 + b] = lm[b];
      }
    }
  }
  __syncthreads();
  float* dst = out + it.row0 * p.out_dim;
  for (int e = tid; e < it.nfr * p.out_dim; e += 256) dst[e] = rows[e];
}
