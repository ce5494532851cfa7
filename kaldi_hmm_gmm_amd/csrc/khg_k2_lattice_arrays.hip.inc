// What the kernels over raw lattices share (K2R, K2F, K2O, K2P): the eleven arrays of a chunk's lattices and the scan that sizes a
// chunk's output.

// the six per-state and five per-arc arrays of a chunk's lattices (LatChunk), the utterances one after the other; arc_begin and next
// are relative to the utterance
template <class I, class F>
struct LatArraysT {
  I *frame, *gstate, *arc_begin;
  F *tot, *extra, *fin;
  I *ilabel, *olabel, *next;
  F *g, *ac;
};
using LatArrays = LatArraysT<int32_t, float>;
using LatArraysIn = LatArraysT<const int32_t, const float>;

// one wave: n pairs of totals, tot[2 * b] and tot[2 * b + 1] -> exclusive offsets (int64), the first column at off[b], the second at
// off[n + 1 + b], the sums at off[n] and off[2 * n + 1]
__global__ __launch_bounds__(64) void k2_lattice_scan_pairs(const int64_t* tot, int64_t* off, int32_t n) {
  const int lane = (int)threadIdx.x;
  long long ts = 0, ta = 0;
  for (int bb = 0; bb < n; bb += 64) {
    const int b = bb + lane;
    const long long c1 = b < n ? tot[2 * (int64_t)b] : 0, c2 = b < n ? tot[2 * (int64_t)b + 1] : 0;
    long long i1 = c1, i2 = c2;
    for (int o = 1; o < 64; o <<= 1) {
      const long long t1 = __shfl_up(i1, o), t2 = __shfl_up(i2, o);
      if (lane >= o) { i1 += t1; i2 += t2; }
    }
    if (b < n) { off[b] = ts + i1 - c1; off[(int64_t)n + 1 + b] = ta + i2 - c2; }
    ts += __shfl(i1, 63); ta += __shfl(i2, 63);
  }
  if (lane == 0) { off[n] = ts; off[2 * (int64_t)n + 1] = ta; }
}
