// K2L: batched, order-faithful LatticeFasterDecoder + DecodeUtteranceLatticeFaster (khg_decode_lattice_faster), one workgroup per
// utterance, one lane doing the token passing in the reference's order (the pattern of k2_viterbi_faithful).
//
// Restates, in float and in the reference's association order (reference csrc/):
//   lattice-faster-decoder.cc:61-98     InitDecoding / Decode
//   :221-228 PossiblyResizeHash  :254-299 FindOrAddToken  :305-380 PruneForwardLinks  :386-472 PruneForwardLinksFinal
//   :492-548 PruneTokensForFrame / PruneActiveTokens  :551-588 ComputeFinalCosts  :591-653 AdvanceDecoding / FinalizeDecoding
//   :657-727 GetCutoff (both branches)  :730-825 ProcessEmitting  :840-905 ProcessNonemitting  :935-1013 TopSortTokens
//   :101-192 GetBestPath = GetRawLattice + OpenFst ShortestPath (n = 1, StateOrderQueue on the top-sorted raw lattice)
//   decoder-wrappers.cc:186-224          DecodeUtteranceLatticeFaster: (succeeded, alignment, words, like = -(graph + acoustic))
// The HashList is K2HashList, shared with k2_viterbi_faithful (hash-list-inl.h:129-174 restated: bucket-ordered list,
// find-or-insert), here over the utterance's HBM scratch slice.  Tokens and forward links live in that slice too, with free lists (the reference's memory
// pools); running out of either sets KHG_LAT_SCRATCH for the utterance and stops it -- never a silent truncation.  The graph is read
// from the set's CSR tables (HBM, through L2).
//
// The best path is found on the surviving links after FinalizeDecoding: states are the tokens numbered by frame, then in
// TopSortTokens order inside the frame (its unordered_map walked in creation order, its reprocess set in insertion order --
// DESIGN.md); visiting them in that order with strict-improvement relaxation under Kaldi's LatticeWeight order (Value1 + Value2,
// then Value1) is OpenFst's SingleShortestPath on a top-sorted FST.  The distance pairs are the path's LatticeWeight products
// (component-wise float adds, left to right), which is what GetLinearSymbolSequence multiplies back.

struct LatArgs {
  const int64_t* frame_off;   // [U+1]
  const int32_t* gidx;        // [U] the row of state_off / start an utterance decodes on (identity; zeros on a shared graph)
  const int64_t* state_off;   // [rows+1]
  const int32_t* start;       // [U]
  const int64_t* in_off;      // [sumS+1]
  const int32_t* in_col;      // -1: epsilon input
  const int32_t* in_tid;
  const int32_t* in_olabel;
  const float* in_w;
  const int64_t* out_off;     // [sumS+1]
  const int32_t* out_inidx;
  const float* final_w;
  const float* trans_cost;    // or nullptr
  const float* ll;
  const int64_t* ll_off;
  // the utterances of this pass: workgroup b of a launch at list position u0 decodes utterance list[u0 + b]; its scratch slice is at
  // scratch + scr_off[u0 + b] (offsets relative to the launch's first slice), with tok_cap / link_cap[u0 + b] tokens / links
  const int32_t* list;
  unsigned char* scratch;
  const int64_t* scr_off;
  const int32_t* tok_cap;
  const int32_t* link_cap;
  int32_t hb;                 // hash buckets (>= the largest hash_size any frame can ask for)
  int32_t amax;               // arc bound the slices were laid out with (>= every utterance's arc count)
  // outputs
  int32_t* ali;               // [sumT]
  int32_t* words;             // per utterance words_off[u+1] - words_off[u]
  const int64_t* words_off;
  int32_t* num_words;
  double* like;
  int32_t* status;
  // config
  float beam, lattice_beam, beam_delta, hash_ratio, prune_scale, acoustic_scale;
  int32_t max_active, min_active, prune_interval, allow_partial;
};

struct LatTok { float tot, extra, d1, d2, fcost; int32_t links, next, pos, rp_slot, plink, ptok, flags; };
struct LatLink { int32_t next_tok, ilabel, olabel; float graph_cost, acoustic_cost; int32_t next; };
struct LatElem { int32_t key, val, tail; };
#define LAT_F_RP 1      // in TopSortTokens' reprocess set
#define LAT_F_DIST 2    // ShortestPath distance set

// the per-utterance slice: [toks][links][elems x 2][buckets x 2][queue][tmp][dst][nieps][frame heads][frame flags][cost offsets]
// [order][reprocess x 2][slots]; only when the raw lattice is asked for (khg_k2_lattice_faster_raw.hip.inc), behind all of that:
// [graph state of every token][per state: token, frame, first arc][first state of every frame]
struct LatLayout {
  int64_t toks, links, elems0, elems1, blast, bprev, queue, tmp, dst, nieps, fhead, fflags, coff, ord, rp0, rp1, slot, total;
  int64_t gst, stok, sfr, sarc, fbase;
  int32_t qcap, rpcap, slotcap;
};
__host__ __device__ inline LatLayout lat_layout(int64_t T, int64_t S, int64_t A, int64_t hb, int64_t tc, int64_t lc, bool lat = false) {
  LatLayout L;
  int64_t o = 0;
  auto take = [&](int64_t bytes) { int64_t r = o; o += (bytes + 15) & ~int64_t(15); return r; };
  L.qcap = (int32_t)(2 * (S + A) + 16);
  L.rpcap = (int32_t)(2 * S + 64);
  L.slotcap = (int32_t)(S + 2 * L.rpcap);
  L.toks = take(tc * (int64_t)sizeof(LatTok));
  L.links = take(lc * (int64_t)sizeof(LatLink));
  L.elems0 = take(S * (int64_t)sizeof(LatElem));
  L.elems1 = take(S * (int64_t)sizeof(LatElem));
  L.blast = take(4 * hb);
  L.bprev = take(4 * hb);
  L.queue = take(4 * (int64_t)L.qcap);
  L.tmp = take(4 * S);
  L.dst = take(4 * A);
  L.nieps = take(4 * S);
  L.fhead = take(4 * (T + 1));
  L.fflags = take(4 * (T + 1));
  L.coff = take(4 * (T + 1));
  L.ord = take(4 * (S + 1));
  L.rp0 = take(4 * (int64_t)L.rpcap);
  L.rp1 = take(4 * (int64_t)L.rpcap);
  L.slot = take(4 * (int64_t)L.slotcap);
  L.gst = L.stok = L.sfr = L.sarc = L.fbase = 0;
  if (lat) {       // a state is a surviving token: at most tc of them
    L.gst = take(4 * tc);
    L.stok = take(4 * tc);
    L.sfr = take(4 * tc);
    L.sarc = take(4 * (tc + 1));
    L.fbase = take(4 * (T + 2));
  }
  L.total = o;
  return L;
}

// k-th order statistic of tmp[0..n) (the value std::nth_element leaves at position k); reorders tmp
__device__ float lat_kth(float* tmp, int n, int k) {
  if (k >= n) return tmp[k];     // nth_element on an empty tail (min_active == max_active): the value already there
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const float pivot = tmp[(lo + hi) >> 1];
    int i = lo, j = hi;
    while (i <= j) {
      while (tmp[i] < pivot) ++i;
      while (pivot < tmp[j]) --j;
      if (i <= j) { float t = tmp[i]; tmp[i] = tmp[j]; tmp[j] = t; ++i; --j; }
    }
    if (k <= j) hi = j;
    else if (k >= i) lo = i;
    else break;
  }
  return tmp[k];
}

__device__ __forceinline__ bool lat_less(float a1, float a2, float b1, float b2) {   // NaturalLess: (a1, a2) strictly better
  const float fa = a1 + a2, fb = b1 + b2;
  if (fa < fb) return true;
  if (fa > fb) return false;
  return a1 < b1;
}

// The decoder kernel's body is khg_k2_lattice_body.hip.inc, included textually: k2_lattice_faster compiles with nothing lattice-related
// in it (LAT false: the same instruction stream as before the raw lattice existed).  LAT: also leave in the slice what
// k2_lattice_faster_raw_fill emits the raw lattice from (utt_tot[2 * b], [2 * b + 1]: the states and arcs of the launch's utterance b,
// 0 unless it succeeded).
__global__ __launch_bounds__(64) void k2_lattice_faster(LatArgs a, int u0) {
#pragma clang fp contract(off)
  constexpr bool LAT = false;
  int64_t* const utt_tot = nullptr;
#include "khg_k2_lattice_body.hip.inc"
}
// khg_decode_lattice_faster_raw's decoder launch
__global__ __launch_bounds__(64) void k2_lattice_faster_lat(LatArgs a, int u0, int64_t* utt_tot) {
#pragma clang fp contract(off)
  constexpr bool LAT = true;
#include "khg_k2_lattice_body.hip.inc"
}
