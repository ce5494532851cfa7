// The decoding-graph container of the host API and what the alignment entry points do with it, in C++.
//
// The reference takes fst::VectorFst<fst::StdArc> from the separate kaldifst package (scripts/gmm_align_compiled.py:6,14), which
// is not available offline; this is the minimal tropical-semiring VectorFst with the kaldifst method names the reference's scripts
// and tests use.  On top of it (reference, /root/reference/kaldi-hmm-gmm/csrc/): AddTransitionProbs (hmm-utils.cc:465-493),
// ModifyGraphForCarefulAlignment (decoder-wrappers.cc:111-140), and FasterDecoder's host side (faster-decoder.cc:33-53 decode /
// :346-423 ReachedFinal / GetBestPath; python/csrc/faster-decoder.cc:14-53) over K1 + K2.
#pragma once
#include <functional>

#include "khg_host_align.hpp"

namespace khg {

constexpr int kNoStateId = -1;

struct StdArc {
  int ilabel = 0, olabel = 0;
  float weight = 0.0f;
  int nextstate = 0;
  std::string ToString() const;
};

class StdVectorFst {
 public:
  int AddState() { arcs_.emplace_back(); final_.push_back(std::numeric_limits<float>::infinity()); return (int)arcs_.size() - 1; }
  int NumStates() const { return (int)arcs_.size(); }
  int Start() const { return start_; }
  void SetStart(int s) { start_ = s; }
  void AddArc(int state, const StdArc& a) { KHG_REQUIRE(state >= 0 && state < NumStates(), "add_arc: bad state"); arcs_[(size_t)state].push_back(a); }
  void SetFinal(int state, float w) { KHG_REQUIRE(state >= 0 && state < NumStates(), "set_final: bad state"); final_[(size_t)state] = w; }
  float Final(int state) const { KHG_REQUIRE(state >= 0 && state < NumStates(), "final: bad state"); return final_[(size_t)state]; }
  bool IsFinal(int state) const { return Final(state) != std::numeric_limits<float>::infinity(); }     // +inf == TropicalWeight::Zero()
  const std::vector<StdArc>& Arcs(int state) const { KHG_REQUIRE(state >= 0 && state < NumStates(), "arcs: bad state"); return arcs_[(size_t)state]; }
  std::vector<StdArc>& MutableArcs(int state) { KHG_REQUIRE(state >= 0 && state < NumStates(), "arcs: bad state"); return arcs_[(size_t)state]; }
  int64_t NumArcs() const { int64_t n = 0; for (auto& a : arcs_) n += (int64_t)a.size(); return n; }
  std::vector<std::vector<StdArc>>& arcs() { return arcs_; }
  const std::vector<std::vector<StdArc>>& arcs() const { return arcs_; }
  std::vector<float>& finals() { return final_; }
  const std::vector<float>& finals() const { return final_; }

 private:
  std::vector<std::vector<StdArc>> arcs_;
  std::vector<float> final_;
  int start_ = kNoStateId;
};

// the CSR block khg_utts_create consumes, for a list of graphs
GraphsCsr ConcatGraphs(const std::vector<const StdVectorFst*>& fsts);
// csrc/decoder-wrappers.cc:111-140 (+ OpenFst Concat): in place
void ModifyGraphForCarefulAlignment(StdVectorFst* fst);
// csrc/hmm-utils.cc:465-493: arc.weight (x)= -scaled transition log-prob, in place
void AddTransitionProbs(const TransitionModel& tm, const std::vector<int>& disambig_syms, float transition_scale, float self_loop_scale, StdVectorFst* fst);

// AlignUtteranceWrapper / FasterDecoder::Decode for ANY DecodableInterface (csrc/decoder-wrappers.cc:16-108 takes a
// DecodableInterface*, python/csrc/decodable-itf.cc:16-53 lets Python subclass it): the scores of every (frame, transition-id on
// the graph) are sampled through the interface into K2's score matrix (khg_loglikes_upload) and K2 decodes them unscaled -- the
// decodable already applied its own scale; `like` is divided by like_scale.  r.pdfs lists index - 1 for the sampled indices,
// r.loglikes their [n][T] scores.
AlignResult AlignDecodable(const StdVectorFst& fst, const DecodableInterface& decodable, const AlignConfig& config, float like_scale,
                           const FasterDecoderOptions* decoder_opts);

// DecodeUtteranceLatticeFaster for ANY DecodableInterface: scores of every (frame, index on the graph) sampled through the interface
// (as AlignDecodable does) and decoded unscaled by the lattice decoder.
LatticeResult DecodeLatticeDecodable(const StdVectorFst& fst, const DecodableInterface& decodable, const LatticeFasterDecoderConfig& config,
                                     bool allow_partial, int scratch_per_frame = 0);

// python/csrc/lattice-faster-decoder.cc:46-56: the decoder object holds its graph and configuration; the work is done by
// decode_utterance_lattice_faster (DecodeUtteranceLatticeFaster), each call on a fresh decoder state.
struct LatticeFasterDecoder {
  std::shared_ptr<StdVectorFst> fst;
  LatticeFasterDecoderConfig config;
};

// DecodeUtteranceLatticeSimple for ANY DecodableInterface, the same way (zero frames allowed: the decoder itself decides)
LatticeResult DecodeLatticeSimpleDecodable(const StdVectorFst& fst, const DecodableInterface& decodable, const LatticeSimpleDecoderConfig& config,
                                           bool allow_partial, int scratch_per_frame = 0);

// python/csrc/lattice-simple-decoder.cc:33-37: the graph and configuration; decode_utterance_lattice_simple does the work
struct LatticeSimpleDecoder {
  std::shared_ptr<StdVectorFst> fst;
  LatticeSimpleDecoderConfig config;
};

struct LatticeWeight {        // kaldifst LatticeWeight (graph cost, acoustic cost); Times adds component-wise
  double value1 = 0.0, value2 = 0.0;
};
struct LatticeArc {
  int ilabel = 0, olabel = 0;
  LatticeWeight weight;
  int nextstate = 0;
};
// The linear fst::VectorFst<LatticeArc> FasterDecoder::GetBestPath returns: state i has the single arc arcs[i] to state i + 1; the
// last state is final with `final`.
struct LinearLattice {
  std::vector<LatticeArc> arcs;
  LatticeWeight final_w;
  int start = -1;
  int NumStates() const { return start < 0 ? 0 : (int)arcs.size() + 1; }
  // kaldifst GetLinearSymbolSequence -> ok; ilabels != 0, olabels != 0, total weight
  bool GetLinearSymbolSequence(std::vector<int>* ilabels, std::vector<int>* olabels, LatticeWeight* total) const;
};

// Lattice::BestPath: KHG_LAT_* status (SUCCEEDED, NO_PATH, EPS_LOOP); the path's non-zero ilabels and olabels, its lattice arcs, its two
// float sums taken left to right from One() with the final weight last (v1, v2), the final state and its forward pair plus final weight
// (f1, f2), and the forward pairs / back-pointers of every state
struct LatticeBestPath {
  int status = 0;
  std::vector<int32_t> ali, words, arcs;
  float v1 = 0.0f, v2 = 0.0f, f1 = 0.0f, f2 = 0.0f;
  int final_state = -1;
  std::vector<float> alpha1, alpha2;
  std::vector<int32_t> bp;
};

// Lattice::ForwardBackward (what khg_lattices_posteriors gives for one lattice): KHG_LAT_* status (SUCCEEDED, NO_PATH,
// EPS_LOOP), the total log-likelihood, alpha / beta per state, the posterior of every arc, and per frame 0 .. T - 1 the emitting arcs'
// posteriors merged by ilabel, ascending.  Without SUCCEEDED: tot_like = -inf and everything else empty.
struct LatticePosteriors {
  int status = 0;
  double tot_like = 0.0;
  std::vector<double> alpha, beta, arc_post;
  std::vector<std::vector<std::pair<int32_t, double>>> post;
};

// Lattice::ForwardBackwardMpe (what khg_lattices_mpe_posteriors gives for one lattice): ForwardBackward's fields -- here
// arc_post holds the SIGNED values d and post their per-frame sums -- plus the expected accuracy of a path and the forward / backward
// accuracies per state.  KHG_LAT_NO_REF: the alignment is empty, not of the lattice's frame count, or holds an id outside 1 .. num_tids.
struct LatticeMpePosteriors : LatticePosteriors {
  double avg_acc = 0.0;
  std::vector<double> acc_fwd, acc_bwd;      // A, B
};

// A backoff n-gram LM as the flat arrays of khg_lm_create (include/khg_hip.h): state 0 is the empty history, state h
// owns the arcs arc_begin[h] .. arc_begin[h + 1] with words ascending.  Not validated here: khg_lm_validate does that.
struct BackoffLm {
  std::vector<int32_t> backoff, arc_begin, word, next;
  std::vector<float> backoff_cost, cost, final_cost;
  int32_t start = 0;
  // advance(h, w): -> the next state and *c (float sums, one rounding each), or -1: out of vocabulary
  int Advance(int h, int w, float* c) const;
};
class Lattice;
// Lattice::LmRescore: the KHG_LAT_* status, the rescored lattice (empty without KHG_LAT_SUCCEEDED) and the largest |H(s)|
struct LatticeLmRescored {
  int status = 0;
  std::shared_ptr<Lattice> lattice;
  int64_t max_hist = 0;
};

// Lattice::Determinize: the KHG_LAT_* status, the determinized lattice (empty without KHG_LAT_SUCCEEDED) and the counts
struct LatticeDeterminized {
  int status = 0;
  std::shared_ptr<Lattice> lattice;
  khg_det_stats stats = {0, 0, 0, 0, 0, 0, 0, 0};
};

// One entry of Lattice::Nbest: the path's transition-ids by frame (one per frame of the lattice, 0 where the path has none), its
// words, its arcs, its weight pair (a, b) and its total, the final state it ends in and its rank in that state's list
struct LatticeNbestEntry {
  std::vector<int32_t> ali, words, arcs;
  float a = 0.0f, b = 0.0f, total = 0.0f;
  int end_state = -1, rank = 0;
};

// Lattice::Oracle (what khg_lattices_oracle gives for one lattice): KHG_LAT_* status (SUCCEEDED, NO_PATH, EPS_LOOP), the
// counts (errors, insertions, deletions, substitutions; (R, 0, R, 0) without a path), the oracle path's words, its arcs, and its
// transition-ids by frame (one entry per frame of the lattice, 0 where the path has none)
struct LatticeOracle {
  int status = 0;
  int32_t counts[4] = {0, 0, 0, 0};
  std::vector<int32_t> words, arcs, ali;
};

// Lattice::Mbr (what khg_lattices_mbr gives for one lattice): KHG_LAT_* status, the number of updates made, the Bayes
// risk (+inf without SUCCEEDED), the hypothesis, a confidence per word, the distinct olabels (0 first) and gamma [Q][vocab.size()]
// row-major, the weights used (arc_cond per arc, final_cond per state), the cap on the words, and the risk of every accumulation
struct LatticeMbr {
  int status = 0, iters = 0;
  double bayes_risk = 0.0;
  std::vector<int32_t> words, vocab;
  std::vector<double> conf, gamma, arc_cond, final_cond, risks;
  int32_t cap = 0;
};

// The fst::VectorFst<LatticeArc> LatticeSimpleDecoder::GetRawLattice builds (csrc/lattice-simple-decoder.cc:654-735), as the flat arrays
// khg_lattices_download hands back: a state per surviving token, numbered by frame, then by graph state (:684-690); state s owns arcs
// arc_begin[s] .. arc_begin[s + 1], one per surviving forward link in the order of the graph's arcs in its state (:700-722); the last
// frame's final tokens are final with (final_cost, 0) (:723-733).  Which lattice that is (the order-independent one): DESIGN.md 7d.
// From the lattice-faster decoder (LatticeFasterDecoder::GetRawLattice, csrc/lattice-faster-decoder.cc:101-192) the
// second numbering rule holds instead: states by frame, then in TopSortTokens order inside the frame with the gaps removed;
// graph_state is the state the token was created for; a state's arcs follow its forward-link list, head first; without any final
// state reached every last-frame state is final with (0, 0).  That lattice is acyclic and top-sorted.
class Lattice {
 public:
  // per state
  std::vector<int32_t> frame, graph_state;
  std::vector<float> tot_cost, extra_cost, final_cost;     // final_cost: +inf unless the state is final
  std::vector<int32_t> arc_begin;                          // [NumStates() + 1]
  // per arc
  std::vector<int32_t> ilabel, olabel, nextstate;
  std::vector<float> graph_cost, acoustic_cost;
  int start = kNoStateId;

  int NumStates() const { return (int)frame.size(); }
  int Start() const { return start; }
  int64_t NumArcs() const { return (int64_t)ilabel.size(); }
  int NumArcs(int s) const { Check(s); return arc_begin[(size_t)s + 1] - arc_begin[(size_t)s]; }
  std::vector<LatticeArc> Arcs(int s) const;
  LatticeWeight Final(int s) const;      // LatticeWeight::Zero() = (+inf, +inf) for a state that is not final
  // OpenFst ShortestPath over the lattice by the tie rule of the decoder kernel: frame by frame, emitting in-links
  // first, then epsilon in-links in Jacobi rounds; a state takes its in-links ordered by (source state, arc) and changes only on a
  // strictly better LatticeWeight; the final state is the lowest among exact ties.  Distances are float sums, left to right, as in
  // the kernel.  Every arc of the path is kept (epsilons too).  An empty lattice, or none of its final states reached: start == -1.
  // The same under scales: every arc weighs (fl(graph_scale * graph_cost), fl(acoustic_scale * acoustic_cost)), a final
  // state (fl(graph_scale * final_cost), 0); at (1, 1) the products are exact.  The linear lattice carries the scaled weights.
  LinearLattice ShortestPath(float graph_scale = 1.0f, float acoustic_scale = 1.0f) const;
  // What khg_lattices_best_path gives for one lattice and one scale pair; nothing throws on a negative epsilon cycle (KHG_LAT_EPS_LOOP)
  LatticeBestPath BestPath(float graph_scale = 1.0f, float acoustic_scale = 1.0f) const;
  // lattice-prune under scales (what khg_lattices_prune gives): the states and arcs whose best path through them is within `beam` of the
  // best path (sums in the association order of DESIGN.md 7e), plus the best path itself; states and arcs keep their order, costs
  // stay unscaled.  No reachable final state, or a negative epsilon cycle: an empty lattice; *status the KHG_LAT_* bits.
  std::shared_ptr<Lattice> Prune(float beam, float graph_scale = 1.0f, float acoustic_scale = 1.0f, int* status = nullptr) const;
  // LatticeForwardBackward / lattice-to-post in the log semiring, float64, serially in state order: an arc's
  // log-likelihood is -(graph_scale * graph_cost + acoustic_scale * acoustic_cost), no acoustic term on an epsilon arc; a final state's
  // -graph_scale * final_cost on the last frame.  Every arc must go to a higher state: an epsilon arc that does not gives
  // KHG_LAT_EPS_LOOP (checked on the structure, before any arithmetic).  Each log-sum is max-then-sum over a state's arcs in arc order.
  LatticePosteriors ForwardBackward(float graph_scale = 1.0f, float acoustic_scale = 1.0f) const;
  // LatticeForwardBackwardMpeVariants: ForwardBackward's likelihood part, and beside it the expected frame accuracy in
  // the linear domain, serially in state order.  smbr: an arc matches the reference by pdf (tid2pdf), else by phone; the alignment has
  // one id per frame.  tid2phone / tid2pdf have an entry per transition-id and entry 0 (tid2pdf may be empty unless smbr).
  LatticeMpePosteriors ForwardBackwardMpe(const std::vector<int32_t>& tid2phone, const std::vector<int32_t>& tid2pdf,
                                          const std::vector<int32_t>& silence_phones, const std::vector<int32_t>& alignment, bool smbr,
                                          bool one_silence_class, float graph_scale = 1.0f, float acoustic_scale = 1.0f) const;
  // gmm-rescore-lattice (what khg_lattices_rescore gives for one lattice): a copy in which every arc with ilabel != 0
  // leaving a state of frame t has acoustic_cost = -(acoustic_scale * loglike(t, ilabel)), one float multiply and a sign; everything
  // else as stored (tot_cost / extra_cost are then stale)
  std::shared_ptr<Lattice> Rescore(const std::function<float(int, int)>& loglike, float acoustic_scale = 1.0f) const;
  // lattice-boost-ali (Kaldi's LatticeBoost; what khg_lattices_boost gives for one lattice): a copy in which every arc with ilabel != 0
  // at frame t has graph_cost = fl(graph_cost + fl(-b * e)), e = 0 where tid2phone[ilabel] == tid2phone[alignment[t]], max_silence_error
  // where they differ and the arc's phone is a silence phone, 1 otherwise.  tid2phone[0] is unused.  The alignment has one id in
  // 1 .. tid2phone.size() - 1 per frame of the lattice, and every ilabel lies in that range.
  std::shared_ptr<Lattice> Boost(const std::vector<int32_t>& tid2phone, const std::vector<int32_t>& silence_phones,
                                 const std::vector<int32_t>& alignment, float b, float max_silence_error) const;
  // lattice-lmrescore (what khg_lattices_lm_rescore gives for one lattice): every state split by the LM histories that
  // reach it, every arc with a word given fl(scale * the LM's cost of the word) more graph cost; the rule is stated at
  // khg_lattices_lm_rescore.  The history sets may hold min(hist_factor * states, 2^31 - 1) entries together (KHG_LAT_SCRATCH).
  LatticeLmRescored LmRescore(const BackoffLm& lm, float scale = 1.0f, int hist_factor = 8) const;
  // lattice-determinize-pruned (what khg_lattices_determinize gives for one lattice): one path per word sequence of the
  // beam-pruned lattice, the cheapest, made of copies of its arcs; the rule is stated at khg_lattices_determinize, and this is it, serially
  LatticeDeterminized Determinize(float graph_scale = 1.0f, float acoustic_scale = 1.0f, float beam = 10.0f, float delta = 1.0f / 1024.0f,
                                  int state_factor = 8) const;
  // lattice-to-nbest | nbest-to-linear (what khg_lattices_nbest gives for one lattice): the n cheapest paths under the
  // scalar key of the rule stated at khg_lattices_nbest, and this is it, serially -- every candidate of a state is generated, the lot
  // is sorted by (t', e, j) and cut at n; no merge.  *status: the KHG_LAT_* bits (SUCCEEDED, NO_PATH, EPS_LOOP, SCRATCH).
  std::vector<LatticeNbestEntry> Nbest(int n, float graph_scale = 1.0f, float acoustic_scale = 1.0f, int* status = nullptr) const;
  // lattice-add-penalty (what khg_lattices_add_penalty gives for one lattice): a copy in which every arc with olabel != 0 has
  // graph_cost = fl(graph_cost + word_ins_penalty); everything else as stored
  std::shared_ptr<Lattice> AddPenalty(float word_ins_penalty) const;
  // lattice-oracle: the path with the fewest word errors against `ref` (words > 0), sequentially, cell by cell, by the
  // rule written at khg_lattices_oracle in include/khg_hip.h
  LatticeOracle Oracle(const std::vector<int32_t>& ref) const;
  // lattice-mbr-decode and the confidences of lattice-to-ctm-conf: the rule written at khg_lattices_mbr in
  // include/khg_hip.h, serially.  init: the initial hypothesis (nullptr: BestPath's words at the same pair).  arc_cond / final_cond
  // (one per arc / per state; both or neither) replace the weights the host would compute from ForwardBackward's alpha: given the
  // device's, every other output equals the device's bit for bit.
  LatticeMbr Mbr(float graph_scale, float acoustic_scale, bool decode_mbr = true, int max_iter = 32, const std::vector<int32_t>* init = nullptr,
                 int max_words = 0, const std::vector<double>* arc_cond = nullptr, const std::vector<double>* final_cond = nullptr) const;
  // Kaldi's text form of a lattice: "src dst ilabel olabel graph,acoustic" per arc, "state graph,acoustic" per final state
  std::string ToText() const;

 private:
  void Check(int s) const { KHG_REQUIRE(s >= 0 && s < NumStates(), "Lattice: bad state"); }
  bool Forward(float gs, float as, std::vector<float>* d1, std::vector<float>* d2, std::vector<int32_t>* bp) const;
  bool Backward(float gs, float as, std::vector<float>* e1, std::vector<float>* e2) const;
};

// GetRawLattice for a batch (the data-parallel lattice-simple decoder, khg_decode_lattice_simple_raw): what DecodeLatticeSimpleBatch
// returns, and in (*lattices)[u] the raw lattice of utterance u (no states unless it succeeded).  seconds (optional, 2 entries): the
// time of the C-ABI decode call and of the download of the lattices.
std::vector<LatticeResult> GetRawLatticeSimpleBatch(const AmDiagGmm& am, const TransitionModel& tm, const GraphsCsr& graphs,
                                                    const std::vector<const float*>& feats, const std::vector<int64_t>& nframes,
                                                    const LatticeSimpleDecoderConfig& config, float acoustic_scale, bool return_scores,
                                                    int scratch_per_frame, std::vector<std::shared_ptr<Lattice>>* lattices,
                                                    double* seconds = nullptr);

// every utterance's lattice of a khg_lattices handle, downloaded (khg_lattices_download)
std::vector<std::shared_ptr<Lattice>> DownloadLattices(khg_ctx* ctx, const khg_lattices* h);
// The same decode that keeps the batch's raw lattices on the device: *lattices is the khg_lattices handle (the caller frees it with
// khg_lattices_destroy), on the default context; nothing is downloaded.
std::vector<LatticeResult> GetRawLatticeSimpleDeviceBatch(const AmDiagGmm& am, const TransitionModel& tm, const GraphsCsr& graphs,
                                                          const std::vector<const float*>& feats, const std::vector<int64_t>& nframes,
                                                          const LatticeSimpleDecoderConfig& config, float acoustic_scale, bool return_scores,
                                                          int scratch_per_frame, khg_lattices** lattices);

// The same two for the lattice-faster decoder (khg_decode_lattice_faster_raw): what DecodeLatticeBatch returns plus the raw lattices
std::vector<LatticeResult> GetRawLatticeFasterBatch(const AmDiagGmm& am, const TransitionModel& tm, const GraphsCsr& graphs,
                                                    const std::vector<const float*>& feats, const std::vector<int64_t>& nframes,
                                                    const LatticeFasterDecoderConfig& config, float acoustic_scale, bool allow_partial,
                                                    bool return_scores, int scratch_per_frame, std::vector<std::shared_ptr<Lattice>>* lattices,
                                                    double* seconds = nullptr);
std::vector<LatticeResult> GetRawLatticeFasterDeviceBatch(const AmDiagGmm& am, const TransitionModel& tm, const GraphsCsr& graphs,
                                                          const std::vector<const float*>& feats, const std::vector<int64_t>& nframes,
                                                          const LatticeFasterDecoderConfig& config, float acoustic_scale, bool allow_partial,
                                                          bool return_scores, int scratch_per_frame, khg_lattices** lattices);

// python/csrc/faster-decoder.cc:33-53 on the GPU path: Decode runs K1 + K2 for the utterance of a DecodableAmDiagGmmScaled (any other
// DecodableInterface: its sampled scores + K2, AlignDecodable above) with the options' beam / max_active / min_active / beam_delta /
// hash_ratio (no retry); GetBestPath rebuilds the linear lattice of
// csrc/faster-decoder.cc:355-423 from the alignment: arc weights (graph cost, acoustic cost) per token, final weight, true epsilons
// removed.  Whole utterances only: AdvanceDecoding with a frame limit is not supported.
class FasterDecoder {
 public:
  FasterDecoder(std::shared_ptr<StdVectorFst> fst, const FasterDecoderOptions& config) : fst_(std::move(fst)) { SetOptions(config); }
  void SetOptions(const FasterDecoderOptions& config);
  void InitDecoding();
  void Decode(const std::shared_ptr<DecodableInterface>& decodable) { InitDecoding(); AdvanceDecoding(decodable, -1); }
  void AdvanceDecoding(const std::shared_ptr<DecodableInterface>& decodable, int max_num_frames);
  int NumFramesDecoded() const { return nframes_; }
  bool ReachedFinal() const { return has_res_ && res_.ok; }
  bool GetBestPath(LinearLattice* lat, bool use_final_probs) const;

 private:
  std::shared_ptr<StdVectorFst> fst_;
  FasterDecoderOptions cfg_;
  std::shared_ptr<DecodableInterface> dec_;
  AlignResult res_;
  std::vector<double> ac_;           // acoustic cost of each aligned frame: -(score the decoder read for (frame, alignment[frame]))
  bool has_res_ = false;
  int nframes_ = -1;
};

}  // namespace khg
