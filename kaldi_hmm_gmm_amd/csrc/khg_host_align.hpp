// Host-side C++ of the alignment API: AlignConfig, FasterDecoderOptions, DecodableAmDiagGmmUnmapped / Scaled and the batched
// AlignUtteranceWrapper over resident graphs.
//
// Mirrors (reference, /root/reference/kaldi-hmm-gmm/): csrc/decoder-wrappers.{h,cc} (AlignConfig :23-37, AlignUtteranceWrapper
// :16-108), csrc/faster-decoder.h:24-63 (FasterDecoderOptions), csrc/decodable-am-diag-gmm.h:30-103; pybind surface
// python/csrc/{decoder-wrappers,faster-decoder,decodable-am-diag-gmm}.cc.  The work is K1 (log-likes) + K2 (Viterbi) through the
// C-ABI, for one utterance or a whole batch; graphs come as the CSR block of khg_utts_create (the reference holds them in
// kaldifst's fst::VectorFst<StdArc>, a third-party container that stays on the Python side here).
#pragma once
#include <limits>

#include "khg_host_gmm.hpp"
#include "khg_host_hmm.hpp"

namespace khg {

struct AlignConfig {                 // csrc/decoder-wrappers.h:23-37
  float beam = 200.0f, retry_beam = 0.0f;
  bool careful = false;
};

struct FasterDecoderOptions {        // csrc/faster-decoder.h:24-63
  float beam = 16.0f;
  int32_t max_active = std::numeric_limits<int32_t>::max(), min_active = 20;
  float beam_delta = 0.5f, hash_ratio = 2.0f;
  std::string ToString() const;
};

struct DeterminizeLatticePhonePrunedOptions {   // csrc/determinize-lattice-pruned.h:53-95 (stored only: nothing determinises)
  float delta = 1.0f / 1024.0f;                  // fst::kDelta
  int32_t max_mem = 50000000;
  bool phone_determinize = true, word_determinize = true, minimize = false;
  std::string ToString() const;
};

struct LatticeFasterDecoderConfig {             // csrc/lattice-faster-decoder.h:30-105
  float beam = 16.0f;
  int32_t max_active = std::numeric_limits<int32_t>::max(), min_active = 200;
  float lattice_beam = 10.0f;
  int32_t prune_interval = 25;
  bool determinize_lattice = true;
  float beam_delta = 0.5f, hash_ratio = 2.0f, prune_scale = 0.1f;
  int32_t memory_pool_tokens_block_size = 1 << 8, memory_pool_links_block_size = 1 << 8;
  DeterminizeLatticePhonePrunedOptions det_opts;
  std::string ToString() const;
  void Check() const;
};

struct LatticeSimpleDecoderConfig {            // csrc/lattice-simple-decoder.h:26-79
  float beam = 16.0f, lattice_beam = 10.0f;
  int32_t prune_interval = 25;
  bool determinize_lattice = true;
  // the reference's ToString prints prune_lattice, which its constructor never initialises and pybind never binds: False here
  bool prune_lattice = false;
  float beam_ratio = 0.9f, prune_scale = 0.1f;
  DeterminizeLatticePhonePrunedOptions det_opts;
  std::string ToString() const;
  void Check() const;
};

struct LatticeResult {               // DecodeUtteranceLatticeFaster's (succeeded, alignment, words, like) + the KHG_LAT_* bits
  int status = 0;
  int err_frame = -1;                // the lattice-simple decoder's KHG_LAT_NO_EPS_TOKEN frame
  bool succeeded = false, partial = false;
  std::vector<int32_t> alignment, words;
  double like = 0.0;
  int num_frames = 0;
  std::vector<float> loglikes;       // [npdf][T] (return_scores)
  std::vector<int32_t> pdfs;
};

struct GraphsCsr {                   // fst::VectorFst<StdArc> per utterance, concatenated as khg_utts_create takes them
  std::vector<int64_t> state_off, arc_off;
  std::vector<int32_t> start, ilabel, olabel, nextstate;
  std::vector<float> weight, final_w;
  // One decoding graph for the whole batch (decoding: one HCLG, many utterances): the arrays above hold that ONE graph
  // (state_off = {0, S}), or nothing when `device` is a graph already resident (khg_graph_create; borrowed).  The batch entry
  // points then build their set with khg_utts_create_on_graph: planned and uploaded once, not once per utterance.
  bool shared = false;
  khg_graph* device = nullptr;
};
// the batch's utterance set: khg_utts_create (one graph per utterance), or khg_utts_create_on_graph for a shared graph
void CreateBatchSet(khg_ctx* ctx, khg_tm* tm, const GraphsCsr& g, int n_utt, int dim, const int64_t* frame_off, const float* feats, khg_utts** out);

// csrc/decodable-itf.h: what a decoder asks of an acoustic model (1-based index, 0-based frame).  The HIP kernels read scores from
// K1's matrices, so the classes below are what the alignment entry points accept; the interface itself is there for callers
// that score frames from Python or C++ through the reference's protocol.
class DecodableInterface {
 public:
  virtual ~DecodableInterface() = default;
  virtual float LogLikelihood(int frame, int index) const = 0;
  virtual bool IsLastFrame(int frame) const = 0;
  virtual int NumFramesReady() const { throw Error("NumFramesReady() not implemented for this decodable type."); }
  virtual int NumIndices() const = 0;
};

// csrc/decodable-am-diag-gmm.h:30-78: (frame, pdf-id + 1) -> log-likelihood.  Scores for every pdf are produced by one K1 launch
// on first use and kept (the reference's one-frame cache).
// NOTE (DecodableInterface above): LogLikelihood is declared const here; the reference's is non-const because of that cache.
class DecodableAmDiagGmmUnmapped : public DecodableInterface {
 public:
  DecodableAmDiagGmmUnmapped(std::shared_ptr<AmDiagGmm> am, const float* feats, int64_t T, int D);
  float LogLikelihood(int frame, int index) const override { return ZeroBased(frame, index - 1); }
  float ZeroBased(int frame, int state) const;
  int NumFramesReady() const override { return (int)T_; }
  int NumIndices() const override { return am_->NumPdfs(); }
  bool IsLastFrame(int frame) const override;
  const std::shared_ptr<AmDiagGmm>& am() const { return am_; }
  const std::vector<float>& feats() const { return feats_; }
  int Dim() const { return D_; }

 protected:
  const std::vector<float>& Scores() const;
  std::shared_ptr<AmDiagGmm> am_;
  std::vector<float> feats_;
  int64_t T_;
  int D_;
  mutable std::vector<float> ll_;    // [num_pdfs][T], filled on first use
};

// csrc/decodable-am-diag-gmm.h:83-103: scale * LL(frame, TransitionIdToPdf(tid))
class DecodableAmDiagGmmScaled : public DecodableAmDiagGmmUnmapped {
 public:
  DecodableAmDiagGmmScaled(std::shared_ptr<AmDiagGmm> am, std::shared_ptr<TransitionModel> tm, const float* feats, int64_t T, int D, float scale)
      : DecodableAmDiagGmmUnmapped(std::move(am), feats, T, D), tm_(std::move(tm)), scale_(scale) {}
  float LogLikelihood(int frame, int tid) const override { return scale_ * ZeroBased(frame, tm_->TransitionIdToPdf(tid)); }
  int NumIndices() const override { return tm_->NumTransitionIds(); }
  const std::shared_ptr<TransitionModel>& tm() const { return tm_; }
  float scale() const { return scale_; }

 private:
  std::shared_ptr<TransitionModel> tm_;
  float scale_;
};

// csrc/decodable-ctc.{h,cc}: LogLikelihood(frame, index) = feats(frame, index - 1) of a [frames][indices] matrix.  The decode paths
// copy the matrix straight into the score layout (Row), with no call per cell.
class DecodableCtc : public DecodableInterface {
 public:
  DecodableCtc(const float* feats, int64_t rows, int64_t cols) : m_(feats, feats + rows * cols), rows_((int)rows), cols_((int)cols) {}
  float LogLikelihood(int frame, int index) const override;
  int NumFramesReady() const override { return rows_; }
  int NumIndices() const override { return cols_; }
  bool IsLastFrame(int frame) const override { return frame == rows_ - 1; }
  const float* Row(int frame) const { return m_.data() + (size_t)frame * (size_t)cols_; }

 private:
  std::vector<float> m_;
  int rows_, cols_;
};
// score of (frame, index) for the decode paths: DecodableCtc's matrix read directly (ctc from one dynamic_cast), else the interface
inline float DecodableScore(const DecodableInterface& dec, const DecodableCtc* ctc, int frame, int index) {
  return ctc ? ctc->Row(frame)[index - 1] : dec.LogLikelihood(frame, index);
}

struct AlignResult {
  bool ok = false, retried = false;
  int status = 0;
  std::vector<int32_t> alignment, words;
  float like = 0.0f;
  int num_frames = 0;
  std::vector<float> loglikes;       // [npdf][T] of the utterance's own pdf list (return_scores)
  std::vector<int32_t> pdfs;
};

// Batched AlignUtteranceWrapper: all utterances in one K1 + K2 pass.  The graphs carry their final arc weights unless trans_cost
// (per-tid additive cost, TransitionModel::ScaledTransCost) is given, in which case it is added on the device.  config.careful
// only tells K2 the graphs were doubled (the caller applied ModifyGraphForCarefulAlignment / khg_careful_graph).
std::vector<AlignResult> AlignBatch(const AmDiagGmm& am, const TransitionModel& tm, const GraphsCsr& graphs, const std::vector<const float*>& feats,
                                    const std::vector<int64_t>& nframes, const AlignConfig& config, float acoustic_scale, const float* trans_cost,
                                    const FasterDecoderOptions* decoder_opts, bool return_scores, float like_scale = 0.0f);
// (like_scale: divisor of `like` when it is not the score scale -- a decodable whose own scale differs from the wrapper's
// acoustic_scale argument, csrc/decoder-wrappers.cc:95; 0 = acoustic_scale)

// DecodeUtteranceLatticeFaster (csrc/decoder-wrappers.cc:186-224) for a batch: K1 (every pdf of each utterance's graph) + the lattice
// decoder (khg_decode_lattice_faster), each utterance on a fresh decoder; scores scaled by acoustic_scale (DecodableAmDiagGmmScaled).
// scratch_per_frame: 0 = the C-ABI's automatic size.
std::vector<LatticeResult> DecodeLatticeBatch(const AmDiagGmm& am, const TransitionModel& tm, const GraphsCsr& graphs, const std::vector<const float*>& feats,
                                              const std::vector<int64_t>& nframes, const LatticeFasterDecoderConfig& config, float acoustic_scale,
                                              bool allow_partial, bool return_scores, int scratch_per_frame = 0);
// the C-ABI call on a prepared set (scores resident) -> results without scores
std::vector<LatticeResult> DecodeLatticeOnSet(khg_ctx* ctx, khg_tm* tm, khg_utts* us, const std::vector<int64_t>& frame_off,
                                              const LatticeFasterDecoderConfig& config, float acoustic_scale, bool allow_partial, int scratch_per_frame,
                                              int64_t total_states, khg_lattices** lattices = nullptr);
// (lattices: khg_decode_lattice_faster_raw instead, the batch's raw lattices left on the device for the caller to download and destroy)

// DecodeUtteranceLatticeSimple (csrc/decoder-wrappers.cc:142-182) for a batch: K1 as in DecodeLatticeBatch + the data-parallel
// lattice-simple decoder (khg_decode_lattice_simple).  scratch_per_frame: the most live tokens a frame may hold (0: no limit).
std::vector<LatticeResult> DecodeLatticeSimpleBatch(const AmDiagGmm& am, const TransitionModel& tm, const GraphsCsr& graphs,
                                                    const std::vector<const float*>& feats, const std::vector<int64_t>& nframes,
                                                    const LatticeSimpleDecoderConfig& config, float acoustic_scale, bool allow_partial,
                                                    bool return_scores, int scratch_per_frame = 0);
std::vector<LatticeResult> DecodeLatticeSimpleOnSet(khg_ctx* ctx, khg_tm* tm, khg_utts* us, const std::vector<int64_t>& frame_off,
                                                    const LatticeSimpleDecoderConfig& config, float acoustic_scale, bool allow_partial,
                                                    int scratch_per_frame, int64_t total_states, khg_lattices** lattices = nullptr);
// (lattices: khg_decode_lattice_simple_raw instead, the batch's raw lattices left on the device for the caller to download and destroy)

}  // namespace khg
