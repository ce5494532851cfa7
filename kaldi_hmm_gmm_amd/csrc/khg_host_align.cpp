// Implementation of khg_host_align.hpp: see the header for what each piece mirrors in the reference.
#include "khg_host_align.hpp"

#include <chrono>
#include <cstdio>
#include <sstream>

#include "khg_host_fst.hpp"

namespace khg {

std::string FasterDecoderOptions::ToString() const {
  char buf[256];
  std::snprintf(buf, sizeof(buf), "FasterDecoderOptions(beam=%g, max_active=%d, min_active=%d, beam_delta=%g, hash_ratio=%g)", (double)beam, max_active,
                min_active, (double)beam_delta, (double)hash_ratio);
  return buf;
}

DecodableAmDiagGmmUnmapped::DecodableAmDiagGmmUnmapped(std::shared_ptr<AmDiagGmm> am, const float* feats, int64_t T, int D)
    : am_(std::move(am)), feats_(feats, feats + (size_t)T * D), T_(T), D_(D) {
  KHG_REQUIRE(am_ != nullptr, "DecodableAmDiagGmm: no model");
}
const std::vector<float>& DecodableAmDiagGmmUnmapped::Scores() const {
  if (ll_.empty() && T_ > 0) {
    KHG_REQUIRE(am_->Dim() == D_, "Dim mismatch: data dim = " + std::to_string(D_) + " vs. model dim = " + std::to_string(am_->Dim()));
    std::vector<int32_t> pdfs((size_t)am_->NumPdfs());
    for (int p = 0; p < am_->NumPdfs(); ++p) pdfs[(size_t)p] = p;
    ll_ = GpuLoglikesOn(am_->DeviceModel(DefaultCtx()), D_, feats_.data(), T_, pdfs.data(), am_->NumPdfs());
  }
  return ll_;
}
float DecodableAmDiagGmmUnmapped::ZeroBased(int frame, int state) const {
  KHG_REQUIRE(frame >= 0 && frame < NumFramesReady(), "frame < NumFramesReady() assertion failed");
  KHG_REQUIRE(state >= 0 && state < am_->NumPdfs(), "Likely graph/model mismatch, e.g. using wrong HCLG.fst");
  return Scores()[(size_t)state * (size_t)T_ + (size_t)frame];
}
bool DecodableAmDiagGmmUnmapped::IsLastFrame(int frame) const {
  KHG_REQUIRE(frame < NumFramesReady(), "frame < NumFramesReady() assertion failed");
  return frame == NumFramesReady() - 1;
}

std::string DeterminizeLatticePhonePrunedOptions::ToString() const {
  std::ostringstream os;                       // determinize-lattice-pruned.h:85-94
  os << "DeterminizeLatticePhonePrunedOptions(" << "delta=" << delta << ", " << "max_mem=" << max_mem << ", "
     << "phone_determinize=" << (phone_determinize ? "True" : "False") << ", " << "word_determinize=" << (word_determinize ? "True" : "False")
     << ", " << "minimize=" << (minimize ? "True" : "False") << ")";
  return os.str();
}
std::string LatticeFasterDecoderConfig::ToString() const {
  std::ostringstream os;                       // lattice-faster-decoder.h:77-97
  os << "LatticeFasterDecoderConfig(" << "beam=" << beam << ", " << "max_active=" << max_active << ", " << "min_active=" << min_active << ", "
     << "lattice_beam=" << lattice_beam << ", " << "prune_interval=" << prune_interval << ", "
     << "determinize_lattice=" << (determinize_lattice ? "True" : "False") << ", " << "beam_delta=" << beam_delta << ", "
     << "hash_ratio=" << hash_ratio << ", " << "prune_scale=" << prune_scale << ", " << "memory_pool_tokens_block_size=" << memory_pool_tokens_block_size
     << ", " << "memory_pool_links_block_size=" << memory_pool_links_block_size << ")";
  return os.str();
}
void LatticeFasterDecoderConfig::Check() const {    // lattice-faster-decoder.h:99-104
  KHG_REQUIRE(beam > 0.0 && max_active > 1 && lattice_beam > 0.0 && min_active <= max_active && prune_interval > 0 && beam_delta > 0.0 &&
                  hash_ratio >= 1.0 && prune_scale > 0.0 && prune_scale < 1.0,
              "beam > 0.0 && max_active > 1 && lattice_beam > 0.0 && min_active <= max_active && prune_interval > 0 && beam_delta > 0.0 && "
              "hash_ratio >= 1.0 && prune_scale > 0.0 && prune_scale < 1.0 assertion failed");
}

std::string LatticeSimpleDecoderConfig::ToString() const {
  std::ostringstream os;                       // lattice-simple-decoder.h:59-74
  os << "LatticeSimpleDecoderConfig(" << "beam=" << beam << ", " << "lattice_beam=" << lattice_beam << ", " << "prune_interval=" << prune_interval
     << ", " << "determinize_lattice=" << (determinize_lattice ? "True" : "False") << ", " << "prune_lattice=" << (prune_lattice ? "True" : "False")
     << ", " << "beam_ratio=" << beam_ratio << ", " << "prune_scale=" << prune_scale << ", " << "det_opts=" << det_opts.ToString() << ")";
  return os.str();
}
void LatticeSimpleDecoderConfig::Check() const {    // lattice-simple-decoder.h:76-78 (KHG_ASSERT)
  KHG_REQUIRE(beam > 0.0 && lattice_beam > 0.0 && prune_interval > 0, "Check failed!\nx: beam > 0.0 && lattice_beam > 0.0 && prune_interval > 0");
}

float DecodableCtc::LogLikelihood(int frame, int index) const {    // decodable-ctc.cc:15-22 (its assert is compiled out there)
  KHG_REQUIRE(index >= 1, "DecodableCtc: index >= 1 assertion failed");
  KHG_REQUIRE(frame >= 0 && frame < rows_ && index <= cols_, "DecodableCtc: (frame, index) out of range");
  return Row(frame)[index - 1];
}

namespace {
struct UttsH { khg_utts* h = nullptr; ~UttsH() { if (h) khg_utts_destroy(h); } };
std::string G(double x) { char b[64]; std::snprintf(b, sizeof(b), "%g", x); return b; }
}  // namespace

void CreateBatchSet(khg_ctx* ctx, khg_tm* tm, const GraphsCsr& g, int n_utt, int dim, const int64_t* frame_off, const float* feats, khg_utts** out) {
  if (!g.shared) {
    CApi(khg_utts_create(ctx, tm, n_utt, dim, frame_off, feats, nullptr, g.state_off.data(), g.start.data(), g.arc_off.data(), g.ilabel.data(),
                         g.olabel.data(), g.weight.data(), g.nextstate.data(), g.final_w.data(), out));
    return;
  }
  struct GraphH { khg_graph* h = nullptr; ~GraphH() { if (h) khg_graph_destroy(h); } } own;     // (the set keeps its own reference)
  khg_graph* dg = g.device;
  if (!dg) {
    CApi(khg_graph_create(ctx, tm, (int32_t)g.state_off.back(), g.start[0], g.arc_off.data(), g.ilabel.data(), g.olabel.data(), g.weight.data(),
                          g.nextstate.data(), g.final_w.data(), &own.h));
    dg = own.h;
  }
  CApi(khg_utts_create_on_graph(ctx, tm, dg, n_utt, dim, frame_off, feats, nullptr, out));
}
namespace {
// one graph per utterance, or one for all of them
bool GraphsFit(const GraphsCsr& g, int n_utt) {
  if (g.shared) return g.device || (g.start.size() == 1 && g.state_off.size() == 2);
  return (int)g.start.size() == n_utt && (int)g.state_off.size() == n_utt + 1;
}
// bound on the states under all utterances (the words a lattice decode can return: frames + states + 64 per utterance)
int64_t BatchStates(const GraphsCsr& g, int n_utt) {
  if (!g.shared) return g.state_off.back();
  int64_t S = g.state_off.empty() ? 0 : g.state_off.back();
  if (g.device) CApi(khg_graph_info(g.device, &S, nullptr, nullptr, nullptr, nullptr));
  return S * (int64_t)n_utt;
}
}  // namespace

std::vector<AlignResult> AlignBatch(const AmDiagGmm& am, const TransitionModel& tm, const GraphsCsr& g, const std::vector<const float*>& feats,
                                    const std::vector<int64_t>& nframes, const AlignConfig& config, float acoustic_scale, const float* trans_cost,
                                    const FasterDecoderOptions* dopts, bool return_scores, float like_scale) {
  KHG_REQUIRE(!((config.retry_beam != 0 && config.retry_beam <= config.beam) || config.beam <= 0.0f),
              "Beams do not make sense: beam " + G(config.beam) + ", retry-beam " + G(config.retry_beam));   // csrc/decoder-wrappers.cc:29-33
  const int n_utt = (int)feats.size(), D = am.Dim();
  KHG_REQUIRE((int)nframes.size() == n_utt && GraphsFit(g, n_utt), "AlignBatch: one graph and one feature matrix per utterance");
  khg_ctx* ctx = DefaultCtx();
  // the model and the transition table live on the device across calls: cached on the host objects, uploaded again only when they
  // changed (AmDiagGmm::DeviceModel / TransitionModel::DeviceTm) -- the scripts call this once per utterance
  struct { khg_model* h; } dm{am.DeviceModel(ctx)};
  struct { khg_tm* h; } dt{tm.DeviceTm(ctx)};
  UttsH us;
  CApi(khg_tm_set_trans_cost(dt.h, trans_cost));
  std::vector<int64_t> frame_off((size_t)n_utt + 1, 0);
  for (int u = 0; u < n_utt; ++u) frame_off[(size_t)u + 1] = frame_off[(size_t)u] + nframes[(size_t)u];
  std::vector<float> all;
  const float* fp = nullptr;
  if (n_utt == 1) fp = feats[0];            // one utterance: its matrix as it is
  else {
    all.resize((size_t)std::max<int64_t>(frame_off[(size_t)n_utt], 1) * D);
    for (int u = 0; u < n_utt; ++u)
      if (nframes[(size_t)u] > 0) std::memcpy(all.data() + (size_t)frame_off[(size_t)u] * D, feats[(size_t)u], sizeof(float) * (size_t)nframes[(size_t)u] * D);
    fp = all.data();
  }
  static const float kNoFrames[1] = {0.0f};
  if (!fp) fp = kNoFrames;
  CreateBatchSet(ctx, dt.h, g, n_utt, D, frame_off.data(), fp, &us.h);
  // only the cells a decoder token can read; with a wide beam (few failed beam certificates to repair) also not the cells that only
  // tokens past any accepting path read (khg_loglikes_band: identical alignments, ~13 % fewer cells on chain graphs)
  if (config.beam >= 100.0f) CApi(khg_loglikes_band(ctx, dm.h, us.h));
  else CApi(khg_loglikes_reachable(ctx, dm.h, us.h));
  khg_align_config c;
  khg_align_config_default(&c);
  c.beam = config.beam; c.retry_beam = config.retry_beam; c.careful = config.careful ? 1 : 0; c.acoustic_scale = acoustic_scale;
  c.like_scale = like_scale;
  if (dopts) { c.max_active = dopts->max_active; c.min_active = dopts->min_active; c.beam_delta = dopts->beam_delta; c.hash_ratio = dopts->hash_ratio; }
  const int64_t N = frame_off[(size_t)n_utt], wcap = N + 16 * (int64_t)n_utt + 1024;
  std::vector<int32_t> ali((size_t)std::max<int64_t>(N, 1)), words((size_t)wcap), status((size_t)n_utt);
  std::vector<int64_t> woff((size_t)n_utt + 1, 0);
  std::vector<float> like((size_t)n_utt);
  CApi(khg_align(ctx, dt.h, us.h, &c, ali.data(), words.data(), woff.data(), wcap, like.data(), status.data()));
  std::vector<float> scores;
  std::vector<int64_t> ll_off((size_t)n_utt + 1, 0), pdf_off((size_t)n_utt + 1, 0);
  std::vector<int32_t> pdfs;
  if (return_scores) {
    int64_t total = 0;
    CApi(khg_loglikes_layout(us.h, ll_off.data(), &total));
    scores.resize((size_t)std::max<int64_t>(total, 1));
    CApi(khg_loglikes_download(ctx, us.h, scores.data()));
    CApi(khg_utts_num_pdfs(us.h, pdf_off.data()));
    pdfs.resize((size_t)std::max<int64_t>(pdf_off[(size_t)n_utt], 1));
    CApi(khg_utts_pdfs(us.h, pdfs.data()));
  }
  std::vector<AlignResult> out((size_t)n_utt);
  for (int u = 0; u < n_utt; ++u) {
    AlignResult& r = out[(size_t)u];
    r.status = status[(size_t)u];
    r.ok = (r.status & KHG_ALIGN_ERROR) == 0;
    r.retried = (r.status & KHG_ALIGN_RETRIED) != 0;
    r.num_frames = (int)nframes[(size_t)u];
    if (r.ok) {
      r.alignment.assign(ali.begin() + frame_off[(size_t)u], ali.begin() + frame_off[(size_t)u + 1]);
      r.words.assign(words.begin() + woff[(size_t)u], words.begin() + woff[(size_t)u + 1]);
      r.like = like[(size_t)u];
    }
    if (return_scores) {
      const int64_t T = nframes[(size_t)u], tpad = (T + 31) & ~int64_t(31);
      const int npdf = (int)(pdf_off[(size_t)u + 1] - pdf_off[(size_t)u]);
      r.pdfs.assign(pdfs.begin() + pdf_off[(size_t)u], pdfs.begin() + pdf_off[(size_t)u + 1]);
      r.loglikes.resize((size_t)npdf * (size_t)T);
      for (int j = 0; j < npdf; ++j)
        if (T > 0) std::memcpy(r.loglikes.data() + (size_t)j * T, scores.data() + ll_off[(size_t)u] + (size_t)j * tpad, sizeof(float) * (size_t)T);
    }
  }
  return out;
}

std::vector<LatticeResult> DecodeLatticeOnSet(khg_ctx* ctx, khg_tm* tm, khg_utts* us, const std::vector<int64_t>& frame_off,
                                              const LatticeFasterDecoderConfig& config, float acoustic_scale, bool allow_partial, int scratch_per_frame,
                                              int64_t total_states, khg_lattices** lattices) {
  const int n_utt = (int)frame_off.size() - 1;
  khg_lattice_faster_config c;
  khg_lattice_faster_config_default(&c);
  c.beam = config.beam; c.max_active = config.max_active; c.min_active = config.min_active; c.lattice_beam = config.lattice_beam;
  c.prune_interval = config.prune_interval; c.beam_delta = config.beam_delta; c.hash_ratio = config.hash_ratio; c.prune_scale = config.prune_scale;
  c.acoustic_scale = acoustic_scale; c.allow_partial = allow_partial ? 1 : 0; c.scratch_per_frame = scratch_per_frame;
  const int64_t N = frame_off[(size_t)n_utt];
  std::vector<int64_t> woff((size_t)n_utt + 1, 0);
  std::vector<int32_t> ali((size_t)std::max<int64_t>(N, 1)), status((size_t)n_utt);
  std::vector<double> like((size_t)n_utt);
  // words: the C-ABI keeps at most frames + states + 64 per utterance
  std::vector<int32_t> words((size_t)(N + total_states + 64 * (int64_t)n_utt + 16));
  if (lattices)
    CApi(khg_decode_lattice_faster_raw(ctx, tm, us, &c, ali.data(), words.data(), woff.data(), (int64_t)words.size(), like.data(), status.data(),
                                       lattices));
  else
    CApi(khg_decode_lattice_faster(ctx, tm, us, &c, ali.data(), words.data(), woff.data(), (int64_t)words.size(), like.data(), status.data()));
  std::vector<LatticeResult> out((size_t)n_utt);
  for (int u = 0; u < n_utt; ++u) {
    LatticeResult& r = out[(size_t)u];
    r.status = status[(size_t)u];
    r.succeeded = (r.status & KHG_LAT_SUCCEEDED) != 0;
    r.partial = (r.status & KHG_LAT_PARTIAL) != 0;
    r.num_frames = (int)(frame_off[(size_t)u + 1] - frame_off[(size_t)u]);
    if (r.succeeded) {
      r.alignment.assign(ali.begin() + frame_off[(size_t)u], ali.begin() + frame_off[(size_t)u + 1]);
      r.words.assign(words.begin() + woff[(size_t)u], words.begin() + woff[(size_t)u + 1]);
      r.like = like[(size_t)u];
    }
  }
  return out;
}

namespace {
// K1 (every pdf of each utterance's graph) on a fresh set, then `on_set(ctx, tm, set, frame_off)`; scores copied back when asked
template <class OnSet>
std::vector<LatticeResult> K1ThenDecode(const AmDiagGmm& am, const TransitionModel& tm, const GraphsCsr& g, const std::vector<const float*>& feats,
                                        const std::vector<int64_t>& nframes, bool return_scores, const std::string& name, OnSet on_set) {
  const int n_utt = (int)feats.size(), D = am.Dim();
  KHG_REQUIRE((int)nframes.size() == n_utt && GraphsFit(g, n_utt), name + ": one graph and one feature matrix per utterance");
  khg_ctx* ctx = DefaultCtx();
  khg_model* dm = am.DeviceModel(ctx);
  khg_tm* dt = tm.DeviceTm(ctx);
  UttsH us;
  CApi(khg_tm_set_trans_cost(dt, nullptr));       // the graph's own weights (HCLG carries its transition probabilities)
  std::vector<int64_t> frame_off((size_t)n_utt + 1, 0);
  for (int u = 0; u < n_utt; ++u) frame_off[(size_t)u + 1] = frame_off[(size_t)u] + nframes[(size_t)u];
  std::vector<float> all((size_t)std::max<int64_t>(frame_off[(size_t)n_utt], 1) * D);
  for (int u = 0; u < n_utt; ++u)
    if (nframes[(size_t)u] > 0) std::memcpy(all.data() + (size_t)frame_off[(size_t)u] * D, feats[(size_t)u], sizeof(float) * (size_t)nframes[(size_t)u] * D);
  CreateBatchSet(ctx, dt, g, n_utt, D, frame_off.data(), all.data(), &us.h);
  CApi(khg_loglikes(ctx, dm, us.h));              // every cell: a partial path may read any (frame, pdf) of the graph
  std::vector<LatticeResult> out = on_set(ctx, dt, us.h, frame_off);
  if (return_scores) {
    std::vector<int64_t> ll_off((size_t)n_utt + 1, 0), pdf_off((size_t)n_utt + 1, 0);
    int64_t total = 0;
    CApi(khg_loglikes_layout(us.h, ll_off.data(), &total));
    std::vector<float> scores((size_t)std::max<int64_t>(total, 1));
    CApi(khg_loglikes_download(ctx, us.h, scores.data()));
    CApi(khg_utts_num_pdfs(us.h, pdf_off.data()));
    std::vector<int32_t> pdfs((size_t)std::max<int64_t>(pdf_off[(size_t)n_utt], 1));
    CApi(khg_utts_pdfs(us.h, pdfs.data()));
    for (int u = 0; u < n_utt; ++u) {
      LatticeResult& r = out[(size_t)u];
      const int64_t T = nframes[(size_t)u], tpad = (T + 31) & ~int64_t(31);
      const int npdf = (int)(pdf_off[(size_t)u + 1] - pdf_off[(size_t)u]);
      r.pdfs.assign(pdfs.begin() + pdf_off[(size_t)u], pdfs.begin() + pdf_off[(size_t)u + 1]);
      r.loglikes.resize((size_t)npdf * (size_t)T);
      for (int j = 0; j < npdf; ++j)
        if (T > 0) std::memcpy(r.loglikes.data() + (size_t)j * T, scores.data() + ll_off[(size_t)u] + (size_t)j * tpad, sizeof(float) * (size_t)T);
    }
  }
  return out;
}
}  // namespace

std::vector<LatticeResult> DecodeLatticeBatch(const AmDiagGmm& am, const TransitionModel& tm, const GraphsCsr& g, const std::vector<const float*>& feats,
                                              const std::vector<int64_t>& nframes, const LatticeFasterDecoderConfig& config, float acoustic_scale,
                                              bool allow_partial, bool return_scores, int scratch_per_frame) {
  config.Check();
  for (int64_t T : nframes) KHG_REQUIRE(T > 0, "num_frames > 0 assertion failed");     // GetRawLattice (lattice-faster-decoder.cc:137)
  return K1ThenDecode(am, tm, g, feats, nframes, return_scores, "decode_lattice_faster_batch",
                      [&](khg_ctx* ctx, khg_tm* dt, khg_utts* us, const std::vector<int64_t>& frame_off) {
                        return DecodeLatticeOnSet(ctx, dt, us, frame_off, config, acoustic_scale, allow_partial, scratch_per_frame,
                                                  BatchStates(g, (int)feats.size()));
                      });
}

std::vector<LatticeResult> DecodeLatticeSimpleOnSet(khg_ctx* ctx, khg_tm* tm, khg_utts* us, const std::vector<int64_t>& frame_off,
                                                    const LatticeSimpleDecoderConfig& config, float acoustic_scale, bool allow_partial,
                                                    int scratch_per_frame, int64_t total_states, khg_lattices** lattices) {
  const int n_utt = (int)frame_off.size() - 1;
  khg_lattice_simple_config c;
  khg_lattice_simple_config_default(&c);
  c.beam = config.beam; c.lattice_beam = config.lattice_beam; c.prune_interval = config.prune_interval; c.prune_scale = config.prune_scale;
  c.acoustic_scale = acoustic_scale; c.allow_partial = allow_partial ? 1 : 0; c.scratch_per_frame = scratch_per_frame;
  const int64_t N = frame_off[(size_t)n_utt];
  std::vector<int64_t> woff((size_t)n_utt + 1, 0);
  std::vector<int32_t> ali((size_t)std::max<int64_t>(N, 1)), status((size_t)n_utt), ef((size_t)n_utt);
  std::vector<double> like((size_t)n_utt);
  // words: the C-ABI keeps at most frames + states + 64 per utterance
  std::vector<int32_t> words((size_t)(N + total_states + 64 * (int64_t)n_utt + 16));
  if (lattices)
    CApi(khg_decode_lattice_simple_raw(ctx, tm, us, &c, ali.data(), words.data(), woff.data(), (int64_t)words.size(), like.data(), status.data(),
                                       ef.data(), lattices));
  else
    CApi(khg_decode_lattice_simple(ctx, tm, us, &c, ali.data(), words.data(), woff.data(), (int64_t)words.size(), like.data(), status.data(), ef.data()));
  std::vector<LatticeResult> out((size_t)n_utt);
  for (int u = 0; u < n_utt; ++u) {
    LatticeResult& r = out[(size_t)u];
    r.status = status[(size_t)u];
    r.err_frame = ef[(size_t)u];
    r.succeeded = (r.status & KHG_LAT_SUCCEEDED) != 0;
    r.num_frames = (int)(frame_off[(size_t)u + 1] - frame_off[(size_t)u]);
    if (r.succeeded) {
      r.alignment.assign(ali.begin() + frame_off[(size_t)u], ali.begin() + frame_off[(size_t)u + 1]);
      r.words.assign(words.begin() + woff[(size_t)u], words.begin() + woff[(size_t)u + 1]);
      r.like = like[(size_t)u];
    }
  }
  return out;
}

std::vector<LatticeResult> DecodeLatticeSimpleBatch(const AmDiagGmm& am, const TransitionModel& tm, const GraphsCsr& g,
                                                    const std::vector<const float*>& feats, const std::vector<int64_t>& nframes,
                                                    const LatticeSimpleDecoderConfig& config, float acoustic_scale, bool allow_partial,
                                                    bool return_scores, int scratch_per_frame) {
  config.Check();
  for (int64_t T : nframes) KHG_REQUIRE(T > 0, "decode_lattice_simple_batch: an utterance without frames");
  return K1ThenDecode(am, tm, g, feats, nframes, return_scores, "decode_lattice_simple_batch",
                      [&](khg_ctx* ctx, khg_tm* dt, khg_utts* us, const std::vector<int64_t>& frame_off) {
                        return DecodeLatticeSimpleOnSet(ctx, dt, us, frame_off, config, acoustic_scale, allow_partial, scratch_per_frame,
                                                        BatchStates(g, (int)feats.size()));
                      });
}

std::vector<LatticeResult> GetRawLatticeSimpleBatch(const AmDiagGmm& am, const TransitionModel& tm, const GraphsCsr& g,
                                                    const std::vector<const float*>& feats, const std::vector<int64_t>& nframes,
                                                    const LatticeSimpleDecoderConfig& config, float acoustic_scale, bool return_scores,
                                                    int scratch_per_frame, std::vector<std::shared_ptr<Lattice>>* lattices, double* seconds) {
  config.Check();
  KHG_REQUIRE(lattices != nullptr, "get_raw_lattice_simple_batch: no place for the lattices");
  for (int64_t T : nframes) KHG_REQUIRE(T > 0, "get_raw_lattice_simple_batch: an utterance without frames");
  const int n_utt = (int)feats.size();
  lattices->assign((size_t)n_utt, nullptr);
  struct LatH { khg_lattices* h = nullptr; ~LatH() { if (h) khg_lattices_destroy(h); } } lh;
  using Clock = std::chrono::steady_clock;
  return K1ThenDecode(am, tm, g, feats, nframes, return_scores, "get_raw_lattice_simple_batch",
                      [&](khg_ctx* ctx, khg_tm* dt, khg_utts* us, const std::vector<int64_t>& frame_off) {
                        const Clock::time_point t0 = Clock::now();
                        std::vector<LatticeResult> out = DecodeLatticeSimpleOnSet(ctx, dt, us, frame_off, config, acoustic_scale, true, scratch_per_frame,
                                                                                  BatchStates(g, n_utt), &lh.h);
                        const Clock::time_point t1 = Clock::now();
                        std::vector<int64_t> so((size_t)n_utt + 1, 0), ao((size_t)n_utt + 1, 0);
                        CApi(khg_lattices_sizes(lh.h, so.data(), ao.data()));
                        const size_t NS = (size_t)so[(size_t)n_utt], NA = (size_t)ao[(size_t)n_utt];
                        std::vector<int32_t> frame(NS + 1), gstate(NS + 1), abeg(NS + 1), il(NA + 1), ol(NA + 1), ns(NA + 1), start((size_t)n_utt + 1);
                        std::vector<float> tot(NS + 1), extra(NS + 1), fin(NS + 1), gc(NA + 1), ac(NA + 1);
                        CApi(khg_lattices_download(ctx, lh.h, frame.data(), gstate.data(), tot.data(), extra.data(), fin.data(), abeg.data(), il.data(),
                                                   ol.data(), gc.data(), ac.data(), ns.data(), start.data()));
                        if (seconds) {
                          seconds[0] = std::chrono::duration<double>(t1 - t0).count();
                          seconds[1] = std::chrono::duration<double>(Clock::now() - t1).count();
                        }
                        for (int u = 0; u < n_utt; ++u) {
                          auto l = std::make_shared<Lattice>();
                          const size_t s0 = (size_t)so[(size_t)u], s1 = (size_t)so[(size_t)u + 1], a0 = (size_t)ao[(size_t)u], a1 = (size_t)ao[(size_t)u + 1];
                          l->frame.assign(frame.begin() + s0, frame.begin() + s1); l->graph_state.assign(gstate.begin() + s0, gstate.begin() + s1);
                          l->tot_cost.assign(tot.begin() + s0, tot.begin() + s1); l->extra_cost.assign(extra.begin() + s0, extra.begin() + s1);
                          l->final_cost.assign(fin.begin() + s0, fin.begin() + s1);
                          l->arc_begin.assign(abeg.begin() + s0, abeg.begin() + s1);
                          l->arc_begin.push_back((int32_t)(a1 - a0));
                          l->ilabel.assign(il.begin() + a0, il.begin() + a1); l->olabel.assign(ol.begin() + a0, ol.begin() + a1);
                          l->nextstate.assign(ns.begin() + a0, ns.begin() + a1);
                          l->graph_cost.assign(gc.begin() + a0, gc.begin() + a1); l->acoustic_cost.assign(ac.begin() + a0, ac.begin() + a1);
                          l->start = s1 > s0 ? start[(size_t)u] : kNoStateId;
                          (*lattices)[(size_t)u] = std::move(l);
                        }
                        return out;
                      });
}

std::vector<std::shared_ptr<Lattice>> DownloadLattices(khg_ctx* ctx, const khg_lattices* h) {
  int32_t n_utt = 0;
  CApi(khg_lattices_num_utts(h, &n_utt));
  std::vector<int64_t> so((size_t)n_utt + 1, 0), ao((size_t)n_utt + 1, 0);
  CApi(khg_lattices_sizes(h, so.data(), ao.data()));
  const size_t NS = (size_t)so[(size_t)n_utt], NA = (size_t)ao[(size_t)n_utt];
  std::vector<int32_t> frame(NS + 1), gstate(NS + 1), abeg(NS + 1), il(NA + 1), ol(NA + 1), ns(NA + 1), start((size_t)n_utt + 1);
  std::vector<float> tot(NS + 1), extra(NS + 1), fin(NS + 1), gc(NA + 1), ac(NA + 1);
  CApi(khg_lattices_download(ctx, h, frame.data(), gstate.data(), tot.data(), extra.data(), fin.data(), abeg.data(), il.data(), ol.data(), gc.data(),
                             ac.data(), ns.data(), start.data()));
  std::vector<std::shared_ptr<Lattice>> out((size_t)n_utt);
  for (int u = 0; u < n_utt; ++u) {
    auto l = std::make_shared<Lattice>();
    const size_t s0 = (size_t)so[(size_t)u], s1 = (size_t)so[(size_t)u + 1], a0 = (size_t)ao[(size_t)u], a1 = (size_t)ao[(size_t)u + 1];
    l->frame.assign(frame.begin() + s0, frame.begin() + s1); l->graph_state.assign(gstate.begin() + s0, gstate.begin() + s1);
    l->tot_cost.assign(tot.begin() + s0, tot.begin() + s1); l->extra_cost.assign(extra.begin() + s0, extra.begin() + s1);
    l->final_cost.assign(fin.begin() + s0, fin.begin() + s1);
    l->arc_begin.assign(abeg.begin() + s0, abeg.begin() + s1);
    l->arc_begin.push_back((int32_t)(a1 - a0));
    l->ilabel.assign(il.begin() + a0, il.begin() + a1); l->olabel.assign(ol.begin() + a0, ol.begin() + a1);
    l->nextstate.assign(ns.begin() + a0, ns.begin() + a1);
    l->graph_cost.assign(gc.begin() + a0, gc.begin() + a1); l->acoustic_cost.assign(ac.begin() + a0, ac.begin() + a1);
    l->start = s1 > s0 ? start[(size_t)u] : kNoStateId;
    out[(size_t)u] = std::move(l);
  }
  return out;
}

std::vector<LatticeResult> GetRawLatticeSimpleDeviceBatch(const AmDiagGmm& am, const TransitionModel& tm, const GraphsCsr& g,
                                                          const std::vector<const float*>& feats, const std::vector<int64_t>& nframes,
                                                          const LatticeSimpleDecoderConfig& config, float acoustic_scale, bool return_scores,
                                                          int scratch_per_frame, khg_lattices** lattices) {
  config.Check();
  KHG_REQUIRE(lattices != nullptr, "get_raw_lattice_simple_device_batch: no place for the lattices");
  *lattices = nullptr;
  for (int64_t T : nframes) KHG_REQUIRE(T > 0, "get_raw_lattice_simple_device_batch: an utterance without frames");
  const int n_utt = (int)feats.size();
  return K1ThenDecode(am, tm, g, feats, nframes, return_scores, "get_raw_lattice_simple_device_batch",
                      [&](khg_ctx* ctx, khg_tm* dt, khg_utts* us, const std::vector<int64_t>& frame_off) {
                        return DecodeLatticeSimpleOnSet(ctx, dt, us, frame_off, config, acoustic_scale, true, scratch_per_frame,
                                                        BatchStates(g, n_utt), lattices);
                      });
}

std::vector<LatticeResult> GetRawLatticeFasterBatch(const AmDiagGmm& am, const TransitionModel& tm, const GraphsCsr& g,
                                                    const std::vector<const float*>& feats, const std::vector<int64_t>& nframes,
                                                    const LatticeFasterDecoderConfig& config, float acoustic_scale, bool allow_partial,
                                                    bool return_scores, int scratch_per_frame, std::vector<std::shared_ptr<Lattice>>* lattices,
                                                    double* seconds) {
  config.Check();
  KHG_REQUIRE(lattices != nullptr, "get_raw_lattice_faster_batch: no place for the lattices");
  for (int64_t T : nframes) KHG_REQUIRE(T > 0, "num_frames > 0 assertion failed");     // GetRawLattice (lattice-faster-decoder.cc:137)
  const int n_utt = (int)feats.size();
  lattices->assign((size_t)n_utt, nullptr);
  struct LatH { khg_lattices* h = nullptr; ~LatH() { if (h) khg_lattices_destroy(h); } } lh;
  using Clock = std::chrono::steady_clock;
  return K1ThenDecode(am, tm, g, feats, nframes, return_scores, "get_raw_lattice_faster_batch",
                      [&](khg_ctx* ctx, khg_tm* dt, khg_utts* us, const std::vector<int64_t>& frame_off) {
                        const Clock::time_point t0 = Clock::now();
                        std::vector<LatticeResult> out = DecodeLatticeOnSet(ctx, dt, us, frame_off, config, acoustic_scale, allow_partial,
                                                                            scratch_per_frame, BatchStates(g, n_utt), &lh.h);
                        const Clock::time_point t1 = Clock::now();
                        *lattices = DownloadLattices(ctx, lh.h);
                        if (seconds) {
                          seconds[0] = std::chrono::duration<double>(t1 - t0).count();
                          seconds[1] = std::chrono::duration<double>(Clock::now() - t1).count();
                        }
                        return out;
                      });
}

std::vector<LatticeResult> GetRawLatticeFasterDeviceBatch(const AmDiagGmm& am, const TransitionModel& tm, const GraphsCsr& g,
                                                          const std::vector<const float*>& feats, const std::vector<int64_t>& nframes,
                                                          const LatticeFasterDecoderConfig& config, float acoustic_scale, bool allow_partial,
                                                          bool return_scores, int scratch_per_frame, khg_lattices** lattices) {
  config.Check();
  KHG_REQUIRE(lattices != nullptr, "get_raw_lattice_faster_device_batch: no place for the lattices");
  *lattices = nullptr;
  for (int64_t T : nframes) KHG_REQUIRE(T > 0, "num_frames > 0 assertion failed");
  const int n_utt = (int)feats.size();
  return K1ThenDecode(am, tm, g, feats, nframes, return_scores, "get_raw_lattice_faster_device_batch",
                      [&](khg_ctx* ctx, khg_tm* dt, khg_utts* us, const std::vector<int64_t>& frame_off) {
                        return DecodeLatticeOnSet(ctx, dt, us, frame_off, config, acoustic_scale, allow_partial, scratch_per_frame,
                                                  BatchStates(g, n_utt), lattices);
                      });
}

// scripts/gmm_acc_stats_ali.py:46-58 through K3, into the accumulators' device block (khg_host_gmm.hpp)
double AccumAmDiagGmm::AccumulateAli(const AmDiagGmm& model, const TransitionModel& tm, const float* feats, const int64_t* frame_off, int n_utt,
                                     const int32_t* ali, float weight) {
  KHG_REQUIRE(n_utt >= 1 && frame_off && frame_off[0] == 0, "AccumulateAli: bad arguments");
  const int64_t N = frame_off[n_utt];
  if (N == 0) return 0.0;
  KHG_REQUIRE(NumAccs() == model.NumPdfs(), "gmm_accs.NumAccs() == am_gmm.NumPdfs() assertion failed");
  const int nt = tm.NumTransitionIds();
  for (int64_t t = 0; t < N; ++t) KHG_REQUIRE(ali[t] >= 1 && ali[t] <= nt, "gmm_acc_stats_ali: transition-id out of range");
  return AccumulateOnDevice(model, tm.DeviceTm(DefaultCtx()), nt, feats, frame_off, n_utt, ali, weight);
}

// gmm-acc-stats through khg_acc_stats_post, into the same block
double AccumAmDiagGmm::AccumulatePost(const AmDiagGmm& model, const TransitionModel& tm, const float* feats, const int64_t* frame_off, int n_utt,
                                      const int64_t* entry_begin, const int32_t* tid, const double* post_weight, float scale) {
  KHG_REQUIRE(n_utt >= 1 && frame_off && frame_off[0] == 0 && entry_begin, "AccumulatePost: bad arguments");
  if (frame_off[n_utt] == 0 || entry_begin[frame_off[n_utt]] == 0) return 0.0;
  KHG_REQUIRE(NumAccs() == model.NumPdfs(), "gmm_accs.NumAccs() == am_gmm.NumPdfs() assertion failed");
  const int nt = tm.NumTransitionIds();
  return AccumulateOnDevice(model, tm.DeviceTm(DefaultCtx()), nt, feats, frame_off, n_utt, nullptr, scale, entry_begin, tid, post_weight);
}

// One K3 call into the device-resident block (made for this model version and this many transition-ids); -> the call's own
// sum of weight * log-like.  `dt` == nullptr: the per-frame entry points' table, transition-id = pdf + 1, owned by the block.
double AccumAmDiagGmm::AccumulateOnDevice(const AmDiagGmm& model, khg_tm* dt, int nt, const float* feats, const int64_t* frame_off, int n_utt,
                                          const int32_t* ali, float weight, const int64_t* entry_begin, const int32_t* tid, const double* post_weight) {
  const int D = model.Dim();
  khg_ctx* ctx = DefaultCtx();
  khg_model* dm = model.DeviceModel(ctx);
  const uint64_t mv = model.Version();
  if (dev_ && (dev_->ctx != ctx || dev_->model_version != mv || dev_->num_tids != nt)) {
    // another model (or the same one after an update that may have moved its layout): what is pending belongs to the old layout
    Flush();
    dev_.reset();
  }
  if (!dev_) {
    auto d = std::make_shared<Dev>();
    d->ctx = ctx; d->model_version = mv; d->num_tids = nt; d->D = D;
    d->gauss_off.assign((size_t)model.NumPdfs() + 1, 0);
    for (int p = 0; p < model.NumPdfs(); ++p) {
      const int G = model.GetPdf(p)->NumGauss();
      KHG_REQUIRE(accs_[(size_t)p]->NumGauss() == G && accs_[(size_t)p]->Dim() == D, "gmm_accs was not initialised for this model (AccumAmDiagGmm.init)");
      d->gauss_off[(size_t)p + 1] = d->gauss_off[(size_t)p] + G;
    }
    if (!dt) {
      std::vector<int32_t> id2pdf((size_t)nt + 1, 0);
      for (int p = 0; p < nt; ++p) id2pdf[(size_t)p + 1] = p;
      CApi(khg_tm_create(ctx, nt, id2pdf.data(), &d->pdf_tm));
    }
    CApi(khg_accs_create(ctx, dm, dt ? dt : d->pdf_tm, &d->h));
    dev_ = d;
  }
  if (!dt) dt = dev_->pdf_tm;
  KHG_REQUIRE(dt != nullptr, "AccumAmDiagGmm: the device block was made for a transition model, not for per-frame calls");
  UttsH us;
  CApi(khg_utts_create(ctx, nullptr, n_utt, D, frame_off, feats, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &us.h));
  if (ali) {
    CApi(khg_ali_upload(ctx, us.h, ali));
    CApi(khg_acc_stats(ctx, dm, dt, us.h, weight, dev_->h));
  } else {
    struct PostH { khg_posteriors* h = nullptr; ~PostH() { if (h) khg_posteriors_destroy(h); } } post;
    CApi(khg_posteriors_upload(ctx, n_utt, frame_off, entry_begin, tid, post_weight, &post.h));
    CApi(khg_acc_stats_post(ctx, dm, dt, us.h, post.h, weight, dev_->h));
    CApi(khg_ctx_sync(ctx));          // the handle goes with this scope: its kernels first
  }
  dev_->pending = true;
  double sc[8];
  CApi(khg_accs_download_trans(ctx, dev_->h, nullptr, sc));      // the 8 scalars: [frames, log-like, ...] running totals of the block
  const double ll = sc[1] - dev_->seen_ll;
  dev_->seen_frames = sc[0]; dev_->seen_ll = sc[1];
  return ll;
}

// csrc/mle-am-diag-gmm.cc:41-52 (AccumulateForGmm): one frame for one pdf -- the loop body of the reference's own
// scripts/gmm_acc_stats_ali.py:46-56.  The same device-resident block as AccumulateAli (a set of one frame, transition-id = pdf + 1):
// no model upload, no statistics download per frame; the return value is the frame's log-likelihood.
float AccumAmDiagGmm::AccumulateForGmm(const AmDiagGmm& model, const float* data, size_t n, int i, float weight) {
  Chk(i);
  KHG_REQUIRE(NumAccs() == model.NumPdfs(), "gmm_accs.NumAccs() == am_gmm.NumPdfs() assertion failed");
  KHG_REQUIRE((int)n == model.Dim(), "data.size() == Dim() assertion failed");
  if (weight == 0.0f) return model.GetPdf(i)->LogLikelihood(data, n);      // nothing to add; the reference still returns the likelihood
  const int64_t fo[2] = {0, 1};
  const int32_t tid = i + 1;
  const int nt = model.NumPdfs();
  if (dev_ && !dev_->pdf_tm && dev_->num_tids == nt) { Flush(); dev_.reset(); }   // a block AccumulateAli made for a transition model with exactly as many ids has no pdf table
  const double wll = AccumulateOnDevice(model, nullptr, nt, data, fo, 1, &tid, weight);
  return (float)(wll / (double)weight);
}

}  // namespace khg
