// pybind11 bindings of the alignment API (khg_host_align.hpp, khg_host_fst.hpp) with the names of python/csrc/{decoder-wrappers,
// faster-decoder,decodable-am-diag-gmm,decodable-itf,hmm-utils}.cc in /root/reference/kaldi-hmm-gmm, and of the graph container with
// the kaldifst method names the reference's scripts use (StdVectorFst, StdArc).
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include "khg_host_fst.hpp"
#include "khg_py_lattices.hpp"

namespace py = pybind11;
using namespace khg;

namespace {
template <class T>
using Arr = py::array_t<T, py::array::c_style | py::array::forcecast>;

template <class T>
Arr<T> Vec1(const std::vector<T>& v) {
  Arr<T> a({(py::ssize_t)v.size()});
  if (!v.empty()) std::memcpy(a.mutable_data(), v.data(), sizeof(T) * v.size());
  return a;
}
py::dict CsrToDict(const GraphsCsr& c) {
  py::dict d;
  d["state_off"] = Vec1(c.state_off); d["arc_off"] = Vec1(c.arc_off); d["start"] = Vec1(c.start);
  d["ilabel"] = Vec1(c.ilabel); d["olabel"] = Vec1(c.olabel); d["nextstate"] = Vec1(c.nextstate);
  d["weight"] = Vec1(c.weight); d["final"] = Vec1(c.final_w);
  return d;
}

// DecodingGraph(fst, tm, ctx=None): one decoding graph resident in HBM (khg_graph_create) that any number of utterance sets and
// batch calls decode on.  tm: a TransitionModel (its cached device table on `ctx`, default: the default context) or a
// DeviceTransitions (then the graph lives on that table's context).
struct PyDecodingGraph {
  khg_graph* h = nullptr;
  py::object keep_ctx, keep_tm;
  int64_t num_states = 0, num_arcs = 0, device_bytes = 0;
  int32_t num_pdfs = 0, max_in_degree = 0;
  PyDecodingGraph(std::shared_ptr<StdVectorFst> fst, py::object tm, py::object ctx) : keep_ctx(ctx), keep_tm(tm) {
    if (!fst) throw Error("DecodingGraph: fst is None");
    if (fst->Start() == kNoStateId) throw Error("start_state != fst::kNoStateId assertion failed");
    khg_ctx* c = nullptr;
    khg_tm* t = nullptr;
    if (py::isinstance<TransitionModel>(tm)) {
      c = ctx.is_none() ? DefaultCtx() : reinterpret_cast<khg_ctx*>(ctx.attr("h").cast<uintptr_t>());
      t = tm.cast<std::shared_ptr<TransitionModel>>()->DeviceTm(c);
    } else {
      if (ctx.is_none()) keep_ctx = tm.attr("ctx");
      c = reinterpret_cast<khg_ctx*>(keep_ctx.attr("h").cast<uintptr_t>());
      t = reinterpret_cast<khg_tm*>(tm.attr("h").cast<uintptr_t>());
    }
    const GraphsCsr g = ConcatGraphs({fst.get()});
    {
      py::gil_scoped_release nogil;
      CApi(khg_graph_create(c, t, (int32_t)g.state_off.back(), g.start[0], g.arc_off.data(), g.ilabel.data(), g.olabel.data(), g.weight.data(),
                            g.nextstate.data(), g.final_w.data(), &h));
    }
    CApi(khg_graph_info(h, &num_states, &num_arcs, &num_pdfs, &max_in_degree, &device_bytes));
  }
  PyDecodingGraph(const PyDecodingGraph&) = delete;
  ~PyDecodingGraph() { close(); }
  void close() { if (h) { khg_graph_destroy(h); h = nullptr; } }
};

// python/csrc/decodable-itf.cc:14-53: a decodable written in Python overrides these four
class PyDecodableInterface : public DecodableInterface {
 public:
  using DecodableInterface::DecodableInterface;
  float LogLikelihood(int frame, int index) const override { PYBIND11_OVERRIDE_PURE_NAME(float, DecodableInterface, "log_likelihood", LogLikelihood, frame, index); }
  bool IsLastFrame(int frame) const override { PYBIND11_OVERRIDE_PURE_NAME(bool, DecodableInterface, "is_last_frame", IsLastFrame, frame); }
  int NumFramesReady() const override { PYBIND11_OVERRIDE_NAME(int, DecodableInterface, "num_frames_ready", NumFramesReady); }
  int NumIndices() const override { PYBIND11_OVERRIDE_PURE_NAME(int, DecodableInterface, "num_indices", NumIndices); }
};

AlignConfig ConfigFrom(py::object o) {
  if (py::isinstance<AlignConfig>(o)) return o.cast<AlignConfig>();
  AlignConfig c;
  c.beam = o.attr("beam").cast<float>(); c.retry_beam = o.attr("retry_beam").cast<float>(); c.careful = o.attr("careful").cast<bool>();
  return c;
}
void CheckBeams(const AlignConfig& cfg) {      // csrc/decoder-wrappers.cc:29-33
  if ((cfg.retry_beam != 0 && cfg.retry_beam <= cfg.beam) || cfg.beam <= 0.0f) {
    char b[128];
    std::snprintf(b, sizeof(b), "Beams do not make sense: beam %g, retry-beam %g", (double)cfg.beam, (double)cfg.retry_beam);
    throw Error(b);
  }
}

py::list ResultsToList(const std::vector<AlignResult>& rs, const std::vector<int64_t>& nframes, bool return_scores) {
  py::list out;
  for (size_t u = 0; u < rs.size(); ++u) {
    const AlignResult& r = rs[u];
    py::dict d;
    d["ok"] = r.ok; d["retried"] = r.retried; d["status"] = r.status;
    d["alignment"] = py::cast(r.alignment); d["words"] = py::cast(r.words);
    d["like"] = r.ok ? (double)r.like : 0.0;
    d["num_frames"] = r.num_frames;
    if (return_scores) {
      Arr<float> m({(py::ssize_t)r.pdfs.size(), (py::ssize_t)nframes[u]});
      if (!r.loglikes.empty()) std::memcpy(m.mutable_data(), r.loglikes.data(), sizeof(float) * r.loglikes.size());
      d["loglikes"] = m;
      d["pdfs"] = Vec1(r.pdfs);
    }
    out.append(d);
  }
  return out;
}

// align_batch(am, tm, fsts, feats_list, config, acoustic_scale, trans_cost=None, decoder_opts=None, return_scores=False)
// fsts: one graph per utterance; or ONE for all of them -- a StdVectorFst, a list of one, or a DecodingGraph -- which the batch then
// shares (GraphsCsr::shared: planned and uploaded once)
py::list AlignBatchPy(std::shared_ptr<AmDiagGmm> am, std::shared_ptr<TransitionModel> tm, py::object fsts_o, py::list feats_list,
                      py::object config, float acoustic_scale, py::object trans_cost, py::object decoder_opts, bool return_scores) {
  const AlignConfig cfg = ConfigFrom(config);
  CheckBeams(cfg);
  GraphsCsr csr;
  if (py::isinstance<PyDecodingGraph>(fsts_o)) {
    if (cfg.careful) throw Error("align_batch: careful alignment modifies the graph; pass the StdVectorFst, not a DecodingGraph");
    PyDecodingGraph& dg = fsts_o.cast<PyDecodingGraph&>();
    if (!dg.h) throw Error("align_batch: the DecodingGraph is closed");
    csr.shared = true; csr.device = dg.h;
  } else {
    std::vector<std::shared_ptr<StdVectorFst>> fsts;
    if (py::isinstance<StdVectorFst>(fsts_o)) fsts.push_back(fsts_o.cast<std::shared_ptr<StdVectorFst>>());
    else fsts = fsts_o.cast<std::vector<std::shared_ptr<StdVectorFst>>>();
    const bool shared = (py::isinstance<StdVectorFst>(fsts_o) || (fsts.size() == 1 && py::len(feats_list) >= 1)) && fsts[0] &&
                        fsts[0]->Start() != kNoStateId;       // (an empty graph: the per-utterance path reports it per utterance)
    std::vector<StdVectorFst> careful;           // on copies: the batch entry point leaves the caller's graphs alone
    std::vector<const StdVectorFst*> gp;
    if (cfg.careful) {
      careful.reserve(fsts.size());
      for (auto& f : fsts) {
        careful.push_back(*f);
        if (careful.back().Start() != kNoStateId) ModifyGraphForCarefulAlignment(&careful.back());
      }
      for (auto& f : careful) gp.push_back(&f);
    } else {
      for (auto& f : fsts) gp.push_back(f.get());
    }
    if (!shared && py::isinstance<StdVectorFst>(fsts_o)) for (size_t i = 1; i < py::len(feats_list); ++i) gp.push_back(gp[0]);
    csr = ConcatGraphs(gp);
    csr.shared = shared;
  }
  const int D = am->Dim();
  std::vector<Arr<float>> keep;
  std::vector<const float*> fp;
  std::vector<int64_t> nf;
  for (py::handle f : feats_list) {
    Arr<float> a = f.cast<Arr<float>>();
    if (D <= 0 || a.size() % D != 0) throw Error("Dim mismatch: data dim vs. model dim = " + std::to_string(D));
    keep.push_back(a);
    fp.push_back(a.data());
    nf.push_back((int64_t)(a.size() / D));
  }
  Arr<float> tc;
  const float* tcp = nullptr;
  if (!trans_cost.is_none()) {
    tc = trans_cost.cast<Arr<float>>();
    if (tc.size() != tm->NumTransitionIds() + 1) throw Error("trans_cost: one cost per transition-id (+ entry 0)");
    tcp = tc.data();
  }
  FasterDecoderOptions dopts;
  const bool has_opts = !decoder_opts.is_none();
  if (has_opts) dopts = decoder_opts.cast<FasterDecoderOptions>();
  std::vector<AlignResult> rs;
  {
    py::gil_scoped_release nogil;
    rs = AlignBatch(*am, *tm, csr, fp, nf, cfg, acoustic_scale, tcp, has_opts ? &dopts : nullptr, return_scores);
  }
  return ResultsToList(rs, nf, return_scores);
}
py::dict LatticeToDict(const LatticeResult& r, int64_t T, bool return_scores) {
  py::dict d;
  d["succeeded"] = r.succeeded; d["partial"] = r.partial; d["status"] = r.status;
  d["alignment"] = py::cast(r.alignment); d["words"] = py::cast(r.words); d["like"] = r.like; d["num_frames"] = r.num_frames;
  if (return_scores) {
    Arr<float> m({(py::ssize_t)r.pdfs.size(), (py::ssize_t)T});
    if (!r.loglikes.empty()) std::memcpy(m.mutable_data(), r.loglikes.data(), sizeof(float) * r.loglikes.size());
    d["loglikes"] = m;
    d["pdfs"] = Vec1(r.pdfs);
  }
  return d;
}
// the batched lattice calls' (fsts, feats_list): one graph for all utterances or one each; feature matrices of the model's dimension
struct BatchArgs {
  std::vector<Arr<float>> keep;
  std::vector<const float*> fp;
  std::vector<int64_t> nf;
  std::vector<const StdVectorFst*> gp;
  std::vector<std::shared_ptr<StdVectorFst>> hold;
  bool shared = false;
  khg_graph* device = nullptr;
  BatchArgs(const AmDiagGmm& am, py::object fsts, py::list feats_list, const std::string& name) {
    const int D = am.Dim();
    for (py::handle f : feats_list) {
      Arr<float> a = f.cast<Arr<float>>();
      if (D <= 0 || a.size() % D != 0) throw Error("Dim mismatch: data dim vs. model dim = " + std::to_string(D));
      keep.push_back(a);
      fp.push_back(a.data());
      nf.push_back((int64_t)(a.size() / D));
    }
    if (py::isinstance<PyDecodingGraph>(fsts)) {
      PyDecodingGraph& dg = fsts.cast<PyDecodingGraph&>();
      if (!dg.h) throw Error(name + ": the DecodingGraph is closed");
      shared = true; device = dg.h;
      return;
    }
    if (py::isinstance<StdVectorFst>(fsts)) {
      hold.push_back(fsts.cast<std::shared_ptr<StdVectorFst>>());
      shared = true;
    } else {
      hold = fsts.cast<std::vector<std::shared_ptr<StdVectorFst>>>();
      shared = hold.size() == 1;
    }
    for (auto& f : hold) gp.push_back(f.get());
    if (!shared && gp.size() != fp.size()) throw Error(name + ": one graph, or one graph per utterance");
    for (auto* g : gp) if (!g || g->Start() == kNoStateId) throw Error("start_state != fst::kNoStateId assertion failed");
  }
  // one graph for all utterances is shared, not repeated: planned and uploaded once (khg_utts_create_on_graph)
  GraphsCsr Csr() const {
    GraphsCsr c;
    if (!device) c = ConcatGraphs(gp);
    c.shared = shared; c.device = device;
    return c;
  }
};
// what the reference stops on in DecodeUtteranceLatticeSimple (KHG_ERR / KHG_ASSERT), raised with its message
void RaiseLatticeSimple(const LatticeResult& r, const std::string& utt) {
  if (r.status & KHG_LAT_NO_EPS_TOKEN) throw Error("Error in ProcessNonEmitting: no surviving tokens: frame is " + std::to_string(r.err_frame));
  if (r.status & KHG_LAT_NAN) throw Error("Check failed!\nx: link_extra_cost == link_extra_cost");
  if (r.status & KHG_LAT_EPS_LOOP)
    throw Error("decode_utterance_lattice_simple: a negative-cost epsilon cycle in the decoding graph for utterance " + utt +
                " (the reference's ProcessNonemitting never returns)");
  if (r.status & KHG_LAT_NO_TRACEBACK) {
    if (r.num_frames == 0) throw Error("Check failed!\nx: num_frames > 0");
    throw Error("Failed to get traceback for utterance " + utt);
  }
  if (r.status & KHG_LAT_SCRATCH) throw Error("decode_utterance_lattice_simple: more live tokens on a frame than scratch_per_frame for utterance " + utt);
  if (r.status & KHG_LAT_WORDS) throw Error("decode_utterance_lattice_simple: more words on the best path than the output holds for utterance " + utt);
}
py::dict LatticeSimpleToDict(const LatticeResult& r, int64_t T, bool return_scores) {
  py::dict d = LatticeToDict(r, T, return_scores);
  d["error_frame"] = r.err_frame;
  return d;
}
// a read-only numpy view of one of a Lattice's arrays; the Lattice stays alive as its base
template <class T>
py::array LatView(py::object self, const std::vector<T>& v, size_t n) {
  py::array_t<T> a({(py::ssize_t)n}, {(py::ssize_t)sizeof(T)}, v.data(), self);
  py::detail::array_proxy(a.ptr())->flags &= ~py::detail::npy_api::NPY_ARRAY_WRITEABLE_;
  return std::move(a);
}
template <class T>
std::vector<T> VecOf(py::object o) {
  Arr<T> a = o.cast<Arr<T>>();
  return std::vector<T>(a.data(), a.data() + a.size());
}
// a list of Lattice as the flat arrays of khg_lattices_upload; ctx == nullptr: the checks alone
khg_lattices* UploadLattices(khg_ctx* ctx, const std::vector<std::shared_ptr<Lattice>>& lats) {
  const int U = (int)lats.size();
  std::vector<int64_t> so((size_t)U + 1, 0), ao((size_t)U + 1, 0);
  std::vector<int32_t> frame, gstate, abeg, il, ol, ns, start;
  std::vector<float> tot, extra, fin, gc, ac;
  for (int u = 0; u < U; ++u) {
    if (!lats[(size_t)u]) throw Error("DeviceLattices.from_lattices: lattice " + std::to_string(u) + " is None");
    const Lattice& l = *lats[(size_t)u];
    so[(size_t)u + 1] = so[(size_t)u] + l.NumStates();
    ao[(size_t)u + 1] = ao[(size_t)u] + l.NumArcs();
    frame.insert(frame.end(), l.frame.begin(), l.frame.end()); gstate.insert(gstate.end(), l.graph_state.begin(), l.graph_state.end());
    tot.insert(tot.end(), l.tot_cost.begin(), l.tot_cost.end()); extra.insert(extra.end(), l.extra_cost.begin(), l.extra_cost.end());
    fin.insert(fin.end(), l.final_cost.begin(), l.final_cost.end());
    abeg.insert(abeg.end(), l.arc_begin.begin(), l.arc_begin.begin() + l.NumStates());
    il.insert(il.end(), l.ilabel.begin(), l.ilabel.end()); ol.insert(ol.end(), l.olabel.begin(), l.olabel.end());
    gc.insert(gc.end(), l.graph_cost.begin(), l.graph_cost.end()); ac.insert(ac.end(), l.acoustic_cost.begin(), l.acoustic_cost.end());
    ns.insert(ns.end(), l.nextstate.begin(), l.nextstate.end());
    start.push_back(l.NumStates() ? l.start : kNoStateId);
  }
  for (auto* v : {&frame, &gstate, &abeg, &il, &ol, &ns, &start}) v->push_back(0);      // (never a NULL array)
  for (auto* v : {&tot, &extra, &fin, &gc, &ac}) v->push_back(0.0f);
  khg_lattices* h = nullptr;
  if (!ctx) {
    CApi(khg_lattices_validate(U, so.data(), ao.data(), frame.data(), gstate.data(), tot.data(), extra.data(), fin.data(), abeg.data(), il.data(),
                               ol.data(), gc.data(), ac.data(), ns.data(), start.data()));
    return nullptr;
  }
  py::gil_scoped_release nogil;
  CApi(khg_lattices_upload(ctx, U, so.data(), ao.data(), frame.data(), gstate.data(), tot.data(), extra.data(), fin.data(), abeg.data(), il.data(),
                           ol.data(), gc.data(), ac.data(), ns.data(), start.data(), &h));
  return h;
}
std::pair<std::vector<int64_t>, std::vector<int64_t>> LatSizes(PyDeviceLattices& d) {
  if (!d.h) throw Error("DeviceLattices: closed");
  int32_t U = 0;
  CApi(khg_lattices_num_utts(d.h, &U));
  std::vector<int64_t> so((size_t)U + 1), ao((size_t)U + 1);
  CApi(khg_lattices_sizes(d.h, so.data(), ao.data()));
  return {so, ao};
}
// what Lattice.forward_backward and .forward_backward_mpe share: status, tot_like, arc_post, alpha, beta, post (per frame [(tid, weight), ...])
py::dict PosteriorsDict(const LatticePosteriors& r) {
  py::dict d;
  d["status"] = r.status; d["tot_like"] = r.tot_like; d["arc_post"] = Vec1(r.arc_post); d["alpha"] = Vec1(r.alpha); d["beta"] = Vec1(r.beta);
  py::list post;
  for (const auto& row : r.post) {
    py::list e;
    for (const auto& x : row) e.append(py::make_tuple(x.first, x.second));
    post.append(e);
  }
  d["post"] = post;
  return d;
}
// the reference of DeviceLattices.boost / .mpe_posteriors (`who` in the error text): None, or a list of U arrays of transition-ids ->
// (aoff [U + 1], ali); aoff stays empty for None
void FlattenAlignments(const std::string& who, py::object alignment, int U, std::vector<int64_t>* aoff, std::vector<int32_t>* ali) {
  if (alignment.is_none()) return;
  py::list al = alignment.cast<py::list>();
  if ((int)al.size() != U) throw Error(who + ": " + std::to_string(al.size()) + " alignments for " + std::to_string(U) + " lattices");
  aoff->assign(1, 0);
  for (py::handle h : al) {
    Arr<int32_t> a = py::reinterpret_borrow<py::object>(h).cast<Arr<int32_t>>();
    ali->insert(ali->end(), a.data(), a.data() + a.size());
    aoff->push_back((int64_t)ali->size());
  }
  ali->push_back(0);      // (never a NULL array)
}
// the references of DeviceLattices.oracle / .wer: a sequence of word sequences -> (off [n + 1], words)
void FlattenRefs(py::object refs, std::vector<int64_t>* off, std::vector<int32_t>* words) {
  off->assign(1, 0);
  for (py::handle h : refs) {
    Arr<int32_t> a = py::reinterpret_borrow<py::object>(h).cast<Arr<int32_t>>();
    words->insert(words->end(), a.data(), a.data() + a.size());
    off->push_back((int64_t)words->size());
  }
  words->push_back(0);      // (never a NULL array)
}
// an NgramLm (anything with to_arrays() -> {"backoff", "backoff_cost", "arc_begin", "word", "cost", "next", "final_cost", "start"}) as
// the host's BackoffLm; checked by khg_lm_validate
BackoffLm LmOf(py::object lm) {
  py::dict d = lm.attr("to_arrays")().cast<py::dict>();
  BackoffLm r;
  r.backoff = VecOf<int32_t>(d["backoff"]); r.backoff_cost = VecOf<float>(d["backoff_cost"]); r.arc_begin = VecOf<int32_t>(d["arc_begin"]);
  r.word = VecOf<int32_t>(d["word"]); r.cost = VecOf<float>(d["cost"]); r.next = VecOf<int32_t>(d["next"]);
  r.final_cost = VecOf<float>(d["final_cost"]); r.start = d["start"].cast<int32_t>();
  const size_t S = r.backoff.size();
  if (S < 1 || r.backoff_cost.size() != S || r.final_cost.size() != S || r.arc_begin.size() != S + 1)
    throw Error("khg_lm_validate: one backoff, backoff_cost and final_cost per state, one arc_begin more");
  for (size_t h = 0; h < S; ++h) if (r.arc_begin[h + 1] < r.arc_begin[h] || r.arc_begin[0] != 0) throw Error("khg_lm_validate: arc_begin must run from 0, monotone");
  const size_t A = (size_t)r.arc_begin[S];
  if (r.word.size() != A || r.cost.size() != A || r.next.size() != A) throw Error("khg_lm_validate: one word, cost and next per arc");
  CApi(khg_lm_validate((int32_t)S, r.backoff.data(), r.backoff_cost.data(), r.arc_begin.data(), r.word.data(), r.cost.data(), r.next.data(),
                       r.final_cost.data(), r.start));
  return r;
}
// DeviceLm: owns a khg_lm handle (a backoff n-gram LM resident on the device)
struct PyDeviceLm {
  khg_lm* h = nullptr;
  khg_ctx* ctx = nullptr;
  py::object ctx_obj;
  PyDeviceLm() = default;
  PyDeviceLm(const PyDeviceLm&) = delete;
  PyDeviceLm& operator=(const PyDeviceLm&) = delete;
  ~PyDeviceLm() { close(); }
  void close() { if (h) { khg_lm_destroy(h); h = nullptr; } }
};
py::dict LmStatsDict(const khg_lm_rescore_stats& s) {
  py::dict d;
  d["in_states"] = s.in_states; d["in_arcs"] = s.in_arcs; d["out_states"] = s.out_states; d["out_arcs"] = s.out_arcs; d["max_hist"] = s.max_hist;
  return d;
}
py::list NbestList(const std::vector<LatticeNbestEntry>& v) {
  py::list r;
  for (const LatticeNbestEntry& x : v) r.append(py::make_tuple(py::cast(x.words), py::cast(x.ali), py::make_tuple(x.a, x.b), x.total));
  return r;
}
// DeviceNbest: owns a khg_nbest handle (what DeviceLattices.nbest made, resident on the device)
struct PyDeviceNbest {
  khg_nbest* h = nullptr;
  khg_ctx* ctx = nullptr;
  py::object ctx_obj;
  int U = 0;
  std::vector<int32_t> status;       // KHG_LAT_* bits per utterance
  std::vector<int64_t> frames;       // [U]: the frames of every utterance's lattice (an alignment's length)
  PyDeviceNbest() = default;
  PyDeviceNbest(const PyDeviceNbest&) = delete;
  PyDeviceNbest& operator=(const PyDeviceNbest&) = delete;
  ~PyDeviceNbest() { close(); }
  void close() { if (h) { khg_nbest_destroy(h); h = nullptr; } }
};
std::vector<int64_t> NbestEntryOff(PyDeviceNbest& d) {
  if (!d.h) throw Error("DeviceNbest: closed");
  std::vector<int64_t> eo((size_t)d.U + 1, 0);
  CApi(khg_nbest_sizes(d.h, eo.data(), nullptr));
  return eo;
}
py::dict DetStatsDict(const khg_det_stats& s) {
  py::dict d;
  d["in_states"] = s.in_states; d["in_arcs"] = s.in_arcs; d["pruned_states"] = s.pruned_states; d["det_states"] = s.det_states;
  d["out_states"] = s.out_states; d["out_arcs"] = s.out_arcs; d["max_subset"] = s.max_subset; d["max_closure"] = s.max_closure;
  return d;
}
}  // namespace

void BindLattice(py::module_& m) {
  // fst::VectorFst<LatticeArc> as LatticeSimpleDecoder::GetRawLattice builds it (csrc/lattice-simple-decoder.cc:654-735; the reference's
  // Python binding does not expose the call): kaldifst's method names, plus the flat arrays as read-only numpy views
  py::class_<Lattice, std::shared_ptr<Lattice>>(m, "Lattice")
      .def_static("from_arrays", [](py::object frame, py::object graph_state, py::object tot_cost, py::object extra_cost, py::object final_cost,
                                    py::object arc_begin, py::object ilabel, py::object olabel, py::object graph_cost, py::object acoustic_cost,
                                    py::object nextstate, int start) {
        auto l = std::make_shared<Lattice>();
        l->frame = VecOf<int32_t>(frame); l->graph_state = VecOf<int32_t>(graph_state); l->tot_cost = VecOf<float>(tot_cost);
        l->extra_cost = VecOf<float>(extra_cost); l->final_cost = VecOf<float>(final_cost); l->arc_begin = VecOf<int32_t>(arc_begin);
        l->ilabel = VecOf<int32_t>(ilabel); l->olabel = VecOf<int32_t>(olabel); l->graph_cost = VecOf<float>(graph_cost);
        l->acoustic_cost = VecOf<float>(acoustic_cost); l->nextstate = VecOf<int32_t>(nextstate); l->start = start;
        const size_t N = l->frame.size(), A = l->ilabel.size();
        if (l->graph_state.size() != N || l->tot_cost.size() != N || l->extra_cost.size() != N || l->final_cost.size() != N || l->arc_begin.size() != N + 1 ||
            l->olabel.size() != A || l->graph_cost.size() != A || l->acoustic_cost.size() != A || l->nextstate.size() != A)
          throw Error("Lattice.from_arrays: one entry per state (arc_begin: one more) and one per arc");
        if (l->arc_begin[0] != 0 || (size_t)l->arc_begin[N] != A) throw Error("Lattice.from_arrays: arc_begin must run from 0 to the number of arcs");
        for (size_t s = 0; s < N; ++s) {
          if (l->arc_begin[s] > l->arc_begin[s + 1]) throw Error("Lattice.from_arrays: arc_begin not monotone");
          if (s > 0 && l->frame[s] < l->frame[s - 1]) throw Error("Lattice.from_arrays: states must be ordered by frame");
        }
        for (int32_t n : l->nextstate) if (n < 0 || (size_t)n >= N) throw Error("Lattice.from_arrays: nextstate out of range");
        if (N == 0 ? start != kNoStateId : (start < 0 || (size_t)start >= N)) throw Error("Lattice.from_arrays: start out of range");
        return l;
      }, py::arg("frame"), py::arg("graph_state"), py::arg("tot_cost"), py::arg("extra_cost"), py::arg("final_cost"), py::arg("arc_begin"),
         py::arg("ilabel"), py::arg("olabel"), py::arg("graph_cost"), py::arg("acoustic_cost"), py::arg("nextstate"), py::arg("start"))
      .def_property_readonly("num_states", &Lattice::NumStates)
      .def_property_readonly("start", &Lattice::Start)
      .def_property_readonly("num_arcs_total", [](const Lattice& l) { return l.NumArcs(); })
      .def("num_arcs", [](const Lattice& l, int s) { return l.NumArcs(s); }, py::arg("state"))
      .def("arcs", &Lattice::Arcs, py::arg("state"))
      .def("final", &Lattice::Final, py::arg("state"))
      .def("shortest_path", &Lattice::ShortestPath, py::arg("graph_scale") = 1.0f, py::arg("acoustic_scale") = 1.0f)
      // what DeviceLattices.best_path gives for this lattice and one scale pair: status (KHG_LAT_* bits), ali, words, weight (v1, v2)
      .def("best_path", [](const Lattice& l, float gs, float as) {
        const LatticeBestPath b = l.BestPath(gs, as);
        py::dict d;
        d["status"] = b.status; d["ali"] = py::cast(b.ali); d["words"] = py::cast(b.words); d["weight"] = py::make_tuple(b.v1, b.v2);
        d["arcs"] = py::cast(b.arcs);
        return d;
      }, py::arg("graph_scale") = 1.0f, py::arg("acoustic_scale") = 1.0f)
      .def("prune", [](const Lattice& l, float beam, float gs, float as) { return l.Prune(beam, gs, as); }, py::arg("beam"),
           py::arg("graph_scale") = 1.0f, py::arg("acoustic_scale") = 1.0f)
      .def("prune_with_status", [](const Lattice& l, float beam, float gs, float as) {
        int st = 0;
        std::shared_ptr<Lattice> r = l.Prune(beam, gs, as, &st);
        return py::make_tuple(r, st);
      }, py::arg("beam"), py::arg("graph_scale") = 1.0f, py::arg("acoustic_scale") = 1.0f)
      // what DeviceLattices.posteriors gives for this lattice: status, tot_like, arc_post, post (per frame [(tid, weight), ...]), alpha, beta
      .def("forward_backward", [](const Lattice& l, float gs, float as) {
        return PosteriorsDict(l.ForwardBackward(gs, as));
      }, py::arg("graph_scale") = 1.0f, py::arg("acoustic_scale") = 1.0f)
      // what DeviceLattices.mpe_posteriors gives for this lattice: forward_backward's keys -- arc_post and post hold the
      // signed values -- plus avg_acc, acc_fwd (A) and acc_bwd (B)
      .def("forward_backward_mpe", [](const Lattice& l, std::vector<int32_t> tid2phone, std::vector<int32_t> silence_phones, std::vector<int32_t> alignment,
                                      const std::string& criterion, std::vector<int32_t> tid2pdf, bool one_silence_class, float gs, float as) {
        if (criterion != "smbr" && criterion != "mpfe") throw Error("Lattice.forward_backward_mpe: criterion is \"smbr\" or \"mpfe\"");
        const LatticeMpePosteriors r = l.ForwardBackwardMpe(tid2phone, tid2pdf, silence_phones, alignment, criterion == "smbr", one_silence_class, gs, as);
        py::dict d = PosteriorsDict(r);
        d["avg_acc"] = r.avg_acc; d["acc_fwd"] = Vec1(r.acc_fwd); d["acc_bwd"] = Vec1(r.acc_bwd);
        return d;
      }, py::arg("tid2phone"), py::arg("silence_phones"), py::arg("alignment"), py::arg("criterion") = "smbr", py::arg("tid2pdf") = std::vector<int32_t>(),
         py::arg("one_silence_class") = true, py::arg("graph_scale") = 1.0f, py::arg("acoustic_scale") = 1.0f)
      // gmm-rescore-lattice on the host (what DeviceLattices.rescore gives for this lattice): loglikes is a [num_tids + 1][T] array of
      // log-likelihoods by (transition-id, frame), or a callable (frame, transition-id) -> float
      .def("rescore", [](const Lattice& l, py::object loglikes, float acoustic_scale) {
        if (PyCallable_Check(loglikes.ptr()))
          return l.Rescore([&](int t, int tid) { return loglikes(t, tid).cast<float>(); }, acoustic_scale);
        Arr<float> a = loglikes.cast<Arr<float>>();
        if (a.ndim() != 2) throw Error("Lattice.rescore: loglikes is a [num_tids + 1][T] array or a callable (frame, tid) -> float");
        const py::ssize_t n = a.shape(0), T = a.shape(1);
        const float* d = a.data();
        return l.Rescore([&](int t, int tid) {
          if (tid < 0 || tid >= n || t < 0 || t >= T) throw Error("Lattice.rescore: (frame " + std::to_string(t) + ", transition-id " + std::to_string(tid) + ") outside loglikes");
          return d[(size_t)tid * (size_t)T + (size_t)t];
        }, acoustic_scale);
      }, py::arg("loglikes"), py::arg("acoustic_scale") = 1.0f)
      // lattice-boost-ali on the host (what DeviceLattices.boost gives for this lattice)
      .def("boost", [](const Lattice& l, std::vector<int32_t> tid2phone, std::vector<int32_t> silence_phones, std::vector<int32_t> alignment, float b,
                       float max_silence_error) { return l.Boost(tid2phone, silence_phones, alignment, b, max_silence_error); },
           py::arg("tid2phone"), py::arg("silence_phones"), py::arg("alignment"), py::arg("b") = 0.1f, py::arg("max_silence_error") = 0.0f)
      // lattice-lmrescore on the host (what DeviceLattices.lm_rescore gives for this lattice): lm is an NgramLm ->
      // (Lattice, status, stats)
      .def("lm_rescore", [](const Lattice& l, py::object lm, float scale, int hist_factor) {
        const BackoffLm b = LmOf(lm);
        const LatticeLmRescored r = l.LmRescore(b, scale, hist_factor);
        khg_lm_rescore_stats s = {l.NumStates(), l.NumArcs(), r.lattice->NumStates(), r.lattice->NumArcs(), r.max_hist};
        return py::make_tuple(r.lattice, r.status, LmStatsDict(s));
      }, py::arg("lm"), py::arg("scale") = 1.0f, py::arg("hist_factor") = 8)
      // lattice-determinize-pruned on the host (what DeviceLattices.determinize gives for this lattice) ->
      // (Lattice, status, stats)
      .def("determinize", [](const Lattice& l, float gs, float as, float beam, float delta, int state_factor) {
        const LatticeDeterminized r = l.Determinize(gs, as, beam, delta, state_factor);
        return py::make_tuple(r.lattice, r.status, DetStatsDict(r.stats));
      }, py::arg("graph_scale") = 1.0f, py::arg("acoustic_scale") = 1.0f, py::arg("beam") = 10.0f, py::arg("delta") = 1.0f / 1024.0f,
         py::arg("state_factor") = 8)
      // lattice-to-nbest on the host (what DeviceLattices.nbest gives for this lattice) -> a list of (words, alignment,
      // (graph, acoustic), total), cheapest first; nbest_with_status -> (that list, status, per entry its arcs with the final state last)
      .def("nbest", [](const Lattice& l, int n, float gs, float as) { return NbestList(l.Nbest(n, gs, as)); }, py::arg("n"),
           py::arg("graph_scale") = 1.0f, py::arg("acoustic_scale") = 1.0f)
      .def("nbest_with_status", [](const Lattice& l, int n, float gs, float as) {
        int st = 0;
        const std::vector<LatticeNbestEntry> v = l.Nbest(n, gs, as, &st);
        py::list paths;
        for (const LatticeNbestEntry& x : v) {
          std::vector<int32_t> p = x.arcs;
          p.push_back(x.end_state);
          paths.append(py::tuple(py::cast(p)));
        }
        return py::make_tuple(NbestList(v), st, paths);
      }, py::arg("n"), py::arg("graph_scale") = 1.0f, py::arg("acoustic_scale") = 1.0f)
      // lattice-add-penalty on the host (what DeviceLattices.add_penalty gives for this lattice)
      .def("add_penalty", [](const Lattice& l, float p) { return l.AddPenalty(p); }, py::arg("word_ins_penalty"))
      // lattice-oracle on the host (what DeviceLattices.oracle gives for this lattice): status (KHG_LAT_* bits), counts
      // (errors, insertions, deletions, substitutions), words, ali (one transition-id per frame, 0 where the path has none), arcs
      .def("oracle", [](const Lattice& l, std::vector<int32_t> ref) {
        const LatticeOracle r = l.Oracle(ref);
        py::dict d;
        d["status"] = r.status; d["counts"] = Vec1(std::vector<int32_t>(r.counts, r.counts + 4)); d["words"] = Vec1(r.words); d["ali"] = Vec1(r.ali);
        d["arcs"] = Vec1(r.arcs);
        return d;
      }, py::arg("ref"))
      // lattice-mbr-decode and the word confidences on the host (what DeviceLattices.mbr gives for this lattice): status,
      // iters, bayes_risk, words, conf, vocab, gamma [Q][len(vocab)], arc_cond, final_cond, cap, risks (one per accumulation).  init: the
      // initial hypothesis (None: the best path's words); arc_cond / final_cond replace the host's own weights (the device's, to compare
      // bit for bit)
      .def("mbr", [](const Lattice& l, float gs, float as, bool decode_mbr, int max_iter, py::object init, int max_words, py::object arc_cond,
                     py::object final_cond) {
        std::vector<int32_t> h;
        std::vector<double> ac, fc;
        if (!init.is_none()) h = VecOf<int32_t>(init);
        if (!arc_cond.is_none()) ac = VecOf<double>(arc_cond);
        if (!final_cond.is_none()) fc = VecOf<double>(final_cond);
        const LatticeMbr r = l.Mbr(gs, as, decode_mbr, max_iter, init.is_none() ? nullptr : &h, max_words, arc_cond.is_none() ? nullptr : &ac,
                                   final_cond.is_none() ? nullptr : &fc);
        const bool ok = (r.status & KHG_LAT_SUCCEEDED) != 0;
        const py::ssize_t V = ok ? (py::ssize_t)r.vocab.size() : 0, Q = ok ? 2 * (py::ssize_t)r.words.size() + 1 : 0;
        py::dict d;
        d["status"] = r.status; d["iters"] = r.iters; d["bayes_risk"] = r.bayes_risk; d["words"] = Vec1(r.words); d["conf"] = Vec1(r.conf);
        d["vocab"] = Vec1(ok ? r.vocab : std::vector<int32_t>());
        Arr<double> g({Q, V});
        if (ok && !r.gamma.empty()) std::memcpy(g.mutable_data(), r.gamma.data(), sizeof(double) * r.gamma.size());
        d["gamma"] = g; d["arc_cond"] = Vec1(r.arc_cond); d["final_cond"] = Vec1(r.final_cond); d["cap"] = r.cap; d["risks"] = Vec1(r.risks);
        return d;
      }, py::arg("graph_scale") = 1.0f, py::arg("acoustic_scale") = 1.0f, py::arg("decode_mbr") = true, py::arg("max_iter") = 32, py::arg("init") = py::none(),
         py::arg("max_words") = 0, py::arg("arc_cond") = py::none(), py::arg("final_cond") = py::none())
      .def("to_text", &Lattice::ToText)
      .def("__str__", &Lattice::ToText)
      .def_property_readonly("frame", [](py::object s) { auto& l = s.cast<Lattice&>(); return LatView(s, l.frame, l.frame.size()); })
      .def_property_readonly("graph_state", [](py::object s) { auto& l = s.cast<Lattice&>(); return LatView(s, l.graph_state, l.graph_state.size()); })
      .def_property_readonly("tot_cost", [](py::object s) { auto& l = s.cast<Lattice&>(); return LatView(s, l.tot_cost, l.tot_cost.size()); })
      .def_property_readonly("extra_cost", [](py::object s) { auto& l = s.cast<Lattice&>(); return LatView(s, l.extra_cost, l.extra_cost.size()); })
      .def_property_readonly("final_cost", [](py::object s) { auto& l = s.cast<Lattice&>(); return LatView(s, l.final_cost, l.final_cost.size()); })
      .def_property_readonly("arc_begin", [](py::object s) { auto& l = s.cast<Lattice&>(); return LatView(s, l.arc_begin, l.arc_begin.size()); })
      .def_property_readonly("ilabel", [](py::object s) { auto& l = s.cast<Lattice&>(); return LatView(s, l.ilabel, l.ilabel.size()); })
      .def_property_readonly("olabel", [](py::object s) { auto& l = s.cast<Lattice&>(); return LatView(s, l.olabel, l.olabel.size()); })
      .def_property_readonly("graph_cost", [](py::object s) { auto& l = s.cast<Lattice&>(); return LatView(s, l.graph_cost, l.graph_cost.size()); })
      .def_property_readonly("acoustic_cost", [](py::object s) { auto& l = s.cast<Lattice&>(); return LatView(s, l.acoustic_cost, l.acoustic_cost.size()); })
      .def_property_readonly("nextstate", [](py::object s) { auto& l = s.cast<Lattice&>(); return LatView(s, l.nextstate, l.nextstate.size()); });

  // get_raw_lattice_simple_batch(am, tm, fsts, feats_list, config, acoustic_scale, scratch_per_frame=0, return_scores=False,
  // return_times=False) -> one dict per utterance: decode_lattice_simple_batch's keys plus "lattice" (a Lattice; no states unless
  // the utterance succeeded).  fsts as there: a list of graphs, one StdVectorFst or a DecodingGraph (shared, nothing repeated).
  // return_times: (dicts, {"decode_s", "download_s"}) -- the C-ABI decode call and the download of the lattices.
  m.def("get_raw_lattice_simple_batch", [](std::shared_ptr<AmDiagGmm> am, std::shared_ptr<TransitionModel> tm, py::object fsts, py::list feats_list,
                                           const LatticeSimpleDecoderConfig& config, float acoustic_scale, int scratch_per_frame, bool return_scores,
                                           bool return_times) -> py::object {
    BatchArgs b(*am, fsts, feats_list, "get_raw_lattice_simple_batch");
    std::vector<LatticeResult> rs;
    std::vector<std::shared_ptr<Lattice>> lats;
    double sec[2] = {0.0, 0.0};
    {
      const GraphsCsr csr = b.Csr();
      py::gil_scoped_release nogil;
      rs = GetRawLatticeSimpleBatch(*am, *tm, csr, b.fp, b.nf, config, acoustic_scale, return_scores, scratch_per_frame, &lats, sec);
    }
    py::list out;
    for (size_t u = 0; u < rs.size(); ++u) {
      py::dict d = LatticeSimpleToDict(rs[u], b.nf[u], return_scores);
      d["lattice"] = lats[u];
      out.append(d);
    }
    if (!return_times) return std::move(out);
    py::dict t;
    t["decode_s"] = sec[0]; t["download_s"] = sec[1];
    return py::make_tuple(out, t);
  }, py::arg("am"), py::arg("tm"), py::arg("fsts"), py::arg("feats_list"), py::arg("config"), py::arg("acoustic_scale"),
     py::arg("scratch_per_frame") = 0, py::arg("return_scores") = false, py::arg("return_times") = false);

  // DeviceLattices: the raw lattices of a batch resident on the device (a khg_lattices handle) and the operations on them
  py::class_<PyDeviceLattices, std::shared_ptr<PyDeviceLattices>>(m, "DeviceLattices")
      .def_static("from_lattices", [](std::vector<std::shared_ptr<Lattice>> lats, py::object ctx) {
        auto d = std::make_shared<PyDeviceLattices>();
        d->ctx_obj = ctx;
        d->ctx = ctx.is_none() ? DefaultCtx() : reinterpret_cast<khg_ctx*>(ctx.attr("h").cast<uintptr_t>());
        d->h = UploadLattices(d->ctx, lats);
        return d;
      }, py::arg("lattices"), py::arg("ctx") = py::none())
      // the host-only half of from_lattices: raises what khg_lattices_upload would refuse
      .def_static("validate", [](std::vector<std::shared_ptr<Lattice>> lats) { (void)UploadLattices(nullptr, lats); }, py::arg("lattices"))
      .def_property_readonly("num_utts", [](PyDeviceLattices& d) { return (int)LatSizes(d).first.size() - 1; })
      .def_property_readonly("state_off", [](PyDeviceLattices& d) { return Vec1(LatSizes(d).first); })
      .def_property_readonly("arc_off", [](PyDeviceLattices& d) { return Vec1(LatSizes(d).second); })
      // the decoder launches (chunks of <= 4 GiB of scratch) the lattices were emitted in, and the first utterance of each (n_utt last)
      .def_property_readonly("num_chunks", [](PyDeviceLattices& d) {
        if (!d.h) throw Error("DeviceLattices: closed");
        int32_t n = 0;
        CApi(khg_lattices_num_chunks(d.h, &n));
        return (int)n;
      })
      .def_property_readonly("chunk_off", [](PyDeviceLattices& d) {
        if (!d.h) throw Error("DeviceLattices: closed");
        int32_t n = 0;
        CApi(khg_lattices_num_chunks(d.h, &n));
        std::vector<int32_t> first((size_t)n + 1, 0);
        CApi(khg_lattices_chunk_utts(d.h, first.data()));
        return std::vector<int>(first.begin(), first.end());
      })
      .def_property_readonly("device_bytes", [](PyDeviceLattices& d) {
        if (!d.h) throw Error("DeviceLattices: closed");
        int64_t b = 0;
        CApi(khg_lattices_device_bytes(d.h, &b));
        return b;
      })
      // of the prune that made this handle (None otherwise): KHG_LAT_* bits per utterance
      .def_property_readonly("status", [](PyDeviceLattices& d) -> py::object { if (d.status.empty()) return py::none(); return Vec1(d.status); })
      .def("best_path", [](PyDeviceLattices& d, Arr<float> gs, Arr<float> as) {
        const auto so = LatSizes(d);
        if (gs.ndim() != 1 || as.ndim() != 1 || gs.shape(0) != as.shape(0) || gs.shape(0) < 1)
          throw Error("DeviceLattices.best_path: graph_scales and acoustic_scales are two lists of the same length >= 1");
        const int U = (int)so.first.size() - 1, K = (int)gs.shape(0);
        std::vector<int32_t> st((size_t)K * U);
        std::vector<int64_t> woff((size_t)K * U + 1);
        std::vector<float> w(2 * (size_t)K * U);
        const int64_t wcap = (int64_t)K * so.first.back() + 1;       // a path visits a state once
        std::unique_ptr<int32_t[]> words(new int32_t[(size_t)wcap]);        // (not zeroed: only the packed words are read)
        // the alignment layout: the frame of every utterance's last state (a path has one transition-id per frame)
        std::vector<int64_t> aoff((size_t)U + 1, 0);
        CApi(khg_lattices_ali_layout(d.ctx, d.h, aoff.data()));
        const int64_t at = aoff.back();
        Arr<int32_t> ali({(py::ssize_t)K, (py::ssize_t)at});
        {
          py::gil_scoped_release nogil;
          CApi(khg_lattices_best_path(d.ctx, d.h, K, gs.data(), as.data(), ali.mutable_data(), words.get(), woff.data(), wcap, w.data(), st.data()));
        }
        Arr<int32_t> wa1({(py::ssize_t)woff.back()});
        if (woff.back() > 0) std::memcpy(wa1.mutable_data(), words.get(), sizeof(int32_t) * (size_t)woff.back());
        py::dict r;
        r["ali"] = ali; r["words"] = wa1; r["words_off"] = Vec1(woff); r["status"] = Vec1(st); r["ali_off"] = Vec1(aoff);
        Arr<float> wa({(py::ssize_t)K * U, (py::ssize_t)2});
        if (!w.empty()) std::memcpy(wa.mutable_data(), w.data(), sizeof(float) * w.size());
        r["weight"] = wa;
        return r;
      }, py::arg("graph_scales"), py::arg("acoustic_scales"))
      .def("prune", [](PyDeviceLattices& d, float beam, float gs, float as) {
        const int U = (int)LatSizes(d).first.size() - 1;
        auto r = std::make_shared<PyDeviceLattices>();
        r->ctx = d.ctx; r->ctx_obj = d.ctx_obj;
        r->status.assign((size_t)std::max(U, 1), 0);
        {
          py::gil_scoped_release nogil;
          CApi(khg_lattices_prune(d.ctx, d.h, gs, as, beam, r->status.data(), &r->h));
        }
        r->status.resize((size_t)U);
        return r;
      }, py::arg("beam"), py::arg("graph_scale") = 1.0f, py::arg("acoustic_scale") = 1.0f)
      // LatticeForwardBackward / lattice-to-post under one scale pair -> DevicePosteriors, resident on the device
      .def("posteriors", [](PyDeviceLattices& d, float gs, float as) {
        const auto so = LatSizes(d);
        const int U = (int)so.first.size() - 1;
        auto r = std::make_shared<PyDevicePosteriors>();
        r->ctx = d.ctx; r->ctx_obj = d.ctx_obj; r->arc_off = so.second;
        r->status.assign((size_t)std::max(U, 1), 0);
        r->tot_like.assign((size_t)std::max(U, 1), 0.0);
        {
          py::gil_scoped_release nogil;
          CApi(khg_lattices_posteriors(d.ctx, d.h, gs, as, r->status.data(), r->tot_like.data(), &r->h));
        }
        r->status.resize((size_t)U); r->tot_like.resize((size_t)U);
        return r;
      }, py::arg("graph_scale") = 1.0f, py::arg("acoustic_scale") = 1.0f)
      // gmm-rescore-lattice -> a new DeviceLattices: every emitting arc's acoustic_cost = -(acoustic_scale * loglike of
      // its (frame, pdf)).  mode "cells": computed from the set's features and the model for the distinct cells the lattices name (a
      // features-only set works); "from_ll": gathered from the set's resident scores.  The result carries .status and .rescore_stats
      .def("rescore", [](PyDeviceLattices& d, py::object utts, py::object model, py::object transitions, float acoustic_scale, const std::string& mode) {
        if (!d.h) throw Error("DeviceLattices: closed");
        int md;
        if (mode == "cells") md = KHG_RESCORE_CELLS;
        else if (mode == "from_ll") md = KHG_RESCORE_FROM_LL;
        else throw Error("DeviceLattices.rescore: mode is \"cells\" or \"from_ll\"");
        khg_utts* uh = reinterpret_cast<khg_utts*>(utts.attr("h").cast<uintptr_t>());
        khg_model* mh = reinterpret_cast<khg_model*>(model.attr("h").cast<uintptr_t>());
        khg_tm* th = reinterpret_cast<khg_tm*>(transitions.attr("h").cast<uintptr_t>());
        auto r = std::make_shared<PyDeviceLattices>();
        r->ctx = d.ctx; r->ctx_obj = d.ctx_obj;
        {
          py::gil_scoped_release nogil;
          CApi(khg_lattices_rescore(d.ctx, mh, th, uh, d.h, acoustic_scale, md, &r->rescore_stats, &r->h));
        }
        r->has_rescore_stats = true;
        int32_t U = 0;
        CApi(khg_lattices_num_utts(r->h, &U));
        r->status.assign((size_t)std::max(U, 1), 0);
        CApi(khg_lattices_op_status(r->h, r->status.data()));
        r->status.resize((size_t)U);
        return r;
      }, py::arg("utts"), py::arg("model"), py::arg("transitions"), py::arg("acoustic_scale") = 1.0f, py::arg("mode") = "cells")
      // {"arcs", "emitting_arcs", "cells"} of the rescore that made this handle (None otherwise)
      .def_property_readonly("rescore_stats", [](PyDeviceLattices& d) -> py::object {
        if (!d.has_rescore_stats) return py::none();
        py::dict s;
        s["arcs"] = d.rescore_stats.arcs; s["emitting_arcs"] = d.rescore_stats.emitting_arcs; s["cells"] = d.rescore_stats.cells;
        return std::move(s);
      })
      // lattice-boost-ali -> a new DeviceLattices with graph_cost += -b * e per emitting arc.  alignment: one array of
      // transition-ids per utterance (a list), or ali_set: an UtteranceSet whose resident alignment (align / upload_ali) is the reference
      .def("boost", [](PyDeviceLattices& d, Arr<int32_t> tid2phone, Arr<int32_t> silence_phones, py::object alignment, py::object ali_set, float b,
                       float max_silence_error) {
        if (!d.h) throw Error("DeviceLattices: closed");
        if (tid2phone.ndim() != 1 || tid2phone.shape(0) < 1 || silence_phones.ndim() != 1) throw Error("DeviceLattices.boost: tid2phone [num_tids + 1] and silence_phones are flat arrays");
        const int U = (int)LatSizes(d).first.size() - 1;
        std::vector<int64_t> aoff;
        std::vector<int32_t> ali;
        FlattenAlignments("DeviceLattices.boost", alignment, U, &aoff, &ali);
        const khg_utts* sh = ali_set.is_none() ? nullptr : reinterpret_cast<const khg_utts*>(ali_set.attr("h").cast<uintptr_t>());
        auto r = std::make_shared<PyDeviceLattices>();
        r->ctx = d.ctx; r->ctx_obj = d.ctx_obj;
        r->status.assign((size_t)std::max(U, 1), 0);
        {
          py::gil_scoped_release nogil;
          CApi(khg_lattices_boost(d.ctx, d.h, (int32_t)tid2phone.shape(0) - 1, tid2phone.data(), (int32_t)silence_phones.shape(0), silence_phones.data(),
                                  aoff.empty() ? nullptr : aoff.data(), aoff.empty() ? nullptr : ali.data(), sh, b, max_silence_error, r->status.data(), &r->h));
        }
        r->status.resize((size_t)U);
        return r;
      }, py::arg("tid2phone"), py::arg("silence_phones"), py::arg("alignment") = py::none(), py::arg("ali_set") = py::none(), py::arg("b") = 0.1f,
         py::arg("max_silence_error") = 0.0f)
      // lattice-to-mpe-post / lattice-to-smbr-post -> DevicePosteriors with SIGNED weights, carrying .avg_acc (the expected
      // frame accuracy per utterance).  The reference as boost takes it: alignment (a list of arrays) or ali_set
      .def("mpe_posteriors", [](PyDeviceLattices& d, Arr<int32_t> tid2phone, Arr<int32_t> silence_phones, py::object alignment, py::object ali_set,
                                const std::string& criterion, py::object tid2pdf, bool one_silence_class, float gs, float as) {
        if (!d.h) throw Error("DeviceLattices: closed");
        if (tid2phone.ndim() != 1 || tid2phone.shape(0) < 1 || silence_phones.ndim() != 1)
          throw Error("DeviceLattices.mpe_posteriors: tid2phone [num_tids + 1] and silence_phones are flat arrays");
        int crit;
        if (criterion == "smbr") crit = KHG_MPE_SMBR;
        else if (criterion == "mpfe") crit = KHG_MPE_MPFE;
        else throw Error("DeviceLattices.mpe_posteriors: criterion is \"smbr\" or \"mpfe\"");
        Arr<int32_t> t2pdf;
        const bool has_pdf = !tid2pdf.is_none();
        if (has_pdf) {
          t2pdf = tid2pdf.cast<Arr<int32_t>>();
          if (t2pdf.ndim() != 1 || t2pdf.shape(0) != tid2phone.shape(0)) throw Error("DeviceLattices.mpe_posteriors: tid2pdf has tid2phone's length");
        }
        const auto so = LatSizes(d);
        const int U = (int)so.first.size() - 1;
        std::vector<int64_t> aoff;
        std::vector<int32_t> ali;
        FlattenAlignments("DeviceLattices.mpe_posteriors", alignment, U, &aoff, &ali);
        const khg_utts* sh = ali_set.is_none() ? nullptr : reinterpret_cast<const khg_utts*>(ali_set.attr("h").cast<uintptr_t>());
        auto r = std::make_shared<PyDevicePosteriors>();
        r->ctx = d.ctx; r->ctx_obj = d.ctx_obj; r->arc_off = so.second;
        r->status.assign((size_t)std::max(U, 1), 0);
        r->tot_like.assign((size_t)std::max(U, 1), 0.0);
        r->avg_acc.assign((size_t)std::max(U, 1), 0.0);
        r->has_avg_acc = true;
        {
          py::gil_scoped_release nogil;
          CApi(khg_lattices_mpe_posteriors(d.ctx, d.h, (int32_t)tid2phone.shape(0) - 1, tid2phone.data(), has_pdf ? t2pdf.data() : nullptr,
                                           (int32_t)silence_phones.shape(0), silence_phones.data(), aoff.empty() ? nullptr : aoff.data(),
                                           aoff.empty() ? nullptr : ali.data(), sh, crit, one_silence_class ? 1 : 0, gs, as, r->status.data(),
                                           r->tot_like.data(), r->avg_acc.data(), &r->h));
        }
        r->status.resize((size_t)U); r->tot_like.resize((size_t)U); r->avg_acc.resize((size_t)U);
        return r;
      }, py::arg("tid2phone"), py::arg("silence_phones"), py::arg("alignment") = py::none(), py::arg("ali_set") = py::none(), py::arg("criterion") = "smbr",
         py::arg("tid2pdf") = py::none(), py::arg("one_silence_class") = true, py::arg("graph_scale") = 1.0f, py::arg("acoustic_scale") = 1.0f)
      // lattice-lmrescore -> (a new DeviceLattices carrying .status, status, stats): lm is a DeviceLm of the same context
      .def("lm_rescore", [](PyDeviceLattices& d, PyDeviceLm& lm, float scale, int hist_factor) {
        if (!d.h) throw Error("DeviceLattices: closed");
        if (!lm.h) throw Error("DeviceLm: closed");
        const int U = (int)LatSizes(d).first.size() - 1;
        auto r = std::make_shared<PyDeviceLattices>();
        r->ctx = d.ctx; r->ctx_obj = d.ctx_obj;
        r->status.assign((size_t)std::max(U, 1), 0);
        khg_lm_rescore_stats st = {0, 0, 0, 0, 0};
        {
          py::gil_scoped_release nogil;
          CApi(khg_lattices_lm_rescore(d.ctx, d.h, lm.h, scale, hist_factor, r->status.data(), &st, &r->h));
        }
        r->status.resize((size_t)U);
        return py::make_tuple(r, Vec1(r->status), LmStatsDict(st));
      }, py::arg("lm"), py::arg("scale") = 1.0f, py::arg("hist_factor") = 8)
      // lattice-determinize-pruned -> (a new DeviceLattices carrying .status, status, stats)
      .def("determinize", [](PyDeviceLattices& d, float gs, float as, float beam, float delta, int state_factor) {
        if (!d.h) throw Error("DeviceLattices: closed");
        const int U = (int)LatSizes(d).first.size() - 1;
        auto r = std::make_shared<PyDeviceLattices>();
        r->ctx = d.ctx; r->ctx_obj = d.ctx_obj;
        r->status.assign((size_t)std::max(U, 1), 0);
        khg_det_stats st = {0, 0, 0, 0, 0, 0, 0, 0};
        {
          py::gil_scoped_release nogil;
          CApi(khg_lattices_determinize(d.ctx, d.h, gs, as, beam, delta, state_factor, r->status.data(), &st, &r->h));
        }
        r->status.resize((size_t)U);
        return py::make_tuple(r, Vec1(r->status), DetStatsDict(st));
      }, py::arg("graph_scale") = 1.0f, py::arg("acoustic_scale") = 1.0f, py::arg("beam") = 10.0f, py::arg("delta") = 1.0f / 1024.0f,
         py::arg("state_factor") = 8)
      // lattice-add-penalty -> a new DeviceLattices: graph_cost += word_ins_penalty on every arc with a word
      .def("add_penalty", [](PyDeviceLattices& d, float p) {
        if (!d.h) throw Error("DeviceLattices: closed");
        auto r = std::make_shared<PyDeviceLattices>();
        r->ctx = d.ctx; r->ctx_obj = d.ctx_obj;
        {
          py::gil_scoped_release nogil;
          CApi(khg_lattices_add_penalty(d.ctx, d.h, p, &r->h));
        }
        return r;
      }, py::arg("word_ins_penalty"))
      // lattice-oracle: refs is one word sequence per utterance -> counts [U][4] (errors, insertions, deletions,
      // substitutions), words / words_off, ali / ali_off (the oracle path's transition-ids by frame), status
      .def("oracle", [](PyDeviceLattices& d, py::object refs, int64_t scratch_bytes) {
        const auto so = LatSizes(d);
        const int U = (int)so.first.size() - 1;
        std::vector<int64_t> roff;
        std::vector<int32_t> rw;
        FlattenRefs(refs, &roff, &rw);
        std::vector<int64_t> aoff((size_t)U + 1, 0), woff((size_t)U + 1, 0);
        std::vector<int32_t> st((size_t)std::max(U, 1), 0);
        Arr<int32_t> counts({(py::ssize_t)U, (py::ssize_t)4});
        const int64_t wcap = so.first.back() + 1;       // a path visits a state once
        std::unique_ptr<int32_t[]> words(new int32_t[(size_t)wcap]);
        if ((int)roff.size() - 1 == U) CApi(khg_lattices_ali_layout(d.ctx, d.h, aoff.data()));
        Arr<int32_t> ali({(py::ssize_t)aoff.back()});
        if (aoff.back() > 0) std::memset(ali.mutable_data(), 0, sizeof(int32_t) * (size_t)aoff.back());
        {
          py::gil_scoped_release nogil;
          CApi(khg_lattices_oracle(d.ctx, d.h, (int32_t)roff.size() - 1, rw.data(), roff.data(), scratch_bytes, counts.mutable_data(), words.get(), woff.data(),
                                   wcap, ali.mutable_data(), st.data()));
        }
        st.resize((size_t)U);
        Arr<int32_t> wa({(py::ssize_t)woff.back()});
        if (woff.back() > 0) std::memcpy(wa.mutable_data(), words.get(), sizeof(int32_t) * (size_t)woff.back());
        py::dict r;
        r["counts"] = counts; r["words"] = wa; r["words_off"] = Vec1(woff); r["ali"] = ali; r["ali_off"] = Vec1(aoff); r["status"] = Vec1(st);
        return r;
      }, py::arg("refs"), py::arg("scratch_bytes") = 0)
      // score.sh's sweep: for every (graph_scale, acoustic_scale, penalty) triple the best path's word errors against refs
      // -> counts [K * U][4], nwords [K * U], status [K * U]; entry k * U + u is triple k of utterance u
      .def("wer", [](PyDeviceLattices& d, py::object refs, Arr<float> gs, Arr<float> as, Arr<float> pen) {
        const auto so = LatSizes(d);
        if (gs.ndim() != 1 || as.ndim() != 1 || pen.ndim() != 1 || gs.shape(0) != as.shape(0) || gs.shape(0) != pen.shape(0) || gs.shape(0) < 1)
          throw Error("DeviceLattices.wer: graph_scales, acoustic_scales and penalties are three lists of the same length >= 1");
        const int U = (int)so.first.size() - 1, K = (int)gs.shape(0);
        std::vector<int64_t> roff;
        std::vector<int32_t> rw;
        FlattenRefs(refs, &roff, &rw);
        Arr<int32_t> counts({(py::ssize_t)K * U, (py::ssize_t)4});
        std::vector<int32_t> nw((size_t)K * U + 1, 0), st((size_t)K * U + 1, 0);
        {
          py::gil_scoped_release nogil;
          CApi(khg_lattices_wer(d.ctx, d.h, (int32_t)roff.size() - 1, rw.data(), roff.data(), K, gs.data(), as.data(), pen.data(), counts.mutable_data(),
                                nw.data(), st.data()));
        }
        nw.resize((size_t)K * U); st.resize((size_t)K * U);
        py::dict r;
        r["counts"] = counts; r["nwords"] = Vec1(nw); r["status"] = Vec1(st);
        return r;
      }, py::arg("refs"), py::arg("graph_scales"), py::arg("acoustic_scales"), py::arg("penalties"))
      // lattice-mbr-decode and word confidences.  init: None, or one word sequence (or None: the best path's words) per
      // utterance -> status, iters, bayes_risk [U]; words / conf with words_off; vocab with vocab_off; gamma (flat; utterance u's
      // [Q][len(vocab)] table at gamma_off[u]); arc_cond / final_cond with arc_off / state_off: the weights the device used
      .def("mbr", [](PyDeviceLattices& d, float gs, float as, bool decode_mbr, int max_iter, py::object init, int max_words, int64_t scratch_bytes) {
        const auto so = LatSizes(d);
        const int U = (int)so.first.size() - 1;
        std::vector<int64_t> ioff;
        std::vector<int32_t> iw, given;
        int32_t n_utt = U;
        if (!init.is_none()) {
          ioff.assign(1, 0);
          for (py::handle h : init) {
            py::object o = py::reinterpret_borrow<py::object>(h);
            given.push_back(o.is_none() ? 0 : 1);
            if (!o.is_none()) {
              Arr<int32_t> a = o.cast<Arr<int32_t>>();
              iw.insert(iw.end(), a.data(), a.data() + a.size());
            }
            ioff.push_back((int64_t)iw.size());
          }
          n_utt = (int32_t)given.size();
          given.push_back(0);
        }
        iw.push_back(0);      // (never a NULL array)
        khg_mbr* mh = nullptr;
        {
          py::gil_scoped_release nogil;
          CApi(khg_lattices_mbr(d.ctx, d.h, gs, as, decode_mbr ? 1 : 0, max_iter, n_utt, iw.data(), ioff.empty() ? nullptr : ioff.data(),
                                ioff.empty() ? nullptr : given.data(), max_words, scratch_bytes, &mh));
        }
        std::unique_ptr<khg_mbr, int (*)(khg_mbr*)> guard(mh, khg_mbr_destroy);
        std::vector<int64_t> woff((size_t)U + 1, 0), voff((size_t)U + 1, 0), goff((size_t)U + 1, 0);
        CApi(khg_mbr_sizes(mh, woff.data(), voff.data(), goff.data()));
        std::vector<int32_t> st((size_t)U + 1, 0), it((size_t)U + 1, 0);
        Arr<double> risk({(py::ssize_t)U}), conf({(py::ssize_t)woff.back()}), gamma({(py::ssize_t)goff.back()}), ac({(py::ssize_t)so.second.back()}),
            fc({(py::ssize_t)so.first.back()});
        Arr<int32_t> words({(py::ssize_t)woff.back()}), vocab({(py::ssize_t)voff.back()});
        {
          py::gil_scoped_release nogil;
          CApi(khg_mbr_download(d.ctx, mh, st.data(), it.data(), risk.mutable_data(), words.mutable_data(), conf.mutable_data(), vocab.mutable_data(),
                                gamma.mutable_data(), ac.mutable_data(), fc.mutable_data()));
        }
        st.resize((size_t)U); it.resize((size_t)U);
        py::dict r;
        r["status"] = Vec1(st); r["iters"] = Vec1(it); r["bayes_risk"] = risk; r["words"] = words; r["words_off"] = Vec1(woff); r["conf"] = conf;
        r["vocab"] = vocab; r["vocab_off"] = Vec1(voff); r["gamma"] = gamma; r["gamma_off"] = Vec1(goff); r["arc_cond"] = ac; r["final_cond"] = fc;
        r["arc_off"] = Vec1(so.second); r["state_off"] = Vec1(so.first);
        return r;
      }, py::arg("graph_scale") = 1.0f, py::arg("acoustic_scale") = 1.0f, py::arg("decode_mbr") = true, py::arg("max_iter") = 32, py::arg("init") = py::none(),
         py::arg("max_words") = 0, py::arg("scratch_bytes") = 0)
      // lattice-to-nbest -> a DeviceNbest: the n cheapest paths of every utterance, resident on the device
      .def("nbest", [](PyDeviceLattices& d, int n, float gs, float as) {
        const int U = (int)LatSizes(d).first.size() - 1;
        auto r = std::make_shared<PyDeviceNbest>();
        r->ctx = d.ctx; r->ctx_obj = d.ctx_obj; r->U = U;
        r->status.assign((size_t)std::max(U, 1), 0);
        std::vector<int64_t> aoff((size_t)U + 1, 0);
        {
          py::gil_scoped_release nogil;
          CApi(khg_lattices_nbest(d.ctx, d.h, gs, as, n, r->status.data(), &r->h));
          CApi(khg_lattices_ali_layout(d.ctx, d.h, aoff.data()));
        }
        r->status.resize((size_t)U);
        for (int u = 0; u < U; ++u) r->frames.push_back(aoff[(size_t)u + 1] - aoff[(size_t)u]);
        return r;
      }, py::arg("n"), py::arg("graph_scale") = 1.0f, py::arg("acoustic_scale") = 1.0f)
      .def("download", [](PyDeviceLattices& d) {
        if (!d.h) throw Error("DeviceLattices: closed");
        std::vector<std::shared_ptr<Lattice>> out;
        {
          py::gil_scoped_release nogil;
          out = DownloadLattices(d.ctx, d.h);
        }
        return out;
      })
      .def("close", &PyDeviceLattices::close);

  // DeviceNbest: the n-best lists of a batch resident on the device (a khg_nbest handle)
  py::class_<PyDeviceNbest, std::shared_ptr<PyDeviceNbest>>(m, "DeviceNbest")
      .def_property_readonly("num_utts", [](PyDeviceNbest& d) { return d.U; })
      // the entries of every utterance
      .def_property_readonly("counts", [](PyDeviceNbest& d) {
        const std::vector<int64_t> eo = NbestEntryOff(d);
        std::vector<int64_t> c((size_t)d.U);
        for (int u = 0; u < d.U; ++u) c[(size_t)u] = eo[(size_t)u + 1] - eo[(size_t)u];
        return Vec1(c);
      })
      .def_property_readonly("status", [](PyDeviceNbest& d) { return Vec1(d.status); })
      .def_property_readonly("device_bytes", [](PyDeviceNbest& d) {
        if (!d.h) throw Error("DeviceNbest: closed");
        int64_t b = 0;
        CApi(khg_nbest_device_bytes(d.h, &b));
        return b;
      })
      // -> the flat arrays: status [U], entry_off [U + 1], and per entry words (words_off), ali (ali_off), weight [entries][2], total
      .def("download", [](PyDeviceNbest& d) {
        const std::vector<int64_t> eo = NbestEntryOff(d);
        const int64_t E = eo.back();
        std::vector<int64_t> wo((size_t)E + 1, 0), ao((size_t)E + 1, 0);
        CApi(khg_nbest_sizes(d.h, nullptr, wo.data()));
        for (int u = 0; u < d.U; ++u)
          for (int64_t e = eo[(size_t)u]; e < eo[(size_t)u + 1]; ++e) ao[(size_t)e + 1] = ao[(size_t)e] + d.frames[(size_t)u];
        Arr<int32_t> ali({(py::ssize_t)ao.back()}), words({(py::ssize_t)wo.back()});
        Arr<float> weight({(py::ssize_t)E, (py::ssize_t)2}), total({(py::ssize_t)E});
        {
          py::gil_scoped_release nogil;
          CApi(khg_nbest_download(d.ctx, d.h, ali.mutable_data(), words.mutable_data(), weight.mutable_data(), total.mutable_data()));
        }
        py::dict r;
        r["status"] = Vec1(d.status); r["entry_off"] = Vec1(eo); r["words"] = words; r["words_off"] = Vec1(wo); r["ali"] = ali; r["ali_off"] = Vec1(ao);
        r["weight"] = weight; r["total"] = total;
        return r;
      })
      .def("close", &PyDeviceNbest::close);

  // compute-wer's core on the host (khg_edit_distance): (errors, insertions, deletions, substitutions) of hyp against ref
  m.def("edit_distance_counts", [](Arr<int32_t> ref, Arr<int32_t> hyp) {
    if (ref.ndim() != 1 || hyp.ndim() != 1) throw Error("edit_distance_counts: ref and hyp are flat sequences of word ids");
    const int64_t roff[2] = {0, (int64_t)ref.shape(0)}, hoff[2] = {0, (int64_t)hyp.shape(0)};
    const int32_t none = 0;
    Arr<int32_t> counts({(py::ssize_t)4});
    CApi(khg_edit_distance(1, ref.shape(0) ? ref.data() : &none, roff, hyp.shape(0) ? hyp.data() : &none, hoff, counts.mutable_data()));
    return counts;
  }, py::arg("ref"), py::arg("hyp"));

  // DeviceLm(lm, ctx=None): an NgramLm uploaded (khg_lm_create); the handle belongs to its context
  py::class_<PyDeviceLm, std::shared_ptr<PyDeviceLm>>(m, "DeviceLm")
      .def(py::init([](py::object lm, py::object ctx) {
        const BackoffLm b = LmOf(lm);
        auto d = std::make_shared<PyDeviceLm>();
        d->ctx_obj = ctx;
        d->ctx = ctx.is_none() ? DefaultCtx() : reinterpret_cast<khg_ctx*>(ctx.attr("h").cast<uintptr_t>());
        CApi(khg_lm_create(d->ctx, (int32_t)b.backoff.size(), b.backoff.data(), b.backoff_cost.data(), b.arc_begin.data(), b.word.data(), b.cost.data(),
                           b.next.data(), b.final_cost.data(), b.start, &d->h));
        return d;
      }), py::arg("lm"), py::arg("ctx") = py::none())
      .def_property_readonly("h", [](PyDeviceLm& d) { return reinterpret_cast<uintptr_t>(d.h); })
      .def_readonly("ctx", &PyDeviceLm::ctx_obj)
      .def_property_readonly("num_states", [](PyDeviceLm& d) {
        if (!d.h) throw Error("DeviceLm: closed");
        int32_t n = 0;
        CApi(khg_lm_num_states(d.h, &n));
        return (int)n;
      })
      .def_property_readonly("device_bytes", [](PyDeviceLm& d) {
        if (!d.h) throw Error("DeviceLm: closed");
        int64_t b = 0;
        CApi(khg_lm_device_bytes(d.h, &b));
        return b;
      })
      .def("close", &PyDeviceLm::close);

  // DevicePosteriors: the arc and per-frame transition-id posteriors of a batch of lattices, resident on the device
  auto post_sizes = [](PyDevicePosteriors& d) {
    if (!d.h) throw Error("DevicePosteriors: closed");
    const size_t U = d.status.size();
    std::vector<int64_t> fo(U + 1), eo(U + 1);
    CApi(khg_posteriors_sizes(d.h, fo.data(), eo.data()));
    return std::make_pair(fo, eo);
  };
  // the four flat arrays of a batch of Kaldi Posteriors (posterior.py: posts_to_arrays): checked for shape here, for content by
  // khg_posteriors_validate
  auto post_check = [](const Arr<int64_t>& fo, const Arr<int64_t>& eb, const Arr<int32_t>& tid, const Arr<double>& w) {
    if (fo.ndim() != 1 || eb.ndim() != 1 || tid.ndim() != 1 || w.ndim() != 1 || fo.shape(0) < 1 || tid.shape(0) != w.shape(0))
      throw Error("DevicePosteriors: frame_off [n_utt + 1], entry_begin [frames + 1], tid and weight [entries] are flat arrays");
    const py::ssize_t U = fo.shape(0) - 1;
    // (what sizes entry_begin must be right before khg_posteriors_validate reads it)
    for (py::ssize_t u = 0; u < U; ++u) if (fo.at(u + 1) < fo.at(u)) throw Error("khg_posteriors_validate: frame_off decreases at utterance " + std::to_string(u));
    if (fo.at(0) != 0 || eb.shape(0) != fo.at(U) + 1) throw Error("khg_posteriors_validate: frame_off starts at 0 and entry_begin has one element per frame plus one");
    CApi(khg_posteriors_validate((int32_t)U, fo.data(), eb.data(), (int64_t)tid.shape(0), tid.data(), w.data()));
  };
  m.def("posteriors_validate", post_check, py::arg("frame_off"), py::arg("entry_begin"), py::arg("tid"), py::arg("weight"));
  py::class_<PyDevicePosteriors, std::shared_ptr<PyDevicePosteriors>>(m, "DevicePosteriors")
      // a handle from host arrays (khg_posteriors_upload): no arc posteriors; an utterance without frames has status KHG_LAT_NO_PATH
      .def_static("from_arrays", [post_check](py::object ctx, Arr<int64_t> fo, Arr<int64_t> eb, Arr<int32_t> tid, Arr<double> w) {
        post_check(fo, eb, tid, w);
        const size_t U = (size_t)fo.shape(0) - 1;
        auto r = std::make_shared<PyDevicePosteriors>();
        r->ctx_obj = ctx;
        r->ctx = ctx.is_none() ? DefaultCtx() : reinterpret_cast<khg_ctx*>(ctx.attr("h").cast<uintptr_t>());
        r->arc_off.assign(U + 1, 0);
        r->status.resize(U); r->tot_like.assign(U, 0.0);
        for (size_t u = 0; u < U; ++u) r->status[u] = fo.at(u + 1) > fo.at(u) ? KHG_LAT_SUCCEEDED : KHG_LAT_NO_PATH;
        {
          py::gil_scoped_release nogil;
          CApi(khg_posteriors_upload(r->ctx, (int32_t)U, fo.data(), eb.data(), tid.data(), w.data(), &r->h));
        }
        return r;
      }, py::arg("ctx"), py::arg("frame_off"), py::arg("entry_begin"), py::arg("tid"), py::arg("weight"))
      // ali-to-post on the device (khg_posteriors_from_ali): one entry of weight 1 per frame of the set's resident alignment; an
      // utterance whose alignment failed has no frames (status KHG_LAT_NO_PATH)
      .def_static("from_alignment", [](py::object utts) {
        py::object ctx = utts.attr("ctx");
        auto r = std::make_shared<PyDevicePosteriors>();
        r->ctx_obj = ctx;
        r->ctx = reinterpret_cast<khg_ctx*>(ctx.attr("h").cast<uintptr_t>());
        khg_utts* uh = reinterpret_cast<khg_utts*>(utts.attr("h").cast<uintptr_t>());
        if (!uh) throw Error("DevicePosteriors.from_alignment: the UtteranceSet is closed");
        const size_t U = (size_t)utts.attr("n_utt").cast<int>();
        {
          py::gil_scoped_release nogil;
          CApi(khg_posteriors_from_ali(r->ctx, uh, &r->h));
        }
        std::vector<int64_t> fo(U + 1), eo(U + 1);
        CApi(khg_posteriors_sizes(r->h, fo.data(), eo.data()));
        r->arc_off.assign(U + 1, 0);
        r->status.resize(U); r->tot_like.assign(U, 0.0);
        for (size_t u = 0; u < U; ++u) r->status[u] = fo[u + 1] > fo[u] ? KHG_LAT_SUCCEEDED : KHG_LAT_NO_PATH;
        return r;
      }, py::arg("utts"))
      // ... from Kaldi's Posterior per utterance: posts[u][t] is a list of (tid, weight)
      .def_static("from_posteriors", [](py::object ctx, py::list posts) {
        py::object arrays = py::module_::import("kaldi_hmm_gmm_amd.posterior").attr("posts_to_arrays")(posts);
        return py::module_::import("kaldi_hmm_gmm_amd").attr("DevicePosteriors").attr("from_arrays")(ctx, *arrays);
      }, py::arg("ctx"), py::arg("posts"))
      .def_property_readonly("status", [](PyDevicePosteriors& d) { return Vec1(d.status); })
      .def_property_readonly("tot_like", [](PyDevicePosteriors& d) { return Vec1(d.tot_like); })
      // of the mpe_posteriors that made this handle (None otherwise): the expected frame accuracy of a path, per utterance
      .def_property_readonly("avg_acc", [](PyDevicePosteriors& d) -> py::object { if (!d.has_avg_acc) return py::none(); return Vec1(d.avg_acc); })
      .def_property_readonly("num_utts", [](PyDevicePosteriors& d) { return (int)d.status.size(); })
      .def_property_readonly("frame_off", [post_sizes](PyDevicePosteriors& d) { return Vec1(post_sizes(d).first); })
      .def_property_readonly("entry_off", [post_sizes](PyDevicePosteriors& d) { return Vec1(post_sizes(d).second); })
      .def_property_readonly("device_bytes", [](PyDevicePosteriors& d) {
        if (!d.h) throw Error("DevicePosteriors: closed");
        int64_t b = 0;
        CApi(khg_posteriors_device_bytes(d.h, &b));
        return b;
      })
      // per utterance a list over its frames of [(tid, weight), ...], ids ascending (no frames without KHG_LAT_SUCCEEDED)
      .def("download", [post_sizes](PyDevicePosteriors& d) {
        const auto sz = post_sizes(d);
        const size_t U = d.status.size();
        std::vector<int64_t> eb((size_t)sz.first.back() + 1, 0);
        std::vector<int32_t> tid((size_t)sz.second.back() + 1);
        std::vector<double> w((size_t)sz.second.back() + 1);
        {
          py::gil_scoped_release nogil;
          CApi(khg_posteriors_download(d.ctx, d.h, eb.data(), tid.data(), w.data(), nullptr));
        }
        py::list out;
        for (size_t u = 0; u < U; ++u) {
          py::list frames;
          for (int64_t f = sz.first[u]; f < sz.first[u + 1]; ++f) {
            py::list e;
            for (int64_t i = eb[(size_t)f]; i < eb[(size_t)f + 1]; ++i) e.append(py::make_tuple(tid[(size_t)i], w[(size_t)i]));
            frames.append(e);
          }
          out.append(frames);
        }
        return out;
      })
      // the flat arrays of download(): entry_begin [frames + 1], tid, weight [entries]
      .def("download_arrays", [post_sizes](PyDevicePosteriors& d) {
        const auto sz = post_sizes(d);
        std::vector<int64_t> eb((size_t)sz.first.back() + 1, 0);
        std::vector<int32_t> tid((size_t)sz.second.back() + 1);
        std::vector<double> w((size_t)sz.second.back() + 1);
        {
          py::gil_scoped_release nogil;
          CApi(khg_posteriors_download(d.ctx, d.h, eb.data(), tid.data(), w.data(), nullptr));
        }
        tid.pop_back(); w.pop_back();
        return py::make_tuple(Vec1(eb), Vec1(tid), Vec1(w));
      })
      // per utterance a float64 array over its arcs in the lattice's arc order (empty without KHG_LAT_SUCCEEDED)
      .def("arc_post", [](PyDevicePosteriors& d) {
        if (!d.h) throw Error("DevicePosteriors: closed");
        const size_t U = d.status.size();
        std::vector<double> ap((size_t)(d.arc_off.empty() ? 0 : d.arc_off.back()) + 1);
        {
          py::gil_scoped_release nogil;
          CApi(khg_posteriors_download(d.ctx, d.h, nullptr, nullptr, nullptr, ap.data()));
        }
        py::list out;
        for (size_t u = 0; u < U; ++u) {
          const bool ok = (d.status[u] & KHG_LAT_SUCCEEDED) != 0;
          const int64_t a0 = d.arc_off[u], a1 = ok ? d.arc_off[u + 1] : a0;
          Arr<double> a({(py::ssize_t)(a1 - a0)});
          if (a1 > a0) std::memcpy(a.mutable_data(), ap.data() + a0, sizeof(double) * (size_t)(a1 - a0));
          out.append(a);
        }
        return out;
      })
      .def("close", &PyDevicePosteriors::close);

  // get_raw_lattice_simple_device_batch(am, tm, fsts, feats_list, config, acoustic_scale, scratch_per_frame=0) -> (one dict per
  // utterance with decode_lattice_simple_batch's keys, DeviceLattices): get_raw_lattice_simple_batch that keeps the lattices on the device
  m.def("get_raw_lattice_simple_device_batch", [](std::shared_ptr<AmDiagGmm> am, std::shared_ptr<TransitionModel> tm, py::object fsts, py::list feats_list,
                                                  const LatticeSimpleDecoderConfig& config, float acoustic_scale, int scratch_per_frame) {
    BatchArgs b(*am, fsts, feats_list, "get_raw_lattice_simple_device_batch");
    std::vector<LatticeResult> rs;
    auto d = std::make_shared<PyDeviceLattices>();
    d->ctx = DefaultCtx();
    d->ctx_obj = py::none();
    {
      const GraphsCsr csr = b.Csr();
      py::gil_scoped_release nogil;
      rs = GetRawLatticeSimpleDeviceBatch(*am, *tm, csr, b.fp, b.nf, config, acoustic_scale, false, scratch_per_frame, &d->h);
    }
    py::list out;
    for (size_t u = 0; u < rs.size(); ++u) out.append(LatticeSimpleToDict(rs[u], b.nf[u], false));
    return py::make_tuple(out, d);
  }, py::arg("am"), py::arg("tm"), py::arg("fsts"), py::arg("feats_list"), py::arg("config"), py::arg("acoustic_scale"),
     py::arg("scratch_per_frame") = 0);

  // python/csrc/determinize-lattice-pruned.cc:13-25
  py::class_<DeterminizeLatticePhonePrunedOptions>(m, "DeterminizeLatticePhonePrunedOptions")
      .def(py::init([](float delta, int32_t max_mem, bool pd, bool wd, bool mn) {
             DeterminizeLatticePhonePrunedOptions o;
             o.delta = delta; o.max_mem = max_mem; o.phone_determinize = pd; o.word_determinize = wd; o.minimize = mn;
             return o;
           }), py::arg("delta") = 1.0f / 1024.0f, py::arg("max_mem") = 50000000, py::arg("phone_determinize") = true, py::arg("word_determinize") = true,
           py::arg("minimize") = false)
      .def_readwrite("delta", &DeterminizeLatticePhonePrunedOptions::delta).def_readwrite("max_mem", &DeterminizeLatticePhonePrunedOptions::max_mem)
      .def_readwrite("phone_determinize", &DeterminizeLatticePhonePrunedOptions::phone_determinize)
      .def_readwrite("word_determinize", &DeterminizeLatticePhonePrunedOptions::word_determinize)
      .def_readwrite("minimize", &DeterminizeLatticePhonePrunedOptions::minimize)
      .def("__str__", &DeterminizeLatticePhonePrunedOptions::ToString);

  // python/csrc/lattice-faster-decoder.cc:14-44
  using Cfg = LatticeFasterDecoderConfig;
  py::class_<Cfg>(m, "LatticeFasterDecoderConfig")
      .def(py::init([](float beam, int32_t max_active, int32_t min_active, float lattice_beam, int32_t prune_interval, bool determinize_lattice,
                       float beam_delta, float hash_ratio, float prune_scale, int32_t tb, int32_t lb, const DeterminizeLatticePhonePrunedOptions& det) {
             Cfg c;
             c.beam = beam; c.max_active = max_active; c.min_active = min_active;
             c.lattice_beam = lattice_beam; c.prune_interval = prune_interval; c.determinize_lattice = determinize_lattice; c.beam_delta = beam_delta;
             c.hash_ratio = hash_ratio; c.prune_scale = prune_scale; c.memory_pool_tokens_block_size = tb; c.memory_pool_links_block_size = lb;
             c.det_opts = det;
             return c;
           }), py::arg("beam") = 16.0f, py::arg("max_active") = std::numeric_limits<int32_t>::max(), py::arg("min_active") = 200,
           py::arg("lattice_beam") = 10.0f, py::arg("prune_interval") = 25, py::arg("determinize_lattice") = true, py::arg("beam_delta") = 0.5f,
           py::arg("hash_ratio") = 2.0f, py::arg("prune_scale") = 0.1f, py::arg("memory_pool_tokens_block_size") = 1 << 8,
           py::arg("memory_pool_links_block_size") = 1 << 8, py::arg("det_opts") = DeterminizeLatticePhonePrunedOptions{})
      .def_readwrite("beam", &Cfg::beam).def_readwrite("max_active", &Cfg::max_active).def_readwrite("min_active", &Cfg::min_active)
      .def_readwrite("lattice_beam", &Cfg::lattice_beam).def_readwrite("prune_interval", &Cfg::prune_interval)
      .def_readwrite("determinize_lattice", &Cfg::determinize_lattice).def_readwrite("beam_delta", &Cfg::beam_delta)
      .def_readwrite("hash_ratio", &Cfg::hash_ratio).def_readwrite("prune_scale", &Cfg::prune_scale)
      .def_readwrite("memory_pool_tokens_block_size", &Cfg::memory_pool_tokens_block_size)
      .def_readwrite("memory_pool_links_block_size", &Cfg::memory_pool_links_block_size)
      .def_readwrite("det_opts", &Cfg::det_opts)
      .def("__str__", &Cfg::ToString);

  // python/csrc/lattice-faster-decoder.cc:46-66 (the StdVectorFst instantiation is the same class here)
  py::class_<LatticeFasterDecoder>(m, "LatticeFasterDecoder")
      .def(py::init([](std::shared_ptr<StdVectorFst> fst, const Cfg& config) {
             if (!fst) throw Error("LatticeFasterDecoder: fst is None");
             config.Check();
             return LatticeFasterDecoder{std::move(fst), config};
           }), py::arg("fst"), py::arg("config"))
      .def_property_readonly("_config", [](const LatticeFasterDecoder& d) { return d.config; });
  m.attr("LatticeFasterDecoderStdVectorFst") = m.attr("LatticeFasterDecoder");

  // python/csrc/decoder-wrappers.cc:70-90 -> (succeeded, alignment, words, like)
  m.def("decode_utterance_lattice_faster", [](LatticeFasterDecoder& decoder, std::shared_ptr<DecodableInterface> decodable,
                                              const TransitionInformation& /*trans_model: the reference only passes it on*/,
                                              const std::string& utt, bool allow_partial) {
    if (!decodable) throw Error("decode_utterance_lattice_faster: decodable is None");
    LatticeResult r;
    if (auto dec = std::dynamic_pointer_cast<DecodableAmDiagGmmScaled>(decodable)) {
      py::gil_scoped_release nogil;
      r = DecodeLatticeBatch(*dec->am(), *dec->tm(), ConcatGraphs({decoder.fst.get()}), {dec->feats().data()}, {(int64_t)dec->NumFramesReady()},
                             decoder.config, dec->scale(), allow_partial, false)[0];
    } else {
      r = DecodeLatticeDecodable(*decoder.fst, *decodable, decoder.config, allow_partial);     // GIL held: the scores may come from Python
    }
    // what the reference stops on (KHG_ERR / KHG_ASSERT) raises here too
    if (r.status & KHG_LAT_EPS_LOOP) throw Error("Epsilon loops exist in your decoding graph (this is not allowed!)");
    if (r.status & KHG_LAT_NO_TRACEBACK) throw Error("Failed to get traceback for utterance " + utt);
    if (r.status & KHG_LAT_SCRATCH) throw Error("decode_utterance_lattice_faster: out of lattice scratch (queue / sort bound) for utterance " + utt);
    if (r.status & KHG_LAT_WORDS) throw Error("decode_utterance_lattice_faster: more words on the best path than the output holds for utterance " + utt);
    return py::make_tuple(r.succeeded, r.alignment, r.words, r.like);
  }, py::arg("decoder"), py::arg("decodable"), py::arg("trans_model"), py::arg("utt"), py::arg("allow_partial"));

  // the batched form: decode_lattice_faster_batch(am, tm, fsts, feats_list, config, acoustic_scale, allow_partial=True, return_scores=False)
  // -> one dict per utterance (succeeded, partial, status, alignment, words, like, num_frames[, loglikes, pdfs]); fsts may be one graph
  m.def("decode_lattice_faster_batch", [](std::shared_ptr<AmDiagGmm> am, std::shared_ptr<TransitionModel> tm, py::object fsts, py::list feats_list,
                                          const Cfg& config, float acoustic_scale, bool allow_partial, bool return_scores, int scratch_per_frame) {
    BatchArgs b(*am, fsts, feats_list, "decode_lattice_faster_batch");
    const std::vector<const float*>& fp = b.fp;
    const std::vector<int64_t>& nf = b.nf;
    std::vector<LatticeResult> rs;
    {
      const GraphsCsr csr = b.Csr();
      py::gil_scoped_release nogil;
      rs = DecodeLatticeBatch(*am, *tm, csr, fp, nf, config, acoustic_scale, allow_partial, return_scores, scratch_per_frame);
    }
    py::list out;
    for (size_t u = 0; u < rs.size(); ++u) out.append(LatticeToDict(rs[u], nf[u], return_scores));
    return out;
  }, py::arg("am"), py::arg("tm"), py::arg("fsts"), py::arg("feats_list"), py::arg("config"), py::arg("acoustic_scale"), py::arg("allow_partial") = true,
     py::arg("return_scores") = false, py::arg("scratch_per_frame") = 0);
  // get_raw_lattice_faster_batch(am, tm, fsts, feats_list, config, acoustic_scale, allow_partial=True, scratch_per_frame=0,
  // return_scores=False, return_times=False) -> decode_lattice_faster_batch's dicts plus "lattice" (a Lattice: GetRawLattice's, no states
  // unless the utterance succeeded).  return_times: (dicts, {"decode_s", "download_s"}).
  m.def("get_raw_lattice_faster_batch", [](std::shared_ptr<AmDiagGmm> am, std::shared_ptr<TransitionModel> tm, py::object fsts, py::list feats_list,
                                           const Cfg& config, float acoustic_scale, bool allow_partial, int scratch_per_frame, bool return_scores,
                                           bool return_times) -> py::object {
    BatchArgs b(*am, fsts, feats_list, "get_raw_lattice_faster_batch");
    std::vector<LatticeResult> rs;
    std::vector<std::shared_ptr<Lattice>> lats;
    double sec[2] = {0.0, 0.0};
    {
      const GraphsCsr csr = b.Csr();
      py::gil_scoped_release nogil;
      rs = GetRawLatticeFasterBatch(*am, *tm, csr, b.fp, b.nf, config, acoustic_scale, allow_partial, return_scores, scratch_per_frame, &lats, sec);
    }
    py::list out;
    for (size_t u = 0; u < rs.size(); ++u) {
      py::dict d = LatticeToDict(rs[u], b.nf[u], return_scores);
      d["lattice"] = lats[u];
      out.append(d);
    }
    if (!return_times) return std::move(out);
    py::dict t;
    t["decode_s"] = sec[0]; t["download_s"] = sec[1];
    return py::make_tuple(out, t);
  }, py::arg("am"), py::arg("tm"), py::arg("fsts"), py::arg("feats_list"), py::arg("config"), py::arg("acoustic_scale"), py::arg("allow_partial") = true,
     py::arg("scratch_per_frame") = 0, py::arg("return_scores") = false, py::arg("return_times") = false);

  // get_raw_lattice_faster_device_batch(...) -> (decode_lattice_faster_batch's dicts, DeviceLattices): the lattices stay on the device
  m.def("get_raw_lattice_faster_device_batch", [](std::shared_ptr<AmDiagGmm> am, std::shared_ptr<TransitionModel> tm, py::object fsts, py::list feats_list,
                                                  const Cfg& config, float acoustic_scale, bool allow_partial, int scratch_per_frame, bool return_scores) {
    BatchArgs b(*am, fsts, feats_list, "get_raw_lattice_faster_device_batch");
    std::vector<LatticeResult> rs;
    auto d = std::make_shared<PyDeviceLattices>();
    d->ctx = DefaultCtx();
    d->ctx_obj = py::none();
    {
      const GraphsCsr csr = b.Csr();
      py::gil_scoped_release nogil;
      rs = GetRawLatticeFasterDeviceBatch(*am, *tm, csr, b.fp, b.nf, config, acoustic_scale, allow_partial, return_scores, scratch_per_frame, &d->h);
    }
    py::list out;
    for (size_t u = 0; u < rs.size(); ++u) out.append(LatticeToDict(rs[u], b.nf[u], return_scores));
    return py::make_tuple(out, d);
  }, py::arg("am"), py::arg("tm"), py::arg("fsts"), py::arg("feats_list"), py::arg("config"), py::arg("acoustic_scale"), py::arg("allow_partial") = true,
     py::arg("scratch_per_frame") = 0, py::arg("return_scores") = false);

  // python/csrc/lattice-simple-decoder.cc:11-31
  using SCfg = LatticeSimpleDecoderConfig;
  py::class_<SCfg>(m, "LatticeSimpleDecoderConfig")
      .def(py::init([](float beam, float lattice_beam, int32_t prune_interval, bool determinize_lattice, float beam_ratio, float prune_scale,
                       const DeterminizeLatticePhonePrunedOptions& det) {
             SCfg c;
             c.beam = beam; c.lattice_beam = lattice_beam; c.prune_interval = prune_interval; c.determinize_lattice = determinize_lattice;
             c.beam_ratio = beam_ratio; c.prune_scale = prune_scale; c.det_opts = det;
             return c;
           }), py::arg("beam") = 16.0f, py::arg("lattice_beam") = 10.0f, py::arg("prune_interval") = 25, py::arg("determinize_lattice") = true,
           py::arg("beam_ratio") = 0.9f, py::arg("prune_scale") = 0.1f, py::arg("det_opts") = DeterminizeLatticePhonePrunedOptions{})
      .def_readwrite("beam", &SCfg::beam).def_readwrite("lattice_beam", &SCfg::lattice_beam).def_readwrite("prune_interval", &SCfg::prune_interval)
      .def_readwrite("determinize_lattice", &SCfg::determinize_lattice).def_readwrite("beam_ratio", &SCfg::beam_ratio)
      .def_readwrite("prune_scale", &SCfg::prune_scale).def_readwrite("det_opts", &SCfg::det_opts)
      .def("__str__", &SCfg::ToString);

  // python/csrc/lattice-simple-decoder.cc:33-37: the constructor runs config.Check() (lattice-simple-decoder.h:93-97)
  py::class_<LatticeSimpleDecoder>(m, "LatticeSimpleDecoder")
      .def(py::init([](std::shared_ptr<StdVectorFst> fst, const SCfg& config) {
             if (!fst) throw Error("LatticeSimpleDecoder: fst is None");
             config.Check();
             return LatticeSimpleDecoder{std::move(fst), config};
           }), py::arg("fst"), py::arg("config"))
      .def_property_readonly("_config", [](const LatticeSimpleDecoder& d) { return d.config; });

  // python/csrc/decoder-wrappers.cc:49-68 -> (succeeded, alignment, words, like)
  m.def("decode_utterance_lattice_simple", [](LatticeSimpleDecoder& decoder, std::shared_ptr<DecodableInterface> decodable,
                                              const TransitionInformation& /*trans_model: the reference only passes it on*/,
                                              const std::string& utt, bool allow_partial) {
    if (!decodable) throw Error("decode_utterance_lattice_simple: decodable is None");
    LatticeResult r;
    auto dec = std::dynamic_pointer_cast<DecodableAmDiagGmmScaled>(decodable);
    if (dec && dec->NumFramesReady() > 0) {
      decoder.config.Check();
      if (decoder.fst->Start() == kNoStateId) throw Error("Check failed!\nx: start_state != fst::kNoStateId");
      py::gil_scoped_release nogil;
      r = DecodeLatticeSimpleBatch(*dec->am(), *dec->tm(), ConcatGraphs({decoder.fst.get()}), {dec->feats().data()}, {(int64_t)dec->NumFramesReady()},
                                   decoder.config, dec->scale(), allow_partial, false)[0];
    } else {
      r = DecodeLatticeSimpleDecodable(*decoder.fst, *decodable, decoder.config, allow_partial);     // GIL held: the scores may come from Python
    }
    RaiseLatticeSimple(r, utt);
    return py::make_tuple(r.succeeded, r.alignment, r.words, r.like);
  }, py::arg("decoder"), py::arg("decodable"), py::arg("trans_model"), py::arg("utt"), py::arg("allow_partial"));

  // decode_lattice_simple_batch(am, tm, fsts, feats_list, config, acoustic_scale, allow_partial=True, return_scores=False,
  // scratch_per_frame=0) -> one dict per utterance, as decode_lattice_faster_batch's plus error_frame; nothing raises per utterance
  m.def("decode_lattice_simple_batch", [](std::shared_ptr<AmDiagGmm> am, std::shared_ptr<TransitionModel> tm, py::object fsts, py::list feats_list,
                                          const SCfg& config, float acoustic_scale, bool allow_partial, bool return_scores, int scratch_per_frame) {
    BatchArgs b(*am, fsts, feats_list, "decode_lattice_simple_batch");
    std::vector<LatticeResult> rs;
    {
      const GraphsCsr csr = b.Csr();
      py::gil_scoped_release nogil;
      rs = DecodeLatticeSimpleBatch(*am, *tm, csr, b.fp, b.nf, config, acoustic_scale, allow_partial, return_scores, scratch_per_frame);
    }
    py::list out;
    for (size_t u = 0; u < rs.size(); ++u) out.append(LatticeSimpleToDict(rs[u], b.nf[u], return_scores));
    return out;
  }, py::arg("am"), py::arg("tm"), py::arg("fsts"), py::arg("feats_list"), py::arg("config"), py::arg("acoustic_scale"), py::arg("allow_partial") = true,
     py::arg("return_scores") = false, py::arg("scratch_per_frame") = 0);
}

void BindAlign(py::module_& m) {
  py::class_<AlignConfig>(m, "AlignConfig")      // csrc/decoder-wrappers.h:23-37
      .def(py::init([](float beam, float retry_beam, bool careful) { AlignConfig c; c.beam = beam; c.retry_beam = retry_beam; c.careful = careful; return c; }),
           py::arg("beam") = 200.0f, py::arg("retry_beam") = 0.0f, py::arg("careful") = false)
      .def_readwrite("beam", &AlignConfig::beam).def_readwrite("retry_beam", &AlignConfig::retry_beam).def_readwrite("careful", &AlignConfig::careful)
      .def("__str__", [](const AlignConfig& c) {
        char b[128];
        std::snprintf(b, sizeof(b), "AlignConfig(beam=%g, retry_beam=%g, careful=%s)", (double)c.beam, (double)c.retry_beam, c.careful ? "True" : "False");
        return std::string(b);
      });

  py::class_<FasterDecoderOptions>(m, "FasterDecoderOptions")      // csrc/faster-decoder.h:24-63
      .def(py::init([](float beam, int64_t max_active, int min_active, float beam_delta, float hash_ratio) {
             FasterDecoderOptions o;
             o.beam = beam; o.max_active = (int32_t)std::min<int64_t>(max_active, std::numeric_limits<int32_t>::max()); o.min_active = min_active;
             o.beam_delta = beam_delta; o.hash_ratio = hash_ratio;
             return o;
           }), py::arg("beam") = 16.0f, py::arg("max_active") = (int64_t)std::numeric_limits<int32_t>::max(), py::arg("min_active") = 20, py::arg("beam_delta") = 0.5f,
           py::arg("hash_ratio") = 2.0f)
      .def_readwrite("beam", &FasterDecoderOptions::beam).def_readwrite("max_active", &FasterDecoderOptions::max_active)
      .def_readwrite("min_active", &FasterDecoderOptions::min_active).def_readwrite("beam_delta", &FasterDecoderOptions::beam_delta)
      .def_readwrite("hash_ratio", &FasterDecoderOptions::hash_ratio)
      .def("__str__", &FasterDecoderOptions::ToString);

  py::class_<DecodableInterface, PyDecodableInterface, std::shared_ptr<DecodableInterface>>(m, "DecodableInterface")
      .def(py::init<>())
      .def("log_likelihood", &DecodableInterface::LogLikelihood, py::arg("frame"), py::arg("index"))
      .def("is_last_frame", &DecodableInterface::IsLastFrame, py::arg("frame"))
      .def("num_frames_ready", &DecodableInterface::NumFramesReady)
      .def("num_indices", &DecodableInterface::NumIndices);

  py::class_<DecodableAmDiagGmmUnmapped, DecodableInterface, std::shared_ptr<DecodableAmDiagGmmUnmapped>>(m, "DecodableAmDiagGmmUnmapped")
      .def(py::init([](std::shared_ptr<AmDiagGmm> am, Arr<float> feats, float) {
             if (feats.ndim() != 2) throw Error("feats must be a 2-D float matrix");
             return std::make_shared<DecodableAmDiagGmmUnmapped>(std::move(am), feats.data(), (int64_t)feats.shape(0), (int)feats.shape(1));
           }), py::arg("am"), py::arg("feats"), py::arg("log_sum_exp_prune") = -1.0f)
      .def("log_likelihood", &DecodableAmDiagGmmUnmapped::LogLikelihood, py::arg("frame"), py::arg("index"))
      .def("_zero_based", &DecodableAmDiagGmmUnmapped::ZeroBased)
      .def("num_frames_ready", &DecodableAmDiagGmmUnmapped::NumFramesReady)
      .def("num_indices", &DecodableAmDiagGmmUnmapped::NumIndices)
      .def("is_last_frame", &DecodableAmDiagGmmUnmapped::IsLastFrame, py::arg("frame"))
      .def_property_readonly("_am", [](DecodableAmDiagGmmUnmapped& d) { return d.am(); })
      .def_property_readonly("_feats", [](DecodableAmDiagGmmUnmapped& d) {
        Arr<float> a({(py::ssize_t)d.NumFramesReady(), (py::ssize_t)d.Dim()});
        if (!d.feats().empty()) std::memcpy(a.mutable_data(), d.feats().data(), sizeof(float) * d.feats().size());
        return a;
      });

  py::class_<DecodableAmDiagGmmScaled, DecodableAmDiagGmmUnmapped, std::shared_ptr<DecodableAmDiagGmmScaled>>(m, "DecodableAmDiagGmmScaled")
      .def(py::init([](std::shared_ptr<AmDiagGmm> am, std::shared_ptr<TransitionModel> tm, Arr<float> feats, float scale, float) {
             if (feats.ndim() != 2) throw Error("feats must be a 2-D float matrix");
             return std::make_shared<DecodableAmDiagGmmScaled>(std::move(am), std::move(tm), feats.data(), (int64_t)feats.shape(0), (int)feats.shape(1), scale);
           }), py::arg("am"), py::arg("tm"), py::arg("feats"), py::arg("scale"), py::arg("log_sum_exp_prune") = -1.0f)
      .def_property_readonly("transition_model", [](DecodableAmDiagGmmScaled& d) { return d.tm(); })
      .def_property_readonly("_tm", [](DecodableAmDiagGmmScaled& d) { return d.tm(); })
      .def_property_readonly("_scale", [](DecodableAmDiagGmmScaled& d) { return (double)d.scale(); });

  // python/csrc/decodable-ctc.cc:11-15
  py::class_<DecodableCtc, DecodableInterface, std::shared_ptr<DecodableCtc>>(m, "DecodableCtc")
      .def(py::init([](Arr<float> feats) {
             if (feats.ndim() != 2) throw Error("feats must be a 2-D float matrix");
             return std::make_shared<DecodableCtc>(feats.data(), (int64_t)feats.shape(0), (int64_t)feats.shape(1));
           }), py::arg("feats"));

  py::class_<PyDecodingGraph>(m, "DecodingGraph")
      .def(py::init<std::shared_ptr<StdVectorFst>, py::object, py::object>(), py::arg("fst"), py::arg("tm"), py::arg("ctx") = py::none())
      .def_property_readonly("h", [](PyDecodingGraph& g) { return reinterpret_cast<uintptr_t>(g.h); })
      .def_readonly("ctx", &PyDecodingGraph::keep_ctx)
      .def_readonly("num_states", &PyDecodingGraph::num_states).def_readonly("num_arcs", &PyDecodingGraph::num_arcs)
      .def_readonly("num_pdfs", &PyDecodingGraph::num_pdfs).def_readonly("max_in_degree", &PyDecodingGraph::max_in_degree)
      .def_readonly("device_bytes", &PyDecodingGraph::device_bytes)
      .def("close", &PyDecodingGraph::close);

  m.def("align_batch", &AlignBatchPy, py::arg("am"), py::arg("tm"), py::arg("fsts"), py::arg("feats_list"), py::arg("config"), py::arg("acoustic_scale"),
        py::arg("trans_cost") = py::none(), py::arg("decoder_opts") = py::none(), py::arg("return_scores") = false);

  // python/csrc/decoder-wrappers.cc:25-47 -> (num_done, num_error, num_retried, tot_like, frame_count, alignment, words); the counters
  // are passed by value and returned incremented
  // `decodable` is any DecodableInterface, as in the reference: a DecodableAmDiagGmmScaled runs K1 + K2 (scores scaled by the
  // decodable's own scale, `like` divided by acoustic_scale, decoder-wrappers.cc:95); anything else -- the unmapped GMM decodable, a
  // Python subclass of DecodableInterface -- has its scores sampled through log_likelihood(frame, index) and decoded by K2.
  m.def("align_utterance_wrapper", [](py::object config, const std::string&, float acoustic_scale, std::shared_ptr<StdVectorFst> fst,
                                      std::shared_ptr<DecodableInterface> decodable, int num_done, int num_error, int num_retried, double tot_like,
                                      int64_t frame_count) {
    if (!fst) throw Error("align_utterance_wrapper: fst is None");
    if (!decodable) throw Error("align_utterance_wrapper: decodable is None");
    AlignConfig cfg = ConfigFrom(config);
    CheckBeams(cfg);
    if (fst->Start() == kNoStateId)                   // "Empty decoding graph" (decoder-wrappers.cc:35-41)
      return py::tuple(py::make_tuple(num_done, num_error + 1, num_retried, tot_like, frame_count, py::list(), py::list()));
    if (cfg.careful) {
      ModifyGraphForCarefulAlignment(fst.get());      // the reference mutates the caller's fst (decoder-wrappers.cc:43-45)
      cfg.careful = false;
    }
    AlignResult r;
    if (auto dec = std::dynamic_pointer_cast<DecodableAmDiagGmmScaled>(decodable)) {
      py::gil_scoped_release nogil;
      r = AlignBatch(*dec->am(), *dec->tm(), ConcatGraphs({fst.get()}), {dec->feats().data()}, {(int64_t)dec->NumFramesReady()}, cfg, dec->scale(), nullptr,
                     nullptr, false, acoustic_scale)[0];
    } else {
      r = AlignDecodable(*fst, *decodable, cfg, acoustic_scale, nullptr);       // GIL held: the scores may come from Python
    }
    if (r.retried) num_retried += 1;
    if (!r.ok) return py::tuple(py::make_tuple(num_done, num_error + 1, num_retried, tot_like, frame_count, py::list(), py::list()));
    return py::tuple(py::make_tuple(num_done + 1, num_error, num_retried, tot_like + (double)r.like, frame_count + (int64_t)r.num_frames, py::cast(r.alignment),
                                    py::cast(r.words)));
  }, py::arg("config"), py::arg("utt"), py::arg("acoustic_scale"), py::arg("fst"), py::arg("decodable"), py::arg("num_done"), py::arg("num_error"),
     py::arg("num_retried"), py::arg("tot_like"), py::arg("frame_count"));

  // ---- the graph container (kaldifst's method names) -----------------------------------------------------------------------------
  m.attr("kNoStateId") = kNoStateId;
  py::class_<StdArc>(m, "StdArc")
      .def(py::init([](int il, int ol, double w, int ns) { return StdArc{il, ol, (float)w, ns}; }), py::arg("ilabel"), py::arg("olabel"), py::arg("weight"),
           py::arg("nextstate"))
      .def_readwrite("ilabel", &StdArc::ilabel).def_readwrite("olabel", &StdArc::olabel).def_readwrite("nextstate", &StdArc::nextstate)
      .def_property("weight", [](const StdArc& a) { return (double)a.weight; }, [](StdArc& a, double w) { a.weight = (float)w; })
      .def("__repr__", &StdArc::ToString);

  py::class_<StdVectorFst, std::shared_ptr<StdVectorFst>>(m, "StdVectorFst")
      .def(py::init<>())
      .def("add_state", &StdVectorFst::AddState)
      .def_property_readonly("num_states", &StdVectorFst::NumStates)
      .def_property("start", &StdVectorFst::Start, &StdVectorFst::SetStart)
      .def("set_start", &StdVectorFst::SetStart)
      .def("add_arc", [](StdVectorFst& f, int state, py::object arc, py::kwargs kw) {
        if (!arc.is_none()) { f.AddArc(state, arc.cast<StdArc>()); return; }
        f.AddArc(state, StdArc{kw["ilabel"].cast<int>(), kw["olabel"].cast<int>(), kw.contains("weight") ? (float)kw["weight"].cast<double>() : 0.0f,
                               kw["nextstate"].cast<int>()});
      }, py::arg("state"), py::arg("arc") = py::none())
      .def("set_final", [](StdVectorFst& f, int s, double w) { f.SetFinal(s, (float)w); }, py::arg("state"), py::arg("weight") = 0.0)
      .def("final", [](StdVectorFst& f, int s) { return (double)f.Final(s); }, py::arg("state"))
      .def("is_final", &StdVectorFst::IsFinal, py::arg("state"))
      .def("arcs", [](StdVectorFst& f, int s) { return f.Arcs(s); }, py::arg("state"))       // copies: the container owns its arcs
      .def("num_arcs", [](StdVectorFst& f, py::object s) { return s.is_none() ? f.NumArcs() : (int64_t)f.Arcs(s.cast<int>()).size(); }, py::arg("state") = py::none())
      .def("copy", [](StdVectorFst& f) { return std::make_shared<StdVectorFst>(f); })
      .def_property_readonly("_arcs", [](StdVectorFst& f) { return f.arcs(); })
      .def_property_readonly("_final", [](StdVectorFst& f) { return std::vector<double>(f.finals().begin(), f.finals().end()); })
      .def_property_readonly("_start", &StdVectorFst::Start)
      .def("to_csr", [](StdVectorFst& f) {
        const GraphsCsr c = ConcatGraphs({&f});
        py::dict d;
        d["start"] = f.Start(); d["arc_off"] = Vec1(c.arc_off); d["ilabel"] = Vec1(c.ilabel); d["olabel"] = Vec1(c.olabel); d["weight"] = Vec1(c.weight);
        d["nextstate"] = Vec1(c.nextstate); d["final"] = Vec1(c.final_w);
        return d;
      })
      .def_static("from_csr", [](int start, Arr<int64_t> arc_off, Arr<int32_t> il, Arr<int32_t> ol, Arr<float> w, Arr<int32_t> ns, Arr<float> fin) {
        auto f = std::make_shared<StdVectorFst>();
        for (py::ssize_t s = 0; s < fin.size(); ++s) {
          f->AddState();
          f->SetFinal((int)s, fin.at(s));
          for (int64_t a = arc_off.at(s); a < arc_off.at(s + 1); ++a) f->AddArc((int)s, StdArc{il.at(a), ol.at(a), w.at(a), ns.at(a)});
        }
        f->SetStart(start);
        return f;
      }, py::arg("start"), py::arg("arc_off"), py::arg("ilabel"), py::arg("olabel"), py::arg("weight"), py::arg("nextstate"), py::arg("final"));

  m.def("concat_graphs", [](std::vector<std::shared_ptr<StdVectorFst>> fsts) {
    std::vector<const StdVectorFst*> p;
    for (auto& f : fsts) p.push_back(f.get());
    return CsrToDict(ConcatGraphs(p));
  }, py::arg("fsts"));
  m.def("modify_graph_for_careful_alignment", [](StdVectorFst& f) { ModifyGraphForCarefulAlignment(&f); }, py::arg("fst"));
  // python/csrc/hmm-utils.cc:14-19: disambig_syms defaults to empty; the rest are required
  // (pybind11 lets a defaulted argument precede required ones, as the reference's binding does)
  m.def("add_transition_probs", [](const TransitionModel& tm, std::vector<int> disambig, float ts, float sl, std::shared_ptr<StdVectorFst> fst) {
    if (!fst) throw Error("add_transition_probs: fst is None");
    AddTransitionProbs(tm, disambig, ts, sl, fst.get());
  }, py::arg("trans_model"), py::arg("disambig_syms") = std::vector<int>(), py::arg("transition_scale"), py::arg("self_loop_scale"), py::arg("fst"));

  py::class_<LatticeWeight>(m, "LatticeWeight")
      .def(py::init([](double a, double b) { return LatticeWeight{a, b}; }), py::arg("value1") = 0.0, py::arg("value2") = 0.0)
      .def_readwrite("value1", &LatticeWeight::value1).def_readwrite("value2", &LatticeWeight::value2)
      .def("__repr__", [](const LatticeWeight& w) {
        return "LatticeWeight(" + py::repr(py::float_(w.value1)).cast<std::string>() + ", " + py::repr(py::float_(w.value2)).cast<std::string>() + ")";
      });
  py::class_<LatticeArc>(m, "LatticeArc")
      .def(py::init([](int il, int ol, LatticeWeight w, int ns) { return LatticeArc{il, ol, w, ns}; }), py::arg("ilabel"), py::arg("olabel"), py::arg("weight"),
           py::arg("nextstate"))
      .def_readwrite("ilabel", &LatticeArc::ilabel).def_readwrite("olabel", &LatticeArc::olabel).def_readwrite("weight", &LatticeArc::weight)
      .def_readwrite("nextstate", &LatticeArc::nextstate);
  py::class_<LinearLattice>(m, "LinearLattice")
      .def(py::init<>())
      .def_readwrite("arcs", &LinearLattice::arcs).def_readwrite("final", &LinearLattice::final_w).def_readwrite("start", &LinearLattice::start)
      .def_property_readonly("num_states", &LinearLattice::NumStates)
      .def("get_linear_symbol_sequence", [](const LinearLattice& l) {
        std::vector<int> il, ol;
        LatticeWeight w;
        const bool ok = l.GetLinearSymbolSequence(&il, &ol, &w);
        return py::make_tuple(ok, il, ol, w);
      });

  py::class_<FasterDecoder>(m, "FasterDecoder")      // python/csrc/faster-decoder.cc:33-53 (the method is spelled advanced_decoding there)
      .def(py::init<std::shared_ptr<StdVectorFst>, const FasterDecoderOptions&>(), py::arg("fst"), py::arg("config"))
      .def("set_options", &FasterDecoder::SetOptions, py::arg("config"))
      .def("init_decoding", &FasterDecoder::InitDecoding)
      .def("decode", [](FasterDecoder& d, std::shared_ptr<DecodableInterface> dec) { d.Decode(dec); }, py::arg("decodable"))
      .def("advanced_decoding", [](FasterDecoder& d, std::shared_ptr<DecodableInterface> dec, int max_num_frames) { d.AdvanceDecoding(dec, max_num_frames); },
           py::arg("decodable"), py::arg("max_num_frames") = -1)
      .def("num_frames_decoded", &FasterDecoder::NumFramesDecoded)
      .def("reached_final", &FasterDecoder::ReachedFinal)
      .def("get_best_path", [](FasterDecoder& d, bool use_final_probs) {
        LinearLattice lat;
        const bool ok = d.GetBestPath(&lat, use_final_probs);
        return py::make_tuple(ok, lat);
      }, py::arg("use_final_probs") = true);
}
