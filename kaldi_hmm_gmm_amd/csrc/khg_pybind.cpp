// kaldi_hmm_gmm_amd/csrc/khg_pybind.cpp -- the pybind11 host surface over the C-ABI (include/khg_hip.h).
//
// The reference's host boundary is ONE pybind11 module, `_kaldi_hmm_gmm` (python/csrc/kaldi-hmm-gmm.cc:35-69), whose
// classes wrap Eigen-backed C++ objects.  This module, `_kaldi_hmm_gmm_amd`, is its counterpart for the accelerated
// path: C++ classes that own the C-ABI handles (device model, transition tables, resident utterance sets, accumulator
// block, RCCL communicator) and take / return numpy arrays, plus the host-side functions of the M-step, plus (BindHost,
// khg_py_host.cpp / khg_py_hmm.cpp / khg_py_align.cpp) the C++ host classes behind the reference's names: DiagGmm, AmDiagGmm,
// AccumDiagGmm, AccumAmDiagGmm, HmmTopology, TransitionModel, AlignConfig, DecodableAmDiagGmmScaled, align_utterance_wrapper ...
// kaldi_hmm_gmm_amd/*.py re-export them.
// Errors: a non-zero C-ABI status becomes a Python RuntimeError subclass (KhgError), as KHG_ERR does in the reference
// (csrc/log.h:46-53 -> std::runtime_error -> RuntimeError).
#include <chrono>

#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/khg_hip.h"
#include "khg_py_ebw.hpp"
#include "khg_py_lattices.hpp"

namespace py = pybind11;

namespace {

py::object g_khg_error;   // kaldi_hmm_gmm_amd._lib.KhgError (set at import)

void Check(int rc) {
  if (rc == KHG_OK) return;
  const char* msg = khg_last_error();
  if (g_khg_error && !g_khg_error.is_none()) {
    PyErr_SetString(g_khg_error.ptr(), msg ? msg : "khg error");
    throw py::error_already_set();
  }
  throw std::runtime_error(msg ? msg : "khg error");
}

// The C-ABI calls that launch kernels, wait for the stream or copy between host and device run WITHOUT the GIL (two contexts on
// two streams driven from two Python threads is a supported mode); Check() needs it back: it may raise.
template <class F>
int NoGil(F&& f) {
  py::gil_scoped_release release;
  return f();
}

template <class T>
using Arr = py::array_t<T, py::array::c_style | py::array::forcecast>;

template <class T>
Arr<T> Zeros(std::vector<py::ssize_t> shape) {
  Arr<T> a(shape);
  std::memset(a.mutable_data(), 0, sizeof(T) * (size_t)a.size());
  return a;
}

struct KContext {
  khg_ctx* h = nullptr;
  int device = 0;
  KContext(int dev, py::object stream) : device(dev) {
    void* st = stream.is_none() ? nullptr : reinterpret_cast<void*>(stream.cast<uintptr_t>());
    Check(khg_ctx_create(dev, st, &h));
  }
  ~KContext() { close(); }
  void close() { if (h) { khg_ctx_destroy(h); h = nullptr; } }
  void sync() { Check(NoGil([&] { return khg_ctx_sync(h); })); }
  void set_timing(bool on) { Check(khg_ctx_set_timing(h, on ? 1 : 0)); }
  void set_k1_form(const std::string& f) {
    int v = f == "auto" ? KHG_K1_AUTO : (f == "pdf" || f == "fp32") ? KHG_K1_FP32_PDF : f == "utt" ? KHG_K1_FP32_UTT : f == "f16x2" ? KHG_K1_F16X2 : f == "f16x2s" ? KHG_K1_F16X2S : -1;
    if (v < 0) throw py::key_error(f);
    Check(khg_ctx_set_k1_form(h, v));
  }
  // khg_ctx_set_option by name ("k3_form", ...) or by number; -> the previous value
  static int opt_id(const py::object& o) {
    if (py::isinstance<py::int_>(o)) return o.cast<int>();
    static const char* names[KHG_OPT_COUNT] = {"k1_form", "k1_order", "k1_nf", "k1p_ts", "k1_interleave", "k1_dbg", "k2_inorder", "k2_ks", "k2_serial",
                                               "k2_prof", "k3_bucket", "k3_form", "k3_phase_b", "k3_ny", "debug", "k3_phase_a", "k2_split", "k2s_hub", "lat_ops_lds", "k1_launch", "k1_pgrid", "k1_prof", "k2_ladder", "k3_planes", "k2_tail", "nbest_arena"};
    const std::string n = o.cast<std::string>();
    for (int i = 0; i < KHG_OPT_COUNT; ++i) if (n == names[i]) return i;
    if (n == "scratch_bytes") return KHG_INFO_SCRATCH_BYTES;       // read-only
    if (n == "scratch_blocks") return KHG_INFO_SCRATCH_BLOCKS;
    throw py::key_error(n);
  }
  int get_option(py::object name) { int v = 0; Check(khg_ctx_get_option(h, opt_id(name), &v)); return v; }
  int set_option(py::object name, int value) {
    const int id = opt_id(name);
    int old = 0;
    Check(khg_ctx_get_option(h, id, &old));
    Check(khg_ctx_set_option(h, id, value));
    return old;
  }
  py::list timings() {
    const int cap = 4096;
    std::vector<char> names(1 << 16);
    std::vector<float> ms(cap);
    int32_t n = 0;
    Check(khg_ctx_get_timings(h, names.data(), (int64_t)names.size(), ms.data(), cap, &n));
    py::list out;
    const char* p = names.data();
    for (int i = 0; i < n && i < cap; ++i) {
      const char* e = std::strchr(p, '\n');
      std::string nm = e ? std::string(p, e) : std::string(p);
      out.append(py::make_tuple(nm, ms[i]));
      if (!e) break;
      p = e + 1;
    }
    return out;
  }
};

struct KComm {
  void* h = nullptr;
  int nranks = 1, rank = 0;
  static py::bytes unique_id() {
    char id[KHG_COMM_ID_BYTES];
    Check(khg_comm_unique_id(id));
    return py::bytes(id, KHG_COMM_ID_BYTES);
  }
  KComm(KContext& ctx, int n, int r, py::bytes uid) : nranks(n), rank(r) {
    std::string s = uid;
    if (s.size() != KHG_COMM_ID_BYTES) throw py::value_error("Comm: the id is 128 bytes");
    Check(NoGil([&] { return khg_comm_create(ctx.h, n, r, s.data(), &h); }));      // collective: blocks until every rank has called it
  }
  py::dict info() {          // what RCCL itself reports: ncclCommCount / ncclCommUserRank / ncclGetVersion
    int32_t n = 0, r = -1, v = 0;
    Check(khg_comm_info(h, &n, &r, &v));
    py::dict d;
    d["nranks"] = n; d["rank"] = r; d["version"] = v;
    return d;
  }
  ~KComm() { close(); }
  void close() { if (h) { khg_comm_destroy(h); h = nullptr; } }
};

struct KAccs;

struct KModel {
  khg_model* h = nullptr;
  py::object ctx_obj;
  KContext* ctx;
  int num_pdfs = 0, dim = 0;
  Arr<int32_t> gauss_off;
  KModel(py::object ctx_o, Arr<int32_t> go, Arr<float> gc, Arr<float> miv, Arr<float> iv, py::object weights)
      : ctx_obj(ctx_o), ctx(ctx_o.cast<KContext*>()), gauss_off(go) {
    num_pdfs = (int)go.shape(0) - 1;
    if (miv.ndim() != 2 || iv.ndim() != 2 || miv.shape(0) != iv.shape(0) || miv.shape(1) != iv.shape(1) || num_pdfs < 1 ||
        miv.shape(0) != go.at(num_pdfs) || gc.shape(0) != miv.shape(0))
      throw py::value_error("DeviceModel: inconsistent shapes");
    dim = (int)miv.shape(1);
    Check(khg_model_create(ctx->h, num_pdfs, dim, go.data(), gc.data(), miv.data(), iv.data(), &h));
    if (!weights.is_none()) set_weights(weights.cast<Arr<float>>());
  }
  ~KModel() { close(); }
  void close() { if (h) { khg_model_destroy(h); h = nullptr; } }
  int64_t sumG() const { return gauss_off.at(num_pdfs); }
  void set_weights(Arr<float> w) {
    if (w.shape(0) != sumG()) throw py::value_error("set_weights: one weight per Gaussian");
    Check(khg_model_set_weights(ctx->h, h, w.data()));
  }
  py::dict mle_update(KAccs& accs, py::object opts, int flags);
  py::dict mle_result(float oc, float cnt, int32_t fe, int32_t fg, int32_t rm);
  py::dict mle_update_sharded(KAccs& accs, py::object opts, int flags, py::object comm);
  void mle_update_range(KAccs& accs, py::object opts, int flags, int first_pdf, int n_pdf);
  py::dict mle_rows_download(int first_pdf, int n_pdf);
  void mle_rows_upload(py::dict d);
  py::dict mle_update_finish();
  py::dict ebw_update(KAccs& num_accs, KAccs& den_accs, py::object opts, py::object weight_opts, int flags);
  void invalidate() { Check(khg_model_invalidate(h)); }
  // gmm-transform-means on the handle (khg_model_transform_means): M [dim, dim]
  void transform_means(Arr<float> M) {
    if (M.ndim() != 2 || M.shape(0) != dim || M.shape(1) != dim) throw py::value_error("transform_means: M must be [dim, dim]");
    Check(NoGil([&] { return khg_model_transform_means(ctx->h, h, M.data()); }));
  }
  void scale_weights(Arr<int32_t> pdfs, float scale) { Check(khg_model_scale_weights(ctx->h, h, (int32_t)pdfs.shape(0), pdfs.data(), scale)); }
  void split(Arr<int32_t> targets, float perturb, py::object randn) {
    if (targets.shape(0) != num_pdfs) throw py::value_error("split: one target per pdf");
    Arr<float> r;
    const float* rp = nullptr;
    int64_t nr = 0;
    if (!randn.is_none()) { r = randn.cast<Arr<float>>(); rp = r.data(); nr = (int64_t)r.size(); }
    Check(NoGil([&] { return khg_model_split(ctx->h, h, targets.data(), perturb, rp, nr); }));
    Arr<int32_t> go({(py::ssize_t)num_pdfs + 1});
    Check(khg_model_num_gauss(h, nullptr, go.mutable_data()));
    gauss_off = go;
  }
  void merge(Arr<int32_t> targets) {
    if (targets.shape(0) != num_pdfs) throw py::value_error("merge: one target per pdf");
    Check(NoGil([&] { return khg_model_merge(ctx->h, h, targets.data()); }));
    Arr<int32_t> go({(py::ssize_t)num_pdfs + 1});
    Check(khg_model_num_gauss(h, nullptr, go.mutable_data()));
    gauss_off = go;
  }
  py::dict download(bool weights) {
    const py::ssize_t G = sumG();
    Arr<float> gc({G}), miv({G, (py::ssize_t)dim}), iv({G, (py::ssize_t)dim});
    py::object w = py::none();
    float* wp = nullptr;
    Arr<float> wa;
    if (weights) { wa = Arr<float>({G}); wp = wa.mutable_data(); w = wa; }
    Check(NoGil([&] { return khg_model_download(ctx->h, h, wp, gc.mutable_data(), miv.mutable_data(), iv.mutable_data()); }));
    py::dict d;
    d["gauss_off"] = py::array(gauss_off).attr("copy")();
    d["weights"] = w; d["gconsts"] = gc; d["means_invvars"] = miv; d["inv_vars"] = iv;
    return d;
  }
};

struct KTransitions {
  khg_tm* h = nullptr;
  py::object ctx_obj;
  Arr<int32_t> id2pdf;
  int num_tids = 0;
  KTransitions(py::object ctx_o, Arr<int32_t> i2p) : ctx_obj(ctx_o), id2pdf(i2p) {
    num_tids = (int)i2p.shape(0) - 1;
    Check(khg_tm_create(ctx_o.cast<KContext*>()->h, num_tids, i2p.data(), &h));
  }
  ~KTransitions() { close(); }
  void close() { if (h) { khg_tm_destroy(h); h = nullptr; } }
  void set_trans_cost(py::object cost) {
    if (cost.is_none()) { Check(khg_tm_set_trans_cost(h, nullptr)); return; }
    Arr<float> c = cost.cast<Arr<float>>();
    if (c.shape(0) != num_tids + 1) throw py::value_error("set_trans_cost: num_tids + 1 entries");
    Check(khg_tm_set_trans_cost(h, c.data()));
  }
};

struct KAccs {
  khg_accs* h = nullptr;
  py::object ctx_obj;
  KContext* ctx;
  int64_t sumG = 0, size = 0;
  int dim = 0, num_tids = 0;
  KAccs(py::object ctx_o, KModel& m, KTransitions& tm) : ctx_obj(ctx_o), ctx(ctx_o.cast<KContext*>()) {
    sumG = m.sumG(); dim = m.dim; num_tids = tm.num_tids;
    Check(khg_accs_create(ctx->h, m.h, tm.h, &h));
    Check(khg_accs_size(h, &size));
  }
  ~KAccs() { close(); }
  void close() { if (h) { khg_accs_destroy(h); h = nullptr; } }
  void zero() { Check(khg_accs_zero(ctx->h, h)); }
  uintptr_t device_ptr() { void* p = nullptr; Check(khg_accs_device_ptr(h, &p)); return reinterpret_cast<uintptr_t>(p); }
  void allreduce_range(KModel& m, int first_pdf, int n_pdf, py::object comm) {
    void* c = comm.is_none() ? nullptr : comm.cast<KComm*>()->h;
    Check(NoGil([&] { return khg_accs_allreduce_range(ctx->h, h, m.h, first_pdf, n_pdf, c); }));
  }
  void allreduce(py::object comm, bool wire_fp32) {
    void* c = comm.is_none() ? nullptr : comm.cast<KComm*>()->h;
    Check(NoGil([&] { return wire_fp32 ? khg_accs_allreduce_f32(ctx->h, h, c) : khg_accs_allreduce(ctx->h, h, c); }));
  }
  py::dict split(Arr<double> buf) {
    const int64_t G = sumG, D = dim, nt = num_tids;
    if (buf.size() < G * (1 + 2 * D) + nt + 1 + 8) throw py::value_error("split: buffer too small");
    py::array base = buf;
    auto sl = [&](int64_t first, std::vector<py::ssize_t> shape) {
      std::vector<py::ssize_t> strides(shape.size());
      py::ssize_t st = sizeof(double);
      for (int i = (int)shape.size() - 1; i >= 0; --i) { strides[i] = st; st *= shape[i]; }
      return py::array(py::dtype::of<double>(), shape, strides, buf.data() + first, base);   // a view, like the ctypes twin
    };
    py::dict d;
    int64_t o = 0;
    d["occ"] = sl(o, {G}); o += G;
    d["mean_acc"] = sl(o, {G, D}); o += G * D;
    d["var_acc"] = sl(o, {G, D}); o += G * D;
    d["trans_acc"] = sl(o, {nt + 1}); o += nt + 1;
    d["total_frames"] = buf.data()[o];
    d["total_log_like"] = buf.data()[o + 1];
    return d;
  }
  void relayout(KModel& m) {
    Check(khg_accs_relayout(ctx->h, h, m.h));
    sumG = m.sumG();
    Check(khg_accs_size(h, &size));
  }
  Arr<double> download_range(int64_t first, int64_t count) {
    Arr<double> out({(py::ssize_t)count});
    Check(NoGil([&] { return khg_accs_download_range(ctx->h, h, first, count, out.mutable_data()); }));
    return out;
  }
  py::dict download_trans() {
    Arr<double> tr({(py::ssize_t)num_tids + 1});
    double sc[8];
    Check(NoGil([&] { return khg_accs_download_trans(ctx->h, h, tr.mutable_data(), sc); }));
    py::dict d;
    d["trans_acc"] = tr; d["total_frames"] = sc[0]; d["total_log_like"] = sc[1];
    return d;
  }
  py::dict download() {
    Arr<double> buf({(py::ssize_t)size});
    Check(NoGil([&] { return khg_accs_download(ctx->h, h, buf.mutable_data()); }));
    return split(buf);
  }
  void upload(Arr<double> b) {
    if (b.size() != size) throw py::value_error("upload: wrong block size");
    Check(NoGil([&] { return khg_accs_upload(ctx->h, h, b.data()); }));
  }
  // gmm-sum-accs / gmm-ismooth-stats on the resident block (khg_accs_add / _scale / _smooth_with_accum)
  void add(float scale, KAccs& src) { Check(khg_accs_add(ctx->h, h, scale, src.h)); }
  void scale(float f) { Check(khg_accs_scale(ctx->h, h, f)); }
  py::object smooth_with_accum(float tau, KAccs& src, KModel& m, bool count) {
    int32_t n = 0;
    Check(NoGil([&] { return khg_accs_smooth_with_accum(ctx->h, h, tau, src.h, m.h, count ? &n : nullptr); }));
    return count ? py::object(py::int_(n)) : py::object(py::none());
  }
};

static void ParseMleOptions(py::object opts, int dim, khg_mle_options& o, Arr<double>& vfv) {
  khg_mle_options_default(&o);
  if (!opts.is_none()) {
    o.min_gaussian_weight = opts.attr("min_gaussian_weight").cast<float>();
    o.min_gaussian_occupancy = opts.attr("min_gaussian_occupancy").cast<float>();
    o.min_variance = opts.attr("min_variance").cast<double>();
    o.remove_low_count_gaussians = opts.attr("remove_low_count_gaussians").cast<bool>() ? 1 : 0;
    if (py::hasattr(opts, "variance_floor_vector") && !opts.attr("variance_floor_vector").is_none()) {
      vfv = opts.attr("variance_floor_vector").cast<Arr<double>>();
      if (vfv.size() > 0) {
        if (vfv.size() != dim) throw py::value_error("variance_floor_vector: one floor per dimension");
        o.variance_floor_vector = vfv.data();
      }
    }
  }
}
py::dict KModel::mle_result(float oc, float cnt, int32_t fe, int32_t fg, int32_t rm) {
  if (rm) {
    Arr<int32_t> go({(py::ssize_t)num_pdfs + 1});
    Check(khg_model_num_gauss(h, nullptr, go.mutable_data()));
    gauss_off = go;
  }
  py::dict d;
  d["objf_change"] = oc; d["count"] = cnt; d["floored_elements"] = fe; d["floored_gaussians"] = fg; d["removed"] = rm;
  return d;
}
py::dict KModel::mle_update(KAccs& accs, py::object opts, int flags) {
  khg_mle_options o;
  Arr<double> vfv;                                    // keeps the floor vector alive for the call
  ParseMleOptions(opts, dim, o, vfv);
  float oc = 0, cnt = 0;
  int32_t fe = 0, fg = 0, rm = 0;
  Check(NoGil([&] { return khg_model_mle_update(ctx->h, h, accs.h, &o, (uint16_t)(flags & 0xFFFF), &oc, &cnt, &fe, &fg, &rm); }));
  return mle_result(oc, cnt, fe, fg, rm);
}
// the Extended Baum-Welch update (khg_model_ebw_update): opts / weight_opts are EbwOptions / EbwWeightOptions (or None: the defaults)
py::dict KModel::ebw_update(KAccs& num_accs, KAccs& den_accs, py::object opts, py::object weight_opts, int flags) {
  khg_ebw_options o;
  khg_ebw_weight_options wo;
  khg_ebw_options_default(&o);
  khg_ebw_weight_options_default(&wo);
  if (!opts.is_none()) { o.E = opts.attr("E").cast<double>(); o.tau = opts.attr("tau").cast<double>(); }
  if (!weight_opts.is_none()) {
    wo.min_num_count_weight_update = weight_opts.attr("min_num_count_weight_update").cast<double>();
    wo.min_gaussian_weight = weight_opts.attr("min_gaussian_weight").cast<double>();
    wo.tau = weight_opts.attr("tau").cast<double>();
  }
  khg_ebw_results r;
  Check(NoGil([&] { return khg_model_ebw_update(ctx->h, h, num_accs.h, den_accs.h, &o, &wo, (uint16_t)(flags & 0xFFFF), &r); }));
  return EbwResultsDict(r);
}
// the sharded M-step (khg_model_mle_update_sharded) and its pieces
py::dict KModel::mle_update_sharded(KAccs& accs, py::object opts, int flags, py::object comm) {
  khg_mle_options o;
  Arr<double> vfv;
  ParseMleOptions(opts, dim, o, vfv);
  KComm* c = comm.is_none() ? nullptr : comm.cast<KComm*>();
  float oc = 0, cnt = 0;
  int32_t fe = 0, fg = 0, rm = 0;
  Check(NoGil([&] { return khg_model_mle_update_sharded(ctx->h, h, accs.h, &o, (uint16_t)(flags & 0xFFFF), c ? c->h : nullptr, c ? c->nranks : 1,
                                                        c ? c->rank : 0, &oc, &cnt, &fe, &fg, &rm); }));
  return mle_result(oc, cnt, fe, fg, rm);
}
void KModel::mle_update_range(KAccs& accs, py::object opts, int flags, int first_pdf, int n_pdf) {
  khg_mle_options o;
  Arr<double> vfv;
  ParseMleOptions(opts, dim, o, vfv);
  Check(NoGil([&] { return khg_model_mle_update_range(ctx->h, h, accs.h, &o, (uint16_t)(flags & 0xFFFF), first_pdf, n_pdf); }));
}
py::dict KModel::mle_rows_download(int first_pdf, int n_pdf) {
  if (first_pdf < 0 || n_pdf < 0 || first_pdf + n_pdf > num_pdfs) throw py::value_error("mle_rows_download: pdf range outside the model");
  const py::ssize_t ng = gauss_off.at(first_pdf + n_pdf) - gauss_off.at(first_pdf);
  Arr<float> w({ng}), gc({ng}), miv({ng, (py::ssize_t)dim}), iv({ng, (py::ssize_t)dim});
  py::array_t<uint8_t> res({(py::ssize_t)n_pdf, (py::ssize_t)32});
  Check(NoGil([&] { return khg_model_mle_rows_download(ctx->h, h, first_pdf, n_pdf, w.mutable_data(), gc.mutable_data(), miv.mutable_data(),
                                                       iv.mutable_data(), res.mutable_data()); }));
  py::dict d;
  d["first_pdf"] = first_pdf; d["n_pdf"] = n_pdf; d["weights"] = w; d["gconsts"] = gc; d["means_invvars"] = miv; d["inv_vars"] = iv; d["results"] = res;
  return d;
}
void KModel::mle_rows_upload(py::dict d) {
  const int first_pdf = d["first_pdf"].cast<int>(), n_pdf = d["n_pdf"].cast<int>();
  if (first_pdf < 0 || n_pdf < 0 || first_pdf + n_pdf > num_pdfs) throw py::value_error("mle_rows_upload: pdf range outside the model");
  const py::ssize_t ng = gauss_off.at(first_pdf + n_pdf) - gauss_off.at(first_pdf);
  Arr<float> w = d["weights"].cast<Arr<float>>(), gc = d["gconsts"].cast<Arr<float>>(), miv = d["means_invvars"].cast<Arr<float>>(),
             iv = d["inv_vars"].cast<Arr<float>>();
  py::array_t<uint8_t, py::array::c_style | py::array::forcecast> res = d["results"].cast<py::array_t<uint8_t, py::array::c_style | py::array::forcecast>>();
  if (w.size() != ng || gc.size() != ng || miv.size() != ng * dim || iv.size() != ng * dim || res.size() != (py::ssize_t)n_pdf * 32)
    throw py::value_error("mle_rows_upload: array sizes do not match the pdf range");
  Check(NoGil([&] { return khg_model_mle_rows_upload(ctx->h, h, first_pdf, n_pdf, w.data(), gc.data(), miv.data(), iv.data(), res.data()); }));
}
py::dict KModel::mle_update_finish() {
  float oc = 0, cnt = 0;
  int32_t fe = 0, fg = 0, rm = 0;
  Check(NoGil([&] { return khg_model_mle_update_finish(ctx->h, h, &oc, &cnt, &fe, &fg, &rm); }));
  return mle_result(oc, cnt, fe, fg, rm);
}

// FmllrDiagGmmAccs of n_spk speakers resident in HBM (khg_fmllr_stats)
struct KFmllrStats {
  khg_fmllr_stats* h = nullptr;
  py::object ctx_obj;
  KContext* ctx;
  int n_spk = 0, dim = 0;
  KFmllrStats(py::object ctx_o, int n, int d) : ctx_obj(ctx_o), ctx(ctx_o.cast<KContext*>()), n_spk(n), dim(d) {
    Check(khg_fmllr_stats_create(ctx->h, n, d, &h));
  }
  ~KFmllrStats() { close(); }
  void close() { if (h) { khg_fmllr_stats_destroy(h); h = nullptr; } }
  void zero() { Check(khg_fmllr_stats_zero(ctx->h, h)); }
  py::ssize_t packed() const { return (py::ssize_t)(dim + 1) * (dim + 2) / 2; }
  py::dict download() {
    Arr<double> beta({(py::ssize_t)n_spk}), K({(py::ssize_t)n_spk, (py::ssize_t)dim, (py::ssize_t)dim + 1}), G({(py::ssize_t)n_spk, (py::ssize_t)dim, packed()});
    Check(NoGil([&] { return khg_fmllr_stats_download(ctx->h, h, beta.mutable_data(), K.mutable_data(), G.mutable_data()); }));
    py::dict d;
    d["beta"] = beta; d["K"] = K; d["G"] = G;
    return d;
  }
  void upload(Arr<double> beta, Arr<double> K, Arr<double> G) {
    if (beta.size() != n_spk || K.size() != (py::ssize_t)n_spk * dim * (dim + 1) || G.size() != (py::ssize_t)n_spk * dim * packed())
      throw py::value_error("DeviceFmllrStats.upload: beta [n_spk], K [n_spk, dim, dim + 1], G [n_spk, dim, (dim + 1)(dim + 2) / 2]");
    Check(NoGil([&] { return khg_fmllr_stats_upload(ctx->h, h, beta.data(), K.data(), G.data()); }));
  }
  // the estimate on the device (khg_fmllr_stats_estimate); W_d: a device pointer that receives the float transforms, or None
  py::dict estimate(double min_count, int num_iters, py::object W_d) {
    khg_fmllr_options o;
    khg_fmllr_options_default(&o);
    o.min_count = min_count; o.num_iters = num_iters;
    Arr<float> W({(py::ssize_t)n_spk, (py::ssize_t)dim, (py::ssize_t)dim + 1});
    Arr<double> impr({(py::ssize_t)n_spk}), count({(py::ssize_t)n_spk});
    Arr<int32_t> status({(py::ssize_t)n_spk});
    float* wd = W_d.is_none() ? nullptr : reinterpret_cast<float*>(W_d.cast<uintptr_t>());
    Check(NoGil([&] { return khg_fmllr_stats_estimate(ctx->h, h, &o, W.mutable_data(), wd, impr.mutable_data(), count.mutable_data(), status.mutable_data()); }));
    py::dict d;
    d["W"] = W; d["objf_impr"] = impr; d["count"] = count; d["status"] = status;
    return d;
  }
  void add(float scale, KFmllrStats& src) { Check(khg_fmllr_stats_add(ctx->h, h, scale, src.h)); }
  void set_chunk_frames(int64_t frames) { Check(khg_fmllr_stats_set_chunk_frames(h, frames)); }
  int num_chunks() { int32_t n = 0; Check(khg_fmllr_stats_num_chunks(h, &n)); return n; }
};

// MlltAccs resident in HBM (khg_mllt_stats)
struct KMlltStats {
  khg_mllt_stats* h = nullptr;
  py::object ctx_obj;
  KContext* ctx;
  int dim = 0;
  KMlltStats(py::object ctx_o, int d) : ctx_obj(ctx_o), ctx(ctx_o.cast<KContext*>()), dim(d) { Check(khg_mllt_stats_create(ctx->h, d, &h)); }
  ~KMlltStats() { close(); }
  void close() { if (h) { khg_mllt_stats_destroy(h); h = nullptr; } }
  void zero() { Check(khg_mllt_stats_zero(ctx->h, h)); }
  py::ssize_t packed() const { return (py::ssize_t)dim * (dim + 1) / 2; }
  py::dict download() {
    Arr<double> G({(py::ssize_t)dim, packed()});
    double beta = 0.0;
    Check(NoGil([&] { return khg_mllt_stats_download(ctx->h, h, &beta, G.mutable_data()); }));
    py::dict d;
    d["beta"] = beta; d["G"] = G;
    return d;
  }
  void upload(double beta, Arr<double> G) {
    if (G.size() != (py::ssize_t)dim * packed()) throw py::value_error("DeviceMlltStats.upload: beta, G [dim, dim (dim + 1) / 2]");
    Check(NoGil([&] { return khg_mllt_stats_upload(ctx->h, h, &beta, G.data()); }));
  }
  void add(float scale, KMlltStats& src) { Check(khg_mllt_stats_add(ctx->h, h, scale, src.h)); }
  void set_chunk_frames(int64_t frames) { Check(khg_mllt_stats_set_chunk_frames(h, frames)); }
  int num_chunks() { int32_t n = 0; Check(khg_mllt_stats_num_chunks(h, &n)); return n; }
};

// LdaEstimate accumulators resident in HBM (khg_lda_stats)
struct KLdaStats {
  khg_lda_stats* h = nullptr;
  py::object ctx_obj;
  KContext* ctx;
  int num_classes = 0, dim = 0, left = 0, right = 0, dim_z = 0;
  KLdaStats(py::object ctx_o, int c, int d, int l, int r) : ctx_obj(ctx_o), ctx(ctx_o.cast<KContext*>()), num_classes(c), dim(d), left(l), right(r) {
    Check(khg_lda_stats_create(ctx->h, c, d, l, r, &h));
    dim_z = d * (l + r + 1);
  }
  ~KLdaStats() { close(); }
  void close() { if (h) { khg_lda_stats_destroy(h); h = nullptr; } }
  void zero() { Check(khg_lda_stats_zero(ctx->h, h)); }
  py::ssize_t packed() const { return (py::ssize_t)dim_z * (dim_z + 1) / 2; }
  py::dict download() {
    Arr<double> z({(py::ssize_t)num_classes}), f({(py::ssize_t)num_classes, (py::ssize_t)dim_z}), s2({packed()});
    Check(NoGil([&] { return khg_lda_stats_download(ctx->h, h, z.mutable_data(), f.mutable_data(), s2.mutable_data()); }));
    py::dict d;
    d["zero_acc"] = z; d["first_acc"] = f; d["total_second_acc"] = s2;
    return d;
  }
  void upload(Arr<double> z, Arr<double> f, Arr<double> s2) {
    if (z.size() != num_classes || f.size() != (py::ssize_t)num_classes * dim_z || s2.size() != packed())
      throw py::value_error("DeviceLdaStats.upload: zero_acc [num_classes], first_acc [num_classes, dim_z], total_second_acc [dim_z (dim_z + 1) / 2]");
    Check(NoGil([&] { return khg_lda_stats_upload(ctx->h, h, z.data(), f.data(), s2.data()); }));
  }
  void add(float scale, KLdaStats& src) { Check(khg_lda_stats_add(ctx->h, h, scale, src.h)); }
  void set_chunk_frames(int64_t frames) { Check(khg_lda_stats_set_chunk_frames(h, frames)); }
  int num_chunks() { int32_t n = 0; Check(khg_lda_stats_num_chunks(h, &n)); return n; }
};

// CMVN statistics per speaker resident in HBM (khg_cmvn_stats)
struct KCmvnStats {
  khg_cmvn_stats* h = nullptr;
  py::object ctx_obj;
  KContext* ctx;
  int n_spk = 0, dim = 0;
  KCmvnStats(py::object ctx_o, int s, int d) : ctx_obj(ctx_o), ctx(ctx_o.cast<KContext*>()), n_spk(s), dim(d) { Check(khg_cmvn_stats_create(ctx->h, s, d, &h)); }
  ~KCmvnStats() { close(); }
  void close() { if (h) { khg_cmvn_stats_destroy(h); h = nullptr; } }
  void zero() { Check(khg_cmvn_stats_zero(ctx->h, h)); }
  Arr<double> download() {
    Arr<double> st({(py::ssize_t)n_spk, (py::ssize_t)2, (py::ssize_t)dim + 1});
    Check(NoGil([&] { return khg_cmvn_stats_download(ctx->h, h, st.mutable_data()); }));
    return st;
  }
  void upload(Arr<double> st) {
    if (st.size() != (py::ssize_t)n_spk * 2 * (dim + 1)) throw py::value_error("DeviceCmvnStats.upload: stats [n_spk, 2, dim + 1]");
    Check(NoGil([&] { return khg_cmvn_stats_upload(ctx->h, h, st.data()); }));
  }
  void add(float scale, KCmvnStats& src) { Check(khg_cmvn_stats_add(ctx->h, h, scale, src.h)); }
  void set_chunk_frames(int64_t frames) { Check(khg_cmvn_stats_set_chunk_frames(h, frames)); }
  int num_chunks() { int32_t n = 0; Check(khg_cmvn_stats_num_chunks(h, &n)); return n; }
};

// the waveform front end's tables resident in HBM (khg_frontend)
struct KFrontend {
  khg_frontend* h = nullptr;
  py::object ctx_obj;
  KContext* ctx;
  khg_frontend_opts opts;
  int dim = 0;
  KFrontend(py::object ctx_o, const khg_frontend_opts& o) : ctx_obj(ctx_o), ctx(ctx_o.cast<KContext*>()), opts(o) {
    int32_t d[8];
    Check(khg_frontend_dims(&o, d));
    dim = d[5];
    Check(khg_frontend_create(ctx->h, &o, &h));
  }
  ~KFrontend() { close(); }
  void close() { if (h) { khg_frontend_destroy(h); h = nullptr; } }
  // samples: a host array (float32 or int16, by sample_type) or None with samples_d, a device pointer; out: a device pointer or None
  // (then only the frame offsets are computed)
  Arr<int64_t> compute(Arr<int64_t> sample_off, py::object samples_h, uintptr_t samples_d, int sample_type, py::object out) {
    if (!h) throw py::value_error("DeviceFrontend.compute: the handle is closed");
    if (sample_off.ndim() != 1 || sample_off.size() < 1) throw py::value_error("DeviceFrontend.compute: sample_off [n_utt + 1]");
    const int32_t n_utt = (int32_t)sample_off.size() - 1;
    const void* sh = nullptr;
    py::array keep;
    if (!samples_h.is_none()) {
      keep = py::array::ensure(samples_h, py::array::c_style);
      const bool i16 = sample_type == KHG_WAVE_I16;
      if (!keep || keep.ndim() != 1 || !keep.dtype().is(i16 ? py::dtype::of<int16_t>() : py::dtype::of<float>()))
        throw py::value_error("DeviceFrontend.compute: samples must be a contiguous 1-d array of the sample type");
      if (keep.size() < sample_off.at(n_utt)) throw py::value_error("DeviceFrontend.compute: fewer samples than sample_off says");
      sh = keep.data();
    }
    float* od = out.is_none() ? nullptr : reinterpret_cast<float*>(out.cast<uintptr_t>());
    Arr<int64_t> fo((py::ssize_t)n_utt + 1);
    Check(NoGil([&] { return khg_frontend_compute(ctx->h, h, n_utt, sample_off.data(), sh, reinterpret_cast<const void*>(samples_d), sample_type, fo.mutable_data(), od); }));
    return fo;
  }
};

// decision-tree statistics resident in HBM (khg_tree_stats)
struct KTreeStats {
  khg_tree_stats* h = nullptr;
  py::object ctx_obj;
  KContext* ctx;
  int dim = 0, N = 0, P = 0;
  KTreeStats(py::object ctx_o, int d, int n, int p) : ctx_obj(ctx_o), ctx(ctx_o.cast<KContext*>()), dim(d), N(n), P(p) { Check(khg_tree_stats_create(ctx->h, d, n, p, &h)); }
  ~KTreeStats() { close(); }
  void close() { if (h) { khg_tree_stats_destroy(h); h = nullptr; } }
  void zero() { Check(khg_tree_stats_zero(ctx->h, h)); }
  int64_t num_keys() { int64_t n = 0; Check(khg_tree_stats_num_keys(ctx->h, h, &n)); return n; }
  py::dict download() {
    const py::ssize_t K = (py::ssize_t)num_keys(), K1 = K > 0 ? K : 1;
    Arr<int32_t> keys({K1, (py::ssize_t)N + 1});
    Arr<double> cnt({K1}), x({K1, (py::ssize_t)dim}), x2({K1, (py::ssize_t)dim});
    Check(NoGil([&] { return khg_tree_stats_download(ctx->h, h, keys.mutable_data(), cnt.mutable_data(), x.mutable_data(), x2.mutable_data()); }));
    py::dict d;
    const py::slice sl(0, K, 1);
    d["keys"] = py::array(keys)[sl]; d["count"] = py::array(cnt)[sl]; d["x"] = py::array(x)[sl]; d["x2"] = py::array(x2)[sl];
    return d;
  }
  void upload(Arr<int32_t> keys, Arr<double> cnt, Arr<double> x, Arr<double> x2) {
    const py::ssize_t K = cnt.size();
    if (keys.size() != K * (N + 1) || x.size() != K * dim || x2.size() != K * dim)
      throw py::value_error("DeviceTreeStats.upload: keys [num_keys, N + 1], count [num_keys], x and x2 [num_keys, dim]");
    Check(NoGil([&] { return khg_tree_stats_upload(ctx->h, h, (int64_t)K, keys.data(), cnt.data(), x.data(), x2.data()); }));
  }
  void add(float scale, KTreeStats& src) { Check(NoGil([&] { return khg_tree_stats_add(ctx->h, h, scale, src.h); })); }
};

// the variants of khg_hip.h (KHG_K3V_*) by name, for khg_k3_forms / khg_utts_k3_last
static const char* K3VariantName(int v) {
  static const char* const names[] = {"wave", "wave16", "wave16_records", "finalize", "mfma", "block16", "valu"};
  return v >= 0 && v < 7 ? names[v] : "?";
}
struct KUtts {
  khg_utts* h = nullptr;
  py::object ctx_obj, keep, keep_model;
  KContext* ctx;
  Arr<int64_t> frame_off;
  int n_utt = 0, dim = 0;
  int64_t state_total = 0;     // states over all graphs (bounds the words of a lattice decode)
  KUtts(py::object ctx_o, py::object tm, Arr<int64_t> fo, py::object feats, py::object dim_o, py::object graphs, py::object graph)
      : ctx_obj(ctx_o), ctx(ctx_o.cast<KContext*>()), frame_off(fo) {
    if (!graphs.is_none() && !graph.is_none()) throw py::value_error("UtteranceSet: exactly one of graphs / graph");
    n_utt = (int)fo.shape(0) - 1;
    const float* feats_h = nullptr;
    const float* feats_d = nullptr;
    Arr<float> fh;
    if (py::isinstance<py::tuple>(feats)) {        // (device pointer, keep-alive object): features already in HBM
      py::tuple t = feats;
      feats_d = reinterpret_cast<const float*>(t[0].cast<uintptr_t>());
      keep = t[1];
      if (dim_o.is_none()) throw py::value_error("UtteranceSet: dim is required with device features");
      dim = dim_o.cast<int>();
    } else {
      fh = feats.cast<Arr<float>>();
      if (fh.ndim() != 2 || fh.shape(0) != fo.at(n_utt)) throw py::value_error("UtteranceSet: feats must be [frames, dim]");
      dim = (int)fh.shape(1);
      feats_h = fh.data();
    }
    const khg_tm* tmh = tm.is_none() ? nullptr : tm.cast<KTransitions*>()->h;
    if (!graph.is_none()) {          // a DecodingGraph: every utterance decodes on it (the set holds its own reference to the tables)
      khg_graph* gh = reinterpret_cast<khg_graph*>(graph.attr("h").cast<uintptr_t>());
      if (!gh) throw py::value_error("UtteranceSet: the DecodingGraph is closed");
      Check(khg_utts_create_on_graph(ctx->h, tmh, gh, n_utt, dim, fo.data(), feats_h, feats_d, &h));
      state_total = graph.attr("num_states").cast<int64_t>() * n_utt;
    } else if (graphs.is_none()) {
      Check(khg_utts_create(ctx->h, tmh, n_utt, dim, fo.data(), feats_h, feats_d, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                            nullptr, nullptr, &h));
    } else {
      py::dict g = graphs;
      auto so = g["state_off"].cast<Arr<int64_t>>(); auto st = g["start"].cast<Arr<int32_t>>();
      auto ao = g["arc_off"].cast<Arr<int64_t>>(); auto il = g["ilabel"].cast<Arr<int32_t>>();
      auto ol = g["olabel"].cast<Arr<int32_t>>(); auto w = g["weight"].cast<Arr<float>>();
      auto ns = g["nextstate"].cast<Arr<int32_t>>(); auto fin = g["final"].cast<Arr<float>>();
      Check(khg_utts_create(ctx->h, tmh, n_utt, dim, fo.data(), feats_h, feats_d, so.data(), st.data(), ao.data(), il.data(), ol.data(),
                            w.data(), ns.data(), fin.data(), &h));
      state_total = so.at(n_utt);
    }
  }
  ~KUtts() { close(); }
  void close() { if (h) { khg_utts_destroy(h); h = nullptr; } }
  void set_pdf_list(Arr<int32_t> p) { Check(khg_utts_set_pdf_list(h, (int32_t)p.shape(0), p.data())); }
  void features_changed() { Check(khg_utts_features_changed(h)); }
  py::tuple pdf_lists() {
    Arr<int64_t> off({(py::ssize_t)n_utt + 1});
    Check(khg_utts_num_pdfs(h, off.mutable_data()));
    const py::ssize_t n = off.at(n_utt);
    Arr<int32_t> pdfs({n > 0 ? n : 1});
    Check(khg_utts_pdfs(h, pdfs.mutable_data()));
    return py::make_tuple(off, py::array(pdfs)[py::slice(0, n, 1)]);
  }
  // khg_utts_k2_plan: what align() would launch under the context's current options
  py::dict k2_plan(py::object ctx_o) {
    int32_t o[8];
    Check(khg_utts_k2_plan(ctx_o.cast<KContext*>()->h, h, o));
    py::dict d;
    d["KS"] = o[0]; d["DEG"] = o[1]; d["FAST"] = o[2] != 0; d["GMEM"] = o[3] != 0; d["SC"] = o[4] != 0;
    d["nthr"] = o[5]; d["lds_bytes"] = o[6]; d["faithful_form"] = o[7];
    return d;
  }
  // khg_utts_k3_planes: K3's split feature records on the set
  py::dict k3_planes() {
    int64_t bytes = 0, packs = 0; int32_t used = 0;
    Check(khg_utts_k3_planes(h, &bytes, &packs, &used));
    py::dict d;
    d["bytes"] = bytes; d["packs"] = packs; d["used"] = used != 0;
    return d;
  }
  // khg_utts_k3_last: what the last statistics pass over the set launched, one dict per run of its plan
  py::list k3_last() {
    int32_t o[2][12]; int32_t n = 0;
    Check(khg_utts_k3_last(h, o, &n));
    py::list out;
    for (int i = 0; i < n; ++i) {
      py::dict d;
      d["variant"] = K3VariantName(o[i][0]); d["KQ"] = o[i][1]; d["NB"] = o[i][2]; d["waves"] = o[i][3]; d["POST"] = o[i][4] != 0;
      d["f16a"] = o[i][5] != 0; d["f16b"] = o[i][6] != 0; d["planes"] = o[i][7] != 0; d["ny"] = o[i][8]; d["cls_lo"] = o[i][9];
      d["cls_hi"] = o[i][10]; d["lds_bytes"] = o[i][11];
      out.append(d);
    }
    return out;
  }
  // khg_utts_k1_last: what the last loglikes() call on the set chose and launched; None before the first call
  py::object k1_last() {
    static const char* const forms[] = {"none", "f16x2s", "f16x2", "pdf", "utt", "wide"};
    static const char* const keys[] = {"declined", "K", "mode", "pack", "persistent", "grid", "chunks", "per", "order", "tail_shift", "shift_mode",
                                       "nf", "aligned", "interleave"};
    int32_t o[KHG_K1_LAST_WORDS];
    Check(khg_utts_k1_last(h, o));
    if (!o[0]) return py::none();
    py::dict d;
    d["form"] = forms[o[1] >= 0 && o[1] < 6 ? o[1] : 0]; d["asked"] = forms[o[2] >= 0 && o[2] < 6 ? o[2] : 0];
    for (int i = 0; i < 14; ++i) d[keys[i]] = o[3 + i];
    py::list nb;
    for (int i = 0; i < 8; ++i) nb.append(o[17 + i]);
    d["nb_slices"] = nb; d["repacked"] = o[25]; d["repaired"] = o[26];
    return d;
  }
  // khg_utts_k2_ladder: align() would run the ladder form of that kernel
  bool k2_ladder(py::object ctx_o) {
    int32_t o = 0;
    Check(khg_utts_k2_ladder(ctx_o.cast<KContext*>()->h, h, &o));
    return o != 0;
  }
  // khg_utts_k2_tail: (scanned, serial) replay batches per utterance of the last align() under option k2_prof
  py::array k2_tail() {
    Arr<int32_t> o({(py::ssize_t)n_utt, (py::ssize_t)2});
    Check(khg_utts_k2_tail(h, o.mutable_data(), 2 * (int64_t)n_utt));
    return o;
  }
  py::object pdf_first_frames() {
    Arr<int64_t> off({(py::ssize_t)n_utt + 1});
    Check(khg_utts_num_pdfs(h, off.mutable_data()));
    const py::ssize_t n = off.at(n_utt);
    Arr<int32_t> first({n > 0 ? n : 1});
    Check(khg_utts_pdf_first(h, first.mutable_data()));
    return py::array(first)[py::slice(0, n, 1)];
  }
  py::object pdf_last_frames() {
    Arr<int64_t> off({(py::ssize_t)n_utt + 1});
    Check(khg_utts_num_pdfs(h, off.mutable_data()));
    const py::ssize_t n = off.at(n_utt);
    Arr<int32_t> last({n > 0 ? n : 1});
    Check(khg_utts_pdf_last(h, last.mutable_data()));
    return py::array(last)[py::slice(0, n, 1)];
  }
  // reachable_only: from each pdf's first readable frame (khg_loglikes_reachable); band: ... up to its last useful frame, the rest
  // filled with an upper bound (khg_loglikes_band; `model` must stay alive until the align that follows has returned)
  void loglikes(KModel& m, bool reachable_only, bool band) {
    keep_model = band ? py::cast(&m) : py::object();
    Check(NoGil([&] { return band ? khg_loglikes_band(ctx->h, m.h, h) : reachable_only ? khg_loglikes_reachable(ctx->h, m.h, h) : khg_loglikes(ctx->h, m.h, h); }));
  }
  py::tuple loglikes_layout() {
    Arr<int64_t> off({(py::ssize_t)n_utt + 1});
    int64_t tot = 0;
    Check(khg_loglikes_layout(h, off.mutable_data(), &tot));
    return py::make_tuple(off, tot);
  }
  py::list download_loglikes() {
    Arr<int64_t> off({(py::ssize_t)n_utt + 1}), poff({(py::ssize_t)n_utt + 1});
    int64_t tot = 0;
    Check(khg_loglikes_layout(h, off.mutable_data(), &tot));
    Check(khg_utts_num_pdfs(h, poff.mutable_data()));
    std::vector<float> buf((size_t)(tot > 0 ? tot : 1));
    Check(NoGil([&] { return khg_loglikes_download(ctx->h, h, buf.data()); }));
    py::list out;
    for (int u = 0; u < n_utt; ++u) {
      const int64_t T = frame_off.at(u + 1) - frame_off.at(u), tpad = (T + 31) / 32 * 32, n = poff.at(u + 1) - poff.at(u);
      Arr<float> m({(py::ssize_t)n, (py::ssize_t)T});
      for (int64_t j = 0; j < n; ++j) std::memcpy(m.mutable_data() + j * T, buf.data() + off.at(u) + j * tpad, sizeof(float) * (size_t)T);
      out.append(m);
    }
    return out;
  }
  void upload_loglikes(py::list mats) {
    Arr<int64_t> off({(py::ssize_t)n_utt + 1});
    int64_t tot = 0;
    Check(khg_loglikes_layout(h, off.mutable_data(), &tot));
    std::vector<float> buf((size_t)(tot > 0 ? tot : 1), 0.0f);
    for (int u = 0; u < n_utt && u < (int)mats.size(); ++u) {
      Arr<float> m = mats[u].cast<Arr<float>>();
      const int64_t T = frame_off.at(u + 1) - frame_off.at(u), tpad = (T + 31) / 32 * 32;
      for (py::ssize_t j = 0; j < m.shape(0); ++j) std::memcpy(buf.data() + off.at(u) + j * tpad, m.data() + j * m.shape(1), sizeof(float) * (size_t)T);
    }
    Check(NoGil([&] { return khg_loglikes_upload(ctx->h, h, buf.data()); }));
  }
  // khg_decode_lattice_faster on the resident scores (which must not come from loglikes(band=True))
  py::dict decode_lattice_faster(KTransitions& tm, float beam, int32_t max_active, int32_t min_active, float lattice_beam, int32_t prune_interval,
                                 float beam_delta, float hash_ratio, float prune_scale, float acoustic_scale, bool allow_partial, int32_t scratch_per_frame) {
    khg_lattice_faster_config c;
    khg_lattice_faster_config_default(&c);
    c.beam = beam; c.max_active = max_active; c.min_active = min_active; c.lattice_beam = lattice_beam; c.prune_interval = prune_interval;
    c.beam_delta = beam_delta; c.hash_ratio = hash_ratio; c.prune_scale = prune_scale; c.acoustic_scale = acoustic_scale;
    c.allow_partial = allow_partial ? 1 : 0; c.scratch_per_frame = scratch_per_frame;
    const int64_t N = frame_off.at(n_utt), wcap = 2 * N + 1024 * (int64_t)n_utt + 1024;
    Arr<int32_t> ali({(py::ssize_t)(N > 0 ? N : 1)}), words({(py::ssize_t)wcap}), status({(py::ssize_t)n_utt});
    Arr<int64_t> woff({(py::ssize_t)n_utt + 1});
    Arr<double> like({(py::ssize_t)n_utt});
    Check(NoGil([&] { return khg_decode_lattice_faster(ctx->h, tm.h, h, &c, ali.mutable_data(), words.mutable_data(), woff.mutable_data(), wcap,
                                                       like.mutable_data(), status.mutable_data()); }));
    py::dict d;
    d["ali"] = py::array(ali)[py::slice(0, N, 1)];
    d["like"] = like; d["status"] = status;
    d["words"] = py::array(words)[py::slice(0, woff.at(n_utt), 1)];
    d["words_off"] = woff;
    return d;
  }
  // khg_decode_lattice_faster_raw on the resident scores: decode_lattice_faster's outputs plus the batch's raw lattices
  // (LatticeFasterDecoder::GetRawLattice), as raw_lattice_simple's flat arrays (device=false) or as "lattices", a DeviceLattices on this
  // set's context with nothing downloaded (device=true)
  py::dict raw_lattice_faster_impl(KTransitions& tm, float beam, int32_t max_active, int32_t min_active, float lattice_beam, int32_t prune_interval,
                                   float beam_delta, float hash_ratio, float prune_scale, float acoustic_scale, bool allow_partial,
                                   int32_t scratch_per_frame, bool device) {
    khg_lattice_faster_config c;
    khg_lattice_faster_config_default(&c);
    c.beam = beam; c.max_active = max_active; c.min_active = min_active; c.lattice_beam = lattice_beam; c.prune_interval = prune_interval;
    c.beam_delta = beam_delta; c.hash_ratio = hash_ratio; c.prune_scale = prune_scale; c.acoustic_scale = acoustic_scale;
    c.allow_partial = allow_partial ? 1 : 0; c.scratch_per_frame = scratch_per_frame;
    const int64_t N = frame_off.at(n_utt), wcap = 2 * N + 1024 * (int64_t)n_utt + 1024;
    Arr<int32_t> ali({(py::ssize_t)(N > 0 ? N : 1)}), words({(py::ssize_t)wcap}), status({(py::ssize_t)n_utt});
    Arr<int64_t> woff({(py::ssize_t)n_utt + 1});
    Arr<double> like({(py::ssize_t)n_utt});
    auto lat = std::make_shared<khg::PyDeviceLattices>();       // (frees the handle when it goes)
    lat->ctx = ctx->h; lat->ctx_obj = ctx_obj;
    const auto t0 = std::chrono::steady_clock::now();
    Check(NoGil([&] { return khg_decode_lattice_faster_raw(ctx->h, tm.h, h, &c, ali.mutable_data(), words.mutable_data(), woff.mutable_data(), wcap,
                                                           like.mutable_data(), status.mutable_data(), &lat->h); }));
    const auto t1 = std::chrono::steady_clock::now();
    py::dict d;
    d["ali"] = py::array(ali)[py::slice(0, N, 1)];
    d["like"] = like; d["status"] = status;
    d["words"] = py::array(words)[py::slice(0, woff.at(n_utt), 1)];
    d["words_off"] = woff;
    if (device) { d["lattices"] = lat; return d; }
    Arr<int64_t> so({(py::ssize_t)n_utt + 1}), ao({(py::ssize_t)n_utt + 1});
    Check(khg_lattices_sizes(lat->h, so.mutable_data(), ao.mutable_data()));
    const py::ssize_t NS = (py::ssize_t)so.at(n_utt), NA = (py::ssize_t)ao.at(n_utt);
    Arr<int32_t> frame({NS}), gstate({NS}), abeg({NS}), il({NA}), ol({NA}), ns({NA}), start({(py::ssize_t)n_utt});
    Arr<float> tot({NS}), extra({NS}), fin({NS}), gc({NA}), ac({NA});
    Check(NoGil([&] { return khg_lattices_download(ctx->h, lat->h, frame.mutable_data(), gstate.mutable_data(), tot.mutable_data(), extra.mutable_data(),
                                                   fin.mutable_data(), abeg.mutable_data(), il.mutable_data(), ol.mutable_data(), gc.mutable_data(),
                                                   ac.mutable_data(), ns.mutable_data(), start.mutable_data()); }));
    const auto t2 = std::chrono::steady_clock::now();
    int64_t bytes = 0;
    Check(khg_lattices_device_bytes(lat->h, &bytes));
    d["state_off"] = so; d["arc_off"] = ao; d["start"] = start;
    d["frame"] = frame; d["graph_state"] = gstate; d["tot_cost"] = tot; d["extra_cost"] = extra; d["final_cost"] = fin; d["arc_begin"] = abeg;
    d["ilabel"] = il; d["olabel"] = ol; d["graph_cost"] = gc; d["acoustic_cost"] = ac; d["nextstate"] = ns;
    d["device_bytes"] = bytes;
    d["decode_s"] = std::chrono::duration<double>(t1 - t0).count();
    d["download_s"] = std::chrono::duration<double>(t2 - t1).count();
    return d;
  }
  py::dict raw_lattice_faster(KTransitions& tm, float beam, int32_t max_active, int32_t min_active, float lattice_beam, int32_t prune_interval,
                              float beam_delta, float hash_ratio, float prune_scale, float acoustic_scale, bool allow_partial, int32_t scratch_per_frame) {
    return raw_lattice_faster_impl(tm, beam, max_active, min_active, lattice_beam, prune_interval, beam_delta, hash_ratio, prune_scale, acoustic_scale,
                                   allow_partial, scratch_per_frame, false);
  }
  py::dict raw_lattices_faster_device(KTransitions& tm, float beam, int32_t max_active, int32_t min_active, float lattice_beam, int32_t prune_interval,
                                      float beam_delta, float hash_ratio, float prune_scale, float acoustic_scale, bool allow_partial,
                                      int32_t scratch_per_frame) {
    return raw_lattice_faster_impl(tm, beam, max_active, min_active, lattice_beam, prune_interval, beam_delta, hash_ratio, prune_scale, acoustic_scale,
                                   allow_partial, scratch_per_frame, true);
  }
  // khg_decode_lattice_simple on the resident scores (which must not come from loglikes(band=True))
  py::dict decode_lattice_simple(KTransitions& tm, float beam, float lattice_beam, int32_t prune_interval, float prune_scale, float acoustic_scale,
                                 bool allow_partial, int32_t scratch_per_frame) {
    khg_lattice_simple_config c;
    khg_lattice_simple_config_default(&c);
    c.beam = beam; c.lattice_beam = lattice_beam; c.prune_interval = prune_interval; c.prune_scale = prune_scale; c.acoustic_scale = acoustic_scale;
    c.allow_partial = allow_partial ? 1 : 0; c.scratch_per_frame = scratch_per_frame;
    const int64_t N = frame_off.at(n_utt), wcap = 2 * N + 1024 * (int64_t)n_utt + 1024 + state_total;
    Arr<int32_t> ali({(py::ssize_t)(N > 0 ? N : 1)}), words({(py::ssize_t)wcap}), status({(py::ssize_t)n_utt}), ef({(py::ssize_t)n_utt});
    Arr<int64_t> woff({(py::ssize_t)n_utt + 1});
    Arr<double> like({(py::ssize_t)n_utt});
    Check(NoGil([&] { return khg_decode_lattice_simple(ctx->h, tm.h, h, &c, ali.mutable_data(), words.mutable_data(), woff.mutable_data(), wcap,
                                                       like.mutable_data(), status.mutable_data(), ef.mutable_data()); }));
    py::dict d;
    d["ali"] = py::array(ali)[py::slice(0, N, 1)];
    d["like"] = like; d["status"] = status; d["error_frame"] = ef;
    d["words"] = py::array(words)[py::slice(0, woff.at(n_utt), 1)];
    d["words_off"] = woff;
    return d;
  }
  // khg_decode_lattice_simple_raw on the resident scores: decode_lattice_simple's outputs plus the batch's raw lattices as flat arrays
  // (state_off / arc_off [n_utt + 1]; per state frame, graph_state, tot_cost, extra_cost, final_cost, arc_begin; per arc ilabel, olabel,
  // graph_cost, acoustic_cost, nextstate; per utterance start), the bytes they took on the device and the seconds of the decode call
  // and of the download
  py::dict raw_lattice_simple(KTransitions& tm, float beam, float lattice_beam, int32_t prune_interval, float prune_scale, float acoustic_scale,
                              int32_t scratch_per_frame) {
    khg_lattice_simple_config c;
    khg_lattice_simple_config_default(&c);
    c.beam = beam; c.lattice_beam = lattice_beam; c.prune_interval = prune_interval; c.prune_scale = prune_scale; c.acoustic_scale = acoustic_scale;
    c.scratch_per_frame = scratch_per_frame;
    const int64_t N = frame_off.at(n_utt), wcap = 2 * N + 1024 * (int64_t)n_utt + 1024 + state_total;
    Arr<int32_t> ali({(py::ssize_t)(N > 0 ? N : 1)}), words({(py::ssize_t)wcap}), status({(py::ssize_t)n_utt}), ef({(py::ssize_t)n_utt});
    Arr<int64_t> woff({(py::ssize_t)n_utt + 1}), so({(py::ssize_t)n_utt + 1}), ao({(py::ssize_t)n_utt + 1});
    Arr<double> like({(py::ssize_t)n_utt});
    struct LatH { khg_lattices* h = nullptr; ~LatH() { if (h) khg_lattices_destroy(h); } } lh;
    const auto t0 = std::chrono::steady_clock::now();
    Check(NoGil([&] { return khg_decode_lattice_simple_raw(ctx->h, tm.h, h, &c, ali.mutable_data(), words.mutable_data(), woff.mutable_data(), wcap,
                                                           like.mutable_data(), status.mutable_data(), ef.mutable_data(), &lh.h); }));
    const auto t1 = std::chrono::steady_clock::now();
    Check(khg_lattices_sizes(lh.h, so.mutable_data(), ao.mutable_data()));
    const py::ssize_t NS = (py::ssize_t)so.at(n_utt), NA = (py::ssize_t)ao.at(n_utt);
    Arr<int32_t> frame({NS}), gstate({NS}), abeg({NS}), il({NA}), ol({NA}), ns({NA}), start({(py::ssize_t)n_utt});
    Arr<float> tot({NS}), extra({NS}), fin({NS}), gc({NA}), ac({NA});
    Check(NoGil([&] { return khg_lattices_download(ctx->h, lh.h, frame.mutable_data(), gstate.mutable_data(), tot.mutable_data(), extra.mutable_data(),
                                                   fin.mutable_data(), abeg.mutable_data(), il.mutable_data(), ol.mutable_data(), gc.mutable_data(),
                                                   ac.mutable_data(), ns.mutable_data(), start.mutable_data()); }));
    const auto t2 = std::chrono::steady_clock::now();
    int64_t bytes = 0;
    Check(khg_lattices_device_bytes(lh.h, &bytes));
    py::dict d;
    d["ali"] = py::array(ali)[py::slice(0, N, 1)];
    d["like"] = like; d["status"] = status; d["error_frame"] = ef;
    d["words"] = py::array(words)[py::slice(0, woff.at(n_utt), 1)];
    d["words_off"] = woff;
    d["state_off"] = so; d["arc_off"] = ao; d["start"] = start;
    d["frame"] = frame; d["graph_state"] = gstate; d["tot_cost"] = tot; d["extra_cost"] = extra; d["final_cost"] = fin; d["arc_begin"] = abeg;
    d["ilabel"] = il; d["olabel"] = ol; d["graph_cost"] = gc; d["acoustic_cost"] = ac; d["nextstate"] = ns;
    d["device_bytes"] = bytes;
    d["decode_s"] = std::chrono::duration<double>(t1 - t0).count();
    d["download_s"] = std::chrono::duration<double>(t2 - t1).count();
    return d;
  }
  // raw_lattice_simple that keeps the lattices on the device: decode_lattice_simple's outputs plus "lattices", a DeviceLattices on this
  // set's context (best_path / prune / download there); nothing of the lattices is downloaded
  py::dict raw_lattices_simple_device(KTransitions& tm, float beam, float lattice_beam, int32_t prune_interval, float prune_scale, float acoustic_scale,
                                      int32_t scratch_per_frame) {
    khg_lattice_simple_config c;
    khg_lattice_simple_config_default(&c);
    c.beam = beam; c.lattice_beam = lattice_beam; c.prune_interval = prune_interval; c.prune_scale = prune_scale; c.acoustic_scale = acoustic_scale;
    c.scratch_per_frame = scratch_per_frame;
    const int64_t N = frame_off.at(n_utt), wcap = 2 * N + 1024 * (int64_t)n_utt + 1024 + state_total;
    Arr<int32_t> ali({(py::ssize_t)(N > 0 ? N : 1)}), words({(py::ssize_t)wcap}), status({(py::ssize_t)n_utt}), ef({(py::ssize_t)n_utt});
    Arr<int64_t> woff({(py::ssize_t)n_utt + 1});
    Arr<double> like({(py::ssize_t)n_utt});
    auto lat = std::make_shared<khg::PyDeviceLattices>();
    lat->ctx = ctx->h; lat->ctx_obj = ctx_obj;
    Check(NoGil([&] { return khg_decode_lattice_simple_raw(ctx->h, tm.h, h, &c, ali.mutable_data(), words.mutable_data(), woff.mutable_data(), wcap,
                                                           like.mutable_data(), status.mutable_data(), ef.mutable_data(), &lat->h); }));
    py::dict d;
    d["ali"] = py::array(ali)[py::slice(0, N, 1)];
    d["like"] = like; d["status"] = status; d["error_frame"] = ef;
    d["words"] = py::array(words)[py::slice(0, woff.at(n_utt), 1)];
    d["words_off"] = woff;
    d["lattices"] = lat;
    return d;
  }
  py::object align(KTransitions& tm, float beam, float retry_beam, float acoustic_scale, bool careful, int64_t max_active, int min_active,
                   float beam_delta, float hash_ratio, py::object download) {
    khg_align_config c;
    khg_align_config_default(&c);
    c.beam = beam; c.retry_beam = retry_beam; c.careful = careful ? 1 : 0; c.acoustic_scale = acoustic_scale;
    c.max_active = (int32_t)std::min<int64_t>(max_active, std::numeric_limits<int32_t>::max());
    c.min_active = min_active; c.beam_delta = beam_delta; c.hash_ratio = hash_ratio;
    const bool summary = py::isinstance<py::str>(download) && download.cast<std::string>() == "summary";
    if (!summary && !download.cast<bool>()) {
      Check(NoGil([&] { return khg_align(ctx->h, tm.h, h, &c, nullptr, nullptr, nullptr, 0, nullptr, nullptr); }));
      return py::none();
    }
    Arr<float> like({(py::ssize_t)n_utt});
    Arr<int32_t> status({(py::ssize_t)n_utt});
    py::dict d;
    if (summary) {
      Check(NoGil([&] { return khg_align(ctx->h, tm.h, h, &c, nullptr, nullptr, nullptr, 0, like.mutable_data(), status.mutable_data()); }));
      d["like"] = like; d["status"] = status;
      return d;
    }
    const int64_t N = frame_off.at(n_utt), wcap = N + 16 * (int64_t)n_utt + 1024;
    Arr<int32_t> ali({(py::ssize_t)(N > 0 ? N : 1)}), words({(py::ssize_t)wcap});
    Arr<int64_t> woff({(py::ssize_t)n_utt + 1});
    Check(NoGil([&] { return khg_align(ctx->h, tm.h, h, &c, ali.mutable_data(), words.mutable_data(), woff.mutable_data(), wcap, like.mutable_data(), status.mutable_data()); }));
    d["ali"] = py::array(ali)[py::slice(0, N, 1)];
    d["like"] = like; d["status"] = status;
    d["words"] = py::array(words)[py::slice(0, woff.at(n_utt), 1)];
    d["words_off"] = woff;
    return d;
  }
  void upload_ali(Arr<int32_t> a) {
    if (a.shape(0) != frame_off.at(n_utt)) throw py::value_error("upload_ali: one transition-id per frame");
    Check(NoGil([&] { return khg_ali_upload(ctx->h, h, a.data()); }));
  }
  py::object download_ali() {
    const int64_t N = frame_off.at(n_utt);
    Arr<int32_t> a({(py::ssize_t)(N > 0 ? N : 1)});
    Check(NoGil([&] { return khg_ali_download(ctx->h, h, a.mutable_data()); }));
    return py::array(a)[py::slice(0, N, 1)];
  }
  void acc_stats_reduce(KModel& m, KTransitions& tm, KAccs& accs, float weight, py::object comm, int nparts) {
    void* c = comm.is_none() ? nullptr : comm.cast<KComm*>()->h;
    Check(NoGil([&] { return khg_acc_stats_reduce(ctx->h, m.h, tm.h, h, weight, accs.h, c, nparts); }));
  }
  void acc_stats(KModel& m, KTransitions& tm, KAccs& accs, float weight) { Check(NoGil([&] { return khg_acc_stats(ctx->h, m.h, tm.h, h, weight, accs.h); })); }
  // gmm-acc-stats (khg_acc_stats_post): the statistics of every (transition-id, weight) of the posteriors, utterance u of `post` on
  // utterance u of this set; no resident alignment needed
  void acc_stats_post(KModel& m, KTransitions& tm, khg::PyDevicePosteriors& post, KAccs& accs, float scale) {
    if (!post.h) throw py::value_error("acc_stats_post: the DevicePosteriors are closed");
    Check(NoGil([&] { return khg_acc_stats_post(ctx->h, m.h, tm.h, h, post.h, scale, accs.h); }));
  }
  // gmm-acc-stats2 (khg_acc_stats_post2): the positive weights into num_accs, the negated negative ones into den_accs
  void acc_stats_post2(KModel& m, KTransitions& tm, khg::PyDevicePosteriors& post, KAccs& num_accs, KAccs& den_accs, float scale) {
    if (!post.h) throw py::value_error("acc_stats_post2: the DevicePosteriors are closed");
    Check(NoGil([&] { return khg_acc_stats_post2(ctx->h, m.h, tm.h, h, post.h, scale, num_accs.h, den_accs.h); }));
  }
  // gmm-est-fmllr's accumulation (khg_acc_fmllr_stats_post): utterance u of `post` counts for speaker utt2spk[u] (< 0: for nobody)
  void acc_fmllr_stats_post(KModel& m, KTransitions& tm, khg::PyDevicePosteriors& post, Arr<int32_t> utt2spk, KFmllrStats& stats, float scale) {
    if (!post.h) throw py::value_error("acc_fmllr_stats_post: the DevicePosteriors are closed");
    if (utt2spk.size() != n_utt) throw py::value_error("acc_fmllr_stats_post: one speaker per utterance");
    Check(NoGil([&] { return khg_acc_fmllr_stats_post(ctx->h, m.h, tm.h, h, post.h, scale, utt2spk.data(), stats.h); }));
  }
  // gmm-acc-mllt (khg_acc_mllt_stats_post)
  void acc_mllt_stats_post(KModel& m, KTransitions& tm, khg::PyDevicePosteriors& post, KMlltStats& stats, float scale) {
    if (!post.h) throw py::value_error("acc_mllt_stats_post: the DevicePosteriors are closed");
    Check(NoGil([&] { return khg_acc_mllt_stats_post(ctx->h, m.h, tm.h, h, post.h, scale, stats.h); }));
  }
  // acc-lda (khg_acc_lda_stats_post): no model, the transition model names the class
  void acc_lda_stats_post(KTransitions& tm, khg::PyDevicePosteriors& post, KLdaStats& stats, float scale) {
    if (!post.h) throw py::value_error("acc_lda_stats_post: the DevicePosteriors are closed");
    Check(NoGil([&] { return khg_acc_lda_stats_post(ctx->h, tm.h, h, post.h, scale, stats.h); }));
  }
  // acc-tree-stats (khg_acc_tree_stats): from the resident alignment; the tables are [num_tids + 1], index 0 unused -> status [n_utt]
  py::object acc_tree_stats(Arr<int32_t> tid2phone, Arr<int32_t> tid2pdf_class, Arr<int32_t> tid_flags, Arr<int32_t> ci_phones, KTreeStats& stats) {
    if (tid2phone.size() < 2 || tid2pdf_class.size() != tid2phone.size() || tid_flags.size() != tid2phone.size())
      throw py::value_error("acc_tree_stats: tid2phone, tid2pdf_class and tid_flags must be [num_tids + 1]");
    Arr<int32_t> status({(py::ssize_t)(n_utt > 0 ? n_utt : 1)});
    Check(NoGil([&] { return khg_acc_tree_stats(ctx->h, h, (int32_t)tid2phone.size() - 1, tid2phone.data(), tid2pdf_class.data(), tid_flags.data(), (int32_t)ci_phones.size(),
                                                ci_phones.data(), stats.h, status.mutable_data()); }));
    return py::array(status)[py::slice(0, n_utt, 1)];
  }
  // splice-feats | transform-feats (khg_utts_splice_transform_feats): M [out_dim, dim_z (+ 1)] from the host, or None for the spliced
  // rows themselves; out: a device pointer for [rows, out_dim] floats
  void splice_transform_feats(int left, int right, py::object M, uintptr_t out) {
    if (left < 0 || right < 0) throw py::value_error("splice_transform_feats: left and right must be >= 0");
    const int dz = dim * (left + right + 1);
    Arr<float> ma;
    const float* mh = nullptr;
    int out_dim = dz, has_offset = 0;
    if (!M.is_none()) {
      ma = M.cast<Arr<float>>();
      if (ma.ndim() != 2 || (ma.shape(1) != dz && ma.shape(1) != dz + 1) || ma.shape(0) < 1)
        throw py::value_error("splice_transform_feats: M must be [out_dim, dim (left + right + 1)] or one column more");
      out_dim = (int)ma.shape(0); has_offset = ma.shape(1) == dz + 1; mh = ma.data();
    }
    Check(NoGil([&] { return khg_utts_splice_transform_feats(ctx->h, h, left, right, out_dim, has_offset, mh, reinterpret_cast<float*>(out)); }));
  }
  // transform-feats (khg_utts_transform_feats): W [n_spk, dim, dim + 1] from the host or, as an integer, a device pointer; out: a device
  // pointer for the transformed rows, or None for the set's own rows in place
  void transform_feats(Arr<int32_t> utt2spk, py::object W, py::object out, int n_spk) {
    if (utt2spk.size() != n_utt) throw py::value_error("transform_feats: one speaker per utterance");
    const float *wh = nullptr, *wd = nullptr;
    Arr<float> wa;
    if (py::isinstance<py::int_>(W)) {
      if (n_spk < 1) throw py::value_error("transform_feats: n_spk is required with a device pointer");
      wd = reinterpret_cast<const float*>(W.cast<uintptr_t>());
    } else {
      wa = W.cast<Arr<float>>();
      if (wa.ndim() != 3 || wa.shape(1) != dim || wa.shape(2) != dim + 1) throw py::value_error("transform_feats: W must be [n_spk, dim, dim + 1]");
      n_spk = (int)wa.shape(0);
      wh = wa.data();
    }
    float* od = out.is_none() ? nullptr : reinterpret_cast<float*>(out.cast<uintptr_t>());
    Check(NoGil([&] { return khg_utts_transform_feats(ctx->h, h, n_spk, utt2spk.data(), wh, wd, od); }));
  }
  // compute-cmvn-stats (khg_acc_cmvn_stats): one speaker number per utterance (< 0: none)
  void acc_cmvn_stats(Arr<int32_t> utt2spk, KCmvnStats& stats) {
    if (utt2spk.size() != n_utt) throw py::value_error("acc_cmvn_stats: one speaker per utterance");
    if (!stats.h) throw py::value_error("acc_cmvn_stats: the DeviceCmvnStats are closed");
    Check(NoGil([&] { return khg_acc_cmvn_stats(ctx->h, h, utt2spk.data(), stats.h); }));
  }
  // the normaliser arguments of apply_cmvn / add_deltas: norm [n_spk, 2, dim], one speaker per utterance, status [n_spk] or None
  void norm_args(const char* who, const Arr<float>& norm, const Arr<int32_t>& utt2spk, const py::object& status, Arr<int32_t>* st, const int32_t** sp) {
    if (norm.ndim() != 3 || norm.shape(1) != 2 || norm.shape(2) != dim) throw py::value_error(std::string(who) + ": norm must be [n_spk, 2, dim]");
    if (utt2spk.size() != n_utt) throw py::value_error(std::string(who) + ": one speaker per utterance");
    *sp = nullptr;
    if (!status.is_none()) {
      *st = status.cast<Arr<int32_t>>();
      if (st->size() != norm.shape(0)) throw py::value_error(std::string(who) + ": one status per speaker");
      *sp = st->data();
    }
  }
  // apply-cmvn (khg_utts_apply_cmvn): out: a device pointer for the normalised rows, or None for the set's own rows in place
  void apply_cmvn(Arr<int32_t> utt2spk, Arr<float> norm, py::object status, py::object out) {
    Arr<int32_t> st;
    const int32_t* sp = nullptr;
    norm_args("apply_cmvn", norm, utt2spk, status, &st, &sp);
    float* od = out.is_none() ? nullptr : reinterpret_cast<float*>(out.cast<uintptr_t>());
    Check(NoGil([&] { return khg_utts_apply_cmvn(ctx->h, h, (int32_t)norm.shape(0), utt2spk.data(), norm.data(), sp, od); }));
  }
  // add-deltas (khg_utts_add_deltas): out: a device pointer for [rows, dim (order + 1)] floats; norm None: no CMVN
  void add_deltas(int order, int window, uintptr_t out, py::object norm, py::object utt2spk, py::object status) {
    if (norm.is_none()) {
      Check(NoGil([&] { return khg_utts_add_deltas(ctx->h, h, order, window, 0, nullptr, nullptr, nullptr, reinterpret_cast<float*>(out)); }));
      return;
    }
    if (utt2spk.is_none()) throw py::value_error("add_deltas: a normaliser needs utt2spk");
    Arr<float> na = norm.cast<Arr<float>>();
    Arr<int32_t> ua = utt2spk.cast<Arr<int32_t>>(), st;
    const int32_t* sp = nullptr;
    norm_args("add_deltas", na, ua, status, &st, &sp);
    Check(NoGil([&] { return khg_utts_add_deltas(ctx->h, h, order, window, (int32_t)na.shape(0), ua.data(), na.data(), sp, reinterpret_cast<float*>(out)); }));
  }
};

}  // namespace

void BindHost(py::module_& m, py::object* error_class);      // khg_py_host.cpp: the host classes behind the reference's names

PYBIND11_MODULE(_kaldi_hmm_gmm_amd, m) {
  m.doc() = "pybind11 host surface of libkhg_hip.so (include/khg_hip.h): the accelerated EM hot path of kaldi-hmm-gmm on MI355X";
  m.def("_set_error_class", [](py::object cls) { g_khg_error = cls; });
  BindHost(m, &g_khg_error);
  m.def("version", [] { return khg_version(); });
  // khg_k3_forms: the library's table of K3 accumulate instantiations, one dict per row (no context, no device)
  m.def("k3_forms", [] {
    int32_t n = 0;
    Check(khg_k3_forms(nullptr, 0, &n));
    std::vector<int32_t> rows((size_t)6 * n);
    Check(khg_k3_forms(rows.data(), n, &n));
    py::list out;
    for (int i = 0; i < n; ++i) {
      const int32_t* o = rows.data() + 6 * (size_t)i;
      py::dict d;
      d["variant"] = K3VariantName(o[0]); d["KQ"] = o[1]; d["NB"] = o[2]; d["waves"] = o[3]; d["POST"] = o[4] != 0; d["f16a"] = o[5] != 0;
      out.append(d);
    }
    return out;
  });
  m.attr("ALIGN_DONE") = KHG_ALIGN_DONE; m.attr("ALIGN_ERROR") = KHG_ALIGN_ERROR; m.attr("ALIGN_RETRIED") = KHG_ALIGN_RETRIED;
  m.attr("ALIGN_EXACT_DP") = KHG_ALIGN_EXACT_DP; m.attr("ALIGN_FALLBACK") = KHG_ALIGN_FALLBACK;

  py::class_<KContext>(m, "Context")
      .def(py::init<int, py::object>(), py::arg("device") = 0, py::arg("stream") = py::none())
      .def_property_readonly("h", [](KContext& c) { return reinterpret_cast<uintptr_t>(c.h); })
      .def_readonly("device", &KContext::device)
      .def("sync", &KContext::sync).def("set_timing", &KContext::set_timing).def("timings", &KContext::timings)
      .def("set_k1_form", &KContext::set_k1_form).def("set_option", &KContext::set_option, py::arg("name"), py::arg("value"))
      .def("get_option", &KContext::get_option, py::arg("name")).def("close", &KContext::close);

  py::class_<KComm>(m, "Comm")
      .def_static("unique_id", &KComm::unique_id)
      .def(py::init<KContext&, int, int, py::bytes>(), py::arg("ctx"), py::arg("nranks"), py::arg("rank"), py::arg("uid"), py::keep_alive<1, 2>())
      .def_property_readonly("h", [](KComm& c) { return reinterpret_cast<uintptr_t>(c.h); })
      .def_readonly("nranks", &KComm::nranks).def_readonly("rank", &KComm::rank).def("close", &KComm::close).def("info", &KComm::info)
      .def_property_readonly_static("ID_BYTES", [](py::object) { return KHG_COMM_ID_BYTES; });

  py::class_<KModel>(m, "DeviceModel")
      .def(py::init<py::object, Arr<int32_t>, Arr<float>, Arr<float>, Arr<float>, py::object>(), py::arg("ctx"), py::arg("gauss_off"),
           py::arg("gconsts"), py::arg("means_invvars"), py::arg("inv_vars"), py::arg("weights") = py::none())
      .def_property_readonly("h", [](KModel& x) { return reinterpret_cast<uintptr_t>(x.h); })
      .def_readonly("ctx", &KModel::ctx_obj).def_readonly("num_pdfs", &KModel::num_pdfs).def_readonly("dim", &KModel::dim)
      .def_readonly("gauss_off", &KModel::gauss_off)
      .def("set_weights", &KModel::set_weights)
      .def("mle_update", &KModel::mle_update, py::arg("accs"), py::arg("opts") = py::none(), py::arg("flags") = 0x7)
      .def("mle_update_sharded", &KModel::mle_update_sharded, py::arg("accs"), py::arg("opts") = py::none(), py::arg("flags") = 0x7,
           py::arg("comm") = py::none())
      .def("mle_update_range", &KModel::mle_update_range, py::arg("accs"), py::arg("opts"), py::arg("flags"), py::arg("first_pdf"), py::arg("n_pdf"))
      .def("mle_rows_download", &KModel::mle_rows_download).def("mle_rows_upload", &KModel::mle_rows_upload)
      .def("mle_update_finish", &KModel::mle_update_finish)
      .def("ebw_update", &KModel::ebw_update, py::arg("num_accs"), py::arg("den_accs"), py::arg("opts") = py::none(),
           py::arg("weight_opts") = py::none(), py::arg("flags") = 0x7)
      .def("scale_weights", &KModel::scale_weights)
      .def("invalidate", &KModel::invalidate)
      .def("transform_means", &KModel::transform_means, py::arg("M"))
      .def("split", &KModel::split, py::arg("targets"), py::arg("perturb_factor"), py::arg("randn"))
      .def("merge", &KModel::merge, py::arg("targets"))
      .def("download", &KModel::download, py::arg("weights") = true)
      .def("close", &KModel::close);

  py::class_<KTransitions>(m, "DeviceTransitions")
      .def(py::init<py::object, Arr<int32_t>>(), py::arg("ctx"), py::arg("id2pdf"))
      .def_property_readonly("h", [](KTransitions& x) { return reinterpret_cast<uintptr_t>(x.h); })
      .def_readonly("ctx", &KTransitions::ctx_obj).def_readonly("id2pdf", &KTransitions::id2pdf).def_readonly("num_tids", &KTransitions::num_tids)
      .def("set_trans_cost", &KTransitions::set_trans_cost).def("close", &KTransitions::close);

  py::class_<KAccs>(m, "DeviceAccs")
      .def(py::init<py::object, KModel&, KTransitions&>(), py::arg("ctx"), py::arg("model"), py::arg("tm"))
      .def_property_readonly("h", [](KAccs& x) { return reinterpret_cast<uintptr_t>(x.h); })
      .def_readonly("ctx", &KAccs::ctx_obj).def_readonly("sumG", &KAccs::sumG).def_readonly("dim", &KAccs::dim)
      .def_readonly("num_tids", &KAccs::num_tids).def_readonly("size", &KAccs::size)
      .def("zero", &KAccs::zero).def("device_ptr", &KAccs::device_ptr)
      .def("allreduce", &KAccs::allreduce, py::arg("comm") = py::none(), py::arg("wire_fp32") = false)
      .def("allreduce_range", &KAccs::allreduce_range, py::arg("model"), py::arg("first_pdf"), py::arg("n_pdf"), py::arg("comm") = py::none())
      .def("split", &KAccs::split).def("relayout", &KAccs::relayout).def("download_range", &KAccs::download_range)
      .def("download_occ", [](KAccs& a) { return a.download_range(0, a.sumG); })
      .def("download_trans", &KAccs::download_trans).def("download", &KAccs::download).def("upload", &KAccs::upload)
      .def("add", &KAccs::add, py::arg("scale"), py::arg("src")).def("scale", &KAccs::scale, py::arg("f"))
      .def("smooth_with_accum", &KAccs::smooth_with_accum, py::arg("tau"), py::arg("src"), py::arg("model"), py::arg("count") = true)
      .def("close", &KAccs::close);

  py::class_<KUtts>(m, "UtteranceSet")
      .def(py::init<py::object, py::object, Arr<int64_t>, py::object, py::object, py::object, py::object>(), py::arg("ctx"), py::arg("tm"), py::arg("frame_off"),
           py::arg("feats"), py::arg("dim") = py::none(), py::arg("graphs") = py::none(), py::arg("graph") = py::none())
      .def_property_readonly("graph_bytes", [](KUtts& x) { int64_t b = 0; Check(khg_utts_graph_bytes(x.h, &b)); return b; })
      .def_property_readonly("h", [](KUtts& x) { return reinterpret_cast<uintptr_t>(x.h); })
      .def_readonly("ctx", &KUtts::ctx_obj).def_readonly("frame_off", &KUtts::frame_off).def_readonly("n_utt", &KUtts::n_utt)
      .def_readonly("dim", &KUtts::dim)
      .def("set_pdf_list", &KUtts::set_pdf_list).def("features_changed", &KUtts::features_changed).def("pdf_lists", &KUtts::pdf_lists).def("k2_plan", &KUtts::k2_plan, py::arg("ctx")).def("k2_ladder", &KUtts::k2_ladder, py::arg("ctx")).def("k3_planes", &KUtts::k3_planes).def("k3_last", &KUtts::k3_last).def("k1_last", &KUtts::k1_last).def("k2_tail", &KUtts::k2_tail).def("pdf_first_frames", &KUtts::pdf_first_frames)
      .def("pdf_last_frames", &KUtts::pdf_last_frames)
      .def("loglikes", &KUtts::loglikes, py::arg("model"), py::arg("reachable_only") = false, py::arg("band") = false)
      .def("loglikes_layout", &KUtts::loglikes_layout).def("download_loglikes", &KUtts::download_loglikes)
      .def("upload_loglikes", &KUtts::upload_loglikes)
      .def("align", &KUtts::align, py::arg("tm"), py::arg("beam") = 200.0f, py::arg("retry_beam") = 0.0f, py::arg("acoustic_scale") = 1.0f,
           py::arg("careful") = false, py::arg("max_active") = (int64_t)std::numeric_limits<int32_t>::max(), py::arg("min_active") = 20,
           py::arg("beam_delta") = 0.5f, py::arg("hash_ratio") = 2.0f, py::arg("download") = true)
      .def("decode_lattice_faster", &KUtts::decode_lattice_faster, py::arg("tm"), py::arg("beam") = 16.0f,
           py::arg("max_active") = std::numeric_limits<int32_t>::max(), py::arg("min_active") = 200, py::arg("lattice_beam") = 10.0f,
           py::arg("prune_interval") = 25, py::arg("beam_delta") = 0.5f, py::arg("hash_ratio") = 2.0f, py::arg("prune_scale") = 0.1f,
           py::arg("acoustic_scale") = 1.0f, py::arg("allow_partial") = true, py::arg("scratch_per_frame") = 0)
      .def("raw_lattice_faster", &KUtts::raw_lattice_faster, py::arg("tm"), py::arg("beam") = 16.0f,
           py::arg("max_active") = std::numeric_limits<int32_t>::max(), py::arg("min_active") = 200, py::arg("lattice_beam") = 10.0f,
           py::arg("prune_interval") = 25, py::arg("beam_delta") = 0.5f, py::arg("hash_ratio") = 2.0f, py::arg("prune_scale") = 0.1f,
           py::arg("acoustic_scale") = 1.0f, py::arg("allow_partial") = true, py::arg("scratch_per_frame") = 0)
      .def("raw_lattices_faster_device", &KUtts::raw_lattices_faster_device, py::arg("tm"), py::arg("beam") = 16.0f,
           py::arg("max_active") = std::numeric_limits<int32_t>::max(), py::arg("min_active") = 200, py::arg("lattice_beam") = 10.0f,
           py::arg("prune_interval") = 25, py::arg("beam_delta") = 0.5f, py::arg("hash_ratio") = 2.0f, py::arg("prune_scale") = 0.1f,
           py::arg("acoustic_scale") = 1.0f, py::arg("allow_partial") = true, py::arg("scratch_per_frame") = 0)
      .def("decode_lattice_simple", &KUtts::decode_lattice_simple, py::arg("tm"), py::arg("beam") = 16.0f, py::arg("lattice_beam") = 10.0f,
           py::arg("prune_interval") = 25, py::arg("prune_scale") = 0.1f, py::arg("acoustic_scale") = 1.0f, py::arg("allow_partial") = true,
           py::arg("scratch_per_frame") = 0)
      .def("raw_lattice_simple", &KUtts::raw_lattice_simple, py::arg("tm"), py::arg("beam") = 16.0f, py::arg("lattice_beam") = 10.0f,
           py::arg("prune_interval") = 25, py::arg("prune_scale") = 0.1f, py::arg("acoustic_scale") = 1.0f, py::arg("scratch_per_frame") = 0)
      .def("raw_lattices_simple_device", &KUtts::raw_lattices_simple_device, py::arg("tm"), py::arg("beam") = 16.0f, py::arg("lattice_beam") = 10.0f,
           py::arg("prune_interval") = 25, py::arg("prune_scale") = 0.1f, py::arg("acoustic_scale") = 1.0f, py::arg("scratch_per_frame") = 0)
      .def("upload_ali", &KUtts::upload_ali).def("download_ali", &KUtts::download_ali)
      .def("acc_stats", &KUtts::acc_stats, py::arg("model"), py::arg("tm"), py::arg("accs"), py::arg("weight") = 1.0f)
      .def("acc_stats_post", &KUtts::acc_stats_post, py::arg("model"), py::arg("tm"), py::arg("post"), py::arg("accs"), py::arg("scale") = 1.0f)
      .def("acc_stats_post2", &KUtts::acc_stats_post2, py::arg("model"), py::arg("tm"), py::arg("post"), py::arg("num_accs"), py::arg("den_accs"),
           py::arg("scale") = 1.0f)
      .def("acc_stats_reduce", &KUtts::acc_stats_reduce, py::arg("model"), py::arg("tm"), py::arg("accs"), py::arg("weight") = 1.0f,
           py::arg("comm") = py::none(), py::arg("nparts") = 4)
      .def("acc_fmllr_stats_post", &KUtts::acc_fmllr_stats_post, py::arg("model"), py::arg("tm"), py::arg("post"), py::arg("utt2spk"), py::arg("stats"),
           py::arg("scale") = 1.0f)
      .def("acc_mllt_stats_post", &KUtts::acc_mllt_stats_post, py::arg("model"), py::arg("tm"), py::arg("post"), py::arg("stats"), py::arg("scale") = 1.0f)
      .def("acc_lda_stats_post", &KUtts::acc_lda_stats_post, py::arg("tm"), py::arg("post"), py::arg("stats"), py::arg("scale") = 1.0f)
      .def("_acc_tree_stats", &KUtts::acc_tree_stats, py::arg("tid2phone"), py::arg("tid2pdf_class"), py::arg("tid_flags"), py::arg("ci_phones"), py::arg("stats"))
      .def("splice_transform_feats", &KUtts::splice_transform_feats, py::arg("left"), py::arg("right"), py::arg("M"), py::arg("out"))
      .def("transform_feats", &KUtts::transform_feats, py::arg("utt2spk"), py::arg("W"), py::arg("out") = py::none(), py::arg("n_spk") = 0)
      .def("acc_cmvn_stats", &KUtts::acc_cmvn_stats, py::arg("utt2spk"), py::arg("stats"))
      .def("apply_cmvn", &KUtts::apply_cmvn, py::arg("utt2spk"), py::arg("norm"), py::arg("status") = py::none(), py::arg("out") = py::none())
      .def("add_deltas", &KUtts::add_deltas, py::arg("order"), py::arg("window"), py::arg("out"), py::arg("norm") = py::none(), py::arg("utt2spk") = py::none(),
           py::arg("status") = py::none())
      .def("close", &KUtts::close);

  py::class_<KFmllrStats>(m, "DeviceFmllrStats")
      .def(py::init<py::object, int, int>(), py::arg("ctx"), py::arg("n_spk"), py::arg("dim"))
      .def_property_readonly("h", [](KFmllrStats& x) { return reinterpret_cast<uintptr_t>(x.h); })
      .def_readonly("ctx", &KFmllrStats::ctx_obj).def_readonly("n_spk", &KFmllrStats::n_spk).def_readonly("dim", &KFmllrStats::dim)
      .def("zero", &KFmllrStats::zero).def("download", &KFmllrStats::download)
      .def("upload", &KFmllrStats::upload, py::arg("beta"), py::arg("K"), py::arg("G"))
      .def("add", &KFmllrStats::add, py::arg("scale"), py::arg("src"))
      .def("estimate", &KFmllrStats::estimate, py::arg("min_count") = 500.0, py::arg("num_iters") = 40, py::arg("W_d") = py::none())
      .def("set_chunk_frames", &KFmllrStats::set_chunk_frames, py::arg("frames")).def("num_chunks", &KFmllrStats::num_chunks)
      .def("close", &KFmllrStats::close);

  py::class_<KMlltStats>(m, "DeviceMlltStats")
      .def(py::init<py::object, int>(), py::arg("ctx"), py::arg("dim"))
      .def_property_readonly("h", [](KMlltStats& x) { return reinterpret_cast<uintptr_t>(x.h); })
      .def_readonly("ctx", &KMlltStats::ctx_obj).def_readonly("dim", &KMlltStats::dim)
      .def("zero", &KMlltStats::zero).def("download", &KMlltStats::download)
      .def("upload", &KMlltStats::upload, py::arg("beta"), py::arg("G"))
      .def("add", &KMlltStats::add, py::arg("scale"), py::arg("src"))
      .def("set_chunk_frames", &KMlltStats::set_chunk_frames, py::arg("frames")).def("num_chunks", &KMlltStats::num_chunks)
      .def("close", &KMlltStats::close);

  py::class_<KLdaStats>(m, "DeviceLdaStats")
      .def(py::init<py::object, int, int, int, int>(), py::arg("ctx"), py::arg("num_classes"), py::arg("dim"), py::arg("left") = 4, py::arg("right") = 4)
      .def_property_readonly("h", [](KLdaStats& x) { return reinterpret_cast<uintptr_t>(x.h); })
      .def_readonly("ctx", &KLdaStats::ctx_obj).def_readonly("num_classes", &KLdaStats::num_classes).def_readonly("dim", &KLdaStats::dim)
      .def_readonly("left", &KLdaStats::left).def_readonly("right", &KLdaStats::right).def_readonly("dim_z", &KLdaStats::dim_z)
      .def("zero", &KLdaStats::zero).def("download", &KLdaStats::download)
      .def("upload", &KLdaStats::upload, py::arg("zero_acc"), py::arg("first_acc"), py::arg("total_second_acc"))
      .def("add", &KLdaStats::add, py::arg("scale"), py::arg("src"))
      .def("set_chunk_frames", &KLdaStats::set_chunk_frames, py::arg("frames")).def("num_chunks", &KLdaStats::num_chunks)
      .def("close", &KLdaStats::close);

  py::class_<KCmvnStats>(m, "DeviceCmvnStats")
      .def(py::init<py::object, int, int>(), py::arg("ctx"), py::arg("n_spk"), py::arg("dim"))
      .def_property_readonly("h", [](KCmvnStats& x) { return reinterpret_cast<uintptr_t>(x.h); })
      .def_readonly("ctx", &KCmvnStats::ctx_obj).def_readonly("n_spk", &KCmvnStats::n_spk).def_readonly("dim", &KCmvnStats::dim)
      .def("zero", &KCmvnStats::zero).def("download", &KCmvnStats::download)
      .def("upload", &KCmvnStats::upload, py::arg("stats"))
      .def("add", &KCmvnStats::add, py::arg("scale"), py::arg("src"))
      .def("set_chunk_frames", &KCmvnStats::set_chunk_frames, py::arg("frames")).def("num_chunks", &KCmvnStats::num_chunks)
      .def("close", &KCmvnStats::close);

  py::class_<KTreeStats>(m, "DeviceTreeStats", py::dynamic_attr())
      .def(py::init<py::object, int, int, int>(), py::arg("ctx"), py::arg("dim"), py::arg("N") = 3, py::arg("P") = 1)
      .def_property_readonly("h", [](KTreeStats& x) { return reinterpret_cast<uintptr_t>(x.h); })
      .def_readonly("ctx", &KTreeStats::ctx_obj).def_readonly("dim", &KTreeStats::dim).def_readonly("N", &KTreeStats::N).def_readonly("P", &KTreeStats::P)
      .def("zero", &KTreeStats::zero).def("num_keys", &KTreeStats::num_keys).def("download", &KTreeStats::download)
      .def("upload", &KTreeStats::upload, py::arg("keys"), py::arg("count"), py::arg("x"), py::arg("x2"))
      .def("add", &KTreeStats::add, py::arg("scale"), py::arg("src"))
      .def("close", &KTreeStats::close);

  // ---- host-side functions (no GPU): gconsts, M-step, merge, transition update, AddTransitionProbs costs ----
  m.def("compute_gconsts", [](Arr<int32_t> go, Arr<float> w, Arr<float> iv, Arr<float> miv) {
    const int P = (int)go.shape(0) - 1;
    Arr<float> gc({w.shape(0)});
    int32_t bad = 0;
    Check(khg_compute_gconsts(P, (int)iv.shape(1), go.data(), w.data(), iv.data(), miv.data(), gc.mutable_data(), &bad));
    return py::make_tuple(gc, bad);
  }, "DiagGmm::ComputeGconsts (csrc/diag-gmm.cc:103-147) over a ragged model -> (gconsts, num_bad)");
  m.def("diag_gmm_merge", [](Arr<float> w, Arr<float> miv, Arr<float> iv, int target) {
    int32_t G = (int32_t)w.shape(0), nh = 0;
    const int D = (int)miv.shape(1);
    Arr<float> w2 = py::array(w).attr("copy")(), miv2 = py::array(miv).attr("copy")(), iv2 = py::array(iv).attr("copy")();
    Arr<float> gc({(py::ssize_t)G});
    std::vector<int32_t> hist((size_t)2 * (G > 0 ? G : 1));
    Check(khg_diag_gmm_merge(&G, D, target, w2.mutable_data(), gc.mutable_data(), miv2.mutable_data(), iv2.mutable_data(), hist.data(), &nh));
    hist.resize((size_t)nh);
    py::dict d;
    d["num_gauss"] = G; d["weights"] = w2; d["gconsts"] = gc; d["means_invvars"] = miv2; d["inv_vars"] = iv2; d["history"] = hist;
    return d;
  }, "DiagGmm::Merge (csrc/diag-gmm.cc:557-759): the first num_gauss rows of the returned arrays are the merged model");
  m.def("fmllr_compute", [](Arr<double> beta, Arr<double> K, Arr<double> G, double min_count, int num_iters) {
    if (K.ndim() != 3 || G.ndim() != 3 || K.shape(0) != beta.shape(0) || G.shape(0) != beta.shape(0) || K.shape(2) != K.shape(1) + 1 ||
        G.shape(1) != K.shape(1) || G.shape(2) != (K.shape(1) + 1) * (K.shape(1) + 2) / 2)
      throw py::value_error("fmllr_compute: beta [n_spk], K [n_spk, dim, dim + 1], G [n_spk, dim, (dim + 1)(dim + 2) / 2]");
    const py::ssize_t S = beta.shape(0), D = K.shape(1);
    khg_fmllr_options o;
    khg_fmllr_options_default(&o);
    o.min_count = min_count; o.num_iters = num_iters;
    Arr<float> W({S, D, D + 1});
    Arr<double> W64({S, D, D + 1}), impr({S}), count({S});
    Arr<int32_t> status({S});
    Check(NoGil([&] { return khg_fmllr_compute(&o, (int32_t)S, (int32_t)D, beta.data(), K.data(), G.data(), W.mutable_data(), W64.mutable_data(),
                                               impr.mutable_data(), count.mutable_data(), status.mutable_data()); }));
    py::dict d;
    d["W"] = W; d["W64"] = W64; d["objf_impr"] = impr; d["count"] = count; d["status"] = status;
    return d;
  }, py::arg("beta"), py::arg("K"), py::arg("G"), py::arg("min_count") = 500.0, py::arg("num_iters") = 40,
     "ComputeFmllrMatrixDiagGmmFull per speaker on host statistics (khg_fmllr_compute; DESIGN.md 7l)");
  m.attr("FMLLR_OK") = KHG_FMLLR_OK; m.attr("FMLLR_LOW_COUNT") = KHG_FMLLR_LOW_COUNT; m.attr("FMLLR_SINGULAR") = KHG_FMLLR_SINGULAR;
  m.attr("FMLLR_MAX_DIM") = KHG_FMLLR_MAX_DIM;
  m.def("mllt_compute", [](double beta, Arr<double> G, int num_iters) {
    if (G.ndim() != 2 || G.shape(0) < 1 || G.shape(1) != G.shape(0) * (G.shape(0) + 1) / 2)
      throw py::value_error("mllt_compute: beta, G [dim, dim (dim + 1) / 2]");
    const py::ssize_t D = G.shape(0);
    khg_mllt_options o;
    khg_mllt_options_default(&o);
    o.num_iters = num_iters;
    Arr<float> M({D, D});
    Arr<double> M64({D, D});
    double impr = 0.0, count = 0.0;
    int32_t status = 0;
    Check(NoGil([&] { return khg_mllt_compute(&o, (int32_t)D, beta, G.data(), M.mutable_data(), M64.mutable_data(), &impr, &count, &status); }));
    py::dict d;
    d["M"] = M; d["M64"] = M64; d["objf_impr"] = impr; d["count"] = count; d["status"] = (int)status;
    return d;
  }, py::arg("beta"), py::arg("G"), py::arg("num_iters") = 200, "MlltAccs::Update on host statistics (khg_mllt_compute; DESIGN.md 7m)");
  m.attr("MLLT_OK") = KHG_MLLT_OK; m.attr("MLLT_SINGULAR") = KHG_MLLT_SINGULAR; m.attr("MLLT_MAX_DIM") = KHG_MLLT_MAX_DIM;
  m.def("lda_compute", [](Arr<double> zero, Arr<double> first, Arr<double> second, int target_dim, bool remove_offset, double within_class_factor) {
    if (first.ndim() != 2 || zero.ndim() != 1 || second.ndim() != 1 || first.shape(0) != zero.shape(0) || first.shape(0) < 1 || first.shape(1) < 1 ||
        second.shape(0) != first.shape(1) * (first.shape(1) + 1) / 2)
      throw py::value_error("lda_compute: zero_acc [num_classes], first_acc [num_classes, dim_z], total_second_acc [dim_z (dim_z + 1) / 2]");
    const py::ssize_t C = first.shape(0), n = first.shape(1);
    khg_lda_options o;
    khg_lda_options_default(&o);
    o.target_dim = target_dim; o.remove_offset = remove_offset ? 1 : 0; o.within_class_factor = within_class_factor;
    if (target_dim < 1 || target_dim > n) throw py::value_error("lda_compute: target_dim must be in 1 .. dim_z");
    const py::ssize_t MW = n + (remove_offset ? 1 : 0);
    Arr<float> M({(py::ssize_t)target_dim, MW});
    Arr<double> M64({(py::ssize_t)target_dim, MW}), Mfull({n, n}), eig({n});
    double count = 0.0;
    int32_t status = 0;
    Check(NoGil([&] { return khg_lda_compute(&o, (int32_t)C, (int32_t)n, zero.data(), first.data(), second.data(), M.mutable_data(), M64.mutable_data(),
                                             Mfull.mutable_data(), eig.mutable_data(), &count, &status); }));
    py::dict d;
    d["M"] = M; d["M64"] = M64; d["M_full"] = Mfull; d["eig"] = eig; d["count"] = count; d["status"] = (int)status;
    return d;
  }, py::arg("zero_acc"), py::arg("first_acc"), py::arg("total_second_acc"), py::arg("target_dim") = 40, py::arg("remove_offset") = false,
     py::arg("within_class_factor") = 1.0, "LdaEstimate::Estimate on host statistics (khg_lda_compute; DESIGN.md 7n)");
  m.attr("LDA_OK") = KHG_LDA_OK; m.attr("LDA_SINGULAR") = KHG_LDA_SINGULAR; m.attr("LDA_MAX_SPLICED_DIM") = KHG_LDA_MAX_SPLICED_DIM;
  m.def("cmvn_compute", [](Arr<double> stats, bool norm_means, bool norm_vars, bool reverse) {
    if (stats.ndim() != 3 || stats.shape(1) != 2 || stats.shape(2) < 2) throw py::value_error("cmvn_compute: stats [n_spk, 2, dim + 1]");
    const py::ssize_t S = stats.shape(0), D = stats.shape(2) - 1;
    Arr<float> norm({S, (py::ssize_t)2, D});
    Arr<int32_t> status({S});
    Check(NoGil([&] { return khg_cmvn_compute((int32_t)S, (int32_t)D, stats.data(), norm_means ? 1 : 0, norm_vars ? 1 : 0, reverse ? 1 : 0, norm.mutable_data(),
                                              status.mutable_data()); }));
    py::dict d;
    d["norm"] = norm; d["status"] = status;
    return d;
  }, py::arg("stats"), py::arg("norm_means") = true, py::arg("norm_vars") = false, py::arg("reverse") = false,
     "ApplyCmvn's offsets and scales from host statistics (khg_cmvn_compute; DESIGN.md 7p)");
  m.def("delta_scales", [](int order, int window) {
    if (order < 0 || window < 1) throw py::value_error("delta_scales: order must be >= 0 and window >= 1");
    std::vector<float> flat((size_t)(order + 1) + (size_t)window * order * (order + 1));
    Check(khg_delta_scales(order, window, flat.data()));
    py::list out;
    for (int i = 0; i <= order; ++i) {
      Arr<float> a({(py::ssize_t)(2 * i * window + 1)});
      std::memcpy(a.mutable_data(), flat.data() + i + (size_t)window * i * (i - 1), sizeof(float) * (size_t)a.size());
      out.append(a);
    }
    return out;
  }, py::arg("order"), py::arg("window"), "DeltaFeatures' coefficient tables, one float32 array per order 0 .. order (khg_delta_scales; DESIGN.md 7p)");
  m.attr("CMVN_OK") = KHG_CMVN_OK; m.attr("CMVN_NO_DATA") = KHG_CMVN_NO_DATA; m.attr("CMVN_NONFINITE") = KHG_CMVN_NONFINITE;
  m.attr("FEAT_TILE_LDS_BYTES") = KHG_FEAT_TILE_LDS_BYTES;
  // the waveform front end
  py::class_<khg_frontend_opts>(m, "FrontendOptions", "Kaldi's MFCC / filterbank options (khg_frontend_opts); keyword arguments set fields")
      .def(py::init([](py::kwargs kw) {
        khg_frontend_opts o;
        khg_frontend_opts_default(&o);
        py::object po = py::cast(&o, py::return_value_policy::reference);
        for (auto kv : kw) py::setattr(po, kv.first, kv.second);
        return o;
      }))
      .def("copy", [](const khg_frontend_opts& o) { return o; })
#define FE_FIELD(f) .def_readwrite(#f, &khg_frontend_opts::f)
      FE_FIELD(kind) FE_FIELD(samp_freq) FE_FIELD(frame_length_ms) FE_FIELD(frame_shift_ms) FE_FIELD(preemph_coeff) FE_FIELD(remove_dc_offset)
      FE_FIELD(window_type) FE_FIELD(blackman_coeff) FE_FIELD(snip_edges) FE_FIELD(round_to_power_of_two) FE_FIELD(dither) FE_FIELD(num_mel_bins)
      FE_FIELD(low_freq) FE_FIELD(high_freq) FE_FIELD(vtln_warp) FE_FIELD(htk_compat) FE_FIELD(num_ceps) FE_FIELD(cepstral_lifter) FE_FIELD(use_energy)
      FE_FIELD(raw_energy) FE_FIELD(energy_floor) FE_FIELD(use_log_fbank) FE_FIELD(use_power);
#undef FE_FIELD
  m.attr("FE_MFCC") = KHG_FE_MFCC; m.attr("FE_FBANK") = KHG_FE_FBANK; m.attr("FE_TILE_FRAMES") = KHG_FE_TILE_FRAMES;
  m.attr("WIN_POVEY") = KHG_WIN_POVEY; m.attr("WIN_HAMMING") = KHG_WIN_HAMMING; m.attr("WIN_HANNING") = KHG_WIN_HANNING;
  m.attr("WIN_RECTANGULAR") = KHG_WIN_RECTANGULAR; m.attr("WIN_BLACKMAN") = KHG_WIN_BLACKMAN;
  m.attr("WAVE_F32") = KHG_WAVE_F32; m.attr("WAVE_I16") = KHG_WAVE_I16;
  m.def("frontend_dims", [](const khg_frontend_opts& o) {
    int32_t d[8];
    Check(khg_frontend_dims(&o, d));
    py::dict r;
    r["L"] = d[0]; r["S"] = d[1]; r["N"] = d[2]; r["num_mel_bins"] = d[3]; r["num_ceps"] = d[4]; r["dim"] = d[5]; r["num_weights"] = d[6];
    return r;
  }, py::arg("opts"), "frame length, shift, padded window and the table sizes the options imply (khg_frontend_dims)");
  m.def("num_frames", [](const khg_frontend_opts& o, int64_t n) {
    int64_t T = 0;
    Check(khg_frontend_num_frames(&o, n, &T));
    return T;
  }, py::arg("opts"), py::arg("n_samples"), "frames of an utterance of n_samples (khg_frontend_num_frames; DESIGN.md 7q)");
  m.def("frontend_tables", [](const khg_frontend_opts& o) {
    int32_t d[8];
    Check(khg_frontend_dims(&o, d));
    Arr<float> win((py::ssize_t)d[0]), w((py::ssize_t)d[6]), dct({(py::ssize_t)d[4], (py::ssize_t)d[3]}), lif((py::ssize_t)d[4]), tw({(py::ssize_t)d[2] / 2, (py::ssize_t)2});
    Arr<int32_t> off((py::ssize_t)d[3]), len((py::ssize_t)d[3]);
    Check(khg_frontend_tables(&o, win.mutable_data(), off.mutable_data(), len.mutable_data(), w.mutable_data(), dct.mutable_data(), lif.mutable_data(), tw.mutable_data()));
    py::dict r;
    r["L"] = d[0]; r["S"] = d[1]; r["N"] = d[2];
    r["window"] = win; r["mel_off"] = off; r["mel_len"] = len; r["mel_w"] = w; r["dct"] = dct; r["lifter"] = lif; r["twiddles"] = tw;
    return r;
  }, py::arg("opts"), "the window, mel filters (first bin, length, weights one after the other), DCT rows, lifter and FFT twiddles (khg_frontend_tables)");
  py::class_<KFrontend>(m, "DeviceFrontend")
      .def(py::init<py::object, const khg_frontend_opts&>(), py::arg("ctx"), py::arg("opts"))
      .def_property_readonly("h", [](KFrontend& x) { return reinterpret_cast<uintptr_t>(x.h); })
      .def_readonly("ctx", &KFrontend::ctx_obj).def_readonly("dim", &KFrontend::dim)
      .def_property_readonly("opts", [](KFrontend& x) { return x.opts; })
      .def("compute", &KFrontend::compute, py::arg("sample_off"), py::arg("samples_h"), py::arg("samples_d"), py::arg("sample_type"), py::arg("out") = py::none())
      .def("close", &KFrontend::close);
  m.def("build_tree", [](int N, int P, Arr<int32_t> keys, Arr<double> cnt, Arr<double> x, Arr<double> x2, Arr<int32_t> qkeys, Arr<int64_t> qkey_off, Arr<int64_t> q_off,
                         Arr<int32_t> q_vals, Arr<int64_t> set_off, Arr<int32_t> set_phones, Arr<int32_t> share_roots, Arr<int32_t> do_split, Arr<int32_t> p2n, double thresh,
                         int max_leaves, double cluster_thresh, double var_floor) {
    const py::ssize_t K = cnt.size(), nq = qkeys.size(), ns = share_roots.size();
    if (x.ndim() != 2 || x2.ndim() != 2 || x.shape(0) != K || x2.shape(0) != K || x.shape(1) != x2.shape(1) || x.shape(1) < 1 || keys.size() != K * ((py::ssize_t)N + 1))
      throw py::value_error("build_tree: keys [num_keys, N + 1], count [num_keys], x and x2 [num_keys, dim]");
    if (qkey_off.size() != nq + 1 || q_off.size() < 1 || (nq > 0 && q_off.size() != qkey_off.at(nq) + 1) || (q_vals.size() != q_off.at(q_off.size() - 1)))
      throw py::value_error("build_tree: the question offset lists do not fit together");
    if (ns < 1 || do_split.size() != ns || set_off.size() != ns + 1 || set_phones.size() != set_off.at(ns))
      throw py::value_error("build_tree: one share_roots / do_split entry per phone set, set_off [num_sets + 1]");
    // One build: the first buffer holds any stream these arguments can give -- the header, per phone set its stub nodes (a table over
    // the pdf-classes, a split on the central phone with a yes-set of at most every phone), the table over the phones, and per split an
    // SE node with the largest question as its yes-set and one new leaf -- unless that bound is above 64 MiB; only then can a second
    // build be needed (khg_build_tree's size query costs a full build).
    int64_t max_pc = 1, max_q = 0, highest = 0;
    for (py::ssize_t i = 0; i < p2n.size(); ++i) max_pc = std::max<int64_t>(max_pc, p2n.at(i));
    for (py::ssize_t i = 0; i + 1 < q_off.size(); ++i) max_q = std::max<int64_t>(max_q, q_off.at(i + 1) - q_off.at(i));
    for (py::ssize_t i = 0; i < set_phones.size(); ++i) highest = std::max<int64_t>(highest, set_phones.at(i));
    const int64_t splits = max_leaves > 0 ? (int64_t)max_leaves : std::max<int64_t>((int64_t)K, 1);
    const bool multi = set_phones.size() > ns;     // a set of several phones: the stub splits the sets in halves, and a half of single phones is a table of its own
    const int64_t bound = 128 + (int64_t)ns * (64 + 8 * max_pc + (multi ? 4 * (int64_t)set_phones.size() + 5 * (highest + 2) : 0)) + 5 * (highest + 2) +
                          splits * (48 + 4 * max_q);
    std::string buf((size_t)std::min<int64_t>(std::max<int64_t>(bound, 1 << 16), (int64_t)64 << 20), '\0');
    int64_t nbytes = 0;
    double impr = 0.0, loss = 0.0;
    int32_t nl = 0, nr = 0;
    auto run = [&] {
      return khg_build_tree(N, P, (int32_t)x.shape(1), (int64_t)K, keys.data(), cnt.data(), x.data(), x2.data(), (int32_t)nq, qkeys.data(), qkey_off.data(), q_off.data(),
                            q_vals.data(), (int32_t)ns, set_off.data(), set_phones.data(), share_roots.data(), do_split.data(), (int32_t)p2n.size(), p2n.data(), thresh,
                            max_leaves, cluster_thresh, var_floor, reinterpret_cast<unsigned char*>(&buf[0]), (int64_t)buf.size(), &nbytes, &impr, &loss, &nl, &nr);
    };
    Check(NoGil(run));
    if (nbytes > (int64_t)buf.size()) { buf.assign((size_t)nbytes, '\0'); Check(NoGil(run)); }
    py::dict d;
    d["tree"] = py::bytes(buf.data(), (size_t)nbytes); d["objf_impr"] = impr; d["cluster_loss"] = loss; d["num_leaves"] = (int)nl; d["num_removed"] = (int)nr;
    return d;
  }, py::arg("N"), py::arg("P"), py::arg("keys"), py::arg("count"), py::arg("x"), py::arg("x2"), py::arg("qkeys"), py::arg("qkey_off"), py::arg("q_off"), py::arg("q_vals"),
     py::arg("set_off"), py::arg("set_phones"), py::arg("share_roots"), py::arg("do_split"), py::arg("phone2num_pdf_classes"), py::arg("thresh"), py::arg("max_leaves"),
     py::arg("cluster_thresh"), py::arg("var_floor") = 0.01, "BuildTree on host statistics (khg_build_tree; DESIGN.md 7o) -> the binary ContextDependency stream and its figures");
  m.attr("TREE_MAX_CONTEXT") = KHG_TREE_MAX_CONTEXT; m.attr("TREE_MAX_PHONE") = KHG_TREE_MAX_PHONE; m.attr("TREE_MAX_PDF_CLASS") = KHG_TREE_MAX_PDF_CLASS;
  m.attr("TREE_TID_SELF_LOOP") = KHG_TREE_TID_SELF_LOOP; m.attr("TREE_TID_FINAL") = KHG_TREE_TID_FINAL;
  m.attr("TREE_STATUS_NO_ALI") = KHG_TREE_STATUS_NO_ALI; m.attr("TREE_STATUS_MIXED_PHONES") = KHG_TREE_STATUS_MIXED_PHONES; m.attr("TREE_STATUS_OPEN_END") = KHG_TREE_STATUS_OPEN_END;
  m.def("scaled_trans_cost", [](Arr<float> lp, Arr<float> nsl, Arr<int32_t> id2state, Arr<uint8_t> isl, float ts, float sls) {
    const int nt = (int)lp.shape(0) - 1;
    Arr<float> out({(py::ssize_t)nt + 1});
    Check(khg_scaled_trans_cost(nt, lp.data(), nsl.data(), id2state.data(), isl.data(), ts, sls, out.mutable_data()));
    return out;
  }, "-GetScaledTransitionLogProb (csrc/hmm-utils.cc:442-463) for every transition-id");
}
