// Implementation of khg_host_fst.hpp: see the header for what each piece mirrors in the reference.
#include "khg_host_fst.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>

namespace khg {

std::string StdArc::ToString() const {
  char b[96];
  std::snprintf(b, sizeof(b), "StdArc(%d, %d, %g, %d)", ilabel, olabel, (double)weight, nextstate);
  return b;
}

GraphsCsr ConcatGraphs(const std::vector<const StdVectorFst*>& fsts) {
  GraphsCsr c;
  c.state_off.push_back(0);
  c.arc_off.push_back(0);
  for (const StdVectorFst* f : fsts) {
    c.state_off.push_back(c.state_off.back() + f->NumStates());
    c.start.push_back(f->Start());
    for (int s = 0; s < f->NumStates(); ++s) {
      for (const StdArc& a : f->Arcs(s)) {
        c.ilabel.push_back(a.ilabel); c.olabel.push_back(a.olabel); c.weight.push_back(a.weight); c.nextstate.push_back(a.nextstate);
      }
      c.arc_off.push_back((int64_t)c.ilabel.size());
      c.final_w.push_back(f->Final(s));
    }
  }
  return c;
}

void ModifyGraphForCarefulAlignment(StdVectorFst* fst) {
  const int S = fst->NumStates();
  if (S == 0) return;       // "Empty FST input." -- left as it is
  const float inf = std::numeric_limits<float>::infinity();
  std::vector<std::vector<StdArc>> rhs = fst->arcs();           // the right copy, before the left one gains its epsilons
  for (auto& arcs : rhs) for (StdArc& a : arcs) a.nextstate += S;
  const int pre_initial = 2 * S;
  for (int s = 0; s < S; ++s)
    if (fst->finals()[(size_t)s] != inf) {                       // Concat: a final state's weight moves onto an epsilon arc
      fst->arcs()[(size_t)s].push_back(StdArc{0, 0, fst->finals()[(size_t)s], pre_initial});
      fst->finals()[(size_t)s] = inf;
    }
  for (auto& arcs : rhs) { fst->arcs().push_back(std::move(arcs)); fst->finals().push_back(inf); }
  fst->arcs().push_back({StdArc{0, 0, 0.0f, fst->Start() + S}});   // the pre-initial state of the right copy: final, epsilon to its start
  fst->finals().push_back(0.0f);
}

void AddTransitionProbs(const TransitionModel& tm, const std::vector<int>& disambig, float transition_scale, float self_loop_scale, StdVectorFst* fst) {
  for (size_t i = 1; i < disambig.size(); ++i) KHG_REQUIRE(disambig[i - 1] < disambig[i], "IsSortedAndUniq(disambig_syms) assertion failed");
  const std::vector<float> cost = tm.ScaledTransCost(transition_scale, self_loop_scale);
  const int nt = tm.NumTransitionIds();
  for (int s = 0; s < fst->NumStates(); ++s)
    for (StdArc& a : fst->MutableArcs(s)) {
      if (a.ilabel >= 1 && a.ilabel <= nt) a.weight = a.weight + cost[(size_t)a.ilabel];
      else if (a.ilabel != 0 && !std::binary_search(disambig.begin(), disambig.end(), a.ilabel))
        throw Error("AddTransitionProbs: invalid symbol " + std::to_string(a.ilabel) + " on graph input side.");
    }
}

bool LinearLattice::GetLinearSymbolSequence(std::vector<int>* il, std::vector<int>* ol, LatticeWeight* total) const {
  il->clear(); ol->clear();
  *total = LatticeWeight();
  if (start < 0) return false;
  LatticeWeight w = final_w;
  for (const LatticeArc& a : arcs) {
    w.value1 += a.weight.value1; w.value2 += a.weight.value2;
    if (a.ilabel) il->push_back(a.ilabel);
    if (a.olabel) ol->push_back(a.olabel);
  }
  *total = w;
  return true;
}

std::vector<LatticeArc> Lattice::Arcs(int s) const {
  Check(s);
  std::vector<LatticeArc> out;
  for (int a = arc_begin[(size_t)s]; a < arc_begin[(size_t)s + 1]; ++a)
    out.push_back(LatticeArc{ilabel[(size_t)a], olabel[(size_t)a], LatticeWeight{(double)graph_cost[(size_t)a], (double)acoustic_cost[(size_t)a]},
                             nextstate[(size_t)a]});
  return out;
}

LatticeWeight Lattice::Final(int s) const {
  Check(s);
  const double inf = std::numeric_limits<double>::infinity();
  if (final_cost[(size_t)s] == std::numeric_limits<float>::infinity()) return LatticeWeight{inf, inf};
  return LatticeWeight{(double)final_cost[(size_t)s], 0.0};
}

std::string Lattice::ToText() const {
  std::string out;
  char b[160];
  for (int s = 0; s < NumStates(); ++s)
    for (int a = arc_begin[(size_t)s]; a < arc_begin[(size_t)s + 1]; ++a) {
      std::snprintf(b, sizeof(b), "%d %d %d %d %.9g,%.9g\n", s, nextstate[(size_t)a], ilabel[(size_t)a], olabel[(size_t)a],
                    (double)graph_cost[(size_t)a], (double)acoustic_cost[(size_t)a]);
      out += b;
    }
  for (int s = 0; s < NumStates(); ++s)
    if (final_cost[(size_t)s] != std::numeric_limits<float>::infinity()) {
      std::snprintf(b, sizeof(b), "%d %.9g,%.9g\n", s, (double)final_cost[(size_t)s], 0.0);
      out += b;
    }
  return out;
}

namespace {
// NaturalLess of LatticeWeight on float pairs: (a1, a2) strictly better than (b1, b2)
inline bool LatLess(float a1, float a2, float b1, float b2) {
  const float fa = a1 + a2, fb = b1 + b2;
  if (fa < fb) return true;
  if (fa > fb) return false;
  return a1 < b1;
}
}  // namespace

// the forward pairs and back-pointers under (gs, as); false: a negative-cost epsilon cycle
bool Lattice::Forward(float gs, float as, std::vector<float>* d1p, std::vector<float>* d2p, std::vector<int32_t>* bpp) const {
  const int N = NumStates();
  const float INF = std::numeric_limits<float>::infinity();
  // in-links of every state, stable by (source state, arc): the in-arc order of the decoder kernel
  const int64_t A = NumArcs();
  std::vector<int64_t> in_off((size_t)N + 1, 0);
  for (int64_t a = 0; a < A; ++a) in_off[(size_t)nextstate[(size_t)a] + 1]++;
  for (int s = 0; s < N; ++s) in_off[(size_t)s + 1] += in_off[(size_t)s];
  std::vector<int32_t> in_arc((size_t)A), in_src((size_t)A);
  {
    std::vector<int64_t> cur(in_off.begin(), in_off.end() - 1);
    for (int s = 0; s < N; ++s)
      for (int a = arc_begin[(size_t)s]; a < arc_begin[(size_t)s + 1]; ++a) {
        const int64_t pos = cur[(size_t)nextstate[(size_t)a]]++;
        in_arc[(size_t)pos] = a; in_src[(size_t)pos] = s;
      }
  }
  std::vector<float>& d1 = *d1p; std::vector<float>& d2 = *d2p; std::vector<int32_t>& bp = *bpp;
  d1.assign((size_t)N, INF); d2.assign((size_t)N, INF); bp.assign((size_t)N, -1);
  std::vector<float> n1((size_t)N), n2((size_t)N);
  d1[(size_t)start] = 0.0f; d2[(size_t)start] = 0.0f;
  const int T = frame[(size_t)N - 1];
  int lo = 0;
  for (int f = 0; f <= T; ++f) {
    int hi = lo;
    while (hi < N && frame[(size_t)hi] == f) ++hi;
    if (f > 0)
      for (int n = lo; n < hi; ++n) {          // emitting in-links, from the frame before
        float b1 = INF, b2 = INF;
        for (int64_t i = in_off[(size_t)n]; i < in_off[(size_t)n + 1]; ++i) {
          const int a = in_arc[(size_t)i], m = in_src[(size_t)i];
          if (ilabel[(size_t)a] == 0 || d1[(size_t)m] == INF) continue;
          const float w1 = gs * graph_cost[(size_t)a], w2 = as * acoustic_cost[(size_t)a];
          const float c1 = d1[(size_t)m] + w1, c2 = d2[(size_t)m] + w2;
          if (b1 == INF || LatLess(c1, c2, b1, b2)) { b1 = c1; b2 = c2; bp[(size_t)n] = a; }
        }
        d1[(size_t)n] = b1; d2[(size_t)n] = b2;
      }
    for (int round = 0;; ++round) {            // epsilon in-links: Jacobi rounds
      bool changed = false;
      for (int n = lo; n < hi; ++n) {
        float b1 = d1[(size_t)n], b2 = d2[(size_t)n];
        for (int64_t i = in_off[(size_t)n]; i < in_off[(size_t)n + 1]; ++i) {
          const int a = in_arc[(size_t)i], m = in_src[(size_t)i];
          if (ilabel[(size_t)a] != 0 || d1[(size_t)m] == INF) continue;
          const float w1 = gs * graph_cost[(size_t)a];
          const float c1 = d1[(size_t)m] + w1, c2 = d2[(size_t)m] + 0.0f;
          if (b1 == INF || LatLess(c1, c2, b1, b2)) { b1 = c1; b2 = c2; bp[(size_t)n] = a; changed = true; }
        }
        n1[(size_t)n] = b1; n2[(size_t)n] = b2;
      }
      for (int n = lo; n < hi; ++n) { d1[(size_t)n] = n1[(size_t)n]; d2[(size_t)n] = n2[(size_t)n]; }
      if (!changed) break;
      if (round > hi - lo) return false;
    }
    lo = hi;
  }
  return true;
}

// the backward pairs: the mirror image of Forward, over out-arcs
bool Lattice::Backward(float gs, float as, std::vector<float>* e1p, std::vector<float>* e2p) const {
  const int N = NumStates();
  const float INF = std::numeric_limits<float>::infinity();
  std::vector<float>& e1 = *e1p; std::vector<float>& e2 = *e2p;
  e1.assign((size_t)N, INF); e2.assign((size_t)N, INF);
  std::vector<float> n1((size_t)N), n2((size_t)N);
  const int T = frame[(size_t)N - 1];
  int hi = N;
  while (hi > 0) {
    const int f = frame[(size_t)hi - 1];
    int lo = hi;
    while (lo > 0 && frame[(size_t)lo - 1] == f) --lo;
    for (int n = lo; n < hi; ++n) {
      float b1 = INF, b2 = INF;
      if (f == T && final_cost[(size_t)n] != INF) { b1 = gs * final_cost[(size_t)n]; b2 = 0.0f; }
      for (int a = arc_begin[(size_t)n]; a < arc_begin[(size_t)n + 1]; ++a) {
        const int k = nextstate[(size_t)a];
        if (ilabel[(size_t)a] == 0 || e1[(size_t)k] == INF) continue;
        const float w1 = gs * graph_cost[(size_t)a], w2 = as * acoustic_cost[(size_t)a];
        const float c1 = w1 + e1[(size_t)k], c2 = w2 + e2[(size_t)k];
        if (b1 == INF || LatLess(c1, c2, b1, b2)) { b1 = c1; b2 = c2; }
      }
      e1[(size_t)n] = b1; e2[(size_t)n] = b2;
    }
    for (int round = 0;; ++round) {
      bool changed = false;
      for (int n = lo; n < hi; ++n) {
        float b1 = e1[(size_t)n], b2 = e2[(size_t)n];
        for (int a = arc_begin[(size_t)n]; a < arc_begin[(size_t)n + 1]; ++a) {
          const int k = nextstate[(size_t)a];
          if (ilabel[(size_t)a] != 0 || e1[(size_t)k] == INF) continue;
          const float w1 = gs * graph_cost[(size_t)a];
          const float c1 = w1 + e1[(size_t)k], c2 = 0.0f + e2[(size_t)k];
          if (b1 == INF || LatLess(c1, c2, b1, b2)) { b1 = c1; b2 = c2; changed = true; }
        }
        n1[(size_t)n] = b1; n2[(size_t)n] = b2;
      }
      for (int n = lo; n < hi; ++n) { e1[(size_t)n] = n1[(size_t)n]; e2[(size_t)n] = n2[(size_t)n]; }
      if (!changed) break;
      if (round > hi - lo) return false;
    }
    hi = lo;
  }
  return true;
}

LatticeBestPath Lattice::BestPath(float gs, float as) const {
  KHG_REQUIRE(gs >= 0.0f && as >= 0.0f, "Lattice: graph_scale and acoustic_scale must be >= 0");
  LatticeBestPath out;
  const float INF = std::numeric_limits<float>::infinity();
  out.v1 = out.v2 = out.f1 = out.f2 = INF;
  out.status = KHG_LAT_NO_PATH;
  const int N = NumStates();
  if (N == 0 || start < 0) return out;
  if (!Forward(gs, as, &out.alpha1, &out.alpha2, &out.bp)) { out.status = KHG_LAT_EPS_LOOP; return out; }
  const std::vector<float>&d1 = out.alpha1, &d2 = out.alpha2;
  const std::vector<int32_t>& bp = out.bp;
  const int64_t A = NumArcs();
  const int T = frame[(size_t)N - 1];
  int fin = -1;
  float f1 = INF, f2 = INF;
  for (int n = 0; n < N; ++n) {
    if (frame[(size_t)n] != T || d1[(size_t)n] == INF || final_cost[(size_t)n] == INF) continue;
    const float fw = gs * final_cost[(size_t)n];
    const float w1 = d1[(size_t)n] + fw, w2 = d2[(size_t)n] + 0.0f;
    if (fin < 0 || LatLess(w1, w2, f1, f2)) { f1 = w1; f2 = w2; fin = n; }
  }
  if (fin < 0) return out;
  std::vector<int32_t> path;
  for (int n = fin; !(n == start && bp[(size_t)n] < 0);) {
    const int a = bp[(size_t)n];
    if (a < 0 || (int64_t)path.size() > A) return out;
    path.push_back(a);
    // the source of arc a: the state whose arc range holds it
    n = (int)(std::upper_bound(arc_begin.begin(), arc_begin.end(), a) - arc_begin.begin()) - 1;
  }
  std::reverse(path.begin(), path.end());
  float v1 = 0.0f, v2 = 0.0f;
  for (int a : path) {
    const float w1 = gs * graph_cost[(size_t)a], w2 = ilabel[(size_t)a] != 0 ? as * acoustic_cost[(size_t)a] : 0.0f;
    v1 = v1 + w1; v2 = v2 + w2;
    if (ilabel[(size_t)a]) out.ali.push_back(ilabel[(size_t)a]);
    if (olabel[(size_t)a]) out.words.push_back(olabel[(size_t)a]);
  }
  const float fw = gs * final_cost[(size_t)fin];
  out.v1 = v1 + fw; out.v2 = v2 + 0.0f;
  out.f1 = f1; out.f2 = f2;
  out.arcs = std::move(path);
  out.final_state = fin;
  out.status = KHG_LAT_SUCCEEDED;
  return out;
}

LinearLattice Lattice::ShortestPath(float gs, float as) const {
  LinearLattice out;
  const LatticeBestPath b = BestPath(gs, as);
  KHG_REQUIRE(!(b.status & KHG_LAT_EPS_LOOP), "Lattice::ShortestPath: a negative-cost epsilon cycle");
  if (!(b.status & KHG_LAT_SUCCEEDED)) return out;
  out.start = 0;
  for (size_t i = 0; i < b.arcs.size(); ++i) {
    const int a = b.arcs[i];
    const float w1 = gs * graph_cost[(size_t)a], w2 = as * acoustic_cost[(size_t)a];
    out.arcs.push_back(LatticeArc{ilabel[(size_t)a], olabel[(size_t)a], LatticeWeight{(double)w1, (double)w2}, (int)i + 1});
  }
  const float fw = gs * final_cost[(size_t)b.final_state];
  out.final_w = LatticeWeight{(double)fw, 0.0};
  return out;
}

namespace {
// log(exp(init) + sum exp(x[i])), the maximum taken out first; -inf when every term is
double LogSumExp(double init, const std::vector<double>& x) {
  const double NINF = -std::numeric_limits<double>::infinity();
  double m = init;
  for (double v : x) m = std::max(m, v);
  if (m == NINF) return NINF;
  double sum = std::exp(init - m);
  for (double v : x) sum += std::exp(v - m);
  return m + std::log(sum);
}
}  // namespace

LatticePosteriors Lattice::ForwardBackward(float graph_scale, float acoustic_scale) const {
  KHG_REQUIRE(graph_scale >= 0.0f && acoustic_scale >= 0.0f && graph_scale != std::numeric_limits<float>::infinity() &&
                  acoustic_scale != std::numeric_limits<float>::infinity(),
              "Lattice::ForwardBackward: graph_scale and acoustic_scale must be finite and >= 0");
  const double NINF = -std::numeric_limits<double>::infinity();
  const float FINF = std::numeric_limits<float>::infinity();
  const double gs = graph_scale, as = acoustic_scale;
  LatticePosteriors out;
  out.status = KHG_LAT_NO_PATH;
  out.tot_like = NINF;
  const int N = NumStates();
  if (N == 0 || start < 0) return out;
  const int64_t A = NumArcs();
  std::vector<int32_t> src((size_t)A);
  for (int s = 0; s < N; ++s)
    for (int a = arc_begin[(size_t)s]; a < arc_begin[(size_t)s + 1]; ++a) {
      src[(size_t)a] = s;
      if (nextstate[(size_t)a] <= s) {
        KHG_REQUIRE(ilabel[(size_t)a] == 0, "Lattice::ForwardBackward: an emitting arc must go to the next frame");
        out.status = KHG_LAT_EPS_LOOP;
      }
    }
  if (out.status == KHG_LAT_EPS_LOOP) return out;
  std::vector<double> w((size_t)A);
  for (int64_t a = 0; a < A; ++a) {
    const double g = gs * (double)graph_cost[(size_t)a];
    const double c = ilabel[(size_t)a] != 0 ? as * (double)acoustic_cost[(size_t)a] : 0.0;
    w[(size_t)a] = -(g + c);
  }
  const int T = frame[(size_t)N - 1];
  auto fin = [&](int s) { return frame[(size_t)s] == T && final_cost[(size_t)s] != FINF ? -(gs * (double)final_cost[(size_t)s]) : NINF; };
  // in-arcs of every state in global arc order
  std::vector<std::vector<int32_t>> in((size_t)N);
  for (int64_t a = 0; a < A; ++a) in[(size_t)nextstate[(size_t)a]].push_back((int32_t)a);
  std::vector<double> alpha((size_t)N, NINF), beta((size_t)N, NINF), x;
  for (int s = 0; s < N; ++s) {
    x.clear();
    for (int32_t a : in[(size_t)s]) x.push_back(alpha[(size_t)src[(size_t)a]] + w[(size_t)a]);
    alpha[(size_t)s] = LogSumExp(s == start ? 0.0 : NINF, x);
  }
  x.clear();
  for (int s = 0; s < N; ++s) if (fin(s) != NINF) x.push_back(alpha[(size_t)s] + fin(s));
  const double tot = LogSumExp(NINF, x);
  if (tot == NINF) return out;
  for (int s = N - 1; s >= 0; --s) {
    x.clear();
    for (int a = arc_begin[(size_t)s]; a < arc_begin[(size_t)s + 1]; ++a) x.push_back(w[(size_t)a] + beta[(size_t)nextstate[(size_t)a]]);
    beta[(size_t)s] = LogSumExp(fin(s), x);
  }
  out.status = KHG_LAT_SUCCEEDED;
  out.tot_like = tot;
  out.arc_post.assign((size_t)A, 0.0);
  std::vector<char> live((size_t)A, 0);
  for (int64_t a = 0; a < A; ++a) {
    const double al = alpha[(size_t)src[(size_t)a]], be = beta[(size_t)nextstate[(size_t)a]];
    if (al == NINF || be == NINF) continue;
    live[(size_t)a] = 1;
    out.arc_post[(size_t)a] = std::exp(((al + w[(size_t)a]) + be) - tot);
  }
  // per frame: the live emitting arcs that leave it, merged by ilabel (weights summed in arc order), ascending
  out.post.assign((size_t)T, {});
  for (int64_t a = 0; a < A; ++a) {
    if (!live[(size_t)a] || ilabel[(size_t)a] == 0) continue;
    const int t = frame[(size_t)src[(size_t)a]];
    if (t < 0 || t >= T) continue;
    auto& row = out.post[(size_t)t];
    auto it = std::find_if(row.begin(), row.end(), [&](const std::pair<int32_t, double>& e) { return e.first == ilabel[(size_t)a]; });
    if (it == row.end()) row.emplace_back(ilabel[(size_t)a], out.arc_post[(size_t)a]);
    else it->second += out.arc_post[(size_t)a];
  }
  for (auto& row : out.post) std::sort(row.begin(), row.end(), [](const std::pair<int32_t, double>& a, const std::pair<int32_t, double>& b) { return a.first < b.first; });
  out.alpha = std::move(alpha);
  out.beta = std::move(beta);
  return out;
}

LatticeMpePosteriors Lattice::ForwardBackwardMpe(const std::vector<int32_t>& tid2phone, const std::vector<int32_t>& tid2pdf,
                                                 const std::vector<int32_t>& silence_phones, const std::vector<int32_t>& alignment, bool smbr,
                                                 bool one_silence_class, float graph_scale, float acoustic_scale) const {
  const std::string who = "Lattice::ForwardBackwardMpe: ";
  KHG_REQUIRE(graph_scale >= 0.0f && acoustic_scale >= 0.0f && graph_scale != std::numeric_limits<float>::infinity() &&
                  acoustic_scale != std::numeric_limits<float>::infinity(),
              who + "graph_scale and acoustic_scale must be finite and >= 0");
  KHG_REQUIRE(!tid2phone.empty(), who + "tid2phone needs an entry per transition-id, and entry 0");
  KHG_REQUIRE(!smbr || tid2pdf.size() == tid2phone.size(), who + "sMBR needs tid2pdf, of tid2phone's length");
  const int32_t num_tids = (int32_t)tid2phone.size() - 1;
  for (int32_t sp : silence_phones)
    KHG_REQUIRE(std::find(tid2phone.begin() + 1, tid2phone.end(), sp) != tid2phone.end(),
                who + "silence phone " + std::to_string(sp) + " is the phone of no transition-id");
  for (int32_t il : ilabel) KHG_REQUIRE(il >= 0 && il <= num_tids, who + "an arc carries an ilabel outside 0 .. num_tids");
  const double NINF = -std::numeric_limits<double>::infinity();
  LatticeMpePosteriors out;
  out.status = KHG_LAT_NO_PATH;
  out.tot_like = NINF;
  const int N = NumStates();
  if (N == 0 || start < 0) return out;
  const int T = frame[(size_t)N - 1];
  bool ref_ok = !alignment.empty() && (int64_t)alignment.size() == (int64_t)T;
  for (int32_t x : alignment) ref_ok = ref_ok && x >= 1 && x <= num_tids;
  if (!ref_ok) { out.status = KHG_LAT_NO_REF; return out; }
  // the likelihood part: alpha, beta, the total and the plain arc posteriors g
  const LatticePosteriors fb = ForwardBackward(graph_scale, acoustic_scale);
  out.status = fb.status;
  if (fb.status != KHG_LAT_SUCCEEDED) return out;
  out.tot_like = fb.tot_like;
  const double gs = graph_scale, as = acoustic_scale, tot = fb.tot_like;
  const float FINF = std::numeric_limits<float>::infinity();
  const int64_t A = NumArcs();
  const std::vector<double>&alpha = fb.alpha, &beta = fb.beta;
  std::vector<int32_t> src((size_t)A);
  std::vector<double> w((size_t)A), acc((size_t)A, 0.0);
  auto sil = [&](int32_t tid) { return std::find(silence_phones.begin(), silence_phones.end(), tid2phone[(size_t)tid]) != silence_phones.end(); };
  for (int s = 0; s < N; ++s)
    for (int a = arc_begin[(size_t)s]; a < arc_begin[(size_t)s + 1]; ++a) {
      src[(size_t)a] = s;
      const double g = gs * (double)graph_cost[(size_t)a];
      const double c = ilabel[(size_t)a] != 0 ? as * (double)acoustic_cost[(size_t)a] : 0.0;
      w[(size_t)a] = -(g + c);
      const int32_t il = ilabel[(size_t)a];
      if (il == 0 || frame[(size_t)s] >= T) continue;
      const int32_t r = alignment[(size_t)frame[(size_t)s]];
      const bool match = smbr ? tid2pdf[(size_t)il] == tid2pdf[(size_t)r] : tid2phone[(size_t)il] == tid2phone[(size_t)r];
      const bool ok = one_silence_class ? (match || (sil(il) && sil(r))) : (match && !sil(il));
      acc[(size_t)a] = ok ? 1.0 : 0.0;
    }
  std::vector<std::vector<int32_t>> in((size_t)N);
  for (int64_t a = 0; a < A; ++a) in[(size_t)nextstate[(size_t)a]].push_back((int32_t)a);
  std::vector<double> fwd((size_t)N, 0.0), bwd((size_t)N, 0.0);
  for (int s = 0; s < N; ++s) {
    if (s == start || alpha[(size_t)s] == NINF) continue;
    double sum = 0.0;
    for (int32_t a : in[(size_t)s]) {
      const double al = alpha[(size_t)src[(size_t)a]];
      if (al == NINF) continue;
      sum += std::exp((al + w[(size_t)a]) - alpha[(size_t)s]) * (fwd[(size_t)src[(size_t)a]] + acc[(size_t)a]);
    }
    fwd[(size_t)s] = sum;
  }
  double avg = 0.0;
  for (int s = 0; s < N; ++s) {
    if (frame[(size_t)s] != T || final_cost[(size_t)s] == FINF || alpha[(size_t)s] == NINF) continue;
    avg += std::exp((alpha[(size_t)s] + -(gs * (double)final_cost[(size_t)s])) - tot) * fwd[(size_t)s];
  }
  for (int s = N - 1; s >= 0; --s) {
    if (beta[(size_t)s] == NINF) continue;
    double sum = 0.0;
    for (int a = arc_begin[(size_t)s]; a < arc_begin[(size_t)s + 1]; ++a) {
      const double be = beta[(size_t)nextstate[(size_t)a]];
      if (be == NINF) continue;
      sum += std::exp((w[(size_t)a] + be) - beta[(size_t)s]) * (acc[(size_t)a] + bwd[(size_t)nextstate[(size_t)a]]);
    }
    bwd[(size_t)s] = sum;
  }
  out.avg_acc = avg;
  out.arc_post.assign((size_t)A, 0.0);
  std::vector<char> live((size_t)A, 0);
  for (int64_t a = 0; a < A; ++a) {
    const double al = alpha[(size_t)src[(size_t)a]], be = beta[(size_t)nextstate[(size_t)a]];
    if (al == NINF || be == NINF) continue;
    live[(size_t)a] = 1;
    const double g = std::exp(((al + w[(size_t)a]) + be) - tot);
    out.arc_post[(size_t)a] = g * (((fwd[(size_t)src[(size_t)a]] + acc[(size_t)a]) + bwd[(size_t)nextstate[(size_t)a]]) - avg);
  }
  out.post.assign((size_t)T, {});
  for (int64_t a = 0; a < A; ++a) {
    if (!live[(size_t)a] || ilabel[(size_t)a] == 0) continue;
    const int t = frame[(size_t)src[(size_t)a]];
    if (t < 0 || t >= T) continue;
    auto& row = out.post[(size_t)t];
    auto it = std::find_if(row.begin(), row.end(), [&](const std::pair<int32_t, double>& e) { return e.first == ilabel[(size_t)a]; });
    if (it == row.end()) row.emplace_back(ilabel[(size_t)a], out.arc_post[(size_t)a]);
    else it->second += out.arc_post[(size_t)a];
  }
  for (auto& row : out.post) std::sort(row.begin(), row.end(), [](const std::pair<int32_t, double>& a, const std::pair<int32_t, double>& b) { return a.first < b.first; });
  out.alpha = alpha;
  out.beta = beta;
  out.acc_fwd = std::move(fwd);
  out.acc_bwd = std::move(bwd);
  return out;
}

std::shared_ptr<Lattice> Lattice::Rescore(const std::function<float(int, int)>& loglike, float acoustic_scale) const {
  KHG_REQUIRE(std::isfinite(acoustic_scale), "Lattice::Rescore: acoustic_scale must be finite");
  auto r = std::make_shared<Lattice>(*this);
  for (int s = 0; s < NumStates(); ++s)
    for (int32_t a = arc_begin[(size_t)s]; a < arc_begin[(size_t)s + 1]; ++a)
      if (ilabel[(size_t)a] != 0) {
        const float prod = acoustic_scale * loglike(frame[(size_t)s], ilabel[(size_t)a]);
        r->acoustic_cost[(size_t)a] = -prod;
      }
  return r;
}

std::shared_ptr<Lattice> Lattice::Boost(const std::vector<int32_t>& tid2phone, const std::vector<int32_t>& silence_phones,
                                        const std::vector<int32_t>& alignment, float b, float max_silence_error) const {
  KHG_REQUIRE(std::isfinite(b) && std::isfinite(max_silence_error), "Lattice::Boost: b and max_silence_error must be finite");
  KHG_REQUIRE(!tid2phone.empty(), "Lattice::Boost: tid2phone needs an entry per transition-id, and entry 0");
  const int32_t num_tids = (int32_t)tid2phone.size() - 1;
  for (int32_t sp : silence_phones)
    KHG_REQUIRE(std::find(tid2phone.begin() + 1, tid2phone.end(), sp) != tid2phone.end(),
                "Lattice::Boost: silence phone " + std::to_string(sp) + " is the phone of no transition-id");
  const int T = NumStates() ? frame.back() : 0;
  KHG_REQUIRE((int64_t)alignment.size() == (int64_t)T, "Lattice::Boost: the alignment has " + std::to_string(alignment.size()) +
                                                           " frames, the lattice " + std::to_string(T));
  for (int32_t x : alignment) KHG_REQUIRE(x >= 1 && x <= num_tids, "Lattice::Boost: the alignment holds an id outside 1 .. num_tids");
  auto r = std::make_shared<Lattice>(*this);
  const float nb = -b;
  for (int s = 0; s < NumStates(); ++s)
    for (int32_t a = arc_begin[(size_t)s]; a < arc_begin[(size_t)s + 1]; ++a) {
      const int32_t il = ilabel[(size_t)a];
      if (il == 0) continue;
      KHG_REQUIRE(il >= 1 && il <= num_tids, "Lattice::Boost: an arc carries an ilabel outside 0 .. num_tids");
      KHG_REQUIRE(frame[(size_t)s] < T, "Lattice::Boost: an emitting arc leaves the last frame");
      const int32_t ph = tid2phone[(size_t)il], ref = tid2phone[(size_t)alignment[(size_t)frame[(size_t)s]]];
      const float e = ph == ref ? 0.0f : std::find(silence_phones.begin(), silence_phones.end(), ph) != silence_phones.end() ? max_silence_error : 1.0f;
      const float term = nb * e;
      r->graph_cost[(size_t)a] = graph_cost[(size_t)a] + term;
    }
  return r;
}

int BackoffLm::Advance(int h, int w, float* c) const {
  float acc = 0.0f;
  for (;;) {
    const auto b = word.begin() + arc_begin[(size_t)h], e = word.begin() + arc_begin[(size_t)h + 1];
    const auto it = std::lower_bound(b, e, w);
    if (it != e && *it == w) { *c = acc + cost[(size_t)(it - word.begin())]; return next[(size_t)(it - word.begin())]; }
    if (h == 0) { *c = acc; return -1; }
    acc = acc + backoff_cost[(size_t)h];
    h = backoff[(size_t)h];
  }
}

LatticeLmRescored Lattice::LmRescore(const BackoffLm& lm, float scale, int hist_factor) const {
  KHG_REQUIRE(std::isfinite(scale), "Lattice::LmRescore: scale must be finite");
  KHG_REQUIRE(hist_factor >= 1, "Lattice::LmRescore: hist_factor must be >= 1");
  LatticeLmRescored out;
  auto r = std::make_shared<Lattice>();
  r->arc_begin.push_back(0);
  out.lattice = r;
  const int N = NumStates();
  if (N == 0) { out.status = KHG_LAT_NO_PATH; return out; }
  for (int s = 0; s < N; ++s)
    for (int32_t a = arc_begin[(size_t)s]; a < arc_begin[(size_t)s + 1]; ++a)
      if (nextstate[(size_t)a] <= s) { out.status = KHG_LAT_EPS_LOOP; return out; }
  // the history sets in state order; an arc is looked at when its source's set is known, so every set is complete when its turn comes
  const int64_t cap = std::min<int64_t>((int64_t)hist_factor * N, INT32_MAX);
  std::vector<std::vector<int32_t>> H((size_t)N);
  H[(size_t)start].push_back(lm.start);
  int64_t used = 0, max_hist = 0;
  for (int d = 0; d < N; ++d) {
    std::vector<int32_t>& hd = H[(size_t)d];
    if (std::find(hd.begin(), hd.end(), -1) != hd.end()) { out.status = KHG_LAT_LM_OOV; return out; }
    std::sort(hd.begin(), hd.end());
    hd.erase(std::unique(hd.begin(), hd.end()), hd.end());
    used += (int64_t)hd.size();
    if (used > cap) { out.status = KHG_LAT_SCRATCH; return out; }
    max_hist = std::max<int64_t>(max_hist, (int64_t)hd.size());
    for (int32_t a = arc_begin[(size_t)d]; a < arc_begin[(size_t)d + 1]; ++a)
      for (int32_t h : hd) {
        float c;
        H[(size_t)nextstate[(size_t)a]].push_back(olabel[(size_t)a] == 0 ? h : lm.Advance(h, olabel[(size_t)a], &c));
      }
  }
  std::vector<int64_t> first((size_t)N + 1, 0);
  for (int s = 0; s < N; ++s) first[(size_t)s + 1] = first[(size_t)s] + (int64_t)H[(size_t)s].size();
  const float INF = std::numeric_limits<float>::infinity();
  for (int s = 0; s < N; ++s)
    for (int32_t h : H[(size_t)s]) {
      r->frame.push_back(frame[(size_t)s]); r->graph_state.push_back(graph_state[(size_t)s]);
      r->tot_cost.push_back(tot_cost[(size_t)s]); r->extra_cost.push_back(extra_cost[(size_t)s]);
      float f = final_cost[(size_t)s];
      if (f != INF) { const float t = scale * lm.final_cost[(size_t)h]; f = f + t; }
      r->final_cost.push_back(f);
      for (int32_t a = arc_begin[(size_t)s]; a < arc_begin[(size_t)s + 1]; ++a) {
        const int d = nextstate[(size_t)a], w = olabel[(size_t)a];
        float g = graph_cost[(size_t)a];
        int32_t hh = h;
        if (w != 0) {
          float c;
          hh = lm.Advance(h, w, &c);
          const float t = scale * c;
          g = g + t;
        }
        const std::vector<int32_t>& hd = H[(size_t)d];
        r->ilabel.push_back(ilabel[(size_t)a]); r->olabel.push_back(w); r->graph_cost.push_back(g);
        r->acoustic_cost.push_back(acoustic_cost[(size_t)a]);
        r->nextstate.push_back((int32_t)(first[(size_t)d] + (std::lower_bound(hd.begin(), hd.end(), hh) - hd.begin())));
      }
      KHG_REQUIRE(r->ilabel.size() <= (size_t)INT32_MAX, "Lattice::LmRescore: more than 2^31 - 1 arcs");
      r->arc_begin.push_back((int32_t)r->ilabel.size());
    }
  r->start = (int32_t)first[(size_t)start];
  out.status = KHG_LAT_SUCCEEDED;
  out.max_hist = max_hist;
  return out;
}

namespace {
// a determinized state: K / R, and the closure in ascending state number with E, pred (-1: external) and, per arc of every closure
// state, the determinized state its copy leads to (-1: the arc is not kept)
struct DetState {
  std::vector<int32_t> K, s, pred, slot_off, slot;
  std::vector<float> Ra, Rb, a, b;
  int32_t fin = -1;       // the closure state that keeps its final cost
};

// steps 2 to 5 of khg_lattices_determinize on the pruned lattice X (at least one state, every arc to a higher state); false: scratch
bool DetSplit(const Lattice& X, float gs, float as, float delta, int state_factor, Lattice* Y, khg_det_stats* stats) {
  const int N = X.NumStates();
  const int64_t A = X.NumArcs();
  const float INF = std::numeric_limits<float>::infinity();
  const std::vector<int32_t>&ab = X.arc_begin, &nxt = X.nextstate, &ol = X.olabel;
  std::vector<float> wa((size_t)A), wb((size_t)A);
  std::vector<int32_t> src((size_t)A), in_off((size_t)N + 1, 0), in_arc((size_t)A);
  for (int s = 0; s < N; ++s)
    for (int32_t a = ab[(size_t)s]; a < ab[(size_t)s + 1]; ++a) {
      src[(size_t)a] = s;
      wa[(size_t)a] = gs * X.graph_cost[(size_t)a];
      wb[(size_t)a] = X.ilabel[(size_t)a] != 0 ? as * X.acoustic_cost[(size_t)a] : 0.0f;
      in_off[(size_t)nxt[(size_t)a] + 1]++;
    }
  for (int s = 0; s < N; ++s) in_off[(size_t)s + 1] += in_off[(size_t)s];
  {
    std::vector<int32_t> cur(in_off.begin(), in_off.end() - 1);
    for (int64_t a = 0; a < A; ++a) in_arc[(size_t)cur[(size_t)nxt[(size_t)a]]++] = (int32_t)a;
  }
  const int64_t cap_s = std::min<int64_t>((int64_t)state_factor * N, INT32_MAX), cap_a = std::min<int64_t>((int64_t)state_factor * A, INT32_MAX);
  const int T = X.frame[(size_t)N - 1];
  std::vector<DetState> Ds;
  std::vector<int32_t> cl_stamp((size_t)N, 0), in_stamp((size_t)N, 0), cl_pred((size_t)N), cl_idx((size_t)N);
  std::vector<float> cl_a((size_t)N), cl_b((size_t)N), in_a((size_t)N), in_b((size_t)N);
  int32_t stamp = 0;
  int64_t used_s = 0, used_a = 0;
  // the arrival of I (ascending states): -> the number of its determinized state, -1: scratch; cl_pred holds the arrival's own pred
  auto arrive = [&](const std::vector<int32_t>& Is, const std::vector<float>& Ia, const std::vector<float>& Ib) -> int {
    ++stamp;
    size_t best = 0;
    for (size_t i = 1; i < Is.size(); ++i)
      if (LatLess(Ia[i], Ib[i], Ia[best], Ib[best])) best = i;
    for (size_t i = 0; i < Is.size(); ++i) {
      in_stamp[(size_t)Is[i]] = stamp;
      in_a[(size_t)Is[i]] = Ia[i] - Ia[best]; in_b[(size_t)Is[i]] = Ib[i] - Ib[best];
    }
    DetState c;
    int hi = Is.back();       // the highest state the closure can still reach
    int64_t arcs = 0;
    for (int s = Is[0]; s <= hi; ++s) {
      bool has = in_stamp[(size_t)s] == stamp;
      float ca = has ? in_a[(size_t)s] : 0.0f, cb = has ? in_b[(size_t)s] : 0.0f;
      int32_t pr = -1;
      for (int32_t j = in_off[(size_t)s]; j < in_off[(size_t)s + 1]; ++j) {
        const int32_t a = in_arc[(size_t)j], p = src[(size_t)a];
        if (ol[(size_t)a] != 0 || cl_stamp[(size_t)p] != stamp) continue;
        const float ta = cl_a[(size_t)p] + wa[(size_t)a], tb = cl_b[(size_t)p] + wb[(size_t)a];
        if (!has || LatLess(ta, tb, ca, cb)) { has = true; ca = ta; cb = tb; pr = a; }
      }
      if (!has) continue;
      cl_stamp[(size_t)s] = stamp; cl_a[(size_t)s] = ca; cl_b[(size_t)s] = cb; cl_pred[(size_t)s] = pr; cl_idx[(size_t)s] = (int32_t)c.s.size();
      c.s.push_back(s); c.a.push_back(ca); c.b.push_back(cb); c.pred.push_back(pr);
      c.slot_off.push_back((int32_t)arcs);
      arcs += ab[(size_t)s + 1] - ab[(size_t)s];
      for (int32_t a = ab[(size_t)s]; a < ab[(size_t)s + 1]; ++a)
        if (ol[(size_t)a] == 0) hi = std::max(hi, nxt[(size_t)a]);
    }
    for (int32_t s : Is)
      if (cl_pred[(size_t)s] < 0) { c.K.push_back(s); c.Ra.push_back(cl_a[(size_t)s]); c.Rb.push_back(cl_b[(size_t)s]); }
    for (size_t d = 0; d < Ds.size(); ++d) {
      const DetState& D = Ds[d];
      if (D.K != c.K) continue;
      bool same = true;
      for (size_t i = 0; i < c.K.size() && same; ++i) {
        const float da = c.Ra[i] - D.Ra[i], db = c.Rb[i] - D.Rb[i];
        same = std::fabs(da) <= delta && std::fabs(db) <= delta;
      }
      if (same) return (int)d;
    }
    used_s += (int64_t)c.s.size(); used_a += arcs;
    if (used_s > cap_s || used_a > cap_a) return -1;
    const int32_t me = (int32_t)Ds.size();
    c.slot.assign((size_t)arcs, -1);
    float f1 = 0.0f, f2 = 0.0f;
    for (size_t i = 0; i < c.s.size(); ++i) {
      const int32_t s = c.s[i], pr = c.pred[i];
      if (pr >= 0) { const int32_t p = src[(size_t)pr]; c.slot[(size_t)(c.slot_off[(size_t)cl_idx[(size_t)p]] + (pr - ab[(size_t)p]))] = me; }
      if (X.final_cost[(size_t)s] == INF || X.frame[(size_t)s] != T) continue;
      const float fw = gs * X.final_cost[(size_t)s];
      const float v1 = c.a[i] + fw, v2 = c.b[i];
      if (c.fin < 0 || LatLess(v1, v2, f1, f2)) { c.fin = s; f1 = v1; f2 = v2; }
    }
    stats->max_subset = std::max<int64_t>(stats->max_subset, (int64_t)c.K.size());
    stats->max_closure = std::max<int64_t>(stats->max_closure, (int64_t)c.s.size());
    Ds.push_back(std::move(c));
    return me;
  };
  if (arrive({X.start}, {0.0f}, {0.0f}) < 0) return false;
  struct Cand { int32_t w, dest, arc, elem; float a, b; };
  std::vector<Cand> cand;
  std::vector<int32_t> Is, Iarc, Ielem;
  std::vector<float> Ia, Ib;
  for (size_t d = 0; d < Ds.size(); ++d) {
    cand.clear();
    for (size_t i = 0; i < Ds[d].s.size(); ++i) {
      const int32_t p = Ds[d].s[i];
      for (int32_t a = ab[(size_t)p]; a < ab[(size_t)p + 1]; ++a)
        if (ol[(size_t)a] != 0) {
          const float ta = Ds[d].a[i] + wa[(size_t)a], tb = Ds[d].b[i] + wb[(size_t)a];
          cand.push_back(Cand{ol[(size_t)a], nxt[(size_t)a], a, (int32_t)i, ta, tb});
        }
    }
    // by (word, dest); inside a pair the candidates stay in ascending arc number
    std::stable_sort(cand.begin(), cand.end(), [](const Cand& x, const Cand& y) { return x.w != y.w ? x.w < y.w : x.dest < y.dest; });
    for (size_t i = 0; i < cand.size();) {
      Is.clear(); Ia.clear(); Ib.clear(); Iarc.clear(); Ielem.clear();
      const int32_t w = cand[i].w;
      while (i < cand.size() && cand[i].w == w) {
        size_t k = i;
        for (size_t j = i + 1; j < cand.size() && cand[j].w == w && cand[j].dest == cand[i].dest; ++j)
          if (LatLess(cand[j].a, cand[j].b, cand[k].a, cand[k].b)) k = j;
        Is.push_back(cand[k].dest); Ia.push_back(cand[k].a); Ib.push_back(cand[k].b); Iarc.push_back(cand[k].arc); Ielem.push_back(cand[k].elem);
        const int32_t dest = cand[i].dest;
        while (i < cand.size() && cand[i].w == w && cand[i].dest == dest) ++i;
      }
      const int d2 = arrive(Is, Ia, Ib);
      if (d2 < 0) return false;
      DetState& D = Ds[d];
      for (size_t k = 0; k < Is.size(); ++k)
        if (cl_pred[(size_t)Is[k]] < 0) D.slot[(size_t)(D.slot_off[(size_t)Ielem[k]] + (Iarc[k] - ab[(size_t)D.s[(size_t)Ielem[k]]]))] = d2;
    }
  }
  stats->det_states = (int64_t)Ds.size();
  // Y: the elements ordered by (s, D)
  std::vector<std::vector<std::pair<int32_t, int32_t>>> of((size_t)N);      // per state: (D, its place in D's closure), D ascending
  for (size_t d = 0; d < Ds.size(); ++d)
    for (size_t i = 0; i < Ds[d].s.size(); ++i) of[(size_t)Ds[d].s[i]].emplace_back((int32_t)d, (int32_t)i);
  std::vector<int64_t> first((size_t)N + 1, 0);
  for (int s = 0; s < N; ++s) first[(size_t)s + 1] = first[(size_t)s] + (int64_t)of[(size_t)s].size();
  Y->arc_begin.clear();
  for (int s = 0; s < N; ++s)
    for (const auto& e : of[(size_t)s]) {
      const DetState& D = Ds[(size_t)e.first];
      Y->frame.push_back(X.frame[(size_t)s]); Y->graph_state.push_back(X.graph_state[(size_t)s]);
      Y->tot_cost.push_back(X.tot_cost[(size_t)s]); Y->extra_cost.push_back(X.extra_cost[(size_t)s]);
      Y->final_cost.push_back(D.fin == s ? X.final_cost[(size_t)s] : INF);
      Y->arc_begin.push_back((int32_t)Y->ilabel.size());
      for (int32_t a = ab[(size_t)s]; a < ab[(size_t)s + 1]; ++a) {
        const int32_t t = D.slot[(size_t)(D.slot_off[(size_t)e.second] + (a - ab[(size_t)s]))];
        if (t < 0) continue;
        const auto& od = of[(size_t)nxt[(size_t)a]];
        const auto it = std::lower_bound(od.begin(), od.end(), std::make_pair(t, (int32_t)0));
        Y->ilabel.push_back(X.ilabel[(size_t)a]); Y->olabel.push_back(ol[(size_t)a]); Y->graph_cost.push_back(X.graph_cost[(size_t)a]);
        Y->acoustic_cost.push_back(X.acoustic_cost[(size_t)a]);
        Y->nextstate.push_back((int32_t)(first[(size_t)nxt[(size_t)a]] + (it - od.begin())));
      }
    }
  Y->arc_begin.push_back((int32_t)Y->ilabel.size());
  Y->start = (int32_t)first[(size_t)X.start];
  return true;
}
}  // namespace

LatticeDeterminized Lattice::Determinize(float gs, float as, float beam, float delta, int state_factor) const {
  const std::string who = "Lattice::Determinize: ";
  KHG_REQUIRE(gs >= 0.0f && as >= 0.0f && std::isfinite(gs) && std::isfinite(as), who + "graph_scale and acoustic_scale must be finite and >= 0");
  KHG_REQUIRE(std::isfinite(beam) && beam >= 0.0f, who + "beam must be finite and >= 0");
  KHG_REQUIRE(std::isfinite(delta) && delta >= 0.0f, who + "delta must be finite and >= 0");
  KHG_REQUIRE(state_factor >= 1, who + "state_factor must be >= 1");
  LatticeDeterminized out;
  auto none = std::make_shared<Lattice>();
  none->arc_begin.push_back(0);
  out.lattice = none;
  const int N = NumStates();
  out.stats.in_states = N; out.stats.in_arcs = NumArcs();
  if (N == 0) { out.status = KHG_LAT_NO_PATH; return out; }
  for (int s = 0; s < N; ++s)
    for (int32_t a = arc_begin[(size_t)s]; a < arc_begin[(size_t)s + 1]; ++a)
      if (nextstate[(size_t)a] <= s) { out.status = KHG_LAT_EPS_LOOP; return out; }
  int st = 0;
  const std::shared_ptr<Lattice> X = Prune(beam, gs, as, &st);
  out.status = st;
  if (st != KHG_LAT_SUCCEEDED) return out;
  out.stats.pruned_states = X->NumStates();
  Lattice Y;
  khg_det_stats ds = out.stats;
  if (!DetSplit(*X, gs, as, delta, state_factor, &Y, &ds)) { out.status = KHG_LAT_SCRATCH; return out; }
  const std::shared_ptr<Lattice> res = Y.Prune(beam, gs, as, &st);
  out.status = st;
  if (st != KHG_LAT_SUCCEEDED) return out;
  out.stats = ds;
  out.stats.out_states = res->NumStates(); out.stats.out_arcs = res->NumArcs();
  out.lattice = res;
  return out;
}

std::vector<LatticeNbestEntry> Lattice::Nbest(int n, float gs, float as, int* status) const {
  const std::string who = "Lattice::Nbest: ";
  KHG_REQUIRE(gs >= 0.0f && as >= 0.0f && std::isfinite(gs) && std::isfinite(as), who + "graph_scale and acoustic_scale must be finite and >= 0");
  KHG_REQUIRE(n >= 1 && n <= KHG_NBEST_MAX, who + "n must lie in 1 .. " + std::to_string(KHG_NBEST_MAX));
  std::vector<LatticeNbestEntry> out;
  int st_local = 0;
  int& st = status ? *status : st_local;
  const int N = NumStates();
  if (N == 0) { st = KHG_LAT_NO_PATH; return out; }
  for (int s = 0; s < N; ++s)
    for (int32_t a = arc_begin[(size_t)s]; a < arc_begin[(size_t)s + 1]; ++a)
      if (nextstate[(size_t)a] <= s) { st = KHG_LAT_EPS_LOOP; return out; }
  const float INF = std::numeric_limits<float>::infinity();
  struct Prefix { float t, a, b; int32_t nw, e, j; };
  const auto by_key = [](const Prefix& x, const Prefix& y) {
    if (x.t < y.t) return true;
    if (y.t < x.t) return false;
    return x.e != y.e ? x.e < y.e : x.j < y.j;
  };
  // the in-arcs of every state
  std::vector<std::vector<int32_t>> in((size_t)N);
  std::vector<int32_t> src((size_t)NumArcs());
  for (int s = 0; s < N; ++s)
    for (int32_t a = arc_begin[(size_t)s]; a < arc_begin[(size_t)s + 1]; ++a) { in[(size_t)nextstate[(size_t)a]].push_back(a); src[(size_t)a] = s; }
  // the scratch bound is on the lists' bounds len[s] = min(n, sum of len[p]), which do not know of dropped candidates
  {
    std::vector<int64_t> len((size_t)N, 0);
    int64_t tot = 0;
    for (int s = 0; s < N; ++s) {
      int64_t c = s == start ? 1 : 0;
      if (s != start) for (int32_t e : in[(size_t)s]) c += len[(size_t)src[(size_t)e]];
      len[(size_t)s] = std::min<int64_t>(c, n);
      tot += len[(size_t)s];
    }
    if (tot > (int64_t)INT32_MAX) { st = KHG_LAT_SCRATCH; return out; }
  }
  std::vector<std::vector<Prefix>> A((size_t)N);
  for (int s = 0; s < N; ++s) {
    std::vector<Prefix>& L = A[(size_t)s];
    if (s == start) L.push_back(Prefix{0.0f, 0.0f, 0.0f, 0, -1, 0});
    else
      for (int32_t e : in[(size_t)s]) {
        const float wa = gs * graph_cost[(size_t)e];
        const float wb = ilabel[(size_t)e] != 0 ? as * acoustic_cost[(size_t)e] : 0.0f;
        const float c = wa + wb;
        const std::vector<Prefix>& P = A[(size_t)src[(size_t)e]];
        for (size_t j = 0; j < P.size(); ++j) {
          const float t = P[j].t + c;
          if (!(t < INF)) continue;
          L.push_back(Prefix{t, P[j].a + wa, P[j].b + wb, P[j].nw + (olabel[(size_t)e] != 0 ? 1 : 0), e, (int32_t)j});
        }
      }
    std::sort(L.begin(), L.end(), by_key);
    if (L.size() > (size_t)n) L.resize((size_t)n);
  }
  const int T = frame[(size_t)N - 1];
  std::vector<Prefix> F;
  for (int s = 0; s < N; ++s) {
    const float fc = final_cost[(size_t)s];
    if (frame[(size_t)s] != T || !std::isfinite(fc)) continue;
    const float fw = gs * fc;
    const std::vector<Prefix>& P = A[(size_t)s];
    for (size_t j = 0; j < P.size(); ++j) {
      const float t = P[j].t + fw;
      if (!(t < INF)) continue;
      F.push_back(Prefix{t, P[j].a + fw, P[j].b, P[j].nw, s, (int32_t)j});
    }
  }
  std::sort(F.begin(), F.end(), by_key);
  if (F.size() > (size_t)n) F.resize((size_t)n);
  if (F.empty()) { st = KHG_LAT_NO_PATH; return out; }
  for (const Prefix& f : F) {
    LatticeNbestEntry x;
    x.a = f.a; x.b = f.b; x.total = f.t; x.end_state = f.e; x.rank = f.j;
    x.ali.assign((size_t)std::max(T, 0), 0);
    int s = f.e, j = f.j;
    for (;;) {
      const Prefix& q = A[(size_t)s][(size_t)j];
      if (q.e < 0) break;
      const int32_t e = q.e;
      s = src[(size_t)e]; j = q.j;
      x.arcs.push_back(e);
      if (ilabel[(size_t)e] != 0 && frame[(size_t)s] >= 0 && frame[(size_t)s] < T) x.ali[(size_t)frame[(size_t)s]] = ilabel[(size_t)e];
      if (olabel[(size_t)e] != 0) x.words.push_back(olabel[(size_t)e]);
    }
    std::reverse(x.arcs.begin(), x.arcs.end());
    std::reverse(x.words.begin(), x.words.end());
    out.push_back(std::move(x));
  }
  st = KHG_LAT_SUCCEEDED;
  return out;
}

std::shared_ptr<Lattice> Lattice::AddPenalty(float word_ins_penalty) const {
  KHG_REQUIRE(std::isfinite(word_ins_penalty), "Lattice::AddPenalty: word_ins_penalty must be finite");
  auto r = std::make_shared<Lattice>(*this);
  for (size_t a = 0; a < olabel.size(); ++a)
    if (olabel[a] != 0) r->graph_cost[a] = graph_cost[a] + word_ins_penalty;
  return r;
}

LatticeOracle Lattice::Oracle(const std::vector<int32_t>& ref) const {
  for (int32_t w : ref) KHG_REQUIRE(w > 0, "Lattice::Oracle: a reference word is not > 0");
  const int N = NumStates();
  const int64_t R = (int64_t)ref.size(), W = R + 1;
  KHG_REQUIRE((int64_t)N + R < (int64_t(1) << 29), "Lattice::Oracle: states + reference words reach 2^29");
  LatticeOracle out;
  out.status = KHG_LAT_NO_PATH;
  out.counts[0] = out.counts[2] = (int32_t)R;
  if (N == 0 || start < 0) return out;
  out.ali.assign((size_t)std::max(frame[(size_t)N - 1], 0), 0);
  for (int s = 0; s < N; ++s)
    for (int32_t a = arc_begin[(size_t)s]; a < arc_begin[(size_t)s + 1]; ++a)
      if (nextstate[(size_t)a] <= s) { out.status = KHG_LAT_EPS_LOOP; return out; }
  const int32_t INF = 1 << 30, NONE = -1, DEL = -2;
  // the in-arcs of every state in ascending arc number, with their sources
  std::vector<std::vector<int32_t>> in((size_t)N);
  std::vector<int32_t> src((size_t)NumArcs());
  for (int s = 0; s < N; ++s)
    for (int32_t a = arc_begin[(size_t)s]; a < arc_begin[(size_t)s + 1]; ++a) { src[(size_t)a] = s; in[(size_t)nextstate[(size_t)a]].push_back(a); }
  std::vector<int32_t> E((size_t)((int64_t)N * W), INF), M((size_t)((int64_t)N * W), NONE);      // a move: the arc (EPS, DIAG), -3 - arc (INS), NONE or DEL
  for (int s = 0; s < N; ++s) {
    int32_t* Es = E.data() + (int64_t)s * W;
    int32_t* Ms = M.data() + (int64_t)s * W;
    for (int64_t q = 0; q < W; ++q) {
      int32_t C = s == start && q == 0 ? 0 : INF, mv = NONE;
      for (int32_t a : in[(size_t)s]) {
        const int32_t* Ep = E.data() + (int64_t)src[(size_t)a] * W;
        const int32_t w = olabel[(size_t)a];
        if (w == 0) {
          if (Ep[q] < INF && Ep[q] < C) { C = Ep[q]; mv = a; }
        } else {
          if (q >= 1 && Ep[q - 1] < INF) { const int32_t c = Ep[q - 1] + (w != ref[(size_t)q - 1] ? 1 : 0); if (c < C) { C = c; mv = a; } }
          if (Ep[q] < INF) { const int32_t c = Ep[q] + 1; if (c < C) { C = c; mv = -3 - a; } }
        }
      }
      if (q >= 1 && Es[q - 1] < INF && Es[q - 1] + 1 < C) { C = Es[q - 1] + 1; mv = DEL; }
      Es[q] = C; Ms[q] = mv;
    }
  }
  const int T = frame[(size_t)N - 1];
  const float FINF = std::numeric_limits<float>::infinity();
  int fin = -1;
  for (int s = 0; s < N; ++s) {
    if (frame[(size_t)s] != T || final_cost[(size_t)s] == FINF) continue;
    const int32_t e = E[(size_t)((int64_t)s * W + R)];
    if (e < INF && (fin < 0 || e < E[(size_t)((int64_t)fin * W + R)])) fin = s;
  }
  if (fin < 0) return out;
  int32_t ins = 0, del = 0, sub = 0;
  int s = fin;
  int64_t q = R;
  for (;;) {
    const int32_t mv = M[(size_t)((int64_t)s * W + q)];
    if (mv == NONE) break;
    if (mv == DEL) { ++del; --q; continue; }
    const int32_t a = mv >= 0 ? mv : -3 - mv, w = olabel[(size_t)a];
    if (mv < 0) ++ins;
    else if (w != 0) { --q; if (w != ref[(size_t)q]) ++sub; }
    if (w != 0) out.words.push_back(w);
    out.arcs.push_back(a);
    const int f = frame[(size_t)src[(size_t)a]];
    if (ilabel[(size_t)a] != 0 && f >= 0 && f < T) out.ali[(size_t)f] = ilabel[(size_t)a];
    s = src[(size_t)a];
  }
  std::reverse(out.words.begin(), out.words.end());
  std::reverse(out.arcs.begin(), out.arcs.end());
  out.counts[0] = ins + del + sub; out.counts[1] = ins; out.counts[2] = del; out.counts[3] = sub;
  out.status = KHG_LAT_SUCCEEDED;
  return out;
}

LatticeMbr Lattice::Mbr(float graph_scale, float acoustic_scale, bool decode_mbr, int max_iter, const std::vector<int32_t>* init, int max_words,
                        const std::vector<double>* arc_cond, const std::vector<double>* final_cond) const {
  KHG_REQUIRE(max_iter >= 0, "Lattice::Mbr: max_iter must be >= 0");
  KHG_REQUIRE(max_words >= 0 && max_words <= 2047, "Lattice::Mbr: max_words must lie in 0 .. 2047");
  KHG_REQUIRE((arc_cond == nullptr) == (final_cond == nullptr), "Lattice::Mbr: arc_cond and final_cond come together");
  if (init) for (int32_t w : *init) KHG_REQUIRE(w > 0, "Lattice::Mbr: an initial word is not > 0");
  const double INF = std::numeric_limits<double>::infinity(), NINF = -INF;
  const float FINF = std::numeric_limits<float>::infinity();
  const double gs = graph_scale, as = acoustic_scale;
  LatticeMbr out;
  out.bayes_risk = INF;
  const LatticePosteriors fb = ForwardBackward(graph_scale, acoustic_scale);      // (refuses bad scales)
  out.status = fb.status;
  const int N = NumStates();
  const int64_t A = NumArcs();
  out.arc_cond.assign((size_t)A, 0.0);
  out.final_cond.assign((size_t)N, 0.0);
  if (!(fb.status & KHG_LAT_SUCCEEDED)) return out;
  std::vector<int32_t> src((size_t)A);
  std::vector<std::vector<int32_t>> in((size_t)N);      // ascending arc number
  for (int s = 0; s < N; ++s)
    for (int a = arc_begin[(size_t)s]; a < arc_begin[(size_t)s + 1]; ++a) { src[(size_t)a] = s; in[(size_t)nextstate[(size_t)a]].push_back(a); }
  const int T = frame[(size_t)N - 1];
  int last_lo = N - 1;
  while (last_lo > 0 && frame[(size_t)last_lo - 1] == T) --last_lo;
  if (arc_cond) {
    KHG_REQUIRE((int64_t)arc_cond->size() == A && (int)final_cond->size() == N, "Lattice::Mbr: one arc_cond per arc, one final_cond per state");
    out.arc_cond = *arc_cond; out.final_cond = *final_cond;
  } else {
    for (int64_t a = 0; a < A; ++a) {
      const double al = fb.alpha[(size_t)src[(size_t)a]], ad = fb.alpha[(size_t)nextstate[(size_t)a]];
      if (al == NINF || ad == NINF) continue;
      const double g = gs * (double)graph_cost[(size_t)a];
      const double c = ilabel[(size_t)a] != 0 ? as * (double)acoustic_cost[(size_t)a] : 0.0;
      out.arc_cond[(size_t)a] = std::exp((al + -(g + c)) - ad);
    }
    for (int s = last_lo; s < N; ++s)
      if (final_cost[(size_t)s] != FINF && fb.alpha[(size_t)s] != NINF)
        out.final_cond[(size_t)s] = std::exp((fb.alpha[(size_t)s] + -(gs * (double)final_cost[(size_t)s])) - fb.tot_like);
  }
  // the vocabulary, every arc's index into it, the longest path's words
  out.vocab.assign(1, 0);
  for (int32_t w : olabel) if (w != 0) out.vocab.push_back(w);
  std::sort(out.vocab.begin() + 1, out.vocab.end());
  out.vocab.erase(std::unique(out.vocab.begin() + 1, out.vocab.end()), out.vocab.end());
  const int V = (int)out.vocab.size();
  auto index_of = [&](int32_t w) { const auto it = std::lower_bound(out.vocab.begin() + 1, out.vocab.end(), w); return it != out.vocab.end() && *it == w ? (int)(it - out.vocab.begin()) : (w == 0 ? 0 : -1); };
  int32_t longest = 0;
  {
    std::vector<int32_t> L((size_t)N, -1);
    L[(size_t)start] = 0;
    for (int64_t a = 0; a < A; ++a) {
      const int s = src[(size_t)a], d = nextstate[(size_t)a];
      if (L[(size_t)s] >= 0) L[(size_t)d] = std::max(L[(size_t)d], L[(size_t)s] + (olabel[(size_t)a] != 0 ? 1 : 0));
    }
    for (int s = last_lo; s < N; ++s) if (final_cost[(size_t)s] != FINF) longest = std::max(longest, L[(size_t)s]);
  }
  std::vector<int32_t> h;
  if (init) h = *init;
  else { const LatticeBestPath b = BestPath(graph_scale, acoustic_scale); if (b.status & KHG_LAT_SUCCEEDED) h = b.words; }
  const int64_t cap = max_words > 0 ? max_words : std::max<int64_t>((int64_t)h.size(), longest);
  out.cap = (int32_t)std::min<int64_t>(cap, INT32_MAX);
  if ((int64_t)h.size() > cap || cap > 2047) { out.status = KHG_LAT_WORDS; return out; }
  const double DEL = 1.0 + 1e-5;
  // in-arc j of state n (n == N: the virtual end state): source, word, weight
  auto degree = [&](int n) { return n < N ? (int)in[(size_t)n].size() : N - last_lo; };
  auto in_arc = [&](int n, int j, int* s, int32_t* w, double* p) {
    if (n < N) { const int a = in[(size_t)n][(size_t)j]; *s = src[(size_t)a]; *w = olabel[(size_t)a]; *p = out.arc_cond[(size_t)a]; }
    else { *s = last_lo + j; *w = 0; *p = out.final_cond[(size_t)(last_lo + j)]; }
  };
  std::vector<double> AD, BD, G, arc, ba;
  std::vector<unsigned char> b;
  for (;;) {
    const int W = (int)h.size(), Q = 2 * W + 1, C = Q + 1;
    auto r = [&](int q) { return (q & 1) ? 0 : h[(size_t)(q / 2 - 1)]; };
    auto row = [&](const double* ADs, int32_t w) {      // arc[0 .. Q] and b[1 .. Q]
      const double delw = w != 0 ? DEL : 0.0;
      arc[0] = ADs[0] + delw;
      for (int q = 1; q <= Q; ++q) {
        const int32_t rq = r(q);
        const double a1 = ADs[q - 1] + (w == rq ? 0.0 : 1.0), a2 = ADs[q] + delw, a3 = arc[(size_t)q - 1] + (rq != 0 ? 1.0 : 0.0);
        if (a1 <= a2 && a1 <= a3) { b[(size_t)q] = 1; arc[(size_t)q] = a1; }
        else if (a2 < a1 && a2 <= a3) { b[(size_t)q] = 2; arc[(size_t)q] = a2; }
        else { b[(size_t)q] = 3; arc[(size_t)q] = a3; }
      }
    };
    AD.assign((size_t)(N + 1) * C, 0.0); BD.assign((size_t)(N + 1) * C, 0.0); G.assign((size_t)Q * V, 0.0);
    arc.assign((size_t)C, 0.0); ba.assign((size_t)C + 1, 0.0); b.assign((size_t)C + 1, 0);
    for (int q = 1; q <= Q; ++q) AD[(size_t)start * C + q] = AD[(size_t)start * C + q - 1] + (r(q) != 0 ? 1.0 : 0.0);
    for (int n = 0; n <= N; ++n) {
      if (n == start) continue;
      for (int j = 0; j < degree(n); ++j) {
        int s; int32_t w; double p;
        in_arc(n, j, &s, &w, &p);
        if (p == 0.0) continue;
        row(&AD[(size_t)s * C], w);
        for (int q = 0; q <= Q; ++q) { const double pv = p * arc[(size_t)q]; AD[(size_t)n * C + q] = AD[(size_t)n * C + q] + pv; }
      }
    }
    const double risk = AD[(size_t)N * C + Q];
    out.risks.push_back(risk);
    BD[(size_t)N * C + Q] = 1.0;
    for (int n = N; n >= 0; --n) {
      if (n == start) continue;
      for (int j = 0; j < degree(n); ++j) {
        int s; int32_t w; double p;
        in_arc(n, j, &s, &w, &p);
        if (p == 0.0) continue;
        row(&AD[(size_t)s * C], w);
        const int wi = index_of(w);
        b[(size_t)Q + 1] = 0; ba[(size_t)Q + 1] = 0.0;
        for (int q = Q; q >= 1; --q) {
          const double t = p * BD[(size_t)n * C + q];
          const double x = (b[(size_t)q + 1] == 3 ? ba[(size_t)q + 1] : 0.0) + t;
          ba[(size_t)q] = x;
          if (b[(size_t)q] == 1) { BD[(size_t)s * C + q - 1] = BD[(size_t)s * C + q - 1] + x; G[(size_t)(q - 1) * V + wi] = G[(size_t)(q - 1) * V + wi] + x; }
          else if (b[(size_t)q] == 2) BD[(size_t)s * C + q] = BD[(size_t)s * C + q] + x;
          else G[(size_t)(q - 1) * V] = G[(size_t)(q - 1) * V] + x;
        }
        const double t0 = p * BD[(size_t)n * C];
        const double x0 = (b[1] == 3 ? ba[1] : 0.0) + t0;
        BD[(size_t)s * C] = BD[(size_t)s * C] + x0;
      }
    }
    {
      double x = 0.0;
      for (int q = Q; q >= 1; --q) { x = x + BD[(size_t)start * C + q]; G[(size_t)(q - 1) * V] = G[(size_t)(q - 1) * V] + x; }
    }
    bool stop = !decode_mbr;
    std::vector<int32_t> hn;
    if (!stop) {
      for (int q = 1; q <= Q; ++q) {
        int bi = 0;
        for (int x = 1; x < V; ++x) if (G[(size_t)(q - 1) * V + bi] < G[(size_t)(q - 1) * V + x]) bi = x;
        if (out.vocab[(size_t)bi] != 0) hn.push_back(out.vocab[(size_t)bi]);
      }
      if (hn == h) stop = true;
      else if (out.iters == max_iter) { out.status |= KHG_LAT_NOT_CONVERGED; stop = true; }
      else if ((int64_t)hn.size() > cap) {
        out.status = KHG_LAT_WORDS;
        return out;
      }
    }
    if (stop) {
      out.bayes_risk = risk;
      out.words = h;
      out.gamma = G;
      out.conf.assign((size_t)W, 0.0);
      for (int i = 0; i < W; ++i) { const int wi = index_of(h[(size_t)i]); if (wi >= 0) out.conf[(size_t)i] = G[(size_t)(2 * i + 1) * V + wi]; }
      return out;
    }
    h.swap(hn);
    ++out.iters;
  }
}

std::shared_ptr<Lattice> Lattice::Prune(float beam, float gs, float as, int* status) const {
  KHG_REQUIRE(beam >= 0.0f, "Lattice::Prune: beam must be >= 0");
  auto out = std::make_shared<Lattice>();
  out->arc_begin.push_back(0);
  const LatticeBestPath b = BestPath(gs, as);
  int st = b.status;
  std::vector<float> e1, e2;
  if ((st & KHG_LAT_SUCCEEDED) && !Backward(gs, as, &e1, &e2)) st = KHG_LAT_EPS_LOOP;
  if (status) *status = st;
  if (!(st & KHG_LAT_SUCCEEDED)) return out;
  const float INF = std::numeric_limits<float>::infinity();
  const int N = NumStates();
  const std::vector<float>&d1 = b.alpha1, &d2 = b.alpha2;
  const float best = b.f1 + b.f2;
  const float limit = best + beam;
  // the best path: its states, and per state the arc it leaves by
  std::vector<int32_t> path_arc((size_t)N, -1);
  std::vector<char> on((size_t)N, 0);
  on[(size_t)start] = 1; on[(size_t)b.final_state] = 1;
  {
    int n = start;
    for (int a : b.arcs) { path_arc[(size_t)n] = a; on[(size_t)n] = 1; n = nextstate[(size_t)a]; on[(size_t)n] = 1; }
  }
  std::vector<int32_t> newid((size_t)N, -1);
  int kept = 0;
  for (int s = 0; s < N; ++s) {
    bool k = on[(size_t)s] != 0;
    if (!k && d1[(size_t)s] != INF && e1[(size_t)s] != INF) {
      const float t1 = d1[(size_t)s] + e1[(size_t)s], t2 = d2[(size_t)s] + e2[(size_t)s];
      const float tot = t1 + t2;
      k = tot <= limit;
    }
    if (k) newid[(size_t)s] = kept++;
  }
  out->arc_begin.clear();
  for (int s = 0; s < N; ++s) {
    if (newid[(size_t)s] < 0) continue;
    out->frame.push_back(frame[(size_t)s]); out->graph_state.push_back(graph_state[(size_t)s]); out->tot_cost.push_back(tot_cost[(size_t)s]);
    out->extra_cost.push_back(extra_cost[(size_t)s]); out->final_cost.push_back(final_cost[(size_t)s]);
    out->arc_begin.push_back((int32_t)out->ilabel.size());
    for (int a = arc_begin[(size_t)s]; a < arc_begin[(size_t)s + 1]; ++a) {
      const int k = nextstate[(size_t)a];
      if (newid[(size_t)k] < 0) continue;
      const float w1 = gs * graph_cost[(size_t)a], w2 = ilabel[(size_t)a] != 0 ? as * acoustic_cost[(size_t)a] : 0.0f;
      const float p1 = d1[(size_t)s] + w1, p2 = d2[(size_t)s] + w2;
      const float t1 = p1 + e1[(size_t)k], t2 = p2 + e2[(size_t)k];
      const float tot = t1 + t2;
      if (!(tot <= limit) && path_arc[(size_t)s] != a) continue;
      out->ilabel.push_back(ilabel[(size_t)a]); out->olabel.push_back(olabel[(size_t)a]); out->graph_cost.push_back(graph_cost[(size_t)a]);
      out->acoustic_cost.push_back(acoustic_cost[(size_t)a]); out->nextstate.push_back(newid[(size_t)k]);
    }
  }
  out->arc_begin.push_back((int32_t)out->ilabel.size());
  out->start = newid[(size_t)start];
  return out;
}

void FasterDecoder::SetOptions(const FasterDecoderOptions& c) {
  KHG_REQUIRE(c.hash_ratio >= 1.0f && c.max_active > 1 && c.min_active >= 0 && c.min_active < c.max_active,
              "FasterDecoder: bad options (hash_ratio >= 1, max_active > 1, 0 <= min_active < max_active)");
  cfg_ = c;
}
void FasterDecoder::InitDecoding() {
  KHG_REQUIRE(fst_ && fst_->Start() >= 0, "start_state != fst::kNoStateId assertion failed");
  has_res_ = false;
  nframes_ = 0;
}
namespace {
struct TmH { khg_tm* h = nullptr; ~TmH() { if (h) khg_tm_destroy(h); } };
struct UttsH { khg_utts* h = nullptr; ~UttsH() { if (h) khg_utts_destroy(h); } };
}  // namespace

AlignResult AlignDecodable(const StdVectorFst& fst, const DecodableInterface& dec, const AlignConfig& config, float like_scale,
                           const FasterDecoderOptions* dopts) {
  KHG_REQUIRE(!((config.retry_beam != 0 && config.retry_beam <= config.beam) || config.beam <= 0.0f), "Beams do not make sense");
  const int64_t T = dec.NumFramesReady();
  AlignResult r;
  r.num_frames = (int)T;
  const GraphsCsr g = ConcatGraphs({&fst});
  // the indices the decoder can ask for = the non-epsilon input labels of the graph; "pdf" j of the synthetic table is index j + 1
  int max_index = 0;
  for (int32_t l : g.ilabel) {
    KHG_REQUIRE(l >= 0, "AlignDecodable: negative input label on the graph");
    max_index = std::max(max_index, (int)l);
  }
  if (fst.Start() == kNoStateId || max_index == 0 || T <= 0) {       // nothing K2 could decode: same outcome as the GMM path
    r.status = KHG_ALIGN_ERROR;
    return r;
  }
  KHG_REQUIRE(max_index <= dec.NumIndices(), "AlignDecodable: the graph carries index " + std::to_string(max_index) + " but the decodable has " +
                                                 std::to_string(dec.NumIndices()));
  std::vector<int32_t> id2pdf((size_t)max_index + 1);
  id2pdf[0] = -1;
  for (int i = 1; i <= max_index; ++i) id2pdf[(size_t)i] = i - 1;
  khg_ctx* ctx = DefaultCtx();
  TmH dt; UttsH us;
  CApi(khg_tm_create(ctx, max_index, id2pdf.data(), &dt.h));
  const int64_t frame_off[2] = {0, T};
  const std::vector<float> no_feats((size_t)T, 0.0f);                // K2 reads scores, never features
  CApi(khg_utts_create(ctx, dt.h, 1, 1, frame_off, no_feats.data(), nullptr, g.state_off.data(), g.start.data(), g.arc_off.data(), g.ilabel.data(),
                       g.olabel.data(), g.weight.data(), g.nextstate.data(), g.final_w.data(), &us.h));
  int64_t pdf_off[2] = {0, 0}, ll_off[2] = {0, 0}, total = 0;
  CApi(khg_utts_num_pdfs(us.h, pdf_off));
  const int n = (int)pdf_off[1];
  r.pdfs.resize((size_t)n);
  CApi(khg_utts_pdfs(us.h, r.pdfs.data()));
  CApi(khg_loglikes_layout(us.h, ll_off, &total));
  const int64_t tpad = (T + 31) & ~int64_t(31);
  KHG_REQUIRE(total >= (int64_t)n * tpad, "AlignDecodable: unexpected score layout");
  std::vector<float> scores((size_t)total, 0.0f);
  r.loglikes.resize((size_t)n * (size_t)T);
  const DecodableCtc* ctc = dynamic_cast<const DecodableCtc*>(&dec);
  for (int j = 0; j < n; ++j)
    for (int64_t t = 0; t < T; ++t) {
      const float s = DecodableScore(dec, ctc, (int)t, r.pdfs[(size_t)j] + 1);
      scores[(size_t)(ll_off[0] + (int64_t)j * tpad + t)] = s;
      r.loglikes[(size_t)j * (size_t)T + (size_t)t] = s;
    }
  CApi(khg_loglikes_upload(ctx, us.h, scores.data()));
  khg_align_config c;
  khg_align_config_default(&c);
  c.beam = config.beam; c.retry_beam = config.retry_beam; c.careful = config.careful ? 1 : 0;
  c.acoustic_scale = 1.0f;                      // 1.0f * s == s: the decodable scaled its scores itself
  c.like_scale = like_scale;
  if (dopts) { c.max_active = dopts->max_active; c.min_active = dopts->min_active; c.beam_delta = dopts->beam_delta; c.hash_ratio = dopts->hash_ratio; }
  const int64_t wcap = T + 1040;
  std::vector<int32_t> ali((size_t)T), words((size_t)wcap);
  int64_t woff[2] = {0, 0};
  float like = 0.0f;
  int32_t status = 0;
  CApi(khg_align(ctx, dt.h, us.h, &c, ali.data(), words.data(), woff, wcap, &like, &status));
  r.status = status;
  r.ok = (status & KHG_ALIGN_ERROR) == 0;
  r.retried = (status & KHG_ALIGN_RETRIED) != 0;
  if (r.ok) {
    r.alignment = std::move(ali);
    r.words.assign(words.begin() + woff[0], words.begin() + woff[1]);
    r.like = like;
  }
  return r;
}

namespace {
// the graph's index table and the decodable's scores of every (frame, index on the graph), sampled through the interface (as
// AlignDecodable does), on a one-utterance set; then `on_set(ctx, tm, set, T)`
template <class OnSet>
LatticeResult WithDecodableSet(const StdVectorFst& fst, const DecodableInterface& dec, const std::string& name, OnSet on_set) {
  const int64_t T = dec.NumFramesReady();
  const GraphsCsr g = ConcatGraphs({&fst});
  int max_index = 0;
  for (int32_t l : g.ilabel) {
    KHG_REQUIRE(l >= 0, name + ": negative input label on the graph");
    max_index = std::max(max_index, (int)l);
  }
  KHG_REQUIRE(max_index <= dec.NumIndices(), name + ": the graph carries index " + std::to_string(max_index) +
                                                 " but the decodable has " + std::to_string(dec.NumIndices()));
  std::vector<int32_t> id2pdf((size_t)max_index + 1);
  id2pdf[0] = -1;
  for (int i = 1; i <= max_index; ++i) id2pdf[(size_t)i] = i - 1;
  khg_ctx* ctx = DefaultCtx();
  TmH dt; UttsH us;
  CApi(khg_tm_create(ctx, std::max(max_index, 1), id2pdf.data(), &dt.h));
  const int64_t frame_off[2] = {0, T};
  const std::vector<float> no_feats((size_t)std::max<int64_t>(T, 1), 0.0f);
  CApi(khg_utts_create(ctx, dt.h, 1, 1, frame_off, no_feats.data(), nullptr, g.state_off.data(), g.start.data(), g.arc_off.data(), g.ilabel.data(),
                       g.olabel.data(), g.weight.data(), g.nextstate.data(), g.final_w.data(), &us.h));
  int64_t pdf_off[2] = {0, 0}, ll_off[2] = {0, 0}, total = 0;
  CApi(khg_utts_num_pdfs(us.h, pdf_off));
  const int n = (int)pdf_off[1];
  std::vector<int32_t> pdfs((size_t)std::max(n, 1));
  CApi(khg_utts_pdfs(us.h, pdfs.data()));
  CApi(khg_loglikes_layout(us.h, ll_off, &total));
  const int64_t tpad = (T + 31) & ~int64_t(31);
  std::vector<float> scores((size_t)std::max<int64_t>(total, 1), 0.0f);
  const DecodableCtc* ctc = dynamic_cast<const DecodableCtc*>(&dec);
  for (int j = 0; j < n; ++j)
    for (int64_t t = 0; t < T; ++t)
      scores[(size_t)(ll_off[0] + (int64_t)j * tpad + t)] = DecodableScore(dec, ctc, (int)t, pdfs[(size_t)j] + 1);
  CApi(khg_loglikes_upload(ctx, us.h, scores.data()));
  LatticeResult r = on_set(ctx, dt.h, us.h, T);
  r.num_frames = (int)T;
  return r;
}
}  // namespace

LatticeResult DecodeLatticeDecodable(const StdVectorFst& fst, const DecodableInterface& dec, const LatticeFasterDecoderConfig& config,
                                     bool allow_partial, int scratch_per_frame) {
  config.Check();
  KHG_REQUIRE(fst.Start() != kNoStateId, "start_state != fst::kNoStateId assertion failed");   // lattice-faster-decoder.cc:72
  KHG_REQUIRE(dec.NumFramesReady() > 0, "num_frames > 0 assertion failed");     // GetRawLattice (lattice-faster-decoder.cc:137)
  return WithDecodableSet(fst, dec, "decode_utterance_lattice_faster", [&](khg_ctx* ctx, khg_tm* dt, khg_utts* us, int64_t T) {
    // 1.0f * s == s: the decodable scaled its scores itself
    return DecodeLatticeOnSet(ctx, dt, us, {0, T}, config, 1.0f, allow_partial, scratch_per_frame, (int64_t)fst.NumStates())[0];
  });
}

LatticeResult DecodeLatticeSimpleDecodable(const StdVectorFst& fst, const DecodableInterface& dec, const LatticeSimpleDecoderConfig& config,
                                           bool allow_partial, int scratch_per_frame) {
  config.Check();
  KHG_REQUIRE(fst.Start() != kNoStateId, "Check failed!\nx: start_state != fst::kNoStateId");   // lattice-simple-decoder.cc:52
  return WithDecodableSet(fst, dec, "decode_utterance_lattice_simple", [&](khg_ctx* ctx, khg_tm* dt, khg_utts* us, int64_t T) {
    return DecodeLatticeSimpleOnSet(ctx, dt, us, {0, T}, config, 1.0f, allow_partial, scratch_per_frame, (int64_t)fst.NumStates())[0];
  });
}

void FasterDecoder::AdvanceDecoding(const std::shared_ptr<DecodableInterface>& dec, int max_num_frames) {
  KHG_REQUIRE(dec != nullptr, "FasterDecoder: no decodable");
  KHG_REQUIRE(!(max_num_frames >= 0 && max_num_frames < dec->NumFramesReady()),
              "FasterDecoder.advanced_decoding: partial decoding (max_num_frames) is not supported on the HIP path");
  KHG_REQUIRE(nframes_ >= 0, "num_frames_decoded_ >= 0 assertion failed: call init_decoding() first");
  AlignConfig cfg;
  cfg.beam = cfg_.beam; cfg.retry_beam = 0.0f;
  dec_ = dec;
  ac_.clear();
  if (auto gmm = std::dynamic_pointer_cast<DecodableAmDiagGmmScaled>(dec)) {       // K1 + K2
    const GraphsCsr g = ConcatGraphs({fst_.get()});
    res_ = AlignBatch(*gmm->am(), *gmm->tm(), g, {gmm->feats().data()}, {(int64_t)gmm->NumFramesReady()}, cfg, gmm->scale(), nullptr, &cfg_, true)[0];
    if (res_.ok) {
      const TransitionModel& tm = *gmm->tm();
      const size_t T = res_.alignment.size();
      std::vector<int> col((size_t)tm.NumPdfs(), -1);
      for (size_t i = 0; i < res_.pdfs.size(); ++i) col[(size_t)res_.pdfs[i]] = (int)i;
      for (size_t i = 0; i < T; ++i) {
        const int c = col[(size_t)tm.TransitionIdToPdf(res_.alignment[i])];
        KHG_REQUIRE(c >= 0, "FasterDecoder: alignment uses a pdf outside the utterance's list");
        ac_.push_back((double)(-(gmm->scale() * res_.loglikes[(size_t)c * T + i])));
      }
    }
  } else {                                                                          // sampled scores + K2
    res_ = AlignDecodable(*fst_, *dec, cfg, 0.0f, &cfg_);
    if (res_.ok) {
      const size_t T = res_.alignment.size();
      for (size_t i = 0; i < T; ++i) {
        const auto it = std::lower_bound(res_.pdfs.begin(), res_.pdfs.end(), res_.alignment[i] - 1);
        KHG_REQUIRE(it != res_.pdfs.end() && *it == res_.alignment[i] - 1, "FasterDecoder: alignment uses an index outside the graph's");
        ac_.push_back((double)(-res_.loglikes[(size_t)(it - res_.pdfs.begin()) * T + i]));
      }
    }
  }
  has_res_ = true;
  nframes_ = dec->NumFramesReady();
}

bool FasterDecoder::GetBestPath(LinearLattice* lat, bool use_final_probs) const {
  *lat = LinearLattice();
  if (!ReachedFinal()) return false;     // the reference would fall back to the best non-final token; the HIP kernels keep no such token
  const std::vector<int32_t>& ali = res_.alignment;
  const int T = (int)ali.size(), S = fst_->NumStates();
  const double INF = std::numeric_limits<double>::infinity();
  const std::vector<double>& ac = ac_;
  // cheapest path through the graph with exactly this input-label sequence (= the decoder's best path); layers keep their states
  // in insertion order, a later candidate replaces an earlier one only when strictly cheaper
  struct Back { int prev = -1, arc = -1; };       // arc = index into Arcs(prev)
  struct Layer {
    std::vector<double> cost; std::vector<int> keys;
    explicit Layer(int S) : cost((size_t)S, std::numeric_limits<double>::infinity()) {}
    void Set(int s, double v) { if (cost[(size_t)s] == std::numeric_limits<double>::infinity()) keys.push_back(s); cost[(size_t)s] = v; }
  };
  std::vector<std::vector<Back>> bp_emit((size_t)T + 1, std::vector<Back>()), bp_eps((size_t)T + 1, std::vector<Back>());
  auto closure = [&](Layer& layer, std::vector<Back>& bp) {
    bp.assign((size_t)S, Back());
    std::vector<int> stack = layer.keys;
    while (!stack.empty()) {
      const int s = stack.back(); stack.pop_back();
      const double c = layer.cost[(size_t)s];
      const auto& arcs = fst_->Arcs(s);
      for (size_t k = 0; k < arcs.size(); ++k)
        if (arcs[k].ilabel == 0) {
          const double v = c + (double)arcs[k].weight;
          if (v < layer.cost[(size_t)arcs[k].nextstate]) {
            layer.Set(arcs[k].nextstate, v);
            bp[(size_t)arcs[k].nextstate] = Back{s, (int)k};
            stack.push_back(arcs[k].nextstate);
          }
        }
    }
  };
  Layer layer(S);
  layer.Set(fst_->Start(), 0.0);
  closure(layer, bp_eps[0]);
  for (int i = 0; i < T; ++i) {
    Layer nxt(S);
    bp_emit[(size_t)i + 1].assign((size_t)S, Back());
    for (int s : layer.keys) {
      const double c = layer.cost[(size_t)s];
      const auto& arcs = fst_->Arcs(s);
      for (size_t k = 0; k < arcs.size(); ++k)
        if (arcs[k].ilabel == ali[(size_t)i]) {
          const double v = c + (double)arcs[k].weight + ac[(size_t)i];
          if (v < nxt.cost[(size_t)arcs[k].nextstate]) {
            nxt.Set(arcs[k].nextstate, v);
            bp_emit[(size_t)i + 1][(size_t)arcs[k].nextstate] = Back{s, (int)k};
          }
        }
    }
    closure(nxt, bp_eps[(size_t)i + 1]);
    layer = std::move(nxt);
  }
  double best = INF;
  int bs = -1;
  for (int s : layer.keys)
    if (fst_->IsFinal(s) && layer.cost[(size_t)s] + (double)fst_->Final(s) < best) { best = layer.cost[(size_t)s] + (double)fst_->Final(s); bs = s; }
  if (bs < 0) return false;
  struct Step { int state, arc; bool emitting; double acost; };
  std::vector<Step> path;
  int s = bs;
  for (int i = T; i >= 0; --i) {
    while (bp_eps[(size_t)i][(size_t)s].prev >= 0) {            // epsilon hops inside layer i
      const Back b = bp_eps[(size_t)i][(size_t)s];
      path.push_back(Step{b.prev, b.arc, false, 0.0});
      s = b.prev;
    }
    if (i > 0) {
      const Back b = bp_emit[(size_t)i][(size_t)s];
      KHG_REQUIRE(b.prev >= 0, "FasterDecoder: broken back-pointer chain");
      path.push_back(Step{b.prev, b.arc, true, ac[(size_t)i - 1]});
      s = b.prev;
    }
  }
  std::reverse(path.begin(), path.end());
  lat->start = 0;
  LatticeWeight carry;
  for (const Step& st : path) {
    const StdArc& a = fst_->Arcs(st.state)[(size_t)st.arc];
    const LatticeWeight w{(double)a.weight + carry.value1, (st.emitting ? st.acost : 0.0) + carry.value2};
    if (a.ilabel == 0 && a.olabel == 0) { carry = w; continue; }      // RemoveEpsLocal on a linear lattice: fold true epsilons forward
    carry = LatticeWeight();
    lat->arcs.push_back(LatticeArc{a.ilabel, a.olabel, w, (int)lat->arcs.size() + 1});
  }
  const double fw = use_final_probs ? (double)fst_->Final(bs) : 0.0;
  lat->final_w = LatticeWeight{fw + carry.value1, carry.value2};
  return true;
}

}  // namespace khg
