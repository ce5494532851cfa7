// kaldi_hmm_gmm_amd/csrc/khg_host_tree.cpp -- Kaldi's BuildTree on host statistics and its C entry khg_build_tree.
// All arithmetic in double, one operation at a time (built with -ffp-contract=off), sums in the written order.
#include "khg_host_tree.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <map>
#include <set>
#include <stdexcept>

#include "../../include/khg_hip.h"

int khg_set_error(int code, const std::string& msg);      // khg_ctx_model.hip

namespace khg_tree {
namespace {

constexpr double kLog2Pi = 1.8378770664093454835606594728112;   // M_LOG_2PI

// GaussClusterable (csrc/clusterable-classes.cc:107-181): AddStats / Add / Objf, the objective kept in double
struct Gauss {
  double c = 0.0;
  std::vector<double> x, x2;
  explicit Gauss(int dim) : x((size_t)dim, 0.0), x2((size_t)dim, 0.0) {}
  void add_row(const Stats& st, int64_t r) {
    c += st.count[r];
    for (int d = 0; d < st.dim; ++d) { x[(size_t)d] += st.x[r * st.dim + d]; x2[(size_t)d] += st.x2[r * st.dim + d]; }
  }
  void add(const Gauss& o) {
    c += o.c;
    for (size_t d = 0; d < x.size(); ++d) { x[d] += o.x[d]; x2[d] += o.x2[d]; }
  }
  double objf(double var_floor) const {
    if (c <= 0.0) return 0.0;
    double per_frame = 0.0, logs = 0.0;
    for (size_t d = 0; d < x.size(); ++d) {
      const double mean = x[d] / c;
      const double var = x2[d] / c - mean * mean;
      const double floored = std::max(var, var_floor);
      per_frame += -0.5 * var / floored;
      logs += std::log(floored);
    }
    per_frame += -0.5 * (logs + kLog2Pi * (double)x.size());
    if (std::isnan(per_frame)) return 0.0;
    return per_frame * c;
  }
};

inline int32_t event_value(const Stats& st, int64_t r, int32_t key) { return st.keys[r * (st.N + 1) + (key < 0 ? st.N : key)]; }

int32_t map_event(const Node& n, const Stats& st, int64_t r) {
  switch (n.kind) {
    case Node::CE: return n.answer;
    case Node::TE: {
      const int32_t v = event_value(st, r, n.key);
      if (v < 0 || (size_t)v >= n.table.size() || !n.table[(size_t)v]) return -1;
      return map_event(*n.table[(size_t)v], st, r);
    }
    default: {
      const int32_t v = event_value(st, r, n.key);
      return map_event(std::binary_search(n.yes_set.begin(), n.yes_set.end(), v) ? *n.yes : *n.no, st, r);
    }
  }
}
void collect_leaves(Node* n, std::vector<Node*>* out) {
  if (!n) return;
  if (n->kind == Node::CE) { out->push_back(n); return; }
  if (n->kind == Node::TE) { for (auto& e : n->table) collect_leaves(e.get(), out); return; }
  collect_leaves(n->yes.get(), out);
  collect_leaves(n->no.get(), out);
}
std::unique_ptr<Node> make_ce(int32_t answer) {
  auto n = std::make_unique<Node>();
  n->kind = Node::CE; n->answer = answer;
  return n;
}

struct Leaf {
  int32_t id = 0;
  Node* node = nullptr;
  std::vector<int64_t> rows;
  double best_impr = 0.0;
  int32_t best_qkey = 0, best_q = -1;          // index into Questions::keys / its sets; best_q < 0: no candidate
};

// the best split of a leaf: question keys ascending, sets in the caller's order, the first strictly greater improvement wins
void find_best_split(const Stats& st, const Questions& q, double var_floor, Leaf* leaf) {
  leaf->best_q = -1; leaf->best_impr = 0.0;
  if (leaf->rows.size() < 2) return;
  Gauss total(st.dim);
  for (int64_t r : leaf->rows) total.add_row(st, r);
  const double unsplit = total.objf(var_floor);
  bool have = false;
  for (size_t ki = 0; ki < q.keys.size(); ++ki) {
    std::map<int32_t, Gauss> by_value;           // ascending value; each value's rows in row order
    for (int64_t r : leaf->rows) {
      auto it = by_value.find(event_value(st, r, q.keys[ki]));
      if (it == by_value.end()) it = by_value.emplace(event_value(st, r, q.keys[ki]), Gauss(st.dim)).first;
      it->second.add_row(st, r);
    }
    if (by_value.size() < 2) continue;
    for (size_t qi = 0; qi < q.sets[ki].size(); ++qi) {
      const std::vector<int32_t>& set = q.sets[ki][qi];
      Gauss yes(st.dim), no(st.dim);
      size_t nyes = 0, nno = 0;
      for (const auto& kv : by_value) {
        if (std::binary_search(set.begin(), set.end(), kv.first)) { yes.add(kv.second); ++nyes; }
        else { no.add(kv.second); ++nno; }
      }
      if (nyes == 0 || nno == 0) continue;
      const double impr = yes.objf(var_floor) + no.objf(var_floor) - unsplit;
      if (!have || impr > leaf->best_impr) { have = true; leaf->best_impr = impr; leaf->best_qkey = (int32_t)ki; leaf->best_q = (int32_t)qi; }
    }
  }
}

void write_token(std::string* s, const char* t) { s->append(t); s->push_back(' '); }
void write_i32(std::string* s, int32_t v) { s->push_back('\x04'); s->append(reinterpret_cast<const char*>(&v), 4); }
void write_u32(std::string* s, uint32_t v) { s->push_back((char)-4); s->append(reinterpret_cast<const char*>(&v), 4); }
void write_node(std::string* s, const Node* n) {
  if (!n) { write_token(s, "NULL"); return; }
  if (n->kind == Node::CE) { write_token(s, "CE"); write_i32(s, n->answer); return; }
  if (n->kind == Node::TE) {
    write_token(s, "TE"); write_i32(s, n->key); write_u32(s, (uint32_t)n->table.size()); write_token(s, "(");
    for (const auto& e : n->table) write_node(s, e.get());
    write_token(s, ")");
    return;
  }
  write_token(s, "SE"); write_i32(s, n->key);
  write_i32(s, (int32_t)n->yes_set.size());
  if (!n->yes_set.empty()) s->append(reinterpret_cast<const char*>(n->yes_set.data()), 4 * n->yes_set.size());
  write_token(s, "{");
  write_node(s, n->yes.get());
  write_node(s, n->no.get());
  write_token(s, "}");
}

}  // namespace

// csrc/build-tree-utils.cc:18-121; the node structure of context_dep.get_stub_map
std::unique_ptr<Node> get_stub_map(int32_t P, const std::vector<std::vector<int32_t>>& phone_sets, const std::vector<int32_t>& p2n, const std::vector<bool>& share_roots,
                                   int32_t* num_leaves) {
  if (phone_sets.empty() || share_roots.size() != phone_sets.size()) throw std::invalid_argument("GetStubMap: bad arguments");
  size_t max_set_size = 0; int32_t highest = 0;
  for (const auto& ps : phone_sets) { max_set_size = std::max(max_set_size, ps.size()); highest = std::max(highest, ps.back()); }
  if (phone_sets.size() == 1) {
    if (share_roots[0]) return make_ce((*num_leaves)++);
    int32_t max_len = 0;
    for (int32_t phone : phone_sets[0]) {
      if (phone < 0 || (size_t)phone >= p2n.size() || p2n[(size_t)phone] <= 0) throw std::invalid_argument("GetStubMap: phone " + std::to_string(phone) + " has no pdf classes");
      max_len = std::max(max_len, p2n[(size_t)phone]);
    }
    auto n = std::make_unique<Node>();
    n->kind = Node::TE; n->key = -1;
    for (int32_t pos = 0; pos < max_len; ++pos) n->table.push_back(make_ce((*num_leaves)++));
    return n;
  }
  if (max_set_size == 1 && (int64_t)phone_sets.size() <= 2 * (int64_t)highest) {
    auto n = std::make_unique<Node>();
    n->kind = Node::TE; n->key = P;
    n->table.resize((size_t)highest + 1);
    for (size_t i = 0; i < phone_sets.size(); ++i)
      n->table[(size_t)phone_sets[i][0]] = get_stub_map(P, {phone_sets[i]}, p2n, {share_roots[i]}, num_leaves);
    return n;
  }
  const size_t half = phone_sets.size() / 2;
  std::vector<std::vector<int32_t>> s1(phone_sets.begin(), phone_sets.begin() + half), s2(phone_sets.begin() + half, phone_sets.end());
  std::vector<bool> r1(share_roots.begin(), share_roots.begin() + half), r2(share_roots.begin() + half, share_roots.end());
  auto n = std::make_unique<Node>();
  n->kind = Node::SE; n->key = P;
  n->yes = get_stub_map(P, s1, p2n, r1, num_leaves);
  n->no = get_stub_map(P, s2, p2n, r2, num_leaves);
  for (const auto& ps : s1) n->yes_set.insert(n->yes_set.end(), ps.begin(), ps.end());
  std::sort(n->yes_set.begin(), n->yes_set.end());
  return n;
}

Result build_tree(const Stats& st, const Questions& q, const std::vector<std::vector<int32_t>>& phone_sets, const std::vector<int32_t>& p2n,
                  const std::vector<bool>& share_roots, const std::vector<bool>& do_split, double thresh, int32_t max_leaves, double cluster_thresh, double var_floor) {
  if (st.N < 1 || st.N > KHG_TREE_MAX_CONTEXT || st.P < 0 || st.P >= st.N) throw std::invalid_argument("unsupported context: N = " + std::to_string(st.N) + ", P = " + std::to_string(st.P));
  if (st.dim < 1 || st.num < 0) throw std::invalid_argument("bad statistics");
  if (phone_sets.empty() || share_roots.size() != phone_sets.size() || do_split.size() != phone_sets.size()) throw std::invalid_argument("one share_roots / do_split entry per phone set is needed");
  if (std::isnan(thresh) || std::isnan(cluster_thresh) || !(var_floor >= 0.0)) throw std::invalid_argument("a threshold is not a number");
  std::set<int32_t> seen, nonsplit;
  for (size_t i = 0; i < phone_sets.size(); ++i) {
    const auto& ps = phone_sets[i];
    if (ps.empty()) throw std::invalid_argument("an empty phone set");
    for (size_t j = 0; j < ps.size(); ++j) {
      if (ps[j] < 1 || ps[j] > KHG_TREE_MAX_PHONE) throw std::invalid_argument("phone " + std::to_string(ps[j]) + " in a phone set");
      if (j > 0 && ps[j] <= ps[j - 1]) throw std::invalid_argument("phone sets must be sorted and unique");
      if (!seen.insert(ps[j]).second) throw std::invalid_argument("phone " + std::to_string(ps[j]) + " is in two phone sets");
      if (!do_split[i]) nonsplit.insert(ps[j]);
    }
  }
  for (size_t i = 0; i < q.keys.size(); ++i) {
    if (q.keys[i] < -1 || q.keys[i] >= st.N) throw std::invalid_argument("question key " + std::to_string(q.keys[i]));
    if (i > 0 && q.keys[i] <= q.keys[i - 1]) throw std::invalid_argument("question keys must ascend");
    for (const auto& s : q.sets[i])
      for (size_t j = 1; j < s.size(); ++j)
        if (s[j] <= s[j - 1]) throw std::invalid_argument("question sets must be sorted and unique");
  }
  for (int64_t r = 0; r < st.num; ++r) {
    for (int j = 0; j < st.N; ++j)
      if (event_value(st, r, j) < 0 || event_value(st, r, j) > KHG_TREE_MAX_PHONE) throw std::invalid_argument("statistics row " + std::to_string(r) + " holds phone " + std::to_string(event_value(st, r, j)));
    if (event_value(st, r, -1) < 0 || event_value(st, r, -1) > KHG_TREE_MAX_PDF_CLASS) throw std::invalid_argument("statistics row " + std::to_string(r) + " holds pdf-class " + std::to_string(event_value(st, r, -1)));
  }

  Result res;
  res.tree = get_stub_map(st.P, phone_sets, p2n, share_roots, &res.num_leaves);
  std::vector<int32_t> stub_leaf((size_t)st.num);
  for (int64_t r = 0; r < st.num; ++r) {
    stub_leaf[(size_t)r] = map_event(*res.tree, st, r);
    if (stub_leaf[(size_t)r] < 0)
      throw std::invalid_argument("statistics row " + std::to_string(r) + " (central phone " + std::to_string(event_value(st, r, st.P)) + ", pdf-class " +
                                  std::to_string(event_value(st, r, -1)) + ") maps to no leaf: its phone is in no phone set");
  }
  // ---- SplitDecisionTree ----
  std::vector<Leaf> leaves;
  {
    std::vector<Node*> ce;
    collect_leaves(res.tree.get(), &ce);
    leaves.resize(ce.size());
    for (Node* n : ce) { leaves[(size_t)n->answer].id = n->answer; leaves[(size_t)n->answer].node = n; }
    for (int64_t r = 0; r < st.num; ++r)
      if (!nonsplit.count(event_value(st, r, st.P))) leaves[(size_t)stub_leaf[(size_t)r]].rows.push_back(r);
    for (Leaf& l : leaves) find_best_split(st, q, var_floor, &l);
  }
  double smallest_split = 1e10;
  while (max_leaves <= 0 || res.num_leaves < max_leaves) {
    int best = -1;
    for (size_t i = 0; i < leaves.size(); ++i)
      if (leaves[i].best_q >= 0 && (best < 0 || leaves[i].best_impr > leaves[(size_t)best].best_impr)) best = (int)i;
    if (best < 0 || !(leaves[(size_t)best].best_impr > thresh)) break;
    const int32_t qkey = q.keys[(size_t)leaves[(size_t)best].best_qkey];
    const std::vector<int32_t>& set = q.sets[(size_t)leaves[(size_t)best].best_qkey][(size_t)leaves[(size_t)best].best_q];
    res.objf_impr += leaves[(size_t)best].best_impr;
    smallest_split = std::min(smallest_split, leaves[(size_t)best].best_impr);
    Leaf no;
    no.id = res.num_leaves++;
    std::vector<int64_t> yes_rows;
    for (int64_t r : leaves[(size_t)best].rows) (std::binary_search(set.begin(), set.end(), event_value(st, r, qkey)) ? yes_rows : no.rows).push_back(r);
    Node* n = leaves[(size_t)best].node;
    n->kind = Node::SE; n->key = qkey; n->yes_set = set;
    n->yes = make_ce(leaves[(size_t)best].id);
    n->no = make_ce(no.id);
    leaves[(size_t)best].node = n->yes.get();
    leaves[(size_t)best].rows.swap(yes_rows);
    no.node = n->no.get();
    find_best_split(st, q, var_floor, &leaves[(size_t)best]);
    find_best_split(st, q, var_floor, &no);
    leaves.push_back(std::move(no));           // leaves[i].id == i throughout
  }
  // ---- ClusterEventMapRestrictedByMap: every row, the non-split roots' too ----
  if (cluster_thresh < 0.0) cluster_thresh = smallest_split;
  std::vector<int32_t> mapping((size_t)res.num_leaves);
  for (int32_t i = 0; i < res.num_leaves; ++i) mapping[(size_t)i] = i;
  if (cluster_thresh != 0.0) {
    std::map<int32_t, std::map<int32_t, Gauss>> groups;       // stub leaf -> leaf -> its rows' sum, in row order
    for (int64_t r = 0; r < st.num; ++r) {
      auto& g = groups[stub_leaf[(size_t)r]];
      const int32_t leaf = map_event(*res.tree, st, r);
      auto it = g.find(leaf);
      if (it == g.end()) it = g.emplace(leaf, Gauss(st.dim)).first;
      it->second.add_row(st, r);
    }
    for (auto& sg : groups) {
      std::vector<int32_t> ids; std::vector<Gauss> gs; std::vector<double> objf;
      for (auto& kv : sg.second) { ids.push_back(kv.first); gs.push_back(kv.second); objf.push_back(kv.second.objf(var_floor)); }
      const size_t n = ids.size();
      if (n < 2) continue;
      std::vector<char> alive(n, 1);
      std::vector<double> loss(n * n, 0.0);
      auto pair_loss = [&](size_t a, size_t b) { Gauss s = gs[a]; s.add(gs[b]); return objf[a] + objf[b] - s.objf(var_floor); };
      for (size_t a = 0; a < n; ++a) for (size_t b = a + 1; b < n; ++b) loss[a * n + b] = pair_loss(a, b);
      for (;;) {
        bool have = false; size_t ba = 0, bb = 0;
        for (size_t a = 0; a < n; ++a) {
          if (!alive[a]) continue;
          for (size_t b = a + 1; b < n; ++b)
            if (alive[b] && (!have || loss[a * n + b] < loss[ba * n + bb])) { have = true; ba = a; bb = b; }
        }
        if (!have || !(loss[ba * n + bb] < cluster_thresh)) break;
        res.cluster_loss += loss[ba * n + bb];
        res.num_removed++;
        gs[ba].add(gs[bb]);
        objf[ba] = gs[ba].objf(var_floor);
        alive[bb] = 0;
        mapping[(size_t)ids[bb]] = ids[ba];
        for (size_t o = 0; o < n; ++o) {
          if (!alive[o] || o == ba) continue;
          if (o < ba) loss[o * n + ba] = pair_loss(o, ba); else loss[ba * n + o] = pair_loss(ba, o);
        }
      }
    }
  }
  // ---- the mapping, then RenumberEventMap ----
  std::vector<Node*> ce;
  collect_leaves(res.tree.get(), &ce);
  std::set<int32_t> used;
  for (Node* n : ce) {
    int32_t a = n->answer;
    while (mapping[(size_t)a] != a) a = mapping[(size_t)a];
    n->answer = a;
    used.insert(a);
  }
  std::map<int32_t, int32_t> renum;
  for (int32_t a : used) { const int32_t k = (int32_t)renum.size(); renum[a] = k; }
  for (Node* n : ce) n->answer = renum[n->answer];
  res.num_leaves = (int32_t)renum.size();
  return res;
}

std::string write_context_dependency(int32_t N, int32_t P, const Node& to_pdf) {
  std::string s;
  write_token(&s, "ContextDependency");
  write_i32(&s, N); write_i32(&s, P);
  write_token(&s, "ToPdf");
  write_node(&s, &to_pdf);
  write_token(&s, "EndContextDependency");
  return s;
}

}  // namespace khg_tree

extern "C" int khg_build_tree(int32_t N, int32_t P, int32_t dim, int64_t num_keys, const int32_t* keys_h, const double* count_h, const double* x_h, const double* x2_h,
                              int32_t num_qkeys, const int32_t* qkey_h, const int64_t* qkey_off_h, const int64_t* q_off_h, const int32_t* q_vals_h, int32_t num_sets,
                              const int64_t* set_off_h, const int32_t* set_phones_h, const int32_t* share_roots_h, const int32_t* do_split_h, int32_t num_phones,
                              const int32_t* phone2num_pdf_classes_h, double thresh, int32_t max_leaves, double cluster_thresh, double var_floor, unsigned char* tree_h,
                              int64_t tree_cap, int64_t* tree_bytes, double* objf_impr, double* cluster_loss, int32_t* num_leaves, int32_t* num_removed) {
  const std::string who = "khg_build_tree: ";
  if (num_keys < 0 || (num_keys > 0 && (!keys_h || !count_h || !x_h || !x2_h)) || num_qkeys < 0 || (num_qkeys > 0 && (!qkey_h || !qkey_off_h || !q_off_h)) || num_sets < 1 ||
      !set_off_h || !set_phones_h || !share_roots_h || !do_split_h || num_phones < 0 || (num_phones > 0 && !phone2num_pdf_classes_h) || !tree_bytes || tree_cap < 0)
    return khg_set_error(KHG_E_ARG, who + "bad arguments");
  try {
    khg_tree::Stats st;
    st.N = N; st.P = P; st.dim = dim; st.num = num_keys; st.keys = keys_h; st.count = count_h; st.x = x_h; st.x2 = x2_h;
    khg_tree::Questions q;
    for (int32_t i = 0; i < num_qkeys; ++i) {
      q.keys.push_back(qkey_h[i]);
      q.sets.emplace_back();
      if (qkey_off_h[i] < 0 || qkey_off_h[i + 1] < qkey_off_h[i]) throw std::invalid_argument("question offsets must not descend");
      for (int64_t s = qkey_off_h[i]; s < qkey_off_h[i + 1]; ++s) {
        if (q_off_h[s] < 0 || q_off_h[s + 1] < q_off_h[s] || (q_off_h[s + 1] > q_off_h[s] && !q_vals_h)) throw std::invalid_argument("question offsets must not descend");
        q.sets.back().emplace_back(q_vals_h + q_off_h[s], q_vals_h + q_off_h[s + 1]);
      }
    }
    std::vector<std::vector<int32_t>> phone_sets;
    std::vector<bool> share, split;
    for (int32_t r = 0; r < num_sets; ++r) {
      if (set_off_h[r] < 0 || set_off_h[r + 1] < set_off_h[r]) throw std::invalid_argument("phone set offsets must not descend");
      phone_sets.emplace_back(set_phones_h + set_off_h[r], set_phones_h + set_off_h[r + 1]);
      share.push_back(share_roots_h[r] != 0); split.push_back(do_split_h[r] != 0);
    }
    std::vector<int32_t> p2n(phone2num_pdf_classes_h, phone2num_pdf_classes_h + num_phones);
    khg_tree::Result res = khg_tree::build_tree(st, q, phone_sets, p2n, share, split, thresh, max_leaves, cluster_thresh, var_floor);
    const std::string bytes = khg_tree::write_context_dependency(N, P, *res.tree);
    *tree_bytes = (int64_t)bytes.size();
    if (tree_h && tree_cap >= (int64_t)bytes.size()) memcpy(tree_h, bytes.data(), bytes.size());
    if (objf_impr) *objf_impr = res.objf_impr;
    if (cluster_loss) *cluster_loss = res.cluster_loss;
    if (num_leaves) *num_leaves = res.num_leaves;
    if (num_removed) *num_removed = res.num_removed;
  } catch (const std::invalid_argument& e) {
    return khg_set_error(KHG_E_ARG, who + e.what());
  } catch (const std::exception& e) {
    return khg_set_error(KHG_E_RUNTIME, who + e.what());
  }
  return KHG_OK;
}
