// kaldi_hmm_gmm_amd/csrc/khg_host_tree.hpp -- Kaldi's BuildTree on host statistics: GetStubMap, SplitDecisionTree,
// ClusterEventMapRestrictedByMap, RenumberEventMap, and the binary ContextDependency stream.  Plain C++17, no device.
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

namespace khg_tree {

// an EventMap node: CE (leaf), TE (table over a key) or SE (split on a key by a set)
struct Node {
  enum Kind { CE, TE, SE } kind = CE;
  int32_t answer = -1;                         // CE
  int32_t key = 0;                             // TE / SE
  std::vector<std::unique_ptr<Node>> table;    // TE (null entries allowed)
  std::vector<int32_t> yes_set;                // SE, sorted
  std::unique_ptr<Node> yes, no;               // SE
};

struct Stats {                                 // one row per distinct event, as khg_tree_stats_download lays them out
  int32_t N = 1, P = 0, dim = 0;
  int64_t num = 0;
  const int32_t* keys = nullptr;               // [num][N + 1]: window, then pdf-class
  const double *count = nullptr, *x = nullptr, *x2 = nullptr;
};
struct Questions {                             // per question key (-1 = pdf-class, 0 .. N - 1), ascending: its sets in the caller's order
  std::vector<int32_t> keys;
  std::vector<std::vector<std::vector<int32_t>>> sets;
};
struct Result {
  std::unique_ptr<Node> tree;
  double objf_impr = 0.0, cluster_loss = 0.0;
  int32_t num_leaves = 0, num_removed = 0;
};

// throws std::invalid_argument with a message for malformed input
std::unique_ptr<Node> get_stub_map(int32_t P, const std::vector<std::vector<int32_t>>& phone_sets, const std::vector<int32_t>& phone2num_pdf_classes,
                                   const std::vector<bool>& share_roots, int32_t* num_leaves);
Result build_tree(const Stats& st, const Questions& q, const std::vector<std::vector<int32_t>>& phone_sets, const std::vector<int32_t>& phone2num_pdf_classes,
                  const std::vector<bool>& share_roots, const std::vector<bool>& do_split, double thresh, int32_t max_leaves, double cluster_thresh,
                  double var_floor);
// "ContextDependency N P ToPdf <map> EndContextDependency" in Kaldi's binary form (without the "\0B" file header)
std::string write_context_dependency(int32_t N, int32_t P, const Node& to_pdf);

}  // namespace khg_tree
