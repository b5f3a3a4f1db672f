// voc_host.h — host side of the DBoW2 vocabulary tree (voc.hip): validation of
// a tree given in DBoW2's node ids and its renumbering into the device layout.
// Plain C++ with no HIP call, so kmx_voc_create can reject a malformed tree
// before it touches a device, and voc_check.cpp can run the same code under
// the host sanitizers.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "kmx_abi.h"

namespace kmx {

constexpr int VOC_MAX_DEPTH = 64;

// The tree in breadth-first order: node 0 is the root and every node's
// children are one contiguous block [child_first, child_first + child_count)
// in their original (increasing DBoW2 node id = load) order. Levels are
// contiguous too, so the nodes [0, m) are the top of the tree for every m.
struct VocLayout {
  int32_t n_nodes = 0, n_words = 0, max_children = 0, max_depth = 0;
  std::vector<int32_t> old_of_new;   // [n_nodes] DBoW2 node id of device node i
  std::vector<int32_t> child_first;  // [n_nodes]
  std::vector<int32_t> child_count;  // [n_nodes] 0 = leaf
  std::vector<int32_t> word_of;      // [n_nodes] word id of a leaf, -1 for an inner node
  std::vector<uint32_t> desc;        // [n_nodes][8] descriptors, device order
  std::vector<double> weight;        // [n_nodes] node weights, device order
  std::vector<double> word_weight;   // [n_words] weight of the word's leaf
};

// Returns KMX_OK, KMX_EINVAL (malformed tree) or KMX_EUNSUP (weighting) and a
// message in *err. parent[0] (the root's) is not read.
inline int voc_prepare(int32_t n_nodes, const int32_t* parent, const uint8_t* descriptor, const double* weight,
                       int32_t n_words, const int32_t* word_node, int weighting, VocLayout* out, std::string* err) {
  auto bad = [&](int code, const char* msg) {
    if (err) *err = msg;
    return code;
  };
  if (!parent || !descriptor || !weight || !word_node || !out) return bad(KMX_EINVAL, "null argument");
  if (n_nodes < 2) return bad(KMX_EINVAL, "a vocabulary has a root and at least one word (n_nodes >= 2)");
  if (n_words < 1 || n_words >= n_nodes) return bad(KMX_EINVAL, "n_words must be in [1, n_nodes)");
  if (weighting < 0 || weighting > 3)
    return bad(KMX_EUNSUP, "weighting: 0 TF_IDF, 1 TF, 2 IDF and 3 BINARY are built");
  const size_t n = (size_t)n_nodes;
  for (size_t i = 1; i < n; ++i)
    if (parent[i] < 0 || parent[i] >= n_nodes || (size_t)parent[i] == i)
      return bad(KMX_EINVAL, "parent id out of range");
  // depth of every node: walk up to a node of known depth, at most VOC_MAX_DEPTH steps
  std::vector<int32_t> depth(n, -1);
  depth[0] = 0;
  int32_t max_depth = 0;
  int32_t path[VOC_MAX_DEPTH + 1];
  for (size_t i = 1; i < n; ++i) {
    int32_t len = 0, a = (int32_t)i;
    while (depth[a] < 0) {
      if (len >= VOC_MAX_DEPTH) return bad(KMX_EINVAL, "cycle in the parent links, or a tree deeper than 64");
      path[len++] = a;
      a = parent[a];
    }
    int32_t d = depth[a];
    while (len > 0) depth[path[--len]] = ++d;
    if (depth[i] > VOC_MAX_DEPTH) return bad(KMX_EINVAL, "cycle in the parent links, or a tree deeper than 64");
    if (depth[i] > max_depth) max_depth = depth[i];
  }
  // children of every node in increasing node id (a counting sort by parent)
  std::vector<int32_t> cnt(n, 0), first(n + 1, 0), kids(n - 1);
  for (size_t i = 1; i < n; ++i) cnt[parent[i]]++;
  for (size_t i = 0; i < n; ++i) first[i + 1] = first[i] + cnt[i];
  {
    std::vector<int32_t> fill(first.begin(), first.end() - 1);
    for (size_t i = 1; i < n; ++i) kids[fill[parent[i]]++] = (int32_t)i;
  }
  // words: each maps to a leaf, each leaf is exactly one word
  std::vector<int32_t> word_old(n, -1);
  for (int32_t w = 0; w < n_words; ++w) {
    const int32_t nd = word_node[w];
    if (nd < 1 || nd >= n_nodes) return bad(KMX_EINVAL, "word maps to a node id out of range");
    if (cnt[nd] != 0) return bad(KMX_EINVAL, "word maps to an inner node");
    if (word_old[nd] >= 0) return bad(KMX_EINVAL, "a leaf is two words");
    word_old[nd] = w;
  }
  for (size_t i = 1; i < n; ++i)
    if (cnt[i] == 0 && word_old[i] < 0) return bad(KMX_EINVAL, "a leaf is no word");
  // breadth-first renumbering
  VocLayout& L = *out;
  L = VocLayout();
  L.n_nodes = n_nodes;
  L.n_words = n_words;
  L.max_depth = max_depth;
  L.old_of_new.assign(n, 0);
  L.child_first.assign(n, 0);
  L.child_count.assign(n, 0);
  L.word_of.assign(n, -1);
  size_t tail = 1;  // old_of_new[0] = 0, the root
  for (size_t q = 0; q < n; ++q) {
    if (q >= tail) return bad(KMX_EINVAL, "a node is not reachable from the root");
    const int32_t o = L.old_of_new[q];
    L.child_first[q] = cnt[o] ? (int32_t)tail : 0;
    L.child_count[q] = cnt[o];
    L.word_of[q] = word_old[o];
    if (cnt[o] > L.max_children) L.max_children = cnt[o];
    for (int32_t k = 0; k < cnt[o]; ++k) L.old_of_new[tail++] = kids[first[o] + k];
  }
  L.desc.assign(n * 8, 0u);
  L.weight.assign(n, 0.0);
  for (size_t q = 0; q < n; ++q) {
    std::memcpy(&L.desc[q * 8], descriptor + (size_t)L.old_of_new[q] * 32, 32);
    L.weight[q] = weight[L.old_of_new[q]];
  }
  L.word_weight.assign((size_t)n_words, 0.0);
  for (int32_t w = 0; w < n_words; ++w) L.word_weight[w] = weight[word_node[w]];
  return KMX_OK;
}

}  // namespace kmx
