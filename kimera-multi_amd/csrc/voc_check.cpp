// voc_check.cpp — voc.hip's host code (voc_host.h: tree validation and the
// breadth-first renumbering) as a stand-alone program, built by `make
// voc_check` with the host address and undefined-behaviour sanitizers. It
// feeds kmx::voc_prepare the malformed trees kmx_voc_create must reject and
// random irregular trees, and checks the layout it returns. CPU only.
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "voc_host.h"

namespace {

int g_fail = 0;
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
      ++g_fail;                                                        \
    }                                                                  \
  } while (0)

struct Tree {
  std::vector<int32_t> parent, word_node;
  std::vector<uint8_t> desc;
  std::vector<double> weight;
};

int prepare(const Tree& t, int weighting, kmx::VocLayout* L, std::string* err, int n_nodes = -1) {
  // exact-size copies, so a read past either array is a sanitizer report
  std::vector<int32_t> parent(t.parent), words(t.word_node);
  std::vector<uint8_t> desc(t.desc);
  std::vector<double> weight(t.weight);
  return kmx::voc_prepare(n_nodes < 0 ? (int32_t)parent.size() : n_nodes, parent.data(), desc.data(), weight.data(),
                          (int32_t)words.size(), words.data(), weighting, L, err);
}

Tree make(std::vector<int32_t> parent, std::vector<int32_t> words) {
  Tree t;
  t.parent = std::move(parent);
  t.word_node = std::move(words);
  t.desc.resize(t.parent.size() * 32);
  for (size_t i = 0; i < t.desc.size(); ++i) t.desc[i] = (uint8_t)(i * 131 + 7);
  t.weight.resize(t.parent.size());
  for (size_t i = 0; i < t.weight.size(); ++i) t.weight[i] = 0.5 + (double)i;
  return t;
}

void expect_code(const Tree& t, int weighting, int code, const char* what, int n_nodes = -1) {
  kmx::VocLayout L;
  std::string err;
  const int rc = prepare(t, weighting, &L, &err, n_nodes);
  if (rc != code || (code != KMX_OK && err.find(what) == std::string::npos)) {
    std::fprintf(stderr, "expected %d (%s), got %d (%s)\n", code, what, rc, err.c_str());
    ++g_fail;
  }
}

// A random tree: node ids in creation order with shuffled extras, so ids are
// neither breadth first nor parent-before-child everywhere.
Tree random_tree(std::mt19937& rng, int k, int depth_max, double stop, bool shuffle) {
  std::vector<int32_t> parent{-1};
  std::vector<int> depth{0};
  std::vector<int32_t> frontier{0};
  while (!frontier.empty()) {
    const int32_t p = frontier.back();
    frontier.pop_back();
    if (depth[p] >= depth_max) continue;
    if (p != 0 && std::uniform_real_distribution<double>(0, 1)(rng) < stop) continue;
    const int c = 1 + (int)(rng() % (unsigned)k);
    for (int j = 0; j < c; ++j) {
      parent.push_back(p);
      depth.push_back(depth[p] + 1);
      frontier.push_back((int32_t)parent.size() - 1);
    }
  }
  const size_t n = parent.size();
  if (shuffle && n > 2) {  // relabel nodes 1..n-1 at random
    std::vector<int32_t> perm(n);
    std::iota(perm.begin(), perm.end(), 0);
    std::shuffle(perm.begin() + 1, perm.end(), rng);
    std::vector<int32_t> p2(n, -1);
    for (size_t i = 1; i < n; ++i) p2[perm[i]] = perm[parent[i]];
    parent = p2;
  }
  std::vector<int> cnt(n, 0);
  for (size_t i = 1; i < n; ++i) cnt[parent[i]]++;
  std::vector<int32_t> words;
  for (size_t i = 1; i < n; ++i)
    if (!cnt[i]) words.push_back((int32_t)i);
  return make(parent, words);
}

void check_layout(const Tree& t, const kmx::VocLayout& L) {
  const size_t n = t.parent.size();
  EXPECT((size_t)L.n_nodes == n && L.old_of_new.size() == n && L.desc.size() == n * 8);
  EXPECT(L.old_of_new[0] == 0);
  std::vector<int32_t> new_of_old(n, -1);
  for (size_t q = 0; q < n; ++q) {
    const int32_t o = L.old_of_new[q];
    EXPECT(o >= 0 && (size_t)o < n && new_of_old[o] < 0);  // a permutation
    if (o >= 0 && (size_t)o < n) new_of_old[o] = (int32_t)q;
  }
  size_t kids = 0;
  int32_t next_block = 1;
  for (size_t q = 0; q < n; ++q) {
    const int32_t f = L.child_first[q], c = L.child_count[q];
    EXPECT(c >= 0 && c <= L.max_children);
    if (c == 0) {
      EXPECT(L.word_of[q] >= 0 && L.word_of[q] < L.n_words);
      if (L.word_of[q] >= 0) EXPECT(t.word_node[L.word_of[q]] == L.old_of_new[q]);
      continue;
    }
    EXPECT(L.word_of[q] == -1);
    EXPECT(f == next_block && (size_t)f + c <= n);  // blocks tile [1, n) in breadth-first order
    next_block = f + c;
    for (int32_t j = 0; j < c && (size_t)f + j < n; ++j) {
      const int32_t o = L.old_of_new[f + j];
      EXPECT(t.parent[o] == L.old_of_new[q]);
      if (j) EXPECT(o > L.old_of_new[f + j - 1]);  // stored order = increasing DBoW2 id
      ++kids;
    }
  }
  EXPECT(kids == n - 1 && (size_t)next_block == n);
  for (size_t q = 0; q < n; ++q) {
    EXPECT(std::memcmp(&L.desc[q * 8], &t.desc[(size_t)L.old_of_new[q] * 32], 32) == 0);
    EXPECT(L.weight[q] == t.weight[L.old_of_new[q]]);
  }
  for (size_t w = 0; w < t.word_node.size(); ++w) EXPECT(L.word_weight[w] == t.weight[t.word_node[w]]);
}

}  // namespace

int main() {
  const std::vector<int32_t> good{-1, 0, 0, 0, 1, 1, 2};
  const std::vector<int32_t> words{3, 4, 5, 6};
  expect_code(make(good, words), 0, KMX_OK, "");
  expect_code(make({-1, 0, 0, 99, 1, 1, 2}, words), 0, KMX_EINVAL, "parent id out of range");
  expect_code(make({-1, 0, 0, -1, 1, 1, 2}, words), 0, KMX_EINVAL, "parent id out of range");
  expect_code(make({-1, 0, 0, 3, 1, 1, 2}, words), 0, KMX_EINVAL, "parent id out of range");
  expect_code(make({-1, 0, 0, 0, 5, 4, 2}, words), 0, KMX_EINVAL, "cycle");
  expect_code(make({-1, 2, 3, 1}, {1}), 0, KMX_EINVAL, "cycle");  // a cycle the root never reaches
  expect_code(make(good, {3, 4, 5, 2}), 0, KMX_EINVAL, "inner node");
  expect_code(make(good, {3, 4, 5}), 0, KMX_EINVAL, "no word");
  expect_code(make(good, {3, 4, 5, 5}), 0, KMX_EINVAL, "two words");
  expect_code(make(good, {3, 4, 5, 7}), 0, KMX_EINVAL, "out of range");
  expect_code(make(good, {3, 4, 5, -2}), 0, KMX_EINVAL, "out of range");
  expect_code(make({-1}, {0}), 0, KMX_EINVAL, "n_nodes >= 2");
  expect_code(make(good, words), 0, KMX_EINVAL, "n_nodes >= 2", 0);
  expect_code(make(good, words), 4, KMX_EUNSUP, "weighting");
  expect_code(make(good, words), -1, KMX_EUNSUP, "weighting");
  for (int len : {64, 65, 66, 200}) {  // chains: depth = len
    std::vector<int32_t> chain{-1};
    for (int i = 0; i < len; ++i) chain.push_back(i);
    expect_code(make(chain, {len}), 0, len <= kmx::VOC_MAX_DEPTH ? KMX_OK : KMX_EINVAL, "deeper than 64");
    std::vector<int32_t> rev(chain.size(), -1);  // the same chain with ids reversed: parents after children
    for (int i = 1; i <= len; ++i) rev[i] = i == len ? 0 : i + 1;
    expect_code(make(rev, {1}), 0, len <= kmx::VOC_MAX_DEPTH ? KMX_OK : KMX_EINVAL, "deeper than 64");
  }
  {
    kmx::VocLayout L;
    std::string err;
    EXPECT(kmx::voc_prepare(7, nullptr, nullptr, nullptr, 4, nullptr, 0, &L, &err) == KMX_EINVAL);
  }
  std::mt19937 rng(12345);
  int trees = 0;
  for (int rep = 0; rep < 300; ++rep) {
    const int k = 1 + rep % 17, depth = 1 + rep % 7;
    const Tree t = random_tree(rng, k, depth, 0.1 * (rep % 5), rep % 2 == 1);
    kmx::VocLayout L;
    std::string err;
    const int rc = prepare(t, rep % 4, &L, &err);
    if (rc != KMX_OK) {
      std::fprintf(stderr, "random tree %d rejected: %s\n", rep, err.c_str());
      ++g_fail;
      continue;
    }
    check_layout(t, L);
    ++trees;
  }
  if (g_fail) {
    std::fprintf(stderr, "voc_check: %d failure(s)\n", g_fail);
    return 1;
  }
  std::printf("voc_check ok: %d random trees, malformed trees rejected\n", trees);
  return 0;
}
