// dgraph_check.cpp — dgraph.hip's host code (dgraph_host.h: the node, edge,
// prior and parameter checks, the incidence CSR and the tiles, the union-find
// rule and the free-node map) as a stand-alone program, built by `make
// dgraph_check` with the host address and undefined-behaviour sanitizers. It
// feeds the checks malformed graphs, n = 0 and m = 0, a component without a
// prior and values that are not finite, and compares the CSR of a small graph
// with one written out by hand. CPU only.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "dgraph_host.h"

namespace {

int g_fail = 0;
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
      ++g_fail;                                                        \
    }                                                                  \
  } while (0)

struct Graph {
  std::vector<double> R, g, w;
  std::vector<int32_t> src, dst;
  int32_t n = 0;
  void nodes(int32_t k) {
    n = k;
    for (int32_t i = 0; i < k; ++i) {
      const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
      R.insert(R.end(), I, I + 9);
      g.insert(g.end(), {1.0 * i, 0.5 * i, -2.0 * i});
    }
  }
  void edge(int32_t a, int32_t b, double weight = 1.0) {
    src.push_back(a);
    dst.push_back(b);
    w.push_back(weight);
  }
  // exact-size arrays, so a read past one is a sanitizer report
  int build(kmx::DgGraph* out, std::string* err, bool weights = true) const {
    return kmx::dg_build(n, R.data(), g.data(), (int64_t)src.size(), src.data(), dst.data(),
                         weights ? w.data() : nullptr, out, err);
  }
};

struct Priors {
  std::vector<uint8_t> mode;
  std::vector<double> Rhat, that, kappa, tau;
  explicit Priors(int32_t n) : mode((size_t)n, 0), Rhat((size_t)n * 9, 0.0), that((size_t)n * 3, 0.0),
                               kappa((size_t)n, 0.0), tau((size_t)n, 0.0) {
    for (int32_t i = 0; i < n; ++i) Rhat[(size_t)i * 9] = Rhat[(size_t)i * 9 + 4] = Rhat[(size_t)i * 9 + 8] = 1.0;
  }
  int check(kmx::DgPriors* out, std::string* err) const {
    return kmx::dg_check_priors((int32_t)mode.size(), mode.data(), Rhat.data(), that.data(), kappa.data(), tau.data(),
                                out, err);
  }
};

void test_params() {
  std::string err;
  kmx::DgParams q;
  EXPECT(kmx::dg_check_params(nullptr, &q, &err) == KMX_OK);
  EXPECT(q.lambda_init == 1e-5 && q.factor == 10.0 && q.lambda_min == 1e-10 && q.lambda_max == 1e5);
  EXPECT(q.rel_tol == 1e-5 && q.abs_tol == 0.0 && q.cg_rtol == 1e-6);
  EXPECT(q.max_iterations == 100 && q.cg_max_iterations == 500 && q.check_every == 50);
  kmx_dgraph_params p{};
  p.rel_tol = -1.0;
  EXPECT(kmx::dg_check_params(&p, &q, &err) == KMX_OK && q.rel_tol == 1e-5 && q.cg_rtol == 1e-6);
  p.rel_tol = 0.0;
  p.cg_rtol = 1e-12;
  p.check_every = 7;
  EXPECT(kmx::dg_check_params(&p, &q, &err) == KMX_OK && q.rel_tol == 0.0 && q.cg_rtol == 1e-12 && q.check_every == 7);
  for (double bad : {std::nan(""), HUGE_VAL, -HUGE_VAL}) {
    kmx_dgraph_params b{};
    b.lambda_max = bad;
    EXPECT(kmx::dg_check_params(&b, &q, &err) == KMX_EINVAL);
    kmx_dgraph_params c{};
    c.abs_tol = bad;
    EXPECT(kmx::dg_check_params(&c, &q, &err) == KMX_EINVAL);
  }
  kmx_dgraph_params b{};
  b.lambda_factor = 1.0;
  EXPECT(kmx::dg_check_params(&b, &q, &err) == KMX_EINVAL);
  b = kmx_dgraph_params{};
  b.lambda_init = -1.0;
  EXPECT(kmx::dg_check_params(&b, &q, &err) == KMX_EINVAL);
  b = kmx_dgraph_params{};
  b.max_iterations = -1;
  EXPECT(kmx::dg_check_params(&b, &q, &err) == KMX_EINVAL);
  b = kmx_dgraph_params{};
  b.cg_max_iterations = std::numeric_limits<int32_t>::min();
  EXPECT(kmx::dg_check_params(&b, &q, &err) == KMX_EINVAL);
  b = kmx_dgraph_params{};
  b.lambda_min = 10.0;
  b.lambda_max = 1.0;
  EXPECT(kmx::dg_check_params(&b, &q, &err) == KMX_EINVAL);
  b = kmx_dgraph_params{};
  b.reserved = 1;
  EXPECT(kmx::dg_check_params(&b, &q, &err) == KMX_EUNSUP);
  EXPECT(q.check_every == 7);  // a rejected set changed nothing
}

void test_malformed_graphs() {
  std::string err;
  kmx::DgGraph G;
  G.n = -7;  // stays when a build fails
  Graph a;
  a.nodes(3);
  a.edge(0, 1);
  a.edge(1, 2);
  for (int32_t bad : {-1, 3, INT32_MAX, INT32_MIN}) {
    Graph b = a;
    b.src[1] = bad;
    EXPECT(b.build(&G, &err) == KMX_EINVAL);
    Graph c = a;
    c.dst[0] = bad;
    EXPECT(c.build(&G, &err) == KMX_EINVAL);
  }
  Graph loop = a;
  loop.edge(2, 2);
  EXPECT(loop.build(&G, &err) == KMX_EINVAL);
  for (double bad : {std::nan(""), HUGE_VAL, -HUGE_VAL, -1.0, -1e-300}) {
    Graph b = a;
    b.w[1] = bad;
    EXPECT(b.build(&G, &err) == KMX_EINVAL);
  }
  for (double bad : {std::nan(""), HUGE_VAL, -HUGE_VAL}) {
    Graph b = a;
    b.R[17] = bad;
    EXPECT(b.build(&G, &err) == KMX_EINVAL);
    Graph c = a;
    c.g[8] = bad;
    EXPECT(c.build(&G, &err) == KMX_EINVAL);
  }
  EXPECT(kmx::dg_build(-1, nullptr, nullptr, 0, nullptr, nullptr, nullptr, &G, &err) == KMX_EINVAL);
  EXPECT(kmx::dg_build(0, nullptr, nullptr, -1, nullptr, nullptr, nullptr, &G, &err) == KMX_EINVAL);
  EXPECT(kmx::dg_build(2, nullptr, a.g.data(), 0, nullptr, nullptr, nullptr, &G, &err) == KMX_EINVAL);
  EXPECT(kmx::dg_build(3, a.R.data(), a.g.data(), 2, nullptr, a.dst.data(), nullptr, &G, &err) == KMX_EINVAL);
  EXPECT(kmx::dg_build(3, a.R.data(), a.g.data(), (int64_t)1 << 40, a.src.data(), a.dst.data(), nullptr, &G, &err) ==
         KMX_EINVAL);
  EXPECT(G.n == -7);
  // zero weights are kept
  Graph z = a;
  z.w[0] = 0.0;
  EXPECT(z.build(&G, &err) == KMX_OK && G.m == 2 && G.w[0] == 0.0);
  // no weights: all 1
  EXPECT(a.build(&G, &err, false) == KMX_OK && G.w.size() == 2 && G.w[1] == 1.0);
}

void test_empty() {
  std::string err;
  kmx::DgGraph G;
  EXPECT(kmx::dg_build(0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, &G, &err) == KMX_OK);
  EXPECT(G.n == 0 && G.m == 0 && G.n_tiles == 0 && G.inc_ptr.size() == 1 && G.inc_ptr[0] == 0 && G.inc_other.empty());
  kmx::DgPriors P;
  EXPECT(kmx::dg_check_priors(0, nullptr, nullptr, nullptr, nullptr, nullptr, &P, &err) == KMX_OK);
  EXPECT(P.node_of.empty());
  EXPECT(kmx::dg_check_posed(0, 0, nullptr, nullptr, nullptr, P, &err) == KMX_OK);
  std::vector<double> rw;
  kmx::dg_record_weights(G, nullptr, &rw);
  EXPECT(rw.empty());
  // nodes without edges: every node is its own component
  Graph a;
  a.nodes(2);
  EXPECT(a.build(&G, &err) == KMX_OK && G.m == 0 && G.n_tiles == 1 && G.inc_ptr.size() == 3 && G.inc_ptr[2] == 0);
  Priors pr(2);
  pr.mode[0] = 2;
  EXPECT(pr.check(&P, &err) == KMX_OK);
  EXPECT(kmx::dg_check_posed(2, 0, nullptr, nullptr, nullptr, P, &err) == KMX_EINVAL);  // node 1 floats
  pr.mode[1] = 1;
  pr.tau[1] = 0.5;
  EXPECT(pr.check(&P, &err) == KMX_OK);
  EXPECT(kmx::dg_check_posed(2, 0, nullptr, nullptr, nullptr, P, &err) == KMX_OK);
  // tiles
  EXPECT(kmx::dg_tiles(0) == 0 && kmx::dg_tiles(1) == 1 && kmx::dg_tiles(64) == 1 && kmx::dg_tiles(65) == 2 &&
         kmx::dg_tiles(INT32_MAX) == 33554432);
}

void test_hand_csr() {
  // 0 -> 1, 2 -> 0, 1 -> 2, 0 -> 3, 3 -> 0 with weights 1 .. 5; node 4 has no edge
  Graph a;
  a.nodes(5);
  a.edge(0, 1, 1.0);
  a.edge(2, 0, 2.0);
  a.edge(1, 2, 3.0);
  a.edge(0, 3, 4.0);
  a.edge(3, 0, 5.0);
  kmx::DgGraph G;
  std::string err;
  EXPECT(a.build(&G, &err) == KMX_OK);
  const uint32_t T = kmx::GRAPH_TAIL;
  const int32_t ptr[6] = {0, 4, 6, 8, 10, 10};
  const uint32_t other[10] = {1 | T, 2, 3 | T, 3, 0, 2 | T, 0 | T, 1, 0, 0 | T};
  const int32_t edge[10] = {0, 1, 3, 4, 0, 2, 1, 2, 3, 4};
  EXPECT(G.inc_ptr.size() == 6 && G.inc_other.size() == 10 && G.inc_edge.size() == 10);
  for (int k = 0; k < 6; ++k) EXPECT(G.inc_ptr[k] == ptr[k]);
  for (int k = 0; k < 10; ++k) EXPECT(G.inc_other[k] == other[k] && G.inc_edge[k] == edge[k]);
  std::vector<double> rw;
  kmx::dg_record_weights(G, G.w.data(), &rw);
  for (int k = 0; k < 10; ++k) EXPECT(rw[k] == 1.0 + edge[k]);
  kmx::dg_record_weights(G, nullptr, &rw);
  for (int k = 0; k < 10; ++k) EXPECT(rw[k] == 1.0);
}

void test_priors_and_components() {
  std::string err;
  // two components {0, 1, 2} and {3, 4}, joined only by an edge of weight 0
  Graph a;
  a.nodes(5);
  a.edge(0, 1);
  a.edge(1, 2);
  a.edge(3, 4);
  a.edge(2, 3, 0.0);
  kmx::DgGraph G;
  EXPECT(a.build(&G, &err) == KMX_OK);
  auto posed = [&](const kmx::DgPriors& P, const double* w) {
    return kmx::dg_check_posed(G.n, G.m, G.src.data(), G.dst.data(), w, P, &err);
  };
  kmx::DgPriors P;
  Priors none(5);
  EXPECT(none.check(&P, &err) == KMX_OK && P.node_of.size() == 5);
  EXPECT(posed(P, G.w.data()) == KMX_EINVAL);
  Priors one(5);
  one.mode[1] = 1;
  one.tau[1] = 2.0;
  EXPECT(one.check(&P, &err) == KMX_OK);
  EXPECT(posed(P, G.w.data()) == KMX_EINVAL);  // {3, 4} holds nothing
  EXPECT(posed(P, nullptr) == KMX_OK);         // all weights 1: one component
  Priors kap(5);  // kappa alone does not hold a component
  kap.mode[1] = 1;
  kap.tau[1] = 2.0;
  kap.mode[4] = 1;
  kap.kappa[4] = 3.0;
  EXPECT(kap.check(&P, &err) == KMX_OK);
  EXPECT(posed(P, G.w.data()) == KMX_EINVAL);
  kap.mode[3] = 2;
  EXPECT(kap.check(&P, &err) == KMX_OK);
  EXPECT(posed(P, G.w.data()) == KMX_OK);
  // the free-node map skips the hard node
  EXPECT(P.node_of.size() == 4 && P.free_of[3] == -1 && P.free_of[4] == 3 && P.node_of[3] == 4 && P.free_of[0] == 0);
  EXPECT(P.kappa[4] == 3.0 && P.tau[1] == 2.0 && P.kappa[3] == 0.0);
  // rows of nodes with mode 0 are not read
  Priors skip(5);
  skip.mode[0] = 2;
  skip.mode[3] = 2;
  skip.Rhat[9 * 2 + 1] = std::nan("");
  skip.that[3 * 1] = HUGE_VAL;
  skip.kappa[4] = -1.0;
  EXPECT(skip.check(&P, &err) == KMX_OK && P.Rhat[9 * 2 + 1] == 0.0 && P.Rhat[9 * 2] == 1.0);
  // bad values
  P.node_of.assign(77, 0);
  for (double bad : {std::nan(""), HUGE_VAL, -HUGE_VAL}) {
    Priors b(5);
    b.mode[2] = 2;
    b.Rhat[9 * 2 + 5] = bad;
    EXPECT(b.check(&P, &err) == KMX_EINVAL);
    Priors c(5);
    c.mode[2] = 1;
    c.that[3 * 2 + 2] = bad;
    EXPECT(c.check(&P, &err) == KMX_EINVAL);
    Priors d(5);
    d.mode[2] = 1;
    d.kappa[2] = bad;
    EXPECT(d.check(&P, &err) == KMX_EINVAL);
    Priors e(5);
    e.mode[2] = 1;
    e.tau[2] = bad;
    EXPECT(e.check(&P, &err) == KMX_EINVAL);
  }
  Priors neg(5);
  neg.mode[0] = 1;
  neg.tau[0] = -1e-9;
  EXPECT(neg.check(&P, &err) == KMX_EINVAL);
  Priors mode(5);
  mode.mode[4] = 3;
  EXPECT(mode.check(&P, &err) == KMX_EINVAL);
  EXPECT(kmx::dg_check_priors(5, nullptr, none.Rhat.data(), none.that.data(), none.kappa.data(), none.tau.data(), &P,
                              &err) == KMX_EINVAL);
  EXPECT(P.node_of.size() == 77);  // a rejected set changed nothing
  // weights for set_weights
  std::vector<double> w{1.0, 0.0, 2.0, 0.0};
  EXPECT(kmx::dg_check_weights(4, w.data(), &err) == KMX_OK);
  EXPECT(kmx::dg_check_weights(4, nullptr, &err) == KMX_OK);
  w[3] = -0.5;
  EXPECT(kmx::dg_check_weights(4, w.data(), &err) == KMX_EINVAL);
  w[3] = std::nan("");
  EXPECT(kmx::dg_check_weights(4, w.data(), &err) == KMX_EINVAL);
}

// a long chain, joined back to front: the union-find's path halving
void test_long_chain() {
  std::string err;
  const int32_t n = 5000;
  Graph a;
  a.nodes(n);
  for (int32_t i = n - 1; i > 0; --i) a.edge(i, i - 1);
  kmx::DgGraph G;
  EXPECT(a.build(&G, &err) == KMX_OK && G.n_tiles == 79);
  Priors pr(n);
  pr.mode[n - 1] = 1;
  pr.tau[n - 1] = 1.0;
  kmx::DgPriors P;
  EXPECT(pr.check(&P, &err) == KMX_OK);
  EXPECT(kmx::dg_check_posed(n, G.m, G.src.data(), G.dst.data(), G.w.data(), P, &err) == KMX_OK);
  G.w[2500] = 0.0;  // cut: the half without the prior floats
  EXPECT(kmx::dg_check_posed(n, G.m, G.src.data(), G.dst.data(), G.w.data(), P, &err) == KMX_EINVAL);
}

}  // namespace

int main() {
  test_params();
  test_malformed_graphs();
  test_empty();
  test_hand_csr();
  test_priors_and_components();
  test_long_chain();
  if (g_fail) {
    std::fprintf(stderr, "dgraph_check: %d failures\n", g_fail);
    return 1;
  }
  std::printf("dgraph_check ok\n");
  return 0;
}
