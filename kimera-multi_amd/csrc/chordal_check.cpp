// chordal_check.cpp — chordal.hip's host code (chordal_host.h: the checks of
// kmx_chordal_set_graph / kmx_chordal_set_weights and the incidence CSR and
// tile list they build, and the parameter and fixed-mask checks of
// kmx_chordal_solve_robust) as a stand-alone program, built by `make chordal_check`
// with the host address and undefined-behaviour sanitizers. Every array is
// passed in a vector of exactly the stated size, so a read past one is a
// report. CPU only.
#include <cstdio>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "chordal_host.h"

namespace {

int g_fail = 0;

struct Graph {
  int32_t n = 0;
  std::vector<int32_t> block_ptr, src, dst, anchors;
  std::vector<double> R, t, kappa, tau, weight;
  bool with_weight = true;

  void edge(int32_t i, int32_t j, double k = 2.0, double ta = 3.0, double w = 1.0) {
    src.push_back(i);
    dst.push_back(j);
    const double c = std::cos(0.1 * (double)src.size()), s = std::sin(0.1 * (double)src.size());
    const double Re[9] = {c, -s, 0, s, c, 0, 0, 0, 1};
    R.insert(R.end(), Re, Re + 9);
    for (int q = 0; q < 3; ++q) t.push_back(0.5 * q + (double)src.size());
    kappa.push_back(k);
    tau.push_back(ta);
    weight.push_back(w);
  }
  int build(kmx::ChordalGraph* out, std::string* err) const {
    // exact-size copies
    std::vector<int32_t> bp(block_ptr), s(src), d(dst), a(anchors);
    std::vector<double> r(R), tt(t), k(kappa), ta(tau), w(weight);
    return kmx::chordal_build(n, (int32_t)bp.size() - 1, bp.data(), (int64_t)s.size(), s.empty() ? nullptr : s.data(),
                              d.empty() ? nullptr : d.data(), r.empty() ? nullptr : r.data(),
                              tt.empty() ? nullptr : tt.data(), k.empty() ? nullptr : k.data(),
                              ta.empty() ? nullptr : ta.data(), with_weight && !w.empty() ? w.data() : nullptr,
                              (int32_t)a.size(), a.empty() ? nullptr : a.data(), out, err);
  }
};

void expect(const Graph& g, int code, const char* what, const char* name) {
  kmx::ChordalGraph out;
  out.n = -7;  // a failed build must leave *out alone
  std::string err;
  const int rc = g.build(&out, &err);
  if (rc != code || (code != KMX_OK && err.find(what) == std::string::npos) || (code != KMX_OK && out.n != -7)) {
    std::fprintf(stderr, "%s: expected %d (%s), got %d (%s)\n", name, code, what, rc, err.c_str());
    ++g_fail;
  }
}

Graph chain(int32_t n) {
  Graph g;
  g.n = n;
  g.block_ptr = {0, n};
  g.anchors = {0};
  for (int32_t p = 0; p + 1 < n; ++p) g.edge(p, p + 1);
  return g;
}

// The CSR against the edge list: every edge appears once at each end, in edge
// order within a pose, with the rotation transposed at the source; the tiles
// partition every block in order and never span two.
void check_csr(const Graph& g, const kmx::ChordalGraph& c, const char* name) {
  auto fail = [&](const char* m) {
    std::fprintf(stderr, "%s: CSR: %s\n", name, m);
    ++g_fail;
  };
  const size_t m = g.src.size();
  if (c.inc_ptr.size() != (size_t)g.n + 1 || c.inc_ptr[0] != 0 || (size_t)c.inc_ptr[g.n] != 2 * m) return fail("inc_ptr");
  if (c.inc_other.size() != 2 * m || c.inc_edge.size() != 2 * m || c.inc_M.size() != 18 * m || c.inc_t.size() != 6 * m)
    return fail("sizes");
  std::vector<int> seen_src(m, 0), seen_dst(m, 0);
  for (int32_t p = 0; p < g.n; ++p) {
    if (c.inc_ptr[p + 1] < c.inc_ptr[p]) return fail("inc_ptr not monotone");
    for (int32_t k = c.inc_ptr[p]; k < c.inc_ptr[p + 1]; ++k) {
      const int32_t e = c.inc_edge[k];
      if (e < 0 || (size_t)e >= m) return fail("edge index");
      if (k > c.inc_ptr[p] && c.inc_edge[k - 1] > e) return fail("records of a pose not in edge order");
      const bool out = (c.inc_other[k] & kmx::CH_DIR_OUT) != 0;
      const int32_t o = (int32_t)(c.inc_other[k] & 0x7fffffffu);
      if (out ? (g.src[e] != p || g.dst[e] != o) : (g.dst[e] != p || g.src[e] != o)) return fail("endpoints");
      (out ? seen_src : seen_dst)[e]++;
      for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 3; ++q)
          if (c.inc_M[9 * (size_t)k + 3 * r + q] != (out ? g.R[9 * (size_t)e + 3 * q + r] : g.R[9 * (size_t)e + 3 * r + q]))
            return fail("rotation");
      for (int q = 0; q < 3; ++q)
        if (c.inc_t[3 * (size_t)k + q] != g.t[3 * (size_t)e + q]) return fail("translation");
    }
  }
  for (size_t e = 0; e < m; ++e)
    if (seen_src[e] != 1 || seen_dst[e] != 1) return fail("an edge is not recorded once at each end");
  const int32_t nb = (int32_t)g.block_ptr.size() - 1;
  if (c.tile_ptr.size() != (size_t)nb + 1 || c.tile_ptr[0] != 0) return fail("tile_ptr");
  for (int32_t b = 0; b < nb; ++b) {
    int32_t at = g.block_ptr[b];
    for (int32_t tI = c.tile_ptr[b]; tI < c.tile_ptr[b + 1]; ++tI) {
      if (c.tile_block[tI] != b || c.tile_p0[tI] != at || c.tile_p1[tI] <= at || c.tile_p1[tI] - at > kmx::CH_TILE ||
          c.tile_p1[tI] > g.block_ptr[b + 1])
        return fail("tile");
      at = c.tile_p1[tI];
    }
    if (at != g.block_ptr[b + 1]) return fail("tiles do not cover the block");
  }
  if ((size_t)c.tile_ptr[nb] != c.tile_p0.size()) return fail("tile count");
  std::vector<double> wk, wt;
  kmx::chordal_record_weights(c, g.with_weight ? g.weight.data() : nullptr, &wk, &wt);
  for (size_t k = 0; k < 2 * m; ++k) {
    const int32_t e = c.inc_edge[k];
    const double w = g.with_weight ? g.weight[e] : 1.0;
    if (wk[k] != w * g.kappa[e] || wt[k] != w * g.tau[e]) return fail("record weights");
  }
}

void expect_ok_csr(const Graph& g, const char* name) {
  kmx::ChordalGraph out;
  std::string err;
  const int rc = g.build(&out, &err);
  if (rc != KMX_OK) {
    std::fprintf(stderr, "%s: expected ok, got %d (%s)\n", name, rc, err.c_str());
    ++g_fail;
    return;
  }
  check_csr(g, out, name);
}

}  // namespace

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  int refused = 0;
#define REFUSE(g, what)                    \
  do {                                     \
    expect(g, KMX_EINVAL, what, #what);    \
    ++refused;                             \
  } while (0)
  // legal graphs
  expect_ok_csr(chain(2), "two poses");
  expect_ok_csr(chain(65), "chain of 65");
  expect_ok_csr(chain(200), "chain of 200");
  {
    Graph g = chain(2);  // parallel (duplicate) edges
    g.edge(0, 1, 4.0);
    g.edge(0, 1, 3.0);
    g.edge(1, 0, 2.0);
    expect_ok_csr(g, "parallel edges");
  }
  {
    Graph g = chain(5);  // empty blocks: in front, in the middle, at the end
    g.block_ptr = {0, 0, 5, 5, 5};
    expect_ok_csr(g, "empty blocks");
  }
  {
    Graph g;  // no edge, every pose an anchor
    g.n = 4;
    g.block_ptr = {0, 2, 4};
    g.anchors = {3, 1, 0, 2};
    expect_ok_csr(g, "no edges, all anchors");
  }
  {
    Graph g = chain(4);  // weight NULL
    g.with_weight = false;
    expect_ok_csr(g, "null weight");
  }
  {
    Graph g = chain(4);  // a zero-weight loop closure is legal when the rest connects
    g.edge(0, 3, 2.0, 3.0, 0.0);
    expect_ok_csr(g, "zero-weight loop closure");
  }
  // refusals
  { Graph g = chain(4); g.src[1] = 4; REFUSE(g, "endpoint out of range"); }
  { Graph g = chain(4); g.dst[2] = -1; REFUSE(g, "endpoint out of range"); }
  { Graph g = chain(4); g.dst[0] = 0; REFUSE(g, "to itself"); }
  { Graph g = chain(4); g.block_ptr = {0, 2, 4}; g.anchors = {0, 2}; REFUSE(g, "across blocks"); }
  { Graph g = chain(4); g.R[13] = nan; REFUSE(g, "R not finite"); }
  { Graph g = chain(4); g.t[4] = nan; REFUSE(g, "t not finite"); }
  { Graph g = chain(4); g.t[0] = inf; REFUSE(g, "t not finite"); }
  { Graph g = chain(4); g.kappa[1] = 0.0; REFUSE(g, "kappa must be"); }
  { Graph g = chain(4); g.kappa[1] = nan; REFUSE(g, "kappa must be"); }
  { Graph g = chain(4); g.tau[2] = -1.0; REFUSE(g, "tau must be"); }
  { Graph g = chain(4); g.tau[2] = inf; REFUSE(g, "tau must be"); }
  { Graph g = chain(4); g.weight[0] = -0.5; REFUSE(g, "weight must be"); }
  { Graph g = chain(4); g.weight[0] = nan; REFUSE(g, "weight must be"); }
  { Graph g = chain(4); g.block_ptr = {0, 3, 2, 4}; REFUSE(g, "block_ptr not monotone"); }
  { Graph g = chain(4); g.block_ptr = {1, 4}; REFUSE(g, "must start at 0"); }
  { Graph g = chain(4); g.block_ptr = {0, 3}; REFUSE(g, "must cover"); }
  { Graph g = chain(4); g.block_ptr = {0, 5}; REFUSE(g, "block_ptr not monotone"); }
  { Graph g = chain(4); g.anchors = {4}; REFUSE(g, "anchor out of range"); }
  { Graph g = chain(4); g.anchors = {-1}; REFUSE(g, "anchor out of range"); }
  { Graph g = chain(4); g.anchors = {1, 1}; REFUSE(g, "anchor listed twice"); }
  { Graph g = chain(4); g.anchors = {}; REFUSE(g, "not connected to an anchor"); }
  { Graph g = chain(4); g.n = 0; g.block_ptr = {0, 0}; REFUSE(g, "bad argument"); }
  {
    Graph g = chain(6);  // two blocks, the second without an anchor
    g.src.erase(g.src.begin() + 2);
    g.dst.erase(g.dst.begin() + 2);
    g.R.erase(g.R.begin() + 18, g.R.begin() + 27);
    g.t.erase(g.t.begin() + 6, g.t.begin() + 9);
    g.kappa.pop_back();
    g.tau.pop_back();
    g.weight.pop_back();
    g.block_ptr = {0, 3, 6};
    REFUSE(g, "not connected to an anchor");
    g.anchors = {0, 4};
    expect_ok_csr(g, "two anchored blocks");
  }
  {
    Graph g = chain(4);  // the only edge to pose 3 has weight 0: an anchor-less component
    g.weight[2] = 0.0;
    REFUSE(g, "pose 3 is not connected");
  }
  {
    Graph g = chain(3);  // a free pose without any edge
    g.n = 4;
    g.block_ptr = {0, 4};
    REFUSE(g, "pose 3 is not connected");
  }
  // set_weights' check on a built graph
  {
    Graph g = chain(5);
    g.edge(0, 4);
    kmx::ChordalGraph c;
    std::string err;
    if (g.build(&c, &err) != KMX_OK) ++g_fail;
    std::vector<double> w(g.src.size(), 1.0);
    w[1] = 0.0;  // the loop closure keeps everything connected
    if (kmx::chordal_check_weights(c.n, c.m, c.src.data(), c.dst.data(), w.data(), c.is_free.data(), &err) != KMX_OK) {
      std::fprintf(stderr, "set_weights: connected weights refused (%s)\n", err.c_str());
      ++g_fail;
    }
    w[2] = 0.0;  // pose 2 is cut off
    if (kmx::chordal_check_weights(c.n, c.m, c.src.data(), c.dst.data(), w.data(), c.is_free.data(), &err) != KMX_EINVAL ||
        err.find("pose 2") == std::string::npos) {
      std::fprintf(stderr, "set_weights: disconnecting weights accepted (%s)\n", err.c_str());
      ++g_fail;
    }
  }
  // the robust solve's checks: its parameters, and the fixed mask, whose edges
  // of weight > 0 must connect every free pose to an anchor by themselves
  int robust = 0;
  {
    auto params = [&](kmx_chordal_robust_params rp, int code, const char* what, const char* name) {
      kmx::ChordalRobust q;
      q.max_updates = -7;  // a refusal must leave *out alone
      std::string err;
      const int rc = kmx::chordal_robust_params(&rp, &q, &err);
      if (rc != code || (code != KMX_OK && (err.find(what) == std::string::npos || q.max_updates != -7))) {
        std::fprintf(stderr, "robust params %s: expected %d (%s), got %d (%s)\n", name, code, what, rc, err.c_str());
        ++g_fail;
      }
      ++robust;
    };
    const kmx_chordal_robust_params zero = {0.0, 0.0, 0.0, 0, 0};
    params(zero, KMX_OK, "", "all defaults");
    kmx::ChordalRobust q;
    std::string err;
    if (kmx::chordal_robust_params(nullptr, &q, &err) != KMX_OK || q.barc != 5.0 || q.mu_init != 0.0 ||
        q.mu_step != 1.4 || q.max_updates != 100 || q.start_projected) {
      std::fprintf(stderr, "robust params: wrong defaults\n");
      ++g_fail;
    }
    { auto rp = zero; rp.barc = 3.0; rp.mu_init = 1e-5; rp.mu_step = 1.0000001; rp.max_updates = 7; rp.reserved = 1; params(rp, KMX_OK, "", "all given"); }
    { auto rp = zero; rp.barc = nan; params(rp, KMX_EINVAL, "barc", "NaN barc"); }
    { auto rp = zero; rp.barc = -1.0; params(rp, KMX_EINVAL, "barc", "negative barc"); }
    { auto rp = zero; rp.barc = inf; params(rp, KMX_EINVAL, "barc", "infinite barc"); }
    { auto rp = zero; rp.mu_init = nan; params(rp, KMX_EINVAL, "mu_init", "NaN mu_init"); }
    { auto rp = zero; rp.mu_init = -1e-5; params(rp, KMX_EINVAL, "mu_init", "negative mu_init"); }
    { auto rp = zero; rp.mu_step = 1.0; params(rp, KMX_EINVAL, "mu_step must be > 1", "mu_step = 1"); }
    { auto rp = zero; rp.mu_step = 0.5; params(rp, KMX_EINVAL, "mu_step must be > 1", "mu_step < 1"); }
    { auto rp = zero; rp.mu_step = nan; params(rp, KMX_EINVAL, "mu_step", "NaN mu_step"); }
    { auto rp = zero; rp.mu_step = -2.0; params(rp, KMX_EINVAL, "mu_step", "negative mu_step"); }
    { auto rp = zero; rp.max_updates = -1; params(rp, KMX_EINVAL, "max_updates", "negative max_updates"); }
    { auto rp = zero; rp.reserved = 2; params(rp, KMX_EINVAL, "reserved", "reserved = 2"); }
  }
  {
    Graph g = chain(6);  // edges 0..4: the chain; 5, 6: loop closures; 7: a second 2 -> 3
    g.edge(0, 5);
    g.edge(1, 4);
    g.edge(2, 3);
    kmx::ChordalGraph c;
    std::string err;
    if (g.build(&c, &err) != KMX_OK) ++g_fail;
    auto mask = [&](std::vector<uint8_t> fx, bool null, int code, const char* what, const char* name) {
      std::string e2;
      const int rc = kmx::chordal_check_fixed(c, null ? nullptr : fx.data(), &e2);
      if (rc != code || (code != KMX_OK && e2.find(what) == std::string::npos)) {
        std::fprintf(stderr, "fixed mask %s: expected %d (%s), got %d (%s)\n", name, code, what, rc, e2.c_str());
        ++g_fail;
      }
      ++robust;
    };
    mask({1, 1, 1, 1, 1, 0, 0, 0}, false, KMX_OK, "", "the chain");
    mask({1, 1, 0, 1, 1, 0, 0, 1}, false, KMX_OK, "", "the chain through the parallel edge");
    mask({1, 1, 0, 1, 1, 0, 0, 0}, false, KMX_EINVAL, "pose 3 is not connected", "a mask that disconnects a pose");
    mask({0, 0, 0, 0, 0, 0, 0, 0}, false, KMX_EINVAL, "pose 1 is not connected", "a mask of zeros");
    mask({}, true, KMX_EINVAL, "pose 1 is not connected", "a null mask");
    mask({0, 1, 1, 1, 1, 1, 0, 0}, false, KMX_OK, "", "pose 1 reached over the loop closure 0 -> 5");
    c.w0[5] = 0.0;  // ... which does not count at weight 0
    mask({0, 1, 1, 1, 1, 1, 0, 0}, false, KMX_EINVAL, "pose 1 is not connected", "a fixed edge of weight 0");
    std::vector<uint8_t> rec;
    const std::vector<uint8_t> fx = {1, 0, 1, 0, 1, 0, 1, 0};
    kmx::chordal_record_fixed(c, fx.data(), &rec);
    bool ok = rec.size() == c.inc_edge.size();
    for (size_t k = 0; ok && k < rec.size(); ++k) ok = rec[k] == fx[c.inc_edge[k]];
    kmx::chordal_record_fixed(c, nullptr, &rec);
    for (size_t k = 0; ok && k < rec.size(); ++k) ok = rec[k] == 0;
    if (!ok || rec.size() != c.inc_edge.size()) {
      std::fprintf(stderr, "chordal_record_fixed: wrong flags\n");
      ++g_fail;
    }
    if (c.w0.size() != 8 || c.w0[0] != 1.0) {
      std::fprintf(stderr, "chordal_build: w0 not kept\n");
      ++g_fail;
    }
  }
  {
    Graph g;  // every pose an anchor: no fixed edge is needed
    g.n = 3;
    g.block_ptr = {0, 3};
    g.anchors = {0, 1, 2};
    g.edge(0, 1);
    kmx::ChordalGraph c;
    std::string err;
    if (g.build(&c, &err) != KMX_OK || kmx::chordal_check_fixed(c, nullptr, &err) != KMX_OK) {
      std::fprintf(stderr, "fixed mask: all anchors refused (%s)\n", err.c_str());
      ++g_fail;
    }
    ++robust;
  }
  // random multi-block graphs with parallel edges, hubs and empty blocks
  std::mt19937 rng(1234);
  int graphs = 0;
  for (int rep = 0; rep < 200; ++rep) {
    Graph g;
    const int nb = 1 + (int)(rng() % 5);
    g.block_ptr = {0};
    for (int b = 0; b < nb; ++b) {
      const int32_t nbp = rng() % 4 == 0 ? 0 : 1 + (int32_t)(rng() % 150);
      const int32_t p0 = g.block_ptr.back();
      g.block_ptr.push_back(p0 + nbp);
      if (nbp == 0) continue;
      g.anchors.push_back(p0 + (int32_t)(rng() % nbp));
      for (int32_t p = 0; p + 1 < nbp; ++p) g.edge(p0 + p, p0 + p + 1, 1.0 + (rng() % 7), 1.0 + (rng() % 5));
      const int extra = (int)(rng() % (2 * nbp));
      for (int k = 0; k < extra && nbp > 1; ++k) {
        const int32_t i = p0 + (rng() % 3 == 0 ? 0 : (int32_t)(rng() % nbp)), j = p0 + (int32_t)(rng() % nbp);
        if (i != j) g.edge(i, j, 0.5, 0.25, rng() % 5 == 0 ? 0.0 : 1.5);
      }
    }
    g.n = g.block_ptr.back();
    if (g.n == 0) continue;
    expect_ok_csr(g, "random graph");
    ++graphs;
  }
  if (g_fail) {
    std::fprintf(stderr, "chordal_check: %d failure(s)\n", g_fail);
    return 1;
  }
  std::printf("chordal_check ok: %d random graphs, CSR and tiles verified, %d malformed graphs refused, %d robust-solve checks\n",
              graphs, refused, robust);
  return 0;
}
