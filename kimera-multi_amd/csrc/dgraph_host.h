// dgraph_host.h — host side of the deformation graph handle (dgraph.hip): the
// node, edge, prior and parameter checks, the incidence CSR and the tiles, the
// union-find rule of well-posedness and the free-node map. Plain C++ with no
// HIP call, so every kmx_dgraph_* entry rejects a bad call before it touches a
// device, and dgraph_check.cpp can run the same code under the host
// sanitizers.
#pragma once
#include <cmath>
#include <cstdint>
#include <numeric>
#include <string>
#include <vector>

#include "graph_host.h"
#include "kmx_abi.h"

namespace kmx {

constexpr int DG_TILE = 64;  // nodes per tile: one wave, a lane per node

inline int dg_bad(std::string* err, int code, const std::string& msg) {
  if (err) *err = msg;
  return code;
}

inline bool dg_all_finite(const double* a, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(a[i])) return false;
  return true;
}

// The parameters with every default filled in.
struct DgParams {
  double lambda_init = 1e-5, factor = 10.0, lambda_min = 1e-10, lambda_max = 1e5;
  double rel_tol = 1e-5, abs_tol = 0.0, cg_rtol = 1e-6;
  int32_t max_iterations = 100, cg_max_iterations = 500, check_every = 50;
};

// p == nullptr: every default. KMX_EINVAL for a value that is not finite, a
// negative count or tolerance, a factor <= 1 or lambda_min > lambda_max.
inline int dg_check_params(const kmx_dgraph_params* p, DgParams* out, std::string* err) {
  DgParams q;
  if (p) {
    const double v[7] = {p->lambda_init, p->lambda_factor, p->lambda_min, p->lambda_max,
                         p->rel_tol,     p->abs_tol,       p->cg_rtol};
    if (!dg_all_finite(v, 7)) return dg_bad(err, KMX_EINVAL, "a parameter is not finite");
    if (p->lambda_init < 0 || p->lambda_factor < 0 || p->lambda_min < 0 || p->lambda_max < 0 || p->cg_rtol < 0)
      return dg_bad(err, KMX_EINVAL, "lambda_init, lambda_factor, lambda_min, lambda_max and cg_rtol must be >= 0");
    if (p->max_iterations < 0 || p->cg_max_iterations < 0 || p->check_every < 0)
      return dg_bad(err, KMX_EINVAL, "max_iterations, cg_max_iterations and check_every must be >= 0");
    if (p->reserved != 0) return dg_bad(err, KMX_EUNSUP, "reserved must be 0");
    if (p->lambda_init > 0) q.lambda_init = p->lambda_init;
    if (p->lambda_factor > 0) q.factor = p->lambda_factor;
    if (p->lambda_min > 0) q.lambda_min = p->lambda_min;
    if (p->lambda_max > 0) q.lambda_max = p->lambda_max;
    if (p->rel_tol >= 0) q.rel_tol = p->rel_tol;
    if (p->abs_tol > 0) q.abs_tol = p->abs_tol;
    if (p->cg_rtol > 0) q.cg_rtol = p->cg_rtol;
    if (p->max_iterations > 0) q.max_iterations = p->max_iterations;
    if (p->cg_max_iterations > 0) q.cg_max_iterations = p->cg_max_iterations;
    if (p->check_every > 0) q.check_every = p->check_every;
    if (!(q.factor > 1.0)) return dg_bad(err, KMX_EINVAL, "lambda_factor must be > 1");
    if (q.lambda_min > q.lambda_max) return dg_bad(err, KMX_EINVAL, "lambda_min above lambda_max");
  }
  if (out) *out = q;
  return KMX_OK;
}

// w == nullptr: all 1.
inline int dg_check_weights(int64_t m, const double* w, std::string* err) {
  if (!w) return KMX_OK;
  for (int64_t e = 0; e < m; ++e)
    if (!std::isfinite(w[e]) || w[e] < 0)
      return dg_bad(err, KMX_EINVAL, "edge weight must be finite and >= 0 (edge " + std::to_string(e) + ")");
  return KMX_OK;
}

// What set_graph keeps on the host: the edges, the CSR and the tiles.
struct DgGraph {
  int32_t n = 0;
  int64_t m = 0;
  std::vector<int32_t> src, dst;
  std::vector<double> w;            // [m]
  std::vector<int32_t> inc_ptr;     // [n + 1]
  std::vector<uint32_t> inc_other;  // [2m] the other endpoint, | GRAPH_TAIL where this node is the edge's source
  std::vector<int32_t> inc_edge;    // [2m]
  int32_t n_tiles = 0;              // tile t: nodes [64 t, min(64 t + 64, n))
};

inline int32_t dg_tiles(int32_t n) { return (int32_t)(((int64_t)n + DG_TILE - 1) / DG_TILE); }

// Checks everything, then builds; *out is written only on success.
inline int dg_build(int32_t n, const double* Rrest, const double* g, int64_t m, const int32_t* src, const int32_t* dst,
                    const double* w, DgGraph* out, std::string* err) {
  if (n < 0 || m < 0) return dg_bad(err, KMX_EINVAL, "n and m must be >= 0");
  if (m > (int64_t)INT32_MAX / 2) return dg_bad(err, KMX_EINVAL, "more than 2^30 - 1 edges");
  if (n > INT32_MAX / 8) return dg_bad(err, KMX_EINVAL, "more than 2^28 - 1 nodes");  // 6 n is indexed in 32 bits
  if (n > 0 && (!Rrest || !g)) return dg_bad(err, KMX_EINVAL, "null node array");
  if (m > 0 && (!src || !dst)) return dg_bad(err, KMX_EINVAL, "null edge array");
  if (!dg_all_finite(Rrest, (size_t)n * 9) || !dg_all_finite(g, (size_t)n * 3))
    return dg_bad(err, KMX_EINVAL, "node pose is not finite");
  for (int64_t e = 0; e < m; ++e) {
    if (src[e] < 0 || src[e] >= n || dst[e] < 0 || dst[e] >= n)
      return dg_bad(err, KMX_EINVAL, "edge endpoint out of range (edge " + std::to_string(e) + ")");
    if (src[e] == dst[e]) return dg_bad(err, KMX_EINVAL, "edge from a node to itself (edge " + std::to_string(e) + ")");
  }
  if (int rc = dg_check_weights(m, w, err)) return rc;
  DgGraph G;
  G.n = n;
  G.m = m;
  G.src.assign(src, src + m);
  G.dst.assign(dst, dst + m);
  if (w)
    G.w.assign(w, w + m);
  else
    G.w.assign((size_t)m, 1.0);
  graph_incidence_csr(n, m, src, dst, &G.inc_ptr, &G.inc_other, &G.inc_edge);
  G.n_tiles = dg_tiles(n);
  *out = std::move(G);
  return KMX_OK;
}

// The records' weights in CSR order.
inline void dg_record_weights(const DgGraph& G, const double* w, std::vector<double>* rec_w) {
  rec_w->resize(G.inc_edge.size());
  for (size_t k = 0; k < G.inc_edge.size(); ++k) (*rec_w)[k] = w ? w[G.inc_edge[k]] : 1.0;
}

struct DgPriors {
  std::vector<uint8_t> mode;            // [n]
  std::vector<double> Rhat, that;       // [n][9], [n][3]; I and 0 where mode == 0
  std::vector<double> kappa, tau;       // [n]; 0 where mode != 1
  std::vector<int32_t> free_of, node_of;  // node -> free index or -1; free index -> node
};

// Checks the arrays; rows of nodes with mode 0 are not read. *out on success only.
inline int dg_check_priors(int32_t n, const uint8_t* mode, const double* Rhat, const double* that, const double* kappa,
                           const double* tau, DgPriors* out, std::string* err) {
  if (n > 0 && (!mode || !Rhat || !that || !kappa || !tau)) return dg_bad(err, KMX_EINVAL, "null prior array");
  DgPriors P;
  P.mode.assign((size_t)n, 0);
  P.Rhat.assign((size_t)n * 9, 0.0);
  P.that.assign((size_t)n * 3, 0.0);
  P.kappa.assign((size_t)n, 0.0);
  P.tau.assign((size_t)n, 0.0);
  P.free_of.assign((size_t)n, -1);
  for (int32_t i = 0; i < n; ++i) {
    const std::string at = " (node " + std::to_string(i) + ")";
    if (mode[i] > 2) return dg_bad(err, KMX_EINVAL, "prior mode must be 0, 1 or 2" + at);
    P.mode[(size_t)i] = mode[i];
    if (mode[i] == 0) {
      P.Rhat[(size_t)i * 9] = P.Rhat[(size_t)i * 9 + 4] = P.Rhat[(size_t)i * 9 + 8] = 1.0;
    } else {
      if (!dg_all_finite(Rhat + (size_t)i * 9, 9) || !dg_all_finite(that + (size_t)i * 3, 3))
        return dg_bad(err, KMX_EINVAL, "prior pose is not finite" + at);
      for (int c = 0; c < 9; ++c) P.Rhat[(size_t)i * 9 + c] = Rhat[(size_t)i * 9 + c];
      for (int c = 0; c < 3; ++c) P.that[(size_t)i * 3 + c] = that[(size_t)i * 3 + c];
    }
    if (mode[i] == 1) {
      if (!std::isfinite(kappa[i]) || kappa[i] < 0 || !std::isfinite(tau[i]) || tau[i] < 0)
        return dg_bad(err, KMX_EINVAL, "kappa and tau must be finite and >= 0" + at);
      P.kappa[(size_t)i] = kappa[i];
      P.tau[(size_t)i] = tau[i];
    }
    if (mode[i] != 2) {
      P.free_of[(size_t)i] = (int32_t)P.node_of.size();
      P.node_of.push_back(i);
    }
  }
  *out = std::move(P);
  return KMX_OK;
}

// Union-find over the edges of weight > 0: every component must hold a hard
// node or a soft node with tau > 0.
inline int dg_check_posed(int32_t n, int64_t m, const int32_t* src, const int32_t* dst, const double* w,
                          const DgPriors& P, std::string* err) {
  std::vector<int32_t> parent((size_t)n);
  std::iota(parent.begin(), parent.end(), 0);
  auto find = [&](int32_t x) {
    while (parent[(size_t)x] != x) {
      parent[(size_t)x] = parent[(size_t)parent[(size_t)x]];
      x = parent[(size_t)x];
    }
    return x;
  };
  for (int64_t e = 0; e < m; ++e) {
    if (w && !(w[e] > 0)) continue;
    const int32_t a = find(src[e]), b = find(dst[e]);
    if (a != b) parent[(size_t)(a < b ? b : a)] = a < b ? a : b;
  }
  std::vector<uint8_t> held((size_t)n, 0);
  for (int32_t i = 0; i < n; ++i)
    if (P.mode[(size_t)i] == 2 || (P.mode[(size_t)i] == 1 && P.tau[(size_t)i] > 0)) held[(size_t)find(i)] = 1;
  for (int32_t i = 0; i < n; ++i)
    if (!held[(size_t)find(i)])
      return dg_bad(err, KMX_EINVAL,
                    "the component of node " + std::to_string(i) + " holds no hard node and no soft node with tau > 0");
  return KMX_OK;
}

}  // namespace kmx
