// chordal_host.h — host-side half of chordal.hip that needs no device: the
// checks kmx_chordal_set_graph / kmx_chordal_set_weights run before any device
// call, and the per-pose incidence CSR and tile list they upload. Plain C++, so
// `make chordal_check` can build it with the host sanitizers
// (chordal_check.cpp).
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <string>
#include <vector>

#include "graph_host.h"
#include "kmx_abi.h"

namespace kmx {

constexpr int CH_TILE = 64;                 // poses per tile = lanes per workgroup (one wave)
constexpr uint32_t CH_DIR_OUT = GRAPH_TAIL;  // record bit: this pose is the edge's source (p == i)

// What kmx_chordal_set_graph keeps: the incidence CSR (sorted by pose, in edge
// order within a pose) and the tiles. A tile is at most CH_TILE consecutive
// poses of ONE block, so a block's partial sums do not depend on which other
// blocks are in the batch.
struct ChordalGraph {
  int32_t n = 0, nb = 0;
  int64_t m = 0;
  std::vector<int32_t> inc_ptr;     // [n + 1]
  std::vector<uint32_t> inc_other;  // [2m] other endpoint | CH_DIR_OUT
  std::vector<int32_t> inc_edge;    // [2m] the caller's edge index (weights are per edge)
  std::vector<double> inc_M;        // [2m][9] R_e when the pose is the target, R_e^T when it is the source
  std::vector<double> inc_t;        // [2m][3] t_ij
  std::vector<uint8_t> is_free;     // [n] 0: anchor
  std::vector<int32_t> tile_p0, tile_p1, tile_block;  // [n_tiles]
  std::vector<int32_t> tile_ptr;    // [nb + 1] a block's tiles
  std::vector<double> kappa, tau;   // [m]
  std::vector<int32_t> src, dst;    // [m] (kept for the connectivity check of set_weights)
  std::vector<double> w0;           // [m] the weights in force (set_graph / set_weights), for the robust solve's check
};

namespace chordal_detail {
inline int32_t uf_find(std::vector<int32_t>& parent, int32_t a) {
  while (parent[a] != a) {
    parent[a] = parent[parent[a]];
    a = parent[a];
  }
  return a;
}
}  // namespace chordal_detail

// Every connected component over the edges with weight > 0 (weight NULL: all)
// must hold an anchor; a free pose without a kept edge is such a component.
// The weights are checked here too (finite, >= 0). src / dst must already be
// in range. KMX_OK, or KMX_EINVAL with *err set.
inline int chordal_check_weights(int32_t n, int64_t m, const int32_t* src, const int32_t* dst, const double* weight,
                                 const uint8_t* is_free, std::string* err) {
  auto bad = [&](const std::string& s) {
    if (err) *err = s;
    return KMX_EINVAL;
  };
  if (weight)
    for (int64_t e = 0; e < m; ++e)
      if (!std::isfinite(weight[e]) || weight[e] < 0) return bad("weight must be finite and >= 0 (edge " + std::to_string(e) + ")");
  std::vector<int32_t> parent((size_t)n);
  std::iota(parent.begin(), parent.end(), 0);
  for (int64_t e = 0; e < m; ++e) {
    if (weight && weight[e] == 0) continue;
    const int32_t a = chordal_detail::uf_find(parent, src[e]), b = chordal_detail::uf_find(parent, dst[e]);
    if (a != b) parent[a] = b;
  }
  std::vector<uint8_t> anchored((size_t)n, 0);
  for (int32_t p = 0; p < n; ++p)
    if (!is_free[p]) anchored[chordal_detail::uf_find(parent, p)] = 1;
  for (int32_t p = 0; p < n; ++p)
    if (!anchored[chordal_detail::uf_find(parent, p)])
      return bad("pose " + std::to_string(p) + " is not connected to an anchor over the edges of weight > 0 (singular system)");
  return KMX_OK;
}

// Checks the arguments of kmx_chordal_set_graph and, when they pass, builds
// *out (untouched on failure). KMX_OK, or KMX_EINVAL with *err set.
inline int chordal_build(int32_t n, int32_t nb, const int32_t* block_ptr, int64_t m, const int32_t* src,
                         const int32_t* dst, const double* R, const double* t, const double* kappa, const double* tau,
                         const double* weight, int32_t n_anchors, const int32_t* anchors, ChordalGraph* out,
                         std::string* err) {
  auto bad = [&](const std::string& s) {
    if (err) *err = s;
    return KMX_EINVAL;
  };
  if (!out) return bad("null argument");
  if (n < 1 || nb < 1 || m < 0 || n_anchors < 0) return bad("bad argument (n_poses, n_blocks >= 1; n_edges, n_anchors >= 0)");
  if (!block_ptr) return bad("null block_ptr");
  if (m > 0 && (!src || !dst || !R || !t || !kappa || !tau)) return bad("null edge array");
  if (n_anchors > 0 && !anchors) return bad("null anchors");
  if (m >= (int64_t)INT32_MAX / 2) return bad("too many edges (2 * n_edges must fit int32)");
  if (block_ptr[0] != 0) return bad("block_ptr must start at 0");
  for (int32_t b = 0; b < nb; ++b)
    if (block_ptr[b + 1] < block_ptr[b] || block_ptr[b + 1] > n) return bad("block_ptr not monotone");
  if (block_ptr[nb] != n) return bad("block_ptr must cover [0, n_poses)");
  std::vector<int32_t> pose_block((size_t)n);
  for (int32_t b = 0; b < nb; ++b)
    for (int32_t p = block_ptr[b]; p < block_ptr[b + 1]; ++p) pose_block[p] = b;
  std::vector<uint8_t> is_free((size_t)n, 1);
  for (int32_t a = 0; a < n_anchors; ++a) {
    if (anchors[a] < 0 || anchors[a] >= n) return bad("anchor out of range");
    if (!is_free[anchors[a]]) return bad("anchor listed twice");
    is_free[anchors[a]] = 0;
  }
  std::string werr = graph_check_edges(n, m, src, dst, R, t, kappa, tau, [&](int64_t e) {
    return pose_block[src[e]] != pose_block[dst[e]] ? "edge across blocks" : nullptr;
  });
  if (!werr.empty()) return bad(werr);
  if (chordal_check_weights(n, m, src, dst, weight, is_free.data(), &werr) != KMX_OK) return bad(werr);

  ChordalGraph g;
  g.n = n;
  g.nb = nb;
  g.m = m;
  g.is_free = std::move(is_free);
  g.kappa.assign(kappa, kappa + m);
  g.tau.assign(tau, tau + m);
  g.src.assign(src, src + m);
  g.dst.assign(dst, dst + m);
  g.w0.assign((size_t)m, 1.0);
  if (weight) g.w0.assign(weight, weight + m);
  graph_incidence_csr(n, m, src, dst, &g.inc_ptr, &g.inc_other, &g.inc_edge);
  const size_t nrec = g.inc_edge.size();
  g.inc_M.resize(9 * nrec);
  g.inc_t.resize(3 * nrec);
  for (size_t k = 0; k < nrec; ++k) {  // the source's record: X_j R_e^T, the target's: X_i R_e
    const double* Re = R + 9 * (size_t)g.inc_edge[k];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) g.inc_M[9 * k + 3 * r + c] = (g.inc_other[k] & CH_DIR_OUT) ? Re[3 * c + r] : Re[3 * r + c];
    for (int q = 0; q < 3; ++q) g.inc_t[3 * k + q] = t[3 * (size_t)g.inc_edge[k] + q];
  }
  g.tile_ptr.assign((size_t)nb + 1, 0);
  for (int32_t b = 0; b < nb; ++b) {
    for (int32_t p = block_ptr[b]; p < block_ptr[b + 1]; p += CH_TILE) {
      g.tile_p0.push_back(p);
      g.tile_p1.push_back(std::min<int32_t>(p + CH_TILE, block_ptr[b + 1]));
      g.tile_block.push_back(b);
    }
    g.tile_ptr[b + 1] = (int32_t)g.tile_p0.size();
  }
  *out = std::move(g);
  return KMX_OK;
}

// The per-record weights w*kappa and w*tau the kernels read (weight NULL: 1).
inline void chordal_record_weights(const ChordalGraph& g, const double* weight, std::vector<double>* wk,
                                   std::vector<double>* wt) {
  const size_t nrec = g.inc_edge.size();
  wk->resize(nrec);
  wt->resize(nrec);
  for (size_t k = 0; k < nrec; ++k) {
    const int32_t e = g.inc_edge[k];
    const double w = weight ? weight[e] : 1.0;
    (*wk)[k] = w * g.kappa[e];
    (*wt)[k] = w * g.tau[e];
  }
}

// kmx_chordal_robust_params with the defaults filled in.
struct ChordalRobust {
  double barc = 5.0, mu_init = 0.0, mu_step = 1.4;
  int32_t max_updates = 100;
  bool start_projected = false;  // reserved == 1
};

// The parameter checks of kmx_chordal_solve_robust (rp NULL: the defaults).
inline int chordal_robust_params(const kmx_chordal_robust_params* rp, ChordalRobust* out, std::string* err) {
  auto bad = [&](const std::string& s) {
    if (err) *err = s;
    return KMX_EINVAL;
  };
  ChordalRobust r;
  if (rp) {
    if (!std::isfinite(rp->barc) || rp->barc < 0) return bad("barc must be finite and >= 0 (0: 5.0)");
    if (!std::isfinite(rp->mu_init) || rp->mu_init < 0) return bad("mu_init must be finite and >= 0 (0: from the residuals)");
    if (!std::isfinite(rp->mu_step) || rp->mu_step < 0) return bad("mu_step must be finite and >= 0 (0: 1.4)");
    if (rp->mu_step != 0 && !(rp->mu_step > 1)) return bad("mu_step must be > 1 when it is given");
    if (rp->max_updates < 0) return bad("max_updates must be >= 0 (0: 100)");
    if (rp->reserved != 0 && rp->reserved != 1) return bad("reserved must be 0 (1: the projected warm start)");
    if (rp->barc > 0) r.barc = rp->barc;
    r.mu_init = rp->mu_init;
    if (rp->mu_step > 0) r.mu_step = rp->mu_step;
    if (rp->max_updates > 0) r.max_updates = rp->max_updates;
    r.start_projected = rp->reserved == 1;
  }
  if (out) *out = r;
  return KMX_OK;
}

// The robust solve lets the device choose the weights of the edges that are
// not fixed, down to 0, without a connectivity check per update. That is safe
// only when the fixed edges of weight > 0 connect every free pose to an anchor
// by themselves: checked here, once, with chordal_check_weights' union-find
// (fixed NULL: no edge is fixed, so every pose must be an anchor).
inline int chordal_check_fixed(const ChordalGraph& g, const uint8_t* fixed, std::string* err) {
  std::vector<double> w((size_t)g.m, 0.0);
  if (fixed)
    for (int64_t e = 0; e < g.m; ++e)
      if (fixed[e]) w[(size_t)e] = g.w0[(size_t)e];
  std::string werr;
  if (chordal_check_weights(g.n, g.m, g.src.data(), g.dst.data(), w.data(), g.is_free.data(), &werr) != KMX_OK) {
    if (err) *err = "the fixed edges must connect every free pose to an anchor: " + werr;
    return KMX_EINVAL;
  }
  return KMX_OK;
}

// An edge's flag at both of its incidence records.
inline void chordal_record_fixed(const ChordalGraph& g, const uint8_t* fixed, std::vector<uint8_t>* out) {
  const size_t nrec = g.inc_edge.size();
  out->assign(nrec, 0);
  if (fixed)
    for (size_t k = 0; k < nrec; ++k) (*out)[k] = fixed[g.inc_edge[k]] ? 1 : 0;
}

}  // namespace kmx
