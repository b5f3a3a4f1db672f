// graph_host.h — what chordal_host.h and cert_host.h share: the per-edge
// argument checks of their set_graph calls and the per-pose incidence CSR.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

namespace kmx {

constexpr uint32_t GRAPH_TAIL = 1u << 31;  // record bit: this pose is the edge's source / tail (p == i)

// Every edge: endpoints in [0, n), no self-loop, extra(e) (its message, or nullptr), R and t finite, kappa and
// tau finite and > 0, in this order. Returns the first error's text, empty when all pass.
template <typename Extra>
std::string graph_check_edges(int32_t n, int64_t m, const int32_t* src, const int32_t* dst, const double* R,
                              const double* t, const double* kappa, const double* tau, Extra&& extra) {
  for (int64_t e = 0; e < m; ++e) {
    const std::string at = " (edge " + std::to_string(e) + ")";
    if (src[e] < 0 || src[e] >= n || dst[e] < 0 || dst[e] >= n) return "edge endpoint out of range" + at;
    if (src[e] == dst[e]) return "edge from a pose to itself" + at;
    if (const char* x = extra(e)) return x + at;
    for (int k = 0; k < 9; ++k)
      if (!std::isfinite(R[9 * e + k])) return "R not finite" + at;
    for (int k = 0; k < 3; ++k)
      if (!std::isfinite(t[3 * e + k])) return "t not finite" + at;
    if (!std::isfinite(kappa[e]) || !(kappa[e] > 0)) return "kappa must be finite and > 0" + at;
    if (!std::isfinite(tau[e]) || !(tau[e] > 0)) return "tau must be finite and > 0" + at;
  }
  return std::string();
}

// Incidence CSR by counting sort: a pose's records come in edge order, and an edge's two records are distinct
// (src != dst). inc_other: the other endpoint, | GRAPH_TAIL at the source; inc_edge: the caller's edge index.
inline void graph_incidence_csr(int32_t n, int64_t m, const int32_t* src, const int32_t* dst, std::vector<int32_t>* inc_ptr,
                                std::vector<uint32_t>* inc_other, std::vector<int32_t>* inc_edge) {
  inc_ptr->assign((size_t)n + 1, 0);
  for (int64_t e = 0; e < m; ++e) ++(*inc_ptr)[src[e] + 1], ++(*inc_ptr)[dst[e] + 1];
  for (int32_t p = 0; p < n; ++p) (*inc_ptr)[p + 1] += (*inc_ptr)[p];
  inc_other->resize((size_t)2 * (size_t)m);
  inc_edge->resize((size_t)2 * (size_t)m);
  std::vector<int32_t> fill(inc_ptr->begin(), inc_ptr->end() - 1);
  for (int64_t e = 0; e < m; ++e) {
    const size_t ks = (size_t)fill[src[e]]++, kd = (size_t)fill[dst[e]]++;
    (*inc_other)[ks] = (uint32_t)dst[e] | GRAPH_TAIL;
    (*inc_other)[kd] = (uint32_t)src[e];
    (*inc_edge)[ks] = (*inc_edge)[kd] = (int32_t)e;
  }
}

}  // namespace kmx
