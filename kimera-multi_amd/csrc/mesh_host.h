// mesh_host.h — host side of the mesh deformation handle (mesh.hip): the
// parameter and argument checks, the saturating window arithmetic, the
// per-robot stamp-order check and the per-robot index bookkeeping. Plain C++
// with no HIP call, so every kmx_mesh_* entry rejects a bad call before it
// touches a device, and mesh_check.cpp can run the same code under the host
// sanitizers.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "kmx_abi.h"

#ifdef __HIP__
#define KMX_MESH_HD __host__ __device__
#else
#define KMX_MESH_HD
#endif

namespace kmx {

constexpr int MESH_MAX_K = 8;
constexpr int64_t MESH_I64_MIN = INT64_MIN, MESH_I64_MAX = INT64_MAX;

// s - w and s + w for w >= 0, saturating at the int64 limits (the kernel's
// binary searches and the reference use exactly these two bounds).
KMX_MESH_HD inline int64_t mesh_sat_sub(int64_t s, int64_t w) { return s < MESH_I64_MIN + w ? MESH_I64_MIN : s - w; }
KMX_MESH_HD inline int64_t mesh_sat_add(int64_t s, int64_t w) { return s > MESH_I64_MAX - w ? MESH_I64_MAX : s + w; }

// First position in the sorted stamps[lo, hi) whose stamp is >= v (lower) or
// > v (upper): the window of a vertex is [lower(s - W), upper(s + W)).
KMX_MESH_HD inline int32_t mesh_lower(const int64_t* stamps, int32_t lo, int32_t hi, int64_t v) {
  while (lo < hi) {
    const int32_t mid = lo + (hi - lo) / 2;
    if (stamps[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
KMX_MESH_HD inline int32_t mesh_upper(const int64_t* stamps, int32_t lo, int32_t hi, int64_t v) {
  while (lo < hi) {
    const int32_t mid = lo + (hi - lo) / 2;
    if (stamps[mid] <= v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

inline int mesh_bad(std::string* err, int code, const char* msg) {
  if (err) *err = msg;
  return code;
}

inline int mesh_check_params(const kmx_mesh_params* p, std::string* err) {
  if (!p) return mesh_bad(err, KMX_EINVAL, "null params");
  if (p->k < 1 || p->k > MESH_MAX_K) return mesh_bad(err, KMX_EUNSUP, "k: 1..8 are built");
  if (p->window_ns < 0) return mesh_bad(err, KMX_EINVAL, "window_ns must be >= 0");
  if (p->n_robots < 1 || p->n_robots > 65536) return mesh_bad(err, KMX_EINVAL, "n_robots must be in 1..65536");
  return KMX_OK;
}

inline bool mesh_all_finite(const double* a, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(a[i])) return false;
  return true;
}
inline bool mesh_all_finite(const float* a, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(a[i])) return false;
  return true;
}

// [first, first + n) inside [0, total), n >= 0, without overflow.
inline bool mesh_range_ok(int64_t first, int64_t n, int64_t total) {
  return first >= 0 && n >= 0 && first <= total && n <= total - first;
}

// The control nodes as the host keeps them: per-robot lists in append order
// (stamps non-decreasing within a robot, so each list is sorted and a node's
// position in its robot's list grows with its id), and the concatenation of
// those lists, robot by robot, that the bind kernel searches and scans.
struct MeshNodeIndex {
  int32_t n_robots = 0;
  int64_t n_nodes = 0;
  std::vector<std::vector<int32_t>> ids;  // [robot] node ids, increasing
  std::vector<int64_t> stamp;             // [n_nodes] by node id
  std::vector<double> g;                  // [n_nodes][3] rest positions by node id
  std::vector<int64_t> last_stamp;        // [robot] stamp of its newest node
  std::vector<int64_t> n_vertices;        // [robot]

  void init(int32_t robots) {
    n_robots = robots;
    n_nodes = 0;
    ids.assign((size_t)robots, {});
    stamp.clear();
    g.clear();
    last_stamp.assign((size_t)robots, MESH_I64_MIN);
    n_vertices.assign((size_t)robots, 0);
  }

  // Checks a batch of nodes; changes nothing.
  int check_nodes(int64_t n, const int32_t* robot, const int64_t* stamp_ns, const double* Rrest, const double* gpos,
                  std::string* err) const {
    if (n < 0) return mesh_bad(err, KMX_EINVAL, "n must be >= 0");
    if (n == 0) return KMX_OK;
    if (!robot || !stamp_ns || !Rrest || !gpos) return mesh_bad(err, KMX_EINVAL, "null node array");
    if (n > INT32_MAX - n_nodes) return mesh_bad(err, KMX_EINVAL, "more than 2^31 - 1 nodes");
    std::vector<int64_t> last(last_stamp);
    for (int64_t i = 0; i < n; ++i) {
      if (robot[i] < 0 || robot[i] >= n_robots) return mesh_bad(err, KMX_EINVAL, "node robot id out of range");
      if (stamp_ns[i] < last[(size_t)robot[i]])
        return mesh_bad(err, KMX_EINVAL, "node stamps go backwards within a robot");
      last[(size_t)robot[i]] = stamp_ns[i];
    }
    if (!mesh_all_finite(Rrest, (size_t)n * 9) || !mesh_all_finite(gpos, (size_t)n * 3))
      return mesh_bad(err, KMX_EINVAL, "node pose is not finite");
    return KMX_OK;
  }

  // Appends a checked batch.
  void append_nodes(int64_t n, const int32_t* robot, const int64_t* stamp_ns, const double* gpos) {
    for (int64_t i = 0; i < n; ++i) {
      ids[(size_t)robot[i]].push_back((int32_t)(n_nodes + i));
      last_stamp[(size_t)robot[i]] = stamp_ns[i];
    }
    stamp.insert(stamp.end(), stamp_ns, stamp_ns + n);
    g.insert(g.end(), gpos, gpos + 3 * n);
    n_nodes += n;
  }

  int check_vertices(int64_t n, int64_t n_have, const int32_t* robot, const int64_t* stamp_ns, const float* xyz,
                     std::string* err) const {
    if (n < 0) return mesh_bad(err, KMX_EINVAL, "n must be >= 0");
    if (n == 0) return KMX_OK;
    if (!robot || !stamp_ns || !xyz) return mesh_bad(err, KMX_EINVAL, "null vertex array");
    if (n > INT32_MAX - n_have) return mesh_bad(err, KMX_EINVAL, "more than 2^31 - 1 vertices");
    for (int64_t i = 0; i < n; ++i)
      if (robot[i] < 0 || robot[i] >= n_robots) return mesh_bad(err, KMX_EINVAL, "vertex robot id out of range");
    if (!mesh_all_finite(xyz, (size_t)n * 3)) return mesh_bad(err, KMX_EINVAL, "vertex position is not finite");
    return KMX_OK;
  }

  void count_vertices(int64_t n, const int32_t* robot) {
    for (int64_t i = 0; i < n; ++i) n_vertices[(size_t)robot[i]]++;
  }

  // The concatenated layout: robot a's nodes are positions [off[a], off[a+1]).
  void sorted_layout(std::vector<int32_t>* off, std::vector<int64_t>* s_stamp, std::vector<int32_t>* s_id,
                     std::vector<double>* s_g) const {
    off->assign((size_t)n_robots + 1, 0);
    s_stamp->resize((size_t)n_nodes);
    s_id->resize((size_t)n_nodes);
    s_g->resize((size_t)n_nodes * 3);
    size_t p = 0;
    for (int32_t a = 0; a < n_robots; ++a) {
      (*off)[(size_t)a] = (int32_t)p;
      for (int32_t id : ids[(size_t)a]) {
        (*s_stamp)[p] = stamp[(size_t)id];
        (*s_id)[p] = id;
        for (int c = 0; c < 3; ++c) (*s_g)[p * 3 + c] = g[(size_t)id * 3 + c];
        ++p;
      }
    }
    (*off)[(size_t)n_robots] = (int32_t)p;
  }
};

}  // namespace kmx
