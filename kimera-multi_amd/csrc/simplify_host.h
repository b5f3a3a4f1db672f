// simplify_host.h — host side of the voxel simplification handle
// (simplify.hip): the parameter and argument checks, the key arithmetic the
// kernels share with those checks (the voxel index by an fp64 division, the
// time window by a floor division), the table-size rule and the checks of the
// keyframe arrays of kmx_simplify_graph. Plain C++ with no HIP call, so every
// kmx_simplify_* entry rejects a bad call before it touches a device, and
// simplify_check.cpp can run the same code under the host sanitizers.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>

#include "kmx_abi.h"

#ifdef __HIP__
#define KMX_SIMP_HD __host__ __device__
#else
#define KMX_SIMP_HD
#endif

namespace kmx {

constexpr uint64_t SIMP_DEFAULT_SLOTS = 1024;
constexpr uint32_t SIMP_EMPTY = 0xffffffffu;
// the exclusive scan: a workgroup owns SIMP_SCAN_SPAN elements, and the one
// workgroup of the second level takes the partials SIMP_SCAN_TOP at a time
constexpr int SIMP_SCAN_BLOCK = 256, SIMP_SCAN_ITEMS = 4;
constexpr int SIMP_SCAN_SPAN = SIMP_SCAN_BLOCK * SIMP_SCAN_ITEMS;
constexpr int SIMP_SCAN_TOP = 256;
constexpr int64_t SIMP_SCAN_SPAN2 = (int64_t)SIMP_SCAN_SPAN * SIMP_SCAN_TOP;

// floor(double(x) / resolution): a division, as numpy states it, never a
// multiplication by the reciprocal (49.0f / 49.0 is 1, 49.0f * (1 / 49.0) is not).
KMX_SIMP_HD inline double simp_voxel(float x, double resolution) { return floor((double)x / resolution); }

// s / h rounded toward minus infinity, h > 0.
KMX_SIMP_HD inline int64_t simp_floor_div(int64_t s, int64_t h) {
  const int64_t q = s / h;
  return (s % h != 0 && s < 0) ? q - 1 : q;
}
KMX_SIMP_HD inline int64_t simp_window(int64_t stamp, int64_t horizon_ns) {
  return horizon_ns > 0 ? simp_floor_div(stamp, horizon_ns) : 0;
}

// First position in the non-decreasing stamps[lo, hi) whose stamp is >= v.
KMX_SIMP_HD inline int64_t simp_lower(const int64_t* stamps, int64_t lo, int64_t hi, int64_t v) {
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (stamps[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

inline int simp_bad(std::string* err, int code, const std::string& msg) {
  if (err) *err = msg;
  return code;
}

inline bool simp_pow2(uint64_t v) { return v && !(v & (v - 1)); }

inline int simp_check_params(const kmx_simplify_params* p, std::string* err) {
  if (!p) return simp_bad(err, KMX_EINVAL, "null params");
  if (!(std::isfinite(p->resolution) && p->resolution > 0.0))
    return simp_bad(err, KMX_EINVAL, "resolution must be finite and > 0");
  if (p->horizon_ns < 0) return simp_bad(err, KMX_EINVAL, "horizon_ns must be >= 0");
  if (p->n_robots < 1 || p->n_robots > 65536) return simp_bad(err, KMX_EINVAL, "n_robots must be in 1..65536");
  if (p->initial_slots < 0 || (p->initial_slots > 0 && !simp_pow2((uint64_t)p->initial_slots)))
    return simp_bad(err, KMX_EINVAL, "initial_slots must be 0 or a power of two");
  return KMX_OK;
}

// The table-size rule: a power of two, at least twice the items the table is
// about to hold, never below the initial size and never smaller than it is.
inline uint64_t simp_slots_for(uint64_t current, int32_t initial_slots, int64_t items) {
  uint64_t s = initial_slots > 0 ? (uint64_t)initial_slots : SIMP_DEFAULT_SLOTS;
  if (current > s) s = current;
  while (s < 2 * (uint64_t)items) s *= 2;
  return s;
}

// One append against a handle that holds n_have vertices and f_have input
// faces; changes nothing.
inline int simp_check_add(const kmx_simplify_params& P, int64_t n_have, int64_t f_have, int64_t n,
                          const int32_t* robot, const int64_t* stamp_ns, const float* xyz, int64_t nf,
                          const int32_t* faces, std::string* err) {
  if (n < 0 || nf < 0) return simp_bad(err, KMX_EINVAL, "n_vertices and n_faces must be >= 0");
  if (n > 0 && (!robot || !stamp_ns || !xyz)) return simp_bad(err, KMX_EINVAL, "null vertex array");
  if (nf > 0 && !faces) return simp_bad(err, KMX_EINVAL, "null face array");
  if (n >= INT32_MAX - n_have) return simp_bad(err, KMX_EUNSUP, "2^31 - 1 vertices or more");
  if (nf >= INT32_MAX - f_have) return simp_bad(err, KMX_EUNSUP, "2^31 - 1 faces or more");
  for (int64_t i = 0; i < n; ++i)
    if (robot[i] < 0 || robot[i] >= P.n_robots) return simp_bad(err, KMX_EINVAL, "vertex robot id out of range");
  for (int64_t i = 0; i < 3 * n; ++i) {
    if (!std::isfinite(xyz[i])) return simp_bad(err, KMX_EINVAL, "vertex position is not finite");
    if (!(std::fabs(simp_voxel(xyz[i], P.resolution)) <= (double)INT32_MAX))
      return simp_bad(err, KMX_EINVAL, "voxel index beyond int32: |floor(x / resolution)| > 2^31 - 1");
  }
  const int64_t total = n_have + n;
  for (int64_t i = 0; i < 3 * nf; ++i)
    if (faces[i] < 0 || faces[i] >= total) return simp_bad(err, KMX_EINVAL, "face index out of range");
  return KMX_OK;
}

// The keyframe arrays of kmx_simplify_graph against a handle of P.n_robots
// robots and n_control control vertices.
inline int simp_check_graph(const kmx_simplify_params& P, int64_t n_control, int32_t n_robots,
                            const int64_t* kf_offset, const int64_t* kf_stamp, double w_mesh, double w_link,
                            std::string* err) {
  if (n_robots != P.n_robots) return simp_bad(err, KMX_EINVAL, "n_robots differs from the handle's");
  if (!kf_offset) return simp_bad(err, KMX_EINVAL, "null kf_offset");
  if (kf_offset[0] != 0) return simp_bad(err, KMX_EINVAL, "kf_offset[0] must be 0");
  for (int32_t a = 0; a < n_robots; ++a)
    if (kf_offset[a + 1] < kf_offset[a]) return simp_bad(err, KMX_EINVAL, "kf_offset must not decrease");
  const int64_t nk = kf_offset[n_robots];
  if (nk >= INT32_MAX - n_control) return simp_bad(err, KMX_EUNSUP, "2^31 - 1 graph nodes or more");
  if (nk > 0 && !kf_stamp) return simp_bad(err, KMX_EINVAL, "null kf_stamp");
  if (!std::isfinite(w_mesh) || !std::isfinite(w_link)) return simp_bad(err, KMX_EINVAL, "weight is not finite");
  for (int32_t a = 0; a < n_robots; ++a)
    for (int64_t i = kf_offset[a] + 1; i < kf_offset[a + 1]; ++i)
      if (kf_stamp[i] < kf_stamp[i - 1])
        return simp_bad(err, KMX_EINVAL, "robot " + std::to_string(a) + ": keyframe stamps decrease");
  return KMX_OK;
}

// What kmx_simplify_graph says of control vertices without a keyframe: the
// lowest robot that has some, how many, and the first of them.
inline std::string simp_missing_message(int32_t robot, int64_t count, int64_t first) {
  return "robot " + std::to_string(robot) + ": " + std::to_string(count) +
         " control vertices have no keyframe at their stamp (first: control vertex " + std::to_string(first) + ")";
}

}  // namespace kmx
