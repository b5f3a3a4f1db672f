// simplify_check.cpp — simplify.hip's host code (simplify_host.h: the
// parameter, append and keyframe checks, the voxel division and the window's
// floor division, the table-size rule, the links' binary search) as a
// stand-alone program, built by `make simplify_check` with the host address
// and undefined-behaviour sanitizers. It feeds the checks what the
// kmx_simplify_* entries must reject, in arrays of the exact size so a read
// past one is a sanitizer report, and compares the arithmetic with plain
// restatements. CPU only.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "simplify_host.h"

namespace {

int g_fail = 0;
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
      ++g_fail;                                                        \
    }                                                                  \
  } while (0)

const int64_t I64MIN = std::numeric_limits<int64_t>::min(), I64MAX = std::numeric_limits<int64_t>::max();

kmx_simplify_params good_params() { return kmx_simplify_params{0.5, 0, 2, 0}; }

void test_params() {
  std::string err;
  kmx_simplify_params p = good_params();
  EXPECT(kmx::simp_check_params(&p, &err) == KMX_OK);
  EXPECT(kmx::simp_check_params(nullptr, &err) == KMX_EINVAL);
  for (double r : {0.0, -1.0, (double)NAN, (double)INFINITY, -(double)INFINITY}) {
    p = good_params();
    p.resolution = r;
    EXPECT(kmx::simp_check_params(&p, &err) == KMX_EINVAL && !err.empty());
  }
  p = good_params();
  p.horizon_ns = -1;
  EXPECT(kmx::simp_check_params(&p, &err) == KMX_EINVAL);
  p.horizon_ns = I64MAX;
  EXPECT(kmx::simp_check_params(&p, &err) == KMX_OK);
  for (int nr : {0, -1, 65537}) {
    p = good_params();
    p.n_robots = nr;
    EXPECT(kmx::simp_check_params(&p, &err) == KMX_EINVAL);
  }
  for (int s : {-1, 3, 6, 1000, INT32_MAX}) {
    p = good_params();
    p.initial_slots = s;
    EXPECT(kmx::simp_check_params(&p, &err) == KMX_EINVAL);
  }
  for (int s : {0, 1, 2, 64, 1 << 30}) {
    p = good_params();
    p.initial_slots = s;
    EXPECT(kmx::simp_check_params(&p, &err) == KMX_OK);
  }
}

void test_arithmetic() {
  // the window: toward minus infinity, negative stamps included
  EXPECT(kmx::simp_floor_div(-1, 1000) == -1);
  EXPECT(kmx::simp_floor_div(0, 1000) == 0);
  EXPECT(kmx::simp_floor_div(999, 1000) == 0);
  EXPECT(kmx::simp_floor_div(1000, 1000) == 1);
  EXPECT(kmx::simp_floor_div(-1000, 1000) == -1);
  EXPECT(kmx::simp_floor_div(-1001, 1000) == -2);
  EXPECT(kmx::simp_floor_div(I64MIN, 1) == I64MIN);
  EXPECT(kmx::simp_floor_div(I64MIN, I64MAX) == -2);
  EXPECT(kmx::simp_floor_div(I64MAX, I64MAX) == 1);
  EXPECT(kmx::simp_floor_div(I64MIN + 1, I64MAX) == -1);
  EXPECT(kmx::simp_window(-5, 0) == 0 && kmx::simp_window(12345, 0) == 0);
  EXPECT(kmx::simp_window(-1, 1000000000) == -1 && kmx::simp_window(0, 1000000000) == 0);
  for (int64_t s = -50; s <= 50; ++s)
    for (int64_t h : {1, 2, 3, 7, 50, 51}) EXPECT(kmx::simp_floor_div(s, h) == (int64_t)std::floor((double)s / (double)h));
  // the voxel: a division. 49 k / 49 is k; times the reciprocal it is below k for these k
  const double inv = 1.0 / 49.0;
  for (int k : {1, 2, 3, 4, 6, 7}) {
    const float x = 49.0f * (float)k;
    EXPECT(kmx::simp_voxel(x, 49.0) == (double)k);
    EXPECT(std::floor((double)x * inv) == (double)(k - 1));
  }
  EXPECT(kmx::simp_voxel(-0.0f, 1.0) == 0.0);
  EXPECT(kmx::simp_voxel(-0.25f, 0.5) == -1.0);
  EXPECT(kmx::simp_voxel(-0.5f, 0.5) == -1.0);
  EXPECT(kmx::simp_voxel(0.5f, 0.5) == 1.0);
  EXPECT(kmx::simp_voxel(-1e-30f, 0.5) == -1.0);
}

void test_slots() {
  EXPECT(kmx::simp_slots_for(0, 0, 0) == 1024);
  EXPECT(kmx::simp_slots_for(0, 64, 0) == 64);
  EXPECT(kmx::simp_slots_for(64, 64, 32) == 64);
  EXPECT(kmx::simp_slots_for(64, 64, 33) == 128);
  EXPECT(kmx::simp_slots_for(4096, 64, 3) == 4096);  // never smaller than it is
  EXPECT(kmx::simp_slots_for(1, 1, (int64_t)INT32_MAX - 1) == (1ull << 32));
  for (int64_t items : {1, 2, 511, 512, 513, 100000}) {
    const uint64_t s = kmx::simp_slots_for(0, 1, items);
    EXPECT(kmx::simp_pow2(s) && s >= 2 * (uint64_t)items && s / 2 < 2 * (uint64_t)items);
  }
}

struct Batch {
  std::vector<int32_t> robot, faces;
  std::vector<int64_t> stamp;
  std::vector<float> xyz;
  void vertex(int32_t r, int64_t s, float x, float y, float z) {
    robot.push_back(r);
    stamp.push_back(s);
    xyz.insert(xyz.end(), {x, y, z});
  }
  void face(int a, int b, int c) { faces.insert(faces.end(), {a, b, c}); }
};

int check(const kmx_simplify_params& P, int64_t have, int64_t fhave, const Batch& in, std::string* err) {
  Batch b(in);  // exact-size copies
  return kmx::simp_check_add(P, have, fhave, (int64_t)b.robot.size(), b.robot.data(), b.stamp.data(), b.xyz.data(),
                             (int64_t)b.faces.size() / 3, b.faces.data(), err);
}

void test_add() {
  std::string err;
  const kmx_simplify_params P = good_params();
  Batch b;
  b.vertex(0, 5, 0.f, 1.f, 2.f);
  b.vertex(1, -5, -3.f, 1.f, 2.f);
  b.face(0, 1, 11);
  EXPECT(check(P, 10, 0, b, &err) == KMX_OK);
  EXPECT(check(P, 9, 0, b, &err) == KMX_EINVAL);  // 11 is the vertices so far plus this append's
  EXPECT(err.find("face index") != std::string::npos);
  Batch none;
  EXPECT(check(P, 0, 0, none, &err) == KMX_OK);
  none.face(0, 0, 0);
  EXPECT(check(P, 0, 0, none, &err) == KMX_EINVAL);  // faces with no vertex at all
  EXPECT(check(P, 1, 0, none, &err) == KMX_OK);      // faces among earlier vertices only
  Batch neg(b);
  neg.faces[1] = -1;
  EXPECT(check(P, 10, 0, neg, &err) == KMX_EINVAL);
  for (int32_t r : {-1, 2, INT32_MAX}) {
    Batch c(b);
    c.robot[1] = r;
    EXPECT(check(P, 10, 0, c, &err) == KMX_EINVAL && err.find("robot") != std::string::npos);
  }
  for (float bad : {(float)NAN, (float)INFINITY, -(float)INFINITY}) {
    Batch c(b);
    c.xyz[4] = bad;
    EXPECT(check(P, 10, 0, c, &err) == KMX_EINVAL && err.find("finite") != std::string::npos);
  }
  {  // the voxel index against int32, by the same division
    Batch c(b);
    c.xyz[0] = 1.0e9f;  // / 0.5 = 2e9 < 2^31 - 1
    EXPECT(check(P, 10, 0, c, &err) == KMX_OK);
    c.xyz[0] = 1.1e9f;  // 2.2e9
    EXPECT(check(P, 10, 0, c, &err) == KMX_EINVAL && err.find("int32") != std::string::npos);
    c.xyz[0] = -1.1e9f;
    EXPECT(check(P, 10, 0, c, &err) == KMX_EINVAL);
    kmx_simplify_params Q = P;
    Q.resolution = 1e-300;
    EXPECT(check(Q, 10, 0, b, &err) == KMX_EINVAL);  // the quotient overflows to infinity
  }
  // nulls and negative counts
  EXPECT(kmx::simp_check_add(P, 0, 0, 1, nullptr, b.stamp.data(), b.xyz.data(), 0, nullptr, &err) == KMX_EINVAL);
  EXPECT(kmx::simp_check_add(P, 0, 0, 1, b.robot.data(), nullptr, b.xyz.data(), 0, nullptr, &err) == KMX_EINVAL);
  EXPECT(kmx::simp_check_add(P, 0, 0, 1, b.robot.data(), b.stamp.data(), nullptr, 0, nullptr, &err) == KMX_EINVAL);
  EXPECT(kmx::simp_check_add(P, 5, 0, 0, nullptr, nullptr, nullptr, 1, nullptr, &err) == KMX_EINVAL);
  EXPECT(kmx::simp_check_add(P, 0, 0, -1, nullptr, nullptr, nullptr, 0, nullptr, &err) == KMX_EINVAL);
  EXPECT(kmx::simp_check_add(P, 0, 0, 0, nullptr, nullptr, nullptr, -1, nullptr, &err) == KMX_EINVAL);
  EXPECT(kmx::simp_check_add(P, 0, 0, 0, nullptr, nullptr, nullptr, 0, nullptr, &err) == KMX_OK);
  // totals at or above 2^31 - 1 (decided before an array is read)
  EXPECT(check(P, (int64_t)INT32_MAX - 2, 0, b, &err) == KMX_EUNSUP);
  EXPECT(check(P, (int64_t)INT32_MAX - 3, (int64_t)INT32_MAX - 1, b, &err) == KMX_EUNSUP);
}

void test_graph() {
  std::string err;
  const kmx_simplify_params P = good_params();
  const std::vector<int64_t> off{0, 3, 5}, st{-4, -4, 9, 1, 1};
  EXPECT(kmx::simp_check_graph(P, 7, 2, off.data(), st.data(), 1.0, 1.0, &err) == KMX_OK);
  EXPECT(kmx::simp_check_graph(P, 7, 1, off.data(), st.data(), 1.0, 1.0, &err) == KMX_EINVAL);
  EXPECT(kmx::simp_check_graph(P, 7, 3, off.data(), st.data(), 1.0, 1.0, &err) == KMX_EINVAL);
  EXPECT(kmx::simp_check_graph(P, 7, 2, nullptr, st.data(), 1.0, 1.0, &err) == KMX_EINVAL);
  EXPECT(kmx::simp_check_graph(P, 7, 2, off.data(), nullptr, 1.0, 1.0, &err) == KMX_EINVAL);
  EXPECT(kmx::simp_check_graph(P, 7, 2, off.data(), st.data(), NAN, 1.0, &err) == KMX_EINVAL);
  const std::vector<int64_t> off1{1, 3, 5}, off2{0, 3, 2}, empty{0, 0, 0};
  EXPECT(kmx::simp_check_graph(P, 7, 2, off1.data(), st.data(), 1.0, 1.0, &err) == KMX_EINVAL);
  EXPECT(kmx::simp_check_graph(P, 7, 2, off2.data(), st.data(), 1.0, 1.0, &err) == KMX_EINVAL);
  EXPECT(kmx::simp_check_graph(P, 7, 2, empty.data(), nullptr, 1.0, 1.0, &err) == KMX_OK);
  const std::vector<int64_t> dec{-4, -5, 9, 1, 1}, dec2{-4, -4, 9, 1, 0}, across{5, 6, 9, 1, 1};
  EXPECT(kmx::simp_check_graph(P, 7, 2, off.data(), dec.data(), 1.0, 1.0, &err) == KMX_EINVAL);
  EXPECT(err.find("robot 0") != std::string::npos);
  EXPECT(kmx::simp_check_graph(P, 7, 2, off.data(), dec2.data(), 1.0, 1.0, &err) == KMX_EINVAL);
  EXPECT(err.find("robot 1") != std::string::npos);
  EXPECT(kmx::simp_check_graph(P, 7, 2, off.data(), across.data(), 1.0, 1.0, &err) == KMX_OK);  // 9 then 1: two robots
  EXPECT(kmx::simp_check_graph(P, (int64_t)INT32_MAX - 5, 2, off.data(), st.data(), 1.0, 1.0, &err) == KMX_EUNSUP);
  // the links' search: the first keyframe at the stamp, inside the robot's range only
  EXPECT(kmx::simp_lower(st.data(), 0, 3, -4) == 0);
  EXPECT(kmx::simp_lower(st.data(), 0, 3, 9) == 2);
  EXPECT(kmx::simp_lower(st.data(), 0, 3, 10) == 3);
  EXPECT(kmx::simp_lower(st.data(), 3, 5, 1) == 3);
  EXPECT(kmx::simp_lower(st.data(), 3, 5, 0) == 3);
  EXPECT(kmx::simp_lower(st.data(), 3, 3, 0) == 3);
  const std::string m = kmx::simp_missing_message(1, 12, 345);
  EXPECT(m.find("robot 1: 12 control vertices have no keyframe at their stamp") == 0);
  EXPECT(m.find("345") != std::string::npos);
}

}  // namespace

int main() {
  test_params();
  test_arithmetic();
  test_slots();
  test_add();
  test_graph();
  if (g_fail) {
    std::fprintf(stderr, "simplify_check: %d failure(s)\n", g_fail);
    return 1;
  }
  std::printf("simplify_check ok\n");
  return 0;
}
