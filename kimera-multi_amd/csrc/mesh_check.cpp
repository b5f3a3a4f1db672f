// mesh_check.cpp — mesh.hip's host code (mesh_host.h: the parameter and
// argument checks, the saturating window arithmetic, the per-robot stamp order
// and the per-robot index) as a stand-alone program, built by `make
// mesh_check` with the host address and undefined-behaviour sanitizers. It
// feeds the checks the inputs the kmx_mesh_* entries must reject, the int64
// extremes, an empty robot and n = 0, and compares the windows with a plain
// scan. CPU only.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "mesh_host.h"

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

struct Nodes {
  std::vector<int32_t> robot;
  std::vector<int64_t> stamp;
  std::vector<double> R, g;
  void add(int32_t r, int64_t s, double x = 0.0) {
    robot.push_back(r);
    stamp.push_back(s);
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    R.insert(R.end(), I, I + 9);
    g.insert(g.end(), {x, 2.0 * x, -x});
  }
};

// exact-size copies, so a read past an array is a sanitizer report
int check_nodes(const kmx::MeshNodeIndex& ix, const Nodes& n, std::string* err) {
  std::vector<int32_t> robot(n.robot);
  std::vector<int64_t> stamp(n.stamp);
  std::vector<double> R(n.R), g(n.g);
  return ix.check_nodes((int64_t)robot.size(), robot.data(), stamp.data(), R.data(), g.data(), err);
}

void test_params() {
  std::string err;
  kmx_mesh_params p{4, 2, 1000};
  EXPECT(kmx::mesh_check_params(&p, &err) == KMX_OK);
  EXPECT(kmx::mesh_check_params(nullptr, &err) == KMX_EINVAL);
  for (int k : {0, 9, -1, INT32_MAX}) {
    p.k = k;
    EXPECT(kmx::mesh_check_params(&p, &err) == KMX_EUNSUP);
  }
  for (int k = 1; k <= 8; ++k) {
    p.k = k;
    EXPECT(kmx::mesh_check_params(&p, &err) == KMX_OK);
  }
  p.window_ns = -1;
  EXPECT(kmx::mesh_check_params(&p, &err) == KMX_EINVAL);
  p.window_ns = I64MAX;
  EXPECT(kmx::mesh_check_params(&p, &err) == KMX_OK);
  p.n_robots = 0;
  EXPECT(kmx::mesh_check_params(&p, &err) == KMX_EINVAL);
}

void test_saturation() {
  EXPECT(kmx::mesh_sat_sub(I64MIN, 0) == I64MIN);
  EXPECT(kmx::mesh_sat_sub(I64MIN, 1) == I64MIN);
  EXPECT(kmx::mesh_sat_sub(I64MIN + 5, 5) == I64MIN);
  EXPECT(kmx::mesh_sat_sub(I64MIN + 5, 4) == I64MIN + 1);
  EXPECT(kmx::mesh_sat_sub(0, I64MAX) == -I64MAX);
  EXPECT(kmx::mesh_sat_sub(-2, I64MAX) == I64MIN);
  EXPECT(kmx::mesh_sat_sub(I64MAX, I64MAX) == 0);
  EXPECT(kmx::mesh_sat_add(I64MAX, 0) == I64MAX);
  EXPECT(kmx::mesh_sat_add(I64MAX, 1) == I64MAX);
  EXPECT(kmx::mesh_sat_add(I64MAX - 5, 5) == I64MAX);
  EXPECT(kmx::mesh_sat_add(I64MAX - 5, 4) == I64MAX - 1);
  EXPECT(kmx::mesh_sat_add(I64MIN, I64MAX) == -1);
  EXPECT(kmx::mesh_sat_add(1, I64MAX) == I64MAX);
}

void test_ranges() {
  EXPECT(kmx::mesh_range_ok(0, 0, 0));
  EXPECT(kmx::mesh_range_ok(5, 0, 5));
  EXPECT(!kmx::mesh_range_ok(6, 0, 5));
  EXPECT(kmx::mesh_range_ok(2, 3, 5));
  EXPECT(!kmx::mesh_range_ok(2, 4, 5));
  EXPECT(!kmx::mesh_range_ok(-1, 1, 5));
  EXPECT(!kmx::mesh_range_ok(0, -1, 5));
  EXPECT(!kmx::mesh_range_ok(1, I64MAX, 5));
  EXPECT(!kmx::mesh_range_ok(I64MAX, I64MAX, I64MAX));
}

void test_node_checks() {
  std::string err;
  kmx::MeshNodeIndex ix;
  ix.init(3);  // robot 1 stays empty
  Nodes empty;
  EXPECT(ix.check_nodes(0, nullptr, nullptr, nullptr, nullptr, &err) == KMX_OK);  // n = 0 reads nothing
  EXPECT(ix.check_nodes(-1, nullptr, nullptr, nullptr, nullptr, &err) == KMX_EINVAL);
  EXPECT(ix.check_nodes(1, nullptr, nullptr, nullptr, nullptr, &err) == KMX_EINVAL);
  Nodes a;
  a.add(0, I64MIN, 1.0);
  a.add(2, 5, 2.0);
  a.add(0, I64MIN, 3.0);  // equal stamps are in order
  a.add(0, 0, 4.0);
  a.add(2, I64MAX, 5.0);
  a.add(0, I64MAX, 6.0);
  EXPECT(check_nodes(ix, a, &err) == KMX_OK);
  ix.append_nodes((int64_t)a.robot.size(), a.robot.data(), a.stamp.data(), a.g.data());
  EXPECT(ix.n_nodes == 6 && ix.ids[0].size() == 4 && ix.ids[1].empty() && ix.ids[2].size() == 2);
  EXPECT(ix.last_stamp[0] == I64MAX && ix.last_stamp[1] == I64MIN && ix.last_stamp[2] == I64MAX);
  // backwards: against the robot's newest node, and inside one batch
  Nodes b;
  b.add(0, I64MAX - 1);
  EXPECT(check_nodes(ix, b, &err) == KMX_EINVAL);
  Nodes c;
  c.add(1, 10);
  c.add(1, 9);
  EXPECT(check_nodes(ix, c, &err) == KMX_EINVAL);
  Nodes d;
  d.add(1, 10);
  d.add(1, 10);
  EXPECT(check_nodes(ix, d, &err) == KMX_OK);
  // robot ids
  for (int32_t r : {-1, 3, INT32_MAX, INT32_MIN}) {
    Nodes e;
    e.add(r, I64MAX);
    EXPECT(check_nodes(ix, e, &err) == KMX_EINVAL);
  }
  // values that are not finite
  for (double bad : {std::nan(""), HUGE_VAL, -HUGE_VAL}) {
    Nodes e;
    e.add(1, 0);
    e.R[4] = bad;
    EXPECT(check_nodes(ix, e, &err) == KMX_EINVAL);
    Nodes f;
    f.add(1, 0);
    f.g[2] = bad;
    EXPECT(check_nodes(ix, f, &err) == KMX_EINVAL);
  }
  // a rejected batch changed nothing
  EXPECT(ix.n_nodes == 6 && ix.stamp.size() == 6 && ix.g.size() == 18);

  // the sorted layout: robot by robot, ids increasing inside
  std::vector<int32_t> off, sid;
  std::vector<int64_t> sst;
  std::vector<double> sg;
  ix.sorted_layout(&off, &sst, &sid, &sg);
  EXPECT(off.size() == 4 && off[0] == 0 && off[1] == 4 && off[2] == 4 && off[3] == 6);
  const int32_t want[6] = {0, 2, 3, 5, 1, 4};
  for (int p = 0; p < 6; ++p) {
    EXPECT(sid[p] == want[p]);
    EXPECT(sst[p] == a.stamp[want[p]]);
    EXPECT(sg[3 * p] == a.g[3 * want[p]] && sg[3 * p + 2] == a.g[3 * want[p] + 2]);
  }
  // windows at the int64 extremes and on the empty robot
  auto window = [&](int32_t r, int64_t s, int64_t w, int32_t* lo, int32_t* hi) {
    *lo = kmx::mesh_lower(sst.data(), off[r], off[r + 1], kmx::mesh_sat_sub(s, w));
    *hi = kmx::mesh_upper(sst.data(), off[r], off[r + 1], kmx::mesh_sat_add(s, w));
  };
  int32_t lo, hi;
  window(0, 0, I64MAX, &lo, &hi);
  EXPECT(lo == 2 && hi == 4);  // -I64MAX .. I64MAX: the two nodes at I64MIN are out
  window(0, -1, I64MAX, &lo, &hi);
  EXPECT(lo == 0 && hi == 3);  // I64MIN .. I64MAX - 1
  window(0, I64MIN, 0, &lo, &hi);
  EXPECT(lo == 0 && hi == 2);
  window(0, I64MAX, 0, &lo, &hi);
  EXPECT(lo == 3 && hi == 4);
  window(0, I64MAX, I64MAX, &lo, &hi);
  EXPECT(lo == 2 && hi == 4);
  window(1, 0, I64MAX, &lo, &hi);
  EXPECT(lo == 4 && hi == 4);  // the empty robot
  window(2, 4, 0, &lo, &hi);
  EXPECT(lo == hi);
  window(2, 4, 1, &lo, &hi);
  EXPECT(lo == 4 && hi == 5);
}

void test_vertex_checks() {
  std::string err;
  kmx::MeshNodeIndex ix;
  ix.init(2);
  EXPECT(ix.check_vertices(0, 0, nullptr, nullptr, nullptr, &err) == KMX_OK);
  EXPECT(ix.check_vertices(2, 0, nullptr, nullptr, nullptr, &err) == KMX_EINVAL);
  std::vector<int32_t> robot{0, 1, 1};
  std::vector<int64_t> stamp{I64MAX, I64MIN, 0};  // vertex stamps come in any order
  std::vector<float> xyz(9, 1.5f);
  EXPECT(ix.check_vertices(3, 0, robot.data(), stamp.data(), xyz.data(), &err) == KMX_OK);
  EXPECT(ix.check_vertices(3, (int64_t)INT32_MAX - 2, robot.data(), stamp.data(), xyz.data(), &err) == KMX_EINVAL);
  ix.count_vertices(3, robot.data());
  EXPECT(ix.n_vertices[0] == 1 && ix.n_vertices[1] == 2);
  robot[2] = 2;
  EXPECT(ix.check_vertices(3, 0, robot.data(), stamp.data(), xyz.data(), &err) == KMX_EINVAL);
  robot[2] = -1;
  EXPECT(ix.check_vertices(3, 0, robot.data(), stamp.data(), xyz.data(), &err) == KMX_EINVAL);
  robot[2] = 1;
  for (float bad : {std::nanf(""), HUGE_VALF, -HUGE_VALF}) {
    xyz[8] = bad;
    EXPECT(ix.check_vertices(3, 0, robot.data(), stamp.data(), xyz.data(), &err) == KMX_EINVAL);
  }
}

// random streams: the binary-search windows against a plain scan
void test_random_windows() {
  std::mt19937_64 rng(7);
  for (int trial = 0; trial < 200; ++trial) {
    const int R = 1 + (int)(rng() % 4);
    kmx::MeshNodeIndex ix;
    ix.init(R);
    std::vector<int64_t> cur((size_t)R);
    for (auto& c : cur) c = (rng() % 3 == 0) ? I64MIN : (int64_t)(rng() % 50);
    for (int batch = 0; batch < 3; ++batch) {
      Nodes n;
      const int cnt = (int)(rng() % 20);
      for (int i = 0; i < cnt; ++i) {
        const int32_t r = (int32_t)(rng() % R);
        const int64_t step = (int64_t)(rng() % 4);
        cur[r] = kmx::mesh_sat_add(cur[r], step);
        n.add(r, cur[r], (double)i);
      }
      std::string err;
      EXPECT(check_nodes(ix, n, &err) == KMX_OK);
      ix.append_nodes((int64_t)n.robot.size(), n.robot.data(), n.stamp.data(), n.g.data());
    }
    std::vector<int32_t> off, sid;
    std::vector<int64_t> sst;
    std::vector<double> sg;
    ix.sorted_layout(&off, &sst, &sid, &sg);
    for (int q = 0; q < 50; ++q) {
      const int32_t r = (int32_t)(rng() % R);
      const int64_t s = (rng() % 5 == 0) ? (rng() % 2 ? I64MIN : I64MAX) : (int64_t)(rng() % 120) - 10;
      const int64_t w = (rng() % 5 == 0) ? I64MAX : (int64_t)(rng() % 6);
      const int32_t lo = kmx::mesh_lower(sst.data(), off[r], off[r + 1], kmx::mesh_sat_sub(s, w));
      const int32_t hi = kmx::mesh_upper(sst.data(), off[r], off[r + 1], kmx::mesh_sat_add(s, w));
      for (int32_t p = off[r]; p < off[r + 1]; ++p) {
        // |s_j - s| <= w without overflow, in 128 bits
        const __int128 d = (__int128)sst[p] - (__int128)s;
        const bool in = (d < 0 ? -d : d) <= (__int128)w;
        EXPECT(in == (p >= lo && p < hi));
      }
      for (int32_t p = off[r]; p + 1 < off[r + 1]; ++p) EXPECT(sid[p] < sid[p + 1] && sst[p] <= sst[p + 1]);
    }
  }
}

}  // namespace

int main() {
  test_params();
  test_saturation();
  test_ranges();
  test_node_checks();
  test_vertex_checks();
  test_random_windows();
  if (g_fail) {
    std::fprintf(stderr, "mesh_check: %d failures\n", g_fail);
    return 1;
  }
  std::printf("mesh_check ok\n");
  return 0;
}
