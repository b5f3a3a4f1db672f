// pgo_check.cpp — pgo.hip's host code (pgo_host.h: the checks of
// kmx_pgo_set_graph and the plan it uploads: the public table, the incidence
// records in both widths, the tile and robot-group cut and the GNC /
// shared-weight lists) as a stand-alone program, built by `make pgo_check`
// with the host address and undefined-behaviour sanitizers. Every array is
// passed in a vector of exactly the stated size, so a read past one is a
// report. The expected values are worked out by hand in the comments. CPU only.
#include <climits>
#include <cstdio>
#include <string>
#include <vector>

#include "pgo_host.h"

namespace {

int g_fail = 0;

#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::fprintf(stderr, "pgo_check.cpp:%d: %s\n", __LINE__, #cond);  \
      ++g_fail;                                                         \
    }                                                                   \
  } while (0)

struct Rot {
  double m[9];
};
// rotation by `a` about axis 0 (x), 1 (y) or 2 (z); a half-turn is exact
Rot rot(int axis, double a, bool half_turn = false) {
  const double c = half_turn ? -1.0 : std::cos(a), s = half_turn ? 0.0 : std::sin(a);
  switch (axis) {
    case 0: return Rot{{1, 0, 0, 0, c, -s, 0, s, c}};
    case 1: return Rot{{c, 0, s, 0, 1, 0, -s, 0, c}};
    default: return Rot{{c, -s, 0, s, c, 0, 0, 0, 1}};
  }
}
const Rot IDENT = {{1, 0, 0, 0, 1, 0, 0, 0, 1}};
// about x by -acos(-0.45): trace 0.1 > 0, so Shepperd takes the w branch
// (w = 0.524 > 0) while the largest component is x = -0.852 < 0
const Rot NEG_LARGEST = rot(0, -std::acos(-0.45));

struct Team {
  std::vector<int32_t> n_poses;
  std::vector<uint8_t> local;
  std::vector<int32_t> r1, p1, r2, p2;
  std::vector<double> R, t, kappa, tau, weight;
  std::vector<uint8_t> fixed;

  void edge(int a, int i, int b, int j, const Rot& Re = IDENT, bool fix = false) {
    r1.push_back(a); p1.push_back(i); r2.push_back(b); p2.push_back(j);
    R.insert(R.end(), Re.m, Re.m + 9);
    const double e = (double)r1.size();
    for (int q = 0; q < 3; ++q) t.push_back(0.25 * q - e);
    kappa.push_back(2.0 + e);
    tau.push_back(3.0 + e);
    weight.push_back(0.5);
    fixed.push_back(fix ? 1 : 0);
  }
  void chain(int a, bool fix = true) {
    for (int p = 0; p + 1 < n_poses[a]; ++p) edge(a, p, a, p + 1, rot(2, 0.1 * (p + 1)), fix);
  }
  int plan(const kmx::PgoPlanIn& in, kmx::PgoPlan* out, std::string* err) const {
    // exact-size copies
    std::vector<int32_t> np(n_poses), a1(r1), b1(p1), a2(r2), b2(p2);
    std::vector<uint8_t> lo(local), fx(fixed);
    std::vector<double> r(R), tt(t), k(kappa), ta(tau), w(weight);
    return kmx::pgo_plan(in, (int)np.size(), np.data(), lo.data(), (int64_t)a1.size(), a1.data(), b1.data(),
                         a2.data(), b2.data(), r.data(), tt.data(), k.data(), ta.data(), w.data(), fx.data(), out, err);
  }
};

kmx::PgoPlanIn params(int r = 3, int tile_incidences = 0, int groups_req = 2) {
  kmx::PgoPlanIn in;
  in.r = r;
  in.tile_incidences = tile_incidences;
  in.groups_req = groups_req;
  return in;
}

kmx::PgoPlan must_plan(const Team& g, const kmx::PgoPlanIn& in, const char* name) {
  kmx::PgoPlan out;
  std::string err;
  const int rc = g.plan(in, &out, &err);
  if (rc != KMX_OK) {
    std::fprintf(stderr, "%s: expected a plan, got %d (%s)\n", name, rc, err.c_str());
    ++g_fail;
  }
  return out;
}

void expect_reject(const Team& g, int code, const char* what, const char* name) {
  kmx::PgoPlan out;
  out.nloc = -7;  // a rejected graph must leave *out alone
  out.rec.assign(3, 1.5);
  std::string err;
  const int rc = g.plan(params(), &out, &err);
  if (rc != code || err.find(what) == std::string::npos || out.nloc != -7 || out.rec != std::vector<double>(3, 1.5) ||
      !out.tile.empty() || !out.local_of.empty()) {
    std::fprintf(stderr, "%s: expected %d (%s), got %d (%s)\n", name, code, what, rc, err.c_str());
    ++g_fail;
  }
}

Team two_robots() {
  Team g;
  g.n_poses = {3, 2};
  g.local = {1, 1};
  g.chain(0);
  g.chain(1);
  return g;
}

void check_rejections() {
  { Team g = two_robots(); g.edge(0, 0, 5, 0); expect_reject(g, KMX_EINVAL, "edge robot id out of range", "robot id"); }
  { Team g = two_robots(); g.edge(-1, 0, 1, 0); expect_reject(g, KMX_EINVAL, "edge robot id out of range", "robot id < 0"); }
  { Team g = two_robots(); g.edge(0, 0, 1, 2); expect_reject(g, KMX_EINVAL, "edge pose id out of range", "pose id"); }
  { Team g = two_robots(); g.edge(1, 1, 1, 1); expect_reject(g, KMX_EINVAL, "self-loop edge", "self-loop"); }
  { Team g = two_robots(); g.n_poses[1] = -1; g.local[1] = 0; expect_reject(g, KMX_EINVAL, "negative pose count", "negative count"); }
  { Team g = two_robots(); g.local = {0, 0}; expect_reject(g, KMX_EINVAL, "no local robot", "no local robot"); }
  {
    Team g;
    g.n_poses.assign(1025, 1);
    g.local.assign(1025, 1);
    expect_reject(g, KMX_EUNSUP, "at most 1024 local robots per handle", "1025 local robots");
  }
  {
    // slots (0,0) (1,0) (2,0): the local robots 0 and 2 own slots 0 and 2
    Team g;
    g.n_poses = {2, 2, 2};
    g.local = {1, 0, 1};
    g.edge(0, 0, 1, 0);
    g.edge(1, 0, 2, 0);
    expect_reject(g, KMX_EUNSUP, "local robots must own a contiguous range of the public table", "non-contiguous");
  }
  {
    Team g;
    g.n_poses = {0, 4, 0};
    g.local = {1, 0, 1};
    g.edge(1, 0, 1, 1);
    expect_reject(g, KMX_EINVAL, "no local poses", "no local poses");
  }
  {
    // the local pose total does not fit int32: refused before anything is sized by it
    Team g;
    g.n_poses = {INT32_MAX, INT32_MAX};
    g.local = {1, 1};
    expect_reject(g, KMX_EINVAL, "local pose count does not fit int32", "pose total overflow");
  }
}

// Robots 0 (3 poses) and 1 (2 poses) local, robot 2 (2 poses) foreign:
//   e0 (0,0)->(0,1)  e1 (0,1)->(0,2)  e2 (1,0)->(1,1)  e3 (2,0)->(2,1)   odometry, fixed
//   e4 (0,2)->(1,0)  shared between the two local robots
//   e5 (2,1)->(0,1)  shared, foreign tail
//   e6 (0,0)->(0,2)  private loop closure
// The rotations go through Shepperd's four branches, a negative largest
// component and a generic one.
Team small_team() {
  Team g;
  g.n_poses = {3, 2, 2};
  g.local = {1, 1, 0};
  g.edge(0, 0, 0, 1, IDENT, true);
  g.edge(0, 1, 0, 2, rot(0, 0, true), true);
  g.edge(1, 0, 1, 1, rot(1, 0, true), true);
  g.edge(2, 0, 2, 1, rot(2, 0.7), true);
  g.edge(0, 2, 1, 0, rot(2, 0, true));
  g.edge(2, 1, 0, 1, NEG_LARGEST);
  g.edge(0, 0, 0, 2, rot(2, 0.3));
  return g;
}

struct RecAt {
  int pos, k, tail, other;
};

// Local poses: (0,0) (0,1) (0,2) (1,0) (1,1) = 0..4. Public keys (0,1) (0,2)
// (1,0) (2,1) = slots 0..3, of which 0..2 are owned. Local edges e0 e1 e2 e4
// e5 e6 = k 0..5. Degrees 2 3 3 2 1.
void check_small(bool full) {
  Team g = small_team();
  if (full)
    for (int i = 0; i < 9; ++i) g.R[9 * 4 + i] *= 1.0 + 1e-9;  // e4 is no rotation to 1e-12
  const kmx::PgoPlan p = must_plan(g, params(), full ? "small (full records)" : "small");
  if (p.nloc == 0) return;
  CHECK(p.local_of == (std::vector<int>{0, 1, -1}));
  CHECK(p.robots == (std::vector<int>{0, 1}));
  CHECK(p.loff == (std::vector<int>{0, 3}));
  CHECK(p.nrob == (std::vector<int>{3, 2}));
  CHECK(p.nloc == 5);
  const auto key = [](int64_t rb, uint32_t pp) { return (rb << 32) | pp; };
  CHECK(p.pub_key == (std::vector<int64_t>{key(0, 1), key(0, 2), key(1, 0), key(2, 1)}));
  CHECK(p.npub == 4 && p.first_owned == 0 && p.n_owned == 3);
  CHECK(p.pub_src == (std::vector<int>{1, 2, 3, -1}));
  CHECK(p.own_src == (std::vector<int>{1, 2, 3}));
  CHECK(p.pose_slot == (std::vector<int>{-1, 0, 1, 2, -1}));
  CHECK(p.loc_edge_gid == (std::vector<int64_t>{0, 1, 2, 4, 5, 6}));
  CHECK(p.mloc == 6);
  CHECK(p.m_robot == (std::vector<long long>{5, 2}));  // e4 once for each of its robots
  CHECK(p.inc_ptr == (std::vector<int>{0, 2, 5, 8, 10, 11}));
  CHECK(p.ninc == 11);
  CHECK(p.rw == (full ? 16 : 10));
  // a pose's records in increasing edge id; a shared edge's other endpoint is
  // -1 - slot, also between two local robots (e4)
  const RecAt want[11] = {{0, 0, 1, 1},  {1, 5, 1, 2},  {2, 0, 0, 0},  {3, 1, 1, 2}, {4, 4, 0, -4}, {5, 1, 0, 1},
                          {6, 3, 1, -3}, {7, 5, 0, 0},  {8, 2, 1, 4},  {9, 3, 0, -2}, {10, 2, 0, 3}};
  const int GS = kmx::rec_gs(p.rw);
  CHECK(GS == (full ? 16 : 8));
  CHECK(p.rec.size() == (size_t)12 * GS);
  CHECK(p.rec_o.size() == (full ? (size_t)1 : (size_t)12));
  if (p.rec.size() != (size_t)12 * GS || p.rec_o.size() != (full ? (size_t)1 : (size_t)12)) return;
  for (const RecAt& w : want) {
    const double* c = &p.rec[(size_t)w.pos * GS];
    const int64_t e = p.loc_edge_gid[w.k];
    const double wk = g.weight[e] * g.kappa[e], wt = g.weight[e] * g.tau[e];
    if (!full) {
      const unsigned word = (unsigned)p.rec_o[w.pos];
      CHECK(((int)(word << 3) >> 3) == w.other);
      double q[4], Rq[9];
      kmx::quat_unpack(c, (int)(word >> 29), q);
      kmx::quat_to_rot(q, Rq);
      for (int i = 0; i < 9; ++i) CHECK(std::fabs(Rq[i] - g.R[9 * e + i]) <= 1e-12);
      for (int i = 0; i < 3; ++i) CHECK(c[3 + i] == g.t[3 * e + i]);
      CHECK(c[6] == wk && std::fabs(c[7]) == wt);
      CHECK(std::signbit(c[7]) == (w.tail != 0));  // the tail flag: the sign of w tau
    } else {
      for (int i = 0; i < 9; ++i) CHECK(c[i] == g.R[9 * e + i]);
      for (int i = 0; i < 3; ++i) CHECK(c[9 + i] == g.t[3 * e + i]);
      CHECK(c[12] == wk && c[13] == wt);
      uint64_t bits;
      std::memcpy(&bits, &c[14], 8);
      CHECK((int)(uint32_t)bits == w.other);
      CHECK((int)((bits >> 32) & 0x7fffffffu) == w.k);
      CHECK((bits >> 63) == (uint64_t)w.tail);  // the tail flag: bit 63 of the code word
      CHECK(c[15] == 0.0);
    }
  }
  for (int i = 0; i < GS; ++i) CHECK(p.rec[(size_t)11 * GS + i] == 0.0);  // the pad record
  const int eipos[6][2] = {{0, 2}, {3, 5}, {8, 10}, {6, 9}, {-1, 4}, {1, 7}};
  CHECK(p.eipos.size() == 6);
  for (size_t k = 0; k < 6 && k < p.eipos.size(); ++k) CHECK(p.eipos[k].x == eipos[k][0] && p.eipos[k].y == eipos[k][1]);
  for (int k = 0; k < 6; ++k) {
    const int64_t e = p.loc_edge_gid[k];
    CHECK(p.ek[k] == g.kappa[e] && p.et[k] == g.tau[e] && p.ew[k] == g.weight[e]);
  }
  // lists: the fixed odometry is absent; e4 (2, 3) both local, e5 (-1 - 3, 1), e6 (0, 2)
  CHECK(p.gnc_edge == (std::vector<int>{3, 4, 5}));
  const int ends[3][2] = {{2, 3}, {-4, 1}, {0, 2}};
  CHECK(p.gnc_ends.size() == 3);
  for (size_t i = 0; i < 3 && i < p.gnc_ends.size(); ++i) CHECK(p.gnc_ends[i].x == ends[i][0] && p.gnc_ends[i].y == ends[i][1]);
  CHECK(p.nshared == 2);
  CHECK(p.sh_edge == (std::vector<int>{3, 4}) && p.sh_idx == (std::vector<int>{0, 1}));
  CHECK(p.osh_edge == (std::vector<int>{3, 4}) && p.osh_idx == (std::vector<int>{0, 1}));  // lower robot 0 is local
}

// small_team plus e7 (1,1)->(2,0), seen by a handle that holds robot 1 only:
// poses (1,0) (1,1) = 0, 1; slots (0,1) (0,2) (1,0) (1,1) (2,0) (2,1) = 0..5;
// local edges e2 e4 e7 = k 0..2; shared edges e4 e5 e7 = indices 0..2.
void check_lists_one_robot() {
  Team g = small_team();
  g.edge(1, 1, 2, 0, rot(1, 0.2));
  g.local = {0, 1, 0};
  const kmx::PgoPlan p = must_plan(g, params(), "lists");
  if (p.nloc == 0) return;
  CHECK(p.nloc == 2 && p.npub == 6 && p.first_owned == 2 && p.n_owned == 2);
  CHECK(p.own_src == (std::vector<int>{0, 1}));
  CHECK(p.loc_edge_gid == (std::vector<int64_t>{2, 4, 7}));
  CHECK(p.gnc_edge == (std::vector<int>{1, 2}));  // e2 is fixed
  CHECK(p.gnc_ends.size() == 2);
  if (p.gnc_ends.size() == 2) {
    CHECK(p.gnc_ends[0].x == -2 && p.gnc_ends[0].y == 0);  // e4: foreign (0,2) = slot 1, local (1,0)
    CHECK(p.gnc_ends[1].x == 1 && p.gnc_ends[1].y == -5);  // e7: local (1,1), foreign (2,0) = slot 4
  }
  CHECK(p.nshared == 3);  // e5 is counted though this handle does not hold it
  CHECK(p.sh_edge == (std::vector<int>{1, 2}) && p.sh_idx == (std::vector<int>{0, 2}));
  CHECK(p.osh_edge == (std::vector<int>{2}) && p.osh_idx == (std::vector<int>{2}));  // e4's lower robot 0 is foreign
  CHECK(p.m_robot == (std::vector<long long>{3}));
}

void check_quaternions() {
  const struct {
    Rot R;
    int big;
  } cases[] = {{IDENT, 0}, {rot(0, 0, true), 1}, {rot(1, 0, true), 2}, {rot(2, 0, true), 3}, {NEG_LARGEST, 1},
               {rot(1, 2.5), 2}};
  for (const auto& c : cases) {
    double q[4], q3[3], qr[4], Rq[9];
    kmx::rot_to_quat(c.R.m, q);
    const int big = kmx::quat_pack(q, q3);
    CHECK(big == c.big);
    const double sg = q[big] < 0.0 ? -1.0 : 1.0;
    for (int i = 0, j = 0; i < 4; ++i)
      if (i != big) CHECK(q3[j++] == sg * q[i]);
    kmx::quat_unpack(q3, big, qr);
    kmx::quat_to_rot(qr, Rq);
    for (int i = 0; i < 9; ++i) CHECK(std::fabs(Rq[i] - c.R.m[i]) <= 1e-12);
  }
  {  // the largest component is negative: the three stored ones get the flipped sign
    double q[4], q3[3];
    kmx::rot_to_quat(NEG_LARGEST.m, q);
    CHECK(q[1] < -0.8 && q[0] > 0.5);
    CHECK(kmx::quat_pack(q, q3) == 1);
    CHECK(q3[0] == -q[0] && q3[0] < -0.5);
  }
}

// A chain of 40 poses whose pose 20 has degree 30 (robot 0) and a chain of 7
// (robot 1), both local.
Team hub_team() {
  Team g;
  g.n_poses = {40, 7};
  g.local = {1, 1};
  g.chain(0);
  for (int j = 0; j < 28; ++j) g.edge(0, 20, 0, j < 14 ? j : j + 9, rot(0, 0.05 * (j + 1)));
  g.chain(1);
  return g;
}

// The tiles against inc_ptr and the cap. `tilecap` is the limit in force:
// tile_incidences (at least 16), or the automatic one.
void check_cut(const kmx::PgoPlan& p, int r, int64_t tilecap, const char* name) {
  auto fail = [&](const char* m) {
    std::fprintf(stderr, "%s (r = %d): cut: %s\n", name, r, m);
    ++g_fail;
  };
  const int L = (int)p.robots.size(), TP = kmx::WAVES * (64 / r);
  if (p.rt0.size() != (size_t)L + 1 || p.rt0[0] != 0 || (size_t)p.rt0[L] != p.tile.size()) return fail("rt0");
  for (int l = 0; l < L; ++l) {
    const int n = p.nrob[l], base = p.loff[l];
    const int64_t inc_l = p.inc_ptr[base + n] - p.inc_ptr[base];
    const int64_t full = std::max(1, (n + TP - 1) / TP);
    const int64_t cap = std::min(tilecap, std::max<int64_t>(1, (inc_l * 21 / 20 + full - 1) / full));
    int at = base;
    for (int ti = p.rt0[l]; ti < p.rt0[l + 1]; ++ti) {
      const kmx::TileDesc& td = p.tile[ti];
      const int np = td.np_n & 0xff, ninc = (int)((unsigned)td.np_n >> 8);
      if (td.robot != l || td.p0 != at) return fail("the tiles do not partition a robot's poses in order");
      if (np < 1 || np > TP || at + np > base + n) return fail("tile size");
      if (td.k0 != p.inc_ptr[at] || ninc != p.inc_ptr[at + np] - p.inc_ptr[at]) return fail("k0 / np_n against inc_ptr");
      if (td.rt0 != p.rt0[l] || td.rt1 != p.rt0[l + 1] || td.pad0 != 0 || td.pad1 != 0) return fail("rt0 / rt1");
      if (np > 1 && ninc > cap) return fail("a tile of several poses is past the cap");
      if (at + np < base + n && np < TP && ninc + (p.inc_ptr[at + np + 1] - p.inc_ptr[at + np]) <= cap)
        return fail("a tile closed though the next pose fits");
      at += np;
    }
    if (at != base + n) return fail("a robot's tiles do not cover it");
  }
}

void check_tiles() {
  const Team g = hub_team();
  for (int r : {3, 5, 8}) {
    const int TP = kmx::WAVES * (64 / r);
    CHECK(kmx::tile_poses(r) == TP);
    const kmx::PgoPlan p16 = must_plan(g, params(r, 16), "hub, 16 incidences per tile");
    if (p16.nloc == 0) return;
    CHECK(p16.inc_ptr[21] - p16.inc_ptr[20] == 30);
    check_cut(p16, r, 16, "hub, cap 16");
    bool alone = false;  // the hub's degree alone is past the cap: a tile of its own
    for (const kmx::TileDesc& td : p16.tile) alone = alone || (td.p0 == 20 && td.np_n == (1 | (30 << 8)));
    CHECK(alone);
    const kmx::PgoPlan p1 = must_plan(g, params(r, 1), "hub, tile_incidences 1");  // acts as 16
    CHECK(p1.tile.size() == p16.tile.size() && p1.rt0 == p16.rt0);
    for (size_t i = 0; i < p1.tile.size() && i < p16.tile.size(); ++i)
      CHECK(std::memcmp(&p1.tile[i], &p16.tile[i], sizeof(kmx::TileDesc)) == 0);
    // automatic: two gather chunks at most, not below 180 on a small problem
    const kmx::PgoPlan pa = must_plan(g, params(r, 0), "hub, automatic cap");
    check_cut(pa, r, std::min<int64_t>(2 * (int64_t)TP * r, 180), "hub, automatic cap");
  }
}

// Local robots 0..4 of 10, 0, 30, 0 and 20 poses (chains: 18, 58 and 38
// incidences): the groups against a naive restatement of the rule.
void check_groups() {
  Team g;
  g.n_poses = {10, 0, 30, 0, 20};
  g.local = {1, 1, 1, 1, 1};
  g.chain(0);
  g.chain(2);
  g.chain(4);
  const int L = 5;
  for (int req : {1, 2, 4}) {
    const kmx::PgoPlan p = must_plan(g, params(3, 0, req), "groups");
    if (p.nloc == 0) return;
    std::vector<int64_t> pre(L + 1, 0);
    std::vector<int> tiled(L + 1, 0);
    for (int l = 0; l < L; ++l) {
      pre[l + 1] = pre[l] + (p.inc_ptr[p.loff[l] + p.nrob[l]] - p.inc_ptr[p.loff[l]]);
      tiled[l + 1] = tiled[l] + (p.rt0[l + 1] > p.rt0[l] ? 1 : 0);
    }
    CHECK(pre[L] == 114 && tiled[L] == 3);
    const int G = std::min(req, 3);
    CHECK((int)p.grp.size() == G);
    if ((int)p.grp.size() != G) return;
    int at = 0;
    for (int gi = 0; gi < G; ++gi) {
      const kmx::PgoGroupCut& q = p.grp[gi];
      CHECK(q.l0 == at && q.l1 > q.l0);
      CHECK(tiled[q.l1] > tiled[q.l0] && q.nt > 0);  // every group holds a robot with tiles
      CHECK(q.t0 == p.rt0[q.l0] && q.nt == p.rt0[q.l1] - p.rt0[q.l0]);
      if (gi > 0) {
        // the first boundary c past the previous one that leaves a tiled robot
        // behind it and G - gi of them ahead, nearest to gi / G of the total
        int best = -1;
        for (int c = p.grp[gi - 1].l0 + 1; c < L; ++c) {
          if (tiled[c] == tiled[p.grp[gi - 1].l0] || tiled[L] - tiled[c] < G - gi) continue;
          if (best < 0 || std::llabs(G * pre[c] - gi * pre[L]) < std::llabs(G * pre[best] - gi * pre[L])) best = c;
        }
        CHECK(q.l0 == best);
      }
      at = q.l1;
    }
    CHECK(at == L);
  }
  // by hand: two groups cut at robot 3 (prefix 76 of 114, nearest to 57 among
  // 18, 18, 76, 76: |2 * 76 - 114| = 38 < |2 * 18 - 114| = 78, the first of the tie)
  const kmx::PgoPlan p2 = must_plan(g, params(3, 0, 2), "groups by hand");
  CHECK(p2.grp.size() == 2 && p2.grp[1].l0 == 3);
  // three groups: robots [0, 1) [1, 3) [3, 5)
  const kmx::PgoPlan p4 = must_plan(g, params(3, 0, 4), "groups by hand");
  CHECK(p4.grp.size() == 3 && p4.grp[1].l0 == 1 && p4.grp[2].l0 == 3);
}

void check_choices() {
  const Team g = two_robots();
  kmx::PgoPlanIn in = params();
  kmx::PgoPlan p = must_plan(g, in, "choices");
  CHECK(p.rm == kmx::RM_CONSUMER && p.early_stop == 1 && p.grm == kmx::RM_CONSUMER);  // a small problem
  in.rm_forced = kmx::RM_LAUNCH;
  in.decide_forced = 0;
  in.grm_forced = kmx::RM_LAUNCH;
  p = must_plan(g, in, "forced choices");
  CHECK(p.rm == kmx::RM_LAUNCH && p.early_stop == 0 && p.grm == kmx::RM_LAUNCH);
  in.onesync = true;  // its decisions are taken by every workgroup
  p = must_plan(g, in, "one-sync");
  CHECK(p.rm == kmx::RM_CONSUMER);
}

void check_no_edges() {
  Team g;
  g.n_poses = {3};
  g.local = {1};
  const kmx::PgoPlan p = must_plan(g, params(), "m = 0");
  if (p.nloc == 0) return;
  CHECK(p.nloc == 3 && p.mloc == 0 && p.ninc == 0 && p.npub == 0 && p.n_owned == 0 && p.nshared == 0);
  CHECK(p.inc_ptr == (std::vector<int>{0, 0, 0, 0}));
  CHECK(p.rw == 10 && p.rec == std::vector<double>(8, 0.0) && p.rec_o == std::vector<int>(1, 0));  // one zero pad record
  CHECK(p.gnc_edge.empty() && p.gnc_ends.empty() && p.sh_edge.empty() && p.sh_idx.empty() && p.osh_edge.empty() &&
        p.osh_idx.empty() && p.loc_edge_gid.empty());
  CHECK(p.eipos.size() == 1 && p.eipos[0].x == -1 && p.eipos[0].y == -1);
  CHECK(p.tile.size() == 1 && p.tile[0].p0 == 0 && p.tile[0].np_n == 3 && p.tile[0].k0 == 0);
  CHECK(p.grp.size() == 1 && p.grp[0].l0 == 0 && p.grp[0].l1 == 1 && p.grp[0].nt == 1);
}

}  // namespace

int main() {
  static_assert(sizeof(kmx::TileDesc) == 32 && alignof(kmx::TileDesc) == 16, "TileDesc is one 32-B load");
  static_assert(sizeof(kmx::PgoInt2) == 8, "PgoInt2 is the device's int2");
  check_rejections();
  check_small(false);
  check_small(true);
  check_lists_one_robot();
  check_quaternions();
  check_tiles();
  check_groups();
  check_choices();
  check_no_edges();
  if (g_fail) {
    std::fprintf(stderr, "pgo_check: %d failure(s)\n", g_fail);
    return 1;
  }
  std::printf("pgo_check ok\n");
  return 0;
}
