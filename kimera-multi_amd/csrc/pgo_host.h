// pgo_host.h — host-side half of pgo.hip that needs no device: everything
// kmx_pgo_set_graph works out before its first device call. pgo_plan checks
// the team and the edges and builds the team-wide public table, the local
// edges and their incidence records (compact quaternion or full), the tile and
// robot-group cut and the GNC / shared-weight lists; set_graph only uploads the
// plan. Plain C++, so `make pgo_check` can build it with the host sanitizers
// (pgo_check.cpp).
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "kmx_abi.h"

namespace kmx {

constexpr int WAVES = 4;  // waves per tile workgroup
// A tile holds at most TP = W * (64 / R) poses (W waves; a pose's R rows of 4
// sit in R adjacent lanes, 64 / R pose groups per wave).
constexpr int tile_poses(int r, int w = WAVES) { return w * (64 / r); }
constexpr int TILES_TARGET = 736;  // tile count the cut of small problems aims at (pgo_plan)

// How a robot's tile partials are summed (pgo.hip, "per-robot reductions"): by
// a k_reduce launch, or by every workgroup of the consuming kernel.
enum RedMode { RM_LAUNCH = 0, RM_CONSUMER = 2 };
// reduction mode: set per graph unless KMX_RED forces one (0 launch, 2
// consumer). Measured at the end of round 2
// (profiles/r02/small_round/16_*): the consumer form (no reduction launch,
// the stop decision before the gather) wins per round at 25k poses (244 vs
// 280 us), 37.5k (318 vs 357), 62.5k (530 vs 543) and 75k (583 vs 591), ties
// at 50k and 87.5k, and loses at 100k (773 vs 731-738: two and a bit
// generations of workgroups, each waiting for its robot's sums). The same
// bound decides whether the consumer-form k_hess takes its stop decision
// before the gather (small problems) or after it.
constexpr int RM_CONSUMER_MAX_POSES = 80000;
// The grouped round's reduction form (kmx_pgo::grm).
// On one chain the consumer form only ties at 100k poses (above); on two
// chains it drops 22 of a chain's 45 launches and the other group's
// workgroups fill part of the waits for the robot sums: configs[3]
// 0.603-0.619 ms per round against 0.622-0.633 for the launched form
// (profiles/r08/group_consumer/). Every workgroup of
// the consumer kernels reads all tile partials of its robot, so its cost
// grows with the robot's tile count: with 8 robots in 2 groups it wins 3-5 %
// at 275-288 tiles per robot (12.5k poses), 1-2 % at 310-324 and ~1 % at
// 354-368, loses 1.4 % at 400-421, 7 % at ~500 and 20 % at ~2600 (the
// 1M-pose config). It is the default while no local robot has more than
// GROUP_CONSUMER_MAX_TILES tiles.
constexpr int GROUP_CONSUMER_MAX_TILES = 384;

// doubles per incidence record in HBM (Rec<RW>::GS): 8 for the compact record
// (RW = 10), 16 for the full one (RW = 16)
constexpr int rec_gs(int rw) { return rw == 10 ? 8 : 16; }

// One tile's description, read by a single 32-B scalar load at the start of
// every tile kernel: its robot, its first pose, its incidence range start
// inc_ptr[p0] and, packed, its pose count np (< 256) and incidence count
// n = inc_ptr[p0 + np] - inc_ptr[p0] (np | n << 8), so the record loads do not
// wait for an inc_ptr lookup; and its robot's tile range, so the consumer
// kernels' robot sums do not wait for an rtile0 lookup.
struct alignas(16) TileDesc {
  int robot, p0, k0, np_n;
  int rt0, rt1;  // the robot's tile range: the consumer kernels' robot sums start from it
  int pad0, pad1;
};

// Unit quaternion (w, x, y, z) of a rotation matrix (row-major), by the
// largest of the four diagonal combinations (Shepperd), and back.
inline void rot_to_quat(const double* R, double* q) {
  const double tr = R[0] + R[4] + R[8];
  double w, x, y, z;
  if (tr > 0.0) {
    const double s = 2.0 * std::sqrt(tr + 1.0);
    w = 0.25 * s; x = (R[7] - R[5]) / s; y = (R[2] - R[6]) / s; z = (R[3] - R[1]) / s;
  } else if (R[0] > R[4] && R[0] > R[8]) {
    const double s = 2.0 * std::sqrt(1.0 + R[0] - R[4] - R[8]);
    w = (R[7] - R[5]) / s; x = 0.25 * s; y = (R[1] + R[3]) / s; z = (R[2] + R[6]) / s;
  } else if (R[4] > R[8]) {
    const double s = 2.0 * std::sqrt(1.0 + R[4] - R[0] - R[8]);
    w = (R[2] - R[6]) / s; x = (R[1] + R[3]) / s; y = 0.25 * s; z = (R[5] + R[7]) / s;
  } else {
    const double s = 2.0 * std::sqrt(1.0 + R[8] - R[0] - R[4]);
    w = (R[3] - R[1]) / s; x = (R[2] + R[6]) / s; y = (R[5] + R[7]) / s; z = 0.25 * s;
  }
  const double n = std::sqrt(w * w + x * x + y * y + z * z);
  q[0] = w / n; q[1] = x / n; q[2] = y / n; q[3] = z / n;
}
// Rec<10>'s three stored components: all but the largest (made >= 0 by
// negating the quaternion, which leaves R unchanged), whose index goes to
// rec_o's bits 29-31; and the device's rebuild of the fourth (Rec<10>::load).
inline int quat_pack(const double* q, double* q3) {
  int big = 0;
  for (int i = 1; i < 4; ++i)
    if (std::fabs(q[i]) > std::fabs(q[big])) big = i;
  const double sg = q[big] < 0.0 ? -1.0 : 1.0;
  for (int i = 0, j = 0; i < 4; ++i)
    if (i != big) q3[j++] = sg * q[i];
  return big;
}
inline void quat_unpack(const double* q3, int big, double* q) {
  const double ql = std::sqrt(1.0 - (q3[0] * q3[0] + q3[1] * q3[1] + q3[2] * q3[2]));
  for (int i = 0, j = 0; i < 4; ++i) q[i] = i == big ? ql : q3[j++];
}
// the device's Rec<10>::edge expressions
inline void quat_to_rot(const double* q, double* R) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z;
  const double wx = w * x, wy = w * y, wz = w * z;
  R[0] = 1.0 - 2.0 * (yy + zz); R[1] = 2.0 * (xy - wz); R[2] = 2.0 * (xz + wy);
  R[3] = 2.0 * (xy + wz); R[4] = 1.0 - 2.0 * (xx + zz); R[5] = 2.0 * (yz - wx);
  R[6] = 2.0 * (xz - wy); R[7] = 2.0 * (yz + wx); R[8] = 1.0 - 2.0 * (xx + yy);
}

// What the plan depends on besides the graph: the handle's parameters and its
// forced (>= 0) or automatic (-1) choices.
struct PgoPlanIn {
  int r = 3;                // lifted rank (3..8)
  int tile_incidences = 0;  // kmx_pgo_params.tile_incidences (0: automatic)
  int groups_req = 2;       // robot groups asked for (1, 2 or 4)
  int rm_forced = -1, decide_forced = -1, grm_forced = -1;
  bool onesync = false;  // the one-sync tCG form: its decisions are taken by every workgroup
};

struct PgoInt2 {  // the device's int2
  int32_t x, y;
};
struct PgoGroupCut {
  int l0, l1;  // local robots [l0, l1)
  int t0, nt;  // their tiles [t0, t0 + nt)
};

// Everything kmx_pgo_set_graph computes before its first device allocation.
// Vectors that are uploaded hold at least one element.
struct PgoPlan {
  // team
  std::vector<int> local_of;  // robot -> local index or -1
  std::vector<int> robots;    // local index -> robot
  std::vector<int> loff;      // local robot -> first local pose
  std::vector<int> nrob;      // local robot -> pose count
  int nloc = 0;
  // public table (team-wide, so every handle agrees on slot ids)
  std::vector<int64_t> pub_key;  // sorted (robot<<32 | pose)
  int64_t npub = 0, first_owned = 0, n_owned = 0;
  std::vector<int> pub_src;    // slot -> local pose (-1 if not local)
  std::vector<int> own_src;    // owned slot k -> local pose (index first_owned + k)
  std::vector<int> pose_slot;  // local pose -> owned slot or -1
  // local edges and their incidence records
  std::vector<int64_t> loc_edge_gid;
  int mloc = 0;
  std::vector<long long> m_robot;  // edges per local robot (a shared edge once per robot)
  std::vector<double> ek, et, ew;  // kappa, tau, weight per local edge
  int rw = 10;                     // record width in doubles (10 compact quaternion / 16 full)
  std::vector<int> inc_ptr;        // [nloc + 1]
  int ninc = 0;
  std::vector<double> rec;     // [ninc + 1][rec_gs(rw)], the last a zero pad record
  std::vector<int> rec_o;      // compact: [ninc + 1] other endpoint | dropped component << 29
  std::vector<PgoInt2> eipos;  // local edge -> its records at the tail (x) and the head (y), -1: not local
  // GNC and shared-weight lists
  std::vector<int> gnc_edge;
  std::vector<PgoInt2> gnc_ends;  // a local pose, or -1 - slot
  std::vector<int> sh_edge, sh_idx, osh_edge, osh_idx;
  int64_t nshared = 0;
  // cut
  std::vector<TileDesc> tile;
  std::vector<int> rt0;  // [L + 1] first tile of each local robot
  std::vector<PgoGroupCut> grp;
  int rm = RM_LAUNCH, early_stop = 1, grm = RM_CONSUMER;
};

// Checks the graph of kmx_pgo_set_graph (its arrays, already checked for null
// and 0 <= m < 2^31 - 1) and, when it passes, builds *out (untouched on
// failure). KMX_OK, or the error's code with *err set.
inline int pgo_plan(const PgoPlanIn& in, int n_robots, const int32_t* n_poses, const uint8_t* local, int64_t m,
                    const int32_t* r1, const int32_t* p1, const int32_t* r2, const int32_t* p2, const double* R,
                    const double* t, const double* kappa, const double* tau, const double* weight,
                    const uint8_t* fixed_weight, PgoPlan* out, std::string* err) {
#define KMX_PLAN_CHECK(cond, code, msg) \
  do {                                  \
    if (!(cond)) {                      \
      if (err) *err = (msg);            \
      return (code);                    \
    }                                   \
  } while (0)
  KMX_PLAN_CHECK(out, KMX_EINVAL, "null argument");
  PgoPlan g;
  const int r = in.r;
  g.local_of.assign(n_robots, -1);
  int64_t nloc64 = 0;
  for (int a = 0; a < n_robots; ++a) {
    KMX_PLAN_CHECK(n_poses[a] >= 0, KMX_EINVAL, "negative pose count");
    if (local[a]) {
      g.local_of[a] = (int)g.robots.size();
      g.robots.push_back(a);
      g.loff.push_back((int)nloc64);
      nloc64 += n_poses[a];
      KMX_PLAN_CHECK(nloc64 < INT_MAX, KMX_EINVAL, "local pose count does not fit int32");
    }
  }
  const int nloc = g.nloc = (int)nloc64;
  g.rm = in.rm_forced >= 0 ? in.rm_forced : (nloc <= RM_CONSUMER_MAX_POSES ? RM_CONSUMER : RM_LAUNCH);
  if (in.onesync) g.rm = RM_CONSUMER;  // its decisions are taken by every workgroup
  // decide before the gather on small problems
  g.early_stop = in.decide_forced >= 0 ? in.decide_forced : (nloc <= RM_CONSUMER_MAX_POSES ? 1 : 0);
  const int L = (int)g.robots.size();
  KMX_PLAN_CHECK(L > 0, KMX_EINVAL, "no local robot");
  KMX_PLAN_CHECK(L <= 1024, KMX_EUNSUP, "at most 1024 local robots per handle");
  // validate + public table (team-wide, so every handle agrees on slot ids)
  std::vector<int64_t> keys;
  for (int64_t e = 0; e < m; ++e) {
    KMX_PLAN_CHECK(r1[e] >= 0 && r1[e] < n_robots && r2[e] >= 0 && r2[e] < n_robots, KMX_EINVAL,
                   "edge robot id out of range");
    KMX_PLAN_CHECK(p1[e] >= 0 && p1[e] < n_poses[r1[e]] && p2[e] >= 0 && p2[e] < n_poses[r2[e]], KMX_EINVAL,
                   "edge pose id out of range");
    KMX_PLAN_CHECK(!(r1[e] == r2[e] && p1[e] == p2[e]), KMX_EINVAL, "self-loop edge");
    if (r1[e] != r2[e]) {
      keys.push_back(((int64_t)r1[e] << 32) | (uint32_t)p1[e]);
      keys.push_back(((int64_t)r2[e] << 32) | (uint32_t)p2[e]);
    }
  }
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  g.pub_key = keys;
  g.npub = (int64_t)keys.size();
  KMX_PLAN_CHECK(g.npub <= INT_MAX, KMX_EINVAL, "public pose count does not fit int32");
  auto slot_of = [&](int rb, int pp) -> int64_t {
    const int64_t k = ((int64_t)rb << 32) | (uint32_t)pp;
    auto it = std::lower_bound(g.pub_key.begin(), g.pub_key.end(), k);
    return (it != g.pub_key.end() && *it == k) ? (int64_t)(it - g.pub_key.begin()) : -1;
  };
  g.pub_src.assign(std::max<int64_t>(g.npub, 1), -1);
  g.pose_slot.assign(std::max(nloc, 1), -1);
  int64_t first = -1, last = -1;
  for (int64_t s = 0; s < g.npub; ++s) {
    const int rb = (int)(keys[s] >> 32), pp = (int)(keys[s] & 0xffffffff);
    if (g.local_of[rb] >= 0) {
      g.pub_src[s] = g.loff[g.local_of[rb]] + pp;
      g.pose_slot[g.pub_src[s]] = (int)s;
      if (first < 0) first = s;
      KMX_PLAN_CHECK(last < 0 || last == s - 1, KMX_EUNSUP,
                     "local robots must own a contiguous range of the public table (assign robot ranges to ranks)");
      last = s;
    }
  }
  g.first_owned = first < 0 ? 0 : first;
  g.n_owned = first < 0 ? 0 : last - first + 1;
  // local edges, incidences
  auto lpose = [&](int rb, int pp) { return g.loff[g.local_of[rb]] + pp; };
  std::vector<int64_t>& ledges = g.loc_edge_gid;
  for (int64_t e = 0; e < m; ++e)
    if (g.local_of[r1[e]] >= 0 || g.local_of[r2[e]] >= 0) ledges.push_back(e);
  g.mloc = (int)ledges.size();
  g.ek.assign(std::max(g.mloc, 1), 0.0);
  g.et.assign(std::max(g.mloc, 1), 0.0);
  g.ew.assign(std::max(g.mloc, 1), 0.0);
  std::vector<int> deg((size_t)nloc + 1, 0);
  g.m_robot.assign(L, 0);
  for (int k = 0; k < g.mloc; ++k) {
    const int64_t e = ledges[k];
    g.ek[k] = kappa[e];
    g.et[k] = tau[e];
    g.ew[k] = weight[e];
    const int a1 = g.local_of[r1[e]], a2 = g.local_of[r2[e]];
    if (a1 >= 0) { deg[lpose(r1[e], p1[e])]++; g.m_robot[a1]++; }
    if (a2 >= 0) { deg[lpose(r2[e], p2[e])]++; if (r2[e] != r1[e]) g.m_robot[a2]++; }
  }
  // record width: compact (quaternion) when every local measurement rotation
  // is rebuilt from its unit quaternion to 1e-12 (a rotation), full otherwise
  // (the three stored components per edge, and the rebuilt one's index)
  std::vector<double> quat((size_t)std::max(g.mloc, 1) * 3);
  std::vector<int> qbig(std::max(g.mloc, 1), 0);
  {
    // (the other endpoint takes rec_o's low 29 bits: local poses and public
    // slots below 2^28, far above any single GPU's share)
    bool ok = nloc < (1 << 28) && g.npub < (1 << 28);
    for (int k = 0; k < g.mloc && ok; ++k) {
      const double* Q = R + 9 * ledges[k];
      double q4[4], qr[4], Rq[9];
      rot_to_quat(Q, q4);
      qbig[k] = quat_pack(q4, &quat[3 * (size_t)k]);
      quat_unpack(&quat[3 * (size_t)k], qbig[k], qr);
      quat_to_rot(qr, Rq);
      for (int i = 0; i < 9 && ok; ++i) ok = std::fabs(Rq[i] - Q[i]) <= 1e-12;
    }
    g.rw = ok ? 10 : 16;
  }
  const int RW = g.rw;
  std::vector<int>& inc_ptr = g.inc_ptr;
  inc_ptr.assign((size_t)nloc + 1, 0);
  {
    int64_t ninc64 = 0;
    for (int i = 0; i < nloc; ++i) ninc64 += deg[i];
    KMX_PLAN_CHECK(ninc64 < INT_MAX, KMX_EINVAL, "local incidence count does not fit int32");
  }
  for (int i = 0; i < nloc; ++i) inc_ptr[i + 1] = inc_ptr[i] + deg[i];
  g.ninc = inc_ptr[nloc];
  const int GS = rec_gs(RW);
  g.rec.assign((size_t)((int64_t)g.ninc + 1) * GS, 0.0);  // + one zero pad record
  g.rec_o.assign(RW == 10 ? (size_t)g.ninc + 1 : 1, 0);
  g.eipos.assign(std::max(g.mloc, 1), PgoInt2{-1, -1});
  std::vector<int> fill(inc_ptr.begin(), inc_ptr.end() - 1);
  auto put_rec = [&](int pos, int k, int64_t e, int other, int code) {
    double* c = &g.rec[(size_t)pos * GS];
    const double* Q = RW == 10 ? &quat[3 * (size_t)k] : R + 9 * e;
    int j = 0;
    for (int q = 0; q < (RW == 10 ? 3 : 9); ++q) c[j++] = Q[q];
    for (int q = 0; q < 3; ++q) c[j++] = t[3 * e + q];
    c[j++] = weight[e] * kappa[e];
    const double wt = weight[e] * tau[e];
    if (RW == 10) {  // compact: the tail flag in w tau's sign bit, the other endpoint apart
      c[j++] = (code & 0x80000000) ? -wt : wt;
      g.rec_o[pos] = (int)(((unsigned)other & 0x1fffffffu) | ((unsigned)qbig[k] << 29));
    } else {
      c[j++] = wt;
      const long long bits = (long long)(unsigned)other | (long long)((unsigned long long)(unsigned)code << 32);
      std::memcpy(&c[j], &bits, 8);
    }
  };
  for (int k = 0; k < g.mloc; ++k) {  // increasing global edge id per pose
    const int64_t e = ledges[k];
    const bool priv = r1[e] == r2[e];
    if (g.local_of[r1[e]] >= 0) {
      const int sp = lpose(r1[e], p1[e]);
      const int other = priv ? lpose(r2[e], p2[e]) : (int)(-1 - slot_of(r2[e], p2[e]));
      g.eipos[k].x = fill[sp];
      put_rec(fill[sp]++, k, e, other, (int)(k | 0x80000000u));
    }
    if (g.local_of[r2[e]] >= 0) {
      const int sp = lpose(r2[e], p2[e]);
      const int other = priv ? lpose(r1[e], p1[e]) : (int)(-1 - slot_of(r1[e], p1[e]));
      g.eipos[k].y = fill[sp];
      put_rec(fill[sp]++, k, e, other, k);
    }
  }
  // GNC: every non-fixed local edge is re-weighted here (a shared loop closure
  // on both handles of its robots, identically); the owner-packed shared-weight
  // table (owner = lower robot id, drawio:2198) is kept for the explicit exchange.
  int64_t nsh = 0;
  {
    size_t k = 0;
    for (int64_t e = 0; e < m; ++e) {
      if (r1[e] == r2[e]) continue;
      const int64_t si = nsh++;
      while (k < ledges.size() && ledges[k] < e) ++k;
      if (k < ledges.size() && ledges[k] == e) {
        g.sh_edge.push_back((int)k);
        g.sh_idx.push_back((int)si);
        if (g.local_of[std::min(r1[e], r2[e])] >= 0) {
          g.osh_edge.push_back((int)k);
          g.osh_idx.push_back((int)si);
        }
      }
    }
  }
  g.nshared = nsh;
  for (int k = 0; k < g.mloc; ++k) {
    const int64_t e = ledges[k];
    if (fixed_weight[e]) continue;
    // a local endpoint is read from the iterate, a foreign one from the public
    // table (after the exchange they hold the same row)
    auto enc = [&](int rb, int pp) -> int {
      return g.local_of[rb] >= 0 ? lpose(rb, pp) : (int)(-1 - slot_of(rb, pp));
    };
    g.gnc_edge.push_back(k);
    g.gnc_ends.push_back(PgoInt2{enc(r1[e], p1[e]), enc(r2[e], p2[e])});
  }
  // tiles: at most TP poses of one robot, cut by incidence count so every
  // workgroup's gather walks about the same number of incidences (a tile closes
  // when the next pose would take it past 1.05 x the robot's mean per full tile)
  // and capped at two chunks of TP * r incidences (two LDS hand-offs in k_hess)
  std::vector<int> tr, tp0, tnp;
  std::vector<int>& rt0 = g.rt0;
  rt0.assign(L + 1, 0);
  // incidences per tile: at most two gather chunks; small problems are cut
  // finer, to about TILES_TARGET tiles (3 workgroups per CU, one generation),
  // but not below 180 (3/4 of a chunk). Measured on one 12.5k-pose block
  // (125k incidences): 160.0 / 156.5 / 154.9 / 152.6 us per round at caps
  // 480 / 360 / 240 / 180, 207 at 120 (> 1024 tiles: a second generation);
  // 25k poses: 254.7 at 480, 245.6 at 360, 301 at 240
  // (profiles/r02/small_round/5_tile_cap.log). kmx_pgo_params.tile_incidences
  // overrides it (the multi-rank driver sets it from the team; bench.py
  // --tile-incidences for sweeps).
  int64_t inc_all = (int64_t)inc_ptr[nloc] - inc_ptr[0];
  auto cut = [&](int TP, int64_t tilecap) {
    tr.clear(); tp0.clear(); tnp.clear();
    for (int l = 0; l < L; ++l) {
      const int n = n_poses[g.robots[l]];
      const int base = g.loff[l];
      rt0[l] = (int)tr.size();
      const int64_t inc_l = (int64_t)inc_ptr[base + n] - inc_ptr[base];
      const int64_t full = std::max<int64_t>(1, ((int64_t)n + TP - 1) / TP);
      const int64_t cap = std::min(tilecap, std::max<int64_t>(1, (inc_l * 21 / 20 + full - 1) / full));
      int p0 = 0;
      while (p0 < n) {
        int np = 0;
        int64_t cum = 0;
        while (p0 + np < n && np < TP) {
          const int64_t dg = inc_ptr[base + p0 + np + 1] - inc_ptr[base + p0 + np];
          if (np > 0 && cum + dg > cap) break;
          cum += dg;
          ++np;
        }
        tr.push_back(l);
        tp0.push_back(base + p0);
        tnp.push_back(np);
        p0 += np;
      }
    }
  };
  {
    const int TP = tile_poses(r);
    int64_t tilecap = std::min<int64_t>(2 * (int64_t)TP * r,
                                        std::max<int64_t>(180, (inc_all + TILES_TARGET - 1) / TILES_TARGET));
    if (in.tile_incidences > 0) tilecap = std::max(16, in.tile_incidences);
    cut(TP, tilecap);
  }
  rt0[L] = (int)tr.size();
  const int ntiles = (int)tr.size();
  KMX_PLAN_CHECK(ntiles > 0, KMX_EINVAL, "no local poses");
  {
    // robot groups: contiguous robot ranges, at most as many as robots have
    // tiles, cut where the incidence prefix is nearest to g / G of the total
    // (every group keeps a robot with tiles); a robot without tiles belongs to
    // the group its index falls in and launches nothing
    std::vector<int64_t> pre(L + 1, 0);
    std::vector<int> tiled(L + 1, 0);  // robots with tiles before l
    for (int l = 0; l < L; ++l) {
      const int n = n_poses[g.robots[l]], base = g.loff[l];
      pre[l + 1] = pre[l] + ((int64_t)inc_ptr[base + n] - inc_ptr[base]);
      tiled[l + 1] = tiled[l] + (rt0[l + 1] > rt0[l] ? 1 : 0);
    }
    const int G = std::max(1, std::min(in.groups_req, tiled[L]));
    std::vector<int> start(G + 1, 0);
    start[G] = L;
    for (int gi = 1; gi < G; ++gi) {
      int best = -1;
      for (int c = start[gi - 1] + 1; c < L; ++c) {
        // a tiled robot in [start[gi - 1], c), and G - gi of them left in [c, L)
        if (tiled[c] == tiled[start[gi - 1]] || tiled[L] - tiled[c] < G - gi) continue;
        const int64_t dc = std::llabs(G * pre[c] - gi * pre[L]);
        if (best < 0 || dc < std::llabs(G * pre[best] - gi * pre[L])) best = c;
      }
      start[gi] = best;
    }
    g.grp.resize(G);
    for (int gi = 0; gi < G; ++gi) {
      PgoGroupCut& q = g.grp[gi];
      q.l0 = start[gi];
      q.l1 = start[gi + 1];
      q.t0 = rt0[q.l0];
      q.nt = rt0[q.l1] - rt0[q.l0];
    }
    // the grouped round's reduction form (kmx_pgo::grm)
    int most = 0;
    for (int l = 0; l < L; ++l) most = std::max(most, rt0[l + 1] - rt0[l]);
    g.grm = in.grm_forced >= 0 ? in.grm_forced : (most <= GROUP_CONSUMER_MAX_TILES ? RM_CONSUMER : RM_LAUNCH);
  }
  g.own_src.assign(std::max<int64_t>(g.n_owned, 1), 0);
  for (int64_t k = 0; k < g.n_owned; ++k) g.own_src[k] = g.pub_src[g.first_owned + k];
  g.nrob.resize(L);
  for (int l = 0; l < L; ++l) g.nrob[l] = n_poses[g.robots[l]];
  g.tile.resize(ntiles);
  for (int ti = 0; ti < ntiles; ++ti) {
    TileDesc& td = g.tile[ti];
    td.robot = tr[ti];
    td.p0 = tp0[ti];
    td.k0 = inc_ptr[tp0[ti]];
    const int ninc = inc_ptr[tp0[ti] + tnp[ti]] - td.k0;
    KMX_PLAN_CHECK(tnp[ti] < 256 && ninc < (1 << 23), KMX_EINVAL, "tile too large");
    td.np_n = tnp[ti] | (ninc << 8);
    td.rt0 = rt0[tr[ti]];
    td.rt1 = rt0[tr[ti] + 1];
    td.pad0 = td.pad1 = 0;
  }
  *out = std::move(g);
  return KMX_OK;
#undef KMX_PLAN_CHECK
}

}  // namespace kmx
