// pgo.hip — MI355X (gfx950) RBCD block updates on lifted SE(3) with GNC-TLS.
//
// Replaces dpgo's PGOAgent::iterate / updateMeasurementWeights hot path
// (drawio:2058-2066, 2215, 2466-2469, 2513).
// Design:
//   * Every local robot block lives in HBM and all blocks are updated by the
//     same launches (batched RBCD). Workgroup tiles never straddle robots, so
//     every reduction is per robot and its RTR / tCG scalars live on the device
//     in one Ctl record per robot.
//   * No scalar reaches the host inside a round. Each tile publishes its
//     partial sums; a robot's partials are reduced in tile order
//     (deterministic) either by a one-workgroup-per-robot k_reduce launch
//     (large problems) or by every workgroup of the next kernel, which needs
//     the decision anyway (the consumer form, small problems: no reduction
//     launch at all). The host only reads one progress word per robot to stop
//     enqueueing tCG steps (polled, blind or adaptive, kmx_pgo_set_tcg_poll).
//   * tCG in the linearity form: Hz by gather, delta = -z + beta delta_old,
//     Hdelta = -Hz + beta Hdelta_old; eta = sum coef_k delta_k is folded from
//     two kept directions every second step and finished where the trial
//     point is formed: k_retract, or in the consumer form the k_update that
//     ends the robot's tCG (at the step cap: k_update_last).
//   * Edge data: one 64-B compact record per incidence in CSR order (three
//     components of R's unit quaternion, t, w kappa, +-w tau — the sign bit is
//     the tail flag) plus a 4-B word (Dev::rec_o): its other endpoint and, in
//     bits 29-31, the index of the quaternion's dropped largest component,
//     which the device rebuilds: 68 B per incidence (struct Rec<10>); or a
//     128-B record with the full rotation when some measurement is not a
//     rotation to 1e-12 (Rec<16>). The gathers are incidence-parallel:
//     one lane per incidence evaluates its block against the neighbour's whole
//     r x 4 row and parks the r contribution rows in LDS; the (pose, row) lanes
//     then add their pose's contributions in CSR (= increasing edge id) order.
//     No atomics: every sum has a fixed order, so results are deterministic and
//     independent of rank placement.
//   * GNC-TLS on the device: the round-begin launch decides
//     shouldUpdateMeasurementWeights (drawio:2466-2469: inner iterations >
//     robustOptInnerIters, or every agent converged; capped at
//     robustOptNumWeightUpdates) from device state and re-weights the loop
//     closures in the same launch.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <rccl/rccl.h>
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <thread>
#include <type_traits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <numeric>
#include <string>
#include <vector>

#include "common.h"
#include "pgo_host.h"
#include "so3_project.h"

// KMX_HESS_PROBE (diagnostic builds only, scripts/gpu_hess_probe.sh): bits
// remove one k_hess stream each so its PMC traffic can be attributed; the
// results of such a build are wrong by design. 0 in the product build.
#ifndef KMX_HESS_PROBE
#define KMX_HESS_PROBE 0
#endif

namespace {

// the tile rule, the record sizes, TileDesc, RedMode and the cut's thresholds: pgo_host.h
using namespace kmx;

constexpr int BLOCK = 64 * WAVES;
constexpr int NPART = 4;  // partial sums per tile
// per-kernel LDS reduction area: NPART x WAVES wave sums + the ticket flag
constexpr int RED_BYTES = 8 * NPART * WAVES + 16;

enum Phase { PH_IDLE = 0, PH_START = 1, PH_TCG = 2, PH_STEP = 3 };
enum Mode { MODE_INTERIOR = 0, MODE_BOUNDARY = 1 };
enum RedKind { RED_GRAD = 0, RED_HESS = 1, RED_UPDATE = 2, RED_COST = 3 };

struct Ctl {
  int phase, rtr_iter, tcg_iter, tcg_stop;
  int mode, accepted, commit, updated;
  int hessvecs, skipped, retracted, pad1;  // retracted: the consumer k_update formed the trial point
  double Delta, f_init, gn_init, f_cur;
  double f_final, norm_r0, z_r, e_Pe;
  double e_Pd, d_Pd, alpha, beta;
  double coef, rho, chg_acc, rel_change;
  double r_stop;    // tCG residual stop: ||r_0|| min(||r_0||^theta, kappa), formed once per tCG
  int lin_stop, pad3;  // kappa < ||r_0||^theta: a stop at r_stop is KMX_TCG_LINEAR
  double pad2[8];   // 256 B: one robot's record never shares a line with the next
};
static_assert(sizeof(Ctl) == 256, "Ctl is 256 B");

struct Counters {
  unsigned long long edges_iters;
  unsigned long long block_updates;
  unsigned long long hessvecs;
  unsigned long long gnc_updates;
  double hess_alg_bytes;
  double pad2[3];
};

// GNC schedule state (dpgo PGOAgent: mRobustOptInnerIter, mWeightUpdateCount, mu).
struct Gnc {
  int inner;    // rounds since the last weight update
  int updates;  // weight updates so far
  int fired;    // the last round-begin launch updated the weights
  int rounds;   // rounds completed
  double mu;
  double pad[3];
};

// Field-wise copies of the schedule state (a struct assignment between global
// pointers is lowered through a scratch temporary).
__device__ __forceinline__ Gnc load_gnc(const Gnc* p) {
  Gnc s;
  s.inner = p->inner; s.updates = p->updates; s.fired = p->fired; s.rounds = p->rounds;
  s.mu = p->mu; s.pad[0] = s.pad[1] = s.pad[2] = 0.0;
  return s;
}
__device__ __forceinline__ void store_gnc(Gnc* p, const Gnc& s) {
  p->inner = s.inner; p->updates = s.updates; p->fired = s.fired; p->rounds = s.rounds; p->mu = s.mu;
}

// Host-visible tCG progress of one robot, written after every tCG step by the
// robot's update reduction (k_reduce, or the robot's first tile of the
// consumer-form k_hess) into host-mapped memory as ONE 64-bit word (seq << 1 |
// still-in-tCG): a single relaxed system-scope store, no release fence, so no
// L2 writeback. The host keeps one tCG step queued beyond the last one known
// to be needed and stops enqueueing once no robot is in tCG.
struct HostStatus {
  unsigned long long word;
};
__device__ __forceinline__ void post_status(HostStatus* hs, int l, unsigned long long seq, bool running) {
  __hip_atomic_store(&hs[l].word, (seq << 1) | (running ? 1ull : 0ull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

struct Params {
  int tcg_max, rtr_iters, use_precond, robust;
  double kappa, theta, Delta0, Delta_max, accept_rho, gn_tol, shift, barc, mu_step, rel_tol;
  int gnc_on, inner_iters, max_updates, n_ext;
  int rgd;          // KMX_METHOD_RGD: one preconditioned gradient step per block update
  double rgd_step;
};

struct Dev {
  int ntiles, L, nloc, npub;
  // the tiles of this launch: [gt0, gt0 + gnt), all of them or one robot
  // group's (kmx_pgo::grp); the grid is gnt workgroups
  int gt0, gnt;
  const TileDesc* tile;
  const int* rtile0;   // [L+1]
  const int* inc_ptr;  // [nloc+1]
  double* rec;         // [ninc + 1][Rec<RW>::GS] incidence records in CSR order (+ one zero pad record)
  const int* rec_o;    // [ninc + 1] compact records: the other endpoint of each incidence
  double* ekappa;      // [mloc] per local edge
  double* etau;
  double* ew;          // GNC weight
  const int2* eipos;   // [mloc] record positions (tail, head) of each local edge, -1 if not local
  double *X, *Xt, *g, *r, *z, *hd, *S, *Pinv, *hD, *pub;
  // D_i - S_i (S embedded in the rotation block; SYM4 per pose), written by
  // k_grad: k_hess applies it in place of D_i and S (48 B per pose per launch)
  double* hDS;
  // tCG search directions: delta_k lives in dh + (k % dhn) * vec, so eta =
  // sum_k coef_k delta_k is not updated at every Hess-vec: k_hess folds the
  // dhn oldest directions into eta before their buffer is reused (every dhn
  // steps) and k_retract adds the rest, in step order (the additions of the
  // serial eta += coef delta, same bits).
  double* dh;          // [dhn][vec]
  double* eta;         // [vec] folded directions (tcg_max > dhn only)
  double* coefh;       // [L][tcg_max] the eta coefficient (alpha or tau) of each step
  long long vec;       // doubles per vector
  int dhn;
  double* part;        // [ntiles][NPART]
  double* part_h;      // [ntiles][2] k_hess partials (RM_CONSUMER: read by k_update)
  double* part_u;      // [ntiles][2] k_update partials (RM_CONSUMER: read by the next k_hess)
  Ctl* ctl;
  Ctl* ctl2;           // [L] RM_CONSUMER: the state between k_hess and k_update of a tCG step
  Counters* cnt;
  const long long* m_robot;   // [L] local-problem edges per robot
  const int* n_robot;         // [L] poses per robot
  const int* pose_slot;       // [nloc] owned public-table slot of a pose, or -1
  double* relc;               // [L] relative change of each robot's last block update (inf: none yet)
  Gnc* gnc;                   // schedule state
  Gnc* gnc_next;              // state after the current round-begin launch (k_precond commits it)
  const double* ext;          // [n_ext] peers' largest relative change (multi-process team status)
  const int* gnc_edge;        // [n_gnc] local edges re-weighted here (non-fixed, >= 1 local endpoint)
  const int2* gnc_ends;       // [n_gnc] endpoints: >= 0 local pose, < 0 public slot -1-x
  int n_gnc;
  int* hv_launch;             // [HV_SLOTS] robots that ran a Hess-vec in timed launch k
  Params p;
  // one-sync tCG (P.tcg_form, body_step): H z_k, and w_k = precon(H delta_k)
  // double-buffered by step parity (the gathered vector), and the step's
  // 8-wide partials
  double *hz, *w0, *w1;
  double* part_f;             // [2][ntiles][8], by step parity (a launch reads step k's
                              // partials of every tile of its robot while its own tile writes step k+1's)
};

constexpr int HV_SLOTS = 1 << 16;
// tCG directions kept (Dev::dh). Same-box A/B at configs[3] (profiles/r03/dhist/):
// all ten (eta formed only in k_retract) gives the fastest k_hess (38.2 vs
// 40.5 us) but k_retract then reads up to ten vectors, and the round is 1.7 %
// slower; two (eta folded at every second step) keeps the round at the
// one-buffer form's time or better with half its eta traffic in k_hess.
#ifndef KMX_DHMAX
#define KMX_DHMAX 2
#endif
constexpr int DHMAX = KMX_DHMAX;

// Wave sum by DPP lane moves inside each row of 16 (xor 1, xor 2 by
// quad_perm, then the half-row and row mirrors: every lane of a row holds the
// row's sum, bitwise alike since each step adds the same two values), then
// the four row sums read out as scalars and added in a fixed order: the same
// value in every lane. (A shuffle butterfly costs 12 LDS permutes per sum: the
// one-sync k_step's 15 sums took ~4 us of its decision and epilogue.)
template <int CTRL>
__device__ __forceinline__ double dpp_row(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)b, CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xf, 0xf, false);
  return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}
__device__ __forceinline__ double read_lane(double v, int lane) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)b, lane);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
  return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}
__device__ __forceinline__ double wave_sum(double v) {
  v += dpp_row<0xb1>(v);   // quad_perm [1,0,3,2]
  v += dpp_row<0x4e>(v);   // quad_perm [2,3,0,1]
  v += dpp_row<0x141>(v);  // row_half_mirror
  v += dpp_row<0x140>(v);  // row_mirror
  return (read_lane(v, 0) + read_lane(v, 16)) + (read_lane(v, 32) + read_lane(v, 48));
}

// Sum over all BLOCK threads in fixed order; every thread gets the result.
__device__ __forceinline__ double block_sum(double v, double* lds) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) s += lds[w];
  return s;
}

// Sum of x over the R lanes of this lane's pose group, lane order 0..R-1
// (the order of the oracle's row loop); identical in every lane of the group.
template <int R>
__device__ __forceinline__ double gsum(double x, int base) {
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < R; ++k) s += __shfl(x, base + k, 64);
  return s;
}

__device__ __forceinline__ void load4(const double* p, double v[4]) {
  const double2* q = reinterpret_cast<const double2*>(p);
  double2 a = q[0], b = q[1];
  v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
}
__device__ __forceinline__ void store4(double* p, const double v[4]) {
  double2* q = reinterpret_cast<double2*>(p);
  q[0] = make_double2(v[0], v[1]);
  q[1] = make_double2(v[2], v[3]);
}

// Workgroup barrier for LDS hand-offs only: waits for this wave's LDS ops but
// not for its outstanding global loads (__syncthreads waits vmcnt(0), which
// would drain the next chunk's prefetched records).
// Symmetric 4x4 blocks (Q's diagonal blocks, the preconditioner) are stored
// as their upper triangle, row by row: 10 doubles, five 16-B loads.
constexpr int SYM4 = 10;
// (the five parts as loaded, for a caller that keeps them raw until use)
__device__ __forceinline__ void expand_sym4(const double2 p2[5], double M[16]) {
  const double2 a = p2[0], b = p2[1], c = p2[2], e = p2[3], f = p2[4];
  M[0] = a.x; M[1] = M[4] = a.y; M[2] = M[8] = b.x; M[3] = M[12] = b.y;
  M[5] = c.x; M[6] = M[9] = c.y; M[7] = M[13] = e.x;
  M[10] = e.y; M[11] = M[14] = f.x;
  M[15] = f.y;
}
__device__ __forceinline__ void load_sym4(const double* p, double M[16]) {
  const double2* p2 = reinterpret_cast<const double2*>(p);
  const double2 v[5] = {p2[0], p2[1], p2[2], p2[3], p2[4]};
  expand_sym4(v, M);
}
// S = sym(Y^T G_Y) stored as its 6 upper entries
__device__ __forceinline__ void load_sym3(const double* p, double S[9]) {
  S[0] = p[0]; S[1] = S[3] = p[1]; S[2] = S[6] = p[2];
  S[4] = p[3]; S[5] = S[7] = p[4];
  S[8] = p[5];
}

__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ------------------------------------------------------------ edge records --
struct Edge {
  double R[9], t[3], wk, wt;
};

__device__ __forceinline__ int2 unpack_int2(double v) {
  const long long b = __double_as_longlong(v);
  return make_int2((int)(b & 0xffffffffll), (int)(b >> 32));
}

// RW = 10: compact record — 64 B in HBM (GS = 8 doubles, four 16-B parts):
// three components of the unit quaternion of R (all but its largest, which is
// made >= 0 and rebuilt as sqrt(1 - the others' squares): well conditioned,
// since it is >= 1/2), t, w kappa, +-w tau (the sign bit is the tail flag; w
// tau >= 0, a zero weight is +-0.0); Dev::rec_o (4 B) holds the other endpoint
// in its low 29 bits (two's complement) and the rebuilt component's index in
// bits 29-31: 68 B per incidence (round 5: the whole quaternion, 76 B). In
// registers it is the 10-word form (w, x, y, z, t, w kappa, w tau, {other,
// tail << 31}), five 16-B parts; the gathers rebuild R from the quaternion
// (R R^T = I to rounding, as the preconditioner assumes).
// RW = 16: full record (R, t, w kappa, w tau, {other, edge|tail}, pad), for
// measurement rotations off SO(3).
template <int RW>
struct Rec {
  static constexpr int Q = RW / 2;        // 16-B parts in registers
  static constexpr int GS = rec_gs(RW);         // doubles per record in HBM
  static constexpr int WK = RW == 10 ? 6 : 12;  // index of w kappa (w tau follows)
  static constexpr int QS = RW == 10 ? 4 : Q;   // 16-B parts of the record as stored
  // The load in two halves, for a gather that fetches the word with the other
  // endpoint a chunk ahead of the record (hinc_gather_src's PF): the record as
  // stored, the compact record's 4-B word (rec_o), and the register form of
  // the two. The full record holds the other endpoint itself: no word.
  __device__ static __forceinline__ void load_stored(const Dev& d, size_t k, double2 a[QS]) {
    const double2* p2 = reinterpret_cast<const double2*>(d.rec + (size_t)GS * k);
#pragma unroll
    for (int i = 0; i < QS; ++i) a[i] = p2[i];
  }
  __device__ static __forceinline__ unsigned load_word(const Dev& d, size_t k) {
    static_assert(RW == 10, "compact records only");
    return (unsigned)d.rec_o[k];
  }
  __device__ static __forceinline__ int other_of(unsigned word) {
    static_assert(RW == 10, "compact records only");
    return (int)(word << 3) >> 3;
  }
  __device__ static __forceinline__ void expand(const double2 a[QS], unsigned raw, double2 q[Q]) {
    if constexpr (RW == 10) {
      const double2 a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3];  // (qa, qb) (qc, t0) (t1, t2) (wk, +-wt)
      const int other = (int)(raw << 3) >> 3;
      const unsigned big = raw >> 29;
      const double qa = a0.x, qb = a0.y, qc = a1.x;
      const double ql = sqrt(1.0 - (qa * qa + qb * qb + qc * qc));
      const double w = big == 0 ? ql : qa, x = big == 0 ? qa : (big == 1 ? ql : qb);
      const double y = big <= 1 ? qb : (big == 2 ? ql : qc), z = big == 3 ? ql : qc;
      q[0] = make_double2(w, x);
      q[1] = make_double2(y, z);
      q[2] = make_double2(a1.y, a2.x);
      q[3] = make_double2(a2.y, a3.x);
      const double wt = a3.y;
      const long long bits = (long long)(unsigned)other | (std::signbit(wt) ? (1ll << 63) : 0ll);
      q[4] = make_double2(std::fabs(wt), __longlong_as_double(bits));
    } else {
#pragma unroll
      for (int i = 0; i < Q; ++i) q[i] = a[i];
    }
  }
  __device__ static __forceinline__ void load(const Dev& d, size_t k, double2 q[Q]) {
    double2 a[QS];
    load_stored(d, k, a);
    unsigned word = 0;
    if constexpr (RW == 10) word = load_word(d, k);
    expand(a, word, q);
  }
  // the stored w tau of an incidence (compact: its sign is the tail flag)
  __device__ static __forceinline__ double wt_word(double wt, bool tail) {
    return (RW == 10 && tail) ? -wt : wt;
  }
  __device__ static __forceinline__ void edge(const double2 q[Q], Edge& E) {
    if constexpr (RW == 10) {
      const double w = q[0].x, x = q[0].y, y = q[1].x, z = q[1].y;
      const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z;
      const double wx = w * x, wy = w * y, wz = w * z;
      E.R[0] = 1.0 - 2.0 * (yy + zz); E.R[1] = 2.0 * (xy - wz); E.R[2] = 2.0 * (xz + wy);
      E.R[3] = 2.0 * (xy + wz); E.R[4] = 1.0 - 2.0 * (xx + zz); E.R[5] = 2.0 * (yz - wx);
      E.R[6] = 2.0 * (xz - wy); E.R[7] = 2.0 * (yz + wx); E.R[8] = 1.0 - 2.0 * (xx + yy);
      E.t[0] = q[2].x; E.t[1] = q[2].y; E.t[2] = q[3].x;
      E.wk = q[3].y;
      E.wt = q[4].x;
    } else {
      E.R[0] = q[0].x; E.R[1] = q[0].y; E.R[2] = q[1].x; E.R[3] = q[1].y; E.R[4] = q[2].x;
      E.R[5] = q[2].y; E.R[6] = q[3].x; E.R[7] = q[3].y; E.R[8] = q[4].x;
      E.t[0] = q[4].y; E.t[1] = q[5].x; E.t[2] = q[5].y;
      E.wk = q[6].x;
      E.wt = q[6].y;
    }
  }
  __device__ static __forceinline__ int2 inc(const double2 q[Q]) {
    return unpack_int2(RW == 10 ? q[4].y : q[7].x);
  }
};

// Contribution of one incidence to row a of pose `self`. vs = self row, vo =
// other endpoint row. Expressions mirror oracle/dpgo_oracle.c edge_eval
// exactly. Returns the row's share of 1/2 w (kappa |E_R|^2 + tau E_t^2).
__device__ __forceinline__ double incidence_row(const Edge& E, bool self_tail, const double vs[4],
                                                const double vo[4], double acc[4]) {
  double ER[3], Et;
  if (self_tail) {  // self = i (tail), other = j (head)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      ER[c] = vo[c] - (vs[0] * E.R[0 * 3 + c] + vs[1] * E.R[1 * 3 + c] + vs[2] * E.R[2 * 3 + c]);
    Et = vo[3] - vs[3] - (vs[0] * E.t[0] + vs[1] * E.t[1] + vs[2] * E.t[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c)
      acc[c] -= E.wk * (ER[0] * E.R[c * 3 + 0] + ER[1] * E.R[c * 3 + 1] + ER[2] * E.R[c * 3 + 2]) +
                E.wt * Et * E.t[c];
    acc[3] -= E.wt * Et;
  } else {  // self = j (head), other = i (tail)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      ER[c] = vs[c] - (vo[0] * E.R[0 * 3 + c] + vo[1] * E.R[1 * 3 + c] + vo[2] * E.R[2 * 3 + c]);
    Et = vs[3] - vo[3] - (vo[0] * E.t[0] + vo[1] * E.t[1] + vo[2] * E.t[2]);
    acc[0] += E.wk * ER[0];
    acc[1] += E.wk * ER[1];
    acc[2] += E.wk * ER[2];
    acc[3] += E.wt * Et;
  }
  return 0.5 * (E.wk * (ER[0] * ER[0] + ER[1] * ER[1] + ER[2] * ER[2]) + E.wt * Et * Et);
}

// ------------------------------------------------------ Stiefel group ops --
// S = sym(Y^T G_Y) for the pose group (9 entries, identical in all R lanes).
// LDS = true (kernels with a free BLOCK x 6-double LDS scratch `scr`): every
// lane writes its 6 products, then reads its group's R x 6 back and adds them
// in lane order: one LDS round trip instead of 6 chained shuffle chains. Only
// lanes of one wave exchange data (in-order LDS queue; no workgroup barrier).
// LDS = false: 6 shuffle sums, each chained to the previous one (empty asm) so
// only one sum's R shuffles are in flight (VGPR pressure).
// FL (LDS form): the group members whose read-back is in flight at a time.
constexpr int GSYM_FLIGHT = 2;
constexpr int GSYM_ALL = 8;  // >= R: no bound (k_eval, the parity primitive, which runs at 128 VGPRs either way)
template <int R, bool LDS = false, int FL = GSYM_FLIGHT>
__device__ __forceinline__ void group_symYtG(const double y[4], const double G[4], int base, double S[9],
                                             double* scr = nullptr) {
  if constexpr (LDS) {
    double* mine = scr + 6 * threadIdx.x;
    {
      int j = 0;
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = c; k < 3; ++k) mine[j++] = 0.5 * (y[c] * G[k] + y[k] * G[c]);
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
    const double* grp = scr + 6 * ((threadIdx.x & ~63u) + base);
    double t[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    // FL members' values in flight at a time (12 VGPRs each; all R at once
    // set the register count of the element-wise kernels); the adds keep their
    // order m = 0 .. R - 1
    if constexpr (FL >= R) {
#pragma unroll
      for (int m = 0; m < R; ++m)
#pragma unroll
        for (int j = 0; j < 6; ++j) t[j] += grp[6 * m + j];
    } else {
#pragma unroll
      for (int m = 0; m < R; ++m) {
#pragma unroll
        for (int j = 0; j < 6; ++j) t[j] += grp[6 * m + j];
        if ((m + 1) % FL == 0 && m + 1 < R)
          asm volatile("" : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]), "+v"(t[4]), "+v"(t[5])::"memory");
      }
    }
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    int j = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int k = c; k < 3; ++k, ++j) {
        S[c * 3 + k] = t[j];
        S[k * 3 + c] = t[j];
      }
  } else {
    double prev = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int k = c; k < 3; ++k) {
        double x = 0.5 * (y[c] * G[k] + y[k] * G[c]);
        asm volatile("" : "+v"(x) : "v"(prev));
        prev = gsum<R>(x, base);
        S[c * 3 + k] = prev;
        S[k * 3 + c] = prev;
      }
  }
}

// Tangent projection of row V at Y (group-cooperative): V_Y - Y sym(Y^T V_Y).
template <int R, bool LDS = false, int FL = GSYM_FLIGHT>
__device__ __forceinline__ void group_proj(const double y[4], const double V[4], int base, double out[4],
                                           double* scr = nullptr) {
  double S[9];
  group_symYtG<R, LDS, FL>(y, V, base, S, scr);
#pragma unroll
  for (int c = 0; c < 3; ++c) out[c] = V[c] - (y[0] * S[0 * 3 + c] + y[1] * S[1 * 3 + c] + y[2] * S[2 * 3 + c]);
  out[3] = V[3];
}

// Preconditioner: P_Y(V Pinv_i) (block-Jacobi on Q's 4x4 diagonal blocks).
// Pre (LDS form only, has_pre): the pose's block, already loaded by the caller.
template <int R, bool LDS = false, int FL = GSYM_FLIGHT>
__device__ __forceinline__ void group_precon(const Dev& d, int pose, bool valid, const double y[4],
                                             const double V[4], int base, double out[4], double* scr = nullptr,
                                             const double* Pre = nullptr, bool has_pre = false) {
  if (!d.p.use_precond) {
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = V[k];
    return;
  }
  double buf[4] = {0.0, 0.0, 0.0, 0.0};
  static_assert(LDS, "the LDS form only");
  double P[16];
  if (has_pre) {
#pragma unroll
    for (int i = 0; i < 16; ++i) P[i] = Pre[i];
  } else {
    load_sym4(d.Pinv + SYM4 * (size_t)pose, P);  // pose is valid on every lane
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int k = 0; k < 4; ++k) buf[k] = (i == 0) ? V[0] * P[k] : buf[k] + V[i] * P[4 * i + k];
  group_proj<R, LDS, FL>(y, buf, base, out, scr);
}

// Riemannian Hessian row of V given the Euclidean Hessian row H:
// P_Y(H_Y - V_Y S) ; p-part H_p.
template <int R, bool LDS = false, int FL = GSYM_FLIGHT>
__device__ __forceinline__ void group_rhess(const double y[4], const double V[4], const double H[4],
                                            const double S[9], int base, double out[4], double* scr = nullptr) {
  double buf[4];
#pragma unroll
  for (int k = 0; k < 3; ++k) buf[k] = H[k] - (V[0] * S[0 * 3 + k] + V[1] * S[1 * 3 + k] + V[2] * S[2 * 3 + k]);
  buf[3] = H[3];
  group_proj<R, LDS, FL>(y, buf, base, out, scr);
}

// QF retraction (modified Gram-Schmidt over the 3 columns, positive diagonal).
template <int R>
__device__ __forceinline__ void group_retract(const double x[4], const double v[4], int base, double out[4]) {
  double A[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) A[c] = x[c] + v[c];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int k = 0; k < c; ++k) {
      const double s = gsum<R>(A[k] * A[c], base);
      A[c] -= s * A[k];
    }
    const double nn = gsum<R>(A[c] * A[c], base);
    const double inv = 1.0 / sqrt(nn);
    A[c] *= inv;
  }
  out[0] = A[0]; out[1] = A[1]; out[2] = A[2];
  out[3] = x[3] + v[3];
}

// Proj of the accelerated rounds (k_accel) and KMX_EVAL_PROJECT: the polar
// factor U V^T of the pose's r x 3 rotation block (this lane holds row a in
// m[0..2]); out[3] = m[3]. Every lane of the group fetches the whole block
// (3 R shuffles, all lanes active) and runs the oracle's proj_stiefel on it in
// registers, so nothing below exchanges data and a lane may leave its loops
// alone. One-sided Jacobi, as so3_project.h: plane rotations W turn the
// columns of A = M W orthogonal and Y = sum_k (A_k / |A_k|) W_k^T. The block is
// never squared and no vanishing singular value is divided by: a column that
// is zero, or that one Gram-Schmidt step against the larger columns'
// directions takes more than half of (its direction is rounding noise), is
// replaced by a completion of the frame (the e_k the kept directions are least
// along, made orthogonal in two passes; their squared entries in row k sum to
// at most 2 / R < 1 there, so what is left never vanishes). The output always
// has orthonormal columns; the zero block, and a block with a non-finite
// entry, give e1 e2 e3. `live` is false on the idle tail lanes, whose block
// would mix two groups: they work on zeros.
template <int R>
__device__ __forceinline__ void group_project(const double m[4], int a, int base, bool live, double out[4]) {
  double A[R][3], W[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  double amax = 0.0, fin = 0.0;
#pragma unroll
  for (int k = 0; k < R; ++k) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double x = __shfl(m[c], base + k, 64);
      A[k][c] = live ? x : 0.0;
      amax = fmax(amax, fabs(A[k][c]));
    }
    fin += (A[k][0] + A[k][1] + A[k][2]) * 0.0;  // Inf * 0 and NaN * 0 are NaN
  }
  const bool ok = fin == 0.0 && amax > 0.0 && amax < INFINITY;
#pragma unroll
  for (int k = 0; k < R; ++k)
#pragma unroll
    for (int c = 0; c < 3; ++c) A[k][c] = ok ? A[k][c] / amax : 0.0;  // the projection does not depend on the scale
  for (int sweep = 0; sweep < 30; ++sweep) {
    bool rotated = false;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = i + 1; j < 3; ++j) {
        double aii = 0.0, ajj = 0.0, aij = 0.0;
#pragma unroll
        for (int k = 0; k < R; ++k) aii += A[k][i] * A[k][i];
#pragma unroll
        for (int k = 0; k < R; ++k) ajj += A[k][j] * A[k][j];
#pragma unroll
        for (int k = 0; k < R; ++k) aij += A[k][i] * A[k][j];
        // orthogonal to 4 eps: below it a rotation only moves rounding noise about (the sums'
        // own rounding is R eps / 2), and the Gram-Schmidt step below takes what is left
        if (fabs(aij) <= 0x1p-50 * sqrt(aii * ajj) || aij == 0.0 || !(fabs(aij) < INFINITY)) continue;
        rotated = true;
        const double zeta = (ajj - aii) / (2.0 * aij);
        const double tt = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double cs = 1.0 / sqrt(1.0 + tt * tt), sn = cs * tt;
#pragma unroll
        for (int k = 0; k < R; ++k) {
          const double ai = A[k][i], aj = A[k][j];
          A[k][i] = cs * ai - sn * aj;
          A[k][j] = sn * ai + cs * aj;
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const double vi = W[q][i], vj = W[q][j];
          W[q][i] = cs * vi - sn * vj;
          W[q][j] = sn * vi + cs * vj;
        }
      }
    if (!rotated) break;
  }
  double s2[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int k = 0; k < R; ++k) s2[c] += A[k][c] * A[k][c];
  // columns by decreasing norm, as the oracle picks them: the largest (the
  // first of equals), then the other two in index order unless the later is
  // larger; moved with selects, so no register is indexed
  auto swap_cols = [&](int x, int y, bool on) {
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const double p = A[k][x], q = A[k][y];
      A[k][x] = on ? q : p;
      A[k][y] = on ? p : q;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double p = W[k][x], q = W[k][y];
      W[k][x] = on ? q : p;
      W[k][y] = on ? p : q;
    }
    const double p = s2[x], q = s2[y];
    s2[x] = on ? q : p;
    s2[y] = on ? p : q;
  };
  const bool first2 = s2[2] > fmax(s2[0], s2[1]), first1 = !first2 && s2[1] > s2[0];
  swap_cols(0, 1, first1);  // (1, 0, 2)
  swap_cols(1, 2, first2);  // (0, 2, 1) ...
  swap_cols(0, 1, first2);  // ... (2, 0, 1)
  swap_cols(1, 2, s2[2] > s2[1]);
  // u1: the largest column (zero only for the zero block), in place in A
  {
    const double n1 = sqrt(s2[0]);
#pragma unroll
    for (int k = 0; k < R; ++k) A[k][0] = s2[0] > 0.0 ? A[k][0] / n1 : (k == 0 ? 1.0 : 0.0);
  }
  // u2, u3: one Gram-Schmidt step against the directions before them, or the completion
#pragma unroll
  for (int c = 1; c < 3; ++c) {
    const double s = s2[c], ns = sqrt(s);
    double t[R];
#pragma unroll
    for (int k = 0; k < R; ++k) t[k] = s > 1e-280 ? A[k][c] / ns : 0.0;
#pragma unroll
    for (int j = 0; j < c; ++j) {
      double dot = 0.0;
#pragma unroll
      for (int k = 0; k < R; ++k) dot += A[k][j] * t[k];
#pragma unroll
      for (int k = 0; k < R; ++k) t[k] -= dot * A[k][j];
    }
    double nn = 0.0;
#pragma unroll
    for (int k = 0; k < R; ++k) nn += t[k] * t[k];
    if (nn >= 0.5) {
      const double nt = sqrt(nn);
#pragma unroll
      for (int k = 0; k < R; ++k) A[k][c] = t[k] / nt;
    } else {
      int kb = 0;
      double best = 0.0;
#pragma unroll
      for (int k = 0; k < R; ++k) {
        double q = 0.0;
#pragma unroll
        for (int j = 0; j < c; ++j) q += A[k][j] * A[k][j];
        if (k == 0 || q < best) {
          best = q;
          kb = k;
        }
      }
#pragma unroll
      for (int k = 0; k < R; ++k) t[k] = (k == kb) ? 1.0 : 0.0;
#pragma unroll
      for (int pass = 0; pass < 2; ++pass)
#pragma unroll
        for (int j = 0; j < c; ++j) {
          double dot = 0.0;
#pragma unroll
          for (int k = 0; k < R; ++k) dot += A[k][j] * t[k];
#pragma unroll
          for (int k = 0; k < R; ++k) t[k] -= dot * A[k][j];
        }
      double nw = 0.0;
#pragma unroll
      for (int k = 0; k < R; ++k) nw += t[k] * t[k];
      nw = sqrt(nw);
#pragma unroll
      for (int k = 0; k < R; ++k) A[k][c] = t[k] / nw;
    }
  }
  // this lane's row of U W^T
  double ua[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < R; ++k)
#pragma unroll
    for (int c = 0; c < 3; ++c) ua[c] = (k == a) ? A[k][c] : ua[c];
#pragma unroll
  for (int j = 0; j < 3; ++j) out[j] = ua[0] * W[j][0] + ua[1] * W[j][1] + ua[2] * W[j][2];
  out[3] = m[3];
}

// ------------------------------------------------------------- lane map ----
struct Lane {
  int tile, l, w, ln, pw, a, base, pose;
  int p0, np, k0, n;  // the tile's poses and incidences (TileDesc)
  int rt0, rt1;       // the robot's tiles
  bool valid;
};
template <int R>
__device__ __forceinline__ Lane lane_map(const Dev& d) {
  constexpr int PPW = 64 / R;
  Lane L;
  // XCD-aware, bijective block -> tile remap (cdna_hip_programming.md T1):
  // blocks b and b + 8 share an XCD, so each XCD gets one contiguous range of
  // tiles — about one robot block, whose rows then stay in that XCD's L2.
  {
    const int nwg = d.gnt, b = blockIdx.x;
    const int q = nwg >> 3, rr = nwg & 7, x = b & 7;
    L.tile = d.gt0 + (x < rr ? x * (q + 1) : rr * (q + 1) + (x - rr) * q) + (b >> 3);
  }
  const TileDesc t = d.tile[L.tile];
  L.l = t.robot;
  L.p0 = t.p0;
  L.np = t.np_n & 0xff;
  L.k0 = t.k0;
  L.n = t.np_n >> 8;
  L.rt0 = t.rt0;
  L.rt1 = t.rt1;
  L.w = threadIdx.x >> 6;
  L.ln = threadIdx.x & 63;
  L.pw = L.ln / R;
  L.a = L.ln - L.pw * R;
  L.base = L.pw * R;
  const int local = L.w * PPW + L.pw;
  L.valid = (L.pw < PPW) && (local < L.np);
  L.pose = L.p0 + (L.valid ? local : 0);
  if (L.base + R > 64) L.base = 64 - R;  // idle tail lanes shuffle within range
  return L;
}

// --------------------------------------------------------------- gathers ---
// LDS layouts. A tile holds TP = W * (64 / R) poses (W = WAVES waves per
// workgroup); its
// incidences are one contiguous CSR range walked in chunks of CH incidences
// (one lane each).
template <int R, int W = WAVES>
struct SmemH {  // Hessian gather (k_hess, eval EHESS)
  static constexpr int TP = tile_poses(R, W);
  static constexpr int CH = TP * R;                                       // <= 64 W
  static constexpr int c_off = 0;                                         // double[CH][R][4]
  static constexpr int ptr_off = CH * R * 32;                             // int[TP + 1]
  static constexpr int red_off = ptr_off + ((TP + 1) * 4 + 15) / 16 * 16;
  static constexpr int bytes = red_off + 8 * NPART * W + 16;
};
template <int R, int W = WAVES>
struct SmemHG {  // gradient / cost gathers: a chunk buffer plus the tile's own rows
  static constexpr int TP = tile_poses(R, W);
  static constexpr int CH = 240;                                          // incidences per chunk
  static constexpr int c_off = 0;                                         // double[CH][R][4]
  static constexpr int x_off = CH * R * 32;                               // double[TP][R][4]
  static constexpr int ptr_off = x_off + TP * R * 32;                     // int[TP + 1]
  static constexpr int red_off = ptr_off + ((TP + 1) * 4 + 15) / 16 * 16;
  static constexpr int bytes = red_off + 8 * NPART * W + 16;
};
template <int R, int W = WAVES>
struct SmemC {  // trial cost: own rows + CSR pointers only
  static constexpr int TP = tile_poses(R, W);
  static constexpr int x_off = 0;
  static constexpr int ptr_off = TP * R * 32;
  static constexpr int red_off = ptr_off + ((TP + 1) * 4 + 15) / 16 * 16;
  static constexpr int bytes = red_off + 8 * NPART * W + 16;
};
constexpr int SCR_BYTES = BLOCK * 6 * 8;  // group_symYtG<R, true> scratch
struct SmemU {                            // element-wise kernels: scratch + reduction
  static constexpr int red_off = SCR_BYTES;
  static constexpr int bytes = red_off + RED_BYTES;
};
static_assert(SCR_BYTES <= SmemH<3>::ptr_off && SCR_BYTES <= SmemH<8>::ptr_off, "scratch");
static_assert(SCR_BYTES <= SmemHG<3>::x_off, "scratch");

// Euclidean Hessian-vector product Q V of the tile's poses (the local problem:
// a public neighbour's row counts as zero). Q's diagonal block D_i (k_precond)
// is applied once per pose; an incidence contributes only its off-diagonal
// block applied to the other endpoint's whole r x 4 row.
struct NoPre {
  __device__ bool operator()() const { return true; }
};
struct NoEpi {
  __device__ void operator()() const {}
};
// `pre` runs once the first chunk's records are in flight, before any row is
// gathered (workgroup-uniform; false: leave without gathering).
// REC_FIRST: the first chunk's records are issued before the tile's CSR
// offsets, so the two loads overlap (the consumer form keeps the offsets
// first: its decision in `pre` is a call, and the records live across it
// would spill)
// DIAG = false: the caller applies the diagonal block itself (k_step, whose
// epilogue loads the own row and D_i with the rest of its rows in one batch).
// PF: the next chunk's neighbour rows are issued with its records, once this
// chunk's contributions are in LDS, so both fly across the hand-off and the
// pose sums. A row's address comes from the word with the other endpoint,
// which is therefore fetched one chunk further ahead (one register; the same
// clamp as the records, so it stays inside the tile's range or the pad
// record). k_hess takes it for the compact records (HessPF below); the full
// record carries the other endpoint inside itself and keeps the rows' loads
// at the top of the chunk (with them prefetched k_hess<5, 16, .> spills).
// The gradient gather (hinc_grad) has the same loop; there the prefetch fits
// without scratch but did not shorten k_grad.
// `epi` runs exactly once in a gather that `pre` let through: on the tile's
// last chunk in place of a next chunk's loads (the last chunk is peeled out
// of the loop, so what `epi` loads is not live around the loop), or at once
// on a tile without incidences. k_hess issues its epilogue's loads there;
// none of their addresses depends on the gather.
template <int R, int RW, bool REC_FIRST, typename Src, typename Pre, bool DIAG = true, int W = WAVES,
          bool PF = false, typename Epi = NoEpi>
__device__ __forceinline__ bool hinc_gather_src(const Dev& d, const Lane& L, Src& src, double acc[4], char* smem,
                                                Pre&& pre, Epi&& epi = Epi{}) {
  static_assert(!PF || RW == 10, "the row prefetch reads rec_o ahead: compact records only");
  using SM = SmemH<R, W>;
  using RC = Rec<RW>;
  constexpr int CH = SM::CH;
  double* Cs = reinterpret_cast<double*>(smem + SM::c_off);
  int* sptr = reinterpret_cast<int*>(smem + SM::ptr_off);
  const int tid = threadIdx.x;
  const int p0 = L.p0, np = L.np, K0 = L.k0, n = L.n;
  const int pl = L.pose - p0;
  const int lt = min(tid, CH - 1);
  acc[0] = acc[1] = acc[2] = acc[3] = 0.0;
  // clamped, unconditional record loads (the pad record keeps an empty tile
  // at the end of the array inside it); the record stays as stored until the
  // chunk is computed
  auto at = [&](int c0) { return (size_t)(K0 + max(min(c0 + lt, n - 1), 0)); };
  double2 qs[RC::QS];
  unsigned wo = 0, wo_next = 0;  // the word with the other endpoint: this chunk's, the next one's
  auto ld = [&](int c0) {
    RC::load_stored(d, at(c0), qs);
    if constexpr (RW == 10 && !PF) wo = RC::load_word(d, at(c0));
  };
  if constexpr (REC_FIRST) ld(0);
  if (tid <= np) sptr[tid] = d.inc_ptr[p0 + tid] - K0;
  if constexpr (!REC_FIRST) ld(0);
  if constexpr (PF) {
    wo = RC::load_word(d, at(0));
    wo_next = RC::load_word(d, at(CH));
  }
  __syncthreads();  // sptr
  if (!pre()) return false;
  double2 vr[2 * R];
  if constexpr (PF) {
    if (n > 0) src.nbr(RC::other_of(wo), vr);
  }
  auto chunk = [&](const int c0, auto last_c) __attribute__((always_inline)) {
    constexpr bool LAST = decltype(last_c)::value;
    double2 q[RC::Q];
    RC::expand(qs, wo, q);
    Edge E;
    RC::edge(q, E);
    const int2 in = RC::inc(q);
    const int o = in.x;
    const bool tail = (in.y >> 31) & 1;
    if constexpr (!PF) src.nbr(o, vr);
    if (tid < CH && c0 + tid < n) {
      const double wk = (o >= 0) ? E.wk : 0.0, wt = (o >= 0) ? E.wt : 0.0;
#pragma unroll
      for (int a = 0; a < R; ++a) {
        const double v0 = vr[2 * a].x, v1 = vr[2 * a].y, v2 = vr[2 * a + 1].x, v3 = vr[2 * a + 1].y;
        double h[4];
        if (tail) {  // self = i: row(j) Q_ji = -w [kappa row(j)_Y R^T + tau p_j t^T, tau p_j]
#pragma unroll
          for (int c = 0; c < 3; ++c)
            h[c] = -(wk * (v0 * E.R[c * 3 + 0] + v1 * E.R[c * 3 + 1] + v2 * E.R[c * 3 + 2]) + wt * v3 * E.t[c]);
          h[3] = -(wt * v3);
        } else {  // self = j: row(i) Q_ij = -w [kappa row(i)_Y R, tau (p_i + row(i)_Y t)]
#pragma unroll
          for (int c = 0; c < 3; ++c) h[c] = -(wk * (v0 * E.R[0 * 3 + c] + v1 * E.R[1 * 3 + c] + v2 * E.R[2 * 3 + c]));
          h[3] = -(wt * (v3 + (v0 * E.t[0] + v1 * E.t[1] + v2 * E.t[2])));
        }
        store4(Cs + (tid * R + a) * 4, h);
      }
    }
    // the next chunk's records (PF: and its rows), issued once this chunk's
    // rows are consumed, stay in flight across the LDS hand-off and the pose
    // sums; the last chunk has no next one and issues the caller's loads
    asm volatile("" ::: "memory");
    if constexpr (LAST) {
      epi();
    } else {
      ld(c0 + CH);
      if constexpr (PF) {
        wo = wo_next;
        src.nbr(RC::other_of(wo), vr);
        wo_next = RC::load_word(d, at(c0 + 2 * CH));
      }
    }
    lds_barrier();
    if (L.valid) {
      const int j0 = max(sptr[pl], c0) - c0, j1 = min(sptr[pl + 1], c0 + CH) - c0;
#pragma unroll 4
      for (int j = j0; j < j1; ++j) {
        double h[4];
        load4(Cs + (j * R + L.a) * 4, h);
        acc[0] += h[0]; acc[1] += h[1]; acc[2] += h[2]; acc[3] += h[3];
      }
    }
    lds_barrier();
  };
  // a gather with neither prefetched rows nor a hook keeps the plain loop (its
  // last chunk then issues a clamped record load nobody reads; peeled, k_eval
  // takes more scratch)
  if constexpr (PF || !std::is_same_v<std::decay_t<Epi>, NoEpi>) {
    int c0 = 0;
    for (; c0 + CH < n; c0 += CH) chunk(c0, std::false_type{});
    if (n > 0) chunk(c0, std::true_type{});
    else epi();
  } else {
    for (int c0 = 0; c0 < n; c0 += CH) chunk(c0, std::false_type{});
  }
  if (DIAG && L.valid) {
    double vs[4];
    double D[16];
    src.own(L.pose, L.a, vs);
#if KMX_HESS_PROBE & 2  // traffic attribution build: no diagonal-block loads
    for (int c = 0; c < 16; ++c) D[c] = (c % 5 == 0) ? 1.0 : 0.0;
#else
    load_sym4(d.hD + SYM4 * (size_t)L.pose, D);
#endif
#pragma unroll
    for (int c = 0; c < 4; ++c)
      acc[c] += vs[0] * D[4 * c] + vs[1] * D[4 * c + 1] + vs[2] * D[4 * c + 2] + vs[3] * D[4 * c + 3];
  }
  return true;
}

// Where the gathered rows come from: a stored vector (the rows of the
// traffic-attribution builds replaced by constants).
template <int R>
struct PlainRows {
  const double* V;
  // the other endpoint's whole r x 4 row (o < 0, a public neighbour: any row; its weight is zeroed)
  __device__ __forceinline__ void nbr(int o, double2 vr[2 * R]) const {
    const double2* b2 = reinterpret_cast<const double2*>(V + (size_t)max(o, 0) * 4 * R);
#if KMX_HESS_PROBE & 1  // traffic attribution build: no neighbour rows
#pragma unroll
    for (int i = 0; i < 2 * R; ++i) vr[i] = make_double2(1e-3 * i, 1e-3);
    (void)b2;
#else
#pragma unroll
    for (int i = 0; i < 2 * R; ++i) vr[i] = b2[i];
#endif
  }
  // row a of the lane's own pose
  __device__ __forceinline__ void own(int pose, int a, double vs[4]) {
#if KMX_HESS_PROBE & 2  // traffic attribution build: no own-row loads
    for (int c = 0; c < 4; ++c) vs[c] = 1e-3 * c;
#else
    load4(V + (size_t)pose * 4 * R + 4 * a, vs);
#endif
  }
};
template <int R, int RW, bool REC_FIRST = false, bool DIAG = true, bool PF = false, typename Pre = NoPre,
          typename Epi = NoEpi>
__device__ __forceinline__ bool hinc_gather(const Dev& d, const Lane& L, const double* V, double acc[4],
                                            char* smem, Pre&& pre = Pre{}, Epi&& epi = Epi{}) {
  PlainRows<R> src{V};
  return hinc_gather_src<R, RW, REC_FIRST, PlainRows<R>, Pre&, DIAG, WAVES, PF, Epi&>(d, L, src, acc, smem, pre, epi);
}

// Gradient and cost, incidence-parallel. A lane evaluates its whole incidence
// with incidence_row (diagonal and off-diagonal terms; a public neighbour's row
// from the table), reading its own pose's row from an LDS copy of the tile's
// rows (owning pose found by a binary search of the tile CSR), and adds the
// incidence's cost share (1/2 per endpoint of a local edge; all of a shared
// edge). The pose sums run in CSR order.
template <int R, int RW, int W = WAVES>
__device__ __forceinline__ void hinc_grad(const Dev& d, const Lane& L, const double* V, const double* pub,
                                          double acc[4], double* cost, char* smem) {
  using SM = SmemHG<R, W>;
  using RC = Rec<RW>;
  constexpr int CH = SM::CH;
  double* Cs = reinterpret_cast<double*>(smem + SM::c_off);
  double2* xs = reinterpret_cast<double2*>(smem + SM::x_off);
  int* sptr = reinterpret_cast<int*>(smem + SM::ptr_off);
  const int tid = threadIdx.x;
  const int p0 = L.p0, np = L.np, K0 = L.k0, n = L.n;
  const int pl = L.pose - p0;
  const int lt = min(tid, CH - 1);
  acc[0] = acc[1] = acc[2] = acc[3] = 0.0;
  double csum = 0.0;
  auto ld = [&](int c0, double2* q) { RC::load(d, (size_t)(K0 + max(min(c0 + lt, n - 1), 0)), q); };
  double2 q[RC::Q];
  ld(0, q);  // in flight with the CSR offsets and the tile's rows
  if (tid <= np) sptr[tid] = d.inc_ptr[p0 + tid] - K0;
  {
    const double2* v2 = reinterpret_cast<const double2*>(V + (size_t)p0 * 4 * R);
    for (int i = tid; i < np * 2 * R; i += 64 * W) xs[i] = v2[i];
  }
  __syncthreads();  // sptr, xs
  for (int c0 = 0; c0 < n; c0 += CH) {
    const int k = max(min(c0 + lt, n - 1), 0);
    // the other endpoint's row first (it needs only the record), so its
    // latency runs under the owning pose's search
    const int2 in = RC::inc(q);
    const int o = in.x;
    const bool tail = (in.y >> 31) & 1;
    const double2* o2 =
        reinterpret_cast<const double2*>((o >= 0) ? V + (size_t)o * 4 * R : pub + (size_t)(-1 - o) * 4 * R);
    double2 vo2[2 * R];
#pragma unroll
    for (int i = 0; i < 2 * R; ++i) vo2[i] = o2[i];
    int lo = 0, hi = np;  // owning pose: sptr[lo] <= k < sptr[lo + 1]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (sptr[mid] <= k) lo = mid;
      else hi = mid;
    }
    const double2* s2 = xs + lo * 2 * R;
    Edge E;
    RC::edge(q, E);
    if (tid < CH && c0 + tid < n) {
#pragma unroll
      for (int a = 0; a < R; ++a) {
        const double2 sa = s2[2 * a], sb = s2[2 * a + 1];  // own row, from LDS
        const double vs[4] = {sa.x, sa.y, sb.x, sb.y};
        const double vo[4] = {vo2[2 * a].x, vo2[2 * a].y, vo2[2 * a + 1].x, vo2[2 * a + 1].y};
        double h[4] = {0.0, 0.0, 0.0, 0.0};
        const double c = incidence_row(E, tail, vs, vo, h);
        csum += (o < 0) ? c : 0.5 * c;
        store4(Cs + (tid * R + a) * 4, h);
      }
    }
    asm volatile("" ::: "memory");
    ld(c0 + CH, q);
    lds_barrier();
    if (L.valid) {
      const int j0 = max(sptr[pl], c0) - c0, j1 = min(sptr[pl + 1], c0 + CH) - c0;
#pragma unroll 4
      for (int j = j0; j < j1; ++j) {
        double h[4];
        load4(Cs + (j * R + L.a) * 4, h);
        acc[0] += h[0]; acc[1] += h[1]; acc[2] += h[2]; acc[3] += h[3];
      }
    }
    lds_barrier();
  }
  *cost += csum;
}

// Trial cost f(Xt), one lane per incidence of the tile; only the owner
// incidence of an edge contributes (the tail of a local edge, the local end of
// a shared one), so each edge of the local problem counts once. The owner lane
// reads its own row from LDS and the other endpoint's row, and sums the r
// rows' residual terms: no per-pose reduction.
template <int R, int RW>
__device__ __forceinline__ double inc_owner_cost(const Dev& d, const Lane& L, const double* V, const double* pub,
                                                 char* smem) {
  using SM = SmemC<R>;
  using RC = Rec<RW>;
  int* sptr = reinterpret_cast<int*>(smem + SM::ptr_off);
  double2* xs = reinterpret_cast<double2*>(smem + SM::x_off);
  const int tid = threadIdx.x;
  const int p0 = L.p0, np = L.np, K0 = L.k0, n = L.n;
  if (tid <= np) sptr[tid] = d.inc_ptr[p0 + tid] - K0;
  {
    const double2* v2 = reinterpret_cast<const double2*>(V + (size_t)p0 * 4 * R);
    for (int i = tid; i < np * 2 * R; i += BLOCK) xs[i] = v2[i];
  }
  __syncthreads();
  double cost = 0.0;
  for (int k = tid; k < n; k += BLOCK) {
    double2 q[RC::Q];
    RC::load(d, (size_t)(K0 + k), q);
    const int2 in = RC::inc(q);
    const int o = in.x;
    const bool tail = (in.y >> 31) & 1;
    if (o >= 0 && !tail) continue;  // the head of a local edge: its tail counts it
    // the other endpoint's row first: its latency runs under the owning pose's search
    const double2* o2 =
        reinterpret_cast<const double2*>((o >= 0) ? V + (size_t)o * 4 * R : pub + (size_t)(-1 - o) * 4 * R);
    double2 vs2[2 * R], vo2[2 * R];
#pragma unroll
    for (int i = 0; i < 2 * R; ++i) vo2[i] = o2[i];
    int lo = 0, hi = np;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (sptr[mid] <= k) lo = mid;
      else hi = mid;
    }
    const double2* s2 = xs + lo * 2 * R;
#pragma unroll
    for (int i = 0; i < 2 * R; ++i) vs2[i] = s2[i];
    Edge E;
    RC::edge(q, E);
    double c = 0.0;
#pragma unroll
    for (int a = 0; a < R; ++a) {
      const double vs[4] = {vs2[2 * a].x, vs2[2 * a].y, vs2[2 * a + 1].x, vs2[2 * a + 1].y};
      const double vo[4] = {vo2[2 * a].x, vo2[2 * a].y, vo2[2 * a + 1].x, vo2[2 * a + 1].y};
      double dummy[4] = {0.0, 0.0, 0.0, 0.0};
      c += incidence_row(E, tail, vs, vo, dummy);
    }
    cost += c;
  }
  return cost;
}

// -------------------------------------------------- per-robot reductions --
// Each tile reduces its NV values over the workgroup (wave sums, then the 4
// waves in order) and stores them as the tile's partials; the robot's sums are
// taken in tile order by whoever consumes them (robot_sum's fixed order):
// RM_LAUNCH: k_reduce, a one-workgroup-per-robot launch after the producing
// kernel, which then runs the RTR / tCG control logic; RM_CONSUMER: no
// reduction launch inside tCG — every workgroup of k_update reduces its robot's
// k_hess partials itself (and every workgroup of the next k_hess the k_update
// partials) in the same order and runs the control step on a private copy of
// the robot's state; the robot's first tile writes the state out,
// double-buffered (k_hess: ctl -> ctl2, k_update: ctl2 -> ctl), so no
// workgroup reads a state another one of the same launch writes. The round's
// other reductions are folded too (gradient -> first k_hess, last update ->
// k_cost, trial cost -> k_commit), so a consumer-form round has no k_reduce
// launch (12.5k poses 167.7 -> 161.4 us per round, profiles/r02/small_round/3_*).
// Measured on configs[3] (profiles/r02/ab_red): at 100k poses the consumer
// form loses (k_hess 41.2 us and k_update 22.7 us against 32.4 + 19.8 us plus
// two 4.6 us k_reduce launches: each workgroup of the latency-bound gather
// waits for its robot's sums), so RM_LAUNCH stays the form above 80k poses per
// GPU. Two more forms were measured and removed in round 3: agent-scope
// tickets in the producing launch (k_hess 47.5 vs 39.9 us: the ticket keeps
// each workgroup resident for microseconds after its work) and a half form
// with only the update's k_reduce kept (0.814 / 0.839 vs 0.817 / 0.839 ms per
// round: no gain).
// (enum RedMode { RM_LAUNCH, RM_CONSUMER }: pgo_host.h)

template <int KIND, int NV, int RM, typename Store>
__device__ __forceinline__ void finish_tile(const Dev& d, const Lane& L, const double* vals, char* smem_red,
                                            Store&& store) {
  double* lds = reinterpret_cast<double*>(smem_red);
  static_assert(NV <= NPART && WAVES == 4, "reduction area");
#pragma unroll
  for (int s = 0; s < NV; ++s) {
    const double w = wave_sum(vals[s]);
    if ((threadIdx.x & 63) == 0) lds[s * WAVES + (threadIdx.x >> 6)] = w;
  }
  __syncthreads();
  constexpr bool two = RM == RM_CONSUMER && (KIND == RED_HESS || KIND == RED_UPDATE);
  static_assert(!two || NV <= 2, "consumer partials");
  if (threadIdx.x == 0) {  // 2-wide partials for the consumer launch, else NPART-wide for k_reduce
    double* dst = two ? (KIND == RED_HESS ? d.part_h : d.part_u) + (size_t)L.tile * 2 : d.part + (size_t)L.tile * NPART;
#pragma unroll
    for (int s = 0; s < NV; ++s) {
      double t = 0.0;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) t += lds[s * WAVES + w];
      dst[s] = t;
    }
  }
  store();
}

// The tCG decisions after the Hess-vec and after the update, shared by
// control_on and by RM_CONSUMER's workgroups (which evaluate them from the
// robot's state without a copy of it); contraction off so every call site
// rounds alike.
struct HessStep {
  double alpha, e_Pe_new, coef;
  int boundary, stop;
};
__device__ __forceinline__ HessStep hess_step(double z_r, double e_Pe, double e_Pd, double d_Pd, double Delta,
                                              double d_Hd) {
#pragma clang fp contract(off)
  HessStep h;
  h.alpha = z_r / d_Hd;
  h.e_Pe_new = e_Pe + 2.0 * h.alpha * e_Pd + h.alpha * h.alpha * d_Pd;
  const double D2 = Delta * Delta;
  h.boundary = (d_Hd <= 0.0 || h.e_Pe_new >= D2) ? 1 : 0;
  h.stop = d_Hd <= 0.0 ? KMX_TCG_NEGATIVE_CURVATURE : KMX_TCG_EXCEEDED_TR;
  h.coef = h.boundary ? (-e_Pd + sqrt(e_Pd * e_Pd + d_Pd * (D2 - e_Pe))) / d_Pd : h.alpha;
  return h;
}
struct UpdStep {
  int done, stop;
  double beta;
};
__device__ __forceinline__ UpdStep upd_step(int mode, double r_stop, int lin_stop, double z_r, int tcg_iter, double rr,
                                            double zr_new, const Params& P) {
#pragma clang fp contract(off)
  UpdStep u;
  u.done = 0;
  u.stop = KMX_TCG_MAX_ITER;
  u.beta = 0.0;
  if (mode == MODE_BOUNDARY) {
    u.done = 1;
    u.stop = -1;  // keep the boundary reason
    return u;
  }
  const double norm_r = sqrt(rr);
  if (norm_r <= r_stop) {
    u.done = 1;
    u.stop = lin_stop ? KMX_TCG_LINEAR : KMX_TCG_SUPERLINEAR;
  } else if (tcg_iter >= P.tcg_max) {
    u.done = 1;
    u.stop = KMX_TCG_MAX_ITER;
  } else {
    u.beta = zr_new / z_r;
  }
  return u;
}

// The RTR / tCG scalar logic of robot l after a reduction of `kind`, applied
// to c. `side`: perform the side effects (team status, counters) — exactly one
// caller per robot and reduction does.
__device__ __forceinline__ void control_core(Ctl& c, const Dev& d, int l, int kind, const double* tot, int R_,
                                             bool side) {
  const Params& P = d.p;
  if (kind == RED_GRAD) {
    const double f = tot[0], gn = sqrt(tot[1]);
    if (c.rtr_iter == 0) { c.f_init = f; c.gn_init = gn; }
    c.f_cur = f;
    c.f_final = f;
    c.commit = 0;
    if (gn < P.gn_tol) {  // no step: the iterate does not change
      c.phase = PH_IDLE;
      c.tcg_stop = KMX_TCG_SKIPPED;
      c.tcg_iter = 0;
      c.accepted = 0;
      c.skipped = 1;
      if (side) d.relc[l] = (c.rtr_iter == 0) ? 0.0 : c.rel_change;
    } else if (P.rgd) {  // RGD: eta = -s z (z = precon(g), from k_grad), straight to the step
      c.phase = PH_STEP;
      c.tcg_iter = 0;
      c.tcg_stop = KMX_TCG_NONE;
      c.coef = -P.rgd_step;
      if (side && c.rtr_iter == 0) {
        atomicAdd(&d.cnt->edges_iters, (unsigned long long)d.m_robot[l]);
        atomicAdd(&d.cnt->block_updates, 1ull);
      }
    } else {
      c.phase = PH_TCG;
      c.tcg_iter = 0;
      c.norm_r0 = gn;
      {  // the residual stop of this tCG (upd_step), formed once instead of at every step
        const double pw = pow(gn, P.theta);
        c.r_stop = gn * fmin(pw, P.kappa);
        c.lin_stop = (P.kappa < pw) ? 1 : 0;
      }
      c.z_r = tot[2];
      c.d_Pd = tot[2];
      c.e_Pd = 0.0;
      c.e_Pe = 0.0;
      c.beta = 0.0;
      c.tcg_stop = KMX_TCG_MAX_ITER;
      if (side && c.rtr_iter == 0) {
        atomicAdd(&d.cnt->edges_iters, (unsigned long long)d.m_robot[l]);
        atomicAdd(&d.cnt->block_updates, 1ull);
      }
    }
  } else if (kind == RED_HESS) {
    const double d_Hd = tot[0];
    const HessStep hs = hess_step(c.z_r, c.e_Pe, c.e_Pd, c.d_Pd, c.Delta, d_Hd);
    if (side) d.coefh[(size_t)l * P.tcg_max + min(c.tcg_iter, P.tcg_max - 1)] = hs.coef;  // delta_k's eta coefficient
    c.tcg_iter += 1;
    c.hessvecs += 1;
    if (side) {
      atomicAdd(&d.cnt->hessvecs, 1ull);
      atomicAdd(&d.cnt->hess_alg_bytes, 128.0 * (double)d.m_robot[l] + 2.0 * 8.0 * R_ * 4.0 * (double)d.n_robot[l]);
    }
    if (hs.boundary) {
      c.coef = hs.coef;
      c.mode = MODE_BOUNDARY;
      c.tcg_stop = hs.stop;
    } else {
      c.alpha = hs.alpha;
      c.coef = hs.coef;
      c.e_Pe = hs.e_Pe_new;
      c.mode = MODE_INTERIOR;
    }
  } else if (kind == RED_UPDATE) {
    const double zr_new = tot[1];
    const UpdStep u = upd_step(c.mode, c.r_stop, c.lin_stop, c.z_r, c.tcg_iter, tot[0], zr_new, P);
    if (u.done) {
      if (u.stop >= 0) c.tcg_stop = u.stop;
      c.phase = PH_STEP;
    } else {
      const double beta = u.beta;
      c.e_Pd = beta * (c.e_Pd + c.alpha * c.d_Pd);
      c.d_Pd = zr_new + beta * beta * c.d_Pd;
      c.z_r = zr_new;
      c.beta = beta;
    }
  } else if (P.rgd) {  // RED_COST after an RGD step: always accepted, one step per block update
    c.rho = 0.0;
    c.accepted = 1;
    c.commit = 1;
    c.f_final = tot[0];
    c.chg_acc += tot[3];
    c.rtr_iter += 1;
    c.phase = PH_IDLE;
    c.rel_change = sqrt(c.chg_acc / (double)d.n_robot[l]);
    if (side) d.relc[l] = c.rel_change;
  } else {  // RED_COST: tot[0] = f(Xt), tot[2] = 2 m(eta), tot[3] = ||Xt - X||^2
    const double ft = tot[0];
    const double model_dec = -0.5 * tot[2];
    const double rho = (model_dec > 0.0) ? (c.f_cur - ft) / model_dec : -1.0;
    const bool boundary = (c.tcg_stop == KMX_TCG_NEGATIVE_CURVATURE || c.tcg_stop == KMX_TCG_EXCEEDED_TR);
    if (!(rho >= 0.25)) c.Delta *= 0.25;
    else if (rho > 0.75 && boundary) c.Delta = fmin(2.0 * c.Delta, P.Delta_max);
    c.rho = rho;
    if (rho > P.accept_rho) {
      c.accepted = 1;
      c.commit = 1;
      c.f_final = ft;
      c.chg_acc += tot[3];
    } else {
      c.accepted = 0;
      c.commit = 0;
      c.f_final = c.f_cur;
    }
    c.rtr_iter += 1;
    c.phase = (c.rtr_iter < P.rtr_iters) ? PH_START : PH_IDLE;
    c.retracted = 0;
    c.rel_change = sqrt(c.chg_acc / (double)d.n_robot[l]);
    if (side && c.phase == PH_IDLE) d.relc[l] = c.rel_change;  // the team status of dpgo's getStatus
  }
}
// Out of line: inlined, it costs the 128-VGPR gather kernels spills.
__device__ void control_on(Ctl& c, const Dev& d, int l, int kind, const double* tot, int R_, bool side) {
  control_core(c, d, l, kind, tot, R_, side);
}

// The robot's state from a workgroup's LDS copy to global memory, one 8-byte
// word per lane of wave 0's first 32 (k_reduce's write-back). A single thread
// that assigns the struct holds its 256 B in 64 VGPRs at once, which set the
// consumer k_update's register count. `retracted`: the copy with that flag set.
__device__ __forceinline__ void ctl_publish(Ctl* dst, const Ctl& cs, bool retracted) {
  constexpr int CW = sizeof(Ctl) / 8;
  constexpr int RWORD = offsetof(Ctl, retracted) / 8;
  static_assert(CW <= 64 && offsetof(Ctl, retracted) % 8 == 0, "one word per lane; retracted is a low half");
  if (threadIdx.x < CW) {
    double w = reinterpret_cast<const double*>(&cs)[threadIdx.x];
    if (retracted && threadIdx.x == RWORD) w = __hiloint2double(__double2hiint(w), 1);
    reinterpret_cast<double*>(dst)[threadIdx.x] = w;
  }
}

// RM_LAUNCH: one workgroup per robot reduces the robot's tile partials in
// tile order and runs the control logic (after k_update it also reports the
// robot's tCG progress to the host).
constexpr int RBLOCK = 256;  // k_reduce: one workgroup per robot (1024 threads measured slower: 6.3 vs 4.6 us)
static_assert(RBLOCK == BLOCK, "robot_sum runs in k_reduce and in the tCG kernels");
// Sum of NS partials (row stride `stride`) over tiles [t0, t1) of a robot by
// the whole workgroup: two tiles per thread in flight (512 tiles, ~24k poses
// per robot, in one round trip), tile order within a thread, then the wave
// sums and the 4 waves in order; every thread gets the totals. The one order
// used by k_reduce and by RM_CONSUMER's tCG kernels. lds: >= NS * 4 doubles.
template <int NS>
__device__ __forceinline__ void robot_sum(const double* part, int stride, int t0, int t1, double* lds,
                                          double tot[NPART]) {
  constexpr int RW_ = RBLOCK / 64;
  double v[NPART] = {0.0, 0.0, 0.0, 0.0};
  for (int tb = t0; tb < t1; tb += 2 * RBLOCK) {
    double a[2][NS];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int t = min(tb + (int)threadIdx.x + u * RBLOCK, t1 - 1);
      if constexpr (NS == 4) {
        const double2* p2 = reinterpret_cast<const double2*>(part + (size_t)t * stride);
        const double2 x = p2[0], y = p2[1];
        a[u][0] = x.x; a[u][1] = x.y; a[u][NS - 2] = y.x; a[u][NS - 1] = y.y;
      } else {
        const double2 x = *reinterpret_cast<const double2*>(part + (size_t)t * stride);
        a[u][0] = x.x;
        if constexpr (NS > 1) a[u][NS - 1] = x.y;
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u)
      if (tb + (int)threadIdx.x + u * RBLOCK < t1) {
#pragma unroll
        for (int k = 0; k < NS; ++k) v[k] += a[u][k];
      }
  }
  __syncthreads();  // lds may still be read by an earlier user
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const double w = wave_sum(v[k]);
    if ((threadIdx.x & 63) == 0) lds[k * RW_ + (threadIdx.x >> 6)] = w;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NPART; ++k) {
    double acc = 0.0;
    if (k < NS) {
#pragma unroll
      for (int w = 0; w < RW_; ++w) acc += lds[k * RW_ + w];
    }
    tot[k] = acc;
  }
}

// robot_sum in two halves, so the partial loads can be in flight during other
// work: issue() loads a robot's <= U * RBLOCK tiles into registers (larger
// robots fall back to robot_sum in finish()); finish() adds them in
// robot_sum's order (a thread's tiles in tile order, then the wave sums and
// the waves in order: the same sums for any U).
// NS <= 2: 2-wide partials (part_h / part_u); NS = 3, 4: d.part (stride NPART).
// A tile partial pair part[i], part[i + 1] (i even): one 16-B load.
__device__ __forceinline__ double2 ldpart(const double* part, size_t i) {
  return *reinterpret_cast<const double2*>(part + i);
}

template <int NS, int U = 2>
struct RobotSum {
  double a[U][NS];
  int t0, t1;
  __device__ __forceinline__ void issue(const double* part, int stride, int t0_, int t1_) {
    t0 = t0_;
    t1 = t1_;
    if (t1 - t0 > U * RBLOCK) return;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int t = min(t0 + (int)threadIdx.x + u * RBLOCK, t1 - 1);
      const size_t pt = (size_t)t * stride;
      const double2 x = ldpart(part, pt);
      if constexpr (NS > 2) {
        const double2 y = ldpart(part, pt + 2);
        a[u][2] = y.x;
        if constexpr (NS > 3) a[u][3] = y.y;
      }
      a[u][0] = x.x;
      if constexpr (NS > 1) a[u][1] = x.y;
    }
  }
  __device__ __forceinline__ void finish(const double* part, int stride, double* lds, double tot[NPART]) {
    static_assert(NS <= NPART, "partials");
    if (t1 - t0 > U * RBLOCK) {
      robot_sum<(NS > 2 ? NPART : NS)>(part, stride, t0, t1, lds, tot);
      if constexpr (NS == 3) tot[3] = 0.0;
      return;
    }
    constexpr int RW_ = RBLOCK / 64;
    double v[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) v[k] = 0.0;
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (t0 + (int)threadIdx.x + u * RBLOCK < t1 && threadIdx.x < RBLOCK) {
#pragma unroll
        for (int k = 0; k < NS; ++k) v[k] += a[u][k];
      }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const double w = wave_sum(v[k]);
      if ((threadIdx.x & 63) == 0 && threadIdx.x < RBLOCK) lds[k * RW_ + (threadIdx.x >> 6)] = w;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NPART; ++k) {
      double acc = 0.0;
      if (k < NS) {
#pragma unroll
        for (int w = 0; w < RW_; ++w) acc += lds[k * RW_ + w];
      }
      tot[k] = acc;
    }
  }
};

// The robot's state (256 B, into LDS) and its tile partials are loaded
// together at the start, the control logic runs on the LDS copy and 32 lanes
// write it back: no global round trip is serialised behind another.
__global__ __launch_bounds__(RBLOCK) void k_reduce(Dev d, int first, int kind, int R_, HostStatus* hs,
                                                  unsigned long long seq, int slot, const double* src) {
  constexpr int RW_ = RBLOCK / 64;
  constexpr int CW = sizeof(Ctl) / 8;
  static_assert(CW <= RBLOCK, "Ctl copy");
  __shared__ double lds[NPART * RW_];
  __shared__ Ctl cs;
  const int l = first + blockIdx.x;  // the launch's robots: [first, first + grid)
  if (threadIdx.x < CW)
    reinterpret_cast<double*>(&cs)[threadIdx.x] = reinterpret_cast<const double*>(d.ctl + l)[threadIdx.x];
  const int t0 = d.rtile0[l], t1 = d.rtile0[l + 1];
  double tot[NPART];
  if (src) {  // RM_CONSUMER's 2-wide partials
    RobotSum<2> rs;
    rs.issue(src, 2, t0, t1);
    rs.finish(src, 2, lds, tot);  // (its barriers also publish cs)
  } else {
    RobotSum<NPART> rs;
    rs.issue(d.part, NPART, t0, t1);
    rs.finish(d.part, NPART, lds, tot);
  }
  const int ph = cs.phase;
  bool act = false;
  if (kind == RED_GRAD) act = ph == PH_START;
  if (kind == RED_HESS || kind == RED_UPDATE) act = ph == PH_TCG;
  if (kind == RED_COST) act = ph == PH_STEP;
  if (threadIdx.x == 0) {
    if (act) {
      const int ns = kind == RED_GRAD ? 3 : kind == RED_HESS ? 1 : kind == RED_UPDATE ? 2 : 4;
#pragma unroll
      for (int s = 0; s < NPART; ++s) tot[s] = s < ns ? tot[s] : 0.0;
      control_on(cs, d, l, kind, tot, R_, true);
      if (kind == RED_HESS && slot >= 0) atomicAdd(d.hv_launch + slot, 1);
    }
    if (hs) post_status(hs, l, seq, act && cs.phase == PH_TCG);
  }
  if (!act) return;
  __syncthreads();
  if (threadIdx.x < CW)
    reinterpret_cast<double*>(d.ctl + l)[threadIdx.x] = reinterpret_cast<const double*>(&cs)[threadIdx.x];
}

#define KMX_SMEM extern __shared__ __attribute__((aligned(16))) char smem[]

// Minimum waves per SIMD of the gather kernels: 4 at r <= 5 (128 VGPRs); the
// r >= 6 rows need more registers.
template <int R>
struct LB {
  static constexpr int w = R <= 5 ? 4 : 2;
};

// Start of an RTR iteration: egrad (gather X with public neighbours), cost,
// S = sym(Y^T egrad_Y), g = P_Y(egrad), z = precon(g); partials f, |g|^2, <z,g>.
// The per-pose 4x4 blocks D_i and the preconditioner (k_precond's work, same
// expressions and order), also used by k_grad's gated prologue.
template <int RW>
__device__ __forceinline__ void pose_precond(const Dev& d, int pose) {
  // A: the preconditioner's blocks (kappa I for the rotation part, as in the
  // oracle); Dq: Q's exact diagonal block for the Hessian gather, which with
  // the full records (measurements off SO(3)) carries w kappa R R^T instead
  double A[16], Dq[16];
  for (int i = 0; i < 16; ++i) A[i] = Dq[i] = 0.0;
  for (int k = d.inc_ptr[pose]; k < d.inc_ptr[pose + 1]; ++k) {
    double2 q[Rec<RW>::Q];
    Rec<RW>::load(d, (size_t)k, q);
    Edge E;
    Rec<RW>::edge(q, E);
    const bool tail = (Rec<RW>::inc(q).y >> 31) & 1;
    const double wk = E.wk, wt = E.wt;
    const double* tt = E.t;
    if (tail) {
      for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) {
          A[i * 4 + j] += wt * tt[i] * tt[j] + (i == j ? wk : 0.0);
          const double rr = (RW == 10) ? (i == j ? 1.0 : 0.0)
                                       : E.R[i * 3 + 0] * E.R[j * 3 + 0] + E.R[i * 3 + 1] * E.R[j * 3 + 1] +
                                             E.R[i * 3 + 2] * E.R[j * 3 + 2];
          Dq[i * 4 + j] += wt * tt[i] * tt[j] + wk * rr;
        }
        A[i * 4 + 3] += wt * tt[i];
        A[3 * 4 + i] += wt * tt[i];
        Dq[i * 4 + 3] += wt * tt[i];
        Dq[3 * 4 + i] += wt * tt[i];
      }
      A[15] += wt;
      Dq[15] += wt;
    } else {
      A[0] += wk; A[5] += wk; A[10] += wk; A[15] += wt;
      Dq[0] += wk; Dq[5] += wk; Dq[10] += wk; Dq[15] += wt;
    }
  }
  {
    double* Dp = d.hD + SYM4 * (size_t)pose;
    int j = 0;
    for (int a = 0; a < 4; ++a)
      for (int b = a; b < 4; ++b) Dp[j++] = Dq[a * 4 + b];
  }
  for (int j = 0; j < 4; ++j) A[j * 5] += d.p.shift;
  double Lm[16], Li[16];
  for (int i = 0; i < 16; ++i) { Lm[i] = 0.0; Li[i] = 0.0; }
  for (int j = 0; j < 4; ++j) {
    double s = A[j * 4 + j];
    for (int k = 0; k < j; ++k) s -= Lm[j * 4 + k] * Lm[j * 4 + k];
    Lm[j * 4 + j] = sqrt(s);
    for (int ii = j + 1; ii < 4; ++ii) {
      double t = A[ii * 4 + j];
      for (int k = 0; k < j; ++k) t -= Lm[ii * 4 + k] * Lm[j * 4 + k];
      Lm[ii * 4 + j] = t / Lm[j * 4 + j];
    }
  }
  for (int c = 0; c < 4; ++c)
    for (int ii = 0; ii < 4; ++ii) {
      double s = (ii == c) ? 1.0 : 0.0;
      for (int k = c; k < ii; ++k) s -= Lm[ii * 4 + k] * Li[k * 4 + c];
      Li[ii * 4 + c] = (ii < c) ? 0.0 : s / Lm[ii * 4 + ii];
    }
  double* Pi = d.Pinv + SYM4 * (size_t)pose;  // Li^T Li: symmetric (upper triangle)
  int j = 0;
  for (int x = 0; x < 4; ++x)
    for (int y = x; y < 4; ++y) {
      double s = 0.0;
      for (int k = 0; k < 4; ++k) s += Li[k * 4 + x] * Li[k * 4 + y];
      Pi[j++] = s;
    }
}

// gated: the first gradient of a round whose begin launch may have re-weighted
// (the k_precond launch folded in): the workgroup of global tile 0 commits the
// GNC state (of the launches over robot groups' tiles, only the one that holds
// tile 0 does; no kernel between a round's k_begin and its final k_commit
// reads d.gnc) and, when
// the begin fired, every tile rebuilds D_i and the preconditioner of its own
// poses (only its own incidence records are read) before the phase test, so
// idle robots are rebuilt too. The writes are read back by the tile's own
// lanes after the workgroup barrier (one CU: workgroup-scope visibility).
template <int R, int RW, int RM>
__device__ __forceinline__ void body_grad(const Dev& d, int gated, char* smem) {
  const Lane L = lane_map<R>(d);
  if (gated) {
    if (L.tile == 0 && threadIdx.x == 0) store_gnc(d.gnc, load_gnc(d.gnc_next));
    if (d.gnc_next->fired) {
      const int np = L.np, p0 = L.p0;
      for (int t = threadIdx.x; t < np; t += blockDim.x) pose_precond<RW>(d, p0 + t);
      __syncthreads();
    }
  }
  if (d.ctl[L.l].phase != PH_START) return;
  double y[4] = {0, 0, 0, 0}, G[4], cost = 0.0;
  hinc_grad<R, RW>(d, L, d.X, d.pub, G, &cost, smem);
  if (L.valid) load4(d.X + (size_t)L.pose * 4 * R + 4 * L.a, y);
  // D_i - S_i for k_hess: the pose's D_i (five 16-B parts; a gated re-weight's
  // rebuild above is this workgroup's own writes) is loaded here, spread over its
  // lanes (parts a and a + r), so its latency runs under the group operations
  constexpr int NDP = R >= 5 ? 1 : 2;
  double2 dpart[NDP];
  {
    const double2* Dp2 = reinterpret_cast<const double2*>(d.hD + SYM4 * (size_t)L.pose);
#pragma unroll
    for (int u = 0; u < NDP; ++u) {
      const int i = L.a + u * R;
      dpart[u] = (L.valid && i < 5) ? Dp2[i] : make_double2(0.0, 0.0);
    }
  }
  double S[9], gr[4], zr[4];
  double* scr = reinterpret_cast<double*>(smem);  // the chunk buffer is free after the gather's last barrier
  group_symYtG<R, true>(y, G, L.base, S, scr);
#pragma unroll
  for (int c = 0; c < 3; ++c) gr[c] = G[c] - (y[0] * S[0 * 3 + c] + y[1] * S[1 * 3 + c] + y[2] * S[2 * 3 + c]);
  gr[3] = G[3];
  group_precon<R, true>(d, L.pose, L.valid, y, gr, L.base, zr, scr);
  double vals[3] = {cost, 0.0, 0.0};  // cost is accumulated on every incidence lane
  if (L.valid) {
    vals[1] = gr[0] * gr[0] + gr[1] * gr[1] + gr[2] * gr[2] + gr[3] * gr[3];
    vals[2] = zr[0] * gr[0] + zr[1] * gr[1] + zr[2] * gr[2] + zr[3] * gr[3];
  }
  finish_tile<RED_GRAD, 3, RM>(d, L, vals, smem + SmemHG<R>::red_off, [&]() {
    if (!L.valid) return;
    const size_t o = (size_t)L.pose * 4 * R + 4 * L.a;
    store4(d.g + o, gr);  // r = g at the start of tCG: k_update's first step reads g
    store4(d.z + o, zr);
    if (L.a == 0) {
      double* Sp = d.S + 6 * (size_t)L.pose;
      Sp[0] = S[0]; Sp[1] = S[1]; Sp[2] = S[2]; Sp[3] = S[4]; Sp[4] = S[5]; Sp[5] = S[8];
    }
    // part i holds SYM4 entries 2i, 2i + 1: (00, 01), (02, 03), (11, 12), (13, 22), (23, 33)
    double2* Fp2 = reinterpret_cast<double2*>(d.hDS + SYM4 * (size_t)L.pose);
#pragma unroll
    for (int u = 0; u < NDP; ++u) {
      const int i = L.a + u * R;
      if (i < 5) {
        const double sx = i == 0 ? S[0] : i == 1 ? S[2] : i == 2 ? S[4] : 0.0;
        const double sy = i == 0 ? S[1] : i == 2 ? S[5] : i == 3 ? S[8] : 0.0;
        Fp2[i] = make_double2(dpart[u].x - sx, dpart[u].y - sy);
      }
    }
  });
}

// eta = sum_k coef_k delta_k over a tCG's T directions, in step order (the
// first F were folded into d.eta by the Hess-vec launches), added to et. LAST:
// the coefficient of direction T - 1 is clast (a k_step that ends the tCG
// decided it in the same launch whose writer stores it to coefh).
// In two halves, so that a caller that learns clast late (the last k_update)
// has the rows in flight before it: issue() loads, finish() adds.
struct EtaRows {
  double dd[DHMAX][4];
  int F;
  __device__ __forceinline__ void issue(const Dev& d, size_t o, int T, double et[4]) {
    const int dhn = d.dhn;
    F = T > 0 ? (T - 1) / dhn * dhn : 0;
    if (F > 0) load4(d.eta + o, et);
#pragma unroll
    for (int i = 0; i < DHMAX; ++i)
      if (F + i < T) load4(d.dh + (size_t)i * d.vec + o, dd[i]);
  }
  template <bool LAST>
  __device__ __forceinline__ void finish(const Dev& d, int l, int T, double clast, double et[4]) const {
    const double* ch = d.coefh + (size_t)l * d.p.tcg_max;
#pragma unroll
    for (int i = 0; i < DHMAX; ++i)
      if (F + i < T) {
        const double cj = (LAST && F + i == T - 1) ? clast : ch[F + i];
#pragma unroll
        for (int k = 0; k < 4; ++k) et[k] += cj * dd[i][k];
      }
  }
};
template <bool LAST>
__device__ __forceinline__ void eta_rows(const Dev& d, int l, size_t o, int T, double clast, double et[4]) {
  EtaRows e;
  e.issue(d, o, T, et);
  e.finish<LAST>(d, l, T, clast, et);
}

// The trial point Xt = R_X(eta) of the lane's row, and the tile's partials
// m(eta) = 1/2 <eta, g + r> (as 2 m) and ||Xt - X||^2 into d.part slots 2, 3
// (k_cost adds the cost in slot 0). Every lane of the workgroup calls it.
template <int R>
__device__ __forceinline__ void trial_rows(const Dev& d, const Lane& L, size_t o, const double x[4],
                                           const double gg[4], const double rr[4], const double et[4], char* smem) {
  double xt[4];
  group_retract<R>(x, et, L.base, xt);
  double vals[2] = {0.0, 0.0};
  if (L.valid) {
    store4(d.Xt + o, xt);
    double m = 0.0, ch = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      m += et[k] * (gg[k] + rr[k]);
      const double dd = xt[k] - x[k];
      ch += dd * dd;
    }
    vals[0] = m;
    vals[1] = ch;
  }
  double* lds = reinterpret_cast<double*>(smem);
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const double w = wave_sum(vals[s]);
    if ((threadIdx.x & 63) == 0) lds[s * WAVES + (threadIdx.x >> 6)] = w;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      double t = 0.0;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) t += lds[s * WAVES + w];
      d.part[(size_t)L.tile * NPART + 2 + s] = t;
    }
  }
}

// tCG step, part 1 (the dominant kernel): Hz = Hess(z) by gather; then by
// linearity delta = -z + beta delta_old, Hdelta = -Hz + beta Hdelta_old;
// partial <delta, Hdelta>. delta_k is kept for k_retract's eta (Dev::dh).
// Hz and Hdelta are kept BEFORE the tangent projection (Hz^ = H z - z S;
// the Riemannian H delta = P_Y(H delta^)): projection is linear, so the
// recurrence holds for the unprojected rows, and <delta, Hdelta^> equals
// <delta, P_Y(Hdelta^)> for a tangent delta (Y^T delta skew, Y sym(.) S
// symmetric). k_update, which loads Y anyway, projects; this kernel then
// reads no X row (16 MB per launch at configs[3]: VERDICT r4 item 2).
// Which k_hess instantiations prefetch the next chunk's rows (hinc_gather_src's
// PF); every one takes the epilogue batch on the last chunk. Compact records
// only (see hinc_gather_src), and not the launched form at r < 5: its 86-92
// VGPRs give five workgroups per CU there, with the rows in flight four.
template <int R, int RW, int RM>
struct HessPF {
  static constexpr bool rows = RW == 10 && (R >= 5 || RM == RM_CONSUMER);
};
// GRAD, EARLY (consumer form; the launched form has one body, <false, false>):
// whether this is the host's launch 0 of a tCG loop, and whether the stop
// decision runs before the gather or after it. The host knows both when it
// enqueues, and a body that carries both robot sums and both gathers does not
// fit 128 VGPRs next to the prefetched rows.
template <int R, int RW, int RM, bool GRAD, bool EARLY>
__device__ __forceinline__ void body_hess(const Dev& d, int gated, int slot, HostStatus* hs,
                                          unsigned long long seq, char* smem) {
  static_assert(RM == RM_CONSUMER || (!GRAD && !EARLY), "the launched form has one body");
  const Lane L = lane_map<R>(d);
  int tcg_iter;
  double beta;
  double y[4] = {0, 0, 0, 0}, zs[4] = {0, 0, 0, 0}, H[4];
  const size_t o = (size_t)L.pose * 4 * R + 4 * L.a;
  // every row the epilogue needs in one batch: the own z row, D_i - S_i (the
  // diagonal block with the tangent correction -z S folded in; its five parts
  // stay as loaded until use), delta_old and H delta_old. No address depends
  // on the gather or on the decision, only on tcg_iter, so the gather issues
  // the batch on the tile's last chunk (hinc_gather_src's `epi`) and it flies
  // under the last LDS hand-off and pose sums.
  const int dhn = d.dhn;
  double dold[4] = {0, 0, 0, 0}, hold[4] = {0, 0, 0, 0};
  double2 dg[5];
  bool first;
  auto epi = [&]() {
    if (L.valid) {
#if KMX_HESS_PROBE & 2  // traffic attribution build: no own-row / diagonal-block loads
      for (int k = 0; k < 4; ++k) zs[k] = 1e-3 * k;
      for (int c = 0; c < 5; ++c) dg[c] = make_double2(c == 0 || c == 2 ? 1.0 : 0.0, c >= 3 ? 1.0 : 0.0);  // I
#else
      load4(d.z + o, zs);
      const double2* p2 = reinterpret_cast<const double2*>(d.hDS + SYM4 * (size_t)L.pose);
#pragma unroll
      for (int c = 0; c < 5; ++c) dg[c] = p2[c];
#endif
      if (!first) {
        load4(d.dh + (size_t)((tcg_iter - 1) % dhn) * d.vec + o, dold);
        load4(d.hd + o, hold);
      }
    }
  };
  if constexpr (RM == RM_CONSUMER) {
    // the previous step's k_update partials give this robot's control step
    // after the update (stop test, beta); the partial loads are in flight with
    // the gather's first records, and the decision comes before the rows are
    // gathered (a stopped robot's tiles leave without the gather). The robot's
    // first tile writes the state to ctl2 for k_update and reports tCG
    // progress to the host.
    __shared__ Ctl cs;
    __shared__ double rl[NPART * WAVES];
    const Ctl& c0 = d.ctl[L.l];
    const bool writer = L.tile == L.rt0;
    // the writer's working copy of the state, loaded by wave 0 at the start
    // (its lane 0 reads it after these in-order LDS writes of its own wave)
    if (writer && threadIdx.x < (int)(sizeof(Ctl) / 8))
      reinterpret_cast<double*>(&cs)[threadIdx.x] = reinterpret_cast<const double*>(&c0)[threadIdx.x];
    // GRAD (the host's launch 0 of a tCG loop): a robot in it is at
    // PH_START, the first step of the tCG, whose gradient reduction (k_grad's
    // partials) this launch also consumes in place of a k_reduce launch; later
    // launches find it in PH_TCG. With the early decision the robot sums'
    // loads go out before the state arrives; with the late one they go out
    // with the epilogue's batch (at kernel entry they would be live across
    // the whole gather).
    using RS = std::conditional_t<GRAD, RobotSum<3>, RobotSum<2>>;
    const double* const part = GRAD ? d.part : d.part_u;
    constexpr int stride = GRAD ? NPART : 2;
    RS rs;  // (four tiles per thread here: spills at 128 VGPRs)
    if constexpr (EARLY) rs.issue(part, stride, L.rt0, L.rt1);
    const int ph0 = c0.phase;  // written by an earlier launch: uniform
    const bool active = ph0 == (GRAD ? PH_START : PH_TCG);  // uniform: a tile never straddles robots
    auto idle = [&]() {
      if (writer && threadIdx.x == 0) {
        d.ctl2[L.l] = c0;
        if (hs) post_status(hs, L.l, seq, false);
      }
    };
    // early (below): the phase test waits in the decision, so the first
    // records load with the state instead of after it
    // gated (a launch the host expects to find robots stopped): the phase
    // test before the first records are issued, so a launch with nothing to
    // do reads its control words and leaves
    if (!active && (!EARLY || gated)) {
      idle();
      return;
    }
    tcg_iter = GRAD ? 0 : c0.tcg_iter;
    first = (tcg_iter == 0) || (KMX_HESS_PROBE & 4);  // (probe 4: no delta_old / Hdelta_old traffic)
    UpdStep u{0, 0, 0.0};
    // the decision runs while the first chunk's records are in flight and
    // before any row is gathered: a robot whose tCG stops here (or whose
    // gradient is below tolerance) skips the gather, and the host sees the
    // stop at the start of the launch
    auto decide = [&]() {
      if (!active) {
        idle();
        return false;
      }
      double tot[NPART] = {0.0, 0.0, 0.0, 0.0};
      rs.finish(part, stride, rl, tot);
      // every thread evaluates the decision; the first tile's thread 0 also
      // updates the robot's state (on an LDS copy: a private one would live in
      // scratch) and publishes it
      if constexpr (GRAD) u.done = sqrt(tot[1]) < d.p.gn_tol ? 1 : 0;  // control_on's RED_GRAD test
      else u = upd_step(c0.mode, c0.r_stop, c0.lin_stop, c0.z_r, c0.tcg_iter, tot[0], tot[1], d.p);
      if (writer && threadIdx.x == 0) {
        control_on(cs, d, L.l, GRAD ? RED_GRAD : RED_UPDATE, tot, R, true);
        d.ctl2[L.l] = cs;
        if (hs) post_status(hs, L.l, seq, cs.phase == PH_TCG);
      }
      return !u.done;
    };
    // early (small problems): decide before the gather; otherwise after it,
    // speculatively, so the robot sums' latency hides behind the gather
    bool go;
    if constexpr (EARLY) {
      go = hinc_gather<R, RW, false, false, HessPF<R, RW, RM>::rows>(d, L, d.z, H, smem, decide, epi);
    } else {
      auto epi_late = [&]() {
        epi();
        rs.issue(part, stride, L.rt0, L.rt1);
      };
      hinc_gather<R, RW, false, false, HessPF<R, RW, RM>::rows>(d, L, d.z, H, smem, NoPre{}, epi_late);
      go = decide();
    }
    if (!go) return;
    beta = u.beta;
  } else {
    // the phase test runs once the first chunk's records are in flight (a
    // robot out of tCG leaves before any row is gathered); the robot's state
    // (written by an earlier launch) loads with those records, not after the
    // gather's first barrier
    const Ctl& c = d.ctl[L.l];
    const int ph = c.phase;
    tcg_iter = c.tcg_iter;
    beta = c.beta;
    first = (tcg_iter == 0) || (KMX_HESS_PROBE & 4);
    // gated (see the consumer form): no record is fetched before the phase test
    if (gated && ph != PH_TCG) return;
    if (!hinc_gather<R, RW, true, false, HessPF<R, RW, RM>::rows>(d, L, d.z, H, smem,
                                                                  [&]() { return ph == PH_TCG; }, epi))
      return;
  }
  if (L.valid) {
    double Dg[16];
    expand_sym4(dg, Dg);
#pragma unroll
    for (int c = 0; c < 4; ++c)  // (hinc_gather_src's DIAG term, same expression)
      H[c] += zs[0] * Dg[4 * c] + zs[1] * Dg[4 * c + 1] + zs[2] * Dg[4 * c + 2] + zs[3] * Dg[4 * c + 3];
  }
  double hz[4];  // H z - z S (group_rhess before its projection)
#pragma unroll
  for (int k = 0; k < 4; ++k) hz[k] = H[k];
  (void)y;
  double v = 0.0;
  double dl[4] = {0, 0, 0, 0}, hdl[4] = {0, 0, 0, 0};
  if (L.valid) {
    if (first) {
#pragma unroll
      for (int k = 0; k < 4; ++k) { dl[k] = -zs[k]; hdl[k] = -hz[k]; }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        dl[k] = -zs[k] + beta * dold[k];
        hdl[k] = -hz[k] + beta * hold[k];
      }
      if (tcg_iter >= dhn && tcg_iter % dhn == 0) {
        // tcg_max > dhn only: delta_k goes into the oldest direction's buffer,
        // so the dhn directions k - dhn .. k - 1 join eta first, in step order
        double et[4] = {0, 0, 0, 0};
        if (tcg_iter > dhn) load4(d.eta + o, et);
        const double* ch = d.coefh + (size_t)L.l * d.p.tcg_max;
        for (int j = tcg_iter - dhn; j < tcg_iter; ++j) {
          double dj[4];
          if (j + 1 < tcg_iter) {
            load4(d.dh + (size_t)(j % dhn) * d.vec + o, dj);
          } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) dj[k] = dold[k];
          }
          const double cj = ch[j];
#pragma unroll
          for (int k = 0; k < 4; ++k) et[k] += cj * dj[k];
        }
        store4(d.eta + o, et);
      }
    }
    v = dl[0] * hdl[0] + dl[1] * hdl[1] + dl[2] * hdl[2] + dl[3] * hdl[3];
  }
  finish_tile<RED_HESS, 1, RM>(d, L, &v, smem + SmemH<R>::red_off, [&]() {
    if (L.valid && !(KMX_HESS_PROBE & 8)) {  // (probe 8: no stores)
      store4(d.dh + (size_t)(tcg_iter % dhn) * d.vec + o, dl);
      store4(d.hd + o, hdl);
    }
  });
}

// tCG step, part 2: r += coef Hdelta (eta = sum coef_k delta_k is formed in
// k_retract); interior steps also z = precon(r) and partials <r,r>, <z,r>.
// LAST (consumer form): the update of the host's launch tcg_max - 1. A robot
// it finds in tCG is at the step cap: its tCG ends after this update whatever
// the stop test says, and at the cap upd_step does not read <z,r>. So this
// instantiation forms no z (no preconditioner block, no z store, <z,r> = 0)
// and goes on to the robot's trial point from the rows it holds: x, the
// updated r, and this launch's coefficient as the last direction's (eta_rows'
// clast; k_retract's arithmetic, same bits). It publishes the state with
// `retracted` set and the phase still PH_TCG: the stop reason from ||r||^2 is
// taken by k_cost (body_cost), so the round has no k_retract.
template <int R, int RM, bool LAST = false>
__device__ __forceinline__ void body_update(const Dev& d, HostStatus* hs, unsigned long long seq, int slot,
                                            char* smem) {
  static_assert(!LAST || RM == RM_CONSUMER, "the launched form keeps k_retract");
  const Lane L = lane_map<R>(d);
  int tcg_iter, mode;
  double coef;
  const size_t o = (size_t)L.pose * 4 * R + 4 * L.a;
  double rr[4] = {0, 0, 0, 0}, y[4] = {0, 0, 0, 0}, hdl[4] = {0, 0, 0, 0};
  double gg[4] = {0, 0, 0, 0}, et[4] = {0, 0, 0, 0};  // LAST: the trial point's g row and eta
  EtaRows er;
  int T = 0;
  if constexpr (RM == RM_CONSUMER) {
    // this step's k_hess partials: the control step after the Hess-vec (alpha
    // or the boundary tau) on a private copy, with the step's vector loads in
    // flight; the first tile writes the robot's state (ctl2 -> ctl)
    __shared__ Ctl cs;
    __shared__ double rl[NPART * WAVES];
    Ctl* const cin = d.ctl2;
    Ctl* const cout = d.ctl;
    const Ctl& cq = cin[L.l];
    const bool writer = L.tile == L.rt0;
    if (writer && threadIdx.x < (int)(sizeof(Ctl) / 8))  // as in k_hess
      reinterpret_cast<double*>(&cs)[threadIdx.x] = reinterpret_cast<const double*>(&cq)[threadIdx.x];
    if (cq.phase != PH_TCG) {
      if (cq.phase == PH_STEP && !cq.retracted) {
        // this step's k_hess ended the robot's tCG at its stop test: the trial
        // point and the model partials here (k_retract's arithmetic; every
        // coefficient was decided by an earlier launch), so a round whose
        // robots all stop this way needs no k_retract (the robots still in
        // tCG at the cap take the LAST path below, or with KMX_TCG_TAIL=0
        // k_retract's fold 2)
        const size_t o2 = (size_t)L.pose * 4 * R + 4 * L.a;
        double x[4] = {0, 0, 0, 0}, gg[4] = {0, 0, 0, 0}, rr2[4] = {0, 0, 0, 0}, et[4] = {0, 0, 0, 0};
        if (L.valid) {
          load4(d.X + o2, x);
          load4(d.g + o2, gg);
          load4(d.r + o2, rr2);
          eta_rows<false>(d, L.l, o2, cq.tcg_iter, 0.0, et);
        }
        trial_rows<R>(d, L, o2, x, gg, rr2, et, smem);
        if (writer) ctl_publish(cout + L.l, cs, true);
        return;
      }
      if (writer) ctl_publish(cout + L.l, cs, false);
      return;
    }
    const bool first0 = cq.tcg_iter == 0;  // the control step makes it 1
    if constexpr (LAST) {
      T = cq.tcg_iter + 1;
      if (T != d.p.tcg_max) {  // (cannot happen: a robot in tCG at the host's launch j has run j steps)
        if (writer) ctl_publish(cout + L.l, cs, false);
        return;
      }
    }
    RobotSum<1, 4> rs;
    rs.issue(d.part_h, 2, L.rt0, L.rt1);
    if (L.valid) {
      load4(d.hd + o, hdl);
      load4((first0 ? d.g : d.r) + o, rr);
      load4(d.X + o, y);  // the projection of H delta, and the precon of interior steps
      // (the preconditioner block loads in group_precon, after the projection:
      // held from here it is 20 VGPRs across the projection's read-back, 86
      // against 66 in all, and the round is slower for it)
      if constexpr (LAST) {  // the trial point's rows: no address waits for the step's coefficient
        load4(d.g + o, gg);
        er.issue(d, o, T, et);
      }
    }
    double tot[NPART] = {0.0, 0.0, 0.0, 0.0};
    rs.finish(d.part_h, 2, rl, tot);
    const HessStep hsx = hess_step(cq.z_r, cq.e_Pe, cq.e_Pd, cq.d_Pd, cq.Delta, tot[0]);
    if (writer && threadIdx.x < 64) {  // the state update, on an LDS copy, by wave 0
      if (threadIdx.x == 0) {
        control_on(cs, d, L.l, RED_HESS, tot, R, true);
        if (slot >= 0) atomicAdd(d.hv_launch + slot, 1);
      }
      // lane 0's LDS writes, then the wave's reads (in-order LDS queue)
      __builtin_amdgcn_wave_barrier();
      asm volatile("" ::: "memory");
      ctl_publish(cout + L.l, cs, LAST);
    }
    tcg_iter = cq.tcg_iter + 1;
    mode = hsx.boundary ? MODE_BOUNDARY : MODE_INTERIOR;
    coef = hsx.coef;
  } else {
    const Ctl& c = d.ctl[L.l];
    if (c.phase != PH_TCG) {  // not in tCG: the robot's first tile reports it
      if (hs && threadIdx.x == 0 && L.tile == L.rt0) post_status(hs, L.l, seq, false);
      return;
    }
    tcg_iter = c.tcg_iter;
    mode = c.mode;
    coef = c.coef;
    if (L.valid) {
      load4(d.hd + o, hdl);
      load4((tcg_iter == 1 ? d.g : d.r) + o, rr);  // r_0 = g (k_grad does not store r)
      load4(d.X + o, y);  // the projection of H delta (and the precon of interior steps)
    }
  }
  const bool interior = (mode == MODE_INTERIOR);
  (void)tcg_iter;
  {  // H delta = P_Y(H delta^) (k_hess keeps it unprojected); every lane of the group takes part
    double hp[4];
    group_proj<R, true>(y, hdl, L.base, hp, reinterpret_cast<double*>(smem));
    if (L.valid) {
#pragma unroll
      for (int k = 0; k < 4; ++k) rr[k] += coef * hp[k];
    }
  }
  double vals[2] = {0.0, 0.0}, zr[4] = {0, 0, 0, 0};
  if constexpr (LAST) {
    if (interior && L.valid) vals[0] = rr[0] * rr[0] + rr[1] * rr[1] + rr[2] * rr[2] + rr[3] * rr[3];
    // the update's partials first: finish_tile's barrier ends every wave's use
    // of the projection's scratch, whose start trial_rows reduces in
    finish_tile<RED_UPDATE, 2, RM>(d, L, vals, smem + SmemU::red_off, [&]() {
      if (L.valid) store4(d.r + o, rr);
    });
    if (L.valid) er.template finish<true>(d, L.l, T, coef, et);
    trial_rows<R>(d, L, o, y, gg, rr, et, smem);
    return;
  }
  if (interior) {  // uniform per robot
    group_precon<R, true>(d, L.pose, L.valid, y, rr, L.base, zr, reinterpret_cast<double*>(smem));
    if (L.valid) {
      vals[0] = rr[0] * rr[0] + rr[1] * rr[1] + rr[2] * rr[2] + rr[3] * rr[3];
      vals[1] = zr[0] * rr[0] + zr[1] * rr[1] + zr[2] * rr[2] + zr[3] * rr[3];
    }
  }
  finish_tile<RED_UPDATE, 2, RM>(d, L, vals, smem + SmemU::red_off, [&]() {
    if (L.valid) {
      store4(d.r + o, rr);
      if (interior) store4(d.z + o, zr);
    }
  });
}

// ------------------------------------------------ one-sync tCG (opt-in) ---
// P.tcg_form = KMX_TCG_FORM_ONESYNC: one kernel per tCG step (k_step), so a
// step has one grid-wide dependency instead of two (k_hess -> k_update ->
// k_hess). Launch j applies step j-1's decision and forms step j:
//  1. every workgroup reduces the robot's 8-wide partials of launch j-1
//     (RobotSum8, tile order) and evaluates the decisions on them:
//     alpha (or the boundary tau) from <delta,H delta> and <r,z>, then the
//     stop test and beta from <r',r'> and <r',z'> formed by the recurrences
//       <r',r'> = <r,r> + 2 alpha <r,Hd> + alpha^2 <Hd,Hd>
//       <r',z'> = <r,z> + alpha (<r,w> + <Hd,z>) + alpha^2 <Hd,w>
//     (w = precon(H delta), precon linear); <r,z> and <r,r> are reduced from
//     the recurred vectors at every step, so the scalar recurrences are one
//     step deep. The robot's first tile writes the state (cin -> cout,
//     alternating buffers) and the host status;
//  2. the gather applies the Hessian to w (step 0: to z_0) — one row per
//     incidence, as k_hess — and the owner forms, by linearity,
//       z' = z + alpha w,        Hz' = Hz + alpha Hw,
//       delta' = -z' + beta delta,  H delta' = -Hz' + beta H delta,
//       r' = r + coef H delta,   w' = precon(H delta')
//     (fused multiply-adds, as the restatement), and the 7 partials.
// A robot whose tCG stops in step 1 only updates r (k_retract's model). What
// a launch reads across tiles — w and the robot's 8-wide partials — is
// double-buffered by step parity (launch j reads step j-1's and writes step
// j's); the kept directions are d.dh as in the standard form.
// Restated by oracle/dpgo_oracle.c tcg_onesync (same recurrences); parity
// with the standard form at convergence only.
__device__ __forceinline__ void onesync_scalars(double al, const double* tot, double* rrn, double* zrn) {
#pragma clang fp contract(off)
  *rrn = fmax(tot[2] + 2.0 * al * tot[5] + al * al * tot[6], 0.0);
  *zrn = tot[1] + al * tot[3] + al * al * tot[4];
}

// RobotSum for the one-sync step's 8-wide partials (d.part_f), same order as
// robot_sum: U tiles per thread in one round trip (1024 tiles, the 736-tile
// cut of a 12.5k-pose block included), tile order within a thread, then the
// wave sums and the waves in order; larger robots loop.
template <int U>
struct RobotSum8 {
  double a[U][8];
  int t0, t1;
  __device__ __forceinline__ void load(const double* part, int tb) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int t = min(tb + (int)threadIdx.x + u * RBLOCK, t1 - 1);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double2 x = ldpart(part, (size_t)t * 8 + 2 * k);
        a[u][2 * k] = x.x;
        a[u][2 * k + 1] = x.y;
      }
    }
  }
  __device__ __forceinline__ void issue(const double* part, int t0_, int t1_) {
    t0 = t0_;
    t1 = t1_;
    if (t1 - t0 <= U * RBLOCK) load(part, t0);
  }
  __device__ __forceinline__ void finish(const double* part, double* lds, double tot[8]) {
    constexpr int RW_ = RBLOCK / 64;
    double v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = 0.0;
    for (int tb = t0; tb < t1; tb += U * RBLOCK) {
      if (t1 - t0 > U * RBLOCK) load(part, tb);
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (tb + (int)threadIdx.x + u * RBLOCK < t1 && threadIdx.x < RBLOCK) {
#pragma unroll
          for (int k = 0; k < 8; ++k) v[k] += a[u][k];
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const double w = wave_sum(v[k]);
      if ((threadIdx.x & 63) == 0 && threadIdx.x < RBLOCK) lds[k * RW_ + (threadIdx.x >> 6)] = w;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      double acc = 0.0;
#pragma unroll
      for (int w = 0; w < RW_; ++w) acc += lds[k * RW_ + w];
      tot[k] = acc;
    }
  }
};

template <int R, int W = WAVES>
struct SmemF {  // k_step: the Hessian gather's layout with an 8-wide reduction area
  static constexpr int red_off = SmemH<R, W>::red_off;
  static constexpr int bytes = red_off + 8 * 8 * W + 16;
};

__device__ __forceinline__ double dot4(const double a[4], const double b[4]) {
  return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
}

// KMX_STEP_STAMPS builds (diagnostic, `make stamps`): thread 0 of every
// workgroup of the k_step launches that form step 2 records the wall clock
// (100 MHz) at entry, once the robot sums' loads are issued, once they (and
// the first records) have landed, after the decision, after the gather loop,
// after the Hessian's own-row part and at exit (kmx_pgo_debug_step_stamps;
// scripts/step_stamps.py).
#ifdef KMX_STEP_STAMPS
constexpr int STEP_STAMP_TILES = 8192;
__device__ unsigned long long g_step_stamp[16 * STEP_STAMP_TILES];
#define KMX_SS(i) \
  do { if (threadIdx.x == 0) ss_[i] = wall_clock64(); } while (0)
#else
#define KMX_SS(i) do {} while (0)
#endif

template <int R, int RW>
__device__ __forceinline__ void body_step(const Dev& d, const Ctl* cin, Ctl* cout, int jl, int slot,
                                          HostStatus* hs, unsigned long long seq, char* smem) {
#ifdef KMX_STEP_STAMPS
  unsigned long long ss_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
  KMX_SS(0);
  const Lane L = lane_map<R>(d);
  const size_t o = (size_t)L.pose * 4 * R + 4 * L.a;
  __shared__ Ctl cs;
  __shared__ double rl[8 * WAVES];
  const Ctl& c0 = cin[L.l];
  const bool writer = L.tile == L.rt0;
  if (writer && threadIdx.x < (int)(sizeof(Ctl) / 8))  // as in k_hess
    reinterpret_cast<double*>(&cs)[threadIdx.x] = reinterpret_cast<const double*>(&c0)[threadIdx.x];
  // first (the host's launch 0 of a tCG loop): a robot in it is at PH_START
  // and the launch consumes k_grad's partials, else it is in PH_TCG; the
  // robot sums' loads go out before the state arrives
  const bool grad = jl == 0;
  const int t0 = L.rt0, t1 = L.rt1;
  RobotSum<3> rg;
  RobotSum8<4> rf;
  if (grad) rg.issue(d.part, NPART, t0, t1);
  // launch jl consumes step jl - 1's partials (buffer (jl - 1) & 1) and
  // writes step jl's into the other buffer, so no tile of the robot can
  // overwrite a partial another tile of the same launch has yet to read (a
  // robot in tCG at launch jl is at tcg_iter jl - 1)
  const double* pf_in = d.part_f + (size_t)(((jl + 1) & 1) * d.ntiles) * 8;
  if (!grad) rf.issue(pf_in, t0, t1);
  const int ph0 = c0.phase;
  if (ph0 != (grad ? PH_START : PH_TCG)) {
    if (writer && threadIdx.x == 0) {
      cout[L.l] = c0;
      if (hs) post_status(hs, L.l, seq, false);
    }
    return;
  }
  const int k = grad ? -1 : c0.tcg_iter;  // the step whose partials this launch consumes
  double coef = 0.0, al = 0.0, be = 0.0;
  KMX_SS(1);
  auto decide = [&]() -> bool {
    bool go;
    KMX_SS(2);
    if (grad) {
      double tot[NPART];
      rg.finish(d.part, NPART, rl, tot);
      go = !(sqrt(tot[1]) < d.p.gn_tol);  // control_on's RED_GRAD test
      if (writer && threadIdx.x == 0) control_on(cs, d, L.l, RED_GRAD, tot, R, true);
    } else {
      double tot[8];
      rf.finish(pf_in, rl, tot);
      const double zr = tot[1];
      const HessStep hx = hess_step(zr, c0.e_Pe, c0.e_Pd, c0.d_Pd, c0.Delta, tot[0]);
      double rrn, zrn;
      onesync_scalars(hx.alpha, tot, &rrn, &zrn);
      const UpdStep u = upd_step(hx.boundary ? MODE_BOUNDARY : MODE_INTERIOR, c0.r_stop, c0.lin_stop, zr, k + 1,
                                 rrn, zrn, d.p);
      coef = hx.coef;
      al = hx.alpha;
      be = u.beta;
      go = !u.done;
      if (writer && threadIdx.x == 0) {  // the standard form's two control steps, on the LDS copy
        cs.z_r = zr;
        double th[NPART] = {tot[0], 0.0, 0.0, 0.0};
        control_on(cs, d, L.l, RED_HESS, th, R, true);
        double tu[NPART] = {rrn, zrn, 0.0, 0.0};
        control_on(cs, d, L.l, RED_UPDATE, tu, R, true);
      }
    }
    if (writer && threadIdx.x == 0) {
      cout[L.l] = cs;
      if (hs) post_status(hs, L.l, seq, cs.phase == PH_TCG);
      if (go && slot >= 0) atomicAdd(d.hv_launch + slot, 1);
    }
    KMX_SS(3);
    return go;
  };
  const int dhn = d.dhn;
  const double* V = grad ? d.z : ((k & 1) ? d.w1 : d.w0);  // the vector the Hessian is applied to
  double H[4];
  PlainRows<R> src{V};
  const bool go = hinc_gather_src<R, RW, false, PlainRows<R>, decltype(decide)&, false>(d, L, src, H, smem, decide);
  if (!grad && !go) {
    // the robot's tCG ends here: the last step's residual, then (no k_retract
    // in this form) the trial point of its rows and the model partials, with
    // this launch's coefficient for the last direction
    double x[4] = {0, 0, 0, 0}, gg[4] = {0, 0, 0, 0}, rr[4] = {0, 0, 0, 0}, et[4] = {0, 0, 0, 0};
    if (L.valid) {
      double hd[4];
      load4(d.r + o, rr);
      load4(d.hd + o, hd);
      load4(d.X + o, x);
      load4(d.g + o, gg);
#pragma unroll
      for (int c = 0; c < 4; ++c) rr[c] = fma(coef, hd[c], rr[c]);
      store4(d.r + o, rr);
      eta_rows<true>(d, L.l, o, k + 1, coef, et);
    }
    trial_rows<R>(d, L, o, x, gg, rr, et, smem);
    return;
  }
  if (!go) return;
  const int kn = k + 1;  // the step this launch forms
  KMX_SS(4);
  asm volatile("" ::: "memory");  // keep the epilogue loads below the gather loop (VGPR pressure)
  // every row the epilogue needs, in one batch (one round trip after the gather)
  // delta_kn goes into the oldest direction's buffer: directions kn - dhn ..
  // kn - 1 join eta first, in step order (the standard form's fold; the
  // newest coefficient is this launch's own decision). dhn = 2 (the
  // default): the older direction and eta load with the rest
  const bool fold = !grad && kn >= dhn && kn % dhn == 0;
  const bool fold2 = fold && dhn == 2;
  double dprev[4] = {0, 0, 0, 0}, et[4] = {0, 0, 0, 0};
  const double cprev = fold2 ? d.coefh[(size_t)L.l * d.p.tcg_max + kn - 2] : 0.0;
  double y[4] = {0, 0, 0, 0}, S[9], v[4] = {0, 0, 0, 0}, D[16], Pm[16];
  double rn[4] = {0, 0, 0, 0}, hold[4] = {0, 0, 0, 0}, zo[4] = {0, 0, 0, 0}, hzo[4] = {0, 0, 0, 0},
         dold[4] = {0, 0, 0, 0};
  if (L.valid) {
    load4(V + o, v);
    load_sym4(d.hD + SYM4 * (size_t)L.pose, D);
    load4(d.X + o, y);
    load_sym3(d.S + 6 * (size_t)L.pose, S);
    if (d.p.use_precond) load_sym4(d.Pinv + SYM4 * (size_t)L.pose, Pm);
    if (grad) {
      load4(d.g + o, rn);  // r_0 = g
    } else {
      load4(d.r + o, rn);
      load4(d.hd + o, hold);
      load4(d.z + o, zo);
      load4(d.hz + o, hzo);
      load4(d.dh + (size_t)(k % dhn) * d.vec + o, dold);
      if (fold2) {  // the direction folded with dold (below), and eta
        load4(d.dh + (size_t)(kn % dhn) * d.vec + o, dprev);
        if (kn > dhn) load4(d.eta + o, et);
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)  // the diagonal block (hinc_gather's DIAG term, same expression)
      H[c] += v[0] * D[4 * c] + v[1] * D[4 * c + 1] + v[2] * D[4 * c + 2] + v[3] * D[4 * c + 3];
  } else {
#pragma unroll
    for (int i = 0; i < 9; ++i) S[i] = 0.0;
  }
  double* scr = reinterpret_cast<double*>(smem);  // the chunk buffer is free after the gather
  double hv[4];
  group_rhess<R, true>(y, v, H, S, L.base, hv, scr);  // Riemannian Hess of z_0 or w_k
  KMX_SS(5);
  double zn[4], hzn[4], dl[4], hdl[4];
  if (grad) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      zn[c] = v[c];
      hzn[c] = hv[c];
      dl[c] = -v[c];
      hdl[c] = -hv[c];
    }
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      rn[c] = fma(coef, hold[c], rn[c]);
      zn[c] = fma(al, v[c], zo[c]);
      hzn[c] = fma(al, hv[c], hzo[c]);
      dl[c] = fma(be, dold[c], -zn[c]);
      hdl[c] = fma(be, hold[c], -hzn[c]);
    }
  }
  double wn[4];
  group_precon<R, true>(d, L.pose, L.valid, y, hdl, L.base, wn, scr, Pm, L.valid);
  if (fold2 && L.valid) {
#pragma unroll
    for (int c = 0; c < 4; ++c) et[c] += cprev * dprev[c];
#pragma unroll
    for (int c = 0; c < 4; ++c) et[c] += coef * dold[c];
    store4(d.eta + o, et);
  } else if (fold && L.valid) {  // other KMX_DHMAX builds
    if (kn > dhn) load4(d.eta + o, et);
    const double* ch = d.coefh + (size_t)L.l * d.p.tcg_max;
    for (int j = kn - dhn; j < kn; ++j) {
      double dj[4];
      load4(d.dh + (size_t)(j % dhn) * d.vec + o, dj);
      const double cj = (j == kn - 1) ? coef : ch[j];
#pragma unroll
      for (int c = 0; c < 4; ++c) et[c] += cj * dj[c];
    }
    store4(d.eta + o, et);
  }
  double pv[7] = {0, 0, 0, 0, 0, 0, 0};
  if (L.valid) {
    pv[0] = dot4(dl, hdl);
    pv[1] = dot4(rn, zn);
    pv[2] = dot4(rn, rn);
    pv[3] = dot4(rn, wn) + dot4(hdl, zn);
    pv[4] = dot4(hdl, wn);
    pv[5] = dot4(rn, hdl);
    pv[6] = dot4(hdl, hdl);
  }
  double* lds = reinterpret_cast<double*>(smem + SmemF<R>::red_off);
#pragma unroll
  for (int s2 = 0; s2 < 7; ++s2) {
    const double w = wave_sum(pv[s2]);
    if ((threadIdx.x & 63) == 0) lds[s2 * WAVES + (threadIdx.x >> 6)] = w;
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    double t = 0.0;
    if (threadIdx.x < 7) {
#pragma unroll
      for (int w = 0; w < WAVES; ++w) t += lds[threadIdx.x * WAVES + w];
    }
    d.part_f[((size_t)(kn & 1) * d.ntiles + L.tile) * 8 + threadIdx.x] = t;
  }
  if (L.valid) {
    store4(d.dh + (size_t)(kn % dhn) * d.vec + o, dl);
    store4(d.hd + o, hdl);
    store4(d.hz + o, hzn);
    if (!grad) store4(d.z + o, zn);
    store4(((kn & 1) ? d.w1 : d.w0) + o, wn);
    store4(d.r + o, rn);
  }
#ifdef KMX_STEP_STAMPS
  KMX_SS(6);
  if (kn == 2 && threadIdx.x == 0 && L.tile < STEP_STAMP_TILES) {
    for (int i = 0; i < 7; ++i) g_step_stamp[(size_t)L.tile * 16 + i] = ss_[i];
    g_step_stamp[(size_t)L.tile * 16 + 8] = (unsigned long long)L.np;
    g_step_stamp[(size_t)L.tile * 16 + 9] = (unsigned long long)L.n;
    g_step_stamp[(size_t)L.tile * 16 + 10] = (unsigned long long)blockIdx.x;
    g_step_stamp[(size_t)L.tile * 16 + 11] = (unsigned long long)(L.tile == L.rt0);
  }
#endif
}

// Trial point Xt = R_X(eta); partials: model m(eta) = 1/2 <eta, g + r> (r = g +
// H eta by the tCG recurrence) and ||Xt - X||^2 (slots 2, 3; k_cost reduces).
// fold (RM_CONSUMER): a robot still in tCG ran its last step's update with no
// k_hess after it; its reduction (the 2-wide part_u) and stop decision run
// here, in place of a k_reduce launch. The robot's first tile writes the
// decision into ctl in place: it changes only phase and tcg_stop, and a tile
// that reads the new phase goes straight to the retraction, as the decision
// says, so every tile acts alike.
// src: where the tCG left the robot's state — d.ctl, or d.ctl2 after an odd
// number of one-sync steps; the robot's first tile copies it to d.ctl, which
// the launches after this one read.
template <int R>
__device__ __forceinline__ void body_retract(const Dev& d, int fold, const Ctl* src, char* smem) {
  const Lane L = lane_map<R>(d);
  const Ctl& c = src[L.l];
  __shared__ int sph;
  __shared__ double rl[NPART * WAVES];
  if (threadIdx.x == 0) {
    sph = c.phase;
    if (src != d.ctl && L.tile == L.rt0) d.ctl[L.l] = c;
  }
  __syncthreads();
  const int ph = sph;  // one read per workgroup
  const size_t o = (size_t)L.pose * 4 * R + 4 * L.a;
  double x[4] = {0, 0, 0, 0}, et[4] = {0, 0, 0, 0}, gg[4] = {0, 0, 0, 0}, rr[4] = {0, 0, 0, 0}, dl[4];
  if (fold && ph == PH_TCG) {  // fold 2: a robot at PH_STEP may already be retracted (k_update)
    RobotSum<2> rs;
    rs.issue(d.part_u, 2, L.rt0, L.rt1);
    double tot[NPART] = {0.0, 0.0, 0.0, 0.0};
    rs.finish(d.part_u, 2, rl, tot);
    const UpdStep u = upd_step(c.mode, c.r_stop, c.lin_stop, c.z_r, c.tcg_iter, tot[0], tot[1], d.p);
    if (!u.done) return;  // (cannot happen: the host stops enqueueing only when no robot is in tCG or at tcg_max)
    if (threadIdx.x == 0 && L.tile == L.rt0) {  // (fold: src is d.ctl)
      if (u.stop >= 0) d.ctl[L.l].tcg_stop = u.stop;
      d.ctl[L.l].phase = PH_STEP;
    }
  } else if (ph != PH_STEP || (fold == 2 && c.retracted)) {
    return;
  }
  if (L.valid) {  // all rows in flight before the Gram-Schmidt chain
    load4(d.X + o, x);
    load4(d.g + o, gg);
    load4(d.r + o, rr);
    if (d.p.rgd) {  // RGD: eta = -s z
      load4(d.z + o, dl);
      const double coef = c.coef;
#pragma unroll
      for (int k = 0; k < 4; ++k) et[k] += coef * dl[k];
    } else {
      eta_rows<false>(d, L.l, o, c.tcg_iter, 0.0, et);
    }
  }
  trial_rows<R>(d, L, o, x, gg, rr, et, smem);
}

// src: as k_retract's (the one-sync form has no k_retract: its k_step
// retracts a robot's rows in the launch that ends its tCG, so k_cost carries
// the state over to d.ctl).
template <int R, int RW, int RM>
__device__ __forceinline__ void body_cost(const Dev& d, const Ctl* src, char* smem) {
  const Lane L = lane_map<R>(d);
  const Ctl& c = src[L.l];
  if (src != d.ctl && threadIdx.x == 0 && L.tile == L.rt0) d.ctl[L.l] = c;
  const int ph = c.phase;
  bool go = ph == PH_STEP;
  if constexpr (RM == RM_CONSUMER) {
    // A robot in PH_TCG with `retracted` set: the last k_update (body_update's
    // LAST) found it at the step cap and formed its trial point. Its stop
    // reason from that update's ||r||^2 is decided here, in place of a
    // k_reduce launch, by the robot's first tile alone, which writes it into
    // ctl in place as k_retract's fold does: the write changes only phase and
    // tcg_stop, every other tile takes PH_TCG with `retracted` and PH_STEP
    // alike as "a trial point to cost", and k_commit reads the state one
    // launch later. (The one-sync form's src holds no such robot.)
    go = go || (ph == PH_TCG && c.retracted);
  }
  if (!go) return;
  double cost = inc_owner_cost<R, RW>(d, L, d.Xt, d.pub, smem);
  finish_tile<RED_COST, 1, RM>(d, L, &cost, smem + SmemC<R>::red_off, []() {});
  if constexpr (RM == RM_CONSUMER) {
    // (after the gather, from a second read of the phase, which only this
    // tile writes: decided before the gather it costs k_cost two registers)
    if (L.tile == L.rt0 && c.phase == PH_TCG) {  // uniform per workgroup
      __shared__ double rl[NPART * WAVES];
      RobotSum<2> rs;
      rs.issue(d.part_u, 2, L.rt0, L.rt1);
      double tot[NPART] = {0.0, 0.0, 0.0, 0.0};
      rs.finish(d.part_u, 2, rl, tot);
      const UpdStep u = upd_step(c.mode, c.r_stop, c.lin_stop, c.z_r, c.tcg_iter, tot[0], tot[1], d.p);
      if (threadIdx.x == 0) {  // (u.done: the robot is at the cap; src is d.ctl)
        if (u.stop >= 0) d.ctl[L.l].tcg_stop = u.stop;
        d.ctl[L.l].phase = PH_STEP;
      }
    }
  }
}

// End of a round: X <- Xt where the step was accepted, and the owned public
// rows of the committed poses are published (the single-device exchange), so
// the next round — and a GNC weight update before it — sees the new poses.
// Tile 0 also counts the round for the GNC schedule.
// fold (RM_CONSUMER, one RTR iteration): the trial-cost reduction and the
// accept decision run here in place of a k_reduce launch; every tile decides
// from the robot's totals and f_cur, which the decision does not change. The
// robot's first tile writes the RTR state, except the phase, which stays
// PH_STEP (the next round's k_begin resets it), so tiles that read the state
// after that write still see a robot with a step to decide.
// final = 0: between two RTR iterations of one block update — the accepted
// trial point becomes the iterate the next iteration starts from, but the
// public rows (the neighbours' snapshot of this round) and the round counters
// wait for the block update's end. The final commit then publishes every
// robot that moved in this block update, whether or not its last iteration
// committed.
template <int R>
__device__ __forceinline__ void body_commit(const Dev& d, int fold, int final) {
  const Lane L = lane_map<R>(d);
  if (final && L.tile == 0 && threadIdx.x == 0) {
    d.gnc->inner += 1;
    d.gnc->rounds += 1;
  }
  bool commit;
  if (fold) {
    __shared__ int sph;
    __shared__ Ctl cs;
    __shared__ double rl[NPART * WAVES];
    const Ctl& c = d.ctl[L.l];
    const bool writer = L.tile == L.rt0;
    if (writer && threadIdx.x < (int)(sizeof(Ctl) / 8))  // as in k_hess
      reinterpret_cast<double*>(&cs)[threadIdx.x] = reinterpret_cast<const double*>(&c)[threadIdx.x];
    if (threadIdx.x == 0) sph = c.phase;
    __syncthreads();
    if (sph != PH_STEP) return;
    RobotSum<NPART> rs;
    rs.issue(d.part, NPART, L.rt0, L.rt1);
    double tot[NPART] = {0.0, 0.0, 0.0, 0.0};
    rs.finish(d.part, NPART, rl, tot);
    if (d.p.rgd) {
      commit = true;
    } else {  // control_on's RED_COST acceptance test
      const double model_dec = -0.5 * tot[2];
      const double rho = (model_dec > 0.0) ? (c.f_cur - tot[0]) / model_dec : -1.0;
      commit = rho > d.p.accept_rho;
    }
    if (threadIdx.x == 0 && writer) {
      control_on(cs, d, L.l, RED_COST, tot, R, true);
      cs.phase = PH_STEP;
      d.ctl[L.l] = cs;
    }
  } else {
    const Ctl& c = d.ctl[L.l];
    commit = c.commit != 0;
    // Several RTR iterations: a robot whose last iteration was rejected or
    // skipped has nothing to commit, but an earlier iteration of this block
    // update may have moved X (chg_acc > 0; the non-final commits leave the
    // public table alone): its rows are published from X here. With one
    // iteration chg_acc > 0 only where commit is set.
    if (final && !commit && c.chg_acc > 0.0 && L.valid) {
      const int s = d.pose_slot[L.pose];
      if (s >= 0) {
        const size_t o = (size_t)L.pose * 4 * R + 4 * L.a;
        double v[4];
        load4(d.X + o, v);
        store4(d.pub + (size_t)s * 4 * R + 4 * L.a, v);
      }
    }
  }
  if (!commit || !L.valid) return;
  const size_t o = (size_t)L.pose * 4 * R + 4 * L.a;
  double v[4];
  load4(d.Xt + o, v);
  store4(d.X + o, v);
  if (!final) return;
  const int s = d.pose_slot[L.pose];
  if (s >= 0) store4(d.pub + (size_t)s * 4 * R + 4 * L.a, v);
}

// One kernel per phase of the round.
template <int R, int RW, int RM>
__global__ __launch_bounds__(BLOCK, LB<R>::w) void k_grad(Dev d, int gated) {
  KMX_SMEM;
  body_grad<R, RW, RM>(d, gated, smem);
}
template <int R, int RW, int RM, bool GRAD, bool EARLY>
__global__ __launch_bounds__(BLOCK, LB<R>::w) void k_hess(Dev d, int gated, int slot, HostStatus* hs,
                                                          unsigned long long seq) {
  KMX_SMEM;
  body_hess<R, RW, RM, GRAD, EARLY>(d, gated, slot, hs, seq, smem);
}
template <int R, int RM>
__global__ __launch_bounds__(BLOCK) void k_update(Dev d, HostStatus* hs, unsigned long long seq, int slot) {
  KMX_SMEM;
  body_update<R, RM>(d, hs, seq, slot, smem);
}
// 3 waves per SIMD at r <= 5: the 736-tile cut of a small shard is resident
// in one generation (256 CUs x 3), without the spills of a 128-VGPR bound
template <int R, int RW>
__global__ __launch_bounds__(BLOCK, (R <= 5 ? 3 : 2)) void k_step(Dev d, const Ctl* cin, Ctl* cout, int jl, int slot,
                                                                  HostStatus* hs, unsigned long long seq) {
  KMX_SMEM;
  body_step<R, RW>(d, cin, cout, jl, slot, hs, seq, smem);
}
template <int R>
__global__ __launch_bounds__(BLOCK) void k_retract(Dev d, int fold, const Ctl* src) {
  KMX_SMEM;
  body_retract<R>(d, fold, src, smem);
}
template <int R, int RW, int RM>
__global__ __launch_bounds__(BLOCK, LB<R>::w) void k_cost(Dev d, const Ctl* src) {
  KMX_SMEM;
  body_cost<R, RW, RM>(d, src, smem);
}
template <int R>
__global__ __launch_bounds__(BLOCK) void k_commit(Dev d, int fold, int final) {
  body_commit<R>(d, fold, final);
}
// The consumer form's k_update of the host's launch tcg_max - 1 (body_update's
// LAST). A kernel of its own name, defined after the others: k_update<R, RM>
// keeps its symbol, its registers and its place in the code object.
template <int R>
__global__ __launch_bounds__(BLOCK) void k_update_last(Dev d, HostStatus* hs, unsigned long long seq, int slot) {
  KMX_SMEM;
  body_update<R, RM_CONSUMER, true>(d, hs, seq, slot, smem);
}

// Several RTR iterations per block update: the RTR state sums the squared
// lengths of the accepted steps (chg_acc), which is the block update's change
// only when there is one step. After the final k_commit this kernel, one
// workgroup per robot, takes ||X - X0||^2 over the robot's rows against the
// round's start X0 and writes dpgo's relativeChange of the whole block update
// into the robot's state and its team status. A fixed summation order: equal
// bits in every form of the round.
__global__ __launch_bounds__(BLOCK) void k_change(Dev d, const double* X0, int ps) {
  const int l = blockIdx.x;
  const int t0 = d.rtile0[l], t1 = d.rtile0[l + 1];
  if (t0 == t1 || !d.ctl[l].updated) return;  // no poses, or not active this round
  const long long n = (long long)d.n_robot[l] * ps;
  const size_t o = (size_t)d.tile[t0].p0 * ps;
  double s = 0.0;
  for (long long i = threadIdx.x; i < n; i += BLOCK) {
    const double dd = d.X[o + i] - X0[o + i];
    s += dd * dd;
  }
  __shared__ double ws[WAVES];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) t += ws[w];
    const double rel = sqrt(t / (double)d.n_robot[l]);
    d.ctl[l].rel_change = rel;
    d.relc[l] = rel;
  }
}

// ------------------------------------------------- round begin + GNC-TLS ---
// shouldUpdateMeasurementWeights (drawio:2466-2469): never for L2 or once
// robustOptNumWeightUpdates updates were made; otherwise when more than
// robustOptInnerIters rounds ran since the last update, or when every agent of
// the team has converged (relative change of its last block update <=
// relChangeTol; this handle's robots plus the peers' statuses in `ext`).
__device__ __forceinline__ bool gnc_should_update(const Dev& d) {
  const Params& P = d.p;
  if (!P.robust || !P.gnc_on) return false;
  const Gnc& s = *d.gnc;
  if (s.updates >= P.max_updates) return false;
  if (s.inner > P.inner_iters) return true;
  for (int l = 0; l < d.L; ++l)
    if (!(d.relc[l] <= P.rel_tol)) return false;
  for (int k = 0; k < P.n_ext; ++k)
    if (!(d.ext[k] <= P.rel_tol)) return false;
  return true;
}

// TLS weight of one loop closure on the lifted poses (oracle residual_sq and
// gnc_tls_weight): the owner's and the peer's handles both evaluate a shared
// loop closure from the same two rows, so both get the owner's value bit for
// bit without the measurement_weights message (drawio:2195-2198).
template <int RW>
__device__ __forceinline__ void gnc_edge(const Dev& d, int i, int R_, double mu) {
  const int e = d.gnc_edge[i];
  const int2 en = d.gnc_ends[i];
  const int ps = 4 * R_;
  const double* Xi = en.x >= 0 ? d.X + (size_t)en.x * ps : d.pub + (size_t)(-1 - en.x) * ps;
  const double* Xj = en.y >= 0 ? d.X + (size_t)en.y * ps : d.pub + (size_t)(-1 - en.y) * ps;
  const int2 ip = d.eipos[e];
  double2 q[Rec<RW>::Q];
  Rec<RW>::load(d, (size_t)(ip.x >= 0 ? ip.x : ip.y), q);
  Edge E;
  Rec<RW>::edge(q, E);
  double sR = 0.0, sT = 0.0;
  for (int a = 0; a < R_; ++a) {
    const double* yi = Xi + 4 * a;
    const double* yj = Xj + 4 * a;
    for (int c = 0; c < 3; ++c) {
      const double r = yj[c] - (yi[0] * E.R[0 * 3 + c] + yi[1] * E.R[1 * 3 + c] + yi[2] * E.R[2 * 3 + c]);
      sR += r * r;
    }
    const double et = yj[3] - yi[3] - (yi[0] * E.t[0] + yi[1] * E.t[1] + yi[2] * E.t[2]);
    sT += et * et;
  }
  const double rSq = d.ekappa[e] * sR + d.etau[e] * sT;
  const double barcSq = d.p.barc * d.p.barc;
  const double upper = (mu + 1.0) / mu * barcSq;
  const double lower = mu / (mu + 1.0) * barcSq;
  double w;
  if (rSq >= upper) w = 0.0;
  else if (rSq <= lower) w = 1.0;
  else w = sqrt(barcSq * mu * (mu + 1.0) / rSq) - mu;
  d.ew[e] = w;
  const double wk = w * d.ekappa[e], wt = w * d.etau[e];
  constexpr int WK = Rec<RW>::WK;
  constexpr int GS = Rec<RW>::GS;  // ip.x: the tail's record, ip.y: the head's
  if (ip.x >= 0) { d.rec[(size_t)GS * ip.x + WK] = wk; d.rec[(size_t)GS * ip.x + WK + 1] = Rec<RW>::wt_word(wt, true); }
  if (ip.y >= 0) { d.rec[(size_t)GS * ip.y + WK] = wk; d.rec[(size_t)GS * ip.y + WK + 1] = Rec<RW>::wt_word(wt, false); }
}

__device__ __forceinline__ void begin_robot(const Dev& d, const unsigned char* active, int l) {
  Ctl& c = d.ctl[l];
  const bool a = active ? active[l] != 0 : true;
  const Ctl zero = {};
  c = zero;
  c.phase = a ? PH_START : PH_IDLE;
  c.updated = a ? 1 : 0;
  c.Delta = d.p.Delta0;
}

enum BeginMode { BEGIN_ROUND = 1, BEGIN_FORCE_GNC = 2, BEGIN_SOLO = 4 };

// Round begin (BEGIN_ROUND: reset the robots' Ctl) and/or a GNC weight update:
// scheduled (gnc_should_update) or forced (BEGIN_FORCE_GNC, the explicit
// updateMeasurementWeights). Every block takes the same decision from the
// same state; block 0 writes the next state to gnc_next (k_precond commits
// it), the other blocks re-weight their loop closures and rewrite both
// incidence records of each.
template <int RW>
__global__ void k_begin(Dev d, const unsigned char* active, int mode, int R_) {
  const bool fire = d.p.robust && ((mode & BEGIN_FORCE_GNC) ? true : gnc_should_update(d));
  const double mu = d.gnc->mu;
  if (blockIdx.x == 0) {
    if (mode & BEGIN_ROUND)
      for (int l = threadIdx.x; l < d.L; l += blockDim.x) begin_robot(d, active, l);
    if (threadIdx.x == 0) {
      Gnc s = load_gnc(d.gnc);
      s.fired = fire ? 1 : 0;
      if (fire) {
        s.inner = 0;
        s.updates += 1;
        s.mu = mu * d.p.mu_step;
      }
      store_gnc(d.gnc_next, s);
      if (mode & BEGIN_SOLO) store_gnc(d.gnc, s);  // one-block launch: no reader of the state is left
      if (fire) atomicAdd(&d.cnt->gnc_updates, 1ull);
    }
    return;
  }
  if (!fire) return;
  for (int i = (blockIdx.x - 1) * blockDim.x + threadIdx.x; i < d.n_gnc; i += (gridDim.x - 1) * blockDim.x)
    gnc_edge<RW>(d, i, R_, mu);
}

// 4x4 diagonal blocks D_i of Q per pose (hD, for the Hessian gather) and the
// inverse preconditioner blocks (D_i + shift I)^-1 by Cholesky; same
// accumulation order and expressions as oracle build_precond. `gated`: only
// after a round-begin launch that re-weighted (then block 0 commits gnc_next).
template <int RW>
__global__ void k_precond(Dev d, int gated) {
  if (gated) {
    if (blockIdx.x == 0 && threadIdx.x == 0) store_gnc(d.gnc, load_gnc(d.gnc_next));
    if (!d.gnc_next->fired) return;
  }
  for (int pose = blockIdx.x * blockDim.x + threadIdx.x; pose < d.nloc; pose += gridDim.x * blockDim.x)
    pose_precond<RW>(d, pose);
}

// setMeasurementWeight in bulk: push the per-edge weights into both incidence
// records (w kappa, w tau).
template <int RW>
__global__ void k_apply_weights(Dev d, int mloc) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= mloc) return;
  const double w = d.ew[e];
  const double wk = w * d.ekappa[e], wt = w * d.etau[e];
  const int2 ip = d.eipos[e];
  constexpr int WK = Rec<RW>::WK;
  constexpr int GS = Rec<RW>::GS;  // ip.x: the tail's record, ip.y: the head's
  if (ip.x >= 0) { d.rec[(size_t)GS * ip.x + WK] = wk; d.rec[(size_t)GS * ip.x + WK + 1] = Rec<RW>::wt_word(wt, true); }
  if (ip.y >= 0) { d.rec[(size_t)GS * ip.y + WK] = wk; d.rec[(size_t)GS * ip.y + WK + 1] = Rec<RW>::wt_word(wt, false); }
}

// ------------------------------------------------------- public exchange ---
// One 16-B part i of the owned public rows: slot s = i / (ps / 2) (ps = 4r is
// even, rows are 16-B aligned).
__global__ void k_publish(const double* X, double* pub, const int* src, int nslots, int ps) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int ps2 = ps >> 1;
  const long long s = i / ps2;
  if (s >= nslots) return;
  const int q = (int)(i - s * ps2);
  const int p = src[s];
  if (p >= 0)
    reinterpret_cast<double2*>(pub)[s * ps2 + q] = reinterpret_cast<const double2*>(X)[(long long)p * ps2 + q];
}

// Sparse exchange: rows of the given public slots (owned by this handle) from
// the iterate, and rows received from peers written into the table. With
// per-peer segments (nseg > 0, seg[k] = first row of peer k's segment), every
// segment is followed by one status double (this handle's largest relative
// change, dpgo's Status message, drawio:2375): segment k starts at row
// seg[k] * ps + k. A slot outside the table (or, for gather, not owned here)
// is skipped (gather writes zeros), so a bad index list cannot fault the device.
__device__ __forceinline__ long long seg_offset(const int* seg, int nseg, long long s) {
  int k = 0;
  while (k + 1 < nseg && seg[k + 1] <= s) ++k;
  return nseg > 0 ? k : 0;
}
// The status words ride in the same launch: threads n*ps .. n*ps + nseg - 1
// write this handle's max relative change after every segment (gather) /
// read the peers' into ext (scatter). One launch per side of the exchange.
__global__ void k_gather_slots(const double* X, const int* pub_src, const int* slots, long long n, int npub,
                               double* out, int ps, const int* seg, int nseg, const double* relc, int L) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long s = i / ps;
  if (s >= n) {
    const long long k = i - n * ps;
    if (k >= nseg) return;
    double m = 0.0;
    for (int l = 0; l < L; ++l) m = (relc[l] > m || relc[l] != relc[l]) ? relc[l] : m;
    out[(long long)seg[k + 1] * ps + k] = m;
    return;
  }
  const int q = (int)(i - s * ps);
  const int sl = slots[s];
  const int p = (sl >= 0 && sl < npub) ? pub_src[sl] : -1;
  out[i + seg_offset(seg, nseg, s)] = (p >= 0) ? X[(long long)p * ps + q] : 0.0;
}
__global__ void k_scatter_slots(double* pub, const int* slots, long long n, int npub, const double* rows, int ps,
                                const int* seg, int nseg, double* ext) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long s = i / ps;
  if (s >= n) {
    const long long k = i - n * ps;
    if (k < nseg) ext[k] = rows[(long long)seg[k + 1] * ps + k];
    return;
  }
  const int q = (int)(i - s * ps);
  const int sl = slots[s];
  if (sl >= 0 && sl < npub) pub[(long long)sl * ps + q] = rows[i + seg_offset(seg, nseg, s)];
}

// The native exchange's gather / scatter (enqueue_exchange): the segment of
// every row is precomputed (rseg[s], set_exchange), so a thread reads one int
// instead of walking the segment table; status words as above.
__global__ void k_xgather(const double* X, const int* pub_src, const int* slots, const int* rseg, long long n,
                          double* out, int ps, const int* seg, int nseg, const double* relc, int L) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long s = i / ps;
  if (s >= n) {
    const long long k = i - n * ps;
    if (k >= nseg) return;
    double m = 0.0;
    for (int l = 0; l < L; ++l) m = (relc[l] > m || relc[l] != relc[l]) ? relc[l] : m;
    out[(long long)seg[k + 1] * ps + k] = m;
    return;
  }
  const int q = (int)(i - s * ps);
  const int p = pub_src[slots[s]];
  out[i + rseg[s]] = (p >= 0) ? X[(long long)p * ps + q] : 0.0;
}
__global__ void k_xscatter(double* pub, const int* slots, const int* rseg, long long n, const double* rows, int ps,
                           const int* seg, int nseg, double* ext) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long s = i / ps;
  if (s >= n) {
    const long long k = i - n * ps;
    if (k < nseg) ext[k] = rows[(long long)seg[k + 1] * ps + k];
    return;
  }
  const int q = (int)(i - s * ps);
  pub[(long long)slots[s] * ps + q] = rows[i + rseg[s]];
}

__global__ void k_pack(const double* X, double* out, const int* src, int first, int count, int ps) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long s = i / ps;
  if (s >= count) return;
  const int q = (int)(i - s * ps);
  out[s * ps + q] = X[(long long)src[first + s] * ps + q];
}

__global__ void k_shared_pack(const double* ew, const int* sh_edge, const int* sh_idx, int n, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[sh_idx[i]] = ew[sh_edge[i]];
}
__global__ void k_shared_unpack(double* ew, const int* sh_edge, const int* sh_idx, int n, const double* tab) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  ew[sh_edge[i]] = tab[sh_idx[i]];
}

// --- rounding to SE(3) in the anchor frame (same algorithm as the oracle) --
// R = the nearest rotation to M = Ya^T Yi (so3_project.h: any singular values,
// 0 included, give a finite proper rotation), t = Ya^T (pi - pa).
__global__ void k_traj(const double* X, int n, int R_, const double* anchor, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double* Xi = X + (size_t)i * 4 * R_;
  double M[9], tv[3];
  for (int x = 0; x < 3; ++x) {
    for (int y = 0; y < 3; ++y) {
      double s = 0.0;
      for (int k = 0; k < R_; ++k) s += anchor[4 * k + x] * Xi[4 * k + y];
      M[x * 3 + y] = s;
    }
    double s = 0.0;
    for (int k = 0; k < R_; ++k) s += anchor[4 * k + x] * (Xi[4 * k + 3] - anchor[4 * k + 3]);
    tv[x] = s;
  }
  double Rr[3][3];
  so3_project_block(M, Rr);
  double* o = out + (size_t)i * 12;
  for (int q = 0; q < 9; ++q) o[q] = Rr[q / 3][q % 3];
  o[9] = tv[0]; o[10] = tv[1]; o[11] = tv[2];
}

// Nesterov acceleration (oracle orc_pgo_accel_pre / _post; RBCD++):
//   mode 0: Y = Proj((1 - c) X + c V) -> Yb, X and the owned public rows
//   mode 1: V = Proj(V + c (X - Yb))
//   mode 2: V = X (restart)
// Proj: polar factor of the pose's r x 3 rotation block (group_project);
// translation unchanged. One lane per (pose, row), as k_retract.
template <int R>
__global__ __launch_bounds__(BLOCK) void k_accel(Dev d, double* V, double* Yb, double c, int mode) {
  const Lane L = lane_map<R>(d);
  const size_t o = (size_t)L.pose * 4 * R + 4 * L.a;
  double x[4] = {0, 0, 0, 0}, v[4] = {0, 0, 0, 0}, y[4] = {0, 0, 0, 0};
  if (L.valid) {
    load4(d.X + o, x);
    if (mode != 2) load4(V + o, v);
    if (mode == 1) load4(Yb + o, y);
  }
  if (mode == 2) {
    if (L.valid) store4(V + o, x);
    return;
  }
  double m[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) m[k] = (mode == 0) ? (1.0 - c) * x[k] + c * v[k] : v[k] + c * (x[k] - y[k]);
  double out[4];
  group_project<R>(m, L.a, L.base, L.pw < 64 / R, out);
  if (!L.valid) return;
  if (mode == 0) {
    store4(Yb + o, out);
    store4(d.X + o, out);
    const int s = d.pose_slot[L.pose];
    if (s >= 0) store4(d.pub + (size_t)s * 4 * R + 4 * L.a, out);
  } else {
    store4(V + o, out);
  }
}

// Primitive evaluation for parity tests (tiles of one robot), through the same
// gathers as the round kernels.
template <int R>
struct SmemE {
  static constexpr int g = SmemHG<R>::red_off > SmemH<R>::red_off ? SmemHG<R>::red_off : SmemH<R>::red_off;
  static constexpr int red_off = g;
  static constexpr int bytes = red_off + RED_BYTES;
};
template <int R, int RW>
__global__ __launch_bounds__(BLOCK, LB<R>::w) void k_eval(Dev d, int robot, int mode, const double* V, double* out) {
  KMX_SMEM;
  const Lane L = lane_map<R>(d);
  if (L.l != robot) return;
  const size_t o = (size_t)L.pose * 4 * R + 4 * L.a;
  double res[4] = {0, 0, 0, 0}, cost = 0.0, v[4] = {0, 0, 0, 0};
  double* scr = reinterpret_cast<double*>(smem);
  if (mode == KMX_EVAL_COST_EGRAD) {
    hinc_grad<R, RW>(d, L, V, d.pub, res, &cost, smem);
  } else if (mode == KMX_EVAL_EHESS) {
    hinc_gather<R, RW>(d, L, V, res, smem);
    if (L.valid) load4(V + o, v);
  } else if (mode == KMX_EVAL_PROJECT) {
    if (L.valid) load4(V + o, v);
    group_project<R>(v, L.a, L.base, L.pw < 64 / R, res);
  } else {
    double y[4] = {0, 0, 0, 0}, G[4], c0 = 0.0;
    hinc_grad<R, RW>(d, L, d.X, d.pub, G, &c0, smem);
    if (L.valid) {
      load4(d.X + o, y);
      load4(V + o, v);
    }
    double S[9];
    group_symYtG<R, true, GSYM_ALL>(y, G, L.base, S, scr);
    if (mode == KMX_EVAL_RGRAD) {
      for (int c = 0; c < 3; ++c) res[c] = G[c] - (y[0] * S[0 * 3 + c] + y[1] * S[1 * 3 + c] + y[2] * S[2 * 3 + c]);
      res[3] = G[3];
      for (int k = 0; k < 4; ++k) v[k] = res[k];
    } else if (mode == KMX_EVAL_RHESS) {
      __syncthreads();  // the scratch reads are done before the next gather reuses the LDS
      double H[4];
      hinc_gather<R, RW>(d, L, V, H, smem);
      group_rhess<R, true, GSYM_ALL>(y, v, H, S, L.base, res, scr);
    } else if (mode == KMX_EVAL_PRECON) {
      group_precon<R, true, GSYM_ALL>(d, L.pose, L.valid, y, v, L.base, res, scr);
    } else if (mode == KMX_EVAL_RETRACT) {
      group_retract<R>(y, v, L.base, res);
      for (int k = 0; k < 4; ++k) v[k] = 0.0;
    }
  }
  double s = (mode == KMX_EVAL_COST_EGRAD) ? cost : 0.0;
  if (L.valid) {
    store4(out + o, res);
    if (mode != KMX_EVAL_COST_EGRAD) s = v[0] * res[0] + v[1] * res[1] + v[2] * res[2] + v[3] * res[3];
  }
  const double t = block_sum(s, reinterpret_cast<double*>(smem + SmemE<R>::red_off));
  if (threadIdx.x == 0) d.part[(size_t)L.tile * NPART] = t;
}

}  // namespace

// ============================================================ handle =====
// The graph's device buffers: replaced together by kmx_pgo_set_graph, which
// builds a fresh set aside and commits it by move once its uploads are done.
struct PgoDev {
  template <class T>
  using DevBuf = kmx::DevBuf<T>;
  DevBuf<TileDesc> tile;
  DevBuf<int> rtile0, inc_ptr;
  DevBuf<double> rec;
  DevBuf<int> rec_o;
  DevBuf<double> ekappa, etau, ew;
  DevBuf<int2> eipos;
  DevBuf<double> vec;     // X Xt g r z hd eta, then the dhn tCG directions (nvec())
  DevBuf<double> coefh;   // [L][tcg_max]
  DevBuf<double> part_f;  // [ntiles][8] one-sync tCG partials (P.tcg_form)
  DevBuf<double> S, Pinv, hD, hDS, pub, part;
  DevBuf<Ctl> ctl, ctl2;
  DevBuf<double> part_h, part_u;
  DevBuf<Counters> cnt;
  DevBuf<long long> m_robot;
  DevBuf<int> n_robot;
  DevBuf<int> pub_src;    // slot -> local pose (-1 if not local)
  DevBuf<int> own_src;    // owned slot k -> local pose (index first_owned + k)
  DevBuf<int> pose_slot;  // local pose -> owned slot or -1
  DevBuf<int> gnc_edge;
  DevBuf<int2> gnc_ends;
  DevBuf<int> sh_edge, sh_idx, osh_edge, osh_idx;
  DevBuf<double> relc;
  DevBuf<Gnc> gnc;  // [2]: state, next
  DevBuf<double> ext;
  DevBuf<unsigned char> active;
  DevBuf<double> scratch;  // eval / trajectory in-out, allocated on first use
  DevBuf<int> hv_launch;   // timing
  // Nesterov acceleration (P.acceleration): momentum V and this round's Y
  // (allocated only when enabled)
  DevBuf<double> accV, accY;
  // X at the start of the round, kept when a block update runs several RTR
  // iterations (k_change: its relative change is against this point)
  DevBuf<double> X0;
};
// The native exchange's buffers (kmx_pgo_set_exchange), replaced together.
struct PgoXchg {
  kmx::DevBuf<int> xs_slots, xr_slots, xs_seg, xr_seg;
  kmx::DevBuf<int> xs_rseg, xr_rseg;  // segment index of every row
  kmx::DevBuf<double> xsbuf, xrbuf;
};

struct kmx_pgo : kmx::StreamCore {
  kmx_pgo_params P{};
  // The group streams and the events stand before the buffers: the buffers
  // are destroyed first, then these, then the base's stream.
  static constexpr int MAX_GROUPS = 4;
  kmx::Stream gstream[MAX_GROUPS - 1];
  kmx::Event ev_fork, ev_join[MAX_GROUPS - 1];
  std::vector<kmx::Event> ev_pool;  // timing
  size_t ev_used = 0;
  ~kmx_pgo() {
    if (comm) (void)ncclCommAbort(comm);  // non-blocking communicator: no finalize handshake at teardown
  }
  // team
  int n_robots = 0;
  std::vector<int> npose;
  std::vector<int> local_of;  // robot -> local index or -1
  std::vector<int> robots;    // local index -> robot
  std::vector<int> loff;      // local robot -> first local pose
  int nloc = 0;
  int64_t m_global = 0;
  // public table
  int64_t npub = 0, first_owned = 0, n_owned = 0;
  std::vector<int64_t> pub_key;  // sorted (robot<<32 | pose)
  // local edges
  int mloc = 0;
  std::vector<int64_t> loc_edge_gid;
  int ninc = 0;
  int rw = 10;  // record width in doubles (10 compact quaternion / 16 full)
  int64_t nshared = 0;
  int n_sh_local = 0, n_gnc = 0, n_osh = 0;
  std::vector<long long> m_robot;
  int ntiles = 0;
  std::vector<int> rt0_h;  // [L + 1] first tile of each local robot
  // GNC schedule (host copy of the parameters)
  int gnc_on = 0, gnc_inner_iters = 20, gnc_max_updates = 0x7fffffff, n_ext = 0;
  double gnc_rel_tol = 1e-3;
  // device
  Dev dv{};    // what the kernels take: gd's pointers (filled by set_graph alone)
  PgoDev gd;   // gd.vec null: no graph (ready())
  int ctl_par = 0;  // one-sync tCG: the state after the last tCG loop is in ctl2 (odd step count)
  // tCG progress polling (see HostStatus): mapped, coherent; the kernels take the host pointer itself
  kmx::MappedBuf<HostStatus> hstat;
  unsigned long long seq = 0;
  bool poll = true;          // kmx_pgo_set_tcg_poll(0): enqueue every tCG step (finished robots exit at once)
  // kmx_pgo_set_tcg_poll(-1) (the default): adaptive. A polled tCG loop
  // that ran to within BLIND_SLACK steps of the cap sends the next
  // BLIND_WINDOW loops blind (no host wait: at most BLIND_SLACK empty step
  // pairs of ~1.5 us each, against the host round trip of every polled step
  // and the host seam of a multi-rank round); then one polled loop measures
  // again. Measured on configs[3] (scripts/host_seam.py, round_sizes.py):
  // blind wins at 100k poses (728 vs 740 us), on the N = 4 / 8 rank handles
  // (274 vs 284, 197 vs 217 us), loses on a 12.5k block needing ~5 steps
  // (163 vs 150 us), where the adaptive rule keeps polling.
  bool poll_auto = true;
  // native exchange (kmx_pgo_comm_init + kmx_pgo_set_exchange): every round
  // of iterate / iterate_async starts with gather -> RCCL send/recv with each
  // peer -> scatter, all on the handle's stream (no cross-stream event, no
  // host round trip between the exchange and the round)
  ncclComm_t comm = nullptr;
  int world = 1, rank = 0;
  bool xchg = false, xchg_self_p2p = false;
  PgoXchg xd;
  long long xn_send = 0, xn_recv = 0;
  std::vector<long long> xs_cnt, xr_cnt, xs_off, xr_off;  // per peer, in doubles (rows * 4r + 1 status)
  static constexpr int BLIND_SLACK = 2, BLIND_WINDOW = 8;  // the window's state: Group::blind_left
  // Robot groups (KMX_TCG_GROUPS = 1, 2 or 4; default 2): between a round's
  // k_begin and its final k_commit a robot's launches read only its own rows
  // and the public table, which changes only in that k_commit (DESIGN.md
  // section 13), so the local robots are cut into contiguous groups of about
  // equal incidence counts and each group's launch chain (k_grad, the tCG
  // steps, k_retract, k_cost and their k_reduce launches, over the group's
  // tiles and robots) runs on a stream of its own: group 0 on the handle's
  // stream, group g > 0 on gstream[g - 1], forked by an event after k_begin
  // and joined by one event per side stream before the final k_commit. One
  // group's k_reduce launches, ramps and tails then run under another group's
  // bandwidth-bound kernels. The arithmetic of a robot does not depend on
  // the grouping (its tiles and the order of its tile partials are the same).
  // In effect for RM_LAUNCH and RTR only, and not while timing is on (the
  // evented replay wants launches that do not overlap).
  struct Group {
    int l0 = 0, l1 = 0;  // local robots [l0, l1)
    int t0 = 0, nt = 0;  // their tiles [t0, t0 + nt)
    int blind_left = 0;  // the chain's own adaptive polling state
  };
  int groups_req = 2;
  std::vector<Group> grp;  // the cut of the current graph (one group: no fork)
  // The single chain: every local robot and every tile on the handle's
  // stream. Its adaptive polling state is its own, apart from grp[0]'s.
  Group all;
  // The grouped round's reduction form (KMX_GROUP_RED = 0 launched, 2
  // consumer): which instantiation of enqueue_round_t the groups' chains
  // take; `rm` still decides whether groups are in effect and the single
  // chain's form. Consumer while no local robot has more than
  // GROUP_CONSUMER_MAX_TILES tiles (pgo_host.h, with the measurements).
  int grm = 2;
  int grm_forced = -1;
  // Gated k_hess launches (KMX_HESS_GATE=0: off): every k_hess launch after a
  // tCG's first tests its robot's phase before its first record chunk is
  // fetched. Ungated, a launch enqueued before the host knows whether any robot
  // is still in tCG fetched that chunk before the test (the records' round
  // trip overlapping the state's), so a launch every robot skips still read
  // ~42 MB at configs[3]. Measured (profiles/r06/hess_gate/, two runs each):
  // gating every launch after the first 0.685 / 0.683 ms per round, ungated
  // 0.692 / 0.691, gating only the steps at or past where the last polled loop
  // stopped 0.691 / 0.691 — the state's round trip costs a gated launch less
  // than a skipped launch's record fetch costs the round.
  bool hess_gate = true;
  // The consumer form's round tail (KMX_TCG_TAIL=0: off): the k_update at the
  // step cap forms the trial point and k_cost takes its stop decision, so the
  // chain has no k_retract (tail_fused). Off: the parent's launches, the
  // in-build bitwise reference and the A/B cell.
  bool tcg_tail = true;
  // (measured and removed: a hipStreamQuery before the status spin put a ~5 us
  // bubble before the next tCG step's first kernel, profiles/r02/ab_query)
  // reduction mode: set per graph (pgo_plan: consumer up to
  // RM_CONSUMER_MAX_POSES local poses) unless KMX_RED forces one (0 launch,
  // 2 consumer)
  int rm = RM_LAUNCH;
  int rm_forced = -1;
  // consumer-form k_hess: the stop decision before the gather (small problems)
  // or after it; KMX_HESS_DECIDE forces one (0 after, 1 before)
  int early_stop = 1;
  int decide_forced = -1;
  bool poll_timeout = false;
  // timing
  bool timing = false;
  // Nesterov acceleration (P.acceleration): gamma and the restart counter on the host
  double acc_gamma = 0.0;
  int acc_k = 0;
  bool acc_ready = false, acc_started = false;
};

namespace {

void drop_xchg(kmx_pgo* h) {
  h->xd = {};
  h->xchg = false;
}

// The kernels' compile-time sizes from the handle's run-time ones: f is
// called with a std::integral_constant of the lifted rank r (3..8) or of the
// record width in doubles (10 / 16).
template <typename F>
void with_r(int r, F&& f) {
  switch (r) {
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 5: f(std::integral_constant<int, 5>{}); break;
    case 6: f(std::integral_constant<int, 6>{}); break;
    case 7: f(std::integral_constant<int, 7>{}); break;
    default: f(std::integral_constant<int, 8>{}); break;
  }
}
template <typename F>
void with_rw(int rw, F&& f) {
  if (rw == 10) f(std::integral_constant<int, 10>{});
  else f(std::integral_constant<int, 16>{});
}

hipEvent_t next_event(kmx_pgo* h) {
  if (h->ev_used == h->ev_pool.size()) {
    h->ev_pool.emplace_back();
    (void)h->ev_pool.back().create();
  }
  return h->ev_pool[h->ev_used++];
}

bool ready(kmx_pgo* h) { return h && h->gd.vec.get() != nullptr; }

// Vectors of d_vec: X Xt g r z hd eta + the tCG directions kept for k_retract
// (+ Hz, w_0, w_1 for the one-sync tCG, which needs two directions).
bool onesync(const kmx_pgo* h) {
  return h->P.tcg_form == KMX_TCG_FORM_ONESYNC && h->P.method == KMX_METHOD_RTR;
}
// Several RTR iterations per block update (RGD runs one step whatever rtr_iterations says)
bool multi_rtr(const kmx_pgo* h) { return h->P.method == KMX_METHOD_RTR && h->P.rtr_iterations > 1; }
int dh_count(const kmx_pgo* h) {
  return std::max(onesync(h) ? 2 : 1, std::min(h->P.tcg_max_iterations, DHMAX));
}
size_t nvec(const kmx_pgo* h) { return 7 + (size_t)dh_count(h) + (onesync(h) ? 3 : 0); }

// Scratch of the diagnostic / output entry points (not resident with the graph).
int ensure_scratch(kmx_pgo* h, size_t doubles) {
  if (doubles <= h->gd.scratch.cap()) return 0;
  if (h->gd.scratch.get()) KMX_HIP(hipStreamSynchronize(h->stream));
  h->gd.scratch = {};
  return h->gd.scratch.alloc(doubles);
}


void sync_params(kmx_pgo* h) {
  Params& p = h->dv.p;
  p.tcg_max = h->P.tcg_max_iterations;
  p.rtr_iters = h->P.rtr_iterations;
  p.use_precond = h->P.use_preconditioner;
  p.robust = h->P.robust_cost == KMX_COST_GNC_TLS ? 1 : 0;
  p.kappa = h->P.tcg_kappa;
  p.theta = h->P.tcg_theta;
  p.Delta0 = h->P.rtr_initial_radius;
  p.Delta_max = h->P.rtr_max_radius;
  p.accept_rho = h->P.rtr_accept_rho;
  p.gn_tol = h->P.gradnorm_tol;
  p.shift = h->P.precond_shift;
  p.barc = h->P.gnc_barc;
  p.mu_step = h->P.gnc_mu_step;
  p.rel_tol = h->gnc_rel_tol;
  p.gnc_on = h->gnc_on;
  p.inner_iters = h->gnc_inner_iters;
  p.max_updates = h->gnc_max_updates;
  p.n_ext = h->n_ext;
  p.rgd = h->P.method == KMX_METHOD_RGD ? 1 : 0;
  p.rgd_step = h->P.rgd_stepsize;
  h->dv.ext = h->gd.ext.get();
}

// Room for n peers' status words. The stream's work is done before the old
// words go; a failure changes nothing, and the kernels' copy of the pointer follows.
int ensure_ext(kmx_pgo* h, size_t n) {
  if (n <= h->gd.ext.cap()) return 0;
  KMX_HIP(hipStreamSynchronize(h->stream));
  if (int rc = h->gd.ext.alloc(n)) return rc;
  sync_params(h);
  return 0;
}

// Owned public rows into the table (the single-device exchange).
void enqueue_publish(kmx_pgo* h) {
  const int ps = 4 * h->P.r;
  const long long tot = h->n_owned * ps;
  if (tot == 0) return;
  hipLaunchKernelGGL(k_publish, dim3((unsigned)((tot / 2 + 255) / 256)), dim3(256), 0, h->stream, h->gd.vec.get(),
                     h->gd.pub.get() + (size_t)h->first_owned * ps, h->gd.pub_src.get() + h->first_owned,
                     (int)h->n_owned, ps);
}

void enqueue_precond(kmx_pgo* h, int gated) {
  const int blocks = std::max(1, std::min(gated ? 256 : 1024, (h->nloc + 127) / 128));
  with_rw(h->rw, [&](auto RW) {
    hipLaunchKernelGGL(k_precond<RW()>, dim3(blocks), dim3(128), 0, h->stream, h->dv, gated);
  });
}

// Round begin (mode BEGIN_ROUND) and/or GNC update, then the gated
// preconditioner rebuild that commits the GNC state.
// Returns whether the gated preconditioner rebuild is left to the next k_grad
// (defer: the round's first gradient follows this launch directly).
// done: an event that completes with the begin launch itself (the dispatch's
// own completion signal: no marker packet on the stream behind it).
bool enqueue_begin(kmx_pgo* h, const unsigned char* d_active, int mode, bool defer = false,
                   hipEvent_t done = nullptr) {
  const bool may_fire = h->P.robust_cost == KMX_COST_GNC_TLS && (h->gnc_on || (mode & BEGIN_FORCE_GNC));
  if (!may_fire) mode |= BEGIN_SOLO;  // no weight update possible: one block, no preconditioner rebuild
  // a capped grid: when the schedule does not fire, the launch costs its dispatch
  const unsigned grid = may_fire ? 1 + (unsigned)std::min(256, std::max(1, (h->n_gnc + 255) / 256)) : 1;
  with_rw(h->rw, [&](auto RW) {
    if (done)
      hipExtLaunchKernelGGL(k_begin<RW()>, dim3(grid), dim3(256), 0, h->stream, nullptr, done, 0u, h->dv, d_active,
                            mode, h->P.r);
    else
      hipLaunchKernelGGL(k_begin<RW()>, dim3(grid), dim3(256), 0, h->stream, h->dv, d_active, mode, h->P.r);
  });
  if (may_fire && !defer) enqueue_precond(h, 1);
  return may_fire && defer;
}

// Wait until every robot of [l0, l1) with tiles reported tCG step `seq`;
// returns whether any of them is still in tCG. A device that stops reporting
// for 30 s switches the handle to blind enqueueing (every tCG step launched).
bool wait_running(kmx_pgo* h, unsigned long long seq, int l0, int l1) {
  volatile HostStatus* hs = h->hstat.get();
  const auto t0 = std::chrono::steady_clock::now();
  bool running = false;
  for (int l = l0; l < l1; ++l) {
    if (h->rt0_h[l + 1] == h->rt0_h[l]) continue;  // no tiles: never in tCG
    unsigned long long w;
    while (((w = __atomic_load_n(&hs[l].word, __ATOMIC_ACQUIRE)) >> 1) < seq) {
      if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(30)) {
        h->poll_timeout = true;
        h->poll = false;
        return true;
      }
    }
    running |= (w & 1ull) != 0;
  }
  return running;
}

// Launch chains of the next round. More than one (the robot groups,
// kmx_pgo::grp) for RM_LAUNCH and RTR only; the timed replay (its events want
// launches that do not overlap), RGD and the one-sync tCG run on the single
// chain (kmx_pgo::all), and enqueue_round_t relies on that: its event slots,
// its RGD step and its k_step loop know one chain only.
int groups_in_effect(const kmx_pgo* h) {
  if (h->timing || h->rm != RM_LAUNCH || h->P.method != KMX_METHOD_RTR || onesync(h)) return 1;
  return std::max<int>(1, (int)h->grp.size());
}

// One launch chain of a round: a Dev whose launches cover the chain's tiles,
// its stream, its robots (k_reduce's first robot and grid) and its polling
// state.
struct Chain {
  Dev d;
  hipStream_t s;
  int l0, nl;
  kmx_pgo::Group* st;
};
Chain make_chain(kmx_pgo* h, kmx_pgo::Group& G, hipStream_t s) {
  Chain q{h->dv, s, G.l0, G.l1 - G.l0, &G};
  q.d.gt0 = G.t0;
  q.d.gnt = G.nt;
  return q;
}
// done: an event that completes with this dispatch
template <int R>
void red(const Chain& q, int kind, HostStatus* hs = nullptr, unsigned long long seq = 0, int slot = -1,
         hipEvent_t done = nullptr) {
  if (done)
    hipExtLaunchKernelGGL(k_reduce, dim3(q.nl), dim3(RBLOCK), 0, q.s, nullptr, done, 0u, q.d, q.l0, kind, R, hs, seq,
                          slot, (const double*)nullptr);
  else
    hipLaunchKernelGGL(k_reduce, dim3(q.nl), dim3(RBLOCK), 0, q.s, q.d, q.l0, kind, R, hs, seq, slot,
                       (const double*)nullptr);
}

// A timed launch's slot of Dev::hv_launch and the events that take the
// dispatch's own start / end timestamps (none while timing is off or the
// slots are used up).
struct Timed {
  int slot = -1;
  hipEvent_t e0 = nullptr, e1 = nullptr;
};
Timed next_timed(kmx_pgo* h) {
  Timed t;
  if (h->timing && h->ev_used / 2 < (size_t)HV_SLOTS) {
    t.slot = (int)(h->ev_used / 2);
    t.e0 = next_event(h);
    t.e1 = next_event(h);
  }
  return t;
}

// Whether a chain's next tCG loop polls or goes blind, and what a loop that
// enqueued `steps` steps means for the next ones (see kmx_pgo::poll_auto).
bool tcg_polls(kmx_pgo* h, kmx_pgo::Group& st) {
  if (!(h->poll && h->hstat.get())) return false;
  if (h->poll_auto && st.blind_left > 0) {
    --st.blind_left;
    return false;
  }
  return true;
}
void tcg_polled(const kmx_pgo* h, kmx_pgo::Group& st, bool poll, int steps) {
  if (poll && h->poll_auto && steps + kmx_pgo::BLIND_SLACK >= h->P.tcg_max_iterations)
    st.blind_left = kmx_pgo::BLIND_WINDOW;
}

// The parts of a round: gradient, tCG (host-polled steps), trial point and
// cost; round begin before and commit after. Replaying the launches between
// two tCG loops from a hipGraph was measured on one 12.5k-pose block (170.1
// vs 167.7 us per round eager: the graph launch moves the host latency to the
// first tCG step after it; profiles/r02/small_round/2_*) and not kept.
// RM_CONSUMER folds the round's other reductions into the kernel after them
// (no k_reduce launch in a round): the gradient's into the first k_hess, the
// last tCG update's into k_cost (tail_fused; k_retract with KMX_TCG_TAIL=0),
// the trial cost's into k_commit (one RTR iteration). RGD keeps the
// gradient's launch (no k_hess follows).
template <int RM>
bool fold_grad(const kmx_pgo* h) {
  return RM == RM_CONSUMER && h->P.method != KMX_METHOD_RGD && h->P.tcg_max_iterations > 0;
}
template <int RM>
bool fold_cost(const kmx_pgo* h) {
  return RM == RM_CONSUMER && (h->P.rtr_iterations == 1 || h->P.method == KMX_METHOD_RGD);
}
// The consumer form's standard tCG without k_retract: the k_update of launch
// tcg_max - 1 (k_update_last) forms the trial point of the robots at the step
// cap and k_cost takes their stop decision; a robot that stopped earlier got
// its trial point from the k_update behind the k_hess that stopped it. A
// chain is then 1 + 2 steps + 2 launches: gradient, steps, cost, commit.
// Not RGD (its step is k_retract's), not the one-sync form (k_step retracts);
// KMX_TCG_TAIL=0 keeps k_retract's fold 2 and an ordinary last k_update.
template <int RM>
bool tail_fused(const kmx_pgo* h) {
  return RM == RM_CONSUMER && h->tcg_tail && h->P.method != KMX_METHOD_RGD && !onesync(h) &&
         h->P.tcg_max_iterations > 0;
}

// One k_hess launch. fl: bit 0, the host's launch 0 of a tCG loop; bit 1,
// gated. The consumer form has an instantiation per (launch 0, decision
// position); e0 / e1 (both or neither) take the dispatch's own start / end
// timestamps.
template <int R, int RW, int RM>
void launch_hess(const kmx_pgo* h, dim3 grid, hipStream_t st, const Dev& dv, int fl, int slot, HostStatus* hs,
                 unsigned long long seq, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr) {
  const dim3 blk(BLOCK);
  const int gated = (fl & 2) ? 1 : 0;
  auto go = [&](auto kern) {
    if (e0)
      hipExtLaunchKernelGGL(kern, grid, blk, SmemH<R>::bytes, st, e0, e1, 0u, dv, gated, slot, hs, seq);
    else
      hipLaunchKernelGGL(kern, grid, blk, SmemH<R>::bytes, st, dv, gated, slot, hs, seq);
  };
  if constexpr (RM == RM_CONSUMER) {
    const bool grad = (fl & 1) != 0, early = h->early_stop != 0;
    if (grad && early) go(k_hess<R, RW, RM, true, true>);
    else if (grad) go(k_hess<R, RW, RM, true, false>);
    else if (early) go(k_hess<R, RW, RM, false, true>);
    else go(k_hess<R, RW, RM, false, false>);
  } else {
    go(k_hess<R, RW, RM, false, false>);
  }
}

// The tCG loops of G chains: each step is (k_hess, k_update), with their
// k_reduce launches in the launched form, enqueued launch by launch across
// the chains so no stream runs dry while the host serves another. The loops
// poll per chain: a chain whose robots have all left tCG is no longer
// enqueued while the others go on. stopped[g]: the polled loop saw chain g's
// robots stop.
template <int R, int RW, int RM>
void enqueue_tcg_t(kmx_pgo* h, const Chain* q, int G, bool* stopped) {
  constexpr bool cons = RM == RM_CONSUMER;
  const dim3 blk(BLOCK);
  const int tmax = h->P.tcg_max_iterations;
  bool poll[kmx_pgo::MAX_GROUPS], live[kmx_pgo::MAX_GROUPS];
  unsigned long long prev[kmx_pgo::MAX_GROUPS], seq[kmx_pgo::MAX_GROUPS];
  int steps[kmx_pgo::MAX_GROUPS];  // steps enqueued by a polled loop
  for (int g = 0; g < G; ++g) {
    poll[g] = tcg_polls(h, *q[g].st);
    live[g] = true;
    prev[g] = seq[g] = 0;
    steps[g] = tmax;
  }
  for (int j = 0; j < tmax; ++j) {
    bool any = false;
    for (int g = 0; g < G; ++g) {
      if (!live[g]) continue;
      any = true;
      const Timed t = next_timed(h);  // timing runs one chain (groups_in_effect)
      poll[g] = poll[g] && h->poll;   // a poll timeout inside wait_running switches to blind
      seq[g] = poll[g] ? ++h->seq : 0;
      HostStatus* hs = poll[g] ? h->hstat.get() : nullptr;
      const int fl = (j == 0 ? 1 : 0) | (j > 0 && h->hess_gate ? 2 : 0);
      const dim3 grid(q[g].d.gnt);
      if constexpr (cons) {
        // k_hess reports the stop test of the previous step's update
        launch_hess<R, RW, RM>(h, grid, q[g].s, q[g].d, fl, t.slot, hs, seq[g], t.e0, t.e1);
        // the update at the step cap also forms the trial point (tail_fused)
        if (j == tmax - 1 && tail_fused<RM>(h))
          hipLaunchKernelGGL((k_update_last<R>), grid, blk, SmemU::bytes, q[g].s, q[g].d, (HostStatus*)nullptr, 0ull,
                             t.slot);
        else
          hipLaunchKernelGGL((k_update<R, RM>), grid, blk, SmemU::bytes, q[g].s, q[g].d, (HostStatus*)nullptr, 0ull,
                             t.slot);
      } else {
        launch_hess<R, RW, RM>(h, grid, q[g].s, q[g].d, fl, t.slot, nullptr, 0ull, t.e0, t.e1);
        red<R>(q[g], RED_HESS, nullptr, 0, t.slot);
        hipLaunchKernelGGL((k_update<R, RM>), grid, blk, SmemU::bytes, q[g].s, q[g].d, (HostStatus*)nullptr, seq[g],
                           -1);
        red<R>(q[g], RED_UPDATE, hs, seq[g]);
      }
    }
    if (!any) break;
    for (int g = 0; g < G; ++g) {
      if (!live[g] || !poll[g]) continue;
      // consumer: this step's k_hess reports (its k_update is queued behind
      // it); launched: exactly one step stays queued beyond the last one
      // known to be needed
      if (j > 0 && !wait_running(h, cons ? seq[g] : prev[g], q[g].l0, q[g].l0 + q[g].nl)) {
        steps[g] = j + 1;
        live[g] = false;
        stopped[g] = true;
      }
      prev[g] = seq[g];
    }
  }
  for (int g = 0; g < G; ++g) tcg_polled(h, *q[g].st, poll[g], steps[g]);
}

// The one-sync tCG loop (one chain): one k_step per step. Launch j applies
// step j-1's decision (which it reports at its start) and runs Hess-vec j;
// launch tmax only decides. A polled loop waits for launch j's report while
// launch j still gathers, so the next launch is queued before the GPU runs
// dry. The state ping-pongs between ctl and ctl2; kmx_pgo::ctl_par says where
// the loop left it.
template <int R, int RW>
void enqueue_tcg_onesync_t(kmx_pgo* h, const Chain& q) {
  const dim3 grid(q.d.gnt), blk(BLOCK);
  const int tmax = h->P.tcg_max_iterations;
  bool poll = tcg_polls(h, *q.st);
  int J = tmax + 1;
  for (int j = 0; j <= tmax; ++j) {
    const Timed t = next_timed(h);
    poll = poll && h->poll;
    const unsigned long long seq = poll ? ++h->seq : 0;
    HostStatus* hs = poll ? h->hstat.get() : nullptr;
    const Ctl* cin = (j & 1) ? h->gd.ctl2.get() : h->gd.ctl.get();
    Ctl* cout = (j & 1) ? h->gd.ctl.get() : h->gd.ctl2.get();
    if (t.e0)
      hipExtLaunchKernelGGL((k_step<R, RW>), grid, blk, SmemF<R>::bytes, q.s, t.e0, t.e1, 0u, q.d, cin, cout, j,
                            t.slot, hs, seq);
    else
      hipLaunchKernelGGL((k_step<R, RW>), grid, blk, SmemF<R>::bytes, q.s, q.d, cin, cout, j, t.slot, hs, seq);
    if (poll && j > 0 && !wait_running(h, seq, q.l0, q.l0 + q.nl)) {
      J = j + 1;
      break;
    }
  }
  h->ctl_par = J & 1;
  tcg_polled(h, *q.st, poll, J - 1);
}

// One round over G >= 1 launch chains (groups_in_effect), all of form RM.
// k_begin on the handle's stream; then per chain, on its stream, k_grad, the
// tCG loop, k_retract (none where tail_fused), k_cost and the non-final
// k_commit over the chain's tiles; then the final k_commit of all robots on
// the handle's stream (it writes the public rows the other chains' k_grad /
// k_cost read).
// G = 1 is kmx_pgo::all on the handle's stream: no event, no wait. G > 1 are
// the robot groups, group g > 0 on a stream of its own. Fork: the begin
// launch's own completion is the event the side streams wait for. Join: each
// side stream's last launch (the trial cost's k_reduce, or k_cost itself
// where the final commit takes its sums) carries the event the final commit
// waits for. Neither puts a marker on the stream it is recorded on, so group
// 0's k_grad follows k_begin directly.
// RM_LAUNCH: every chain carries its k_reduce launches. RM_CONSUMER: none
// (fold_grad, fold_cost above): k_update and k_hess reduce each other's
// partials, and with more than one RTR iteration each chain keeps its
// RED_COST k_reduce and its own non-final commit.
template <int R, int RW, int RM>
void enqueue_round_t(kmx_pgo* h, const unsigned char* d_active, int G) {
  constexpr bool cons = RM == RM_CONSUMER;
  const dim3 blk(BLOCK);
  // one chain only (groups_in_effect): the RGD step and the one-sync tCG
  const bool rgd = h->P.method == KMX_METHOD_RGD, os = cons && onesync(h);
  // the round's start for k_change (on the handle's stream, ahead of the begin
  // launch the side streams wait for)
  if (multi_rtr(h))
    (void)hipMemcpyAsync(h->gd.X0.get(), h->dv.X, sizeof(double) * (size_t)h->dv.vec, hipMemcpyDeviceToDevice,
     h->stream);
  // the round's first k_grad runs the gated preconditioner rebuild (there is
  // one: set_graph refuses a graph without tiles)
  const bool pend = enqueue_begin(h, d_active, BEGIN_ROUND, true, G > 1 ? h->ev_fork : nullptr);
  Chain q[kmx_pgo::MAX_GROUPS];
  if (G == 1) q[0] = make_chain(h, h->all, h->stream);
  else
    for (int g = 0; g < G; ++g) q[g] = make_chain(h, h->grp[g], g == 0 ? h->stream : h->gstream[g - 1]);
  // (an event call's error is left to the caller's hipGetLastError, as a launch's)
  for (int g = 1; g < G; ++g) (void)hipStreamWaitEvent(q[g].s, h->ev_fork, 0);
  const int iters = rgd ? 1 : h->P.rtr_iterations;
  const bool fgrad = fold_grad<RM>(h), fcost = fold_cost<RM>(h);
  for (int it = 0; it < iters; ++it) {
    for (int g = 0; g < G; ++g) {
      hipLaunchKernelGGL((k_grad<R, RW, RM>), dim3(q[g].d.gnt), blk, SmemHG<R>::bytes, q[g].s, q[g].d,
                         it == 0 && pend ? 1 : 0);
      if (!fgrad) red<R>(q[g], RED_GRAD);
    }
    bool stopped[kmx_pgo::MAX_GROUPS] = {};
    if constexpr (cons) {
      if (os) enqueue_tcg_onesync_t<R, RW>(h, q[0]);
    }
    if (!rgd && !os) enqueue_tcg_t<R, RW, RM>(h, q, G, stopped);
    // one-sync: each k_step that ended a robot's tCG also formed its trial
    // point, so there is no k_retract; k_cost takes the state from where the
    // tCG left it
    const Ctl* src = os && h->ctl_par ? h->gd.ctl2.get() : h->gd.ctl.get();
    for (int g = 0; g < G; ++g) {
      const dim3 grid(q[g].d.gnt);
      const bool last = it + 1 == iters;
      hipEvent_t join = g > 0 && last ? h->ev_join[g - 1] : nullptr;
      // consumer tCG: the k_update after the k_hess that stopped a robot
      // formed its trial point, and the one at the step cap that of the
      // robots still in tCG there (tail_fused): no k_retract. With
      // KMX_TCG_TAIL=0 k_retract (fold 2) reduces the last update, decides and
      // retracts the robots at the cap, and is not needed when the polled
      // loop saw the chain's robots stop
      if (!os && !(cons && stopped[g]) && !tail_fused<RM>(h))
        hipLaunchKernelGGL((k_retract<R>), grid, blk, SmemU::bytes, q[g].s, q[g].d, cons && !rgd ? 2 : 0,
                           (const Ctl*)h->gd.ctl.get());
      if (fcost && join)  // the side stream's last dispatch: the join event completes with it
        hipExtLaunchKernelGGL((k_cost<R, RW, RM>), grid, blk, SmemC<R>::bytes, q[g].s, nullptr, join, 0u, q[g].d, src);
      else
        hipLaunchKernelGGL((k_cost<R, RW, RM>), grid, blk, SmemC<R>::bytes, q[g].s, q[g].d, src);
      if (!fcost) red<R>(q[g], RED_COST, nullptr, 0, -1, join);
      if (!last)  // the next RTR iteration starts from the accepted point: the robot's own X only
        hipLaunchKernelGGL((k_commit<R>), grid, blk, 0, q[g].s, q[g].d, 0, 0);
    }
  }
  for (int g = 1; g < G; ++g) (void)hipStreamWaitEvent(h->stream, h->ev_join[g - 1], 0);
  hipLaunchKernelGGL((k_commit<R>), dim3(h->ntiles), blk, 0, h->stream, h->dv, fcost ? 1 : 0, 1);
  if (multi_rtr(h))
    hipLaunchKernelGGL(k_change, dim3(h->dv.L), blk, 0, h->stream, h->dv, (const double*)h->gd.X0.get(), 4 * R);
}

// One RBCD round for the robots whose d_active flag is set; it starts with
// the scheduled GNC decision when the handle's schedule is enabled. The
// robot groups take their own reduction form (kmx_pgo::grm).
void enqueue_round(kmx_pgo* h, const unsigned char* d_active) {
  const int G = groups_in_effect(h);
  const int rm = G > 1 ? h->grm : h->rm;
  // (the form outside the record width: the kernels' instantiations then
  // stand in the code object in the order they were measured in)
  with_r(h->P.r, [&](auto R) {
    constexpr int r = decltype(R)::value;
    if (rm == RM_CONSUMER)
      with_rw(h->rw, [&](auto RW) { enqueue_round_t<r, RW(), RM_CONSUMER>(h, d_active, G); });
    else
      with_rw(h->rw, [&](auto RW) { enqueue_round_t<r, RW(), RM_LAUNCH>(h, d_active, G); });
  });
}

// Acceleration (oracle orc_pgo_accel_pre / _post): gamma' = (1 + sqrt(1 +
// 4 N^2 gamma^2)) / (2 N), alpha = 1 / (gamma' N), N = team size.
double accel_gamma_next(const kmx_pgo* h) {
  const double N = (double)h->n_robots;
  return (1.0 + std::sqrt(1.0 + 4.0 * N * N * h->acc_gamma * h->acc_gamma)) / (2.0 * N);
}
void launch_accel(kmx_pgo* h, double c, int mode) {
  with_r(h->P.r, [&](auto R) {
    hipLaunchKernelGGL(k_accel<R()>, dim3(h->ntiles), dim3(BLOCK), 0, h->stream, h->dv, h->gd.accV.get(),
                       h->gd.accY.get(), c, mode);
  });
}
// Y for the upcoming round (X := Y, owned public rows := Y); once per round.
void enqueue_accel_pre(kmx_pgo* h) {
  if (!h->P.acceleration || h->acc_ready || h->ntiles == 0) return;
  if (!h->acc_started) {
    launch_accel(h, 0.0, 2);  // V = X
    h->acc_started = true;
  }
  const double g = accel_gamma_next(h);
  launch_accel(h, 1.0 / (g * (double)h->n_robots), 0);
  h->acc_ready = true;
}
void enqueue_accel_post(kmx_pgo* h) {
  if (!h->P.acceleration || !h->acc_ready || h->ntiles == 0) return;
  const double g = accel_gamma_next(h);
  const bool restart = h->P.restart_interval > 0 && (h->acc_k + 1) % h->P.restart_interval == 0;
  launch_accel(h, g, restart ? 2 : 1);
  h->acc_gamma = restart ? 0.0 : g;
  h->acc_k = restart ? 0 : h->acc_k + 1;
  h->acc_ready = false;
}
void accel_reset(kmx_pgo* h) {
  h->acc_gamma = 0.0;
  h->acc_k = 0;
  h->acc_ready = h->acc_started = false;
}

void enqueue_apply_weights(kmx_pgo* h) {
  if (h->mloc > 0)
    with_rw(h->rw, [&](auto RW) {
      hipLaunchKernelGGL(k_apply_weights<RW()>, dim3((h->mloc + 255) / 256), dim3(256), 0, h->stream, h->dv, h->mloc);
    });
  enqueue_precond(h, 0);
}

}  // namespace

// ================================================================ ABI =====
extern "C" int kmx_pgo_create(const kmx_pgo_params* params, int device, kmx_pgo** out) {
  KMX_GUARD_BEGIN
  KMX_CHECK(params && out, KMX_EINVAL, "null argument");
  KMX_CHECK(params->d == 3, KMX_EUNSUP, "only d = 3 is supported");
  KMX_CHECK(params->r >= 3 && params->r <= 8, KMX_EUNSUP, "relaxation rank must be in [3, 8]");
  KMX_CHECK(params->rtr_iterations >= 1 && params->tcg_max_iterations >= 1, KMX_EINVAL,
            "rtr_iterations and tcg_max_iterations must be >= 1");
  KMX_CHECK(params->robust_cost == KMX_COST_L2 || params->robust_cost == KMX_COST_GNC_TLS, KMX_EUNSUP,
            "robust cost must be L2 or GNC_TLS");
  KMX_CHECK((params->acceleration == 0 || params->acceleration == 1) && params->restart_interval >= 0, KMX_EINVAL,
            "acceleration is 0 or 1, restart_interval >= 0");
  KMX_CHECK(params->method == KMX_METHOD_RTR || params->method == KMX_METHOD_RGD, KMX_EUNSUP,
            "method must be KMX_METHOD_RTR or KMX_METHOD_RGD");
  // (tcg_form 2, the resident round of ABI 7, was removed in ABI 8: DESIGN.md section 10)
  KMX_CHECK(params->tcg_form == KMX_TCG_FORM_STANDARD || params->tcg_form == KMX_TCG_FORM_ONESYNC, KMX_EINVAL,
            "tcg_form must be KMX_TCG_FORM_STANDARD or KMX_TCG_FORM_ONESYNC");
  KMX_CHECK(params->method != KMX_METHOD_RGD || params->rgd_stepsize > 0.0, KMX_EINVAL, "rgd_stepsize must be > 0");
  KMX_CHECK(params->tile_incidences >= 0, KMX_EINVAL, "tile_incidences must be >= 0 (0: automatic)");
  auto h = std::make_unique<kmx_pgo>();
  if (int rc = h->open(device)) return rc;
  h->P = *params;
  if (const char* v = std::getenv("KMX_RED")) {
    const int m = std::atoi(v);
    h->rm_forced = m == 0 ? RM_LAUNCH : m == 2 ? RM_CONSUMER : -1;  // 1 and 3 (tickets, half) were removed
  }
  if (const char* v = std::getenv("KMX_HESS_DECIDE")) h->decide_forced = std::atoi(v) != 0 ? 1 : 0;
  if (const char* v = std::getenv("KMX_HESS_GATE")) h->hess_gate = std::atoi(v) != 0;
  if (const char* v = std::getenv("KMX_TCG_TAIL")) h->tcg_tail = std::atoi(v) != 0;
  if (const char* v = std::getenv("KMX_TCG_GROUPS")) {
    const int g = std::atoi(v);
    h->groups_req = g >= 4 ? 4 : g >= 2 ? 2 : 1;
  }
  if (const char* v = std::getenv("KMX_GROUP_RED")) h->grm_forced = std::atoi(v) == 2 ? RM_CONSUMER : RM_LAUNCH;
  // the side streams of the robot groups (group 0 runs on the handle's stream)
  for (int g = 1; g < h->groups_req; ++g) {
    if (int rc = h->gstream[g - 1].create()) return rc;
    if (int rc = h->ev_join[g - 1].create()) return rc;
  }
  if (h->groups_req > 1)
    if (int rc = h->ev_fork.create()) return rc;
  *out = h.release();
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_pgo_destroy(kmx_pgo* h) {
  if (!h) return KMX_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (hipStream_t s : h->gstream)
    if (s) (void)hipStreamSynchronize(s);
  delete h;  // ~kmx_pgo aborts the communicator before any buffer or stream goes
  return KMX_OK;
}

extern "C" int kmx_pgo_set_stream(kmx_pgo* h, void* s) {
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  return h->adopt(s, false);
}

extern "C" int kmx_pgo_set_tcg_poll(kmx_pgo* h, int mode) {
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  KMX_CHECK(mode >= -1 && mode <= 1, KMX_EINVAL, "mode is -1 (adaptive), 0 (blind) or 1 (polled)");
  h->poll = mode != 0;
  h->poll_auto = mode == -1;
  h->all.blind_left = 0;
  for (auto& g : h->grp) g.blind_left = 0;
  return KMX_OK;
}

extern "C" int kmx_pgo_get_tcg_groups(kmx_pgo* h, int* groups, int32_t* bounds) {
  KMX_CHECK(h && groups, KMX_EINVAL, "null argument");
  *groups = ready(h) ? groups_in_effect(h) : 1;
  if (bounds) {  // the cut of the current graph, also while it is not in effect
    const int G = ready(h) ? (int)h->grp.size() : 0;
    for (int g = 0; g <= kmx_pgo::MAX_GROUPS; ++g)
      bounds[g] = g < G ? h->grp[g].l0 : G > 0 ? h->grp[G - 1].l1 : 0;
  }
  return KMX_OK;
}

extern "C" int kmx_pgo_get_group_reduction(kmx_pgo* h, int* form) {
  KMX_CHECK(h && form, KMX_EINVAL, "null argument");
  *form = ready(h) && groups_in_effect(h) > 1 ? h->grm : h->rm;
  return KMX_OK;
}

// pgo_plan's two-int struct is uploaded as the device's int2
static_assert(sizeof(kmx::PgoInt2) == sizeof(int2) && offsetof(kmx::PgoInt2, x) == offsetof(int2, x) &&
                  offsetof(kmx::PgoInt2, y) == offsetof(int2, y),
              "PgoInt2 is int2");

namespace {
// One plan vector to its device buffer (an empty list has nothing to copy).
template <typename D, typename S>
hipError_t upload(kmx_pgo* h, D* dst, const std::vector<S>& src) {
  static_assert(sizeof(D) == sizeof(S), "uploaded as bytes");
  if (src.empty()) return hipSuccess;
  return hipMemcpyAsync(dst, src.data(), sizeof(S) * src.size(), hipMemcpyHostToDevice, h->stream);
}
}  // namespace

// The graph is checked and planned on the host (pgo_plan, pgo_host.h) before
// the handle is touched: an error from it leaves the handle as it was. Then
// the old graph is dropped and the plan is uploaded.
extern "C" int kmx_pgo_set_graph(kmx_pgo* h, int n_robots, const int32_t* n_poses, const uint8_t* local,
                                 int64_t m, const int32_t* r1, const int32_t* p1, const int32_t* r2,
                                 const int32_t* p2, const double* R, const double* t, const double* kappa,
                                 const double* tau, const double* weight, const uint8_t* fixed_weight) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  KMX_CHECK(n_robots > 0 && n_poses && local, KMX_EINVAL, "bad robot arrays");
  KMX_CHECK(m >= 0 && m < (1ll << 31) - 1, KMX_EINVAL, "edge count out of range");
  KMX_CHECK(m == 0 || (r1 && p1 && r2 && p2 && R && t && kappa && tau && weight && fixed_weight), KMX_EINVAL,
            "null edge array");
  PgoPlanIn in;
  in.r = h->P.r;
  in.tile_incidences = h->P.tile_incidences;
  in.groups_req = h->groups_req;
  in.rm_forced = h->rm_forced;
  in.decide_forced = h->decide_forced;
  in.grm_forced = h->grm_forced;
  in.onesync = onesync(h);
  PgoPlan plan;
  std::string err;
  if (int rc = pgo_plan(in, n_robots, n_poses, local, m, r1, p1, r2, p2, R, t, kappa, tau, weight, fixed_weight,
                        &plan, &err))
    return kmx::fail(rc, err);
  KMX_HIP(hipSetDevice(h->device));
  KMX_HIP(hipStreamSynchronize(h->stream));
  h->gd = {};  // dropped before the new set is allocated: the peak matters at 1M poses
  drop_xchg(h);  // the exchange slot lists index this graph's public table
  accel_reset(h);
  // the plan's host fields
  const int r = h->P.r, ps = 4 * r;
  const int L = (int)plan.robots.size(), nloc = plan.nloc;
  h->n_robots = n_robots;
  h->npose.assign(n_poses, n_poses + n_robots);
  h->m_global = m;
  h->local_of = std::move(plan.local_of);
  h->robots = std::move(plan.robots);
  h->loff = std::move(plan.loff);
  h->nloc = nloc;
  h->rm = plan.rm;
  h->early_stop = plan.early_stop;
  h->grm = plan.grm;
  h->pub_key = std::move(plan.pub_key);
  h->npub = plan.npub;
  h->first_owned = plan.first_owned;
  h->n_owned = plan.n_owned;
  h->loc_edge_gid = std::move(plan.loc_edge_gid);
  h->mloc = plan.mloc;
  h->m_robot = std::move(plan.m_robot);
  h->rw = plan.rw;
  h->ninc = plan.ninc;
  h->nshared = plan.nshared;
  h->n_gnc = (int)plan.gnc_edge.size();
  h->n_sh_local = (int)plan.sh_edge.size();
  h->n_osh = (int)plan.osh_edge.size();
  h->rt0_h = plan.rt0;
  h->ntiles = (int)plan.tile.size();
  h->grp.assign(plan.grp.size(), kmx_pgo::Group{});
  for (size_t g = 0; g < plan.grp.size(); ++g) {
    const PgoGroupCut& c = plan.grp[g];
    h->grp[g].l0 = c.l0; h->grp[g].l1 = c.l1;
    h->grp[g].t0 = c.t0; h->grp[g].nt = c.nt;
  }
  // the single chain (its polling state outlives the graph, as the handle's poll mode)
  h->all.l0 = 0; h->all.l1 = L;
  h->all.t0 = 0; h->all.nt = h->ntiles;
  // device: the new set is built aside. A failure from here on leaves the
  // handle with no graph (ready() false); the host vectors the uploads read
  // are declared before the set, so a set that goes early goes before them
  // (releasing a device buffer waits for the copies)
  const size_t vec = (size_t)std::max(nloc, 1) * ps, n1 = (size_t)std::max(nloc, 1);
  std::vector<double> relc(L);  // no block update yet: not converged (an empty block is)
  for (int l = 0; l < L; ++l) relc[l] = plan.nrob[l] > 0 ? std::numeric_limits<double>::infinity() : 0.0;
  std::vector<Gnc> g0(2, Gnc{});
  g0[0].mu = g0[1].mu = h->P.gnc_mu_init;
  const std::vector<unsigned char> ones(L, 1);
  PgoDev nd;
  int rc;
  if ((rc = nd.tile.alloc(h->ntiles)) || (rc = nd.rtile0.alloc(L + 1)) || (rc = nd.inc_ptr.alloc(nloc + 1)) ||
      (rc = nd.rec.alloc(plan.rec.size())) || (rc = nd.rec_o.alloc(plan.rec_o.size())) ||
      (rc = nd.ekappa.alloc(plan.ek.size())) || (rc = nd.etau.alloc(plan.et.size())) ||
      (rc = nd.ew.alloc(plan.ew.size())) || (rc = nd.eipos.alloc(plan.eipos.size())) ||
      (rc = nd.vec.alloc(vec * nvec(h))) || (rc = nd.S.alloc(n1 * 6)) || (rc = nd.Pinv.alloc(n1 * SYM4)) ||
      (rc = nd.hD.alloc(n1 * SYM4)) || (rc = nd.hDS.alloc(n1 * SYM4)) ||
      (rc = nd.pub.alloc((size_t)std::max<int64_t>(h->npub, 1) * ps)) ||
      (h->P.acceleration && ((rc = nd.accV.alloc(vec)) || (rc = nd.accY.alloc(vec)))) ||
      (multi_rtr(h) && (rc = nd.X0.alloc(vec))) || (rc = nd.part.alloc((size_t)h->ntiles * NPART)) ||
      (rc = nd.ctl.alloc(L)) || (rc = nd.ctl2.alloc(L)) || (rc = nd.part_h.alloc((size_t)h->ntiles * 2)) ||
      (rc = nd.part_u.alloc((size_t)h->ntiles * 2)) || (rc = nd.cnt.alloc(1)) || (rc = nd.m_robot.alloc(L)) ||
      (rc = nd.n_robot.alloc(L)) || (rc = nd.pub_src.alloc(plan.pub_src.size())) ||
      (rc = nd.own_src.alloc(plan.own_src.size())) || (rc = nd.pose_slot.alloc(plan.pose_slot.size())) ||
      (rc = nd.gnc_edge.alloc(h->n_gnc)) || (rc = nd.gnc_ends.alloc(h->n_gnc)) ||
      (rc = nd.sh_edge.alloc(h->n_sh_local)) || (rc = nd.sh_idx.alloc(h->n_sh_local)) || (rc = nd.active.alloc(L)) ||
      (rc = nd.osh_edge.alloc(h->n_osh)) || (rc = nd.osh_idx.alloc(h->n_osh)) || (rc = nd.relc.alloc(L)) ||
      (rc = nd.gnc.alloc(2)) || (rc = nd.ext.alloc(64)) || (rc = nd.hv_launch.alloc(HV_SLOTS)) ||
      (rc = nd.coefh.alloc((size_t)L * std::max(h->P.tcg_max_iterations, 1))) ||
      (onesync(h) && (rc = nd.part_f.alloc((size_t)h->ntiles * 16))))
    return rc;
  KMX_HIP(upload(h, nd.tile.get(), plan.tile));
  KMX_HIP(upload(h, nd.rtile0.get(), plan.rt0));
  KMX_HIP(upload(h, nd.inc_ptr.get(), plan.inc_ptr));
  KMX_HIP(upload(h, nd.rec.get(), plan.rec));
  KMX_HIP(upload(h, nd.rec_o.get(), plan.rec_o));
  KMX_HIP(upload(h, nd.ekappa.get(), plan.ek));
  KMX_HIP(upload(h, nd.etau.get(), plan.et));
  KMX_HIP(upload(h, nd.ew.get(), plan.ew));
  KMX_HIP(upload(h, nd.eipos.get(), plan.eipos));
  KMX_HIP(hipMemsetAsync(nd.vec.get(), 0, sizeof(double) * vec * nvec(h), h->stream));
  KMX_HIP(hipMemsetAsync(nd.coefh.get(), 0, sizeof(double) * L * std::max(h->P.tcg_max_iterations, 1), h->stream));
  KMX_HIP(hipMemsetAsync(nd.pub.get(), 0, sizeof(double) * std::max<int64_t>(h->npub, 1) * ps, h->stream));
  KMX_HIP(hipMemsetAsync(nd.ctl.get(), 0, sizeof(Ctl) * L, h->stream));
  KMX_HIP(hipMemsetAsync(nd.cnt.get(), 0, sizeof(Counters), h->stream));
  KMX_HIP(hipMemsetAsync(nd.ext.get(), 0, sizeof(double) * 64, h->stream));
  KMX_HIP(hipMemsetAsync(nd.hv_launch.get(), 0, sizeof(int) * HV_SLOTS, h->stream));
  if ((size_t)L > h->hstat.cap()) {  // host-mapped per-robot tCG progress
    h->hstat = {};
    if ((rc = h->hstat.alloc(L))) return rc;
  }
  for (int l = 0; l < L; ++l) h->hstat.get()[l].word = 0;
  h->seq = 0;
  KMX_HIP(upload(h, nd.relc.get(), relc));
  KMX_HIP(upload(h, nd.gnc.get(), g0));
  KMX_HIP(upload(h, nd.m_robot.get(), h->m_robot));
  KMX_HIP(upload(h, nd.n_robot.get(), plan.nrob));
  KMX_HIP(upload(h, nd.pub_src.get(), plan.pub_src));
  KMX_HIP(upload(h, nd.own_src.get(), plan.own_src));
  KMX_HIP(upload(h, nd.pose_slot.get(), plan.pose_slot));
  KMX_HIP(upload(h, nd.gnc_edge.get(), plan.gnc_edge));
  KMX_HIP(upload(h, nd.gnc_ends.get(), plan.gnc_ends));
  KMX_HIP(upload(h, nd.sh_edge.get(), plan.sh_edge));
  KMX_HIP(upload(h, nd.sh_idx.get(), plan.sh_idx));
  KMX_HIP(upload(h, nd.osh_edge.get(), plan.osh_edge));
  KMX_HIP(upload(h, nd.osh_idx.get(), plan.osh_idx));
  KMX_HIP(upload(h, nd.active.get(), ones));
  // host vectors must outlive the async copies
  KMX_HIP(hipStreamSynchronize(h->stream));
  h->gd = std::move(nd);  // the uploads are done: commit
  const PgoDev& gd = h->gd;
  Dev& d = h->dv;
  d = Dev{};
  d.ntiles = h->ntiles; d.L = L; d.nloc = nloc; d.npub = (int)h->npub;
  d.gt0 = 0; d.gnt = h->ntiles;
  d.tile = gd.tile.get(); d.rtile0 = gd.rtile0.get();
  d.inc_ptr = gd.inc_ptr.get(); d.rec = gd.rec.get(); d.rec_o = gd.rec_o.get();
  d.ekappa = gd.ekappa.get(); d.etau = gd.etau.get(); d.ew = gd.ew.get(); d.eipos = gd.eipos.get();
  double* const v = gd.vec.get();
  d.X = v; d.Xt = v + vec; d.g = v + 2 * vec; d.r = v + 3 * vec;
  d.z = v + 4 * vec; d.hd = v + 5 * vec; d.eta = v + 6 * vec; d.dh = v + 7 * vec;
  d.coefh = gd.coefh.get(); d.vec = (long long)vec; d.dhn = dh_count(h);
  d.S = gd.S.get(); d.Pinv = gd.Pinv.get(); d.hD = gd.hD.get(); d.hDS = gd.hDS.get();
  d.pub = gd.pub.get(); d.part = gd.part.get();
  d.ctl = gd.ctl.get(); d.cnt = gd.cnt.get();
  d.ctl2 = gd.ctl2.get(); d.part_h = gd.part_h.get(); d.part_u = gd.part_u.get();
  d.m_robot = gd.m_robot.get(); d.n_robot = gd.n_robot.get(); d.pose_slot = gd.pose_slot.get();
  d.relc = gd.relc.get(); d.gnc = gd.gnc.get(); d.gnc_next = gd.gnc.get() + 1;
  d.gnc_edge = gd.gnc_edge.get(); d.gnc_ends = gd.gnc_ends.get(); d.n_gnc = h->n_gnc;
  d.hv_launch = gd.hv_launch.get();
  if (onesync(h)) {
    const size_t v0 = 7 + (size_t)dh_count(h);
    d.hz = v + v0 * vec; d.w0 = v + (v0 + 1) * vec; d.w1 = v + (v0 + 2) * vec;
    d.part_f = gd.part_f.get();
  }
  h->n_ext = 0;
  sync_params(h);
  enqueue_precond(h, 0);
  KMX_HIP(hipGetLastError());
  KMX_HIP(hipStreamSynchronize(h->stream));
  return KMX_OK;
  KMX_GUARD_END
}

static int check_robot(kmx_pgo* h, int robot) {
  KMX_CHECK(ready(h), KMX_ESTATE, "set_graph first");
  KMX_CHECK(robot >= 0 && robot < h->n_robots && h->local_of[robot] >= 0, KMX_EINVAL, "robot is not local");
  return 0;
}

extern "C" int kmx_pgo_set_iterate(kmx_pgo* h, int robot, const double* X) {
  if (int rc = check_robot(h, robot)) return rc;
  KMX_CHECK(X, KMX_EINVAL, "null X");
  KMX_HIP(hipSetDevice(h->device));
  const int ps = 4 * h->P.r, l = h->local_of[robot];
  KMX_HIP(hipMemcpyAsync(h->gd.vec.get() + (size_t)h->loff[l] * ps, X, sizeof(double) * h->npose[robot] * ps,
                         hipMemcpyHostToDevice, h->stream));
  KMX_HIP(hipStreamSynchronize(h->stream));
  accel_reset(h);  // a new initial iterate restarts the acceleration (V = X at the next round)
  return KMX_OK;
}

extern "C" int kmx_pgo_get_iterate(kmx_pgo* h, int robot, double* X) {
  if (int rc = check_robot(h, robot)) return rc;
  KMX_CHECK(X, KMX_EINVAL, "null X");
  KMX_HIP(hipSetDevice(h->device));
  const int ps = 4 * h->P.r, l = h->local_of[robot];
  KMX_HIP(hipMemcpyAsync(X, h->gd.vec.get() + (size_t)h->loff[l] * ps, sizeof(double) * h->npose[robot] * ps,
                         hipMemcpyDeviceToHost, h->stream));
  KMX_HIP(hipStreamSynchronize(h->stream));
  return KMX_OK;
}

extern "C" int kmx_pgo_public_count(kmx_pgo* h, int64_t* n_public, int64_t* first_owned, int64_t* n_owned) {
  KMX_CHECK(ready(h), KMX_ESTATE, "set_graph first");
  if (n_public) *n_public = h->npub;
  if (first_owned) *first_owned = h->first_owned;
  if (n_owned) *n_owned = h->n_owned;
  return KMX_OK;
}

extern "C" int kmx_pgo_pack_public(kmx_pgo* h, void* dev_out) {
  KMX_CHECK(ready(h), KMX_ESTATE, "set_graph first");
  KMX_CHECK(dev_out || h->n_owned == 0, KMX_EINVAL, "null device buffer");
  KMX_HIP(hipSetDevice(h->device));
  const int ps = 4 * h->P.r;
  const long long tot = h->n_owned * ps;
  if (tot)
    hipLaunchKernelGGL(k_pack, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream, h->gd.vec.get(),
                       (double*)dev_out, h->gd.own_src.get(), 0, (int)h->n_owned, ps);
  KMX_HIP(hipGetLastError());
  return KMX_OK;
}

extern "C" int kmx_pgo_unpack_public(kmx_pgo* h, const void* dev_table) {
  KMX_CHECK(ready(h), KMX_ESTATE, "set_graph first");
  KMX_CHECK(dev_table || h->npub == 0, KMX_EINVAL, "null device buffer");
  KMX_HIP(hipSetDevice(h->device));
  if (h->npub)
    KMX_HIP(hipMemcpyAsync(h->gd.pub.get(), dev_table, sizeof(double) * h->npub * 4 * h->P.r, hipMemcpyDeviceToDevice,
                           h->stream));
  return KMX_OK;
}

extern "C" int kmx_pgo_gather_public_rows(kmx_pgo* h, const int32_t* dev_slots, int64_t n, void* dev_out) {
  return kmx_pgo_exchange_pack(h, dev_slots, n, nullptr, 0, dev_out);
}

extern "C" int kmx_pgo_scatter_public_rows(kmx_pgo* h, const int32_t* dev_slots, int64_t n, const void* dev_rows) {
  return kmx_pgo_exchange_unpack(h, dev_slots, n, nullptr, 0, dev_rows);
}

extern "C" int kmx_pgo_exchange_pack(kmx_pgo* h, const int32_t* dev_slots, int64_t n, const int32_t* dev_seg,
                                     int n_seg, void* dev_out) {
  KMX_CHECK(ready(h), KMX_ESTATE, "set_graph first");
  KMX_CHECK(n >= 0 && n_seg >= 0 && n_seg <= 1024 && (n == 0 || (dev_slots && dev_out)) &&
                (n_seg == 0 || (dev_seg && dev_out)),
            KMX_EINVAL, "bad argument");
  KMX_HIP(hipSetDevice(h->device));
  enqueue_accel_pre(h);  // accelerated rounds exchange Y
  const int ps = 4 * h->P.r;
  const long long tot = (long long)n * ps + n_seg;  // rows, then the status words
  if (tot)
    hipLaunchKernelGGL(k_gather_slots, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream, h->gd.vec.get(),
                       h->gd.pub_src.get(), (const int*)dev_slots, (long long)n, (int)h->npub, (double*)dev_out, ps,
                       (const int*)dev_seg, n_seg, (const double*)h->gd.relc.get(), h->dv.L);
  KMX_HIP(hipGetLastError());
  return KMX_OK;
}

extern "C" int kmx_pgo_exchange_unpack(kmx_pgo* h, const int32_t* dev_slots, int64_t n, const int32_t* dev_seg,
                                       int n_seg, const void* dev_in) {
  KMX_CHECK(ready(h), KMX_ESTATE, "set_graph first");
  KMX_CHECK(n >= 0 && n_seg >= 0 && n_seg <= 1024 && (n == 0 || (dev_slots && dev_in)) &&
                (n_seg == 0 || (dev_seg && dev_in)),
            KMX_EINVAL, "bad argument");
  KMX_HIP(hipSetDevice(h->device));
  const int ps = 4 * h->P.r;
  if (int rc = ensure_ext(h, n_seg)) return rc;
  const long long tot = (long long)n * ps + n_seg;  // rows, then the status words
  if (tot)
    hipLaunchKernelGGL(k_scatter_slots, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream, h->gd.pub.get(),
                       (const int*)dev_slots, (long long)n, (int)h->npub, (const double*)dev_in, ps,
                       (const int*)dev_seg, n_seg, h->gd.ext.get());
  h->n_ext = n_seg;
  sync_params(h);
  KMX_HIP(hipGetLastError());
  return KMX_OK;
}

#define KMX_NCCL(call)                                                                      \
  do {                                                                                      \
    const ncclResult_t r_ = (call);                                                         \
    if (r_ != ncclSuccess) return kmx::fail(KMX_EHIP, std::string(#call) + ": " + ncclGetErrorString(r_)); \
  } while (0)

// A call on a non-blocking communicator may return ncclInProgress: wait for
// it to settle (bounded), then report its final status.
int nccl_settle(kmx_pgo* h, ncclResult_t r, const char* what) {
  const auto t0 = std::chrono::steady_clock::now();
  while (r == ncclInProgress) {
    if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(60))
      return kmx::fail(KMX_EHIP, std::string(what) + ": still in progress after 60 s");
    std::this_thread::yield();
    if (ncclCommGetAsyncError(h->comm, &r) != ncclSuccess) r = ncclSystemError;
  }
  if (r != ncclSuccess) return kmx::fail(KMX_EHIP, std::string(what) + ": " + ncclGetErrorString(r));
  return KMX_OK;
}

// publishPublicPoses -> updateNeighborPoses + publishStatus of one round
// (drawio:2340-2375) over RCCL: the rows every peer needs (+ this handle's
// status word) are gathered, each peer's segment goes by ncclSend / ncclRecv in
// one group on the handle's stream, then the received rows land in the public
// table and the peers' status words in ext. Segment layout as
// kmx_pgo_exchange_pack / _unpack.
int enqueue_exchange(kmx_pgo* h) {
  if (!h->xchg) return KMX_OK;
  const int ps = 4 * h->P.r, W = h->world;
  const long long ts = h->xn_send * ps + W, tr = h->xn_recv * ps + W;
  hipLaunchKernelGGL(k_xgather, dim3((unsigned)((ts + 255) / 256)), dim3(256), 0, h->stream, h->gd.vec.get(),
                     h->gd.pub_src.get(), h->xd.xs_slots.get(), h->xd.xs_rseg.get(), h->xn_send, h->xd.xsbuf.get(),
                     ps, h->xd.xs_seg.get(), W,
                     (const double*)h->gd.relc.get(), h->dv.L);
  KMX_NCCL(ncclGroupStart());
  for (int q = 0; q < W; ++q) {
    if (q == h->rank && !h->xchg_self_p2p) continue;
    KMX_NCCL(ncclSend(h->xd.xsbuf.get() + h->xs_off[q], (size_t)h->xs_cnt[q], ncclDouble, q, h->comm, h->stream));
    KMX_NCCL(ncclRecv(h->xd.xrbuf.get() + h->xr_off[q], (size_t)h->xr_cnt[q], ncclDouble, q, h->comm, h->stream));
  }
  // the communicator is non-blocking (kmx_pgo_comm_init): the group may still
  // be enqueueing when ncclGroupEnd returns
  if (int rc = nccl_settle(h, ncclGroupEnd(), "ncclGroupEnd")) return rc;
  if (!h->xchg_self_p2p)  // this handle's own segment (its status word)
    KMX_HIP(hipMemcpyAsync(h->xd.xrbuf.get() + h->xr_off[h->rank], h->xd.xsbuf.get() + h->xs_off[h->rank],
                           sizeof(double) * h->xs_cnt[h->rank], hipMemcpyDeviceToDevice, h->stream));
  hipLaunchKernelGGL(k_xscatter, dim3((unsigned)((tr + 255) / 256)), dim3(256), 0, h->stream, h->gd.pub.get(),
                     h->xd.xr_slots.get(), h->xd.xr_rseg.get(), h->xn_recv, (const double*)h->xd.xrbuf.get(), ps,
                     h->xd.xr_seg.get(), W, h->gd.ext.get());
  if (h->n_ext != W) {
    h->n_ext = W;
    sync_params(h);
  }
  KMX_HIP(hipGetLastError());
  return KMX_OK;
}

// Which RCCL / HIP runtime libkmx's own calls resolve to in this process
// (torch bundles a librccl.so.1 of the same SONAME: whichever was loaded first
// serves both), their versions and the RCCL headers kmx was built against.
extern "C" int kmx_runtime_info(char* out, int64_t nbytes) {
  KMX_GUARD_BEGIN
  KMX_CHECK(out && nbytes > 0, KMX_EINVAL, "null buffer");
  Dl_info di{}, dh{};
  const char* rp = dladdr(reinterpret_cast<void*>(&ncclSend), &di) && di.dli_fname ? di.dli_fname : "?";
  const char* hp = dladdr(reinterpret_cast<void*>(static_cast<hipError_t (*)(void**, size_t)>(&hipMalloc)), &dh) && dh.dli_fname ? dh.dli_fname : "?";
  int rv = 0, hv = 0, dv = 0;
  (void)ncclGetVersion(&rv);
  (void)hipRuntimeGetVersion(&hv);
  (void)hipDriverGetVersion(&dv);
  const std::string js = std::string("{\"rccl_path\": \"") + rp + "\", \"rccl_version\": " + std::to_string(rv) +
                         ", \"rccl_header_version\": " + std::to_string(NCCL_VERSION_CODE) + ", \"hip_path\": \"" + hp +
                         "\", \"hip_runtime_version\": " + std::to_string(hv) + ", \"hip_driver_version\": " +
                         std::to_string(dv) + "}";
  KMX_CHECK((int64_t)js.size() < nbytes, KMX_EINVAL, "buffer too small");
  std::memcpy(out, js.c_str(), js.size() + 1);
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_comm_unique_id(void* out, int64_t nbytes) {
  KMX_GUARD_BEGIN
  KMX_CHECK(out && nbytes >= (int64_t)sizeof(ncclUniqueId), KMX_EINVAL, "need a buffer of KMX_COMM_ID_BYTES");
  ncclUniqueId id;
  KMX_NCCL(ncclGetUniqueId(&id));
  std::memcpy(out, &id, sizeof(id));
  return KMX_OK;
  KMX_GUARD_END
}

// Non-blocking communicator creation with a deadline: a rank whose peers never
// arrive (one of them failed before ncclCommInitRank) aborts its half-built
// communicator and returns an error instead of blocking in the rendezvous.
extern "C" int kmx_pgo_comm_init(kmx_pgo* h, const void* unique_id, int world, int rank, double timeout_s) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h && unique_id, KMX_EINVAL, "null argument");
  KMX_CHECK(world >= 1 && world <= 1024 && rank >= 0 && rank < world, KMX_EINVAL, "bad world / rank");
  KMX_CHECK(timeout_s > 0.0, KMX_EINVAL, "timeout_s must be > 0");
  KMX_CHECK(!h->comm, KMX_ESTATE, "communicator already initialised");
  KMX_HIP(hipSetDevice(h->device));
  ncclUniqueId id;
  std::memcpy(&id, unique_id, sizeof(id));
  ncclComm_t c = nullptr;
  ncclConfig_t cfg = NCCL_CONFIG_INITIALIZER;
  cfg.blocking = 0;
  ncclResult_t r = ncclCommInitRankConfig(&c, world, id, rank, &cfg);
  const auto t0 = std::chrono::steady_clock::now();
  while (r == ncclInProgress) {
    if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s) {
      if (c) (void)ncclCommAbort(c);
      return kmx::fail(KMX_EHIP, "ncclCommInitRankConfig: no rendezvous within the timeout (a peer failed?)");
    }
    std::this_thread::sleep_for(std::chrono::microseconds(100));
    if (ncclCommGetAsyncError(c, &r) != ncclSuccess) r = ncclSystemError;
  }
  if (r != ncclSuccess) {
    if (c) (void)ncclCommAbort(c);
    return kmx::fail(KMX_EHIP, std::string("ncclCommInitRankConfig: ") + ncclGetErrorString(r));
  }
  h->comm = c;
  h->world = world;
  h->rank = rank;
  if (const char* v = std::getenv("KMX_XCHG_SELF_P2P")) h->xchg_self_p2p = std::atoi(v) != 0;
  return KMX_OK;
  KMX_GUARD_END
}

// Abort first: a round whose exchange waits on a peer that never posts its
// half (the peer failed) only leaves the stream once the communicator is
// aborted; then the stream drains and the exchange buffers can go.
extern "C" int kmx_pgo_comm_destroy(kmx_pgo* h) {
  KMX_GUARD_BEGIN
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  KMX_HIP(hipSetDevice(h->device));
  if (h->comm) (void)ncclCommAbort(h->comm);
  h->comm = nullptr;
  KMX_HIP(hipStreamSynchronize(h->stream));
  drop_xchg(h);
  h->world = 1;
  h->rank = 0;
  if (h->n_ext) {  // the peers' statuses came with the exchange
    h->n_ext = 0;
    sync_params(h);
  }
  return KMX_OK;
  KMX_GUARD_END
}

// The handle's stream drained within timeout_s (polled), or KMX_ETIMEOUT: a
// bounded wait for a round whose exchange depends on peers.
extern "C" int kmx_pgo_sync_timeout(kmx_pgo* h, double timeout_s) {
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  KMX_CHECK(timeout_s > 0.0, KMX_EINVAL, "timeout_s must be > 0");
  KMX_HIP(hipSetDevice(h->device));
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    hipError_t e = hipStreamQuery(h->stream);
    if (e == hipSuccess) return KMX_OK;
    if (e != hipErrorNotReady) return kmx::fail(KMX_EHIP, std::string("hipStreamQuery: ") + hipGetErrorString(e));
    if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s)
      return kmx::fail(KMX_ETIMEOUT, "the stream did not drain within the timeout (an exchange peer is missing?)");
    std::this_thread::sleep_for(std::chrono::microseconds(50));
  }
}

extern "C" int kmx_pgo_get_public(kmx_pgo* h, double* table, double* ext) {
  KMX_GUARD_BEGIN
  KMX_CHECK(ready(h), KMX_ESTATE, "set_graph first");
  KMX_CHECK(table || h->npub == 0, KMX_EINVAL, "null table");
  KMX_HIP(hipSetDevice(h->device));
  if (h->npub)
    KMX_HIP(hipMemcpyAsync(table, h->gd.pub.get(), sizeof(double) * h->npub * 4 * h->P.r, hipMemcpyDeviceToHost,
                           h->stream));
  if (ext && h->n_ext)
    KMX_HIP(hipMemcpyAsync(ext, h->gd.ext.get(), sizeof(double) * h->n_ext, hipMemcpyDeviceToHost, h->stream));
  KMX_HIP(hipStreamSynchronize(h->stream));
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_pgo_set_exchange(kmx_pgo* h, const int32_t* send_slots, const int64_t* send_counts,
                                    const int32_t* recv_slots, const int64_t* recv_counts) {
  KMX_GUARD_BEGIN
  KMX_CHECK(ready(h), KMX_ESTATE, "set_graph first");
  KMX_CHECK(h->comm, KMX_ESTATE, "kmx_pgo_comm_init first");
  KMX_CHECK(send_counts && recv_counts, KMX_EINVAL, "null counts");
  const int W = h->world, ps = 4 * h->P.r;
  long long ns = 0, nr = 0;
  for (int q = 0; q < W; ++q) {
    KMX_CHECK(send_counts[q] >= 0 && recv_counts[q] >= 0, KMX_EINVAL, "negative count");
    ns += send_counts[q];
    nr += recv_counts[q];
  }
  KMX_CHECK(send_counts[h->rank] == recv_counts[h->rank], KMX_EINVAL, "own segment: send and receive counts differ");
  KMX_CHECK((ns == 0 || send_slots) && (nr == 0 || recv_slots), KMX_EINVAL, "null slot list");
  for (long long i = 0; i < ns; ++i) KMX_CHECK(send_slots[i] >= 0 && send_slots[i] < h->npub, KMX_EINVAL, "send slot out of range");
  for (long long i = 0; i < nr; ++i) KMX_CHECK(recv_slots[i] >= 0 && recv_slots[i] < h->npub, KMX_EINVAL, "recv slot out of range");
  KMX_HIP(hipSetDevice(h->device));
  KMX_HIP(hipStreamSynchronize(h->stream));
  drop_xchg(h);  // a failure from here on leaves the handle without an exchange
  std::vector<int> sseg(W + 1, 0), rseg(W + 1, 0);
  h->xs_cnt.assign(W, 0); h->xr_cnt.assign(W, 0); h->xs_off.assign(W, 0); h->xr_off.assign(W, 0);
  for (int q = 0; q < W; ++q) {
    sseg[q + 1] = sseg[q] + (int)send_counts[q];
    rseg[q + 1] = rseg[q] + (int)recv_counts[q];
    h->xs_cnt[q] = send_counts[q] * ps + 1;
    h->xr_cnt[q] = recv_counts[q] * ps + 1;
    h->xs_off[q] = (long long)sseg[q] * ps + q;
    h->xr_off[q] = (long long)rseg[q] * ps + q;
  }
  PgoXchg nx;  // built aside, committed once its copies are done
  int rc = 0;
  if ((rc = nx.xs_slots.alloc(ns)) || (rc = nx.xr_slots.alloc(nr)) || (rc = nx.xs_seg.alloc(W + 1)) ||
      (rc = nx.xs_rseg.alloc(ns)) || (rc = nx.xr_rseg.alloc(nr)) || (rc = nx.xr_seg.alloc(W + 1)) ||
      (rc = nx.xsbuf.alloc(ns * ps + W)) || (rc = nx.xrbuf.alloc(nr * ps + W)))
    return rc;
  if ((rc = ensure_ext(h, W))) return rc;
  if (ns) KMX_HIP(hipMemcpy(nx.xs_slots.get(), send_slots, sizeof(int) * ns, hipMemcpyHostToDevice));
  if (nr) KMX_HIP(hipMemcpy(nx.xr_slots.get(), recv_slots, sizeof(int) * nr, hipMemcpyHostToDevice));
  {
    std::vector<int> srs(std::max<long long>(ns, 1)), rrs(std::max<long long>(nr, 1));
    for (int q = 0; q < W; ++q) {
      for (int k = sseg[q]; k < sseg[q + 1]; ++k) srs[k] = q;
      for (int k = rseg[q]; k < rseg[q + 1]; ++k) rrs[k] = q;
    }
    if (ns) KMX_HIP(hipMemcpy(nx.xs_rseg.get(), srs.data(), sizeof(int) * ns, hipMemcpyHostToDevice));
    if (nr) KMX_HIP(hipMemcpy(nx.xr_rseg.get(), rrs.data(), sizeof(int) * nr, hipMemcpyHostToDevice));
  }
  KMX_HIP(hipMemcpy(nx.xs_seg.get(), sseg.data(), sizeof(int) * (W + 1), hipMemcpyHostToDevice));
  KMX_HIP(hipMemcpy(nx.xr_seg.get(), rseg.data(), sizeof(int) * (W + 1), hipMemcpyHostToDevice));
  h->xd = std::move(nx);
  h->xn_send = ns;
  h->xn_recv = nr;
  h->xchg = true;
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_pgo_exchange(kmx_pgo* h) {
  KMX_GUARD_BEGIN
  KMX_CHECK(ready(h), KMX_ESTATE, "set_graph first");
  KMX_CHECK(h->xchg, KMX_ESTATE, "kmx_pgo_set_exchange first");
  KMX_HIP(hipSetDevice(h->device));
  enqueue_accel_pre(h);
  return enqueue_exchange(h);
  KMX_GUARD_END
}

extern "C" int kmx_pgo_refresh_local(kmx_pgo* h) {
  KMX_CHECK(ready(h), KMX_ESTATE, "set_graph first");
  KMX_HIP(hipSetDevice(h->device));
  enqueue_accel_pre(h);  // accelerated rounds publish Y
  enqueue_publish(h);
  KMX_HIP(hipGetLastError());
  return KMX_OK;
}

extern "C" int kmx_pgo_set_neighbor_poses(kmx_pgo* h, int64_t count, const int32_t* robot, const int32_t* pose,
                                          const double* X) {
  KMX_GUARD_BEGIN
  KMX_CHECK(ready(h), KMX_ESTATE, "set_graph first");
  KMX_CHECK(count == 0 || (robot && pose && X), KMX_EINVAL, "null argument");
  KMX_HIP(hipSetDevice(h->device));
  const int ps = 4 * h->P.r;
  std::vector<double> tab((size_t)std::max<int64_t>(h->npub, 1) * ps);
  KMX_HIP(hipMemcpyAsync(tab.data(), h->gd.pub.get(), sizeof(double) * h->npub * ps, hipMemcpyDeviceToHost, h->stream));
  KMX_HIP(hipStreamSynchronize(h->stream));
  for (int64_t i = 0; i < count; ++i) {
    const int64_t k = ((int64_t)robot[i] << 32) | (uint32_t)pose[i];
    auto it = std::lower_bound(h->pub_key.begin(), h->pub_key.end(), k);
    KMX_CHECK(it != h->pub_key.end() && *it == k, KMX_EINVAL, "pose is not public (no shared edge)");
    std::memcpy(&tab[(size_t)(it - h->pub_key.begin()) * ps], X + (size_t)i * ps, sizeof(double) * ps);
  }
  KMX_HIP(hipMemcpyAsync(h->gd.pub.get(), tab.data(), sizeof(double) * h->npub * ps, hipMemcpyHostToDevice, h->stream));
  KMX_HIP(hipStreamSynchronize(h->stream));
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_pgo_iterate(kmx_pgo* h, const uint8_t* active, kmx_iter_stats* stats) {
  KMX_GUARD_BEGIN
  KMX_CHECK(ready(h), KMX_ESTATE, "set_graph first");
  KMX_CHECK(active, KMX_EINVAL, "null active mask");
  KMX_HIP(hipSetDevice(h->device));
  const int L = (int)h->robots.size();
  std::vector<unsigned char> act(L);
  for (int l = 0; l < L; ++l) act[l] = active[h->robots[l]] ? 1 : 0;
  if (h->P.acceleration)
    for (int l = 0; l < L; ++l)
      KMX_CHECK(act[l], KMX_EUNSUP, "acceleration needs every local robot active (concurrent schedule)");
  KMX_HIP(hipMemcpyAsync(h->gd.active.get(), act.data(), L, hipMemcpyHostToDevice, h->stream));
  enqueue_accel_pre(h);
  if (int rc = enqueue_exchange(h)) return rc;
  enqueue_round(h, h->gd.active.get());
  enqueue_accel_post(h);
  KMX_HIP(hipGetLastError());
  std::vector<Ctl> ctl(L);
  KMX_HIP(hipMemcpyAsync(ctl.data(), h->gd.ctl.get(), sizeof(Ctl) * L, hipMemcpyDeviceToHost, h->stream));
  KMX_HIP(hipStreamSynchronize(h->stream));
  // restore the all-active mask used by iterate_async
  std::vector<unsigned char> ones(L, 1);
  KMX_HIP(hipMemcpyAsync(h->gd.active.get(), ones.data(), L, hipMemcpyHostToDevice, h->stream));
  KMX_HIP(hipStreamSynchronize(h->stream));
  if (stats) {
    for (int a = 0; a < h->n_robots; ++a) std::memset(&stats[a], 0, sizeof(kmx_iter_stats));
    for (int l = 0; l < L; ++l) {
      const Ctl& c = ctl[l];
      kmx_iter_stats& s = stats[h->robots[l]];
      s.updated = c.updated;
      s.tcg_iterations = c.tcg_iter;
      s.tcg_stop = c.tcg_stop;
      s.accepted = c.accepted;
      s.f_init = c.f_init;
      s.gradnorm_init = c.gn_init;
      s.f_final = c.f_final;
      s.rho = c.rho;
      s.radius = c.Delta;
      s.rel_change = c.rel_change;
      s.edges = h->m_robot[l];
      s.hessvecs = c.hessvecs;
    }
  }
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_pgo_iterate_async(kmx_pgo* h, int rounds, int refresh_local) {
  KMX_CHECK(ready(h), KMX_ESTATE, "set_graph first");
  KMX_CHECK(rounds >= 0, KMX_EINVAL, "negative rounds");
  KMX_HIP(hipSetDevice(h->device));
  // every round's k_commit republishes the committed owned rows, so the
  // single-device exchange needs one publish per call
  if (refresh_local && rounds > 0) enqueue_publish(h);
  for (int i = 0; i < rounds; ++i) {
    enqueue_accel_pre(h);  // publishes Y itself
    if (int rc = enqueue_exchange(h)) return rc;
    enqueue_round(h, h->gd.active.get());
    enqueue_accel_post(h);
  }
  KMX_HIP(hipGetLastError());
  return KMX_OK;
}

extern "C" int kmx_pgo_sync(kmx_pgo* h) {
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  KMX_HIP(hipSetDevice(h->device));
  KMX_HIP(hipStreamSynchronize(h->stream));
  return KMX_OK;
}

extern "C" int kmx_pgo_set_gnc_schedule(kmx_pgo* h, int enabled, int inner_iters, int max_updates,
                                        double rel_change_tol) {
  KMX_CHECK(ready(h), KMX_ESTATE, "set_graph first");
  KMX_CHECK(inner_iters >= 0 && max_updates >= 0, KMX_EINVAL, "negative schedule parameter");
  h->gnc_on = enabled ? 1 : 0;
  h->gnc_inner_iters = inner_iters;
  h->gnc_max_updates = max_updates;
  h->gnc_rel_tol = rel_change_tol;
  sync_params(h);
  return KMX_OK;
}

extern "C" int kmx_pgo_get_gnc_state(kmx_pgo* h, kmx_gnc_state* out) {
  KMX_CHECK(ready(h) && out, KMX_EINVAL, "null argument / no graph");
  KMX_HIP(hipSetDevice(h->device));
  Gnc g;
  KMX_HIP(hipMemcpyAsync(&g, h->gd.gnc.get(), sizeof(Gnc), hipMemcpyDeviceToHost, h->stream));
  KMX_HIP(hipStreamSynchronize(h->stream));
  std::memset(out, 0, sizeof(*out));
  out->inner_iter = g.inner;
  out->updates = g.updates;
  out->last_fired = g.fired;
  out->rounds = g.rounds;
  out->mu = g.mu;
  return KMX_OK;
}

extern "C" int kmx_pgo_set_gnc_state(kmx_pgo* h, const kmx_gnc_state* in) {
  KMX_CHECK(ready(h) && in && in->mu > 0.0, KMX_EINVAL, "null argument / no graph / mu <= 0");
  KMX_HIP(hipSetDevice(h->device));
  Gnc g[2] = {};
  g[0].inner = in->inner_iter;
  g[0].updates = in->updates;
  g[0].fired = in->last_fired;
  g[0].rounds = in->rounds;
  g[0].mu = in->mu;
  g[1] = g[0];
  KMX_HIP(hipMemcpyAsync(h->gd.gnc.get(), g, sizeof(g), hipMemcpyHostToDevice, h->stream));
  KMX_HIP(hipStreamSynchronize(h->stream));
  return KMX_OK;
}

extern "C" int kmx_pgo_get_status(kmx_pgo* h, double* rel_change) {
  KMX_GUARD_BEGIN
  KMX_CHECK(ready(h) && rel_change, KMX_EINVAL, "null argument / no graph");
  KMX_HIP(hipSetDevice(h->device));
  std::vector<double> v(h->robots.size());
  KMX_HIP(hipMemcpyAsync(v.data(), h->gd.relc.get(), sizeof(double) * v.size(), hipMemcpyDeviceToHost, h->stream));
  KMX_HIP(hipStreamSynchronize(h->stream));
  for (size_t l = 0; l < v.size(); ++l) rel_change[h->robots[l]] = v[l];
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_pgo_set_status(kmx_pgo* h, const double* rel_change) {
  KMX_GUARD_BEGIN
  KMX_CHECK(ready(h) && rel_change, KMX_EINVAL, "null argument / no graph");
  KMX_HIP(hipSetDevice(h->device));
  std::vector<double> v(h->robots.size());
  for (size_t l = 0; l < v.size(); ++l) v[l] = rel_change[h->robots[l]];
  KMX_HIP(hipMemcpyAsync(h->gd.relc.get(), v.data(), sizeof(double) * v.size(), hipMemcpyHostToDevice, h->stream));
  KMX_HIP(hipStreamSynchronize(h->stream));
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_pgo_update_weights(kmx_pgo* h, double* mu_out) {
  KMX_CHECK(ready(h), KMX_ESTATE, "set_graph first");
  KMX_HIP(hipSetDevice(h->device));
  Gnc g;
  KMX_HIP(hipMemcpyAsync(&g, h->gd.gnc.get(), sizeof(Gnc), hipMemcpyDeviceToHost, h->stream));
  KMX_HIP(hipStreamSynchronize(h->stream));
  if (mu_out) *mu_out = g.mu;
  if (h->P.robust_cost != KMX_COST_GNC_TLS) return KMX_OK;
  enqueue_begin(h, h->gd.active.get(), BEGIN_FORCE_GNC);
  KMX_HIP(hipGetLastError());
  KMX_HIP(hipStreamSynchronize(h->stream));
  return KMX_OK;
}

extern "C" int kmx_pgo_get_mu(kmx_pgo* h, double* mu) {
  KMX_CHECK(ready(h) && mu, KMX_EINVAL, "null argument / no graph");
  kmx_gnc_state s;
  if (int rc = kmx_pgo_get_gnc_state(h, &s)) return rc;
  *mu = s.mu;
  return KMX_OK;
}
extern "C" int kmx_pgo_set_mu(kmx_pgo* h, double mu) {
  KMX_CHECK(ready(h) && mu > 0.0, KMX_EINVAL, "mu must be positive / no graph");
  kmx_gnc_state s;
  if (int rc = kmx_pgo_get_gnc_state(h, &s)) return rc;
  s.mu = mu;
  return kmx_pgo_set_gnc_state(h, &s);
}

extern "C" int kmx_pgo_get_weights(kmx_pgo* h, double* w) {
  KMX_GUARD_BEGIN
  KMX_CHECK(ready(h) && w, KMX_EINVAL, "null argument / no graph");
  KMX_HIP(hipSetDevice(h->device));
  std::vector<double> ew(std::max(h->mloc, 1));
  KMX_HIP(hipMemcpyAsync(ew.data(), h->gd.ew.get(), sizeof(double) * h->mloc, hipMemcpyDeviceToHost, h->stream));
  KMX_HIP(hipStreamSynchronize(h->stream));
  for (int k = 0; k < h->mloc; ++k) w[h->loc_edge_gid[k]] = ew[k];
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_pgo_set_weights(kmx_pgo* h, const double* w) {
  KMX_GUARD_BEGIN
  KMX_CHECK(ready(h) && w, KMX_EINVAL, "null argument / no graph");
  KMX_HIP(hipSetDevice(h->device));
  std::vector<double> ew(std::max(h->mloc, 1));
  for (int k = 0; k < h->mloc; ++k) ew[k] = w[h->loc_edge_gid[k]];
  KMX_HIP(hipMemcpyAsync(h->gd.ew.get(), ew.data(), sizeof(double) * h->mloc, hipMemcpyHostToDevice, h->stream));
  enqueue_apply_weights(h);
  KMX_HIP(hipGetLastError());
  KMX_HIP(hipStreamSynchronize(h->stream));
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_pgo_shared_count(kmx_pgo* h, int64_t* n_shared) {
  KMX_CHECK(ready(h) && n_shared, KMX_EINVAL, "null argument / no graph");
  *n_shared = h->nshared;
  return KMX_OK;
}

extern "C" int kmx_pgo_pack_shared_weights(kmx_pgo* h, void* dev_out) {
  KMX_CHECK(ready(h), KMX_ESTATE, "set_graph first");
  KMX_CHECK(dev_out || h->nshared == 0, KMX_EINVAL, "null device buffer");
  KMX_HIP(hipSetDevice(h->device));
  if (h->nshared == 0) return KMX_OK;
  KMX_HIP(hipMemsetAsync(dev_out, 0, sizeof(double) * h->nshared, h->stream));
  if (h->n_osh)
    hipLaunchKernelGGL(k_shared_pack, dim3((h->n_osh + 255) / 256), dim3(256), 0, h->stream,
                       (const double*)h->gd.ew.get(), h->gd.osh_edge.get(), h->gd.osh_idx.get(), h->n_osh,
                       (double*)dev_out);
  KMX_HIP(hipGetLastError());
  return KMX_OK;
}

extern "C" int kmx_pgo_unpack_shared_weights(kmx_pgo* h, const void* dev_table) {
  KMX_CHECK(ready(h), KMX_ESTATE, "set_graph first");
  KMX_CHECK(dev_table || h->nshared == 0, KMX_EINVAL, "null device buffer");
  KMX_HIP(hipSetDevice(h->device));
  if (h->n_sh_local)
    hipLaunchKernelGGL(k_shared_unpack, dim3((h->n_sh_local + 255) / 256), dim3(256), 0, h->stream, h->gd.ew.get(),
                       h->gd.sh_edge.get(), h->gd.sh_idx.get(), h->n_sh_local, (const double*)dev_table);
  enqueue_apply_weights(h);
  KMX_HIP(hipGetLastError());
  return KMX_OK;
}

extern "C" int kmx_pgo_get_trajectory(kmx_pgo* h, int robot, const double* anchor, double* out) {
  KMX_GUARD_BEGIN
  if (int rc = check_robot(h, robot)) return rc;
  KMX_CHECK(anchor && out, KMX_EINVAL, "null argument");
  KMX_HIP(hipSetDevice(h->device));
  const int ps = 4 * h->P.r, l = h->local_of[robot], n = h->npose[robot];
  if (int rc = ensure_scratch(h, (size_t)ps + (size_t)std::max(n, 1) * 12)) return rc;
  double* d_anchor = h->gd.scratch.get();
  double* d_out = h->gd.scratch.get() + ps;
  KMX_HIP(hipMemcpyAsync(d_anchor, anchor, sizeof(double) * ps, hipMemcpyHostToDevice, h->stream));
  if (n)
    hipLaunchKernelGGL(k_traj, dim3((n + 127) / 128), dim3(128), 0, h->stream,
                       (const double*)(h->gd.vec.get() + (size_t)h->loff[l] * ps), n, h->P.r,
                       (const double*)d_anchor, d_out);
  KMX_HIP(hipGetLastError());
  KMX_HIP(hipMemcpyAsync(out, d_out, sizeof(double) * n * 12, hipMemcpyDeviceToHost, h->stream));
  KMX_HIP(hipStreamSynchronize(h->stream));
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_pgo_eval(kmx_pgo* h, int robot, int mode, const double* V, double* out, double* scalar) {
  KMX_GUARD_BEGIN
  if (int rc = check_robot(h, robot)) return rc;
  KMX_CHECK(mode >= KMX_EVAL_COST_EGRAD && mode <= KMX_EVAL_PROJECT, KMX_EINVAL, "bad eval mode");
  KMX_CHECK(out && (V || mode == KMX_EVAL_RGRAD), KMX_EINVAL, "null argument");
  KMX_HIP(hipSetDevice(h->device));
  const int ps = 4 * h->P.r, l = h->local_of[robot], n = h->npose[robot];
  const size_t vec = (size_t)std::max(h->nloc, 1) * ps;
  if (int rc = ensure_scratch(h, vec * 2)) return rc;
  double* dV = h->gd.scratch.get();
  double* dO = h->gd.scratch.get() + vec;
  const size_t o = (size_t)h->loff[l] * ps;
  KMX_HIP(hipMemsetAsync(h->gd.scratch.get(), 0, sizeof(double) * vec * 2, h->stream));
  if (V) KMX_HIP(hipMemcpyAsync(dV + o, V, sizeof(double) * n * ps, hipMemcpyHostToDevice, h->stream));
  with_r(h->P.r, [&](auto R) {
    with_rw(h->rw, [&](auto RW) {
      constexpr int r = decltype(R)::value, rw = decltype(RW)::value;
      hipLaunchKernelGGL((k_eval<r, rw>), dim3(h->ntiles), dim3(BLOCK), SmemE<r>::bytes, h->stream, h->dv, l, mode,
                         (const double*)dV, dO);
    });
  });
  KMX_HIP(hipGetLastError());
  KMX_HIP(hipMemcpyAsync(out, dO + o, sizeof(double) * n * ps, hipMemcpyDeviceToHost, h->stream));
  std::vector<double> part((size_t)h->ntiles * NPART);
  KMX_HIP(hipMemcpyAsync(part.data(), h->gd.part.get(), sizeof(double) * part.size(), hipMemcpyDeviceToHost,
                         h->stream));
  KMX_HIP(hipStreamSynchronize(h->stream));
  // tiles of robot l are contiguous
  const int t0 = h->rt0_h[l], nt = h->rt0_h[l + 1] - h->rt0_h[l];
  double s = 0.0;
  for (int tt = t0; tt < t0 + nt; ++tt) s += part[(size_t)tt * NPART];
  if (scalar) *scalar = s;
  return KMX_OK;
  KMX_GUARD_END
}

extern "C" int kmx_pgo_local_edges(kmx_pgo* h, int robot, int64_t* m_local) {
  if (int rc = check_robot(h, robot)) return rc;
  KMX_CHECK(m_local, KMX_EINVAL, "null argument");
  *m_local = h->m_robot[h->local_of[robot]];
  return KMX_OK;
}

extern "C" int kmx_pgo_memory(kmx_pgo* h, int64_t* device_bytes, int* record_bytes) {
  KMX_CHECK(ready(h), KMX_ESTATE, "set_graph first");
  const int64_t L = (int64_t)h->robots.size(), n = std::max(h->nloc, 1), ps = 4 * h->P.r;
  int64_t b = 0;
  const int rb = h->rw == 10 ? 8 * 8 + 4 : 128;  // bytes per incidence record (compact: 64 + the 4-B other endpoint)
  b += (int64_t)(h->ninc + 1) * rb + (int64_t)(h->nloc + 1) * 4;         // records, CSR
  b += (int64_t)std::max(h->mloc, 1) * (3 * 8 + 8);                      // kappa, tau, w, positions
  b += n * ps * 8 * (int64_t)nvec(h) + n * (6 + 3 * SYM4) * 8;         // vectors, S, Pinv, D, D - S
  b += L * 8 * (int64_t)std::max(h->P.tcg_max_iterations, 1);            // tCG coefficients
  b += std::max<int64_t>(h->npub, 1) * (ps * 8 + 4) + n * 4;             // public table + maps
  b += (int64_t)h->ntiles * (NPART * 8 + 12 + (onesync(h) ? 64 : 0)) + L * (int64_t)(sizeof(Ctl) + 32);
  b += (int64_t)std::max(h->n_gnc, 1) * 12 + (int64_t)h->gd.scratch.cap() * 8;  // GNC lists, scratch in use
  if (h->P.acceleration) b += 2 * n * ps * 8;                              // V, Y
  if (device_bytes) *device_bytes = b;
  if (record_bytes) *record_bytes = rb;
  return KMX_OK;
}

extern "C" int kmx_pgo_enable_timing(kmx_pgo* h, int enable) {
  KMX_CHECK(h, KMX_EINVAL, "null handle");
  h->timing = enable != 0;
  return KMX_OK;
}

extern "C" int kmx_pgo_read_counters(kmx_pgo* h, kmx_pgo_counters* out) {
  KMX_CHECK(ready(h) && out, KMX_EINVAL, "null argument / no graph");
  KMX_HIP(hipSetDevice(h->device));
  KMX_HIP(hipStreamSynchronize(h->stream));
  Counters c;
  KMX_HIP(hipMemcpy(&c, h->gd.cnt.get(), sizeof(Counters), hipMemcpyDeviceToHost));
  // event pairs of k_hess launches in which at least one robot ran a Hess-vec
  const size_t nl = std::min(h->ev_used / 2, (size_t)HV_SLOTS);
  std::vector<int> hv(std::max<size_t>(nl, 1), 0);
  if (nl) KMX_HIP(hipMemcpy(hv.data(), h->gd.hv_launch.get(), sizeof(int) * nl, hipMemcpyDeviceToHost));
  double ms_total = 0.0;
  int64_t launches = 0;
  for (size_t i = 0; i < nl; ++i) {
    if (hv[i] == 0) continue;
    float ms = 0.f;
    KMX_HIP(hipEventElapsedTime(&ms, h->ev_pool[2 * i], h->ev_pool[2 * i + 1]));
    ms_total += ms;
    ++launches;
  }
  if (nl) KMX_HIP(hipMemset(h->gd.hv_launch.get(), 0, sizeof(int) * nl));
  std::memset(out, 0, sizeof(*out));
  out->hessvec_ms_total = ms_total;
  out->hessvec_launches = launches;
  out->hessvec_alg_bytes = c.hess_alg_bytes;
  out->edges_iters = (int64_t)c.edges_iters;
  out->block_updates = (int64_t)c.block_updates;
  out->hessvecs = (int64_t)c.hessvecs;
  out->gnc_updates = (int64_t)c.gnc_updates;
  h->ev_used = 0;
  KMX_HIP(hipMemset(h->gd.cnt.get(), 0, sizeof(Counters)));
  return KMX_OK;
}

// Diagnostic: the k_step phase stamps of a KMX_STEP_STAMPS build (16 words per
// tile: 7 wall-clock stamps, -, poses, incidences, block index, writer);
// KMX_EUNSUP in the product build.
extern "C" int kmx_pgo_debug_step_stamps(uint64_t* out, int64_t n) {
  KMX_GUARD_BEGIN
#ifdef KMX_STEP_STAMPS
  KMX_CHECK(out && n >= 0, KMX_EINVAL, "null buffer");
  const int64_t m = std::min<int64_t>(n, 16 * (int64_t)STEP_STAMP_TILES);
  KMX_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_step_stamp), sizeof(uint64_t) * m, 0, hipMemcpyDeviceToHost));
  return KMX_OK;
#else
  (void)out;
  (void)n;
  return kmx::fail(KMX_EUNSUP, "not a KMX_STEP_STAMPS build");
#endif
  KMX_GUARD_END
}
